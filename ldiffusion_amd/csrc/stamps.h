// In-kernel cycle stamps of the diagnostic builds (-DLDIFF_STAMPS; never the product library: the macros are empty without it).
//   scripts/build_variant.sh <name> --only <kernel file>.hip -DLDIFF_STAMPS
// A kernel that stamps keeps a local `unsigned long long dbg[]`, copies it to its own __device__ array at the end and exports that array through its own
// ldiff_debug_*_stamps(); the slot meanings are the kernel's (see the reader script named at each array).
#pragma once

#ifdef LDIFF_STAMPS
// s_memtime with the LDS queue drained, fenced against the scheduler on both sides
__device__ __forceinline__ unsigned long long stamp_now() {
  __builtin_amdgcn_sched_barrier(0);
  unsigned long long t = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define STAMP(v) const unsigned long long v = stamp_now()
#define STAMP_ACC(i, expr) dbg[i] += (expr)
#else
#define STAMP(v)
#define STAMP_ACC(i, expr)
#endif
