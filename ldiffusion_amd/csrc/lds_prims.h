// Device primitives of the LDS-tiled kernels (the conv3x3 family, the GEMMs): one definition each.  A kernel file whose variant differs keeps its own
// under its own name (lds_wait2 / lds_wait4 of the dataflow kernels, sfor of kernels_gemm_ast.hip).
#pragma once
#include "common.h"

typedef __attribute__((address_space(1))) const void gptr_t;
typedef __attribute__((address_space(3))) void lptr_t;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// LDS rows are 128 B: 16-byte chunk `chunk` of row `row` lives at position chunk ^ ((row >> 1) & 7) (conflict-free ds_read_b128 of the 16x16x32 operand fetch)
__device__ __forceinline__ int swz8(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}
// operand reads as inline asm + counted lgkmcnt waits (hipcc only ever emits lgkmcnt(0) there)
template <int OFF>
__device__ __forceinline__ void lds_read128(f16x8& d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}
// s_waitcnt lgkmcnt(CNT); the fragments it covers are in/out operands so no MFMA consuming them can move above it
template <int CNT>
__device__ __forceinline__ void lds_wait(f16x8& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(CNT)); }
template <int CNT>
__device__ __forceinline__ void lds_wait(f16x8& a, f16x8& b, f16x8& c) { asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(a), "+v"(b), "+v"(c) : "n"(CNT)); }
template <int CNT>
__device__ __forceinline__ void lds_wait(f16x8& a, f16x8& b, f16x8& c, f16x8& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(CNT));
}
template <int CNT>
__device__ __forceinline__ void lds_wait(f16x8& a, f16x8& b, f16x8& c, f16x8& d, f16x8& e) {
  asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : "n"(CNT));
}
