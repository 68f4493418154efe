// Device primitives shared by the kernel files: one definition each, under one name.  The rule: a primitive with a twin in another file lives here; one used
// by a single file stays in that file.
#pragma once
#include "common.h"

typedef __attribute__((address_space(1))) const void gptr_t;
typedef __attribute__((address_space(3))) void lptr_t;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// LDS rows are 128 B: 16-byte chunk `chunk` of row `row` lives at position chunk ^ ((row >> 1) & 7) (conflict-free ds_read_b128 of the 16x16x32 operand fetch)
__device__ __forceinline__ int swz8(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
// Column swizzle of the halo image (the halo-tile conv3x3 kernels): 16-byte chunk c of halo pixel (hy, hx) sits at position c ^ swzx(hx) of its 128-B row.
// A 16x16x32 operand fetch reads 16 consecutive pixels of one halo row starting at column kx = 0, 1 or 2; its four
// ds_read_b128 lane groups mix chunks c (8 lanes) and c^1 (8 lanes).  The table (one 3-bit entry per column PAIR, found by
// exhaustive search against the bank model of MI355X_MICROARCH.md, LDS) makes all three starts conflict-free; the plain
// (hx>>1)&7 is conflict-free only for kx = 0 and costs 2x on the other two thirds of the taps (SQ_LDS_BANK_CONFLICT = 26 %
// of the LDS-active cycles).  The position is an XOR of the chunk index, so k-half 1 is still byte address ^ 64.
__device__ __forceinline__ int swzx(int hx) { return (0xcb5888 >> (3 * (hx >> 1))) & 7; }

__device__ __forceinline__ float silu_f(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f)); }
// (a __builtin_bit_cast applied directly to a vector ELEMENT expression reads element 0 whatever the index: hipcc 7.2; by value it is fine)
__device__ __forceinline__ float u2f(unsigned v) { return __builtin_bit_cast(float, v); }

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

// ---- LDS traffic as inline asm, waited for with counted lgkmcnt ----
// Why not plain loads and stores: hipcc orders every LDS access it knows of behind ALL pending vector-memory operations when an LDS-DMA may be among them
// (it cannot prove they do not alias the DMA's destination: s_waitcnt vmcnt(0), after an epilogue's stores a full write round trip), and it only ever
// emits lgkmcnt(0) in front of the consumer: "ds_read; s_waitcnt lgkmcnt(0); v_mfma" per fragment, every round trip exposed.  So the accesses are issued
// in batches here and the wait names the fragments it covers as in/out operands: no MFMA consuming them can move above it.  Every register exactly once:
// a register named twice is COPIED in front of the statement, i.e. read while its load is still in flight.  T: any register type of the access's size.
template <int OFF, class T>
__device__ __forceinline__ void lds_read128(T& d, unsigned addr) {
  static_assert(sizeof(T) == 16, "ds_read_b128");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}
// the transposing read of a 16-bit matrix: four keys of one head-dim column per lane (the V^T fragments of the attention kernels)
template <int OFF>
__device__ __forceinline__ void lds_read_tr(f16x4& d, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}
__device__ __forceinline__ void lds_read32(float& d, unsigned addr) { asm volatile("ds_read_b32 %0, %1" : "=v"(d) : "v"(addr) : "memory"); }
template <class T>
__device__ __forceinline__ void lds_write32(unsigned addr, T v) {
  static_assert(sizeof(T) == 4, "ds_write_b32");
  asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
template <class T>
__device__ __forceinline__ void lds_write64(unsigned addr, T v) {
  static_assert(sizeof(T) == 8, "ds_write_b64");
  asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
template <int OFF, class T>
__device__ __forceinline__ void lds_write64(unsigned addr, const T& v) {
  static_assert(sizeof(T) == 8, "ds_write_b64");
  asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(addr), "v"(v), "n"(OFF) : "memory");
}
template <class T>
__device__ __forceinline__ void lds_write128(unsigned addr, const T& v) {
  static_assert(sizeof(T) == 16, "ds_write_b128");
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
// s_waitcnt lgkmcnt(CNT) on one to five fragments (no memory clobber: only the named registers are held back)
template <int CNT, class T>
__device__ __forceinline__ void lds_wait(T& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(CNT)); }
template <int CNT, class T>
__device__ __forceinline__ void lds_wait(T& a, T& b) { asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(CNT)); }
template <int CNT, class T>
__device__ __forceinline__ void lds_wait(T& a, T& b, T& c) { asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(a), "+v"(b), "+v"(c) : "n"(CNT)); }
template <int CNT, class T>
__device__ __forceinline__ void lds_wait(T& a, T& b, T& c, T& d) { asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(CNT)); }
template <int CNT, class T>
__device__ __forceinline__ void lds_wait(T& a, T& b, T& c, T& d, T& e) {
  asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : "n"(CNT));
}
// read four progress words and wait for them: their minimum, wave-uniform (the dataflow kernels' polls)
__device__ __forceinline__ unsigned flags_min_now(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
  const unsigned m = min(min(v[0], v[1]), min(v[2], v[3]));
  return (unsigned)__builtin_amdgcn_readfirstlane((int)m);
}
