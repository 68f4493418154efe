// The epilogue of the row-group accumulator layout, ONE definition for igemm and the split-K reduce.
//
// Layout: acc[NT][MT] of f32x4 per lane; the lane holds row l15 of m-tile m and columns ncol + 16 a + 0..3 (ncol = first column of the wave + 4 (lane >> 4)).
// row_of(mt) is the kernel's own arithmetic: the output row of this lane in m-tile mt, or -1 where the tile hangs over the edge.
// Every step: (sum + addends) * 2^-out_shift, + residual hi (+ lo), one rounding, hi (| lo) stored, the statistics operand -- what the consumer will read: the
// fp16 value, or v itself for a split output, NaN where its hi half overflowed -- left in acc.  The addends (bias, time embedding) are the caller's: which
// there are, per column or per row, and the order they are summed in differ by kernel and are not reassociated here.
//
// conv3x3_kernel<8,8>, conv3x3w_kernel (kernels_conv3x3.hip) and gemm_dma_kernel (kernels_gemm.hip) finish on the same layout and keep their own text of
// these steps, with a 16-byte store form on top: written on this header the conv kernels' GroupNorm instantiations came out with other SGPR spill counts and
// gemm_dma<128,64> measured 0.6-0.8 % slower (profiles/epilogue_refactor_resources.txt).  A change to a rule stated here has to be made there too.
#pragma once
#include "common.h"

// a per-column fp32 vector (bias, one image's time embedding; nullptr = zeros) at the lane's NT column groups
template <int NT>
__device__ __forceinline__ void epi_load_cols(const float* src, int ncol, int N, f32x4 (&out)[NT]) {
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src && ncol + a * 16 < N) t = *reinterpret_cast<const float4*>(src + ncol + a * 16);
    out[a] = (f32x4){t.x, t.y, t.z, t.w};
  }
}

// split-K (ConvParams::splitk > 1): the raw fp32 partial sums of K range `ksplit`; splitk_reduce sums them and applies the epilogue
template <int MT, int NT, class RowOf>
__device__ __forceinline__ void epi_store_partial(const ConvParams& p, const f32x4 (&acc)[NT][MT], RowOf row_of, int ksplit, int ncol) {
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const auto row = row_of(m);
    if (row < 0) continue;
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const int n = ncol + a * 16;
      if (n < p.N) *reinterpret_cast<f32x4*>(p.splitk_ws + ((long long)ksplit * p.M + row) * p.N + n) = acc[a][m];
    }
  }
}

// residual hi (and lo, of a split residual) of the whole wave tile, issued back to back before any use: a load -> wait -> store chain per 16x16 tile costs
// one memory round trip per tile
template <int MT, int NT, class RowOf>
__device__ __forceinline__ void epi_load_residual(const ConvParams& p, RowOf row_of, int ncol, f16x4 (&rr)[MT][NT], f16x4 (&rl)[MT][NT]) {
  if (!p.res) return;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const auto row = row_of(m);
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      rr[m][a] = (f16x4){(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
      rl[m][a] = rr[m][a];
      if (row >= 0 && ncol + a * 16 < p.N) {
        rr[m][a] = *reinterpret_cast<const f16x4*>(p.res + (long long)row * p.ld_res + ncol + a * 16);
        if (p.res_lo) rl[m][a] = *reinterpret_cast<const f16x4*>(p.res + (long long)row * p.ld_res + p.res_lo + ncol + a * 16);
      }
    }
  }
}

// the value rule; sum = accumulator + the caller's addends, osc = shift_scale(p.out_shift): the range shift comes before the (pre-shifted) residual
__device__ __forceinline__ f32x4 epi_value(const ConvParams& p, f32x4 v, float osc, const f16x4& res_hi, const f16x4& res_lo) {
  v *= osc;
  if (p.res) { v += up4(res_hi); if (p.res_lo) v += up4(res_lo); }
  return v;
}

// 8-byte form: four columns of one row as fp32, fp16, or fp16 hi | lo; with want_stat the statistics operand goes to `stat`
__device__ __forceinline__ void epi_store8(const ConvParams& p, long long row, int n, const f32x4& v, bool want_stat, f32x4& stat) {
  if (p.out_f32) { *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.y) + row * p.ldy + n) = v; return; }
  const f16x4 o = cvt4(v);
  *reinterpret_cast<f16x4*>(reinterpret_cast<f16*>(p.y) + row * p.ldy + n) = o;
  if (p.y_lo) *reinterpret_cast<f16x4*>(reinterpret_cast<f16*>(p.y) + row * p.ldy + p.y_lo + n) = cvt4(v - up4(o));
  if (want_stat) stat = p.y_lo ? split_stat4(v) : up4(o);
}
// ... of m-tile m (row >= 0); sum(a, m) = acc[a][m] + the addends
template <int MT, int NT, class Sum>
__device__ __forceinline__ void epi_store8_row(const ConvParams& p, f32x4 (&acc)[NT][MT], int m, long long row, Sum sum, float osc, const f16x4 (&rr)[MT][NT],
                                               const f16x4 (&rl)[MT][NT], int ncol) {
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    const int n = ncol + a * 16;
    if (n >= p.N) continue;
    epi_store8(p, row, n, epi_value(p, sum(a, m), osc, rr[m][a], rl[m][a]), p.stats != nullptr, acc[a][m]);
  }
}
// fused GroupNorm statistics of the GEMMs (common.h): one partial per 32 consecutive rows; blk0 = the global 32-row block of the wave's first row
template <int MT, int NT, class RowOf>
__device__ __forceinline__ void epi_stats_blocks32(const ConvParams& p, const f32x4 (&acc)[NT][MT], RowOf row_of, long long blk0, int ncol, int l15) {
  bool ok[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) ok[m] = row_of(m) >= 0;
#pragma unroll
  for (int sb = 0; sb < MT / 2; ++sb) {
    const long long blk = blk0 + sb, R = p.stats_R;   // global 32-row block -> (image, block in image)
    if (blk * 32 < p.M) wave_stats_store<MT, NT>(acc, ok, 2 * sb, 2 * sb + 2, p.stats + ((blk / R) * p.N * R + blk % R) * 2, R, p.N, ncol, l15);
  }
}
