// Training-mode BatchNorm of the cell head's instance classifier (ldiff_resnet_forward_train; include/ldiff.h ldiff_op_bn_*).  The eval-mode forward folds every
// BatchNorm into its conv at load; with batch statistics that is impossible, so conv -> BN -> (+ identity) -> ReLU is three launches:
//   clsconv<..., bn>   kernels_cls.hip: the raw fp16 sums + per row block and channel {sum, sum of squares} of the fp32 accumulators (ConvParams::bn_stats)
//   bn_finalize        per channel: the R partials in index order in DOUBLE -> scale / shift (fp32) and the batch mean / unbiased variance
//   bn_apply           y = fp16(relu?(x scale + shift + id)), id = nothing | a plain tensor | a second raw tensor with its own scale / shift (the downsample branch)
// No atomics anywhere: every figure is bit-reproducible from run to run.
#include "common.h"

namespace {

constexpr double BN_EPS = 1e-5;   // torch.nn.BatchNorm2d's default

// A thread per channel.  The R partials of a channel are contiguous (part[(c R + r) 2]); they are added strictly in index order, so the loop is one dependent chain of double
// additions per figure; the loads are independent of it and unrolled ahead.  mean^2 is subtracted in double: sumsq / n - mean^2 cancels to about 2^-53 of sumsq / n, and what is
// left negative by it is clamped (a constant channel gives exactly 0).
__global__ __launch_bounds__(64) void bn_finalize_kernel(const float* __restrict__ part, int R, int N, double n, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ mean_out, float* __restrict__ var_out) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= N) return;
  const float2* p = reinterpret_cast<const float2*>(part) + (long long)c * R;
  double s = 0.0, q = 0.0;
  int r = 0;
  for (; r + 8 <= R; r += 8) {
    float2 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[r + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) { s += (double)v[i].x; q += (double)v[i].y; }
  }
  for (; r < R; ++r) { const float2 v = p[r]; s += (double)v.x; q += (double)v.y; }
  const double mean = s / n;
  double var = q / n - mean * mean;
  var = var > 0.0 ? var : 0.0;   // (a NaN stays out of here: NaN > 0 is false.  It is reported by the conv's own non-finite flag)
  if (s != s || q != q) var = s + q;
  const double sc = (double)gamma[c] / sqrt(var + BN_EPS);
  scale[c] = (float)sc;
  shift[c] = (float)((double)beta[c] - mean * sc);
  mean_out[c] = (float)mean;
  var_out[c] = (float)(var * n / (n - 1.0));
}

// A thread = 8 channels of one row: 16-byte loads and stores, the fp32 scale / shift (two float4 each) read once per thread.
// MODE 0: no identity, 1: a plain fp16 identity, 2: a raw identity with its own scale / shift.
template <int MODE>
__global__ __launch_bounds__(256) void bn_apply_kernel(const f16* __restrict__ x, long long total, int N8, const float* __restrict__ scale, const float* __restrict__ shift,
                                                       const f16* __restrict__ id, const float* __restrict__ id_scale, const float* __restrict__ id_shift, int relu,
                                                       f16* __restrict__ y, int* __restrict__ nonfinite) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c0 = (int)(i % N8) * 8;
  const f16x8 xv = *reinterpret_cast<const f16x8*>(x + i * 8);
  float sc[8], sh[8];
  *reinterpret_cast<float4*>(sc) = *reinterpret_cast<const float4*>(scale + c0);
  *reinterpret_cast<float4*>(sc + 4) = *reinterpret_cast<const float4*>(scale + c0 + 4);
  *reinterpret_cast<float4*>(sh) = *reinterpret_cast<const float4*>(shift + c0);
  *reinterpret_cast<float4*>(sh + 4) = *reinterpret_cast<const float4*>(shift + c0 + 4);
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = __builtin_fmaf((float)xv[k], sc[k], sh[k]);
  if constexpr (MODE >= 1) {
    const f16x8 rv = *reinterpret_cast<const f16x8*>(id + i * 8);
    if constexpr (MODE == 2) {
      float s2[8], t2[8];
      *reinterpret_cast<float4*>(s2) = *reinterpret_cast<const float4*>(id_scale + c0);
      *reinterpret_cast<float4*>(s2 + 4) = *reinterpret_cast<const float4*>(id_scale + c0 + 4);
      *reinterpret_cast<float4*>(t2) = *reinterpret_cast<const float4*>(id_shift + c0);
      *reinterpret_cast<float4*>(t2 + 4) = *reinterpret_cast<const float4*>(id_shift + c0 + 4);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += __builtin_fmaf((float)rv[k], s2[k], t2[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += (float)rv[k];
    }
  }
  bool bad = false;
  f16x8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (!(__builtin_fabsf(v[k]) <= 65504.f)) bad = true;   // in front of the ReLU, as clsconv's epilogue (a NaN fails the comparison)
    if (relu) v[k] = v[k] > 0.f ? v[k] : 0.f;
    o[k] = (f16)v[k];
  }
  *reinterpret_cast<f16x8*>(y + i * 8) = o;
  if (bad && nonfinite) *nonfinite = 1;
}

}  // namespace

void launch_bn_finalize(const float* part, int R, int N, long long n, const float* gamma, const float* beta, float* scale, float* shift, float* batch_stats, long long offset, long long T,
                        hipStream_t s) {
  // torch: "Expected more than 1 value per channel when training"
  LDIFF_CHECK(n >= 2, LDIFF_ERR_INVALID, "bn_finalize: expected more than 1 value per channel when training, got n = %lld (the unbiased variance divides by n - 1)", n);
  LDIFF_CHECK(part && gamma && beta && scale && shift && batch_stats && R >= 1 && N >= 1 && offset >= 0 && offset + N <= T && ((uintptr_t)part & 7) == 0, LDIFF_ERR_INVALID,
              "bn_finalize: null or misaligned pointer, empty shape, or channels [%lld, %lld) outside the %lld of the statistics buffer", offset, offset + N, T);
  ProfScope prof("bn_finalize", 4.0 * R * (double)N, 8.0 * R * (double)N, s);
  bn_finalize_kernel<<<(unsigned)((N + 63) / 64), 64, 0, s>>>(part, R, N, (double)n, gamma, beta, scale, shift, batch_stats + offset, batch_stats + T + offset);
  HIP_CHECK(hipGetLastError());
}

void launch_bn_apply(const f16* x, long long M, int N, const float* scale, const float* shift, const f16* id, const float* id_scale, const float* id_shift, int relu, f16* y, int* nonfinite,
                     hipStream_t s) {
  LDIFF_CHECK(x && y && scale && shift && M >= 1 && N >= 8 && N % 8 == 0 && (id || (!id_scale && !id_shift)) && (!id_scale == !id_shift), LDIFF_ERR_INVALID,
              "bn_apply: null pointer, empty shape, N = %d not a multiple of 8, or an identity scale / shift without its tensor or its partner", N);
  LDIFF_CHECK((((uintptr_t)x | (uintptr_t)y | (uintptr_t)id | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)id_scale | (uintptr_t)id_shift) & 15) == 0, LDIFF_ERR_INVALID,
              "bn_apply: every pointer must be 16-byte aligned");
  const long long total = M * (N / 8);
  LDIFF_CHECK((total + 255) / 256 < (1ll << 31), LDIFF_ERR_INVALID, "bn_apply: M * N = %lld * %d is too large for one launch", M, N);
  const unsigned grid = (unsigned)((total + 255) / 256);
  const int mode = !id ? 0 : id_scale ? 2 : 1;
  static const char* names[3] = {"bn_apply", "bn_apply<id>", "bn_apply<id,bn>"};
  ProfScope prof(names[mode], (mode == 2 ? 5.0 : 3.0) * M * (double)N, (mode ? 6.0 : 4.0) * M * (double)N, s);
  if (mode == 0) bn_apply_kernel<0><<<grid, 256, 0, s>>>(x, total, N / 8, scale, shift, nullptr, nullptr, nullptr, relu, y, nonfinite);
  else if (mode == 1) bn_apply_kernel<1><<<grid, 256, 0, s>>>(x, total, N / 8, scale, shift, id, nullptr, nullptr, relu, y, nonfinite);
  else bn_apply_kernel<2><<<grid, 256, 0, s>>>(x, total, N / 8, scale, shift, id, id_scale, id_shift, relu, y, nonfinite);
  HIP_CHECK(hipGetLastError());
}
