// Training form of the nnU-Net tissue head (gfx950, MI355X): what a step of nnUNetTrainer.train_step needs beside the conv forward / dgrad / wgrad the
// fine-tuning step already has (kernels_bwd.hip):
//   in_train_fwd / in_train_bwd   InstanceNorm2d(eps, affine) + LeakyReLU(slope) with saved statistics, and its backward
//   dice_ce                       DC_and_CE_loss with MemoryEfficientSoftDiceLoss of ONE deep-supervision scale: value and d loss / d logits
//   dice_ce_stats / _from_sums    the same loss split at its sums, so that data-parallel ranks can add their statistics between the two halves
//   sgd_nesterov_multi            torch.optim.SGD(momentum, nesterov=True, weight_decay) over many tensors in one launch
//   bucket_pack / sumsq           every gradient into one flat buffer in one launch (the all-reduce's operand), and that buffer's L2 norm
// All are bandwidth-bound passes over NHWC fp16 tensors or fp32 gradients.  Every cross-workgroup sum goes through per-workgroup partials in a caller-supplied
// workspace and a small finalize that adds them in a fixed order (double): no floating-point atomics, so a replay on the same inputs is bit-identical.
#include "common.h"

#include <type_traits>

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- InstanceNorm + LeakyReLU ---------------------------------------------------------------------------------------------------------------------
// Thread layout of the three streaming kernels: a row of x is C8 = C / 8 vectors of 8 channels.  G = min(C8, 256) threads cover a row (a thread keeps its
// vector column for the whole slab, so its 8 per-channel constants / accumulators live in registers), nrl = 256 / G such groups take alternate rows, and
// a workgroup owns a slab of nrl * IN_ROWS consecutive rows of one image: at most IN_ROWS terms per fp32 accumulator.
constexpr int IN_ROWS = 32;
struct InLayout { int C8, G, nrl, S, R; };
inline InLayout in_layout(int HW, int C) {
  InLayout l;
  l.C8 = C / 8;
  l.G = l.C8 < 256 ? l.C8 : 256;
  l.nrl = 256 / l.G;
  l.S = l.nrl * IN_ROWS;
  l.R = (HW + l.S - 1) / l.S;
  return l;
}

// the pre-activation, formed the same way by the forward and the backward so that both take the same side of the kink
__device__ __forceinline__ float in_pre(float x, float mu, float r, float g, float b, float& xh) {
  xh = (x - mu) * r;
  return fmaf(xh, g, b);
}

// BWD = false: per-channel {sum x, sum x^2} of a slab;  BWD = true: {sum da, sum da * xhat}, da = dy * lrelu'(a)
// part[((b * R + slab) * C + c) * 2 + {0, 1}]
template <bool BWD>
__global__ __launch_bounds__(256) void in_partial_kernel(const f16* __restrict__ x, const f16* __restrict__ dy, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         float* __restrict__ part, int HW, int C, int G, int nrl, float slope) {
  __shared__ float red[16][256];   // [accumulator][thread]: consecutive threads, consecutive banks
  const int b = blockIdx.y, slab = blockIdx.x, R = gridDim.x, tid = threadIdx.x, C8 = C / 8;
  const int g = tid % G, rl = tid / G;
  const int r0 = slab * nrl * IN_ROWS, r1 = min(HW, r0 + nrl * IN_ROWS);
  for (int cv0 = 0; cv0 < C8; cv0 += G) {
    const int cv = cv0 + g;
    const bool live = cv < C8 && rl < nrl;
    float s0[8], s1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s0[j] = s1[j] = 0.f;
    if (live) {
      float mu[8], rs[8], gm[8], bt[8];
      if (BWD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = cv * 8 + j;
          mu[j] = mean[(long long)b * C + c]; rs[j] = rstd[(long long)b * C + c]; gm[j] = gamma[c]; bt[j] = beta[c];
        }
      }
      for (int row = r0 + rl; row < r1; row += nrl) {
        const long long at = ((long long)b * HW + row) * C + cv * 8;
        const f16x8 xv = *reinterpret_cast<const f16x8*>(x + at);
        if (BWD) {
          const f16x8 dv = *reinterpret_cast<const f16x8*>(dy + at);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float xh;
            const float a = in_pre((float)xv[j], mu[j], rs[j], gm[j], bt[j], xh);
            const float da = (float)dv[j] * (a > 0.f ? 1.0f : slope);
            s0[j] += da;
            s1[j] += da * xh;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) { const float v = (float)xv[j]; s0[j] += v; s1[j] += v * v; }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[j][tid] = s0[j]; red[8 + j][tid] = s1[j]; }
    __syncthreads();
    if (live && rl == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        double a = 0.0, q = 0.0;
        for (int k = 0; k < nrl; ++k) { a += (double)red[j][k * G + g]; q += (double)red[8 + j][k * G + g]; }
        float* dst = part + (((long long)b * R + slab) * C + cv * 8 + j) * 2;
        dst[0] = (float)a; dst[1] = (float)q;
      }
    }
  }
}

// one wave per (image, channel): mean / rstd from the slabs' partial sums, added in double in a fixed order.  The variance is E[x^2] - mean^2 of sums whose
// fp32 partials carry gamma(IN_ROWS + 3) of E[x^2]: rstd is off by up to 1.5 gamma(35) E[x^2] / (var + eps) relative: 6e-6 (1 + (mean / sd)^2), i.e. about
// 1e-5 behind a conv with a small bias, where |mean| stays below the standard deviation.  A channel whose mean is many standard deviations from zero wants
// sums about a shift (or a (mean, M2) merge per slab); nnU-Net's blocks do not produce one, and the tests' bound carries the term.
__global__ __launch_bounds__(256) void in_fwd_finalize_kernel(const float* __restrict__ part, int R, int HW, int C, float eps, float* __restrict__ mean,
                                                              float* __restrict__ rstd) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  double a = 0.0, q = 0.0;
  for (int r = lane; r < R; r += 64) {
    const float* p = part + (((long long)b * R + r) * C + c) * 2;
    a += (double)p[0]; q += (double)p[1];
  }
  a = wave_sum_d(a); q = wave_sum_d(q);
  if (lane == 0) {
    const double mu = a / (double)HW;
    double var = q / (double)HW - mu * mu;
    if (var < 0.0) var = 0.0;
    mean[(long long)b * C + c] = (float)mu;
    rstd[(long long)b * C + c] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// one wave per channel, the images in order: m[b][c] = {mean da, mean da * xhat} of the image (what dx needs), dgamma[c] = sum_b sum da * xhat, dbeta[c] = sum_b sum da
__global__ __launch_bounds__(256) void in_bwd_finalize_kernel(const float* __restrict__ part, int R, int B, int HW, int C, float* __restrict__ m,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  double dg = 0.0, db = 0.0;
  for (int b = 0; b < B; ++b) {
    double a = 0.0, q = 0.0;
    for (int r = lane; r < R; r += 64) {
      const float* p = part + (((long long)b * R + r) * C + c) * 2;
      a += (double)p[0]; q += (double)p[1];
    }
    a = wave_sum_d(a); q = wave_sum_d(q);
    if (lane == 0) {
      m[((long long)b * C + c) * 2] = (float)(a / (double)HW);
      m[((long long)b * C + c) * 2 + 1] = (float)(q / (double)HW);
    }
    db += a; dg += q;
  }
  if (lane == 0) { dgamma[c] = (float)dg; dbeta[c] = (float)db; }
}

// BWD = false: y = lrelu(xhat gamma + beta);  BWD = true: dx = rstd gamma (da - mean da - xhat mean(da xhat))
template <bool BWD>
__global__ __launch_bounds__(256) void in_apply_kernel(const f16* __restrict__ x, const f16* __restrict__ dy, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ m, f16* __restrict__ out, int HW, int C, int G, int nrl, float slope) {
  const int b = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x, C8 = C / 8;
  const int g = tid % G, rl = tid / G;
  if (rl >= nrl) return;
  const int r0 = slab * nrl * IN_ROWS, r1 = min(HW, r0 + nrl * IN_ROWS);
  for (int cv = g; cv < C8; cv += G) {
    float mu[8], rs[8], gm[8], bt[8], m1[8], m2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cv * 8 + j;
      mu[j] = mean[(long long)b * C + c]; rs[j] = rstd[(long long)b * C + c]; gm[j] = gamma[c]; bt[j] = beta[c];
      if (BWD) { m1[j] = m[((long long)b * C + c) * 2]; m2[j] = m[((long long)b * C + c) * 2 + 1]; }
    }
    for (int row = r0 + rl; row < r1; row += nrl) {
      const long long at = ((long long)b * HW + row) * C + cv * 8;
      const f16x8 xv = *reinterpret_cast<const f16x8*>(x + at);
      f16x8 o;
      if (BWD) {
        const f16x8 dv = *reinterpret_cast<const f16x8*>(dy + at);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xh;
          const float a = in_pre((float)xv[j], mu[j], rs[j], gm[j], bt[j], xh);
          const float da = (float)dv[j] * (a > 0.f ? 1.0f : slope);
          o[j] = (f16)(rs[j] * gm[j] * (da - m1[j] - xh * m2[j]));
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xh;
          const float a = in_pre((float)xv[j], mu[j], rs[j], gm[j], bt[j], xh);
          o[j] = (f16)(a > 0.f ? a : a * slope);
        }
      }
      *reinterpret_cast<f16x8*>(out + at) = o;
    }
  }
}

// ---- Dice + cross-entropy of one deep-supervision scale --------------------------------------------------------------------------------------------
// A thread takes a pixel: its ld = 8 NV logits in NV 16-byte loads, softmax over the n real columns in fp32.  A workgroup owns DCE_PIX consecutive pixels
// of one image and writes NACC = 3 * 8 NV + 2 + IGN partial sums: sum_pred[c], intersect[c], sum_gt[c], the cross-entropy sum, the count of labels outside
// [0, n) and, in the ignore form, the count of annotated pixels.
//
// IGN is DC_and_CE_loss(ignore_label = k) in the same kernels.  A pixel whose label is `ignore` takes no part: no accumulator sees it, its logits are never
// loaded (the label is read first), its dlogits row is +0.  The cross-entropy is the sum over annotated pixels over their count -- this process's own -- and
// 0 when there is none, and the finalize leaves 1 / count (0 for count 0) as a device scalar for the gradient kernel, where the plain form passes
// 1 / (B HW) by value.  The count of a batch without an ignored pixel is the integer B HW, so that batch gives the plain form's bits.  IGN = false compiles
// none of this: its kernels have neither the compare nor the arguments.
constexpr int DCE_PIX = 4096;
inline int dce_nacc(int NV, bool ign) { return 3 * 8 * NV + 2 + ign; }

// What the ignore form adds to the streaming kernels' arguments, and what the plain form has in their place: chosen so that no other argument of a
// plain kernel moves (DceNone is one byte of the padding behind `n`; a DceCount<false> is the float it holds).
struct DceNone {};
template <bool IGN> using DceIgnore = std::conditional_t<IGN, int, DceNone>;   // the partial kernel: the label to skip / nothing
template <bool IGN> struct DceCount;                                           // the gradient kernel:
template <> struct DceCount<false> { float inv; };                             //   1 / (B HW), formed on the host
template <> struct DceCount<true> { const float* inv; int ignore; };           //   the finalize's 1 / count, and the label to skip

template <int NV>
__device__ __forceinline__ void dce_softmax(const f16* __restrict__ row, int n, float (&v)[8 * NV], float (&p)[8 * NV], float& log_sum, float& mx) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const f16x8 t = *reinterpret_cast<const f16x8*>(row + 8 * k);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[8 * k + j] = (float)t[j];
  }
  mx = v[0];
#pragma unroll
  for (int k = 1; k < 8 * NV; ++k) if (k < n) mx = fmaxf(mx, v[k]);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8 * NV; ++k) { p[k] = k < n ? expf(v[k] - mx) : 0.f; s += p[k]; }
  const float inv = 1.0f / s;
#pragma unroll
  for (int k = 0; k < 8 * NV; ++k) p[k] *= inv;
  log_sum = logf(s);
}

__device__ __forceinline__ int dce_label(const void* __restrict__ target, int i64, long long at) {
  if (i64) {
    const long long t = reinterpret_cast<const long long*>(target)[at];
    return (t < 0 || t > 255) ? 255 : (int)t;
  }
  return (int)reinterpret_cast<const unsigned char*>(target)[at];
}

template <int NV, bool IGN>
__global__ __launch_bounds__(256) void dce_partial_kernel(const f16* __restrict__ logits, const void* __restrict__ target, int i64, long long HW, int n,
                                                          DceIgnore<IGN> ignore, float* __restrict__ part) {
  constexpr int NC = 8 * NV, NACC = 3 * NC + 2 + IGN;
  __shared__ float red[4][NACC];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * DCE_PIX, p1 = p0 + DCE_PIX < HW ? p0 + DCE_PIX : HW;
  float sp[NC], si[NC], sg[NC], ce = 0.f, bad = 0.f;
  [[maybe_unused]] float ann = 0.f;   // IGN: the annotated pixels
#pragma unroll
  for (int k = 0; k < NC; ++k) sp[k] = si[k] = sg[k] = 0.f;
  for (long long px = p0 + tid; px < p1; px += 256) {
    const long long at = (long long)b * HW + px;
    int t;
    if constexpr (IGN) {   // the label first: an ignored pixel's logits are never loaded.  The plain form keeps its order, the logits' loads ahead
      t = dce_label(target, i64, at);
      if (t == ignore) continue;
    }
    float v[NC], p[NC], lse, mx;
    dce_softmax<NV>(logits + at * NC, n, v, p, lse, mx);
    if constexpr (!IGN) t = dce_label(target, i64, at);
    if (t >= n) { bad += 1.f; continue; }
    if constexpr (IGN) ann += 1.f;
    float vt = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const bool hit = k == t;
      sp[k] += p[k];
      si[k] += hit ? p[k] : 0.f;
      sg[k] += hit ? 1.f : 0.f;
      vt = hit ? v[k] : vt;
    }
    ce += lse + mx - vt;
  }
  const int lane = tid & 63, w = tid >> 6;
  auto wsum = [](float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
  };
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const float a = wsum(sp[k]), c = wsum(si[k]), d = wsum(sg[k]);
    if (lane == 0) { red[w][k] = a; red[w][NC + k] = c; red[w][2 * NC + k] = d; }
  }
  ce = wsum(ce); bad = wsum(bad);
  if constexpr (IGN) ann = wsum(ann);
  if (lane == 0) {
    red[w][3 * NC] = ce; red[w][3 * NC + 1] = bad;
    if constexpr (IGN) red[w][3 * NC + 2] = ann;
  }
  __syncthreads();
  if (tid < NACC) part[((long long)b * gridDim.x + blockIdx.x) * NACC + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// The two halves of the finalize, shared by the one-call loss and the split one (the same statements in both, so world = 1 gives the same bits).
// dce_reduce_sums: sums[Bd][NACC] (double) from the workgroups' partials in ONE fixed order: per slot the images in order, each image's chunks in order.
__device__ __forceinline__ void dce_reduce_sums(const float* __restrict__ part, int chunks, int B, int NACC, int batch_dice, double* sums) {
  const int Bd = batch_dice ? 1 : B, tid = threadIdx.x;
  for (int slot = tid; slot < Bd * NACC; slot += 256) {
    const int bo = slot / NACC, k = slot - bo * NACC;
    const int b0 = batch_dice ? 0 : bo, b1 = batch_dice ? B : bo + 1;
    double a = 0.0;
    for (int b = b0; b < b1; ++b)
      for (int ch = 0; ch < chunks; ++ch) a += (double)part[((long long)b * chunks + ch) * NACC + k];
    sums[slot] = a;
  }
}

// dce_coef_loss: per (sample or batch, foreground class) the Dice coefficient from `dsums` and the two factors of its derivative, then the scalar, whose
// cross-entropy part comes from `lsums` (this process's pixels) over B HW.  With D = sum_gt + sum_pred + smooth, N = 2 intersect + smooth, M = Bd (n - 1) averaged terms:
//   dc = N / max(D, 1e-8);   coef[..][c] = world {2 / (max(D, 1e-8) M),  D < 1e-8 ? 0 : N / (D^2 M)}     d(-mean dc) / d p_c(pixel) = -(coef0 [t == c] - coef1)
// world = 1 and dsums == lsums is the single-process loss.  Under data parallelism dsums is the sum of the ranks' statistics and world their number: the
// gathered statistics' backward all-reduces identical rows, so every rank's Dice gradient carries the factor world (x 1.0 is exact).
// The ignore form is `inv_count` != nullptr (a run-time switch: scalar work of one workgroup, so the finalize kernels exist once): rows of 3 NC + 3, the
// cross-entropy over lsums' annotated count (exact: every partial count is an integer below 2^24, added in double; 0 when the count is 0), and
// inv_count[0] = (float)(1 / count), or 0, left for the gradient kernel.  The Dice sums saw annotated pixels only.
__device__ __forceinline__ void dce_coef_loss(const double* dsums, const double* lsums, int B, long long HW, int n, int NC, int batch_dice, float smooth, double world,
                                              double* dcs, float* __restrict__ coef, float* __restrict__ loss, float* __restrict__ inv_count) {
  const bool ign = inv_count != nullptr;
  const int NACC = 3 * NC + 2 + ign, Bd = batch_dice ? 1 : B, tid = threadIdx.x;
  const double M = (double)Bd * (double)(n - 1);
  for (int e = tid; e < Bd * NC; e += 256) {
    const int bo = e / NC, c = e - bo * NC;
    double dc = 0.0, c0 = 0.0, c1 = 0.0;
    if (c >= 1 && c < n) {
      const double* s = dsums + (long long)bo * NACC;
      const double D = s[2 * NC + c] + s[c] + (double)smooth, N = 2.0 * s[NC + c] + (double)smooth;
      const double Dc = D < 1e-8 ? 1e-8 : D;
      dc = N / Dc;
      c0 = 2.0 / (Dc * M);
      c1 = D < 1e-8 ? 0.0 : N / (D * D * M);
    }
    dcs[e] = dc;
    coef[(long long)e * 2] = (float)(c0 * world);
    coef[(long long)e * 2 + 1] = (float)(c1 * world);
  }
  __syncthreads();
  if (tid == 0) {
    double dsum = 0.0, ce = 0.0, bad = 0.0, count = 0.0;
    for (int e = 0; e < Bd * NC; ++e) dsum += dcs[e];
    for (int bo = 0; bo < Bd; ++bo) {
      ce += lsums[(long long)bo * NACC + 3 * NC];
      bad += lsums[(long long)bo * NACC + 3 * NC + 1];
      if (dsums != lsums) bad += dsums[(long long)bo * NACC + 3 * NC + 1];   // another process's bad label: the exchanged count
      if (ign) count += lsums[(long long)bo * NACC + 3 * NC + 2];
    }
    if (!ign) count = (double)B * (double)HW;
    const double v = (count > 0.0 ? ce / count : 0.0) - dsum / M;
    loss[0] = bad > 0.0 ? __builtin_nanf("") : (float)v;   // a label outside [0, n_heads): torch's cross_entropy raises; here the value and that pixel's dlogits are NaN
    if (ign) inv_count[0] = count > 0.0 ? (float)(1.0 / count) : 0.f;
  }
}

// One workgroup: both halves, the sums in the workspace.
__global__ __launch_bounds__(256) void dce_finalize_kernel(const float* __restrict__ part, int chunks, int B, long long HW, int n, int NC, int batch_dice,
                                                           float smooth, double* sums, double* dcs, float* __restrict__ coef,
                                                           float* __restrict__ loss, float* __restrict__ inv_count) {
  dce_reduce_sums(part, chunks, B, 3 * NC + 2 + (inv_count != nullptr), batch_dice, sums);
  __syncthreads();
  dce_coef_loss(sums, sums, B, HW, n, NC, batch_dice, smooth, 1.0, dcs, coef, loss, inv_count);
}

// The halves as kernels of their own (one workgroup each): the sums leave in a caller's buffer, may be added to other processes', and come back.
__global__ __launch_bounds__(256) void dce_reduce_kernel(const float* __restrict__ part, int chunks, int B, int NACC, int batch_dice, double* __restrict__ sums) {
  dce_reduce_sums(part, chunks, B, NACC, batch_dice, sums);
}

__global__ __launch_bounds__(256) void dce_from_sums_kernel(const double* dsums, const double* lsums, int B, long long HW, int n, int NC, int batch_dice, float smooth,
                                                            int world, double* dcs, float* __restrict__ coef, float* __restrict__ loss,
                                                            float* __restrict__ inv_count) {
  dce_coef_loss(dsums, lsums, B, HW, n, NC, batch_dice, smooth, (double)world, dcs, coef, loss, inv_count);
}

// dlogits[pixel][k] = gsw ((p_k - [k == t]) / count + p_k (g_k - sum_j p_j g_j)),  g_c = -(coef0_c [t == c] - coef1_c) for c >= 1, g_0 = 0;  pad columns 0
// count is B HW, or in the ignore form the annotated pixels, whose rows these are: an ignored pixel's row is +0, selected by the label alone
template <int NV, bool IGN>
__global__ __launch_bounds__(256) void dce_grad_kernel(const f16* __restrict__ logits, const void* __restrict__ target, int i64, long long HW, int n,
                                                       int batch_dice, const float* __restrict__ coef, DceCount<IGN> count, float gsw, f16* __restrict__ dlogits) {
  constexpr int NC = 8 * NV;
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * DCE_PIX, p1 = p0 + DCE_PIX < HW ? p0 + DCE_PIX : HW;
  float c0[NC], c1[NC];
  const float* cf = coef + (long long)(batch_dice ? 0 : b) * NC * 2;
#pragma unroll
  for (int k = 0; k < NC; ++k) { c0[k] = cf[2 * k]; c1[k] = cf[2 * k + 1]; }
  float inv_count;
  if constexpr (IGN) inv_count = count.inv[0]; else inv_count = count.inv;
  for (long long px = p0 + tid; px < p1; px += 256) {
    const long long at = (long long)b * HW + px;
    int t;
    if constexpr (IGN) {   // as in the partial kernel
      t = dce_label(target, i64, at);
      if (t == count.ignore) {
        f16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (f16)0.f;
#pragma unroll
        for (int q = 0; q < NV; ++q) *reinterpret_cast<f16x8*>(dlogits + at * NC + 8 * q) = z;
        continue;
      }
    }
    float v[NC], p[NC], lse, mx;
    dce_softmax<NV>(logits + at * NC, n, v, p, lse, mx);
    if constexpr (!IGN) t = dce_label(target, i64, at);
    const float poison = t >= n ? __builtin_nanf("") : 0.f;   // a label outside [0, n): the loss is NaN and so is this pixel's gradient, so the step is skipped
    float g[NC], dot = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      g[k] = c1[k] - (k == t ? c0[k] : 0.f);
      dot += p[k] * g[k];
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      f16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 8 * q + j;
        const float d = (p[k] - (k == t ? 1.f : 0.f)) * inv_count + p[k] * (g[k] - dot);
        o[j] = (f16)(k < n ? gsw * d + poison : 0.f);
      }
      *reinterpret_cast<f16x8*>(dlogits + at * NC + 8 * q) = o;
    }
  }
}

// The launchers' arguments that depend on the form: `ignore` is read only where IGN, `inv_count` (the workspace's scalar) is null in the plain form.
template <bool IGN>
DceIgnore<IGN> dce_ignore_arg(int ignore) {
  if constexpr (IGN) return ignore; else return {};
}
template <bool IGN>
DceCount<IGN> dce_count_arg(int B, long long HW, const float* inv_count, int ignore) {
  if constexpr (IGN) return {inv_count, ignore}; else return {(float)(1.0 / ((double)B * (double)HW))};
}

template <int NV, bool IGN>
void dce_launch(const f16* logits, const void* target, int i64, int B, long long HW, int n, int ignore, int batch_dice, float smooth, float gsw, float* loss,
                f16* dlogits, double* sums, double* dcs, float* coef, float* inv_count, float* part, hipStream_t s) {
  const int chunks = (int)((HW + DCE_PIX - 1) / DCE_PIX);
  const dim3 grid(chunks, B);
  hipLaunchKernelGGL((dce_partial_kernel<NV, IGN>), grid, dim3(256), 0, s, logits, target, i64, HW, n, dce_ignore_arg<IGN>(ignore), part);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(dce_finalize_kernel, dim3(1), dim3(256), 0, s, part, chunks, B, HW, n, 8 * NV, batch_dice, smooth, sums, dcs, coef, loss, inv_count);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((dce_grad_kernel<NV, IGN>), grid, dim3(256), 0, s, logits, target, i64, HW, n, batch_dice, coef, dce_count_arg<IGN>(B, HW, inv_count, ignore), gsw,
                     dlogits);
  HIP_CHECK(hipGetLastError());
}

template <int NV, bool IGN>
void dce_stats_launch(const f16* logits, const void* target, int i64, int B, long long HW, int n, int ignore, int batch_dice, double* sums_out, float* part,
                      hipStream_t s) {
  const int chunks = (int)((HW + DCE_PIX - 1) / DCE_PIX);
  hipLaunchKernelGGL((dce_partial_kernel<NV, IGN>), dim3(chunks, B), dim3(256), 0, s, logits, target, i64, HW, n, dce_ignore_arg<IGN>(ignore), part);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(dce_reduce_kernel, dim3(1), dim3(256), 0, s, part, chunks, B, dce_nacc(NV, IGN), batch_dice, sums_out);
  HIP_CHECK(hipGetLastError());
}

template <int NV, bool IGN>
void dce_from_sums_launch(const f16* logits, const void* target, int i64, int B, long long HW, int n, int ignore, int batch_dice, float smooth, float gsw,
                          const double* dsums, const double* lsums, int world, float* loss, f16* dlogits, double* dcs, float* coef, float* inv_count, hipStream_t s) {
  const int chunks = (int)((HW + DCE_PIX - 1) / DCE_PIX);
  hipLaunchKernelGGL(dce_from_sums_kernel, dim3(1), dim3(256), 0, s, dsums, lsums, B, HW, n, 8 * NV, batch_dice, smooth, world, dcs, coef, loss, inv_count);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((dce_grad_kernel<NV, IGN>), dim3(chunks, B), dim3(256), 0, s, logits, target, i64, HW, n, batch_dice, coef,
                     dce_count_arg<IGN>(B, HW, inv_count, ignore), gsw, dlogits);
  HIP_CHECK(hipGetLastError());
}

// ---- SGD with Nesterov momentum, every tensor in one launch ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgd_nesterov_multi_kernel(const SgdTensor* __restrict__ tensors, const float* const* __restrict__ grads,
                                                                 const AdamChunk* __restrict__ chunks, float lr, float momentum, float wd, int first,
                                                                 const float* __restrict__ inv_scale, const float* __restrict__ clip_coef) {
  const AdamChunk c = chunks[blockIdx.x];
  const SgdTensor t = tensors[c.tensor];
  const float* __restrict__ g = grads[c.tensor];
  const float sc = inv_scale[0] * clip_coef[0];
  const long long end = c.first + ADAMW_CHUNK < t.n ? c.first + ADAMW_CHUNK : t.n;
  for (long long i = c.first + threadIdx.x; i < end; i += 256) {
    const float pi = t.p[i];
    const float gi = sc * g[i] + wd * pi;
    const float bi = first ? gi : momentum * t.buf[i] + gi;
    t.buf[i] = bi;
    t.p[i] = pi - lr * (gi + momentum * bi);
  }
}

// ---- gradient bucket and its norm (data-parallel step) ------------------------------------------------------------------------------------------------
// bucket[offsets[t] + i] = grads[t][i]: workgroup c takes elements [first, first + ADAMW_CHUNK) of its tensor (the chunk table of the optimizer launches).
// 16-byte loads and stores where source and destination share their offset within 16 bytes (a scalar head up to the boundary, a scalar tail), else dwords.
__global__ __launch_bounds__(256) void bucket_pack_kernel(const float* const* __restrict__ grads, const long long* __restrict__ offsets,
                                                          const AdamChunk* __restrict__ chunks, float* __restrict__ bucket) {
  const AdamChunk c = chunks[blockIdx.x];
  const long long n = offsets[c.tensor + 1] - offsets[c.tensor];
  const long long end = c.first + ADAMW_CHUNK < n ? c.first + ADAMW_CHUNK : n;
  const float* __restrict__ src = grads[c.tensor] + c.first;
  float* __restrict__ dst = bucket + offsets[c.tensor] + c.first;
  const int len = (int)(end - c.first), tid = threadIdx.x;
  const unsigned long long sa = (unsigned long long)src, da = (unsigned long long)dst;
  if (((sa ^ da) & 15) != 0) {
    for (int i = tid; i < len; i += 256) dst[i] = src[i];
    return;
  }
  int head = (int)(((16 - (sa & 15)) & 15) >> 2);
  head = head < len ? head : len;
  const int nv = (len - head) >> 2, tail = head + 4 * nv;
  if (tid < head) dst[tid] = src[tid];
  const float4* __restrict__ sv = reinterpret_cast<const float4*>(src + head);
  float4* __restrict__ dv = reinterpret_cast<float4*>(dst + head);
  for (int i = tid; i < nv; i += 256) dv[i] = sv[i];
  if (tid < len - tail) dst[tail + tid] = src[tail + tid];
}

// sqrt(sum x^2) in two launches.  x = up to 3 scalar head elements to the first 16-byte boundary, nv float4 vectors, up to 3 scalar tail elements.  Workgroup w
// takes vectors [w SSQ_VECS, (w + 1) SSQ_VECS): a thread 16 of them, 256 apart, into one fp32 accumulator per vector lane; workgroup 0 adds the head and
// the tail (one more term in a lane-0 accumulator).  Then the four lanes as (a + b) + (c + d), the wave's xor tree, the four waves as (a + b) + (c + d): at most
// SSQ_CHAIN = 16 + 1 + 2 + 6 + 2 dependent fp32 roundings on any path into a partial.  The finalize adds the partials in double in one fixed order:
// 256 interleaved chains, then 8 chains of 32 of those in order, then the 8 in order.  No atomics: a replay gives the same bits.  Squares are not
// negative, so an inf or a NaN anywhere (an fp32 overflow of the sum included) reaches the result.
constexpr int SSQ_VECS = ADAMW_CHUNK / 4;
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, long long n, int head, long long nv, float* __restrict__ part) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + head);
  const long long v0 = (long long)blockIdx.x * SSQ_VECS, v1 = v0 + SSQ_VECS < nv ? v0 + SSQ_VECS : nv;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (long long i = v0 + tid; i < v1; i += 256) {
    const float4 v = xv[i];
    a0 = fmaf(v.x, v.x, a0); a1 = fmaf(v.y, v.y, a1); a2 = fmaf(v.z, v.z, a2); a3 = fmaf(v.w, v.w, a3);
  }
  if (blockIdx.x == 0) {
    const long long tail = head + 4 * nv;
    if (tid < head) { const float v = x[tid]; a0 = fmaf(v, v, a0); }
    else if (tid >= 64 && tail + (tid - 64) < n) { const float v = x[tail + (tid - 64)]; a0 = fmaf(v, v, a0); }
  }
  float a = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if ((tid & 63) == 0) red[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void sumsq_finalize_kernel(const float* __restrict__ part, int P, float* __restrict__ out) {
  __shared__ double red[256];
  __shared__ double red8[8];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int w = tid; w < P; w += 256) a += (double)part[w];
  red[tid] = a;
  __syncthreads();
  if (tid < 8) {
    double t = 0.0;
    for (int j = 0; j < 32; ++j) t += red[tid * 32 + j];
    red8[tid] = t;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int j = 0; j < 8; ++j) t += red8[j];
    out[0] = (float)sqrt(t);
  }
}

}  // namespace

long long in_train_ws_floats(int B, int HW, int C) {
  const InLayout l = in_layout(HW, C);
  return (long long)B * l.R * C * 2 + (long long)B * C * 2;
}

static void in_train_check(int B, int HW, int C, long long ws_bytes, const char* what) {
  LDIFF_CHECK(B >= 1 && B <= 65535 && HW >= 1 && C >= 8 && C % 8 == 0, LDIFF_ERR_INVALID, "%s: B=%d HW=%d C=%d (C must be a positive multiple of 8)", what, B, HW, C);
  LDIFF_CHECK(ws_bytes >= in_train_ws_floats(B, HW, C) * 4, LDIFF_ERR_INVALID, "%s: workspace of %lld bytes, %lld needed (ldiff_op_in_train_ws_bytes)", what,
              ws_bytes, in_train_ws_floats(B, HW, C) * 4);
}

void launch_in_train_fwd(const f16* x, f16* y, const float* gamma, const float* beta, float* mean, float* rstd, int B, int HW, int C, float eps, float slope,
                         float* ws, long long ws_bytes, hipStream_t s) {
  in_train_check(B, HW, C, ws_bytes, "in_train_fwd");
  const InLayout l = in_layout(HW, C);
  const dim3 grid(l.R, B);
  hipLaunchKernelGGL(in_partial_kernel<false>, grid, dim3(256), 0, s, x, (const f16*)nullptr, gamma, beta, (const float*)nullptr, (const float*)nullptr, ws, HW, C,
                     l.G, l.nrl, slope);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(in_fwd_finalize_kernel, dim3((C + 3) / 4, B), dim3(256), 0, s, ws, l.R, HW, C, eps, mean, rstd);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(in_apply_kernel<false>, grid, dim3(256), 0, s, x, (const f16*)nullptr, gamma, beta, mean, rstd, (const float*)nullptr, y, HW, C, l.G, l.nrl,
                     slope);
  HIP_CHECK(hipGetLastError());
}

void launch_in_train_bwd(const f16* x, const f16* dy, const float* gamma, const float* beta, const float* mean, const float* rstd, f16* dx, float* dgamma,
                         float* dbeta, int B, int HW, int C, float slope, float* ws, long long ws_bytes, hipStream_t s) {
  in_train_check(B, HW, C, ws_bytes, "in_train_bwd");
  const InLayout l = in_layout(HW, C);
  const dim3 grid(l.R, B);
  float* m = ws + (long long)B * l.R * C * 2;
  hipLaunchKernelGGL(in_partial_kernel<true>, grid, dim3(256), 0, s, x, dy, gamma, beta, mean, rstd, ws, HW, C, l.G, l.nrl, slope);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(in_bwd_finalize_kernel, dim3((C + 3) / 4), dim3(256), 0, s, ws, l.R, B, HW, C, m, dgamma, dbeta);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(in_apply_kernel<true>, grid, dim3(256), 0, s, x, dy, gamma, beta, mean, rstd, m, dx, HW, C, l.G, l.nrl, slope);
  HIP_CHECK(hipGetLastError());
}

// workspace: doubles sums[B][NACC], dcs[B][NC]; floats coef[B][NC][2], in the ignore form the 1 / count scalar, part[B][chunks][NACC].  dice_ce uses all of
// them; stats `part`, from_sums `dcs`, `coef` and the scalar.  inv_count is null in the plain form, which is how the finalize kernels tell the forms apart.
struct DceWs {
  int NV;
  bool ign;
  double *sums, *dcs;
  float *coef, *inv_count, *part;
  long long bytes;
  DceWs(void* ws, int B, long long HW, int n_heads, bool ign) : NV((n_heads + 7) / 8), ign(ign) {
    const int NC = 8 * NV, NACC = dce_nacc(NV, ign);
    const long long chunks = (HW + DCE_PIX - 1) / DCE_PIX;
    sums = (double*)ws;
    dcs = sums + (long long)B * NACC;
    coef = (float*)(dcs + (long long)B * NC);
    inv_count = ign ? coef + (long long)B * NC * 2 : nullptr;
    part = coef + (long long)B * NC * 2 + ign;
    bytes = ((long long)B * NACC + (long long)B * NC) * 8 + ((long long)B * NC * 2 + ign + (long long)B * chunks * NACC) * 4;
  }
};

long long dice_ce_ws_bytes(int B, long long HW, int n_heads, bool ign) { return DceWs(nullptr, B, HW, n_heads, ign).bytes; }
int dice_ce_nacc(int n_heads, bool ign) { return dce_nacc((n_heads + 7) / 8, ign); }

// the shape rules of the three entries and their workspace; with an ignore label, that label's rule and the ignore form's layout
static DceWs dice_ce_check(const char* what, int ld, int n_heads, std::optional<int> ignore_label, int B, long long HW, void* ws, long long ws_bytes) {
  const bool ign = ignore_label.has_value();
  LDIFF_CHECK(n_heads >= 2 && n_heads <= 32, LDIFF_ERR_INVALID, "%s: %d heads (2 .. 32: background and at least one foreground class)", what, n_heads);
  LDIFF_CHECK(ld == 8 * ((n_heads + 7) / 8), LDIFF_ERR_INVALID, "%s: row pitch %d, roundup(n_heads, 8) = %d expected (the seg layer's output layout)", what, ld,
              8 * ((n_heads + 7) / 8));
  LDIFF_CHECK(B >= 1 && HW >= 1 && HW <= (1ll << 40), LDIFF_ERR_INVALID, "%s: B=%d HW=%lld", what, B, HW);
  LDIFF_CHECK(B <= 65535, LDIFF_ERR_INVALID, "%s: B=%d exceeds the grid's second dimension", what, B);
  LDIFF_CHECK(!ign || (*ignore_label >= n_heads && *ignore_label <= 254), LDIFF_ERR_INVALID,
              "%s: ignore label %d (n_heads = %d .. 254: no class, and not 255, which every int64 label outside a byte's range is read as)", what,
              ignore_label.value_or(-1), n_heads);
  const DceWs w(ws, B, HW, n_heads, ign);
  LDIFF_CHECK(ws_bytes >= w.bytes, LDIFF_ERR_INVALID, "%s: workspace of %lld bytes, %lld needed (ldiff_op_dice_ce%s_ws_bytes)", what, ws_bytes, w.bytes,
              ign ? "_ignore" : "");
  return w;
}

// f(integral constant NV, bool constant IGN): the launchers are templates on the number of 8-column vectors of a logits row and on the form
template <class F>
static void dce_dispatch(const DceWs& w, F&& f) {
  auto by_nv = [&](auto ign) {
    switch (w.NV) {
      case 1: f(std::integral_constant<int, 1>{}, ign); break;
      case 2: f(std::integral_constant<int, 2>{}, ign); break;
      case 3: f(std::integral_constant<int, 3>{}, ign); break;
      default: f(std::integral_constant<int, 4>{}, ign); break;
    }
  };
  if (w.ign) by_nv(std::true_type{}); else by_nv(std::false_type{});
}

void launch_dice_ce(const f16* logits, int ld, int n_heads, std::optional<int> ignore_label, const void* target, int target_i64, int B, long long HW, int batch_dice,
                    float smooth, float weight, float grad_scale, float* loss, f16* dlogits, void* ws, long long ws_bytes, hipStream_t s) {
  const DceWs w = dice_ce_check(ignore_label ? "dice_ce_ignore" : "dice_ce", ld, n_heads, ignore_label, B, HW, ws, ws_bytes);
  dce_dispatch(w, [&](auto nv, auto ign) {
    dce_launch<decltype(nv)::value, decltype(ign)::value>(logits, target, target_i64, B, HW, n_heads, ignore_label.value_or(0), batch_dice, smooth, weight * grad_scale,
                                                          loss, dlogits, w.sums, w.dcs, w.coef, w.inv_count, w.part, s);
  });
}

void launch_sgd_nesterov_multi(const SgdTensor* tensors, const float* const* grads, const AdamChunk* chunks, long long nchunks, float lr, float momentum, float wd,
                               int first, const float* inv_scale, const float* clip_coef, hipStream_t s) {
  if (nchunks == 0) return;
  hipLaunchKernelGGL(sgd_nesterov_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, tensors, grads, chunks, lr, momentum, wd, first, inv_scale, clip_coef);
  HIP_CHECK(hipGetLastError());
}

void launch_dice_ce_stats(const f16* logits, int ld, int n_heads, std::optional<int> ignore_label, const void* target, int target_i64, int B, long long HW,
                          int batch_dice, double* sums, void* ws, long long ws_bytes, hipStream_t s) {
  const DceWs w = dice_ce_check(ignore_label ? "dice_ce_ignore_stats" : "dice_ce_stats", ld, n_heads, ignore_label, B, HW, ws, ws_bytes);
  dce_dispatch(w, [&](auto nv, auto ign) {
    dce_stats_launch<decltype(nv)::value, decltype(ign)::value>(logits, target, target_i64, B, HW, n_heads, ignore_label.value_or(0), batch_dice, sums, w.part, s);
  });
}

void launch_dice_ce_from_sums(const f16* logits, int ld, int n_heads, std::optional<int> ignore_label, const void* target, int target_i64, int B, long long HW,
                              int batch_dice, float smooth, float weight, float grad_scale, const double* dice_sums, const double* local_sums, int world, float* loss,
                              f16* dlogits, void* ws, long long ws_bytes, hipStream_t s) {
  const char* what = ignore_label ? "dice_ce_ignore_from_sums" : "dice_ce_from_sums";
  const DceWs w = dice_ce_check(what, ld, n_heads, ignore_label, B, HW, ws, ws_bytes);
  LDIFF_CHECK(world >= 1, LDIFF_ERR_INVALID, "%s: world=%d", what, world);
  LDIFF_CHECK(batch_dice || (world == 1 && dice_sums == local_sums), LDIFF_ERR_INVALID,
              "%s: without batch_dice the Dice term is per sample and stays local (world = 1, dice_sums = local_sums)", what);
  dce_dispatch(w, [&](auto nv, auto ign) {
    dce_from_sums_launch<decltype(nv)::value, decltype(ign)::value>(logits, target, target_i64, B, HW, n_heads, ignore_label.value_or(0), batch_dice, smooth,
                                                                    weight * grad_scale, dice_sums, local_sums, world, loss, dlogits, w.dcs, w.coef, w.inv_count, s);
  });
}

void launch_bucket_pack(const float* const* grads, const long long* offsets, const AdamChunk* chunks, long long nchunks, float* bucket, hipStream_t s) {
  if (nchunks == 0) return;
  hipLaunchKernelGGL(bucket_pack_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, grads, offsets, chunks, bucket);
  HIP_CHECK(hipGetLastError());
}

long long sumsq_ws_bytes(long long n) {
  if (n < 1) return 0;
  const long long nv = (n + 3) / 4;
  return ((nv + SSQ_VECS - 1) / SSQ_VECS) * 4;
}

void launch_sumsq(const float* x, long long n, float* out, float* ws, long long ws_bytes, hipStream_t s) {
  LDIFF_CHECK(n >= 1 && n <= (1ll << 40), LDIFF_ERR_INVALID, "sumsq: n=%lld", n);
  LDIFF_CHECK(((unsigned long long)x & 3) == 0, LDIFF_ERR_INVALID, "sumsq: x is not 4-byte aligned");
  LDIFF_CHECK(ws_bytes >= sumsq_ws_bytes(n), LDIFF_ERR_INVALID, "sumsq: workspace of %lld bytes, %lld needed (ldiff_op_sumsq_ws_bytes)", ws_bytes, sumsq_ws_bytes(n));
  long long head = (long long)(((16 - ((unsigned long long)x & 15)) & 15) >> 2);
  head = head < n ? head : n;
  const long long nv = (n - head) / 4;
  const long long P = nv > 0 ? (nv + SSQ_VECS - 1) / SSQ_VECS : 1;   // <= sumsq_ws_bytes(n) / 4: nv <= n / 4
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)P), dim3(256), 0, s, x, n, (int)head, nv, ws);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sumsq_finalize_kernel, dim3(1), dim3(256), 0, s, ws, (int)P, out);
  HIP_CHECK(hipGetLastError());
}
