// Region labels of the nnU-Net tissue head (gfx950, MI355X): one sigmoid head per region, regions may overlap ("lesion = tumour + necrosis").
//   dice_focal                    DC_and_Focal_loss (focal: alpha 0.25, gamma 2) or DC_and_BCE_loss over MemoryEfficientSoftDiceLoss(sigmoid, do_bg) of ONE
//                                 deep-supervision scale: value and d loss / d logits
//   dice_focal_stats / _from_sums the same loss split at its sums, as dice_ce's (kernels_segtrain.hip), for data-parallel ranks
//   region_counts                 tp / fp / fn per region of `logit > threshold` against the label map, exact (int64)
//   region_mask_u8                convert_probabilities_to_segmentation's region branch: regions_class_order written in order where logit > threshold
// The target is the LABEL MAP: membership of a label value in a region is a bit of the 256-entry table the kernels hold in LDS, so the one-hot region
// tensor never exists.  table[v]: bit r = v belongs to region r; bit 31 = v is the ignore label; bit 30 = v is no label of the dataset (a bad label).
// The loss kernels follow kernels_segtrain.hip's Dice + cross-entropy: a thread takes a pixel, a workgroup DFL_PIX consecutive pixels of one image, the
// per-workgroup partial sums are fp32, one workgroup adds them in double in one fixed order.  No floating-point atomics: a replay gives the same bits.
#include "common.h"

namespace {

constexpr int DFL_PIX = 4096;              // pixels per workgroup: 16 per thread, as the plain loss's DCE_PIX
constexpr unsigned REG_IGNORE = 1u << 31;
constexpr unsigned REG_BAD = 1u << 30;
inline int dfl_nacc(int NV) { return 3 * 8 * NV + 3; }   // sum_pred[NC], intersect[NC], sum_gt[NC], the focal / BCE sum, bad labels, annotated pixels

__device__ __forceinline__ int reg_label(const void* __restrict__ target, int i64, long long at) {
  if (i64) {
    const long long t = reinterpret_cast<const long long*>(target)[at];
    return (t < 0 || t > 255) ? 255 : (int)t;   // the host leaves bit 30 in entry 255 unless 255 is itself a label
  }
  return (int)reinterpret_cast<const unsigned char*>(target)[at];
}

// what a pixel is to the loss: 0 = annotated, 1 = ignored (skipped), 2 = bad (poisons).  An ignore bit without use_ignore is a bad label.
__device__ __forceinline__ int reg_kind(unsigned m, int use_ignore) {
  if (m & REG_BAD) return 2;
  if (m & REG_IGNORE) return use_ignore ? 1 : 2;
  return 0;
}

// One (pixel, region) in fp32.  e = exp(-|x|) never overflows; p = sigmoid(x) and pm = 1 - p come from the same quotient, so neither cancels.
//   bce = softplus(-s x) = max(x, 0) - x y + log1p(e),  s = 2 y - 1,  p_t = sigmoid(s x),  q = sigmoid(-s x)
//   focal: f = 0.25 q^2 bce,  df/dx = -0.25 s q^2 (2 p_t bce + q);      BCE: f = bce,  df/dx = p - y
struct RegTerm { float p, pm, f, df; };
template <bool BCE>
__device__ __forceinline__ RegTerm reg_term(float x, bool y) {
  const float e = expf(-fabsf(x));
  const float r = 1.0f / (1.0f + e), big = r, small = e * r;
  const bool pos = x >= 0.f;
  RegTerm t;
  t.p = pos ? big : small;
  t.pm = pos ? small : big;
  // max(x, 0) - x y is 0, x or -x: formed as max(-s x, 0), which is the same value for every finite x and stays 0 where x = +-inf agrees with y
  // (inf - inf would be NaN there, as it is in torch's formulation; an fp16 logit can saturate)
  const float bce = (y ? fmaxf(-x, 0.f) : fmaxf(x, 0.f)) + log1pf(e);
  if constexpr (BCE) {
    t.f = bce;
    t.df = y ? -t.pm : t.p;
  } else {
    const float pt = y ? t.p : t.pm, q = y ? t.pm : t.p;
    const float aq2 = 0.25f * q * q;
    t.f = aq2 * bce;
    const float d = aq2 * (2.0f * pt * bce + q);
    t.df = y ? -d : d;
  }
  if (x != x) t.p = t.pm = t.f = t.df = x;   // a NaN logit reaches every output
  return t;
}

template <int NV>
__device__ __forceinline__ void reg_load_row(const f16* __restrict__ row, float (&v)[8 * NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const f16x8 t = *reinterpret_cast<const f16x8*>(row + 8 * k);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[8 * k + j] = (float)t[j];
  }
}

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int NV, bool BCE>
__global__ __launch_bounds__(256) void dfl_partial_kernel(const f16* __restrict__ logits, const void* __restrict__ target, int i64, const unsigned* __restrict__ table,
                                                          long long HW, int n, int use_ignore, float* __restrict__ part) {
  constexpr int NC = 8 * NV, NACC = 3 * NC + 3;
  __shared__ float red[4][NACC];
  __shared__ unsigned tab[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  tab[tid] = table[tid];
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * DFL_PIX, p1 = p0 + DFL_PIX < HW ? p0 + DFL_PIX : HW;
  float sp[NC], si[NC], sg[NC], fs = 0.f, bad = 0.f, ann = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) sp[k] = si[k] = sg[k] = 0.f;
  for (long long px = p0 + tid; px < p1; px += 256) {
    const long long at = (long long)b * HW + px;
    const unsigned m = tab[reg_label(target, i64, at)];   // the label first: an ignored pixel's logits are never loaded
    const int kind = reg_kind(m, use_ignore);
    if (kind == 1) continue;
    if (kind == 2) { bad += 1.f; continue; }
    ann += 1.f;
    float v[NC];
    reg_load_row<NV>(logits + at * NC, v);
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (k < n) {
        const bool y = (m >> k) & 1u;
        const RegTerm t = reg_term<BCE>(v[k], y);
        sp[k] += t.p;
        si[k] += y ? t.p : 0.f;
        sg[k] += y ? 1.f : 0.f;
        fs += t.f;
      }
    }
  }
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const float a = wave_sum_f(sp[k]), c = wave_sum_f(si[k]), d = wave_sum_f(sg[k]);
    if (lane == 0) { red[w][k] = a; red[w][NC + k] = c; red[w][2 * NC + k] = d; }
  }
  fs = wave_sum_f(fs); bad = wave_sum_f(bad); ann = wave_sum_f(ann);
  if (lane == 0) { red[w][3 * NC] = fs; red[w][3 * NC + 1] = bad; red[w][3 * NC + 2] = ann; }
  __syncthreads();
  if (tid < NACC) part[((long long)b * gridDim.x + blockIdx.x) * NACC + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// sums[Bd][NACC] (double) from the workgroups' partials in ONE fixed order: per slot the images in order, each image's chunks in order (dice_ce's rule)
__device__ __forceinline__ void dfl_reduce_sums(const float* __restrict__ part, int chunks, int B, int NACC, int batch_dice, double* sums) {
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

// Per (sample or batch, region) the Dice coefficient from `dsums` and the two factors of its derivative, then the scalar.  do_bg = True: ALL n regions,
// M = Bd n averaged terms.  With D = sum_gt + sum_pred + smooth, N = 2 intersect + smooth:
//   dc = N / max(D, 1e-8);   coef[..][r] = world {2 / (max(D, 1e-8) M),  D < 1e-8 ? 0 : N / (D^2 M)}     d(-mean dc) / d p_r(pixel) = -(coef0 y_r - coef1)
// The focal / BCE sum comes from `lsums` (this process's pixels).  Its normaliser: use_ignore = 0 the mean over B n HW elements; use_ignore = 1 the sum over
// max(A, 1e-8), A = this process's annotated PIXELS -- the reference does not multiply by n there, so the two differ by the factor n even when nothing is
// ignored.  inv_norm[0] = 1 / normaliser (0 for A = 0, where no row carries a gradient) is left for the gradient kernel.
__device__ __forceinline__ void dfl_coef_loss(const double* dsums, const double* lsums, int B, long long HW, int n, int NC, int batch_dice, int use_ignore, float smooth,
                                              double world, double* dcs, float* __restrict__ coef, float* __restrict__ loss, float* __restrict__ inv_norm) {
  const int NACC = 3 * NC + 3, Bd = batch_dice ? 1 : B, tid = threadIdx.x;
  const double M = (double)Bd * (double)n;
  for (int e = tid; e < Bd * NC; e += 256) {
    const int bo = e / NC, c = e - bo * NC;
    double dc = 0.0, c0 = 0.0, c1 = 0.0;
    if (c < n) {
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
    double dsum = 0.0, fs = 0.0, bad = 0.0, count = 0.0;
    for (int e = 0; e < Bd * NC; ++e) dsum += dcs[e];
    for (int bo = 0; bo < Bd; ++bo) {
      fs += lsums[(long long)bo * NACC + 3 * NC];
      bad += lsums[(long long)bo * NACC + 3 * NC + 1];
      if (dsums != lsums) bad += dsums[(long long)bo * NACC + 3 * NC + 1];   // another process's bad label: the exchanged count
      count += lsums[(long long)bo * NACC + 3 * NC + 2];
    }
    const double norm = use_ignore ? (count > 1e-8 ? count : 1e-8) : (double)B * (double)n * (double)HW;
    const double v = fs / norm - dsum / M;
    loss[0] = bad > 0.0 ? __builtin_nanf("") : (float)v;
    inv_norm[0] = (use_ignore && count <= 0.0) ? 0.f : (float)(1.0 / norm);
  }
}

__global__ __launch_bounds__(256) void dfl_finalize_kernel(const float* __restrict__ part, int chunks, int B, long long HW, int n, int NC, int batch_dice,
                                                           int use_ignore, float smooth, double* sums, double* dcs, float* __restrict__ coef,
                                                           float* __restrict__ loss, float* __restrict__ inv_norm) {
  dfl_reduce_sums(part, chunks, B, 3 * NC + 3, batch_dice, sums);
  __syncthreads();
  dfl_coef_loss(sums, sums, B, HW, n, NC, batch_dice, use_ignore, smooth, 1.0, dcs, coef, loss, inv_norm);
}

__global__ __launch_bounds__(256) void dfl_reduce_kernel(const float* __restrict__ part, int chunks, int B, int NACC, int batch_dice, double* __restrict__ sums) {
  dfl_reduce_sums(part, chunks, B, NACC, batch_dice, sums);
}

__global__ __launch_bounds__(256) void dfl_from_sums_kernel(const double* dsums, const double* lsums, int B, long long HW, int n, int NC, int batch_dice,
                                                            int use_ignore, float smooth, int world, double* dcs, float* __restrict__ coef,
                                                            float* __restrict__ loss, float* __restrict__ inv_norm) {
  dfl_coef_loss(dsums, lsums, B, HW, n, NC, batch_dice, use_ignore, smooth, (double)world, dcs, coef, loss, inv_norm);
}

// dlogits[pixel][r] = gsw (df_r inv_norm + p_r (1 - p_r) (coef1_r - coef0_r y_r));  pad columns and ignored rows +0;  a bad label's row NaN
template <int NV, bool BCE>
__global__ __launch_bounds__(256) void dfl_grad_kernel(const f16* __restrict__ logits, const void* __restrict__ target, int i64, const unsigned* __restrict__ table,
                                                       long long HW, int n, int batch_dice, int use_ignore, const float* __restrict__ coef,
                                                       const float* __restrict__ inv_norm, float gsw, f16* __restrict__ dlogits) {
  constexpr int NC = 8 * NV;
  __shared__ unsigned tab[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  tab[tid] = table[tid];
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * DFL_PIX, p1 = p0 + DFL_PIX < HW ? p0 + DFL_PIX : HW;
  float c0[NC], c1[NC];
  const float* cf = coef + (long long)(batch_dice ? 0 : b) * NC * 2;
#pragma unroll
  for (int k = 0; k < NC; ++k) { c0[k] = cf[2 * k]; c1[k] = cf[2 * k + 1]; }
  const float inv = inv_norm[0];
  for (long long px = p0 + tid; px < p1; px += 256) {
    const long long at = (long long)b * HW + px;
    const unsigned m = tab[reg_label(target, i64, at)];
    const int kind = reg_kind(m, use_ignore);
    if (kind == 1) {
      f16x8 z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = (f16)0.f;
#pragma unroll
      for (int q = 0; q < NV; ++q) *reinterpret_cast<f16x8*>(dlogits + at * NC + 8 * q) = z;
      continue;
    }
    const float poison = kind == 2 ? __builtin_nanf("") : 0.f;
    float v[NC];
    reg_load_row<NV>(logits + at * NC, v);
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      f16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 8 * q + j;
        float d = 0.f;
        if (k < n) {
          const bool y = (m >> k) & 1u;
          const RegTerm t = reg_term<BCE>(v[k], y);
          d = gsw * (t.df * inv + t.p * t.pm * (c1[k] - (y ? c0[k] : 0.f))) + poison;
        }
        o[j] = (f16)d;
      }
      *reinterpret_cast<f16x8*>(dlogits + at * NC + 8 * q) = o;
    }
  }
}

// ---- validation counts ------------------------------------------------------------------------------------------------------------------------------
// part[(b chunks + chunk)][3 NC] (int32): tp, fp, fn per region over the workgroup's annotated pixels; a bad label is no member of any region.
template <int NV>
__global__ __launch_bounds__(256) void region_counts_partial_kernel(const f16* __restrict__ logits, const void* __restrict__ target, int i64,
                                                                    const unsigned* __restrict__ table, long long HW, int n, float threshold, int* __restrict__ part) {
  constexpr int NC = 8 * NV;
  __shared__ int red[4][3 * NC];
  __shared__ unsigned tab[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  tab[tid] = table[tid];
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * DFL_PIX, p1 = p0 + DFL_PIX < HW ? p0 + DFL_PIX : HW;
  int tp[NC], fp[NC], fn[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) tp[k] = fp[k] = fn[k] = 0;
  for (long long px = p0 + tid; px < p1; px += 256) {
    const long long at = (long long)b * HW + px;
    const unsigned m = tab[reg_label(target, i64, at)];
    if (m & REG_IGNORE) continue;
    float v[NC];
    reg_load_row<NV>(logits + at * NC, v);
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const bool y = (m >> k) & 1u, pr = v[k] > threshold;   // a NaN logit compares false
      tp[k] += (pr && y) ? 1 : 0;
      fp[k] += (pr && !y) ? 1 : 0;
      fn[k] += (!pr && y) ? 1 : 0;
    }
  }
  const int lane = tid & 63, w = tid >> 6;
  auto isum = [](int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
  };
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int a = isum(tp[k]), c = isum(fp[k]), d = isum(fn[k]);
    if (lane == 0) { red[w][k] = a; red[w][NC + k] = c; red[w][2 * NC + k] = d; }
  }
  __syncthreads();
  if (tid < 3 * NC) part[((long long)b * gridDim.x + blockIdx.x) * 3 * NC + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// out[3][n] (int64) = the partials' sums
__global__ __launch_bounds__(256) void region_counts_finalize_kernel(const int* __restrict__ part, long long nparts, int n, int NC, long long* __restrict__ out) {
  for (int k = threadIdx.x; k < 3 * NC; k += 256) {
    const int which = k / NC, c = k - which * NC;
    if (c >= n) continue;
    long long a = 0;
    for (long long i = 0; i < nparts; ++i) a += (long long)part[i * 3 * NC + k];
    out[which * n + c] = a;
  }
}

// ---- the mask -----------------------------------------------------------------------------------------------------------------------------------------
struct RegionOrder { unsigned char c[24]; };

template <class T>
__global__ __launch_bounds__(256) void region_mask_kernel(const T* __restrict__ logits, int R, int H, int W, RegionOrder order, float threshold,
                                                          unsigned char* __restrict__ mask, int mask_W, int mask_y0, int mask_x0) {
  const long long HW = (long long)H * W, i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  unsigned char v = 0;
  for (int r = 0; r < R; ++r)
    if ((float)logits[(long long)r * HW + i] > threshold) v = order.c[r];   // later entries overwrite earlier ones; a NaN logit compares false
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  mask[(long long)(mask_y0 + y) * mask_W + mask_x0 + x] = v;
}

struct DflWs {
  int NV;
  double *sums, *dcs;
  float *coef, *inv_norm, *part;
  long long bytes;
  DflWs(void* ws, int B, long long HW, int n) : NV((n + 7) / 8) {
    const int NC = 8 * NV, NACC = dfl_nacc(NV);
    const long long chunks = (HW + DFL_PIX - 1) / DFL_PIX;
    sums = (double*)ws;
    dcs = sums + (long long)B * NACC;
    coef = (float*)(dcs + (long long)B * NC);
    inv_norm = coef + (long long)B * NC * 2;
    part = inv_norm + 1;
    bytes = ((long long)B * NACC + (long long)B * NC) * 8 + ((long long)B * NC * 2 + 1 + (long long)B * chunks * NACC) * 4;
  }
};

DflWs dfl_check(const char* what, int ld, int n, const void* table, int use_ignore, int bce, int B, long long HW, void* ws, long long ws_bytes) {
  LDIFF_CHECK(n >= 1 && n <= 24, LDIFF_ERR_INVALID, "%s: %d regions (1 .. 24: the membership table has 24 region bits)", what, n);
  LDIFF_CHECK(ld == 8 * ((n + 7) / 8), LDIFF_ERR_INVALID, "%s: row pitch %d, roundup(n_regions, 8) = %d expected (the seg layer's output layout)", what, ld,
              8 * ((n + 7) / 8));
  LDIFF_CHECK(B >= 1 && HW >= 1 && HW <= (1ll << 40), LDIFF_ERR_INVALID, "%s: B=%d HW=%lld", what, B, HW);
  LDIFF_CHECK(B <= 65535, LDIFF_ERR_INVALID, "%s: B=%d exceeds the grid's second dimension", what, B);
  LDIFF_CHECK(table != nullptr, LDIFF_ERR_INVALID, "%s: null membership table", what);
  LDIFF_CHECK((use_ignore == 0 || use_ignore == 1) && (bce == 0 || bce == 1), LDIFF_ERR_INVALID, "%s: use_ignore=%d bce=%d (0 or 1 each)", what, use_ignore, bce);
  const DflWs w(ws, B, HW, n);
  LDIFF_CHECK(ws_bytes >= w.bytes, LDIFF_ERR_INVALID, "%s: workspace of %lld bytes, %lld needed (ldiff_op_dice_focal_ws_bytes)", what, ws_bytes, w.bytes);
  return w;
}

// f(integral constant NV, bool constant BCE)
template <class F>
void dfl_dispatch(int NV, int bce, F&& f) {
  auto by_nv = [&](auto form) {
    switch (NV) {
      case 1: f(std::integral_constant<int, 1>{}, form); break;
      case 2: f(std::integral_constant<int, 2>{}, form); break;
      default: f(std::integral_constant<int, 3>{}, form); break;
    }
  };
  if (bce) by_nv(std::true_type{}); else by_nv(std::false_type{});
}

}  // namespace

long long dice_focal_ws_bytes(int B, long long HW, int n_regions) { return DflWs(nullptr, B, HW, n_regions).bytes; }
int dice_focal_nacc(int n_regions) { return dfl_nacc((n_regions + 7) / 8); }

void launch_dice_focal(const f16* logits, int ld, int n, const unsigned* table, const void* target, int target_i64, int use_ignore, int bce, int B, long long HW,
                       int batch_dice, float smooth, float weight, float grad_scale, float* loss, f16* dlogits, void* ws, long long ws_bytes, hipStream_t s) {
  const DflWs w = dfl_check("dice_focal", ld, n, table, use_ignore, bce, B, HW, ws, ws_bytes);
  const int chunks = (int)((HW + DFL_PIX - 1) / DFL_PIX);
  const dim3 grid(chunks, B);
  dfl_dispatch(w.NV, bce, [&](auto nv, auto form) {
    constexpr int NV = decltype(nv)::value;
    constexpr bool BCE = decltype(form)::value;
    hipLaunchKernelGGL((dfl_partial_kernel<NV, BCE>), grid, dim3(256), 0, s, logits, target, target_i64, table, HW, n, use_ignore, w.part);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dfl_finalize_kernel, dim3(1), dim3(256), 0, s, w.part, chunks, B, HW, n, 8 * NV, batch_dice, use_ignore, smooth, w.sums, w.dcs, w.coef, loss,
                       w.inv_norm);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((dfl_grad_kernel<NV, BCE>), grid, dim3(256), 0, s, logits, target, target_i64, table, HW, n, batch_dice, use_ignore, w.coef, w.inv_norm,
                       weight * grad_scale, dlogits);
    HIP_CHECK(hipGetLastError());
  });
}

void launch_dice_focal_stats(const f16* logits, int ld, int n, const unsigned* table, const void* target, int target_i64, int use_ignore, int bce, int B, long long HW,
                             int batch_dice, double* sums, void* ws, long long ws_bytes, hipStream_t s) {
  const DflWs w = dfl_check("dice_focal_stats", ld, n, table, use_ignore, bce, B, HW, ws, ws_bytes);
  const int chunks = (int)((HW + DFL_PIX - 1) / DFL_PIX);
  dfl_dispatch(w.NV, bce, [&](auto nv, auto form) {
    constexpr int NV = decltype(nv)::value;
    hipLaunchKernelGGL((dfl_partial_kernel<NV, decltype(form)::value>), dim3(chunks, B), dim3(256), 0, s, logits, target, target_i64, table, HW, n, use_ignore, w.part);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dfl_reduce_kernel, dim3(1), dim3(256), 0, s, w.part, chunks, B, dfl_nacc(NV), batch_dice, sums);
    HIP_CHECK(hipGetLastError());
  });
}

void launch_dice_focal_from_sums(const f16* logits, int ld, int n, const unsigned* table, const void* target, int target_i64, int use_ignore, int bce, int B,
                                 long long HW, int batch_dice, float smooth, float weight, float grad_scale, const double* dice_sums, const double* local_sums, int world,
                                 float* loss, f16* dlogits, void* ws, long long ws_bytes, hipStream_t s) {
  const char* what = "dice_focal_from_sums";
  const DflWs w = dfl_check(what, ld, n, table, use_ignore, bce, B, HW, ws, ws_bytes);
  LDIFF_CHECK(world >= 1, LDIFF_ERR_INVALID, "%s: world=%d", what, world);
  LDIFF_CHECK(batch_dice || (world == 1 && dice_sums == local_sums), LDIFF_ERR_INVALID,
              "%s: without batch_dice the Dice term is per sample and stays local (world = 1, dice_sums = local_sums)", what);
  LDIFF_CHECK(!use_ignore || (world == 1 && dice_sums == local_sums), LDIFF_ERR_INVALID,
              "%s: the data-parallel exchange with an ignore label is not built (world = 1, dice_sums = local_sums)", what);
  const int chunks = (int)((HW + DFL_PIX - 1) / DFL_PIX);
  dfl_dispatch(w.NV, bce, [&](auto nv, auto form) {
    constexpr int NV = decltype(nv)::value;
    hipLaunchKernelGGL(dfl_from_sums_kernel, dim3(1), dim3(256), 0, s, dice_sums, local_sums, B, HW, n, 8 * NV, batch_dice, use_ignore, smooth, world, w.dcs, w.coef,
                       loss, w.inv_norm);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((dfl_grad_kernel<NV, decltype(form)::value>), dim3(chunks, B), dim3(256), 0, s, logits, target, target_i64, table, HW, n, batch_dice, use_ignore,
                       w.coef, w.inv_norm, weight * grad_scale, dlogits);
    HIP_CHECK(hipGetLastError());
  });
}

long long region_counts_ws_bytes(int B, long long HW, int n_regions) {
  return (long long)B * ((HW + DFL_PIX - 1) / DFL_PIX) * 3 * 8 * ((n_regions + 7) / 8) * 4;
}

void launch_region_counts(const f16* logits, int ld, int n, const unsigned* table, const void* target, int target_i64, int B, long long HW, float threshold,
                          long long* counts, void* ws, long long ws_bytes, hipStream_t s) {
  const char* what = "region_counts";
  LDIFF_CHECK(n >= 1 && n <= 24, LDIFF_ERR_INVALID, "%s: %d regions (1 .. 24)", what, n);
  LDIFF_CHECK(ld == 8 * ((n + 7) / 8), LDIFF_ERR_INVALID, "%s: row pitch %d, roundup(n_regions, 8) = %d expected", what, ld, 8 * ((n + 7) / 8));
  LDIFF_CHECK(B >= 1 && B <= 65535 && HW >= 1 && HW <= (1ll << 40), LDIFF_ERR_INVALID, "%s: B=%d HW=%lld", what, B, HW);
  LDIFF_CHECK(ws_bytes >= region_counts_ws_bytes(B, HW, n), LDIFF_ERR_INVALID, "%s: workspace of %lld bytes, %lld needed (ldiff_op_region_counts_ws_bytes)", what,
              ws_bytes, region_counts_ws_bytes(B, HW, n));
  const int NV = (n + 7) / 8, chunks = (int)((HW + DFL_PIX - 1) / DFL_PIX);
  int* part = (int*)ws;
  const dim3 grid(chunks, B);
  switch (NV) {
    case 1: hipLaunchKernelGGL(region_counts_partial_kernel<1>, grid, dim3(256), 0, s, logits, target, target_i64, table, HW, n, threshold, part); break;
    case 2: hipLaunchKernelGGL(region_counts_partial_kernel<2>, grid, dim3(256), 0, s, logits, target, target_i64, table, HW, n, threshold, part); break;
    default: hipLaunchKernelGGL(region_counts_partial_kernel<3>, grid, dim3(256), 0, s, logits, target, target_i64, table, HW, n, threshold, part); break;
  }
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(region_counts_finalize_kernel, dim3(1), dim3(256), 0, s, part, (long long)B * chunks, n, 8 * NV, counts);
  HIP_CHECK(hipGetLastError());
}

void launch_region_mask_u8(const void* logits, int is_f32, int R, int H, int W, const int* order, float threshold, uint8_t* mask, int mask_H, int mask_W, int mask_y0,
                           int mask_x0, hipStream_t s) {
  const char* what = "region_mask_u8";
  LDIFF_CHECK(R >= 1 && R <= 24, LDIFF_ERR_INVALID, "%s: %d regions (1 .. 24)", what, R);
  LDIFF_CHECK(H >= 1 && W >= 1 && (long long)H * W <= (1ll << 38), LDIFF_ERR_INVALID, "%s: H=%d W=%d", what, H, W);
  LDIFF_CHECK(mask_y0 >= 0 && mask_x0 >= 0 && (long long)mask_y0 + H <= mask_H && (long long)mask_x0 + W <= mask_W, LDIFF_ERR_INVALID,
              "%s: the %d x %d box at (%d, %d) does not lie inside the %d x %d mask", what, H, W, mask_y0, mask_x0, mask_H, mask_W);
  RegionOrder o{};
  for (int r = 0; r < R; ++r) {
    LDIFF_CHECK(order[r] >= 0 && order[r] <= 255, LDIFF_ERR_INVALID, "%s: regions_class_order[%d] = %d does not fit a uint8 mask", what, r, order[r]);
    o.c[r] = (unsigned char)order[r];
  }
  const long long HW = (long long)H * W;
  const dim3 grid((unsigned)((HW + 255) / 256));
  if (is_f32)
    hipLaunchKernelGGL(region_mask_kernel<float>, grid, dim3(256), 0, s, (const float*)logits, R, H, W, o, threshold, mask, mask_W, mask_y0, mask_x0);
  else
    hipLaunchKernelGGL(region_mask_kernel<f16>, grid, dim3(256), 0, s, (const f16*)logits, R, H, W, o, threshold, mask, mask_W, mask_y0, mask_x0);
  HIP_CHECK(hipGetLastError());
}
