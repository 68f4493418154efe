// Kernels of the cell head's instance classifier (ldiff_resnet: torchvision's ResNet152 trunk + adapter conv + linear head on 64 x 64 crops, hundreds per call):
//   clsconv<ks, NT, MT>   implicit-GEMM conv, ks 1 | 3 | 7, stride 1 | 2, pad ks / 2, bias (+ residual) (+ ReLU) in the fp32 epilogue; <..., BN>: the raw sums and their
//                         training-mode BatchNorm partials instead (ConvParams::bn_stats)
//   maxpool3x3s2          the stem's pooling
//   crop_resize_norm      bounding-box crops of the decoded image -> [n, S, S, 8] normalised fp16 (the reference's PIL / torchvision preprocessing chain)
//   cls_head              mean over the adapter's map + Linear -> logits, label = 1 + argmax(logits[1:])
//
// Shape of clsconv.  The maps are 32^2 down to 1^2 per crop, so the GEMM's rows are M = B Hout Wout pixels of ALL crops; Cout is a multiple of 16.
// As in kernels_cond.hip the CHANNELS sit on the MFMA's row side (A = weights straight from the [Cout][ks ks Cin] K-major matrix: 8 consecutive k of a
// lane are one 16-byte load) and 16 pixels on its column side (B = activations: 8 consecutive channels of one tap of the lane's pixel, one 16-byte load,
// zero where the tap is outside the map).  A lane's accumulator is 4 consecutive channels of ONE pixel: an 8-byte NHWC store.
// K = ks ks Cin runs in steps of 32 = four 8-channel chunks in the fixed order k = tap Cin + c (Cin % 8 == 0: a chunk never straddles a tap; the chunks
// past K in the last step are zero on both sides).  No split-K, and neither the tile (NT channel tiles x MT pixel groups per wave, picked from M and N)
// nor the batch changes which products a sum holds or their order: a crop's outputs are bit for bit those it has alone (ldiff.h, ldiff_resnet).
// A wave owns 16 MT pixels x 16 NT channels, a workgroup four such pixel ranges of the same channels; operands come from L1 / L2 (the matrices and the
// maps of a layer are re-read by neighbouring waves), the next step's fragments are in flight while the current step's MFMAs issue.  No LDS.
#include "common.h"

namespace {

template <int KS, int NT, int MT, bool BN>
__global__ __launch_bounds__(256) void clsconv_kernel(const ConvParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, j = lane >> 4;
  const int C8 = p.C1 >> 3, KCH = KS * KS * C8, KSTEPS = (KCH + 3) >> 2;
  const int ld = p.ld1 ? p.ld1 : p.C1;
  const int n0 = blockIdx.y * NT * 16;
  const int m0 = (blockIdx.x * 4 + wave) * (MT * 16);
  const int hw = p.Hout * p.Wout;

  const f16* xim[MT];   // the image of this lane's pixel of group m, and the pixel's top-left tap
  int iy0[MT], ix0[MT];
  bool mval[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mm = m0 + m * 16 + l15;
    mval[m] = mm < p.M;
    const int mc = mval[m] ? mm : 0, b = mc / hw, r = mc - b * hw, oy = r / p.Wout, ox = r - oy * p.Wout;
    iy0[m] = oy * p.stride - KS / 2;
    ix0[m] = ox * p.stride - KS / 2;
    xim[m] = p.x + (long long)b * p.Hin * p.Win * ld;
  }
  const f16* wrow = p.w + (long long)(n0 + l15) * p.K;   // row n0 + 16 a + l15 of the weight matrix

  int tap = j / C8, c8 = j - tap * C8;   // this lane's chunk q = 4 kk + j of the step being LOADED: tap and 8-channel group
  auto load_step = [&](int kk, f16x8 (&af)[NT], f16x8 (&bf)[MT]) {
    const int q = kk * 4 + j;
    const bool valid = q < KCH;
    const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (valid) v = *reinterpret_cast<const f16x8*>(wrow + (long long)a * 16 * p.K + (long long)q * 8);
      af[a] = v;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int iy = iy0[m] + ky, ix = ix0[m] + kx;
      f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (valid && mval[m] && iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) v = *reinterpret_cast<const f16x8*>(xim[m] + ((long long)iy * p.Win + ix) * ld + c8 * 8);
      bf[m] = v;
    }
    c8 += 4;
    while (c8 >= C8) { c8 -= C8; ++tap; }
  };

  f32x4 acc[NT][MT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[a][m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  f16x8 a_cur[NT], b_cur[MT], a_nxt[NT], b_nxt[MT];
  load_step(0, a_cur, b_cur);
#pragma unroll 1
  for (int kk = 0; kk < KSTEPS; ++kk) {
    if (kk + 1 < KSTEPS) load_step(kk + 1, a_nxt, b_nxt);
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_cur[a], b_cur[m], acc[a][m], 0, 0, 0);
#pragma unroll
    for (int a = 0; a < NT; ++a) a_cur[a] = a_nxt[a];
#pragma unroll
    for (int m = 0; m < MT; ++m) b_cur[m] = b_nxt[m];
  }

  // epilogue in fp32: v = sum + bias (+ res), the non-finite test BEFORE the ReLU (v > 0 ? v : 0 turns a NaN into 0), ReLU, one fp16 rounding;
  // lane = pixel l15 of its group, channels n0 + 16 a + 4 j .. + 3
  f16* y = reinterpret_cast<f16*>(p.y);
  bool bad = false;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if (!mval[m]) continue;
    const long long mm = m0 + m * 16 + l15;
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const int ch = n0 + 16 * a + 4 * j;
      f32x4 v = acc[a][m];
      if (p.bias) {
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + ch);
        v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
      }
      if (p.res) {
        const f16x4 rv = *reinterpret_cast<const f16x4*>(p.res + mm * p.ld_res + ch);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!(__builtin_fabsf(v[r]) <= 65504.f)) bad = true;   // (a NaN fails the comparison)
        if (p.relu_out) v[r] = v[r] > 0.f ? v[r] : 0.f;
      }
      *reinterpret_cast<f16x4*>(y + mm * p.ldy + ch) = cvt4(v);
    }
  }
  if (bad && p.nonfinite) *p.nonfinite = 1;   // sticky flag of the owning handle (host-mapped; include/ldiff.h "Non-finite detection")
  // Training-mode BatchNorm partials (BN launches carry no bias, residual or ReLU: acc IS the raw value): per wave = row block r = 4 blockIdx.x + wave and channel the
  // float2 {sum v, sum v^2} of the FP32 accumulators over the block's valid rows, at bn_stats[(n R + r) 2], R = 4 gridDim.x.  A wave past M stores zeros; no atomics.
  // Association (wave_stats_store): a lane adds its MT pixels in index order into a zero (the squares by fma), then row16_sum's fixed butterfly over the 16 pixel lanes
  // (quad xor 1, quad xor 2, half mirror, mirror), so every launch gives the same bits.
  // LONGEST CHAIN of fp32 additions into one partial: L = MT + 4 <= 8 (4 pixels of a lane + 4 butterfly steps).
  if constexpr (BN) {
    const long long R = 4ll * gridDim.x, rblk = (long long)blockIdx.x * 4 + wave;
    wave_stats_store<MT, NT>(acc, mval, 0, MT, p.bn_stats + rblk * 2, R, p.N, n0 + 4 * j, l15);
  }
}

template <int KS, int NT, int MT>
void launch_tile(const ConvParams& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.M + 64 * MT - 1) / (64 * MT)), (unsigned)(p.N / (16 * NT)));
  static const std::string base = "clsconv<" + std::to_string(KS) + "x" + std::to_string(KS) + "," + std::to_string(16 * NT) + "x" + std::to_string(16 * MT);
  static const std::string name_plain = base + ">", name_relu = base + ",relu>", name_bn = base + ",bn>";
  const double bytes = (double)p.B * p.Hin * p.Win * p.C1 * 2.0 + (double)p.N * p.K * 2.0 + (double)p.M * p.N * (p.res ? 4.0 : 2.0);
  ProfScope prof(p.bn_stats ? name_bn.c_str() : p.relu_out ? name_relu.c_str() : name_plain.c_str(), 2.0 * p.M * (double)p.N * p.K, bytes, s);
  if (p.bn_stats) clsconv_kernel<KS, NT, MT, true><<<grid, 256, 0, s>>>(p);
  else clsconv_kernel<KS, NT, MT, false><<<grid, 256, 0, s>>>(p);
  HIP_CHECK(hipGetLastError());
}
// the tile: 64 channels per workgroup where Cout has them; 64 pixels per wave where such workgroups still cover the chip twice
struct ClsTile { bool nt4, mt4; };
ClsTile cls_tile(const ConvParams& p) {
  const bool nt4 = p.N % 64 == 0;
  const long long wgs4 = (long long)((p.M + 255) / 256) * (p.N / (nt4 ? 64 : 16));
  return ClsTile{nt4, wgs4 >= 512};
}
template <int KS>
void launch_ks(const ConvParams& p, hipStream_t s) {
  const ClsTile t = cls_tile(p);
  if (t.nt4) { if (t.mt4) launch_tile<KS, 4, 4>(p, s); else launch_tile<KS, 4, 1>(p, s); }
  else { if (t.mt4) launch_tile<KS, 1, 4>(p, s); else launch_tile<KS, 1, 1>(p, s); }
}

// ---- 3x3 stride-2 max pooling, padding 1 (taps outside the map are ignored), NHWC fp16; a thread = 8 channels of one output pixel ----
__global__ void maxpool3x3s2_kernel(const f16* __restrict__ x, f16* __restrict__ y, int B, int H, int W, int C, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C8 = C >> 3;
  if (i >= (long long)B * Ho * Wo * C8) return;
  const int c8 = (int)(i % C8);
  const long long pix = i / C8;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((long long)Wo * Ho));
  f16x8 m;
  bool first = true;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      const f16x8 v = *reinterpret_cast<const f16x8*>(x + (((long long)b * H + iy) * W + ix) * C + c8 * 8);
      if (first) { m = v; first = false; continue; }
#pragma unroll
      for (int r = 0; r < 8; ++r) m[r] = (v[r] > m[r] || v[r] != v[r]) ? v[r] : m[r];   // (a NaN propagates, as in torch)
    }
  }
  *reinterpret_cast<f16x8*>(y + pix * C + c8 * 8) = m;   // (the centre tap 2 oy, 2 ox is always inside the map)
}

// ---- crops -> classifier input ----
// The weights of one output coordinate along one axis, as torch's anti-aliased bilinear resize computes them (aten UpSampleKernel / PIL's resample):
// scale = in / out, support = max(scale, 1), the triangle filter stretched by it, taps [lo, lo + n) normalised to sum 1.  For in <= out the two
// taps and weights are those of plain bilinear resampling with align_corners = False.
// The filter runs in DOUBLE: the normalisation (v - mean) / std cancels where v is near the mean, and fp32 sums of a dozen taps then miss the
// one-fp16-ulp contract by several ulps around zero (measured: 4.8); the launch is a few thousand threads per crop, its cost does not show.
struct AxisTaps { int lo, n; double center, inv, total; };
__device__ __forceinline__ double tri_w(const AxisTaps& t, int k) {
  const double d = ((double)(k + t.lo) - t.center + 0.5) * t.inv;
  const double w = 1.0 - __builtin_fabs(d);
  return w > 0.0 ? w : 0.0;
}
__device__ __forceinline__ AxisTaps axis_taps(int o, int in, int out) {
  AxisTaps t;
  const double scale = (double)in / (double)out, support = scale >= 1.0 ? scale : 1.0;
  t.inv = scale >= 1.0 ? 1.0 / scale : 1.0;
  t.center = scale * ((double)o + 0.5);
  const int lo = (int)(t.center - support + 0.5), hi = (int)(t.center + support + 0.5);
  t.lo = lo > 0 ? lo : 0;
  t.n = (hi < in ? hi : in) - t.lo;
  t.total = 0.0;
  for (int k = 0; k < t.n; ++k) t.total += tri_w(t, k);
  return t;
}
struct Norm3 { double mean[3], std[3]; };
__global__ void crop_resize_norm_kernel(const uint8_t* __restrict__ rgb, int H, int W, const int* __restrict__ boxes, int n, const uint8_t* __restrict__ lut, int S,
                                        const Norm3 nm, f16* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * S * S) return;
  const int ox = (int)(i % S), oy = (int)((i / S) % S), b = (int)(i / ((long long)S * S));
  const int x1 = boxes[4 * b], y1 = boxes[4 * b + 1], x2 = boxes[4 * b + 2], y2 = boxes[4 * b + 3];
  const int cw = x2 - x1 + 1, ch = y2 - y1 + 1;
  f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
  if (cw >= 1 && ch >= 1 && x1 >= 0 && y1 >= 0 && x2 < W && y2 < H) {   // (a box outside the image yields a zero crop; nothing outside the image is read)
    const AxisTaps ty = axis_taps(oy, ch, S), tx = axis_taps(ox, cw, S);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int ky = 0; ky < ty.n; ++ky) {
      const double wy = tri_w(ty, ky) / ty.total;
      const uint8_t* row = rgb + ((long long)(y1 + ty.lo + ky) * W + x1 + tx.lo) * 3;
      double racc[3] = {0.0, 0.0, 0.0};
      for (int kx = 0; kx < tx.n; ++kx) {
        const double wx = tri_w(tx, kx) / tx.total;
#pragma unroll
        for (int c = 0; c < 3; ++c) racc[c] += wx * ((double)lut[c * 256 + row[3 * kx + c]] / 255.0);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += wy * racc[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (f16)((acc[c] - nm.mean[c]) / nm.std[c]);
  }
  *reinterpret_cast<f16x8*>(out + i * 8) = o;
}

// ---- head: a wave per instance.  feat[c] = mean over the HW pixels of the adapter's map (fp32 sum of the fp16 values), logits = W feat + b in fp32 ----
__global__ __launch_bounds__(64) void cls_head_kernel(const f16* __restrict__ x, int HW, int A, int ldx, const float* __restrict__ w, const float* __restrict__ bias, int C,
                                                      float* __restrict__ logits, int* __restrict__ labels, float* __restrict__ feat_out) {
  extern __shared__ float feat[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const f16* xb = x + (long long)b * HW * ldx;
  const float inv = 1.0f / (float)HW;
  for (int c = lane; c < A; c += 64) {
    float sum = 0.f;
    for (int i = 0; i < HW; ++i) sum += (float)xb[(long long)i * ldx + c];
    feat[c] = sum * inv;
    if (feat_out) feat_out[(long long)b * A + c] = feat[c];
  }
  __syncthreads();
  float best = 0.f;
  int arg = 0;
  for (int k = 0; k < C; ++k) {
    float part = 0.f;
    for (int c = lane; c < A; c += 64) part = __builtin_fmaf(feat[c], w[(long long)k * A + c], part);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    const float v = part + bias[k];
    if (lane == 0 && logits) logits[(long long)b * C + k] = v;
    if (k >= 1 && (arg == 0 || v > best)) { best = v; arg = k; }   // first maximum among the classes 1 .. C - 1 (softmax is monotonic: the reference's top-1 of softmax[:, 1:])
  }
  if (lane == 0 && labels) labels[b] = arg;
}

}  // namespace

// The launches clsconv takes: ks 1 | 3 | 7 with padding ks / 2 on every side, stride 1 | 2, one plain fp16 source with C1 % 8 == 0, Cout % 16 == 0,
// bias / plain fp16 residual / ReLU behind the sum, plain fp16 output.  Of those the executors' choice (ConvParams::cls_force = 0) is the ones
// that ask for relu_out -- no launch that existed before this kernel changes its route; cls_force = 1 takes every eligible launch (the classifier's own convs
// without a ReLU: downsample, adapter; tests), -1 none.
static bool cls_conv_eligible(const ConvParams& p) {
  if ((p.ks != 1 && p.ks != 3 && p.ks != 7) || (p.stride != 1 && p.stride != 2) || p.pad_t != p.ks / 2 || p.pad_l != p.ks / 2) return false;
  if (p.ups || p.x2 || p.C2 || p.gn_scale || p.gn_shift || p.silu_in || p.lrelu_in || p.temb || p.res_lo || p.out_f32 || p.y_lo || p.geglu || p.stats || p.splitk > 1 || p.lo8_slab0 ||
      p.xs || p.w_par || p.w_bstride || p.out_shift || p.silu_out || p.tconv || p.post_img || p.post_rgb || p.post_luma)
    return false;
  if (p.c3d_ups > 0 || p.df_force > 0 || p.Cs || p.temb || p.lo8_sa) return false;   // requests for another kernel's form: never dropped silently
  if (!p.x || !p.w || !p.y) return false;
  // 16-byte operand loads, float4 bias loads, 8-byte residual loads and output stores
  if (((uintptr_t)p.x & 15) || ((uintptr_t)p.w & 15) || ((uintptr_t)p.bias & 15) || ((uintptr_t)p.res & 7) || ((uintptr_t)p.y & 7)) return false;
  const int ld = p.ld1 ? p.ld1 : p.C1;
  if (p.C1 < 8 || p.C1 % 8 != 0 || ld < p.C1 || ld % 8 != 0 || p.K != p.ks * p.ks * p.C1) return false;
  if (p.N < 16 || p.N % 16 != 0 || p.N > p.Nrows || p.ldy < p.N || p.ldy % 4 != 0) return false;
  if (p.res && (p.ld_res < p.N || p.ld_res % 4 != 0)) return false;
  if (p.B < 1 || p.Hin < 1 || p.Win < 1 || p.Hout != (p.Hin - 1) / p.stride + 1 || p.Wout != (p.Win - 1) / p.stride + 1) return false;
  if ((long long)p.B * p.Hout * p.Wout != p.M) return false;
  return true;
}
bool cls_conv_selected(const ConvParams& p) {
  if (p.cls_force < 0 || (p.cls_force == 0 && !p.relu_out)) return false;
  return cls_conv_eligible(p);
}
bool cls_conv_bn_ok(const ConvParams& p) {
  return p.bn_stats && p.cls_force > 0 && !p.bias && !p.res && !p.relu_out && ((uintptr_t)p.bn_stats & 7) == 0 && cls_conv_eligible(p);
}
int cls_conv_bn_stats_blocks(const ConvParams& p) { return 4 * ((p.M + (cls_tile(p).mt4 ? 256 : 64) - 1) / (cls_tile(p).mt4 ? 256 : 64)); }
void launch_cls_conv(const ConvParams& p, hipStream_t s) {
  LDIFF_CHECK(cls_conv_eligible(p), LDIFF_ERR_INVALID, "clsconv: not a launch of the classifier's conv family (ks=%d stride=%d Cin=%d N=%d)", p.ks, p.stride, p.C1, p.N);
  LDIFF_CHECK(!p.bn_stats || cls_conv_bn_ok(p), LDIFF_ERR_INVALID, "clsconv: bn_stats needs cls_conv = 1 and a launch without bias, residual and ReLU");
  if (p.ks == 1) launch_ks<1>(p, s);
  else if (p.ks == 3) launch_ks<3>(p, s);
  else launch_ks<7>(p, s);
}

void launch_maxpool3x3s2(const f16* x, f16* y, int B, int H, int W, int C, hipStream_t s) {
  LDIFF_CHECK(x && y && B >= 1 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0, LDIFF_ERR_INVALID, "maxpool3x3s2: null pointer, empty shape or C = %d not a multiple of 8", C);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long n = (long long)B * Ho * Wo * (C / 8);
  maxpool3x3s2_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(x, y, B, H, W, C, Ho, Wo);
  HIP_CHECK(hipGetLastError());
}

void launch_crop_resize_norm(const uint8_t* rgb, int H, int W, const int* boxes, int n, const uint8_t* lut, int S, const double* mean3, const double* std3, f16* out, hipStream_t s) {
  LDIFF_CHECK(rgb && boxes && lut && out && mean3 && std3 && H >= 1 && W >= 1 && n >= 1 && S >= 1 && S <= 4096, LDIFF_ERR_INVALID, "crop_resize_norm: null pointer or empty shape");
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    LDIFF_CHECK(std3[c] > 0.0, LDIFF_ERR_INVALID, "crop_resize_norm: std[%d] must be positive", c);
    nm.mean[c] = mean3[c]; nm.std[c] = std3[c];
  }
  const long long total = (long long)n * S * S;
  crop_resize_norm_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(rgb, H, W, boxes, n, lut, S, nm, out);
  HIP_CHECK(hipGetLastError());
}

void launch_cls_head(const f16* x, int B, int HW, int A, int ldx, const float* w, const float* bias, int C, float* logits, int* labels, hipStream_t s) {
  LDIFF_CHECK(x && w && bias && logits && B >= 1 && HW >= 1 && A >= 1 && A <= 8192 && ldx >= A && C >= 2, LDIFF_ERR_INVALID,
              "cls_head: null pointer, empty shape, more than 8192 features or fewer than 2 classes (A=%d C=%d)", A, C);
  cls_head_kernel<<<(unsigned)B, 64, (size_t)A * sizeof(float), s>>>(x, HW, A, ldx, w, bias, C, logits, labels, nullptr);
  HIP_CHECK(hipGetLastError());
}
void launch_cls_head_feat(const f16* x, int B, int HW, int A, int ldx, const float* w, const float* bias, int C, float* logits, int* labels, float* feat, hipStream_t s) {
  LDIFF_CHECK(x && w && bias && B >= 1 && HW >= 1 && A >= 1 && A <= 8192 && ldx >= A && C >= 2, LDIFF_ERR_INVALID,
              "cls_head_feat: null pointer, empty shape, more than 8192 features or fewer than 2 classes (A=%d C=%d)", A, C);
  cls_head_kernel<<<(unsigned)B, 64, (size_t)A * sizeof(float), s>>>(x, HW, A, ldx, w, bias, C, logits, labels, feat);
  HIP_CHECK(hipGetLastError());
}
