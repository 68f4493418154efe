// Kernels of the nnU-Net tissue head (ldiff_segnet: PlainConvUNet, 2-D) that no other family is made for.
//   segconv<...>    the narrow 3x3 convs (Cin 8 | 32 | 32 + 32, Cout 32 | 64, stride 1 | 2) with the InstanceNorm + LeakyReLU prologue on either source and fused
//                   statistics of the fp32 sums; described at the kernel.
//   tconv2x2<...>   ConvTranspose2d with kernel = stride = 2 (decoder.transpconvs.j; /root/reference/segmentor.py:463-488 reaches it through nnUNetPredictor's
//                   network): every coarse pixel produces a 2x2 block of the fine map and no two coarse pixels share an output pixel, so the layer is ONE
//                   GEMM over the coarse map, y4[m, q * N + n] = sum_c a[m, c] * w[q][n][c] with q = dy * 2 + dx, whose epilogue scatters column block q of row
//                   m = (b, iy, ix) to pixel (b, 2 iy + dy, 2 ix + dx) and adds the bias once per output pixel.  The operand is the RAW output of the stage below:
//                   its InstanceNorm + LeakyReLU(0.01) are applied on the way into LDS (one fp16 rounding), as the igemm_lrelu prologue does.
//   in_finalize     per-(image, channel) scale = gamma * rstd, shift = beta - mean * scale from the producer's fused partial sums (or, where the producer
//                   emitted none, from the tensor itself): InstanceNorm is GroupNorm with one channel per group, and the GroupNorm finalize spends a
//                   workgroup per group; here a wave takes a channel, four channels per workgroup.  Writes into a row of `ld_ss` entries at column `ss_off`, and
//                   identity entries for the `ident` channels in front: the scale / shift of cat((upsampled, skip), 1) without a concat of anything.
//   nhwc_f32_to_nchw  the logits' layout cast, fp32 or fp16 output.
// Tiling of tconv2x2 as the register-staged implicit GEMM's (kernels_igemm.hip): 64 coarse pixels x 64 columns x 64 K per 256-thread workgroup, C^T accumulators so
// that a lane holds 4 consecutive output channels of one pixel (8-byte stores), XOR-swizzled 128-byte LDS rows, double buffered, one barrier per K step.
#include "lds_prims.h"

namespace {

constexpr int TBK = 64, TCPR = TBK / 8, TBM = 64, TBN = 64;

// IN: the operand carries an InstanceNorm (+ LeakyReLU where lrelu_in bit 0 is set) prologue
template <bool IN>
__global__ __launch_bounds__(256, 2) void tconv2x2_kernel(const ConvParams p) {
  constexpr int A_IT = TBM * TCPR / 256, B_IT = TBN * TCPR / 256;   // 2, 2
  __shared__ __attribute__((aligned(16))) uint4 sA[2][TBM * TCPR];
  __shared__ __attribute__((aligned(16))) uint4 sB[2][TBN * TCPR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_m = wave >> 1, wave_n = wave & 1;
  const int C = p.C1, ld = p.ld1 ? p.ld1 : p.C1;
  const int N4 = 4 * p.N;
  const int Mc = p.B * p.Hin * p.Win;   // coarse pixels = GEMM rows
  const int ntn = N4 / TBN + (N4 % TBN != 0);
  const int m0 = (blockIdx.x / ntn) * TBM, n0 = (blockIdx.x % ntn) * TBN;   // the n-tiles of one m-tile are neighbours: the activation rows stay in L2
  const int kc = tid & (TCPR - 1);
  const float slope = (p.lrelu_in & 1) ? 0.01f : 1.0f;
  const int HWi = p.Hin * p.Win;

  uint4 ra[A_IT], rw[B_IT];
  int gidx[A_IT];

  auto load_tiles = [&](int kt) {
    const int k0 = kt * TBK + kc * 8;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int m = m0 + (tid >> 3) + i * 32;
      uint4 v = make_uint4(0, 0, 0, 0);
      gidx[i] = -1;
      if (m < Mc && k0 < C) {
        v = *reinterpret_cast<const uint4*>(p.x + (long long)m * ld + k0);
        gidx[i] = (m / HWi) * C + k0;
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int n = n0 + (tid >> 3) + i * 32;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (n < N4 && k0 < C) v = *reinterpret_cast<const uint4*>(p.w + (long long)n * C + k0);
      rw[i] = v;
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int row = (tid >> 3) + i * 32;
      uint4 v = ra[i];
      if (IN) { if (gidx[i] >= 0) v = in_lrelu_apply8(v, p.gn_scale + gidx[i], p.gn_shift + gidx[i], slope); }
      sA[buf][row * TCPR + swz8(row, kc)] = v;
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int row = (tid >> 3) + i * 32;
      sB[buf][row * TCPR + swz8(row, kc)] = rw[i];
    }
  };

  f32x4 acc[2][2];   // [n tile][m tile] of the wave's 32 x 32
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = (C + TBK - 1) / TBK;
  const int g = lane >> 4, l15 = lane & 15;
  load_tiles(0);
  store_tiles(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tiles(kt + 1);
#pragma unroll
    for (int kk = 0; kk < TBK / 32; ++kk) {
      f16x8 wf[2], xf[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int row = wave_n * 32 + a * 16 + l15;
        wf[a] = __builtin_bit_cast(f16x8, sB[cur][row * TCPR + swz8(row, kk * 4 + g)]);
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int row = wave_m * 32 + b * 16 + l15;
        xf[b] = __builtin_bit_cast(f16x8, sA[cur][row * TCPR + swz8(row, kk * 4 + g)]);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[a], xf[b], acc[a][b], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tiles(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: the lane holds y4[m = tile column l15][n4 = 4 g + r]; N % 16 == 0, so a 16-column tile lies inside one tap q ----
  f16* y = reinterpret_cast<f16*>(p.y);
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int n4 = n0 + wave_n * 32 + a * 16 + g * 4;
    if (n4 >= N4) continue;
    const int q = n4 / p.N, n = n4 - q * p.N;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) bv = *reinterpret_cast<const float4*>(p.bias + n);
    const f32x4 bb = (f32x4){bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int m = m0 + wave_m * 32 + b * 16 + l15;
      if (m >= Mc) continue;
      const int bi = m / HWi, rem = m - bi * HWi;
      const int iy = rem / p.Win, ix = rem - iy * p.Win;
      const long long pix = ((long long)bi * p.Hout + 2 * iy + (q >> 1)) * p.Wout + 2 * ix + (q & 1);
      *reinterpret_cast<f16x4*>(y + pix * p.ldy + n) = cvt4(acc[a][b] + bb);
    }
  }
}

// ---- segconv<...>: the narrow 3x3 convs of the full- and half-resolution stages --------------------------------------------------------------
// Cin (both sources together) 8 | 32 | 64, Cout 32 | 64, stride 1 | 2, padding 1.  These maps hold most of the network's bytes and the layers are
// bandwidth-bound (32 -> 32 at 512^2: 4.8 GFLOP against 33.6 MB), so: the halo tile of input pixels is read ONCE per workgroup (all output channels
// in one workgroup: no second column block re-reads it), InstanceNorm + LeakyReLU are applied on the way into LDS (one fp16 rounding; outside the
// image the tile is zero: the padding is of the activated tensor), every output pixel is stored as whole lines, and the InstanceNorm partial sums of
// the output come from the fp32 accumulators (a value that rounds to +-inf in fp16 counts as NaN, so that the finalize kernel flags it).
// MFMA arrangement as the conditioning-embedding kernel's (kernels_cond.hip): channels on the row side (A = weights from the K-major matrix, L1 / L2
// resident: 4.6 - 73 KB), 16 consecutive pixels of an output row on the column side (B = the LDS halo), K = 9 Cin in steps of 32.
// Statistics row blocks: one per wave, r = (ty * tiles_x + tx) * 4 + wave, R = 4 tiles_x tiles_y (segconv_stats_blocks).
constexpr int STW = 32;
constexpr int seg_th(int stride) { return stride == 2 ? 4 : 8; }
constexpr int seg_smem(int cin, int stride) { return ((seg_th(stride) - 1) * stride + 3) * ((STW - 1) * stride + 3) * (cin + 8) * (int)sizeof(f16); }

template <int CIN, int NT, int STRIDE, bool PRO>
__global__ __launch_bounds__(256) void segconv_kernel(const ConvParams p, const int tiles_x, const int tiles_y) {
  constexpr int TH = seg_th(STRIDE), RPW = TH / 4, MT = 2 * RPW;
  constexpr int HH = (TH - 1) * STRIDE + 3, HWD = (STW - 1) * STRIDE + 3, PITCH = CIN + 8;
  constexpr int C8 = CIN / 8, KCH = 9 * C8, KS = (KCH + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) f16 halo[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, j = lane >> 4;
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const int ld1 = p.ld1 ? p.ld1 : p.C1, ld2 = p.ld2 ? p.ld2 : p.C2;

  const int iy0 = ty * TH * STRIDE - 1, ix0 = tx * STW * STRIDE - 1;
  const long long img = (long long)b * p.Hin * p.Win;
  for (int idx = tid; idx < HH * HWD * C8; idx += 256) {
    const int pix = idx / C8, c8 = idx - pix * C8, hy = pix / HWD, hx = pix - hy * HWD;
    const int iy = iy0 + hy, ix = ix0 + hx, c = c8 * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) {
      const long long at = img + (long long)iy * p.Win + ix;
      const bool first = c < p.C1;
      v = first ? *reinterpret_cast<const uint4*>(p.x + at * ld1 + c) : *reinterpret_cast<const uint4*>(p.x2 + at * ld2 + (c - p.C1));
      if (PRO) v = in_lrelu_apply8(v, p.gn_scale + b * CIN + c, p.gn_shift + b * CIN + c, ((first ? p.lrelu_in : p.lrelu_in >> 1) & 1) ? 0.01f : 1.0f);
    }
    *reinterpret_cast<uint4*>(halo + pix * PITCH + c) = v;
  }
  __syncthreads();

  int pbase[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) pbase[m] = ((wave * RPW + m / 2) * STRIDE * HWD + ((m & 1) * 16 + l15) * STRIDE) * PITCH;

  const f16* wrow = p.w + (long long)l15 * p.K;
  auto load_a = [&](int kk, f16x8 (&af)[NT]) {
    const int q = kk * 4 + j;
    const bool valid = q < KCH;
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (valid) v = *reinterpret_cast<const f16x8*>(wrow + (long long)a * 16 * p.K + q * 8);
      af[a] = v;
    }
  };

  f32x4 acc[NT][MT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[a][m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  f16x8 a_cur[NT], a_nxt[NT];
  load_a(0, a_cur);
#pragma unroll 1
  for (int kk = 0; kk < KS; ++kk) {
    if (kk + 1 < KS) load_a(kk + 1, a_nxt);
    const int q = kk * 4 + j;
    const bool valid = q < KCH;
    const int qc = valid ? q : 0;
    const int tap = qc / C8, c0 = (qc - tap * C8) * 8, ky = tap / 3, kx = tap - 3 * ky;
    const int koff = (ky * HWD + kx) * PITCH + c0;
    f16x8 bf[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (valid) v = *reinterpret_cast<const f16x8*>(halo + pbase[m] + koff);
      bf[m] = v;
    }
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_cur[a], bf[m], acc[a][m], 0, 0, 0);
#pragma unroll
    for (int a = 0; a < NT; ++a) a_cur[a] = a_nxt[a];
  }

  // epilogue: + bias, one fp16 rounding; the lane holds pixel l15 of its group, channels 16 a + 4 j .. + 3: the NT tiles and the four j complete the pixel's line
  f16* yb = reinterpret_cast<f16*>(p.y) + (long long)b * p.Hout * p.Wout * p.ldy;
  bool ok[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int oy = ty * TH + wave * RPW + m / 2, ox = tx * STW + (m & 1) * 16 + l15;
    ok[m] = oy < p.Hout && ox < p.Wout;
    f16* yp = yb + ((long long)oy * p.Wout + ox) * p.ldy;
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const int ch = 16 * a + 4 * j;
      f32x4 v = acc[a][m];
      if (p.bias) {
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + ch);
        v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
      }
      if (ok[m]) *reinterpret_cast<f16x4*>(yp + ch) = cvt4(v);
      acc[a][m] = split_stat4(v);   // the statistics' operand: the fp32 value
    }
  }
  if (p.stats) {
    const long long R = p.stats_R, rblk = (long long)(ty * tiles_x + tx) * 4 + wave;
    wave_stats_store<MT, NT>(acc, ok, 0, MT, p.stats + ((long long)b * p.N * R + rblk) * 2, R, p.N, 4 * j, l15);
  }
}

template <int CIN, int COUT, int STRIDE>
void launch_segconv_shape(const ConvParams& p, hipStream_t s) {
  constexpr int NT = COUT / 16, TH = seg_th(STRIDE), SMEM = seg_smem(CIN, STRIDE);
  static_assert(SMEM <= 64 * 1024, "segconv: the halo tile must leave room for two workgroups per CU");
  const int tiles_x = (p.Wout + STW - 1) / STW, tiles_y = (p.Hout + TH - 1) / TH;
  const dim3 grid((unsigned)(tiles_x * tiles_y * p.B));
  const double bytes = (double)p.B * p.Hin * p.Win * CIN * 2.0 + (double)COUT * p.K * 2.0 + (double)p.M * COUT * 2.0;
  static const std::string base = "segconv<" + std::to_string(CIN) + "x" + std::to_string(COUT) + ",s" + std::to_string(STRIDE);
  static const std::string name_plain = base + ">", name_pro = base + ",in>";
  const bool pro = p.gn_scale != nullptr;
  ProfScope prof(pro ? name_pro.c_str() : name_plain.c_str(), 2.0 * p.M * (double)COUT * p.K, bytes, s);
  if (pro) {
    ensure_dyn_smem(reinterpret_cast<const void*>(segconv_kernel<CIN, NT, STRIDE, true>), SMEM);
    segconv_kernel<CIN, NT, STRIDE, true><<<grid, 256, SMEM, s>>>(p, tiles_x, tiles_y);
  } else {
    ensure_dyn_smem(reinterpret_cast<const void*>(segconv_kernel<CIN, NT, STRIDE, false>), SMEM);
    segconv_kernel<CIN, NT, STRIDE, false><<<grid, 256, SMEM, s>>>(p, tiles_x, tiles_y);
  }
  HIP_CHECK(hipGetLastError());
}

bool segconv_eligible(const ConvParams& p) {
  if (p.ks != 3 || p.pad_t != 1 || p.pad_l != 1 || p.ups || (p.stride != 1 && p.stride != 2) || p.temb || p.res || p.out_f32 || p.y_lo || p.geglu || p.splitk > 1 ||
      p.lo8_slab0 || p.xs || p.w_par || p.w_bstride || p.out_shift || p.post_img || p.post_rgb || p.post_luma || p.silu_in || p.silu_out || p.tconv)
    return false;
  const int Cin = p.C1 + p.C2;
  if ((Cin != 8 && Cin != 32 && Cin != 64) || (Cin == 64 && p.stride == 2) /* an 84 KB halo: no layer of the network has it */ || (p.N != 32 && p.N != 64) || p.N > p.Nrows || p.K != 9 * Cin || p.ldy < p.N || p.ldy % 4 != 0) return false;
  if (p.C1 % 8 != 0 || p.C2 % 8 != 0 || (p.C2 == 0) != (p.x2 == nullptr) || ((p.ld1 ? p.ld1 : p.C1) & 7) != 0 || ((p.ld2 ? p.ld2 : p.C2) & 7) != 0) return false;
  if ((p.gn_scale == nullptr) != (p.gn_shift == nullptr) || (p.lrelu_in && !p.gn_scale)) return false;
  return p.Hout == (p.Hin - 1) / p.stride + 1 && p.Wout == (p.Win - 1) / p.stride + 1;
}

// One wave per (image, channel).  part != nullptr: R {sum, sum of squares} pairs, contiguous ([B][C][R][2], common.h); else the channel itself, HW strided reads
__global__ __launch_bounds__(256) void in_finalize_kernel(const float* __restrict__ part, int R, const f16* __restrict__ x, int ldx, int HW, int C, float eps,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ scale,
                                                          float* __restrict__ shift, int ld_ss, int ss_off, int ident, int* __restrict__ nonfinite) {
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, c = blockIdx.x * 4 + (tid >> 6);
  if (blockIdx.x == 0)
    for (int i = tid; i < ident; i += 256) { scale[(long long)b * ld_ss + i] = 1.0f; shift[(long long)b * ld_ss + i] = 0.0f; }
  if (c >= C) return;
  const float gm = gamma[c], bt = beta[c];
  double a = 0.0, q = 0.0;
  if (part) {
    const float2* base = reinterpret_cast<const float2*>(part + ((long long)b * C + c) * R * 2);
    int i = lane;
    for (; i + 192 < R; i += 256) {
      const float2 v0 = base[i], v1 = base[i + 64], v2 = base[i + 128], v3 = base[i + 192];
      a += (double)((v0.x + v1.x) + (v2.x + v3.x));
      q += (double)((v0.y + v1.y) + (v2.y + v3.y));
    }
    for (; i < R; i += 64) { const float2 v = base[i]; a += (double)v.x; q += (double)v.y; }
  } else {
    const f16* base = x + (long long)b * HW * ldx + c;
    for (int i = lane; i < HW; i += 64) { const float v = (float)base[(long long)i * ldx]; a += (double)v; q += (double)v * (double)v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); q += __shfl_xor(q, o); }
  if (lane == 0) {
    if (nonfinite && !(a > -1e300 && a < 1e300 && q < 1e300)) *nonfinite = 1;   // sticky non-finite flag of the handle (include/ldiff.h); NaN fails every comparison
    const double mean = a / (double)HW;
    double var = q / (double)HW - mean * mean;
    if (var < 0.0) var = 0.0;
    const float sc = gm * (float)(1.0 / sqrt(var + (double)eps));
    scale[(long long)b * ld_ss + ss_off + c] = sc;
    shift[(long long)b * ld_ss + ss_off + c] = bt - (float)mean * sc;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void nhwc_f32_to_nchw_kernel(const float* __restrict__ x, T* __restrict__ y, int C, long long HW, int ldx) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= HW) return;
  const float* src = x + ((long long)b * HW + i) * ldx;
  for (int c = 0; c < C; ++c) y[((long long)b * C + c) * HW + i] = (T)src[c];
}

}  // namespace

void launch_tconv2x2(const ConvParams& p, hipStream_t s) {
  const int Mc = p.B * p.Hin * p.Win, N4 = 4 * p.N;
  if (Mc <= 0) return;
  const int ntm = (Mc + TBM - 1) / TBM, ntn = (N4 + TBN - 1) / TBN;
  const bool in = p.gn_scale != nullptr;
  // each coarse pixel read once, each fine pixel written once, the weights once
  const double bytes = ((double)Mc * p.C1 + (double)N4 * p.C1 + (double)Mc * N4) * 2.0;
  ProfScope prof(in ? "tconv2x2<64,64,in>" : "tconv2x2<64,64>", 2.0 * Mc * (double)N4 * p.C1, bytes, s);
  if (in) hipLaunchKernelGGL(tconv2x2_kernel<true>, dim3(ntm * ntn), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(tconv2x2_kernel<false>, dim3(ntm * ntn), dim3(256), 0, s, p);
  HIP_CHECK(hipGetLastError());
}

// The launches the narrow kernel takes (ConvParams::seg_conv): 0 = those that carry the LeakyReLU prologue -- the head's own layers; a plain launch of such a shape goes
// where it always went --, 1 = every eligible launch (the head's first conv, which has no prologue; tests, timing), -1 = none (timing: the implicit-GEMM route)
bool segconv_selected(const ConvParams& p) {
  if (p.seg_conv < 0 || (p.seg_conv == 0 && !p.lrelu_in)) return false;
  return segconv_eligible(p);
}
int segconv_stats_blocks(const ConvParams& p) {
  return 4 * ((p.Wout + STW - 1) / STW) * ((p.Hout + seg_th(p.stride) - 1) / seg_th(p.stride));
}
void launch_segconv(const ConvParams& p, hipStream_t s) {
  LDIFF_CHECK(segconv_eligible(p), LDIFF_ERR_INVALID, "segconv: not a launch of the narrow 3x3 kernel (Cin=%d N=%d stride=%d)", p.C1 + p.C2, p.N, p.stride);
  if (p.M <= 0) return;
  switch ((p.C1 + p.C2) * 1000 + p.N * 10 + p.stride) {
    case 8 * 1000 + 32 * 10 + 1: launch_segconv_shape<8, 32, 1>(p, s); return;
    case 8 * 1000 + 32 * 10 + 2: launch_segconv_shape<8, 32, 2>(p, s); return;
    case 8 * 1000 + 64 * 10 + 1: launch_segconv_shape<8, 64, 1>(p, s); return;
    case 8 * 1000 + 64 * 10 + 2: launch_segconv_shape<8, 64, 2>(p, s); return;
    case 32 * 1000 + 32 * 10 + 1: launch_segconv_shape<32, 32, 1>(p, s); return;
    case 32 * 1000 + 32 * 10 + 2: launch_segconv_shape<32, 32, 2>(p, s); return;
    case 32 * 1000 + 64 * 10 + 1: launch_segconv_shape<32, 64, 1>(p, s); return;
    case 32 * 1000 + 64 * 10 + 2: launch_segconv_shape<32, 64, 2>(p, s); return;
    case 64 * 1000 + 32 * 10 + 1: launch_segconv_shape<64, 32, 1>(p, s); return;
    case 64 * 1000 + 64 * 10 + 1: launch_segconv_shape<64, 64, 1>(p, s); return;
    default: break;
  }
  LDIFF_CHECK(false, LDIFF_ERR_INVALID, "segconv: no instantiation for Cin=%d N=%d stride=%d", p.C1 + p.C2, p.N, p.stride);
}

void launch_in_finalize(const float* part, int R, const f16* x, int ldx, int B, int HW, int C, float eps, const float* gamma, const float* beta, float* scale, float* shift,
                        int ld_ss, int ss_off, int ident, hipStream_t s, int* nonfinite) {
  LDIFF_CHECK((part != nullptr && R > 0) || x != nullptr, LDIFF_ERR_INVALID, "in_finalize: neither partial sums nor the tensor");
  if (B <= 0 || C <= 0) return;
  ProfScope prof("in_finalize", 0.0, part ? (double)B * C * R * 8.0 : (double)B * HW * C * 2.0, s);
  hipLaunchKernelGGL(in_finalize_kernel, dim3((C + 3) / 4, B), dim3(256), 0, s, part, R, x, ldx, HW, C, eps, gamma, beta, scale, shift, ld_ss, ss_off, ident, nonfinite);
  HIP_CHECK(hipGetLastError());
}

void launch_nhwc_f32_to_nchw(const float* x, void* y, int B, int C, int H, int W, int ldx, int out_f16, hipStream_t s) {
  const long long HW = (long long)H * W;
  if (B <= 0 || HW <= 0) return;
  const dim3 grid((unsigned)((HW + 255) / 256), B);
  if (out_f16) hipLaunchKernelGGL(nhwc_f32_to_nchw_kernel<f16>, grid, dim3(256), 0, s, x, reinterpret_cast<f16*>(y), C, HW, ldx);
  else hipLaunchKernelGGL(nhwc_f32_to_nchw_kernel<float>, grid, dim3(256), 0, s, x, reinterpret_cast<float*>(y), C, HW, ldx);
  HIP_CHECK(hipGetLastError());
}
