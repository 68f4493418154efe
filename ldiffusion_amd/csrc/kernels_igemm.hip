// Implicit-GEMM convolution / linear for gfx950 (MI355X): fp16 operands, fp32 accumulate on MFMA 16x16x32.
//
// One kernel family covers every contraction of the sampling path except attention:
//   conv3x3 (stride 1/2, symmetric or VAE-asymmetric padding, optional nearest-2x upsample gather,
//   optional two-source channel concat), conv1x1 and nn.Linear (ks=1), with
//   - GroupNorm-apply (+SiLU) folded into the A-tile load (statistics come from kernels_norm.hip),
//   - bias / per-(batch,channel) time-embedding / residual folded into the epilogue.
// Replaces the ATen conv2d / linear calls made inside diffusers' ResnetBlock2D, Transformer2DModel,
// Downsample2D, Upsample2D (reached from /root/reference/segmentor.py:103,526 and pixel_latent_vector.py:78,81).
//
// Layout: activations NHWC fp16 (channels % 8 == 0), weights [N][ky][kx][Cin] fp16 (K-major rows).
// Tiling: BM x BN x 64 per 256-thread workgroup (4 waves as 2x2), double-buffered LDS, register-staged
// loads issued before the MFMA phase and written to LDS after it (one barrier per K-step).
// The MFMA computes C^T (A-operand = weight rows, B-operand = activation rows) so that each lane ends up
// holding 4 consecutive output channels of one pixel -> 8-byte epilogue loads/stores.
// LDS rows are 128 B; 16-byte chunks are XOR-swizzled with (row>>1)&7, which makes every ds_read_b128
// lane group of the 16x16x32 operand fetch conflict-free (bank math in DESIGN.md).
#include "epilogue.h"
#include "lds_prims.h"

#define BK 64
#define CPR (BK / 8)  // 16-byte chunks per tile row

// x * sigmoid(x) with the two hardware transcendentals only (v_exp_f32, v_rcp_f32: 1 ulp); __frcp_rn would expand to a
// 11-instruction IEEE division per element

__device__ __forceinline__ uint4 gn_apply8(uint4 raw, const float* __restrict__ sc, const float* __restrict__ sh, int silu) {
  f16x8 h = __builtin_bit_cast(f16x8, raw);
  float4 s0 = *reinterpret_cast<const float4*>(sc), s1 = *reinterpret_cast<const float4*>(sc + 4);
  float4 t0 = *reinterpret_cast<const float4*>(sh), t1 = *reinterpret_cast<const float4*>(sh + 4);
  float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  float tv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = (float)h[j] * sv[j] + tv[j];
    const float vs = silu_f(v);
    v = silu ? vs : v;   // select, not a branch per element
    o[j] = (f16)v;
  }
  return __builtin_bit_cast(uint4, o);
}

// LR: the prologue's activation is LeakyReLU (igemm_lrelu_kernel below); the SiLU / plain instantiations do not see it
template <int BM, int BN, bool FAST, bool GN, bool LR>
__device__ __forceinline__ void igemm_body(const ConvParams& p) {
  constexpr int MT = BM / 32, NT = BN / 32;       // 16x16 tiles per wave along m / n (wave tile = BM/2 x BN/2)
  constexpr int A_IT = BM * CPR / 256, B_IT = BN * CPR / 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  uint4* sA = reinterpret_cast<uint4*>(smem_raw);              // [2][BM*CPR]
  uint4* sB = sA + 2 * BM * CPR;                               // [2][BN*CPR]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_m = wave >> 1, wave_n = wave & 1;
  const int Cin = p.C1 + p.C2;
  const int ntn = (p.N + BN - 1) / BN;

  // XCD-aware tile order: workgroups that share an XCD (blockIdx % 8) walk consecutive tiles, so the
  // n-tiles of one m-tile (same activation rows, all 9 taps) hit the same 4 MiB L2.
  int nwg = gridDim.x, id = blockIdx.x;
  int q8 = nwg >> 3, r8 = nwg & 7, xcd = id & 7, idx = id >> 3;
  int sw = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int m0 = (sw / ntn) * BM, n0 = (sw % ntn) * BN;

  // ---- per-thread A rows (fixed over the K loop) ----
  const int kc = tid & (CPR - 1);
  int rb[A_IT], ry[A_IT], rx[A_IT];
  const int HWo = p.Hout * p.Wout;
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    int m = m0 + (tid >> 3) + i * 32;
    if (m < p.M) {
      int b = m / HWo, rem = m - b * HWo;
      int oy = rem / p.Wout, ox = rem - oy * p.Wout;
      rb[i] = b; ry[i] = oy * p.stride - p.pad_t; rx[i] = ox * p.stride - p.pad_l;
    } else { rb[i] = -1; ry[i] = 0; rx[i] = 0; }
  }
  const int He = p.Hin << p.ups, We = p.Win << p.ups;

  uint4 ra[A_IT], rw[B_IT];
  int gidx[A_IT];  // b*Cin + c of the chunk (GN path), -1 when the chunk is padding
  bool gact[A_IT]; // LR: the chunk's source takes the activation

  auto load_tiles = [&](int kt) {
    const int kbase = kt * BK;
    int tap_u = 0, cb_u = 0;
    if (FAST) { tap_u = kbase / Cin; cb_u = kbase - tap_u * Cin; }
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      int tap, c;
      bool kval = true;
      if (FAST) { tap = tap_u; c = cb_u + kc * 8; }
      else {
        int k0 = kbase + kc * 8;
        kval = k0 < p.K;
        tap = k0 / Cin; c = k0 - tap * Cin;
      }
      int ky = tap / p.ks, kx = tap - ky * p.ks;
      int iy = ry[i] + ky, ix = rx[i] + kx;
      bool inb = kval && rb[i] >= 0 && iy >= 0 && iy < He && ix >= 0 && ix < We;
      uint4 v = make_uint4(0, 0, 0, 0);
      gidx[i] = -1;
      if (inb) {
        const f16* src; int cs, Cs;
        if (c < p.C1) { src = p.x; cs = c; Cs = p.ld1 ? p.ld1 : p.C1; } else { src = p.x2; cs = c - p.C1; Cs = p.ld2 ? p.ld2 : p.C2; }
        long long pix = ((long long)rb[i] * p.Hin + (iy >> p.ups)) * p.Win + (ix >> p.ups);
        v = *reinterpret_cast<const uint4*>(src + pix * Cs + cs);
        gidx[i] = rb[i] * Cin + c;
        if (LR) gact[i] = ((c < p.C1 ? p.lrelu_in : p.lrelu_in >> 1) & 1) != 0;
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      int n = n0 + (tid >> 3) + i * 32;
      int k0 = kbase + kc * 8;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (n < p.Nrows && k0 < p.K) v = *reinterpret_cast<const uint4*>(p.w + (long long)n * p.K + k0);
      rw[i] = v;
    }
  };

  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      int row = (tid >> 3) + i * 32;
      uint4 v = ra[i];
      if (LR) { if (gidx[i] >= 0) v = in_lrelu_apply8(v, p.gn_scale + gidx[i], p.gn_shift + gidx[i], gact[i] ? 0.01f : 1.0f); }
      else if (GN) { if (gidx[i] >= 0) v = gn_apply8(v, p.gn_scale + gidx[i], p.gn_shift + gidx[i], p.silu_in); }
      sA[buf * BM * CPR + row * CPR + swz8(row, kc)] = v;
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      int row = (tid >> 3) + i * 32;
      sB[buf * BN * CPR + row * CPR + swz8(row, kc)] = rw[i];
    }
  };

  f32x4 acc[NT][MT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // split-K (few tiles, long K: the stride-2 convs of the deep UNet levels): blockIdx.y owns a contiguous range of K-steps and writes
  // raw fp32 partials; splitk_reduce_kernel (kernels_conv3x3.hip) sums them and applies the epilogue
  const int nk_all = (p.K + BK - 1) / BK, S = p.splitk > 1 ? p.splitk : 1, ksplit = blockIdx.y;
  const int kt0 = S > 1 ? ksplit * nk_all / S : 0, nk = S > 1 ? (ksplit + 1) * nk_all / S : nk_all;
  const int g = lane >> 4, l15 = lane & 15;

  load_tiles(kt0);
  store_tiles(kt0 & 1);
  __syncthreads();

  for (int kt = kt0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tiles(kt + 1);
    const uint4* cA = sA + cur * BM * CPR;
    const uint4* cB = sB + cur * BN * CPR;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      f16x8 wf[NT], xf[MT];
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        int row = wave_n * (BN / 2) + a * 16 + l15;
        wf[a] = __builtin_bit_cast(f16x8, cB[row * CPR + swz8(row, kk * 4 + g)]);
      }
#pragma unroll
      for (int b = 0; b < MT; ++b) {
        int row = wave_m * (BM / 2) + b * 16 + l15;
        xf[b] = __builtin_bit_cast(f16x8, cA[row * CPR + swz8(row, kk * 4 + g)]);
      }
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[a], xf[b], acc[a][b], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tiles(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue (epilogue.h): lane holds y[m = col][n = 4g + r], r = 0..3 ----
  // Loads (bias, time embedding, residual) are issued back to back before any use: a load -> wait -> store chain per
  // 16x16 tile costs one memory round trip per tile.
  const int ncol = n0 + wave_n * (BN / 2) + g * 4;
  auto row_of = [&](int mt) { const int m = m0 + wave_m * (BM / 2) + mt * 16 + l15; return m < p.M ? m : -1; };
  if (S > 1) { epi_store_partial<MT, NT>(p, acc, row_of, ksplit, ncol); return; }
  const float osc = shift_scale(p.out_shift);   // ConvParams::out_shift
  f32x4 bb[NT];
  epi_load_cols<NT>(p.bias, ncol, p.N, bb);
  f16x4 rr[MT][NT], rl[MT][NT];
  epi_load_residual<MT, NT>(p, row_of, ncol, rr, rl);
#pragma unroll
  for (int b = 0; b < MT; ++b) {
    const int m = row_of(b);
    if (m < 0) continue;
    f32x4 tt[NT];   // the time embedding of this row's image
    if (p.temb) epi_load_cols<NT>(p.temb + (long long)(m / HWo) * p.ld_temb, ncol, p.N, tt);
    epi_store8_row<MT, NT>(p, acc, b, m, [&](int a, int mt) { f32x4 v = acc[a][mt] + bb[a]; if (p.temb) v += tt[a]; return v; }, osc, rr, rl, ncol);
  }
  if (p.stats) epi_stats_blocks32<MT, NT>(p, acc, row_of, (m0 + wave_m * (BM / 2)) / 32, ncol, l15);   // fused GroupNorm statistics per 32-row block
}

template <int BM, int BN, bool FAST, bool GN>
__global__ __launch_bounds__(256, 2) void igemm_kernel(const ConvParams p) {   // 2 waves/SIMD: accumulators stay in VGPRs
  igemm_body<BM, BN, FAST, GN, false>(p);
}
template <int BM, int BN, bool FAST>
__global__ __launch_bounds__(256, 2) void igemm_lrelu_kernel(const ConvParams p) { igemm_body<BM, BN, FAST, true, true>(p); }

template <int BM, int BN, bool FAST, bool GN, bool LR = false>
static void launch_cfg(const ConvParams& p, hipStream_t s) {
  const size_t smem = 2 * (BM + BN) * BK * sizeof(f16);
  void (*kern)(const ConvParams);
  if constexpr (LR) kern = igemm_lrelu_kernel<BM, BN, FAST>; else kern = igemm_kernel<BM, BN, FAST, GN>;
  ensure_dyn_smem(reinterpret_cast<const void*>(kern), (int)smem);
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  static const std::string pname = std::string(LR ? "igemm_lrelu<" : "igemm<") + std::to_string(BM) + "," + std::to_string(BN) + (FAST ? ",fast" : ",gen") +
                                   (GN && !LR ? ",gn>" : ">");
  // algorithmic work: 2*M*N*K flops; each source tensor, the weights and the residual read once, the output written once
  const double esz = 2.0;
  const double in_bytes = (double)p.B * p.Hin * p.Win * (p.C1 + p.C2) * esz;
  const double bytes = in_bytes + (double)p.N * p.K * esz + (double)p.M * p.N * (p.out_f32 || p.y_lo ? 4.0 : esz) + (p.res ? (double)p.M * p.N * (p.res_lo ? 4.0 : esz) : 0.0);
  ProfScope prof(pname.c_str(), 2.0 * p.M * (double)p.N * p.K, bytes, s);
  const int S = p.splitk > 1 ? p.splitk : 1;
  LDIFF_CHECK(S == 1 || (p.splitk_ws && !p.geglu), LDIFF_ERR_INVALID, "igemm: split-K needs a workspace");   // (fused statistics of a split launch: by the reduce kernel)
  hipLaunchKernelGGL(kern, dim3(ntm * ntn, S), dim3(256), smem, s, p);
  HIP_CHECK(hipGetLastError());
  if (S > 1) launch_splitk_reduce(p, s);
}

template <int BM, int BN>
static void launch_bmn(const ConvParams& p, bool fast, hipStream_t s) {
  const bool gn = p.gn_scale != nullptr;
  if (p.lrelu_in) { if (fast) launch_cfg<BM, BN, true, true, true>(p, s); else launch_cfg<BM, BN, false, true, true>(p, s); return; }
  if (fast) { if (gn) launch_cfg<BM, BN, true, true>(p, s); else launch_cfg<BM, BN, true, false>(p, s); }
  else      { if (gn) launch_cfg<BM, BN, false, true>(p, s); else launch_cfg<BM, BN, false, false>(p, s); }
}

void launch_igemm(const ConvParams& p, const ConvPlan& pl, hipStream_t s) {
  const int Cin = p.C1 + p.C2;
  LDIFF_CHECK(p.C1 % 8 == 0 && p.C2 % 8 == 0 && Cin > 0, LDIFF_ERR_INVALID, "igemm: channel counts must be multiples of 8 (C1=%d C2=%d)", p.C1, p.C2);
  LDIFF_CHECK(p.K == (p.tconv ? Cin : p.ks * p.ks * Cin), LDIFF_ERR_INVALID, "igemm: K=%d != ks*ks*Cin=%d", p.K, p.ks * p.ks * Cin);
  LDIFF_CHECK(p.N % 4 == 0 && p.N <= p.Nrows && p.ldy % 4 == 0 && (p.geglu ? p.N / 2 : p.N) <= p.ldy, LDIFF_ERR_INVALID, "igemm: bad N=%d Nrows=%d ldy=%d", p.N, p.Nrows, p.ldy);
  LDIFF_CHECK((p.C2 == 0) == (p.x2 == nullptr), LDIFF_ERR_INVALID, "igemm: x2/C2 mismatch");
  LDIFF_CHECK(!p.res || (p.ld_res % 4 == 0 && p.res_lo % 4 == 0), LDIFF_ERR_INVALID, "igemm: ld_res / res_lo must be multiples of 4");
  LDIFF_CHECK(p.y_lo % 4 == 0 && (p.y_lo == 0 || (!p.out_f32 && !p.geglu && p.y_lo >= p.N && p.y_lo + p.N <= p.ldy)), LDIFF_ERR_INVALID,
              "igemm: split output needs fp16 y with N <= y_lo and y_lo + N <= ldy (N=%d y_lo=%d ldy=%d)", p.N, p.y_lo, p.ldy);
  LDIFF_CHECK((p.ld1 == 0 || (p.ld1 >= p.C1 && p.ld1 % 8 == 0)) && (p.ld2 == 0 || (p.ld2 >= p.C2 && p.ld2 % 8 == 0)), LDIFF_ERR_INVALID,
              "igemm: row pitches must be multiples of 8 and >= the channel counts");
  // per-image weights (GroupNorm folded into the layer) exist only in the LDS-DMA GEMM: any other kernel would silently use image 0's
  LDIFF_CHECK(p.w_bstride == 0 || pl.kernel == ConvKernel::GEMM_DMA, LDIFF_ERR_INVALID, "igemm: per-image weights need the DMA GEMM path");
  LDIFF_CHECK(!p.temb || p.ld_temb % 4 == 0, LDIFF_ERR_INVALID, "igemm: ld_temb must be a multiple of 4");
  if (p.M <= 0) return;
  LDIFF_CHECK(p.splitk <= 1 || p.splitk_ws, LDIFF_ERR_INVALID, "conv: split-K needs a workspace");   // (fused statistics of a split launch: by the reduce kernel)
  LDIFF_CHECK(!p.w_par || (p.ups == 1 && p.splitk <= 1), LDIFF_ERR_INVALID, "conv3x3: parity weights need ups=1 and no split-K");
  LDIFF_CHECK(pl.kernel != ConvKernel::NONE, LDIFF_ERR_INVALID, "conv3x3: an fp8 lo half needs the 16 x 16 ping-pong kernel (C1=%d N=%d %dx%d)", p.C1, p.N, p.Hout, p.Wout);
  // every kernel but the dataflow conv ignores ConvParams::xs while the caller has already summed the shortcut's bias into p.bias: refuse instead of a silently wrong sum
  LDIFF_CHECK(!p.xs || pl.kernel == ConvKernel::C3_DATAFLOW, LDIFF_ERR_INVALID, "conv3x3: a folded shortcut (xs) needs the dataflow kernel, which does not take this launch (split-K %d)", p.splitk);
  switch (pl.kernel) {
    case ConvKernel::COND: launch_cond_conv(p, s); return;
    case ConvKernel::TCONV: launch_tconv2x2(p, s); return;
    case ConvKernel::SEGCONV: launch_segconv(p, s); return;
    case ConvKernel::CLSCONV: launch_cls_conv(p, s); return;
    case ConvKernel::C3_NARROW: case ConvKernel::C3_NARROW_FOLD: launch_conv3x3n(p, pl.kernel == ConvKernel::C3_NARROW_FOLD, s); return;
    case ConvKernel::C3_DATAFLOW: launch_conv3x3d(p, s); return;
    case ConvKernel::C3_PINGPONG: launch_conv3x3p(p, s); return;
    case ConvKernel::C3_HALO: launch_conv3x3(p, pl.bm, pl.bn, s); return;
    case ConvKernel::GEMM_DF: launch_gemm_df(p, s); return;
    case ConvKernel::GEMM_DMA: launch_gemm_dma(p, pl.bm, pl.bn, s); return;
    default: break;
  }
  LDIFF_CHECK(!p.geglu, LDIFF_ERR_INVALID, "GEGLU epilogue: only on 1x1 / linear layers with K %% 64 == 0, N %% 32 == 0, fp16 output, no residual");
  const bool fast = (Cin % BK == 0) && (p.C1 % BK == 0);
  if (pl.bm == 128 && pl.bn == 128) launch_bmn<128, 128>(p, fast, s);
  else if (pl.bm == 128) launch_bmn<128, 64>(p, fast, s);
  else launch_bmn<64, 64>(p, fast, s);
}
