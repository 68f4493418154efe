// Direct weight gradient of WIDE convs (gfx950, MI355X): the layers of nnUNetTrainer.train_step that ldiff_op_conv_wgrad (kernels_wgrad.hip) refuses -- more
// than 128 input channels, more than 64 (k = 3) / 128 (k = 1) output channels: the 128- and 256-channel stages, the transposed convs run as linears, the head.
//
//   wgrad_wide      the contraction of wgrad_direct, dW[n][ky][kx][c] = sum_(b,oy,ox) dy[b,oy,ox,n] x[b, oy s - p + ky, ox s - p + kx, c] (0 outside the image),
//                   straight from the NHWC tensors, blocked over the channels on BOTH sides: a workgroup owns a WW_NB x WW_CB = 64 (output channels) x 32 (input
//                   channels) block of dW, all taps.  It stages the 64 dy channels from n0 of a TH x 32 pixel tile and the 32 x channels from c0 of the matching
//                   halo as pixel-major rows, and per tile row and tap issues v_mfma_f32_16x16x32_f16 with A = dy^T, B = x^T, both through ds_read_b64_tr_b16 with the
//                   lane pattern of wgrad_direct (lane 4q + p of 16-lane group g: pixel 4g + q, + 16 for the second read, channels 4p .. 4p + 3), so A and B
//                   share whatever order of the 32 pixels lands in the K slots.  Wave w: input-channel tile w & 1, output-channel tiles 2 (w >> 1), + 1:
//                   2 x 9 x 4 = 72 accumulator registers a lane at k = 3.
//   Work split      grid.x = persistent workgroups walking tiles t = blockIdx.x, + gridDim.x, ...; grid.y = 32-channel slabs of Cx; grid.z = 64-channel slabs of
//                   Cy.  A partial last slab on either side is ZERO in LDS (the staging loads nothing past Cx / Cy), never masked: every lane takes part in every
//                   transposed read (EXEC all ones).  The planned grid.x = min(tiles, WW_AUTO_WGS / (slabs of Cx * slabs of Cy)), at least 1.
//   Reduction       each workgroup writes its block ONCE to ws[wg][n][tap][c] ([wgs][CYP][k k][CXP] floats, CYP = 64 slabs, CXP = 32 slabs; a workgroup that got
//                   no tile writes its zeros), and wgrad_finalize of kernels_wgrad.hip (launch_wgrad_finalize) adds the wgs partials in fin_sum's fixed order and
//                   scatters to torch's [Cout][Cin][k][k]: no floating-point atomics, a replay is bit-identical.  Planned, wgs * slabs * slabs <= 1024, so the
//                   workspace is at most 1024 * 64 * 32 * 9 * 4 B = 75 497 472 B at k = 3 (8 388 608 B at k = 1), whatever the channel counts.
//   LDS             dy: 64 channels * 2 B + 32 B = 160 B a pixel (40 dwords = 8 * 5).  x at stride 1: 32 * 2 + 32 = 96 B (24 dwords = 8 * 3); x at stride 2: 80 B
//                   a pixel, and a read steps TWO pixels = 160 B (40 dwords = 8 * 5).  A transposed read's 32-lane half covers 8 consecutive (stride 2: alternate)
//                   pixels x 32 B = 8 banks each; with a pixel step of 8 * odd dwords the eight 8-bank runs start at banks 8 * (odd * j mod 8), j = 0 .. 7, a
//                   permutation of 0, 8, .., 56: they tile the 64 banks, so every operand read is conflict-free by bank = (addr / 4) % 64.  Tap, tile-row and
//                   channel-tile offsets shift all lanes alike.  Every pitch is a multiple of 16 B and every channel offset a multiple of 8 B (4 pp halves), so
//                   ds_write_b128 staging is 16-byte and every transposed read 8-byte aligned; the dynamic LDS base is the only LDS of the kernel.
//                     <3,1>: 4*32*160 + 6*34*96 = 40 064 B     <3,2>: 20 480 + 9*65*80 = 67 280 B     <1,1>: 8*32*160 + 8*32*96 = 65 536 B
//   Resources       (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; profiles/wgrad_wide_resources.txt), no scratch in any:
//                     <3,1>  58 VGPR + 72 AGPR, 59 SGPR, 3 waves / SIMD by registers; 40 064 B LDS -> 3 workgroups a CU
//                     <3,2>  62 VGPR + 76 AGPR, 58 SGPR, 3 waves / SIMD;              67 280 B LDS -> 2 workgroups a CU
//                     <1,1>  42 VGPR +  8 AGPR, 42 SGPR, 8 waves / SIMD;              65 536 B LDS -> 2 workgroups a CU
//   Not built       a 64 x 64 block (halves the re-staging of dy; 144 accumulator registers a lane) and a second LDS buffer that stages the next tile beside the
//                   MFMAs: DESIGN.md section 7 "Wide weight gradients" records what was measured and what was not.
#include "common.h"

namespace {

constexpr int WW_TW = 32;            // output pixels of a tile row = K of one MFMA
constexpr int WW_CB = 32;            // input channels of a workgroup's block
constexpr int WW_NB = 64;            // output channels of a workgroup's block
constexpr int WW_NTW = WW_NB / 32;   // 16-channel output tiles a wave owns
constexpr int WW_AUTO_WGS = 1024;    // workgroups of the planned persistent grid, over all three grid axes (4 a CU)

template <int K, int S>
struct WwGeom {
  static constexpr int TH = K == 1 ? 8 : 4;
  static constexpr int XH = (TH - 1) * S + K, XW = (WW_TW - 1) * S + K;
  static constexpr int YPITCH = WW_NB * 2 + 32, XPITCH = S == 2 ? 80 : 96;   // bytes per pixel
  static constexpr int SY = TH * WW_TW * YPITCH, SX = XH * XW * XPITCH;
  static constexpr int SMEM = SY + SX;
};

struct WwParams {
  const f16* x; const f16* dy; float* ws;
  int B, H, W, Cx, Ho, Wo, Cy;
  int tiles_x, tiles_y, tiles, CXP, CYP;
  long long M;
};

typedef __attribute__((address_space(3))) s16x4 ww_lds_s16x4;
__device__ __forceinline__ f16x8 ww_tr_frag(const unsigned char* lo_addr, int hi_off) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ww_lds_s16x4*)(lo_addr));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ww_lds_s16x4*)(lo_addr + hi_off));
  const f16x4 a = __builtin_bit_cast(f16x4, lo), b = __builtin_bit_cast(f16x4, hi);
  return (f16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

template <int K, int S>
__global__ __launch_bounds__(256) void wgrad_wide_kernel(WwParams p) {
  using G = WwGeom<K, S>;
  constexpr int TH = G::TH, XH = G::XH, XW = G::XW, YPITCH = G::YPITCH, XPITCH = G::XPITCH, TAPS = K * K, PAD = K / 2, NTW = WW_NTW;
  extern __shared__ __attribute__((aligned(16))) unsigned char ww_smem[];
  unsigned char* sY = ww_smem;
  unsigned char* sX = ww_smem + G::SY;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l15 = lane & 15, q = l15 >> 2, pp = l15 & 3;
  const int ct = wave & 1, nt0 = (wave >> 1) * NTW;
  const int c0 = blockIdx.y * WW_CB, n0 = blockIdx.z * WW_NB;

  f32x4 acc[NTW][TAPS];
#pragma unroll
  for (int i = 0; i < NTW; ++i)
#pragma unroll
    for (int t = 0; t < TAPS; ++t) acc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // lane 4q + pp of group g: pixel 4g + q of the tile row (the second read: + 16), channels 4pp .. 4pp + 3 of the wave's first 16-channel tile
  const unsigned char* yrd = sY + (4 * g + q) * YPITCH + (16 * nt0 + 4 * pp) * 2;
  const unsigned char* xrd = sX + (4 * g + q) * S * XPITCH + (16 * ct + 4 * pp) * 2;

  for (int t = blockIdx.x; t < p.tiles; t += gridDim.x) {
    __syncthreads();   // the previous tile's reads are done
    if constexpr (K == 1) {   // no geometry at k = 1: the tile is TH * 32 consecutive pixels of the flat [M] index (a linear layer arrives as [1, 1, M, C])
      const long long m0 = (long long)t * (TH * WW_TW);
      for (int i = tid; i < TH * WW_TW * (WW_NB / 8); i += 256) {
        const int ch = i & 7, pix = i >> 3, n = n0 + ch * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (m0 + pix < p.M && n < p.Cy) v = *reinterpret_cast<const uint4*>(p.dy + (m0 + pix) * p.Cy + n);
        *reinterpret_cast<uint4*>(sY + pix * YPITCH + ch * 16) = v;
      }
      for (int i = tid; i < TH * WW_TW * (WW_CB / 8); i += 256) {
        const int ch = i & 3, pix = i >> 2, c = c0 + ch * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (m0 + pix < p.M && c < p.Cx) v = *reinterpret_cast<const uint4*>(p.x + (m0 + pix) * p.Cx + c);
        *reinterpret_cast<uint4*>(sX + pix * XPITCH + ch * 16) = v;
      }
    } else {
      const int tx = t % p.tiles_x, ty = (t / p.tiles_x) % p.tiles_y, b = t / (p.tiles_x * p.tiles_y);
      const int oy0 = ty * TH, ox0 = tx * WW_TW, iy0 = oy0 * S - PAD, ix0 = ox0 * S - PAD;
      for (int i = tid; i < TH * WW_TW * (WW_NB / 8); i += 256) {
        const int ch = i & 7, pix = i >> 3, n = n0 + ch * 8;
        const int oy = oy0 + (pix >> 5), ox = ox0 + (pix & 31);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (oy < p.Ho && ox < p.Wo && n < p.Cy) v = *reinterpret_cast<const uint4*>(p.dy + (((long long)b * p.Ho + oy) * p.Wo + ox) * p.Cy + n);
        *reinterpret_cast<uint4*>(sY + pix * YPITCH + ch * 16) = v;
      }
      for (int i = tid; i < XH * XW * (WW_CB / 8); i += 256) {
        const int ch = i & 3, pix = i >> 2;
        const int iy = iy0 + pix / XW, ix = ix0 + pix % XW, c = c0 + ch * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && c < p.Cx) v = *reinterpret_cast<const uint4*>(p.x + (((long long)b * p.H + iy) * p.W + ix) * p.Cx + c);
        *reinterpret_cast<uint4*>(sX + pix * XPITCH + ch * 16) = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TH; ++r) {
      f16x8 a[NTW];
#pragma unroll
      for (int i = 0; i < NTW; ++i) a[i] = ww_tr_frag(yrd + r * WW_TW * YPITCH + i * 32, 16 * YPITCH);
#pragma unroll
      for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const f16x8 bf = ww_tr_frag(xrd + ((r * S + ky) * XW + kx) * XPITCH, 16 * S * XPITCH);
#pragma unroll
          for (int i = 0; i < NTW; ++i) acc[i][ky * K + kx] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], bf, acc[i][ky * K + kx], 0, 0, 0);
        }
    }
  }

  // lane holds D[n = n0 + 16 tile + 4g + r][c = c0 + 16 ct + l15]: rows < CYP and columns < CXP of this workgroup's partial, both padded to whole slabs
  float* dst = p.ws + (long long)blockIdx.x * p.CYP * TAPS * p.CXP + c0 + 16 * ct + l15;
#pragma unroll
  for (int i = 0; i < NTW; ++i)
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[((long long)(n0 + 16 * (nt0 + i) + 4 * g + r) * TAPS + t) * p.CXP] = acc[i][t][r];
}

struct WwPlan { int TH, xslabs, yslabs, tiles_x, tiles_y, tiles, wgs, CYP, CXP; };
WwPlan ww_plan(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) {
  WwPlan pl;
  pl.TH = k == 1 ? 8 : 4;
  pl.xslabs = (Cx + WW_CB - 1) / WW_CB;
  pl.yslabs = (Cy + WW_NB - 1) / WW_NB;
  pl.CXP = pl.xslabs * WW_CB;
  pl.CYP = pl.yslabs * WW_NB;
  pl.tiles_x = (Wo + WW_TW - 1) / WW_TW;
  pl.tiles_y = (Ho + pl.TH - 1) / pl.TH;
  pl.tiles = k == 1 ? (int)(((long long)B * Ho * Wo + pl.TH * WW_TW - 1) / (pl.TH * WW_TW)) : B * pl.tiles_x * pl.tiles_y;
  int cap = WW_AUTO_WGS / (pl.xslabs * pl.yslabs);
  cap = cap < 1 ? 1 : cap;
  pl.wgs = wgs > 0 ? wgs : (pl.tiles < cap ? pl.tiles : cap);
  return pl;
}
bool ww_shape_ok(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) {
  return B >= 1 && Ho >= 1 && Wo >= 1 && (k == 1 || k == 3) && Cx >= 8 && Cx % 8 == 0 && Cx <= 1024 && Cy >= 8 && Cy % 8 == 0 && Cy <= (k == 3 ? 512 : 2048) && wgs >= 0 &&
         wgs <= 65535 && (long long)B * ((Ho + 3) / 4) * ((Wo + WW_TW - 1) / WW_TW) < (1ll << 31);
}

template <int K, int S>
void launch_ww_inst(const WwParams& p, const WwPlan& pl, hipStream_t s) {
  using G = WwGeom<K, S>;
  static_assert(G::SY % 16 == 0 && G::YPITCH % 16 == 0 && G::XPITCH % 16 == 0, "16-byte LDS rows");
  static_assert((G::YPITCH / 4) % 16 == 8 && (S * G::XPITCH / 4) % 16 == 8, "pixel step = 8 * odd dwords");
  static_assert(G::SMEM <= 160 * 1024, "LDS of one workgroup");
  auto kern = wgrad_wide_kernel<K, S>;
  ensure_dyn_smem(reinterpret_cast<const void*>(kern), G::SMEM);
  hipLaunchKernelGGL(kern, dim3(pl.wgs, pl.xslabs, pl.yslabs), dim3(256), G::SMEM, s, p);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

long long conv_wgrad_wide_ws_bytes(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) {
  if (!ww_shape_ok(B, Ho, Wo, Cx, Cy, k, wgs)) return 0;
  const WwPlan pl = ww_plan(B, Ho, Wo, Cx, Cy, k, wgs);
  return (long long)pl.wgs * pl.CYP * k * k * pl.CXP * 4;
}

void launch_conv_wgrad_wide(const f16* x, const f16* dy, float* dw, int B, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout, int Cin, int k, int stride, int wgs,
                            float* ws, long long ws_bytes, hipStream_t s) {
  LDIFF_CHECK(k == 1 || k == 3, LDIFF_ERR_INVALID, "conv_wgrad_wide: k=%d (1 or 3)", k);
  LDIFF_CHECK(stride == 1 || (stride == 2 && k == 3), LDIFF_ERR_INVALID, "conv_wgrad_wide: stride=%d at k=%d (1, or 2 with k = 3)", stride, k);
  LDIFF_CHECK(Cx >= 8 && Cx % 8 == 0 && Cx <= 1024, LDIFF_ERR_INVALID, "conv_wgrad_wide: Cx=%d (a multiple of 8 up to 1024)", Cx);
  LDIFF_CHECK(Cy >= 8 && Cy % 8 == 0 && Cy <= (k == 3 ? 512 : 2048), LDIFF_ERR_INVALID, "conv_wgrad_wide: Cy=%d (a multiple of 8 up to %d at k=%d)", Cy, k == 3 ? 512 : 2048, k);
  LDIFF_CHECK(Cout >= 1 && Cout <= Cy, LDIFF_ERR_INVALID, "conv_wgrad_wide: Cout=%d must lie in 1 .. Cy=%d", Cout, Cy);
  LDIFF_CHECK(Cin >= 1 && Cin <= Cx, LDIFF_ERR_INVALID, "conv_wgrad_wide: Cin=%d must lie in 1 .. Cx=%d", Cin, Cx);
  LDIFF_CHECK(B >= 1 && H >= 1 && W >= 1, LDIFF_ERR_INVALID, "conv_wgrad_wide: B=%d H=%d W=%d", B, H, W);
  const int pad = k / 2;
  LDIFF_CHECK(Ho == (H + 2 * pad - k) / stride + 1 && Wo == (W + 2 * pad - k) / stride + 1, LDIFF_ERR_INVALID,
              "conv_wgrad_wide: Ho=%d Wo=%d do not match H=%d W=%d at k=%d stride=%d pad=%d (no upsampling)", Ho, Wo, H, W, k, stride, pad);
  LDIFF_CHECK(ww_shape_ok(B, Ho, Wo, Cx, Cy, k, wgs), LDIFF_ERR_INVALID, "conv_wgrad_wide: wgs=%d (0 = planned, or 1 .. 65535) / too many tiles", wgs);
  const long long need = conv_wgrad_wide_ws_bytes(B, Ho, Wo, Cx, Cy, k, wgs);
  LDIFF_CHECK(ws_bytes >= need, LDIFF_ERR_INVALID, "conv_wgrad_wide: ws_bytes=%lld, %lld needed (ldiff_op_conv_wgrad_wide_ws_bytes)", ws_bytes, need);
  const WwPlan pl = ww_plan(B, Ho, Wo, Cx, Cy, k, wgs);
  WwParams p{x, dy, ws, B, H, W, Cx, Ho, Wo, Cy, pl.tiles_x, pl.tiles_y, pl.tiles, pl.CXP, pl.CYP, (long long)B * Ho * Wo};
  const double M = (double)B * Ho * Wo;
  {
    char name[64];
    snprintf(name, sizeof name, "wgrad_wide<%d,%d>", k, stride);
    ProfScope prof(name, 2.0 * M * Cy * k * k * Cx, 2.0 * M * Cy * pl.xslabs + 2.0 * (double)B * H * W * Cx * pl.yslabs + (double)need, s);
    if (k == 3 && stride == 1) launch_ww_inst<3, 1>(p, pl, s);
    else if (k == 3) launch_ww_inst<3, 2>(p, pl, s);
    else launch_ww_inst<1, 1>(p, pl, s);
  }
  launch_wgrad_finalize(ws, dw, pl.wgs, pl.CYP, k * k, pl.CXP, Cout, Cin, s);
}
