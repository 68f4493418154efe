// Direct weight and bias gradients of convs over very many pixels (gfx950, MI355X): the backward of nnUNetTrainer.train_step at the planner's size, where
// M = B Ho Wo is 0.05 - 3.1 M rows -- the opposite corner from the fine-tuning step kernels_bwd.hip serves.  ONE kernel behind two entries: ldiff_op_conv_wgrad
// (narrow: Cx <= 128, Cy <= 64 at k = 3 / 128 at k = 1, the whole of Cy in one workgroup) and ldiff_op_conv_wgrad_wide (Cx <= 1024, Cy <= 512 / 2048, Cy in
// blocks of 64: the 128- and 256-channel stages, the transposed convs run as linears, the head).  The entries differ in their limits and in the plan, nothing else.
//
//   wgrad_direct    dW[n][ky][kx][c] = sum_(b,oy,ox) dy[b,oy,ox,n] x[b, oy s - p + ky, ox s - p + kx, c]   (0 outside the image), straight from the NHWC tensors:
//                   no im2col, no transposed copy.  The contraction index is the PIXEL, which is the slow axis of both operands in memory, while an MFMA
//                   fragment wants K fast: ds_read_b64_tr_b16 does that transpose on the way out of LDS.  A workgroup owns a 32 NTW (output channels from n0) x 32
//                   (input channels from c0) block of dW, all taps.  It stages those dy channels of a TH x 32 pixel output tile of one image and those x
//                   channels of the matching halo as plain pixel-major rows (zero outside the image, past the tile's real extent and past the real channels:
//                   a partial last block on either side is ZERO in LDS, never masked), then per tile row and tap issues v_mfma_f32_16x16x32_f16 with
//                   A = dy^T (16 output channels x 32 pixels) and B = x^T (the same 32 pixels shifted by the tap, at pixel stride s x 16 input channels).
//                   Both fragments come through the SAME read pattern -- lane 4q + p of 16-lane group g addresses pixel 4g + q (+ 16 for the second read),
//                   channels 4p .. 4p + 3 -- so whatever order of the 32 pixels lands in a fragment's K slots is shared by A and B.  A tap is an address
//                   offset; stride 2 doubles the pixel pitch of the x read only.
//   Work split      grid.x = persistent workgroups walking tiles t = blockIdx.x, + gridDim.x, ...; grid.y = 32-channel slabs of Cx; grid.z = 32 NTW-channel
//                   slabs of Cy.  A workgroup keeps its whole [32 NTW][k k][32] block in accumulators (wave w: column tile w & 1, row tiles (w >> 1) NTW .. + NTW),
//                   at most NTW 9 4 = 72 registers a lane, and writes it ONCE to the caller's workspace ws[wg][n][tap][c] ([wgs][CYP][k k][CXP] floats, both channel
//                   counts padded to whole slabs); a workgroup that got no tile writes its zeros.  wgrad_finalize adds the wgs partials in one fixed order
//                   (fp32: fin_sum below) and scatters to torch's [Cout][Cin][k][k]: no floating-point atomics, a replay is bit-identical.  An element's terms
//                   and their order depend on the tile walk (wgs) alone, not on the block that holds it.
//   Plans           narrow entry: NTW = 1 / 2 / 4 by Cy <= 32 / 64 / else, one slab of Cy, wgs = min(tiles, 1024 / xslabs).
//                   wide entry:   NTW = 2, ceil(Cy / 64) slabs of Cy, wgs = min(tiles, max(1, 1024 / (xslabs yslabs))): planned, the workspace is at most
//                   1024 * 64 * 32 * 9 * 4 B = 75 497 472 B at k = 3 (8 388 608 B at k = 1), whatever the channel counts.
//   LDS             pixel pitch = channels * 2 + 32 bytes for dy and for x at stride 1 (96 / 160 / 288 B = 24 / 40 / 72 dwords = 8 * odd), 80 B for x at stride 2
//                   (a read steps TWO pixels = 160 B = 40 dwords).  A transposed read's 32-lane half covers 8 consecutive (stride 2: alternate) pixels x 32 B = 8
//                   banks each: with a pixel step of 8 * odd dwords the eight 8-bank runs start at banks 8 * (odd * j mod 8), j = 0 .. 7, a permutation of
//                   0, 8, .., 56 (0, 24, 48, 8, 32, 56, 16, 40 for 96 B): they tile the 64 banks, so every operand read is conflict-free by the bank rule
//                   bank = (addr / 4) % 64; tap, tile-row and channel-tile offsets shift all lanes alike.  Every pitch is a multiple of 16 B and every channel
//                   offset a multiple of 8 B (ds_write_b128 staging, 8-byte aligned transposed reads); the dynamic LDS base is the only LDS of the kernel.  Every
//                   lane takes part in every read (EXEC all ones): the tile is padded, never masked.
//                     <3,1,2>: 4*32*160 + 6*34*96 = 40 064 B     <3,2,2>: 20 480 + 9*65*80 = 67 280 B     <1,1,2>: 8*32*160 + 8*32*96 = 65 536 B
//   Resources       profiles/wgrad_resources.txt (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): no scratch in any of the seven instances.
//   Not built       a 64 x 64 block (halves the re-staging of dy; 144 accumulator registers a lane) and a second LDS buffer that stages the next tile beside the
//                   MFMAs: DESIGN.md section 7 "Wide weight gradients" records what was measured and what was not.
//   colsum_slabs    db[n] = sum_m dy[m, n] through per-slab partials: N / 8 threads cover a row with 16-byte loads, a thread keeps its 8 channels for the
//                   slab, 256 / (N / 8) row lanes take alternate rows, one LDS pass adds the row lanes in order, colsum_finalize adds the slabs in fin_sum's fixed order.
#include "common.h"

namespace {

constexpr int WG_TW = 32;            // output pixels of a tile row = K of one MFMA
constexpr int WG_SLAB = 32;          // input channels of a workgroup's block
constexpr int WG_AUTO_WGS = 1024;    // workgroups of the planned persistent grid, over all three grid axes (4 a CU)

template <int K, int S, int NTW>
struct WgGeom {
  static constexpr int TH = K == 1 ? 8 : 4;
  static constexpr int XH = (TH - 1) * S + K, XW = (WG_TW - 1) * S + K;
  static constexpr int NB = 32 * NTW;   // output channels of a workgroup's block
  static constexpr int YPITCH = NB * 2 + 32, XPITCH = S == 2 ? 80 : 96;   // bytes per pixel
  static constexpr int SY = TH * WG_TW * YPITCH, SX = XH * XW * XPITCH;
  static constexpr int SMEM = SY + SX;
  static_assert(SY % 16 == 0 && YPITCH % 16 == 0 && XPITCH % 16 == 0, "16-byte LDS rows");
  static_assert((YPITCH / 4) % 16 == 8 && (S * XPITCH / 4) % 16 == 8, "pixel step = 8 * odd dwords");
  static_assert(SMEM <= 160 * 1024, "LDS of one workgroup");
};

struct WgradParams {
  const f16* x; const f16* dy; float* ws;
  int B, H, W, Cx, Ho, Wo, Cy;
  int tiles_x, tiles_y, tiles, CXP, CYP;   // CXP, CYP: the channel counts padded to whole slabs
  long long M;
};

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
__device__ __forceinline__ f16x8 tr_frag(const unsigned char* lo_addr, int hi_off) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lo_addr));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lo_addr + hi_off));
  const f16x4 a = __builtin_bit_cast(f16x4, lo), b = __builtin_bit_cast(f16x4, hi);
  return (f16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

template <int K, int S, int NTW>
__global__ __launch_bounds__(256) void wgrad_direct_kernel(WgradParams p) {
  using G = WgGeom<K, S, NTW>;
  constexpr int TH = G::TH, XH = G::XH, XW = G::XW, NB = G::NB, YPITCH = G::YPITCH, XPITCH = G::XPITCH, TAPS = K * K, PAD = K / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char wg_smem[];
  unsigned char* sY = wg_smem;
  unsigned char* sX = wg_smem + G::SY;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l15 = lane & 15, q = l15 >> 2, pp = l15 & 3;
  const int ct = wave & 1, nt0 = (wave >> 1) * NTW;
  const int c0 = blockIdx.y * WG_SLAB, n0 = blockIdx.z * NB;

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
      const long long m0 = (long long)t * (TH * WG_TW);
      for (int i = tid; i < TH * WG_TW * (NB / 8); i += 256) {
        const int ch = i % (NB / 8), pix = i / (NB / 8), n = n0 + ch * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (m0 + pix < p.M && n < p.Cy) v = *reinterpret_cast<const uint4*>(p.dy + (m0 + pix) * p.Cy + n);
        *reinterpret_cast<uint4*>(sY + pix * YPITCH + ch * 16) = v;
      }
      for (int i = tid; i < TH * WG_TW * (WG_SLAB / 8); i += 256) {
        const int ch = i & 3, pix = i >> 2, c = c0 + ch * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (m0 + pix < p.M && c < p.Cx) v = *reinterpret_cast<const uint4*>(p.x + (m0 + pix) * p.Cx + c);
        *reinterpret_cast<uint4*>(sX + pix * XPITCH + ch * 16) = v;
      }
    } else {
      const int tx = t % p.tiles_x, ty = (t / p.tiles_x) % p.tiles_y, b = t / (p.tiles_x * p.tiles_y);
      const int oy0 = ty * TH, ox0 = tx * WG_TW, iy0 = oy0 * S - PAD, ix0 = ox0 * S - PAD;
      for (int i = tid; i < TH * WG_TW * (NB / 8); i += 256) {
        const int ch = i % (NB / 8), pix = i / (NB / 8), n = n0 + ch * 8;
        const int oy = oy0 + (pix >> 5), ox = ox0 + (pix & 31);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (oy < p.Ho && ox < p.Wo && n < p.Cy) v = *reinterpret_cast<const uint4*>(p.dy + (((long long)b * p.Ho + oy) * p.Wo + ox) * p.Cy + n);
        *reinterpret_cast<uint4*>(sY + pix * YPITCH + ch * 16) = v;
      }
      for (int i = tid; i < XH * XW * (WG_SLAB / 8); i += 256) {
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
      for (int i = 0; i < NTW; ++i) a[i] = tr_frag(yrd + r * WG_TW * YPITCH + i * 32, 16 * YPITCH);
#pragma unroll
      for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const f16x8 bf = tr_frag(xrd + ((r * S + ky) * XW + kx) * XPITCH, 16 * S * XPITCH);
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

// Both finalizes add P partials per element in one fixed order: FIN_GROUPS interleaved chains (chain j takes partials j, j + FIN_GROUPS, ... in order; 32 consecutive
// elements a chain, so a warp-wide load is one 128-byte line), then the chains in order through LDS.  A single chain of 1024 dependent adds a thread was 150 us a launch.
constexpr int FIN_GROUPS = 8;
__device__ __forceinline__ float fin_sum(const float* __restrict__ src, long long stride, int P, bool live) {
  __shared__ float red[FIN_GROUPS][32];
  const int e = threadIdx.x & 31, grp = threadIdx.x >> 5;
  float a = 0.f;
  if (live)
    for (int w = grp; w < P; w += FIN_GROUPS) a += src[w * stride];
  red[grp][e] = a;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < FIN_GROUPS; ++j) t += red[j][e];
  return t;
}

// dw[n][c][tap] = sum over the workgroups of ws[wg][n][tap][c]
__global__ __launch_bounds__(256) void wgrad_finalize_kernel(const float* __restrict__ ws, float* __restrict__ dw, int wgs, int CYP, int TAPS, int CXP, int Cout, int Cin) {
  const int i = blockIdx.x * 32 + (threadIdx.x & 31);
  const bool live = i < Cout * TAPS * Cin;
  const int c = i % Cin, tap = (i / Cin) % TAPS, n = live ? i / (Cin * TAPS) : 0;
  const float a = fin_sum(ws + ((long long)n * TAPS + tap) * CXP + c, (long long)CYP * TAPS * CXP, wgs, live);
  if (live && threadIdx.x < 32) dw[((long long)n * Cin + c) * TAPS + tap] = a;
}

// ---- slab-reduced column sum ----
constexpr int CS_ROWS = 256, CS_MAX_SLABS = 1024;

__global__ __launch_bounds__(256) void colsum_slabs_kernel(const f16* __restrict__ dy, float* __restrict__ part, long long M, int N, int ld, long long rows, int NC, int RP) {
  __shared__ float red[8][256];   // [channel of the vector][thread]
  const int tid = threadIdx.x, cg = tid % NC, rl = tid / NC;
  const long long r0 = (long long)blockIdx.x * rows, r1 = r0 + rows < M ? r0 + rows : M;
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.f;
  if (rl < RP)
    for (long long row = r0 + rl; row < r1; row += RP) {
      const f16x8 v = *reinterpret_cast<const f16x8*>(dy + row * ld + cg * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += (float)v[j];
    }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[j][tid] = s[j];
  __syncthreads();
  if (rl == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = 0.f;
      for (int k = 0; k < RP; ++k) a += red[j][k * NC + cg];
      part[(long long)blockIdx.x * N + cg * 8 + j] = a;
    }
  }
}

__global__ __launch_bounds__(256) void colsum_finalize_kernel(const float* __restrict__ part, float* __restrict__ db, int slabs, int N) {
  const int n = blockIdx.x * 32 + (threadIdx.x & 31);
  const bool live = n < N;
  const float a = fin_sum(part + (live ? n : 0), N, slabs, live);
  if (live && threadIdx.x < 32) db[n] = a;
}

// The two entries: their names, channel limits and plan rule.  `wide`: Cy in slabs of 64 and the planned grid capped over all three axes.
struct WgEntry { const char* name; const char* scope; int cx_max, cy_max3, cy_max1; bool wide; };
constexpr WgEntry WG_NARROW{"conv_wgrad", "wgrad_direct", 128, 64, 128, false};
constexpr WgEntry WG_WIDE{"conv_wgrad_wide", "wgrad_wide", 1024, 512, 2048, true};

struct WgPlan { int TH, ntw, xslabs, yslabs, tiles_x, tiles_y, tiles, wgs, CYP, CXP; };
WgPlan wgrad_plan(const WgEntry& e, int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) {
  WgPlan pl;
  pl.TH = k == 1 ? 8 : 4;
  pl.ntw = e.wide ? 2 : Cy <= 32 ? 1 : Cy <= 64 ? 2 : 4;
  pl.xslabs = (Cx + WG_SLAB - 1) / WG_SLAB;
  pl.yslabs = e.wide ? (Cy + 32 * pl.ntw - 1) / (32 * pl.ntw) : 1;
  pl.CXP = pl.xslabs * WG_SLAB;
  pl.CYP = pl.yslabs * 32 * pl.ntw;
  pl.tiles_x = (Wo + WG_TW - 1) / WG_TW;
  pl.tiles_y = (Ho + pl.TH - 1) / pl.TH;
  pl.tiles = k == 1 ? (int)(((long long)B * Ho * Wo + pl.TH * WG_TW - 1) / (pl.TH * WG_TW)) : B * pl.tiles_x * pl.tiles_y;
  int cap = WG_AUTO_WGS / (pl.xslabs * pl.yslabs);
  cap = cap < 1 ? 1 : cap;
  pl.wgs = wgs > 0 ? wgs : (pl.tiles < cap ? pl.tiles : cap);
  return pl;
}
bool wgrad_shape_ok(const WgEntry& e, int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) {
  return B >= 1 && Ho >= 1 && Wo >= 1 && (k == 1 || k == 3) && Cx >= 8 && Cx % 8 == 0 && Cx <= e.cx_max && Cy >= 8 && Cy % 8 == 0 && Cy <= (k == 3 ? e.cy_max3 : e.cy_max1) &&
         wgs >= 0 && wgs <= 65535 && (long long)B * ((Ho + 3) / 4) * ((Wo + WG_TW - 1) / WG_TW) < (1ll << 31);
}
long long wgrad_ws_bytes(const WgEntry& e, int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) {
  if (!wgrad_shape_ok(e, B, Ho, Wo, Cx, Cy, k, wgs)) return 0;
  const WgPlan pl = wgrad_plan(e, B, Ho, Wo, Cx, Cy, k, wgs);
  return (long long)pl.wgs * pl.CYP * k * k * pl.CXP * 4;
}

template <int K, int S, int NTW>
void launch_wgrad_inst(const WgradParams& p, const WgPlan& pl, hipStream_t s) {
  using G = WgGeom<K, S, NTW>;
  auto kern = wgrad_direct_kernel<K, S, NTW>;
  ensure_dyn_smem(reinterpret_cast<const void*>(kern), G::SMEM);
  hipLaunchKernelGGL(kern, dim3(pl.wgs, pl.xslabs, pl.yslabs), dim3(256), G::SMEM, s, p);
  HIP_CHECK(hipGetLastError());
}

void launch_wgrad(const WgEntry& e, const f16* x, const f16* dy, float* dw, int B, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout, int Cin, int k, int stride, int wgs,
                  float* ws, long long ws_bytes, hipStream_t s) {
  const int cy_max = k == 3 ? e.cy_max3 : e.cy_max1;
  LDIFF_CHECK(k == 1 || k == 3, LDIFF_ERR_INVALID, "%s: k=%d (1 or 3)", e.name, k);
  LDIFF_CHECK(stride == 1 || (stride == 2 && k == 3), LDIFF_ERR_INVALID, "%s: stride=%d at k=%d (1, or 2 with k = 3)", e.name, stride, k);
  LDIFF_CHECK(Cx >= 8 && Cx % 8 == 0 && Cx <= e.cx_max, LDIFF_ERR_INVALID, "%s: Cx=%d (a multiple of 8 up to %d)", e.name, Cx, e.cx_max);
  LDIFF_CHECK(Cy >= 8 && Cy % 8 == 0 && Cy <= cy_max, LDIFF_ERR_INVALID, "%s: Cy=%d (a multiple of 8 up to %d at k=%d)", e.name, Cy, cy_max, k);
  LDIFF_CHECK(Cout >= 1 && Cout <= Cy, LDIFF_ERR_INVALID, "%s: Cout=%d must lie in 1 .. Cy=%d", e.name, Cout, Cy);
  LDIFF_CHECK(Cin >= 1 && Cin <= Cx, LDIFF_ERR_INVALID, "%s: Cin=%d must lie in 1 .. Cx=%d", e.name, Cin, Cx);
  LDIFF_CHECK(B >= 1 && H >= 1 && W >= 1, LDIFF_ERR_INVALID, "%s: B=%d H=%d W=%d", e.name, B, H, W);
  const int pad = k / 2;
  LDIFF_CHECK(Ho == (H + 2 * pad - k) / stride + 1 && Wo == (W + 2 * pad - k) / stride + 1, LDIFF_ERR_INVALID,
              "%s: Ho=%d Wo=%d do not match H=%d W=%d at k=%d stride=%d pad=%d (no upsampling)", e.name, Ho, Wo, H, W, k, stride, pad);
  LDIFF_CHECK(wgrad_shape_ok(e, B, Ho, Wo, Cx, Cy, k, wgs), LDIFF_ERR_INVALID, "%s: wgs=%d (0 = planned, or 1 .. 65535) / too many tiles", e.name, wgs);
  const long long need = wgrad_ws_bytes(e, B, Ho, Wo, Cx, Cy, k, wgs);
  LDIFF_CHECK(ws_bytes >= need, LDIFF_ERR_INVALID, "%s: ws_bytes=%lld, %lld needed (ldiff_op_%s_ws_bytes)", e.name, ws_bytes, need, e.name);
  const WgPlan pl = wgrad_plan(e, B, Ho, Wo, Cx, Cy, k, wgs);
  WgradParams p{x, dy, ws, B, H, W, Cx, Ho, Wo, Cy, pl.tiles_x, pl.tiles_y, pl.tiles, pl.CXP, pl.CYP, (long long)B * Ho * Wo};
  const double M = (double)B * Ho * Wo;
  {
    char name[64];   // the scope names of the two entries as the profiles have them: wgrad_direct<k,s,ntw>, wgrad_wide<k,s>
    if (e.wide) snprintf(name, sizeof name, "%s<%d,%d>", e.scope, k, stride);
    else snprintf(name, sizeof name, "%s<%d,%d,%d>", e.scope, k, stride, pl.ntw);
    ProfScope prof(name, 2.0 * M * Cy * k * k * Cx, 2.0 * M * Cy * pl.xslabs + 2.0 * (double)B * H * W * Cx * pl.yslabs + (double)need, s);
    if (k == 3 && stride == 1 && pl.ntw == 1) launch_wgrad_inst<3, 1, 1>(p, pl, s);
    else if (k == 3 && stride == 1) launch_wgrad_inst<3, 1, 2>(p, pl, s);
    else if (k == 3 && pl.ntw == 1) launch_wgrad_inst<3, 2, 1>(p, pl, s);
    else if (k == 3) launch_wgrad_inst<3, 2, 2>(p, pl, s);
    else if (pl.ntw == 1) launch_wgrad_inst<1, 1, 1>(p, pl, s);
    else if (pl.ntw == 2) launch_wgrad_inst<1, 1, 2>(p, pl, s);
    else launch_wgrad_inst<1, 1, 4>(p, pl, s);
  }
  const long long n = (long long)Cout * k * k * Cin;
  hipLaunchKernelGGL(wgrad_finalize_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, s, ws, dw, pl.wgs, pl.CYP, k * k, pl.CXP, Cout, Cin);
  HIP_CHECK(hipGetLastError());
}

struct CsPlan { int NC, RP; long long slabs, rows; };
CsPlan colsum_plan(long long M, int N) {
  CsPlan pl;
  pl.NC = N / 8;
  pl.RP = 256 / pl.NC;
  long long slabs = (M + CS_ROWS - 1) / CS_ROWS;
  slabs = slabs < 1 ? 1 : slabs > CS_MAX_SLABS ? CS_MAX_SLABS : slabs;
  pl.rows = (M + slabs - 1) / slabs;
  pl.slabs = (M + pl.rows - 1) / pl.rows;
  return pl;
}

}  // namespace

long long conv_wgrad_ws_bytes(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) { return wgrad_ws_bytes(WG_NARROW, B, Ho, Wo, Cx, Cy, k, wgs); }
long long conv_wgrad_wide_ws_bytes(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) { return wgrad_ws_bytes(WG_WIDE, B, Ho, Wo, Cx, Cy, k, wgs); }
void launch_conv_wgrad(const f16* x, const f16* dy, float* dw, int B, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout, int Cin, int k, int stride, int wgs,
                       float* ws, long long ws_bytes, hipStream_t s) {
  launch_wgrad(WG_NARROW, x, dy, dw, B, H, W, Cx, Ho, Wo, Cy, Cout, Cin, k, stride, wgs, ws, ws_bytes, s);
}
void launch_conv_wgrad_wide(const f16* x, const f16* dy, float* dw, int B, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout, int Cin, int k, int stride, int wgs,
                            float* ws, long long ws_bytes, hipStream_t s) {
  launch_wgrad(WG_WIDE, x, dy, dw, B, H, W, Cx, Ho, Wo, Cy, Cout, Cin, k, stride, wgs, ws, ws_bytes, s);
}

long long colsum_slabs_ws_bytes(long long M, int N) {
  if (M < 1 || N < 8 || N % 8 != 0 || N > 2048) return 0;
  return colsum_plan(M, N).slabs * N * 4;
}

void launch_colsum_slabs(const f16* dy, float* db, long long M, int N, int ld, float* ws, long long ws_bytes, hipStream_t s) {
  LDIFF_CHECK(M >= 1, LDIFF_ERR_INVALID, "colsum_slabs: M=%lld", M);
  LDIFF_CHECK(N >= 8 && N % 8 == 0 && N <= 2048, LDIFF_ERR_INVALID, "colsum_slabs: N=%d (a multiple of 8 up to 2048)", N);
  LDIFF_CHECK(ld >= N && ld % 8 == 0, LDIFF_ERR_INVALID, "colsum_slabs: ld=%d (a multiple of 8, at least N=%d)", ld, N);
  const long long need = colsum_slabs_ws_bytes(M, N);
  LDIFF_CHECK(ws_bytes >= need, LDIFF_ERR_INVALID, "colsum_slabs: ws_bytes=%lld, %lld needed (ldiff_op_colsum_slabs_ws_bytes)", ws_bytes, need);
  const CsPlan pl = colsum_plan(M, N);
  ProfScope prof("colsum_slabs", (double)M * N, 2.0 * M * N, s);
  hipLaunchKernelGGL(colsum_slabs_kernel, dim3((unsigned)pl.slabs), dim3(256), 0, s, dy, ws, M, N, ld, pl.rows, pl.NC, pl.RP);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3((N + 31) / 32), dim3(256), 0, s, ws, db, (int)pl.slabs, N);
  HIP_CHECK(hipGetLastError());
}
