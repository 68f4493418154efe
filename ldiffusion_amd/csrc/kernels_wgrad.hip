// Direct weight and bias gradients of narrow convs over very many pixels (gfx950, MI355X): the backward of nnUNetTrainer.train_step at the planner's size,
// where M = B Ho Wo is 0.8 - 3.1 M rows and the conv has 32 or 64 output channels -- the opposite corner from the fine-tuning step kernels_bwd.hip serves.
//
//   wgrad_direct    dW[n][ky][kx][c] = sum_(b,oy,ox) dy[b,oy,ox,n] x[b, oy s - p + ky, ox s - p + kx, c]   (0 outside the image), straight from the NHWC tensors:
//                   no im2col, no transposed copy.  The contraction index is the PIXEL, which is the slow axis of both operands in memory, while an MFMA
//                   fragment wants K fast: ds_read_b64_tr_b16 does that transpose on the way out of LDS.  A workgroup stages the dy rows of a TH x 32 pixel
//                   output tile of one image and the matching x halo as plain pixel-major rows (zero outside the image, past the tile's real extent and
//                   past the real channels), then per tile row and tap issues v_mfma_f32_16x16x32_f16 with A = dy^T (16 output channels x 32 pixels) and
//                   B = x^T (the same 32 pixels shifted by the tap, at pixel stride s x 16 input channels).  Both fragments come through the SAME read
//                   pattern -- lane 4q + p of 16-lane group g addresses pixel 4g + q (+ 16 for the second read), channels 4p .. 4p + 3 -- so whatever
//                   order of the 32 pixels lands in a fragment's K slots is shared by A and B.  A tap is an address offset; stride 2 doubles the pixel
//                   pitch of the x read only.
//   Work split      grid.x = persistent workgroups walking tiles t = blockIdx.x, + gridDim.x, ...; grid.y = 32-channel slabs of Cx.  A workgroup keeps its
//                   whole [CYP][k k][32] block in accumulators (wave w: column tile w & 1, row tiles (w >> 1) NTW .. + NTW; CYP = 32 NTW >= Cy), at most
//                   NTW 9 4 = 72 registers a lane, and writes it ONCE to the caller's workspace ws[wg][n][tap][c]; a workgroup that got no tile writes its
//                   zeros.  wgrad_finalize adds the partials in one fixed order (fp32: fin_sum below) and scatters to torch's [Cout][Cin][k][k]: no floating-point
//                   atomics, a replay is bit-identical.
//   LDS             pixel pitch = channels * 2 + 32 bytes for dy and for x at stride 1 (96 / 160 / 288 B = 24 / 40 / 72 dwords = 8 * odd), 80 B for x at stride 2
//                   (pixel step 160 B = 40 dwords).  A transposed read's 32-lane half covers 8 consecutive pixels x 32 B: with a pixel step of 8 * odd dwords
//                   the eight 8-bank runs tile the 64 banks (0, 24, 48, 8, 32, 56, 16, 40 for 96 B), so every operand read is conflict-free by the bank rule
//                   bank = (addr / 4) % 64; tap and channel-tile offsets shift all lanes alike.  All pitches are multiples of 16 B (ds_write_b128 staging,
//                   8-byte aligned transposed reads); the dynamic LDS base is the only LDS of the kernel.  Every lane takes part in every read (EXEC all
//                   ones): the tile is padded, never masked.
//   colsum_slabs    db[n] = sum_m dy[m, n] through per-slab partials: N / 8 threads cover a row with 16-byte loads, a thread keeps its 8 channels for the
//                   slab, 256 / (N / 8) row lanes take alternate rows, one LDS pass adds the row lanes in order, colsum_finalize adds the slabs in fin_sum's fixed order.
#include "common.h"

namespace {

constexpr int WG_TW = 32;            // output pixels of a tile row = K of one MFMA
constexpr int WG_SLAB = 32;          // input channels of a workgroup
constexpr int WG_AUTO_WGS = 1024;    // workgroups of the planned persistent grid, over both grid axes (4 a CU)

template <int K, int S, int NTW>
struct WgGeom {
  static constexpr int TH = K == 1 ? 8 : 4;
  static constexpr int XH = (TH - 1) * S + K, XW = (WG_TW - 1) * S + K;
  static constexpr int CYP = 32 * NTW;
  static constexpr int YPITCH = CYP * 2 + 32, XPITCH = S == 2 ? 80 : 96;   // bytes per pixel
  static constexpr int SY = TH * WG_TW * YPITCH, SX = XH * XW * XPITCH;
  static constexpr int SMEM = SY + SX;
};

struct WgradParams {
  const f16* x; const f16* dy; float* ws;
  int B, H, W, Cx, Ho, Wo, Cy;
  int tiles_x, tiles_y, tiles, CXP;
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
  constexpr int TH = G::TH, XH = G::XH, XW = G::XW, CYP = G::CYP, YPITCH = G::YPITCH, XPITCH = G::XPITCH, TAPS = K * K, PAD = K / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char wg_smem[];
  unsigned char* sY = wg_smem;
  unsigned char* sX = wg_smem + G::SY;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l15 = lane & 15, q = l15 >> 2, pp = l15 & 3;
  const int ct = wave & 1, nt0 = (wave >> 1) * NTW;
  const int c0 = blockIdx.y * WG_SLAB;

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
      for (int i = tid; i < TH * WG_TW * (CYP / 8); i += 256) {
        const int ch = i % (CYP / 8), pix = i / (CYP / 8);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (m0 + pix < p.M && ch * 8 < p.Cy) v = *reinterpret_cast<const uint4*>(p.dy + (m0 + pix) * p.Cy + ch * 8);
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
      for (int i = tid; i < TH * WG_TW * (CYP / 8); i += 256) {
        const int ch = i % (CYP / 8), pix = i / (CYP / 8);
        const int oy = oy0 + (pix >> 5), ox = ox0 + (pix & 31);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (oy < p.Ho && ox < p.Wo && ch * 8 < p.Cy) v = *reinterpret_cast<const uint4*>(p.dy + (((long long)b * p.Ho + oy) * p.Wo + ox) * p.Cy + ch * 8);
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

  // lane holds D[n = 16 tile + 4g + r][c = l15]
  float* dst = p.ws + (long long)blockIdx.x * CYP * TAPS * p.CXP + c0 + 16 * ct + l15;
#pragma unroll
  for (int i = 0; i < NTW; ++i)
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[((long long)(16 * (nt0 + i) + 4 * g + r) * TAPS + t) * p.CXP] = acc[i][t][r];
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

struct WgPlan { int TH, ntw, slabs, tiles_x, tiles_y, tiles, wgs, CYP, CXP; };
WgPlan wgrad_plan(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) {
  WgPlan pl;
  pl.TH = k == 1 ? 8 : 4;
  pl.ntw = Cy <= 32 ? 1 : Cy <= 64 ? 2 : 4;
  pl.CYP = 32 * pl.ntw;
  pl.slabs = (Cx + WG_SLAB - 1) / WG_SLAB;
  pl.CXP = pl.slabs * WG_SLAB;
  pl.tiles_x = (Wo + WG_TW - 1) / WG_TW;
  pl.tiles_y = (Ho + pl.TH - 1) / pl.TH;
  pl.tiles = k == 1 ? (int)(((long long)B * Ho * Wo + pl.TH * WG_TW - 1) / (pl.TH * WG_TW)) : B * pl.tiles_x * pl.tiles_y;
  const int cap = WG_AUTO_WGS / pl.slabs;
  pl.wgs = wgs > 0 ? wgs : (pl.tiles < cap ? pl.tiles : cap);
  return pl;
}
bool wgrad_shape_ok(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) {
  return B >= 1 && Ho >= 1 && Wo >= 1 && (k == 1 || k == 3) && Cx >= 8 && Cx % 8 == 0 && Cx <= 128 && Cy >= 8 && Cy % 8 == 0 && Cy <= (k == 3 ? 64 : 128) && wgs >= 0 &&
         wgs <= 65535 && (long long)B * ((Ho + 3) / 4) * ((Wo + WG_TW - 1) / WG_TW) < (1ll << 31);
}

template <int K, int S, int NTW>
void launch_wgrad_inst(const WgradParams& p, const WgPlan& pl, hipStream_t s) {
  using G = WgGeom<K, S, NTW>;
  static_assert(G::SY % 16 == 0 && G::YPITCH % 16 == 0 && G::XPITCH % 16 == 0, "16-byte LDS rows");
  auto kern = wgrad_direct_kernel<K, S, NTW>;
  ensure_dyn_smem(reinterpret_cast<const void*>(kern), G::SMEM);
  hipLaunchKernelGGL(kern, dim3(pl.wgs, pl.slabs), dim3(256), G::SMEM, s, p);
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

long long conv_wgrad_ws_bytes(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) {
  if (!wgrad_shape_ok(B, Ho, Wo, Cx, Cy, k, wgs)) return 0;
  const WgPlan pl = wgrad_plan(B, Ho, Wo, Cx, Cy, k, wgs);
  return (long long)pl.wgs * pl.CYP * k * k * pl.CXP * 4;
}

void launch_conv_wgrad(const f16* x, const f16* dy, float* dw, int B, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout, int Cin, int k, int stride, int wgs,
                       float* ws, long long ws_bytes, hipStream_t s) {
  LDIFF_CHECK(k == 1 || k == 3, LDIFF_ERR_INVALID, "conv_wgrad: k=%d (1 or 3)", k);
  LDIFF_CHECK(stride == 1 || (stride == 2 && k == 3), LDIFF_ERR_INVALID, "conv_wgrad: stride=%d at k=%d (1, or 2 with k = 3)", stride, k);
  LDIFF_CHECK(Cx >= 8 && Cx % 8 == 0 && Cx <= 128, LDIFF_ERR_INVALID, "conv_wgrad: Cx=%d (a multiple of 8 up to 128)", Cx);
  LDIFF_CHECK(Cy >= 8 && Cy % 8 == 0 && Cy <= (k == 3 ? 64 : 128), LDIFF_ERR_INVALID, "conv_wgrad: Cy=%d (a multiple of 8 up to %d at k=%d)", Cy, k == 3 ? 64 : 128, k);
  LDIFF_CHECK(Cout >= 1 && Cout <= Cy, LDIFF_ERR_INVALID, "conv_wgrad: Cout=%d must lie in 1 .. Cy=%d", Cout, Cy);
  LDIFF_CHECK(Cin >= 1 && Cin <= Cx, LDIFF_ERR_INVALID, "conv_wgrad: Cin=%d must lie in 1 .. Cx=%d", Cin, Cx);
  LDIFF_CHECK(B >= 1 && H >= 1 && W >= 1, LDIFF_ERR_INVALID, "conv_wgrad: B=%d H=%d W=%d", B, H, W);
  const int pad = k / 2;
  LDIFF_CHECK(Ho == (H + 2 * pad - k) / stride + 1 && Wo == (W + 2 * pad - k) / stride + 1, LDIFF_ERR_INVALID,
              "conv_wgrad: Ho=%d Wo=%d do not match H=%d W=%d at k=%d stride=%d pad=%d (no upsampling)", Ho, Wo, H, W, k, stride, pad);
  LDIFF_CHECK(wgrad_shape_ok(B, Ho, Wo, Cx, Cy, k, wgs), LDIFF_ERR_INVALID, "conv_wgrad: wgs=%d (0 = planned, or 1 .. 65535) / too many tiles", wgs);
  const long long need = conv_wgrad_ws_bytes(B, Ho, Wo, Cx, Cy, k, wgs);
  LDIFF_CHECK(ws_bytes >= need, LDIFF_ERR_INVALID, "conv_wgrad: ws_bytes=%lld, %lld needed (ldiff_op_conv_wgrad_ws_bytes)", ws_bytes, need);
  const WgPlan pl = wgrad_plan(B, Ho, Wo, Cx, Cy, k, wgs);
  WgradParams p{x, dy, ws, B, H, W, Cx, Ho, Wo, Cy, pl.tiles_x, pl.tiles_y, pl.tiles, pl.CXP, (long long)B * Ho * Wo};
  const double M = (double)B * Ho * Wo;
  {
    char name[64];
    snprintf(name, sizeof name, "wgrad_direct<%d,%d,%d>", k, stride, pl.ntw);
    ProfScope prof(name, 2.0 * M * Cy * k * k * Cx, 2.0 * M * Cy * pl.slabs + 2.0 * (double)B * H * W * Cx + (double)need, s);
    if (k == 3 && stride == 1 && pl.ntw == 1) launch_wgrad_inst<3, 1, 1>(p, pl, s);
    else if (k == 3 && stride == 1) launch_wgrad_inst<3, 1, 2>(p, pl, s);
    else if (k == 3 && pl.ntw == 1) launch_wgrad_inst<3, 2, 1>(p, pl, s);
    else if (k == 3) launch_wgrad_inst<3, 2, 2>(p, pl, s);
    else if (pl.ntw == 1) launch_wgrad_inst<1, 1, 1>(p, pl, s);
    else if (pl.ntw == 2) launch_wgrad_inst<1, 1, 2>(p, pl, s);
    else launch_wgrad_inst<1, 1, 4>(p, pl, s);
  }
  const int n = Cout * k * k * Cin;
  hipLaunchKernelGGL(wgrad_finalize_kernel, dim3((n + 31) / 32), dim3(256), 0, s, ws, dw, pl.wgs, pl.CYP, k * k, pl.CXP, Cout, Cin);
  HIP_CHECK(hipGetLastError());
}

// the same finalize for the partials of kernels_wgrad_wide.hip: one definition of the fixed order
void launch_wgrad_finalize(const float* ws, float* dw, int wgs, int CYP, int taps, int CXP, int Cout, int Cin, hipStream_t s) {
  const long long n = (long long)Cout * taps * Cin;
  hipLaunchKernelGGL(wgrad_finalize_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, s, ws, dw, wgs, CYP, taps, CXP, Cout, Cin);
  HIP_CHECK(hipGetLastError());
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
