// 3x3 conv (pad 1, stride 1 or 2) + bias + optional SiLU in the EPILOGUE for the ControlNet's conditioning embedding (diffusers
// ControlNetConditioningEmbedding: 3 -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 -> 256 channels on maps up to eight times the latent size per side).
// No other conv family here is made for these channel counts: the halo-tile 3x3 kernels want Cin % 64 == 0, and the register-staged implicit
// GEMM's narrowest tile has 64 output columns (four times the useful ones at 16 outputs) and no activation behind its sum.
//
// Shape of the kernel.  Cout is a multiple of 16, so the output is whole mfma_f32_16x16x32_f16 tiles with the CHANNELS on the MFMA's row side
// (A = weights, straight from the [Cout][9 Cin] K-major matrix: 8 consecutive k per lane are one 16-byte load) and 16 consecutive pixels of
// one output row on its column side (B = activations).  The accumulator of a lane is then 4 consecutive channels of ONE pixel: an 8-byte NHWC
// store, and the NT channel tiles of a pixel complete its line.  K = 9 Cin runs in steps of 32 = four 8-channel chunks; a chunk never
// straddles a tap (Cin % 8 == 0), the chunks past K in the last step are zeroed on both sides (72 / 144 / 288 / 864: less than one step lost).
// A workgroup (4 waves) owns TH x 32 output pixels of one image and 16 NT output channels: the (TH - 1) s + 3 by 31 s + 3 halo of input pixels
// goes into LDS once (pixel pitch Cin + 8 halfs: the 16-byte reads of 16 neighbouring pixels then spread over the banks), all nine taps
// are read from it, and each weight fragment a wave loads (L1 / L2 resident: the matrices are 1 - 442 KB) is used for its MT = TH / 2 pixel groups.
// The next step's weight fragments are in flight while the current step's MFMAs issue.
#include "common.h"

namespace {

struct CondShape { int cin, cout, stride; };
// the layers of the embedding: (stored input channels, output channels, stride); the first layer's 3 input channels are stored padded to 8
constexpr CondShape kCondShapes[] = {{8, 16, 1}, {16, 16, 1}, {16, 32, 2}, {32, 32, 1}, {32, 96, 2}, {96, 96, 1}, {96, 256, 2}};

constexpr int TW = 32;
constexpr int cond_nt(int cout) { return cout == 256 ? 8 : cout / 16; }              // channel tiles per workgroup (256 outputs: two column blocks)
constexpr int cond_th(int cin, int stride) { return cin == 96 && stride == 2 ? 4 : 8; }   // output rows per workgroup (the 96-channel stride-2 halo of 8 rows would not fit LDS)
constexpr int cond_smem(int cin, int stride) {
  return ((cond_th(cin, stride) - 1) * stride + 3) * ((TW - 1) * stride + 3) * (cin + 8) * (int)sizeof(f16);
}

template <int CIN, int NT, int STRIDE, int TH, bool SILU>
__global__ __launch_bounds__(256) void condconv_kernel(const ConvParams p, const int tiles_x, const int tiles_y) {
  constexpr int RPW = TH / 4, MT = 2 * RPW;               // output rows per wave; 16-pixel groups per wave (two per row)
  constexpr int HH = (TH - 1) * STRIDE + 3, HWD = (TW - 1) * STRIDE + 3, PITCH = CIN + 8;
  constexpr int C8 = CIN / 8, KCH = 9 * C8, KS = (KCH + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) f16 halo[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, j = lane >> 4;
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const int n0 = blockIdx.y * NT * 16;
  const int ld = p.ld1 ? p.ld1 : p.C1;

  // the halo tile, zero outside the image (padding 1 on every side)
  const int iy0 = ty * TH * STRIDE - 1, ix0 = tx * TW * STRIDE - 1;
  const f16* xb = p.x + (long long)b * p.Hin * p.Win * ld;
  for (int idx = tid; idx < HH * HWD * C8; idx += 256) {
    const int pix = idx / C8, c8 = idx - pix * C8, hy = pix / HWD, hx = pix - hy * HWD;
    const int iy = iy0 + hy, ix = ix0 + hx;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) v = *reinterpret_cast<const uint4*>(xb + ((long long)iy * p.Win + ix) * ld + c8 * 8);
    *reinterpret_cast<uint4*>(halo + pix * PITCH + c8 * 8) = v;
  }
  __syncthreads();

  int pbase[MT];   // this lane's pixel of group m: its top-left tap in the halo tile
#pragma unroll
  for (int m = 0; m < MT; ++m) pbase[m] = ((wave * RPW + m / 2) * STRIDE * HWD + ((m & 1) * 16 + l15) * STRIDE) * PITCH;

  const f16* wrow = p.w + (long long)(n0 + l15) * p.K;   // row n0 + 16 a + l15 of the K-major weight matrix
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

  // epilogue: + bias, SiLU, one fp16 rounding; lane = pixel l15 of its group, channels n0 + 16 a + 4 j .. + 3
  f16* yb = reinterpret_cast<f16*>(p.y) + (long long)b * p.Hout * p.Wout * p.ldy;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int oy = ty * TH + wave * RPW + m / 2, ox = tx * TW + (m & 1) * 16 + l15;
    if (oy >= p.Hout || ox >= p.Wout) continue;
    f16* yp = yb + ((long long)oy * p.Wout + ox) * p.ldy;
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const int ch = n0 + 16 * a + 4 * j;
      f32x4 v = acc[a][m];
      if (p.bias) {
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + ch);
        v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
      }
      if constexpr (SILU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] * __builtin_amdgcn_rcpf(1.0f + __expf(-v[r]));
      }
      *reinterpret_cast<f16x4*>(yp + ch) = cvt4(v);
    }
  }
}

template <int CIN, int COUT, int STRIDE>
void launch_shape(const ConvParams& p, hipStream_t s) {
  constexpr int NT = cond_nt(COUT), TH = cond_th(CIN, STRIDE), SMEM = cond_smem(CIN, STRIDE);
  static_assert(SMEM <= 160 * 1024 && COUT % (16 * NT) == 0, "conditioning-embedding conv: tile does not fit");
  const int tiles_x = (p.Wout + TW - 1) / TW, tiles_y = (p.Hout + TH - 1) / TH;
  const dim3 grid((unsigned)(tiles_x * tiles_y * p.B), COUT / (16 * NT));
  const double bytes = (double)p.B * p.Hin * p.Win * CIN * 2.0 + (double)COUT * p.K * 2.0 + (double)p.M * COUT * 2.0;
  static const std::string base = "condconv<" + std::to_string(CIN) + "x" + std::to_string(COUT) + ",s" + std::to_string(STRIDE);
  static const std::string name_plain = base + ">", name_silu = base + ",silu>";
  ProfScope prof(p.silu_out ? name_silu.c_str() : name_plain.c_str(), 2.0 * p.M * (double)COUT * p.K, bytes, s);
  if (p.silu_out) {
    ensure_dyn_smem(reinterpret_cast<const void*>(condconv_kernel<CIN, NT, STRIDE, TH, true>), SMEM);
    condconv_kernel<CIN, NT, STRIDE, TH, true><<<grid, 256, SMEM, s>>>(p, tiles_x, tiles_y);
  } else {
    ensure_dyn_smem(reinterpret_cast<const void*>(condconv_kernel<CIN, NT, STRIDE, TH, false>), SMEM);
    condconv_kernel<CIN, NT, STRIDE, TH, false><<<grid, 256, SMEM, s>>>(p, tiles_x, tiles_y);
  }
  HIP_CHECK(hipGetLastError());
}

__global__ void scale_f16_kernel(const f16* x, f16* y, float a, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (f16)((float)x[i] * a);
}

}  // namespace

// y = f16(x * a): a ControlNet's zero-conv weights with conditioning_scale folded in (rebuilt when the scale changes, not per launch)
void launch_scale_f16(const f16* x, f16* y, float a, long long n, hipStream_t s) {
  if (n <= 0) return;
  scale_f16_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(x, y, a, n);
  HIP_CHECK(hipGetLastError());
}

// The launches this family is made for: one of the embedding's (Cin, Cout, stride), 3x3 with padding 1 on every side, one plain fp16 source,
// bias (+ SiLU) only behind the sum, plain fp16 output (cond_conv_eligible).  Of those, the executors' choice (ConvParams::cond_force = 0) is
//   - the ones that ask for the SiLU epilogue -- the embedding's own layers all do -- so that no launch that existed before this kernel changes its route;
//   - where the kernel was measured faster than the route such a layer had before (register-staged implicit GEMM + a SiLU launch), per layer, at SD-v1.5's
//     two sizes (scripts/bench_controlnet.py, profiles/controlnet_bench.txt; medians, spread a few %):
//       B = 8, 512^2 image: 3->16 5.7x, 16->16 5.1x, 16->32 s2 2.4x, 32->32 3.2x, 32->96 s2 1.4x, 96->96 2.0x (>= 512 workgroups each), 96->256 s2 0.79x
//       B = 1, 256^2 image: 3->16 2.5x, 16->16 2.5x (256 workgroups), 16->32 s2 1.17x, 32->32 1.33x (64), 32->96 s2 0.62x, 96->96 0.75x, 96->256 s2 0.63x (16)
//     i.e. never 96 -> 256 stride 2 (its 121 KB halo leaves one workgroup per CU and two column blocks re-read it), and the others from 64 workgroups up
//     (nothing between 16 and 64 was measured: the lower figure stays excluded).
// cond_force = 1 takes every eligible launch, -1 none (tests, A/B timing).
static bool cond_conv_eligible(const ConvParams& p);
static bool cond_conv_pays(const ConvParams& p) {
  if (p.C1 == 96 && p.N == 256) return false;
  const long long wgs = (long long)p.B * ((p.Wout + TW - 1) / TW) * ((p.Hout + cond_th(p.C1, p.stride) - 1) / cond_th(p.C1, p.stride)) * (p.N / (16 * cond_nt(p.N)));
  return wgs >= 64;
}
bool cond_conv_selected(const ConvParams& p) {
  if (p.cond_force < 0 || (p.cond_force == 0 && !p.silu_out)) return false;
  return cond_conv_eligible(p) && (p.cond_force > 0 || cond_conv_pays(p));
}
static bool cond_conv_eligible(const ConvParams& p) {
  if (p.ks != 3 || p.pad_t != 1 || p.pad_l != 1 || p.ups || p.x2 || p.C2 || p.gn_scale || p.temb || p.res || p.out_f32 || p.y_lo || p.geglu ||
      p.stats || p.splitk > 1 || p.lo8_slab0 || p.xs || p.w_par || p.w_bstride || p.out_shift || p.post_img || p.post_rgb || p.post_luma)
    return false;
  if (p.N % 16 != 0 || p.N > p.Nrows || p.ldy < p.N || p.ldy % 4 != 0 || ((p.ld1 ? p.ld1 : p.C1) & 7) != 0 || p.K != 9 * p.C1) return false;
  if (p.Hout != (p.Hin - 1) / p.stride + 1 || p.Wout != (p.Win - 1) / p.stride + 1) return false;
  for (const CondShape& c : kCondShapes)
    if (c.cin == p.C1 && c.cout == p.N && c.stride == p.stride) return true;
  return false;
}

void launch_cond_conv(const ConvParams& p, hipStream_t s) {
  LDIFF_CHECK(cond_conv_eligible(p), LDIFF_ERR_INVALID, "condconv: not a conditioning-embedding launch (Cin=%d N=%d stride=%d)", p.C1, p.N, p.stride);
  const int key = p.C1 * 10000 + p.N * 10 + p.stride;
  switch (key) {
    case 8 * 10000 + 16 * 10 + 1: launch_shape<8, 16, 1>(p, s); return;
    case 16 * 10000 + 16 * 10 + 1: launch_shape<16, 16, 1>(p, s); return;
    case 16 * 10000 + 32 * 10 + 2: launch_shape<16, 32, 2>(p, s); return;
    case 32 * 10000 + 32 * 10 + 1: launch_shape<32, 32, 1>(p, s); return;
    case 32 * 10000 + 96 * 10 + 2: launch_shape<32, 96, 2>(p, s); return;
    case 96 * 10000 + 96 * 10 + 1: launch_shape<96, 96, 1>(p, s); return;
    case 96 * 10000 + 256 * 10 + 2: launch_shape<96, 256, 2>(p, s); return;
    default: break;
  }
  LDIFF_CHECK(false, LDIFF_ERR_INVALID, "condconv: no instantiation for Cin=%d N=%d stride=%d", p.C1, p.N, p.stride);
}
