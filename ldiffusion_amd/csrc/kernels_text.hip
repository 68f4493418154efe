// Kernels of the CLIP text encoder (ldiff_textenc, model_text.hip) for gfx950: the embedding gather, causal self-attention over a short sequence, and the
// LayerNorm of the split stream.  The linears run on the GEMM routes the UNet's transformer blocks use (kernels_gemm.hip; quick_gelu / gelu behind FC1: ConvParams::act_out).
#include "common.h"

namespace {

// ---- text_embed: x[m] = token_embedding[ids[m]] + position_embedding[m % L], summed in fp32, written as the split residual stream [hi(H) | lo(H)] ----
__global__ __launch_bounds__(256) void text_embed_kernel(const int* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos, f16* __restrict__ y,
                                                         int M, int L, int H, int vocab) {
  const int m = blockIdx.x;
  if (m >= M) return;
  int id = ids[m];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);   // (validated on the host; a replayed graph reads whatever the staging buffer holds)
  const float* tr = tok + (long long)id * H;
  const float* pr = pos + (long long)(m % L) * H;
  f16* yr = y + (long long)m * 2 * H;
  for (int c = threadIdx.x * 4; c < H; c += 1024) {   // H % 8 == 0
    const float4 a = *reinterpret_cast<const float4*>(tr + c), b = *reinterpret_cast<const float4*>(pr + c);
    const f32x4 v = (f32x4){a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
    const f16x4 hi = cvt4(v);
    *reinterpret_cast<f16x4*>(yr + c) = hi;
    *reinterpret_cast<f16x4*>(yr + H + c) = cvt4(v - up4(hi));
  }
}

// ---- text_attn<D>: causal softmax(scale Q K^T) V of one (image, head) per workgroup, L <= 128 -------------------------------------------
// Q, K, V are column blocks of the fused projection output qkv [B L, ld]: head h of Q at column h D, of K at hidden + h D, of V at 2 hidden + h D.
// K goes to LDS row-major (pitch DP + 8), V transposed (Vt[c][key], pitch LK + 8); rows / keys beyond L are zeros.  A wave owns 16 queries at a time:
//   S^T tile (16 keys x 16 queries) = mfma(A = K rows, B = Q rows): the lane with (g, l15) holds keys 16 kt + 4 g + r (r = 0..3) of query 16 qt + l15, so a
//   query's row lives in the registers of the four lanes l15 + 16 g.  Keys above the query or beyond L are set to -inf BEFORE the maximum; the softmax is
//   taken over the whole row in fp32 (no online rescale), p rounded once to fp16, the row sum from the unrounded p.
//   O^T tile (16 channels x 16 queries) = mfma(A = Vt rows, B = P^T): the k index of a 32-key step is permuted so that B is exactly what the lane holds --
//   slot s of lane g is key 16 (2 pp + s / 4) + 4 g + s % 4 -- and A reads Vt with the same permutation (two 8-byte reads).
// Key tiles above the diagonal are never computed; a tile pair's missing half is p = 0 against finite (zero-filled) Vt.
template <int D>
__global__ __launch_bounds__(256) void text_attn_kernel(const f16* __restrict__ qkv, int ld, int hidden, f16* __restrict__ o, int ldo, int o_lo, int L, int heads, float scale_log2e) {
  constexpr int DP = (D + 31) / 32 * 32, KP = DP + 8, KS = DP / 32, DT = D / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int LK = (L + 31) / 32 * 32, VP = LK + 8;
  f16* Ks = reinterpret_cast<f16*>(smem_raw);          // [LK][KP]
  f16* Vt = Ks + LK * KP;                               // [D][VP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const f16* base = qkv + (long long)b * L * ld + h * D;

  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  for (int i = tid; i < LK * (DP / 8); i += 256) {
    const int row = i / (DP / 8), c8 = (i % (DP / 8)) * 8;
    uint4 v = zero4;
    if (row < L && c8 < D) v = *reinterpret_cast<const uint4*>(base + (long long)row * ld + hidden + c8);
    *reinterpret_cast<uint4*>(Ks + row * KP + c8) = v;
  }
  for (int i = tid; i < LK * (D / 8); i += 256) {
    const int row = i / (D / 8), c8 = (i % (D / 8)) * 8;
    uint4 v = zero4;
    if (row < L) v = *reinterpret_cast<const uint4*>(base + (long long)row * ld + 2 * hidden + c8);
    const f16x8 e = __builtin_bit_cast(f16x8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) Vt[(c8 + j) * VP + row] = e[j];
  }
  __syncthreads();

  const int nqt = (L + 15) / 16;
  for (int qt = wave; qt < nqt; qt += 4) {   // (qt is wave-uniform)
    const int query = qt * 16 + l15, qrow = query < L ? query : L - 1;
    f16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = ks * 32 + g * 8;
      uint4 v = zero4;
      if (c < D) v = *reinterpret_cast<const uint4*>(base + (long long)qrow * ld + c);
      qf[ks] = __builtin_bit_cast(f16x8, v);
    }
    f32x4 sc[8];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      sc[kt] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (kt <= qt) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const f16x8 kf = *reinterpret_cast<const f16x8*>(Ks + (kt * 16 + l15) * KP + ks * 32 + g * 8);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt * 16 + g * 4 + r;
          const float s = (key > query || key >= L) ? -INFINITY : acc[r] * scale_log2e;
          sc[kt][r] = s;
          mx = fmaxf(mx, s);
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));   // finite: key 0 is never masked
    float z = 0.f;
    f16x4 ph[8];
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      f32x4 p = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (kt <= qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { p[r] = __builtin_amdgcn_exp2f(sc[kt][r] - mx); z += p[r]; }
      }
      ph[kt] = cvt4(p);
    }
    z += __shfl_xor(z, 16);
    z += __shfl_xor(z, 32);
    f32x4 oa[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) oa[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      if (2 * pp <= qt) {
        f16x8 pb;
#pragma unroll
        for (int r = 0; r < 4; ++r) { pb[r] = ph[2 * pp][r]; pb[4 + r] = ph[2 * pp + 1][r]; }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const f16* vr = Vt + (dt * 16 + l15) * VP + pp * 32 + g * 4;
          const f16x4 v0 = *reinterpret_cast<const f16x4*>(vr), v1 = *reinterpret_cast<const f16x4*>(vr + 16);
          f16x8 va;
#pragma unroll
          for (int r = 0; r < 4; ++r) { va[r] = v0[r]; va[4 + r] = v1[r]; }
          oa[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb, oa[dt], 0, 0, 0);
        }
      }
    }
    if (query < L) {   // rows of the padded tile beyond L are never stored
      const float inv = 1.0f / z;
      f16* orow = o + ((long long)b * L + query) * ldo + h * D + g * 4;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const f32x4 v = oa[dt] * inv;
        const f16x4 hi = cvt4(v);
        *reinterpret_cast<f16x4*>(orow + dt * 16) = hi;
        if (o_lo) *reinterpret_cast<f16x4*>(orow + o_lo + dt * 16) = cvt4(v - up4(hi));   // split output: the rounding remainder behind the hi half
      }
    }
  }
}

template <int D>
void launch_ta(const f16* qkv, int ld, int hidden, f16* o, int ldo, int o_lo, int B, int heads, int L, float scale, hipStream_t s) {
  constexpr int DP = (D + 31) / 32 * 32;
  const int LK = (L + 31) / 32 * 32;
  const size_t smem = ((size_t)LK * (DP + 8) + (size_t)D * (LK + 8)) * sizeof(f16);
  auto kern = text_attn_kernel<D>;
  ensure_dyn_smem(reinterpret_cast<const void*>(kern), 2 * 128 * 136 * (int)sizeof(f16));   // the largest any L takes: one attribute call per kernel
  hipLaunchKernelGGL(kern, dim3(B * heads), dim3(256), smem, s, qkv, ld, hidden, o, ldo, o_lo, L, heads, scale * 1.4426950408889634f);
}

// ---- text_ln: LayerNorm of the split stream, one wave per row (LN1, LN2 and the final one); fp32 or fp16 [M, C] to out, and / or the normalised row as a
// split tensor (the operand of the GEMM behind it).  Statistics that are not finite raise the handle's sticky flag. ----
__global__ __launch_bounds__(256) void text_ln_kernel(const f16* __restrict__ x, int C, int M, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                            void* __restrict__ out, int out_f16, f16* __restrict__ ysplit, int* nonfinite) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const f16* xr = x + (long long)row * 2 * C;
  float sum = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const f32x4 v = up4(*reinterpret_cast<const f16x4*>(xr + c)) + up4(*reinterpret_cast<const f16x4*>(xr + C + c));
    sum += (v[0] + v[1]) + (v[2] + v[3]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  const float mean = sum / (float)C;
  float var = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const f32x4 v = up4(*reinterpret_cast<const f16x4*>(xr + c)) + up4(*reinterpret_cast<const f16x4*>(xr + C + c)) - mean;
    var += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) var += __shfl_xor(var, off);
  const float rstd = rsqrtf(var / (float)C + eps);
  if (nonfinite && lane == 0 && !(__builtin_fabsf(sum) <= 3.0e38f && var <= 3.0e38f)) *nonfinite = 1;   // (NaN fails both compares)
  for (int c = lane * 4; c < C; c += 256) {
    const f32x4 v = up4(*reinterpret_cast<const f16x4*>(xr + c)) + up4(*reinterpret_cast<const f16x4*>(xr + C + c));
    const float4 gm = *reinterpret_cast<const float4*>(gamma + c), bt = *reinterpret_cast<const float4*>(beta + c);
    const f32x4 y = (v - mean) * rstd * (f32x4){gm.x, gm.y, gm.z, gm.w} + (f32x4){bt.x, bt.y, bt.z, bt.w};
    if (out) {
      if (out_f16) *reinterpret_cast<f16x4*>(reinterpret_cast<f16*>(out) + (long long)row * C + c) = cvt4(y);
      else *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + (long long)row * C + c) = y;
    }
    if (ysplit) {
      const f16x4 hi = cvt4(y);
      *reinterpret_cast<f16x4*>(ysplit + (long long)row * 2 * C + c) = hi;
      *reinterpret_cast<f16x4*>(ysplit + (long long)row * 2 * C + C + c) = cvt4(y - up4(hi));
    }
  }
}

__global__ void f32_to_f16_kernel(const float* __restrict__ x, f16* __restrict__ y, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (f16)x[i];
}

}  // namespace

void launch_text_embed(const int* ids, const float* tok, const float* pos, f16* y, int M, int L, int H, int vocab, hipStream_t s) {
  LDIFF_CHECK(H % 8 == 0 && M >= 1 && L >= 1, LDIFF_ERR_INVALID, "text_embed: hidden = %d must be a multiple of 8", H);
  ProfScope prof("text_embed", (double)M * H, (double)M * H * 12.0, s);
  hipLaunchKernelGGL(text_embed_kernel, dim3(M), dim3(256), 0, s, ids, tok, pos, y, M, L, H, vocab);
  HIP_CHECK(hipGetLastError());
}

bool text_attention_supported(int d, int L) { return d >= 16 && d <= 128 && d % 16 == 0 && L >= 1 && L <= 128; }

void launch_text_attention(const f16* qkv, int ld, int hidden, f16* o, int ldo, int o_lo, int B, int heads, int L, int d, float scale, hipStream_t s) {
  LDIFF_CHECK(text_attention_supported(d, L), LDIFF_ERR_INVALID, "text_attention: head dim %d must be a multiple of 16 in 16..128 and L = %d in 1..128", d, L);
  LDIFF_CHECK(B >= 1 && heads >= 1 && hidden >= heads * d && ld >= 3 * hidden && ld % 8 == 0 && hidden % 8 == 0 && ldo >= heads * d && ldo % 4 == 0 && o_lo >= 0 && o_lo % 4 == 0 && (o_lo == 0 || (o_lo >= heads * d && ldo >= o_lo + heads * d)) &&
                  (reinterpret_cast<uintptr_t>(qkv) & 15) == 0 && (reinterpret_cast<uintptr_t>(o) & 7) == 0,
              LDIFF_ERR_INVALID, "text_attention: qkv must be [B L, ld >= 3 hidden] with ld %% 8 == 0, hidden %% 8 == 0 and 16-byte alignment, o [B L, ldo >= heads d] with ldo %% 4 == 0 (ld=%d hidden=%d ldo=%d heads=%d d=%d)",
              ld, hidden, ldo, heads, d);
  ProfScope prof("text_attn", 2.0 * B * heads * (double)L * L * d, (double)B * L * hidden * 8.0, s);
  switch (d / 16) {
    case 1: launch_ta<16>(qkv, ld, hidden, o, ldo, o_lo, B, heads, L, scale, s); break;
    case 2: launch_ta<32>(qkv, ld, hidden, o, ldo, o_lo, B, heads, L, scale, s); break;
    case 3: launch_ta<48>(qkv, ld, hidden, o, ldo, o_lo, B, heads, L, scale, s); break;
    case 4: launch_ta<64>(qkv, ld, hidden, o, ldo, o_lo, B, heads, L, scale, s); break;
    case 5: launch_ta<80>(qkv, ld, hidden, o, ldo, o_lo, B, heads, L, scale, s); break;
    case 6: launch_ta<96>(qkv, ld, hidden, o, ldo, o_lo, B, heads, L, scale, s); break;
    case 7: launch_ta<112>(qkv, ld, hidden, o, ldo, o_lo, B, heads, L, scale, s); break;
    default: launch_ta<128>(qkv, ld, hidden, o, ldo, o_lo, B, heads, L, scale, s); break;
  }
  HIP_CHECK(hipGetLastError());
}

void launch_text_ln(const f16* x_split, int M, int C, const float* gamma, const float* beta, float eps, void* out, int out_f16, f16* y_split, int* nonfinite, hipStream_t s) {
  LDIFF_CHECK(C % 8 == 0 && M >= 1, LDIFF_ERR_INVALID, "text_ln: C = %d must be a multiple of 8", C);
  ProfScope prof("text_ln", 8.0 * M * C, (double)M * C * 12.0, s);
  hipLaunchKernelGGL(text_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x_split, C, M, gamma, beta, eps, out, out_f16, y_split, nonfinite);
  HIP_CHECK(hipGetLastError());
}

void launch_f32_to_f16(const float* x, f16* y, long long n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(f32_to_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n);
  HIP_CHECK(hipGetLastError());
}
