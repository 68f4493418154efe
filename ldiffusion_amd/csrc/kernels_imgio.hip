// Device image front end (include/ldiff.h ldiff_op_resize_u8): PIL.Image.resize(size, BILINEAR) of 8-bit interleaved images, bit for bit.
// Pillow's rule for 8-bit data is integer arithmetic on coefficient tables that the HOST makes in double (ldiffusion_amd/imgio.py, one table per
// (in, out) pair); the kernels only apply them:  out = clip((2^21 + sum_j k[j] * src[first + j]) >> 22, 0, 255), the horizontal pass first, the
// intermediate rounded and clipped to uint8 between the passes, a pass skipped when its side does not change.
// Two launches, the uint8 intermediate [B, Hs, Wo, C] in a caller-owned scratch buffer in global memory (DESIGN.md "Dataset pass" says why not LDS).
#include "common.h"

namespace {

constexpr int kPrecisionBits = 22;
constexpr int kRound = 1 << (kPrecisionBits - 1);

__device__ __forceinline__ int clip8(int acc) {
  acc >>= kPrecisionBits;
  return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// the window of one output index, made safe against a table that does not fit the source: every read stays inside [0, n_in)
__device__ __forceinline__ void window(const int* __restrict__ bounds, int idx, int n_in, int taps, int& first, int& len) {
  first = bounds[2 * idx];
  len = bounds[2 * idx + 1];
  first = first < 0 ? 0 : (first > n_in - 1 ? n_in - 1 : first);
  len = len < 0 ? 0 : len;
  len = len > taps ? taps : len;
  len = len > n_in - first ? n_in - first : len;
}

// horizontal pass: one thread per output pixel (all C channels); src [rows, Ws, C] -> dst [rows, Wo, C], rows = B * Hs
template <int C>
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long rows, int Ws, int Wo,
                                                       const int* __restrict__ bounds, const int* __restrict__ coef, int taps) {
  const int xx = blockIdx.x * 256 + threadIdx.x;
  const long long row = blockIdx.y;
  if (xx >= Wo || row >= rows) return;
  int first, len;
  window(bounds, xx, Ws, taps, first, len);
  const int* __restrict__ k = coef + (size_t)xx * taps;
  const uint8_t* __restrict__ p = src + ((size_t)row * Ws + first) * C;
  int acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = kRound;
  for (int j = 0; j < len; ++j) {
    const int kj = k[j];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += kj * (int)p[(size_t)j * C + c];
  }
  uint8_t* __restrict__ q = dst + ((size_t)row * Wo + xx) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) q[c] = (uint8_t)clip8(acc[c]);
}

// vertical pass over the BYTES of a row (a column of bytes is a column of one channel): one thread per 4 consecutive bytes of an output row, one
// output row per blockIdx.y (its window and coefficients are wave-uniform), one image per blockIdx.z.  src [B, Hs, rowb] -> u8 dst [B, Ho, rowb], or
// with a table lut [3][256] -> float dst [B, 3, Ho, Wo] (rowb = Wo * 3).  bounds == nullptr: the identity (Ho == Hs), for the table form alone.
template <bool kAligned, bool kLut>
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst, int Hs, int Ho, int rowb, const int* __restrict__ bounds,
                                                       const int* __restrict__ coef, int taps, const float* __restrict__ lut) {
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int yy = blockIdx.y, b = blockIdx.z;
  if (i0 >= rowb) return;
  const int nb = rowb - i0 < 4 ? rowb - i0 : 4;
  int first = yy, len = 1;
  if (bounds) window(bounds, yy, Hs, taps, first, len);
  const int* __restrict__ k = coef ? coef + (size_t)yy * taps : nullptr;
  const uint8_t* __restrict__ p = src + ((size_t)b * Hs + first) * rowb + i0;
  int v[4];
  if (bounds) {
    int acc[4] = {kRound, kRound, kRound, kRound};
    for (int j = 0; j < len; ++j) {
      const int kj = k[j];
      const uint8_t* __restrict__ r = p + (size_t)j * rowb;
      if (kAligned) {   // rowb % 4 == 0 and a 4-byte aligned base: nb == 4 for every thread
        const uint32_t w = *reinterpret_cast<const uint32_t*>(r);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] += kj * (int)((w >> (8 * t)) & 255u);
      } else {
        for (int t = 0; t < nb; ++t) acc[t] += kj * (int)r[t];
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = clip8(acc[t]);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = t < nb ? (int)p[t] : 0;
  }
  if (kLut) {
    const int Wo = rowb / 3;
    float* __restrict__ out = (float*)dst;
    for (int t = 0; t < nb; ++t) {
      const int i = i0 + t, x = i / 3, c = i - 3 * x;
      out[(((size_t)b * 3 + c) * Ho + yy) * Wo + x] = lut[c * 256 + v[t]];
    }
  } else {
    uint8_t* __restrict__ q = (uint8_t*)dst + ((size_t)b * Ho + yy) * rowb + i0;
    if (kAligned) *reinterpret_cast<uint32_t*>(q) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    else for (int t = 0; t < nb; ++t) q[t] = (uint8_t)v[t];
  }
}

}  // namespace

long long resize_u8_ws_bytes(int B, int Hs, int Ws, int C, int Ho, int Wo, int to_float) {
  if (B < 1 || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || (C != 1 && C != 3)) return -1;
  return (Wo != Ws && (Ho != Hs || to_float)) ? (long long)B * Hs * Wo * C : 0;
}

void launch_resize_u8(const uint8_t* x, int B, int Hs, int Ws, int C, int Ho, int Wo, const int* hbounds, const int* hcoef, int htaps, const int* vbounds, const int* vcoef,
                      int vtaps, const float* lut, void* out, void* ws, long long ws_bytes, hipStream_t s) {
  LDIFF_CHECK(x && out, LDIFF_ERR_INVALID, "resize_u8: x / out is a null pointer");
  LDIFF_CHECK(C == 1 || C == 3, LDIFF_ERR_INVALID, "resize_u8: C = %d: 1 or 3 interleaved channels", C);
  LDIFF_CHECK(!lut || C == 3, LDIFF_ERR_INVALID, "resize_u8: lut (the float [B, 3, Ho, Wo] output) needs C = 3, got C = %d", C);
  LDIFF_CHECK(B >= 1 && B <= 65535, LDIFF_ERR_INVALID, "resize_u8: B = %d outside 1 .. 65535", B);
  LDIFF_CHECK(Hs >= 1 && Ws >= 1, LDIFF_ERR_INVALID, "resize_u8: source side of 0 (Hs = %d, Ws = %d)", Hs, Ws);
  LDIFF_CHECK(Ho >= 1 && Wo >= 1, LDIFF_ERR_INVALID, "resize_u8: output side of 0 (Ho = %d, Wo = %d)", Ho, Wo);
  LDIFF_CHECK(Hs <= 65535 && Ho <= 65535 && Ws <= (1 << 24) && Wo <= (1 << 24), LDIFF_ERR_INVALID, "resize_u8: a height above 65535 or a width above 2^24 (Hs = %d, Ws = %d, Ho = %d, Wo = %d)",
              Hs, Ws, Ho, Wo);
  const bool need_h = Wo != Ws, need_v = Ho != Hs;
  LDIFF_CHECK(!need_h || (hbounds && hcoef), LDIFF_ERR_INVALID, "resize_u8: hbounds / hcoef missing for Ws = %d -> Wo = %d", Ws, Wo);
  LDIFF_CHECK(!need_v || (vbounds && vcoef), LDIFF_ERR_INVALID, "resize_u8: vbounds / vcoef missing for Hs = %d -> Ho = %d", Hs, Ho);
  LDIFF_CHECK(!need_h || (htaps >= 1 && htaps <= LDIFF_RESIZE_MAX_TAPS), LDIFF_ERR_INVALID, "resize_u8: htaps = %d outside 1 .. %d (a window longer than the kernel supports)", htaps,
              LDIFF_RESIZE_MAX_TAPS);
  LDIFF_CHECK(!need_v || (vtaps >= 1 && vtaps <= LDIFF_RESIZE_MAX_TAPS), LDIFF_ERR_INVALID, "resize_u8: vtaps = %d outside 1 .. %d (a window longer than the kernel supports)", vtaps,
              LDIFF_RESIZE_MAX_TAPS);
  const long long need = resize_u8_ws_bytes(B, Hs, Ws, C, Ho, Wo, lut != nullptr);
  LDIFF_CHECK(need == 0 || (ws && ws_bytes >= need), LDIFF_ERR_INVALID, "resize_u8: ws of %lld bytes, %lld needed (ldiff_op_resize_u8_ws_bytes)", ws_bytes, need);
  const long long rows = (long long)B * Hs;
  const bool second = need_v || lut;   // a launch of the vertical kernel follows the horizontal pass
  const uint8_t* mid = x;
  if (need_h) {
    uint8_t* hdst = second ? (uint8_t*)ws : (uint8_t*)out;
    // rows on grid.y in slices of at most 65535
    for (long long r0 = 0; r0 < rows; r0 += 65535) {
      const long long nr = rows - r0 < 65535 ? rows - r0 : 65535;
      const dim3 grid((unsigned)((Wo + 255) / 256), (unsigned)nr);
      const uint8_t* xs = x + (size_t)r0 * Ws * C;
      uint8_t* ds = hdst + (size_t)r0 * Wo * C;
      if (C == 3) resize_h_kernel<3><<<grid, 256, 0, s>>>(xs, ds, nr, Ws, Wo, hbounds, hcoef, htaps);
      else resize_h_kernel<1><<<grid, 256, 0, s>>>(xs, ds, nr, Ws, Wo, hbounds, hcoef, htaps);
      HIP_CHECK(hipGetLastError());
    }
    mid = hdst;
  }
  if (second) {
    const int rowb = Wo * C;
    const dim3 grid((unsigned)((rowb + 1023) / 1024), (unsigned)Ho, (unsigned)B);
    const int* vb = need_v ? vbounds : nullptr;
    const int* vc = need_v ? vcoef : nullptr;
    const bool aligned = rowb % 4 == 0 && ((uintptr_t)mid & 3) == 0 && (lut || ((uintptr_t)out & 3) == 0);
    if (lut) {
      if (aligned) resize_v_kernel<true, true><<<grid, 256, 0, s>>>(mid, out, Hs, Ho, rowb, vb, vc, vtaps, lut);
      else resize_v_kernel<false, true><<<grid, 256, 0, s>>>(mid, out, Hs, Ho, rowb, vb, vc, vtaps, lut);
    } else {
      if (aligned) resize_v_kernel<true, false><<<grid, 256, 0, s>>>(mid, out, Hs, Ho, rowb, vb, vc, vtaps, nullptr);
      else resize_v_kernel<false, false><<<grid, 256, 0, s>>>(mid, out, Hs, Ho, rowb, vb, vc, vtaps, nullptr);
    }
    HIP_CHECK(hipGetLastError());
  } else if (!need_h) {   // both sides unchanged, uint8 out: a copy, as Image.resize returns one
    HIP_CHECK(hipMemcpyAsync(out, x, (size_t)B * Hs * Ws * C, hipMemcpyDeviceToDevice, s));
  }
}
