// The warm-up trainer's dataset on the device (include/ldiff.h ldiff_op_label_table_u8 / _gather_labels / _warmup_labels / _warmup_images; python:
// ldiffusion_amd/dataset.py DeviceLoader).  The store is two uint8 arrays -- images [N, Hs, Ws, 3] already Pillow-resized, labels [N, H, W] already
// through the grey-level table -- and a batch is a list of indices into them:
//   * label_table_u8   bytes through a 256-entry table (the grey levels of a label file -> class indices);
//   * gather_labels    idx -> label uint8 [B, 1, H, W] and mask int64 [B, H, W], one launch;
//   * warmup_labels    idx -> uint8 [B, 1, oh, ow], torch's bilinear (align_corners=False) + truncation at integer ratios, in integers;
//   * warmup_images    idx -> float32 [B, 3, oh, ow]: table (ToTensor + Normalize) and the antialiased triangle reduction in one pass over the bytes: the
//                      float image of 12 MB per 1024^2 sample is never built.
// Every result of a sample is a function of that sample's bytes alone: no atomics, fixed summation order, nothing depends on B or the position in the batch.
// An index outside [0, N) is clamped into it (the caller validates on the host, where the indices are made); no read leaves the store whatever idx holds.
#include "common.h"

namespace {

__device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// ---- label_table_u8: 16 bytes per thread where source and destination are 16-byte aligned, bytes at the tail and otherwise ----
__global__ __launch_bounds__(256) void label_table_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long n, const uint8_t* __restrict__ table, int vec) {
  __shared__ uint8_t t[256];
  t[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
  if (i0 >= n) return;
  if (vec && i0 + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + i0);
    const uint32_t in[4] = {v.x, v.y, v.z, v.w};
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      o[k] = (uint32_t)t[in[k] & 255u] | ((uint32_t)t[(in[k] >> 8) & 255u] << 8) | ((uint32_t)t[(in[k] >> 16) & 255u] << 16) | ((uint32_t)t[in[k] >> 24] << 24);
    *reinterpret_cast<uint4*>(dst + i0) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
    const int m = n - i0 < 16 ? (int)(n - i0) : 16;
    for (int k = 0; k < m; ++k) dst[i0 + k] = t[src[i0 + k]];
  }
}

// ---- gather_labels: 4 pixels per thread (one 4-byte load, one 4-byte store, two 16-byte stores) where a plane is a multiple of 4 bytes ----
template <bool kVec>
__global__ __launch_bounds__(256) void gather_labels_kernel(const uint8_t* __restrict__ cache, int N, long long HW, const int* __restrict__ idx, uint8_t* __restrict__ label,
                                                            long long* __restrict__ mask) {
  const int b = blockIdx.y;
  const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= HW) return;
  const uint8_t* __restrict__ p = cache + (size_t)clamp_index(idx[b], N) * HW + i0;
  uint8_t* __restrict__ q = label + (size_t)b * HW + i0;
  long long* __restrict__ m = mask + (size_t)b * HW + i0;
  if (kVec) {   // HW % 4 == 0 and 4- / 16-byte aligned bases
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
    *reinterpret_cast<uint32_t*>(q) = w;
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    ll2 lo, hi;
    lo.x = w & 255u, lo.y = (w >> 8) & 255u, hi.x = (w >> 16) & 255u, hi.y = w >> 24;
    *reinterpret_cast<ll2*>(m) = lo;
    *reinterpret_cast<ll2*>(m + 2) = hi;
  } else {
    const int n = HW - i0 < 4 ? (int)(HW - i0) : 4;
    for (int k = 0; k < n; ++k) {
      const uint8_t v = p[k];
      q[k] = v;
      m[k] = v;
    }
  }
}

// ---- warmup_labels: one thread per output pixel; ry = H / oh, rx = W / ow exact ----
// torch's source coordinate (i + 0.5) * r - 0.5 is r*i + r/2 - 1 + 0.5 for an even r (weights 1/2, 1/2) and r*i + (r - 1)/2 for an odd one (weight 1 on it):
// with the second tap of an odd axis set to the first, the value is (a + b + c + d) / 4 exactly in float32, and .to(uint8) truncates it.
__global__ __launch_bounds__(256) void warmup_labels_kernel(const uint8_t* __restrict__ cache, int N, int H, int W, const int* __restrict__ idx, int oh, int ow, int ry, int rx,
                                                            uint8_t* __restrict__ out) {
  const int ox = blockIdx.x * 256 + threadIdx.x;
  const int oy = blockIdx.y, b = blockIdx.z;
  if (ox >= ow) return;
  const int y0 = (ry & 1) ? ry * oy + (ry - 1) / 2 : ry * oy + ry / 2 - 1, y1 = (ry & 1) ? y0 : y0 + 1;
  const int x0 = (rx & 1) ? rx * ox + (rx - 1) / 2 : rx * ox + rx / 2 - 1, x1 = (rx & 1) ? x0 : x0 + 1;
  const uint8_t* __restrict__ p = cache + (size_t)clamp_index(idx[b], N) * H * W;
  const int s = (int)p[(size_t)y0 * W + x0] + (int)p[(size_t)y0 * W + x1] + (int)p[(size_t)y1 * W + x0] + (int)p[(size_t)y1 * W + x1];
  out[((size_t)b * oh + oy) * ow + ox] = (uint8_t)(s >> 2);
}

// ---- warmup_images ----
// One workgroup per (column tile, output row, sample); a tile is 256 consecutive (ox, c) columns of the output row, one per lane.  The workgroup walks the source rows of
// its vertical window; each row's byte span [3 * x_lo, 3 * x_hi) -- what the tile's horizontal windows touch -- is staged once into LDS with 16-byte loads (the LDS copy
// keeps the global address's offset inside a 16-byte line, so head and tail bytes take the narrow path and the body is aligned on both sides); every lane then forms its
// horizontal sum from LDS in index order and adds it, times the row's vertical weight, to the accumulator it keeps in a register.
// LDS: [0, 3072) the table, [3072, 3072 + cap) the row.
constexpr int kTableBytes = 3 * 256 * 4;

__global__ __launch_bounds__(256) void warmup_images_kernel(const uint8_t* __restrict__ cache, int N, int Hs, int Ws, const int* __restrict__ idx, const float* __restrict__ table,
                                                            const int* __restrict__ ybounds, const float* __restrict__ ywts, int ytaps, const int* __restrict__ xbounds,
                                                            const float* __restrict__ xwts, int xtaps, int oh, int ow, int cap /* bytes of the row buffer */, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float* __restrict__ lut = reinterpret_cast<float*>(smem);
  uint8_t* __restrict__ row = smem + kTableBytes;
  const int tid = threadIdx.x;
  const int oy = blockIdx.y, b = blockIdx.z;
  const int ncol = 3 * ow;
  const int j0 = blockIdx.x * 256;
  const int j = j0 + tid;
  const bool live = j < ncol;
  for (int k = tid; k < 3 * 256; k += 256) lut[k] = table[k];

  // the span of source pixels this tile's windows touch (wave-uniform): windows are clamped into the source, then the span into the row buffer
  const int jl = j0 + 255 < ncol ? j0 + 255 : ncol - 1;
  int x_lo = Ws, x_hi = 0;
  for (int ox = j0 / 3; ox <= jl / 3; ++ox) {
    int f = xbounds[2 * ox], l = xbounds[2 * ox + 1];
    f = f < 0 ? 0 : (f > Ws - 1 ? Ws - 1 : f);
    l = l < 0 ? 0 : (l > xtaps ? xtaps : l);
    l = l > Ws - f ? Ws - f : l;
    x_lo = f < x_lo ? f : x_lo;
    x_hi = f + l > x_hi ? f + l : x_hi;
  }
  if (x_hi < x_lo) x_hi = x_lo;
  if ((long long)(x_hi - x_lo) * 3 + 16 > cap) x_hi = x_lo + (cap - 16) / 3;   // (never with tables that fit the launch's cap; keeps every LDS access inside the buffer)
  const int nbytes = (x_hi - x_lo) * 3;

  // this lane's horizontal window, inside the staged span
  int xf = 0, xl = 0, c = 0;
  const float* __restrict__ wx = xwts;
  if (live) {
    const int ox = j / 3;
    c = j - 3 * ox;
    xf = xbounds[2 * ox], xl = xbounds[2 * ox + 1];
    xf = xf < 0 ? 0 : (xf > Ws - 1 ? Ws - 1 : xf);
    xl = xl < 0 ? 0 : (xl > xtaps ? xtaps : xl);
    xl = xl > Ws - xf ? Ws - xf : xl;
    if (xf < x_lo) xf = x_lo;
    if (xf + xl > x_hi) xl = x_hi - xf > 0 ? x_hi - xf : 0;
    wx = xwts + (size_t)ox * xtaps;
  }
  int yf = ybounds[2 * oy], yl = ybounds[2 * oy + 1];
  yf = yf < 0 ? 0 : (yf > Hs - 1 ? Hs - 1 : yf);
  yl = yl < 0 ? 0 : (yl > ytaps ? ytaps : yl);
  yl = yl > Hs - yf ? Hs - yf : yl;
  const float* __restrict__ wy = ywts + (size_t)oy * ytaps;
  const uint8_t* __restrict__ img = cache + (size_t)clamp_index(idx[b], N) * Hs * Ws * 3;

  float acc = 0.f;
  for (int r = 0; r < yl; ++r) {
    const uint8_t* __restrict__ g = img + ((size_t)(yf + r) * Ws + x_lo) * 3;
    const int off = (int)((uintptr_t)g & 15);            // the LDS copy starts at the same offset inside a 16-byte line
    const int head = off ? (16 - off < nbytes ? 16 - off : nbytes) : 0;
    const int body = (nbytes - head) >> 4;               // whole 16-byte chunks
    const int tail0 = head + (body << 4);
    __syncthreads();                                     // the previous row's readers are done (first pass: the table is written)
    if (tid < head) row[off + tid] = g[tid];
    for (int k = tid; k < body; k += 256)
      *reinterpret_cast<uint4*>(row + off + head + (k << 4)) = *reinterpret_cast<const uint4*>(g + head + (k << 4));
    if (tid < nbytes - tail0) row[off + tail0 + tid] = g[tail0 + tid];
    __syncthreads();
    if (live) {
      const uint8_t* __restrict__ s = row + off + (xf - x_lo) * 3 + c;
      const float* __restrict__ l = lut + c * 256;
      float h = 0.f;
      for (int x = 0; x < xl; ++x) h += wx[x] * l[s[3 * x]];
      acc += wy[r] * h;
    }
  }
  if (live) {
    const int ox = j / 3;
    out[(((size_t)b * 3 + c) * oh + oy) * ow + ox] = acc;
  }
}

}  // namespace

void launch_label_table_u8(const uint8_t* src, uint8_t* dst, long long n, const uint8_t* table, hipStream_t s) {
  LDIFF_CHECK(src && dst && table, LDIFF_ERR_INVALID, "label_table_u8: src / dst / table is a null pointer");
  LDIFF_CHECK(n >= 0 && n <= (1ll << 40), LDIFF_ERR_INVALID, "label_table_u8: n = %lld outside 0 .. 2^40", n);
  if (n == 0) return;
  const int vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const long long blocks = (n + 4095) / 4096;
  label_table_kernel<<<dim3((unsigned)blocks), 256, 0, s>>>(src, dst, n, table, vec);
  HIP_CHECK(hipGetLastError());
}

static void check_store(const char* who, const void* cache, int N, int H, int W, const void* idx, int B) {
  LDIFF_CHECK(cache && idx, LDIFF_ERR_INVALID, "%s: cache / idx is a null pointer", who);
  LDIFF_CHECK(N >= 1, LDIFF_ERR_INVALID, "%s: N = %d: a store of at least one sample", who, N);
  LDIFF_CHECK(H >= 1 && W >= 1 && H <= 65535 && W <= (1 << 24), LDIFF_ERR_INVALID, "%s: H = %d, W = %d outside 1 .. 65535 x 1 .. 2^24", who, H, W);
  LDIFF_CHECK(B >= 1 && B <= 65535, LDIFF_ERR_INVALID, "%s: B = %d outside 1 .. 65535", who, B);
}

void launch_gather_labels(const uint8_t* cache, int N, int H, int W, const int* idx, int B, uint8_t* label, long long* mask, hipStream_t s) {
  check_store("gather_labels", cache, N, H, W, idx, B);
  LDIFF_CHECK(label && mask, LDIFF_ERR_INVALID, "gather_labels: label / mask is a null pointer");
  const long long HW = (long long)H * W;
  const dim3 grid((unsigned)((HW + 1023) / 1024), (unsigned)B);
  const bool vec = HW % 4 == 0 && (((uintptr_t)cache | (uintptr_t)label) & 3) == 0 && ((uintptr_t)mask & 15) == 0;
  if (vec) gather_labels_kernel<true><<<grid, 256, 0, s>>>(cache, N, HW, idx, label, mask);
  else gather_labels_kernel<false><<<grid, 256, 0, s>>>(cache, N, HW, idx, label, mask);
  HIP_CHECK(hipGetLastError());
}

int warmup_labels_supported(int H, int W, int oh, int ow) { return H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && H % oh == 0 && W % ow == 0; }

void launch_warmup_labels(const uint8_t* cache, int N, int H, int W, const int* idx, int B, int oh, int ow, uint8_t* out, hipStream_t s) {
  check_store("warmup_labels", cache, N, H, W, idx, B);
  LDIFF_CHECK(out, LDIFF_ERR_INVALID, "warmup_labels: out is a null pointer");
  LDIFF_CHECK(oh >= 1 && ow >= 1 && oh <= 65535, LDIFF_ERR_INVALID, "warmup_labels: oh = %d, ow = %d: sides of at least 1, oh at most 65535", oh, ow);
  LDIFF_CHECK(warmup_labels_supported(H, W, oh, ow), LDIFF_ERR_INVALID,
              "warmup_labels: %d x %d -> %d x %d is no integer ratio per axis (ldiff_op_warmup_labels_supported; torch's float32 result is the target there)", H, W, oh, ow);
  const dim3 grid((unsigned)((ow + 255) / 256), (unsigned)oh, (unsigned)B);
  warmup_labels_kernel<<<grid, 256, 0, s>>>(cache, N, H, W, idx, oh, ow, H / oh, W / ow, out);
  HIP_CHECK(hipGetLastError());
}

void launch_warmup_images(const uint8_t* cache, int N, int Hs, int Ws, const int* idx, int B, const float* table, const int* ybounds, const float* ywts, int ytaps, const int* xbounds,
                          const float* xwts, int xtaps, int oh, int ow, float* out, hipStream_t s) {
  check_store("warmup_images", cache, N, Hs, Ws, idx, B);
  LDIFF_CHECK(table && ybounds && ywts && xbounds && xwts && out, LDIFF_ERR_INVALID, "warmup_images: table / bounds / weights / out is a null pointer");
  LDIFF_CHECK(oh >= 1 && ow >= 1 && oh <= 65535 && ow <= (1 << 24), LDIFF_ERR_INVALID, "warmup_images: oh = %d, ow = %d outside 1 .. 65535 x 1 .. 2^24", oh, ow);
  LDIFF_CHECK(ytaps >= 1 && ytaps <= LDIFF_RESIZE_MAX_TAPS, LDIFF_ERR_INVALID, "warmup_images: ytaps = %d outside 1 .. %d", ytaps, LDIFF_RESIZE_MAX_TAPS);
  LDIFF_CHECK(xtaps >= 1 && xtaps <= LDIFF_RESIZE_MAX_TAPS, LDIFF_ERR_INVALID, "warmup_images: xtaps = %d outside 1 .. %d", xtaps, LDIFF_RESIZE_MAX_TAPS);
  // a tile's 256 columns are at most 87 output pixels; their windows span at most 87 steps of Ws / ow plus one window of xtaps, and never more than the row
  const double scale = (double)Ws / (double)ow;
  long long span = (long long)(87.0 * scale) + xtaps + 2;
  if (span > Ws) span = Ws;
  const long long cap = ((span * 3 + 15) / 16) * 16 + 32;   // + the offset inside a 16-byte line, + slack for the clamp
  LDIFF_CHECK(kTableBytes + cap <= 64 * 1024, LDIFF_ERR_INVALID, "warmup_images: Ws = %d -> ow = %d needs %lld bytes of LDS for a row span, 64 KiB are there", Ws, ow, kTableBytes + cap);
  const dim3 grid((unsigned)((3ll * ow + 255) / 256), (unsigned)oh, (unsigned)B);
  warmup_images_kernel<<<grid, 256, (size_t)(kTableBytes + cap), s>>>(cache, N, Hs, Ws, idx, table, ybounds, ywts, ytaps, xbounds, xwts, xtaps, oh, ow, (int)cap, out);
  HIP_CHECK(hipGetLastError());
}
