// Batched sliding window of the nnU-Net tissue head (include/ldiff.h "Tissue head, batched sliding window"): what
// nnUNetPredictor.predict_sliding_window_return_logits does per tile and mirror variant in ATen ops (predict_from_raw_data.py:530-545 mirroring,
// :563-570 accumulation, :572-589 division, inf check and revert of the padding), in three bandwidth-bound element kernels per image:
//   gather      a chunk of tiles x mirror variants out of the (virtually zero padded) image -> the network's NCHW float32 batch
//   accumulate  un-flip, average the variants, weight and add a whole chunk; one thread owns its pixels and walks the chunk's tiles in slicer order
//   finish      logits = acc / cnt, inf flag, arg-max, written at the crop box's place of the full-size mask; for several folds, their mean in between
// The chunk (tile origins, variant masks) is a kernel argument: the indices below read the kernarg segment, nothing is copied to the device.
// Every float operation is rounded on its own, in the order the tensor formulation rounds (see the header): contraction is off for the whole file.
#include <type_traits>

#include "common.h"
#pragma clang fp contract(off)

namespace {

inline int nblocks(long long n) { return (int)((n + 255) / 256); }

// a run of VEC adjacent elements along x as floats; VEC == 4 is one aligned 8- or 16-byte access (the launchers check the alignment)
template <typename E, int VEC>
__device__ inline void load_run(const E* __restrict__ p, float (&o)[VEC]) {
  if constexpr (VEC == 1) {
    o[0] = (float)p[0];
  } else {
    typedef E V __attribute__((ext_vector_type(4)));
    const V v = *reinterpret_cast<const V*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (float)v[j];
  }
}
template <typename E, int VEC>
__device__ inline void store_run(E* __restrict__ p, const float (&o)[VEC]) {
  if constexpr (VEC == 1) {
    p[0] = (E)o[0];
  } else {
    typedef E V __attribute__((ext_vector_type(4)));
    V v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (E)o[j];
    *reinterpret_cast<V*>(p) = v;
  }
}
template <typename E> __device__ inline float rnd(float v) { return (float)(E)v; }   // one rounding to E (the identity for float)
// The correctly rounded float32 quotient as a value of its own: without the (empty) barrier the compiler folds widen -> divide -> narrow of float16
// operands into its float16 division sequence; with it the result is rn16(rn32(a / b)), which equals the correctly rounded float16 quotient
// (24 >= 2 * 11 + 2 bits: the double rounding is innocuous) whatever that sequence does.
__device__ inline float div_rn(float a, float b) {
  float q = __fdiv_rn(a, b);
  asm volatile("" : "+v"(q));
  return q;
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------------------
// One thread per run of VEC outputs along x: x[k, v, c, y, xo .. xo + VEC) <- the padded image at the (flipped) tile coordinate, 0 in the pad.
// The source has no alignment (pad offsets and origins are arbitrary), so it is read by element -- a wave still reads one contiguous piece of a row,
// reversed or not -- and the batch is written in whole vectors.
template <int VEC>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ img, int C, int h, int w, long long rs, long long ps, int pad_top, int pad_left,
                                                            ldiff_window_tiles t, int th, int tw, float* __restrict__ x, long long runs) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= runs) return;
  const int rw = tw / VEC;
  long long r = i / rw;
  const int xo = (int)(i - r * rw) * VEC;
  const int y = (int)(r % th); r /= th;
  const int c = (int)(r % C); r /= C;
  const int v = (int)(r % t.n_variants), k = (int)(r / t.n_variants);
  const int m = t.variants[v];
  const int sy = t.y0[k] + ((m & 1) ? th - 1 - y : y) - pad_top;   // row and column in the unpadded image
  const int sx0 = t.x0[k] - pad_left;
  const float* row = img + (long long)c * ps + (long long)sy * rs;
  float o[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int sx = sx0 + ((m & 2) ? tw - 1 - (xo + j) : xo + j);
    o[j] = (sy >= 0 && sy < h && sx >= 0 && sx < w) ? row[sx] : 0.f;
  }
  store_run<float, VEC>(x + i * VEC, o);
}

// ---- accumulate -----------------------------------------------------------------------------------------------------------------------------
// T: accumulators and weight, P: prediction.  One thread per run of VEC pixels of the bounding box (by0, bx0, bh rows, bwr runs per row) of the
// chunk's valid tiles.  With VEC == 4 every x0, bx0, tw and Wp is a multiple of 4, so a run lies wholly inside or outside a tile and each access
// is one aligned vector; a flipped variant reads the mirrored vector and reverses it in registers.
template <typename T, int VEC>
__device__ inline bool tile_weight(const ldiff_window_tiles& t, int k, int py, int px, int th, int tw, const T* __restrict__ g, int& ty, int& tx, float (&gv)[VEC]) {
  ty = py - t.y0[k];
  tx = px - t.x0[k];
  if (ty < 0 || ty >= th || tx < 0 || tx >= tw) return false;
  if (g) load_run<T, VEC>(g + (long long)ty * tw + tx, gv);
  else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) gv[j] = 1.0f;
  }
  return true;
}

template <typename T, typename P, int VEC>
__global__ __launch_bounds__(256) void window_accumulate_batch_kernel(T* __restrict__ acc, T* __restrict__ cnt, const P* __restrict__ pred, const T* __restrict__ g, int heads,
                                                                      int Hp, int Wp, int th, int tw, ldiff_window_tiles t, int by0, int bx0, int bh, int bwr) {
  // the product has the promoted type of (prediction, weight): float16 only when both are (window_accumulate_kernel's rule; a float16 prediction
  // into float32 accumulators is averaged in float16 and widened first)
  using PP = typename std::conditional<std::is_same<T, f16>::value && std::is_same<P, f16>::value, f16, float>::type;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)bh * bwr) return;
  const int ry = (int)(i / bwr);
  const int py = by0 + ry, px = bx0 + (int)(i - (long long)ry * bwr) * VEC;
  const long long o = (long long)py * Wp + px, img_plane = (long long)Hp * Wp;
  const int M = t.n_variants;
  const float fM = (float)M;
  int ty, tx;
  float gv[VEC];
  for (int c = 0; c < heads; ++c) {
    float a[VEC];
    load_run<T, VEC>(acc + c * img_plane + o, a);
    for (int k = 0; k < t.n_valid; ++k) {
      if (!tile_weight<T, VEC>(t, k, py, px, th, tw, g, ty, tx, gv)) continue;
      float p[VEC];
      for (int v = 0; v < M; ++v) {
        const int m = t.variants[v];
        const P* row = pred + ((((long long)k * M + v) * heads + c) * th + ((m & 1) ? th - 1 - ty : ty)) * tw;
        float q[VEC];
        if (m & 2) {   // pixel tx + j is element tw - 1 - tx - j of the flipped prediction: the run [tw - VEC - tx, tw - tx), reversed
          float rq[VEC];
          load_run<P, VEC>(row + (tw - VEC - tx), rq);
#pragma unroll
          for (int j = 0; j < VEC; ++j) q[j] = rq[VEC - 1 - j];
        } else {
          load_run<P, VEC>(row + tx, q);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) p[j] = v == 0 ? q[j] : rnd<P>(__fadd_rn(p[j], q[j]));
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (M > 1) p[j] = rnd<P>(div_rn(p[j], fM));
        const float prod = g ? rnd<PP>(__fmul_rn(p[j], gv[j])) : p[j];
        a[j] = rnd<T>(__fadd_rn(a[j], prod));
      }
    }
    store_run<T, VEC>(acc + c * img_plane + o, a);
  }
  float n[VEC];
  load_run<T, VEC>(cnt + o, n);
  for (int k = 0; k < t.n_valid; ++k) {
    if (!tile_weight<T, VEC>(t, k, py, px, th, tw, g, ty, tx, gv)) continue;
#pragma unroll
    for (int j = 0; j < VEC; ++j) n[j] = rnd<T>(__fadd_rn(n[j], gv[j]));
  }
  store_run<T, VEC>(cnt + o, n);
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------------------
// One thread per run of VEC pixels of the h x w box at (y0, x0) of the padded extent.  The arg-max is argmax_u8_kernel's (kernels_elem.hip): the
// first maximal class, and class 0 for a pixel with any NaN or +inf logit.
// Both finish kernels run these two steps; they are macros, so that each kernel compiles exactly the statements it would hold written out.
// One class c of pixel j into the run's arg-max: the first maximal class wins, and bad[j] remembers a NaN or +inf logit (the pixel is class 0 then).
#define WINDOW_ARGMAX_TAKE(c, l, j)                                    \
  {                                                                    \
    const bool nan_or_inf = l[j] != l[j] || l[j] == INFINITY;          \
    if (c == 0) { best[j] = l[j]; bi[j] = 0; bad[j] = nan_or_inf; }    \
    else {                                                             \
      bad[j] |= nan_or_inf;                                            \
      if (l[j] > best[j]) { best[j] = l[j]; bi[j] = c; }               \
    }                                                                  \
  }
// The run's classes as bytes at pixel (y, x) of the mask box; VEC == 4 is one aligned 4-byte store (the launchers check the alignment).
#define WINDOW_ARGMAX_STORE()                                                                 \
  if (mask) {                                                                                 \
    uint8_t* mp = mask + (long long)(mask_y0 + y) * mask_W + mask_x0 + x;                     \
    if constexpr (VEC == 1) mp[0] = bad[0] ? (uint8_t)0 : (uint8_t)bi[0];                     \
    else {                                                                                    \
      unsigned u = 0;                                                                         \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) u |= (bad[j] ? 0u : (unsigned)bi[j]) << (8 * j); \
      *reinterpret_cast<unsigned*>(mp) = u;                                                   \
    }                                                                                         \
  }

template <typename T, int VEC>
__global__ __launch_bounds__(256) void window_finish_kernel(const T* __restrict__ acc, const T* __restrict__ cnt, int heads, int Hp, int Wp, int y0, int x0, int h, int w,
                                                            T* __restrict__ logits, uint8_t* __restrict__ mask, int mask_W, int mask_y0, int mask_x0,
                                                            int32_t* __restrict__ inf_flag) {
  const int rw = w / VEC;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)h * rw) return;
  const int y = (int)(i / rw), x = (int)(i - (long long)y * rw) * VEC;
  const long long o = (long long)(y0 + y) * Wp + x0 + x, img_plane = (long long)Hp * Wp, out_plane = (long long)h * w, oo = (long long)y * w + x;
  float n[VEC], best[VEC];
  int bi[VEC];
  bool bad[VEC], any_inf = false;
  load_run<T, VEC>(cnt + o, n);
  for (int c = 0; c < heads; ++c) {
    float l[VEC];
    load_run<T, VEC>(acc + c * img_plane + o, l);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      l[j] = rnd<T>(div_rn(l[j], n[j]));
      any_inf |= l[j] == INFINITY || l[j] == -INFINITY;
      WINDOW_ARGMAX_TAKE(c, l, j)
    }
    if (logits) store_run<T, VEC>(logits + c * out_plane + oo, l);
  }
  if (any_inf) *inf_flag = 1;   // every writer stores the same value
  WINDOW_ARGMAX_STORE()
}

// ---- finish of a fold ensemble --------------------------------------------------------------------------------------------------------------
// The folds' accumulators (or, without a count plane, their finished logits) of one image: each fold's logits as window_finish_kernel makes them, the
// inf flag per fold, then the sum in fold order and the division by the fold count, every step rounded to T (predict_from_raw_data.py:459-494:
// `prediction += logits` and `prediction /= n` on tensors of that type).  The pointer table is a kernel argument, like the chunk of tiles above.
struct window_fold_table { const void* acc[LDIFF_ENSEMBLE_MAX_FOLDS]; };

template <typename T, int VEC>
__global__ __launch_bounds__(256) void window_finish_ensemble_kernel(window_fold_table t, int n_folds, const T* __restrict__ cnt, int heads, int Hp, int Wp, int y0, int x0,
                                                                     int h, int w, T* __restrict__ logits, uint8_t* __restrict__ mask, int mask_W, int mask_y0, int mask_x0,
                                                                     int32_t* __restrict__ inf_flag) {
  const int rw = w / VEC;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)h * rw) return;
  const int y = (int)(i / rw), x = (int)(i - (long long)y * rw) * VEC;
  const long long o = (long long)(y0 + y) * Wp + x0 + x, img_plane = (long long)Hp * Wp, out_plane = (long long)h * w, oo = (long long)y * w + x;
  const float fK = (float)n_folds;
  // The arg-max state starts defined, and `bad` is a word: left as an unset bool for class 0 to set, the element path's flag came out of a scalar register
  // pair that nothing writes (profiles/segwin_ensemble_flag_codegen.txt has the assembly and how to see it again).
  float n[VEC], best[VEC] = {};
  int bi[VEC] = {};
  unsigned bad[VEC] = {};
  bool any_inf = false;
  if (cnt) load_run<T, VEC>(cnt + o, n);
  for (int c = 0; c < heads; ++c) {
    float s[VEC];
    for (int k = 0; k < n_folds; ++k) {
      float l[VEC];
      load_run<T, VEC>((const T*)t.acc[k] + c * img_plane + o, l);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (cnt) l[j] = rnd<T>(div_rn(l[j], n[j]));
        any_inf |= l[j] == INFINITY || l[j] == -INFINITY;
        s[j] = k == 0 ? l[j] : rnd<T>(__fadd_rn(s[j], l[j]));
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if (n_folds > 1) s[j] = rnd<T>(div_rn(s[j], fK));
      WINDOW_ARGMAX_TAKE(c, s, j)
    }
    if (logits) store_run<T, VEC>(logits + c * out_plane + oo, s);
  }
  if (any_inf) *inf_flag = 1;   // every writer stores the same value
  WINDOW_ARGMAX_STORE()
}

// what every launch checks of its chunk: the counts, the variant masks and that tiles 0 .. n - 1 lie inside the padded extent
void check_tiles(const char* who, const ldiff_window_tiles& t, int n, int Hp, int Wp, int th, int tw) {
  LDIFF_CHECK(t.n_tiles >= 1 && t.n_tiles <= LDIFF_WINDOW_MAX_TILES, LDIFF_ERR_INVALID, "%s: n_tiles %d out of range [1, %d] (tiles of one launch)", who, t.n_tiles,
              LDIFF_WINDOW_MAX_TILES);
  LDIFF_CHECK(t.n_valid >= 0 && t.n_valid <= t.n_tiles, LDIFF_ERR_INVALID, "%s: n_valid %d out of range [0, n_tiles = %d]", who, t.n_valid, t.n_tiles);
  LDIFF_CHECK(t.n_variants == 1 || t.n_variants == 2 || t.n_variants == 4, LDIFF_ERR_INVALID, "%s: n_variants %d is not 1, 2 or 4", who, t.n_variants);
  for (int v = 0; v < t.n_variants; ++v)
    LDIFF_CHECK(t.variants[v] >= 0 && t.variants[v] <= 3, LDIFF_ERR_INVALID, "%s: variants[%d] = %d is no 2-bit flip mask", who, v, t.variants[v]);
  LDIFF_CHECK(th >= 1 && tw >= 1 && th <= Hp && tw <= Wp, LDIFF_ERR_INVALID, "%s: tile %d x %d does not fit the padded extent %d x %d", who, th, tw, Hp, Wp);
  for (int k = 0; k < n; ++k)
    LDIFF_CHECK(t.y0[k] >= 0 && t.x0[k] >= 0 && t.y0[k] <= Hp - th && t.x0[k] <= Wp - tw, LDIFF_ERR_INVALID,
                "%s: tile %d (%d x %d at y0 = %d, x0 = %d) leaves the padded extent %d x %d", who, k, th, tw, t.y0[k], t.x0[k], Hp, Wp);
}

inline bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

template <typename T, typename P>
void accumulate_batch(void* acc, void* cnt, const void* pred, const void* g, int heads, int Hp, int Wp, int th, int tw, const ldiff_window_tiles& t, hipStream_t s) {
  int y_lo = t.y0[0], y_hi = t.y0[0], x_lo = t.x0[0], x_hi = t.x0[0];
  bool vec = tw % 4 == 0 && Wp % 4 == 0 && aligned16(acc) && aligned16(cnt) && aligned16(pred) && aligned16(g);
  for (int k = 0; k < t.n_valid; ++k) {
    y_lo = t.y0[k] < y_lo ? t.y0[k] : y_lo; y_hi = t.y0[k] > y_hi ? t.y0[k] : y_hi;
    x_lo = t.x0[k] < x_lo ? t.x0[k] : x_lo; x_hi = t.x0[k] > x_hi ? t.x0[k] : x_hi;
    vec = vec && t.x0[k] % 4 == 0;
  }
  const int bh = y_hi - y_lo + th, bw = x_hi - x_lo + tw;
  if (vec)
    hipLaunchKernelGGL((window_accumulate_batch_kernel<T, P, 4>), dim3(nblocks((long long)bh * (bw / 4))), dim3(256), 0, s, (T*)acc, (T*)cnt, (const P*)pred, (const T*)g,
                       heads, Hp, Wp, th, tw, t, y_lo, x_lo, bh, bw / 4);
  else
    hipLaunchKernelGGL((window_accumulate_batch_kernel<T, P, 1>), dim3(nblocks((long long)bh * bw)), dim3(256), 0, s, (T*)acc, (T*)cnt, (const P*)pred, (const T*)g, heads,
                       Hp, Wp, th, tw, t, y_lo, x_lo, bh, bw);
}

template <typename T>
void finish(const void* acc, const void* cnt, int heads, int Hp, int Wp, int y0, int x0, int h, int w, void* logits, uint8_t* mask, int mask_W, int mask_y0, int mask_x0,
            int32_t* inf_flag, hipStream_t s) {
  const bool vec = w % 4 == 0 && Wp % 4 == 0 && x0 % 4 == 0 && aligned16(acc) && aligned16(cnt) && aligned16(logits) &&
                   (!mask || (mask_W % 4 == 0 && mask_x0 % 4 == 0 && ((size_t)mask & 3) == 0));
  if (vec)
    hipLaunchKernelGGL((window_finish_kernel<T, 4>), dim3(nblocks((long long)h * (w / 4))), dim3(256), 0, s, (const T*)acc, (const T*)cnt, heads, Hp, Wp, y0, x0, h, w,
                       (T*)logits, mask, mask_W, mask_y0, mask_x0, inf_flag);
  else
    hipLaunchKernelGGL((window_finish_kernel<T, 1>), dim3(nblocks((long long)h * w)), dim3(256), 0, s, (const T*)acc, (const T*)cnt, heads, Hp, Wp, y0, x0, h, w, (T*)logits,
                       mask, mask_W, mask_y0, mask_x0, inf_flag);
}

template <typename T>
void finish_ensemble(const window_fold_table& t, int n_folds, const void* cnt, int heads, int Hp, int Wp, int y0, int x0, int h, int w, void* logits, uint8_t* mask, int mask_W,
                     int mask_y0, int mask_x0, int32_t* inf_flag, hipStream_t s) {
  bool vec = w % 4 == 0 && Wp % 4 == 0 && x0 % 4 == 0 && aligned16(cnt) && aligned16(logits) &&
             (!mask || (mask_W % 4 == 0 && mask_x0 % 4 == 0 && ((size_t)mask & 3) == 0));
  for (int k = 0; k < n_folds; ++k) vec = vec && aligned16(t.acc[k]);
  if (vec)
    hipLaunchKernelGGL((window_finish_ensemble_kernel<T, 4>), dim3(nblocks((long long)h * (w / 4))), dim3(256), 0, s, t, n_folds, (const T*)cnt, heads, Hp, Wp, y0, x0, h, w,
                       (T*)logits, mask, mask_W, mask_y0, mask_x0, inf_flag);
  else
    hipLaunchKernelGGL((window_finish_ensemble_kernel<T, 1>), dim3(nblocks((long long)h * w)), dim3(256), 0, s, t, n_folds, (const T*)cnt, heads, Hp, Wp, y0, x0, h, w,
                       (T*)logits, mask, mask_W, mask_y0, mask_x0, inf_flag);
}

}  // namespace

void launch_window_gather(const float* img, int C, int h, int w, long long row_stride, long long plane_stride, int pad_top, int pad_left, int Hp, int Wp,
                          const ldiff_window_tiles& tiles, int th, int tw, float* x, hipStream_t s) {
  const char* who = "window_gather";
  check_tiles(who, tiles, tiles.n_tiles, Hp, Wp, th, tw);
  LDIFF_CHECK(C >= 1 && h >= 1 && w >= 1 && row_stride >= w && plane_stride >= (long long)(h - 1) * row_stride + w, LDIFF_ERR_INVALID,
              "%s: image [%d, %d, %d] with row_stride %lld and plane_stride %lld", who, C, h, w, row_stride, plane_stride);
  LDIFF_CHECK(pad_top >= 0 && pad_left >= 0 && pad_top + h <= Hp && pad_left + w <= Wp, LDIFF_ERR_INVALID,
              "%s: the image %d x %d at pad offsets (%d, %d) leaves the padded extent %d x %d", who, h, w, pad_top, pad_left, Hp, Wp);
  const long long elems = (long long)tiles.n_tiles * tiles.n_variants * C * th * tw;
  LDIFF_CHECK(elems / 256 < 0x7fffffffLL, LDIFF_ERR_INVALID, "%s: a batch of %lld elements is too large for one launch", who, elems);
  if (tw % 4 == 0 && aligned16(x))
    hipLaunchKernelGGL(window_gather_kernel<4>, dim3(nblocks(elems / 4)), dim3(256), 0, s, img, C, h, w, row_stride, plane_stride, pad_top, pad_left, tiles, th, tw, x, elems / 4);
  else
    hipLaunchKernelGGL(window_gather_kernel<1>, dim3(nblocks(elems)), dim3(256), 0, s, img, C, h, w, row_stride, plane_stride, pad_top, pad_left, tiles, th, tw, x, elems);
  HIP_CHECK(hipGetLastError());
}

void launch_window_accumulate_batch(void* acc, void* cnt, const void* pred, const void* g, int heads, int Hp, int Wp, int th, int tw, const ldiff_window_tiles& tiles,
                                    int dtypes, hipStream_t s) {
  const char* who = "window_accumulate_batch";
  LDIFF_CHECK(heads >= 1 && heads <= 32, LDIFF_ERR_INVALID, "%s: heads %d out of range [1, 32]", who, heads);
  LDIFF_CHECK(dtypes >= 0 && dtypes <= 3, LDIFF_ERR_INVALID,
              "%s: dtypes 0 (all float32), 1 (all float16), 2 (float32 accumulators, float16 prediction) or 3 (float16 accumulators, float32 prediction), not %d", who, dtypes);
  LDIFF_CHECK(Hp >= 1 && Wp >= 1, LDIFF_ERR_INVALID, "%s: padded extent %d x %d", who, Hp, Wp);
  check_tiles(who, tiles, tiles.n_valid, Hp, Wp, th, tw);
  if (tiles.n_valid == 0) return;
  if (dtypes == 0) accumulate_batch<float, float>(acc, cnt, pred, g, heads, Hp, Wp, th, tw, tiles, s);
  else if (dtypes == 1) accumulate_batch<f16, f16>(acc, cnt, pred, g, heads, Hp, Wp, th, tw, tiles, s);
  else if (dtypes == 2) accumulate_batch<float, f16>(acc, cnt, pred, g, heads, Hp, Wp, th, tw, tiles, s);
  else accumulate_batch<f16, float>(acc, cnt, pred, g, heads, Hp, Wp, th, tw, tiles, s);
  HIP_CHECK(hipGetLastError());
}

void launch_window_finish(const void* acc, const void* cnt, int heads, int Hp, int Wp, int y0, int x0, int h, int w, int acc_f16, void* logits, uint8_t* mask, int mask_H,
                          int mask_W, int mask_y0, int mask_x0, int32_t* inf_flag, hipStream_t s) {
  const char* who = "window_finish";
  LDIFF_CHECK(heads >= 1 && heads <= 32, LDIFF_ERR_INVALID, "%s: heads %d out of range [1, 32]", who, heads);
  LDIFF_CHECK(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 <= Hp - h && x0 <= Wp - w, LDIFF_ERR_INVALID, "%s: the box %d x %d at (y0 = %d, x0 = %d) leaves the padded extent %d x %d",
              who, h, w, y0, x0, Hp, Wp);
  LDIFF_CHECK(!mask || (mask_y0 >= 0 && mask_x0 >= 0 && mask_y0 <= mask_H - h && mask_x0 <= mask_W - w), LDIFF_ERR_INVALID,
              "%s: the box %d x %d at (mask_y0 = %d, mask_x0 = %d) leaves the mask %d x %d", who, h, w, mask_y0, mask_x0, mask_H, mask_W);
  if (acc_f16) finish<f16>(acc, cnt, heads, Hp, Wp, y0, x0, h, w, logits, mask, mask_W, mask_y0, mask_x0, inf_flag, s);
  else finish<float>(acc, cnt, heads, Hp, Wp, y0, x0, h, w, logits, mask, mask_W, mask_y0, mask_x0, inf_flag, s);
  HIP_CHECK(hipGetLastError());
}

void launch_window_finish_ensemble(const void* const* acc, int n_folds, const void* cnt, int heads, int Hp, int Wp, int y0, int x0, int h, int w, int acc_f16, void* logits,
                                   uint8_t* mask, int mask_H, int mask_W, int mask_y0, int mask_x0, int32_t* inf_flag, hipStream_t s) {
  const char* who = "window_finish_ensemble";
  LDIFF_CHECK(n_folds >= 1 && n_folds <= LDIFF_ENSEMBLE_MAX_FOLDS, LDIFF_ERR_INVALID, "%s: n_folds %d out of range [1, %d]", who, n_folds, LDIFF_ENSEMBLE_MAX_FOLDS);
  LDIFF_CHECK(heads >= 1 && heads <= 32, LDIFF_ERR_INVALID, "%s: heads %d out of range [1, 32]", who, heads);
  LDIFF_CHECK(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 <= Hp - h && x0 <= Wp - w, LDIFF_ERR_INVALID, "%s: the box %d x %d at (y0 = %d, x0 = %d) leaves the padded extent %d x %d",
              who, h, w, y0, x0, Hp, Wp);
  LDIFF_CHECK(!mask || (mask_y0 >= 0 && mask_x0 >= 0 && mask_y0 <= mask_H - h && mask_x0 <= mask_W - w), LDIFF_ERR_INVALID,
              "%s: the box %d x %d at (mask_y0 = %d, mask_x0 = %d) leaves the mask %d x %d", who, h, w, mask_y0, mask_x0, mask_H, mask_W);
  window_fold_table t = {};
  for (int k = 0; k < n_folds; ++k) {
    LDIFF_CHECK(acc[k], LDIFF_ERR_INVALID, "%s: acc[%d] is null (a table of n_folds = %d device pointers)", who, k, n_folds);
    t.acc[k] = acc[k];
  }
  if (acc_f16) finish_ensemble<f16>(t, n_folds, cnt, heads, Hp, Wp, y0, x0, h, w, logits, mask, mask_W, mask_y0, mask_x0, inf_flag, s);
  else finish_ensemble<float>(t, n_folds, cnt, heads, Hp, Wp, y0, x0, h, w, logits, mask, mask_W, mask_y0, mask_x0, inf_flag, s);
  HIP_CHECK(hipGetLastError());
}
