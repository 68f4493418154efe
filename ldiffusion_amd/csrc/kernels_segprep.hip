// Plan-and-preprocess scans of ONE training case of the tissue head (include/ldiff.h "Tissue head, plan and preprocess"): what DefaultPreprocessor.run_case_npy
// and DatasetFingerprintExtractor.analyze_case do per case on the CPU -- crop to non-zero, normalise, locate the foreground -- for an image that is
// already on the device.  Every kernel is a memory-bound walk over [C, H, W] uint8 / float32 planes and a [H, W] uint8 label map with row strides.
//   bbox     rows are dealt to the workgroups; a lane keeps the min / max row and column of its non-zero pixels, the wave folds them by shuffles,
//            the workgroup in LDS, and one integer atomicMin / atomicMax per workgroup and bound reaches memory.  Min and max commute: exact.
//   stats    per channel over the box.  STATS_BLOCKS workgroups per channel, each a FIXED contiguous slice of the box's rows; a lane sums its pixels
//            in the order it meets them, the workgroup folds the lanes by a fixed LDS tree, a second launch adds the STATS_BLOCKS partials in
//            index order.  uint8: exact 64-bit integer sums; float32: float64 sums whose order depends on the shape alone -- no float atomics, a
//            second run is bit-identical.
//   counts   one wave per row of the box: a per-wave LDS histogram of n_heads + 1 bins (the last: labels >= n_heads); lanes that agree on a bin add
//            their popcount from one lane (label maps are constant regions: 64 lanes on one bin otherwise).  A second launch forms, per class and
//            for `label > 0`, the exclusive prefix over the rows -- what rank_to_coord searches -- and the totals.
//   apply    (x - sub) / div per channel into the arena's raw planes (and, on request, the coefficient planes), the labels beside them.
//   rank_to_coord  one wave per rank: binary search of the row prefix, then a ballot / popcount walk along the row, 64 columns a step.
#include "common.h"

#include <type_traits>

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64, MAX_CH = 16, MAX_HEADS = 32, STATS_BLOCKS = 64, BBOX_GRID = 256;
enum { DT_U8 = 0, DT_F32 = 1 };

struct Img {                 // [C, H, W] planes of one case
  const void* p; int C, H, W;
  long long row_stride, plane_stride;   // elements
};
struct Box { int y0, y1, x0, x1; };

template <int DT> __device__ __forceinline__ float load_px(const Img& im, int c, int y, int x) {
  const long long i = (long long)c * im.plane_stride + (long long)y * im.row_stride + x;
  if constexpr (DT == DT_U8) return (float)static_cast<const uint8_t*>(im.p)[i];
  else return static_cast<const float*>(im.p)[i];
}

// ---- (a) the non-zero box ---------------------------------------------------------------------------------------------------------------------
// raw[4] = min row, max row, min column, max column of the non-zero pixels; case_bbox_init sets (H, -1, W, -1), case_bbox_final turns it into
// (y0, y1, x0, x1) with exclusive ends, the full extent for an all-zero image
__global__ void case_bbox_init_kernel(int* raw, int H, int W) { raw[0] = H; raw[1] = -1; raw[2] = W; raw[3] = -1; }
__global__ void case_bbox_final_kernel(int* raw, int H, int W) {
  if (raw[1] < 0) { raw[0] = 0; raw[1] = H; raw[2] = 0; raw[3] = W; }
  else { raw[1] += 1; raw[3] += 1; }
}

template <int DT>
__global__ __launch_bounds__(THREADS) void case_bbox_kernel(Img im, int* raw) {
  __shared__ int sh[4];
  const int tid = threadIdx.x;
  if (tid == 0) { sh[0] = im.H; sh[1] = -1; sh[2] = im.W; sh[3] = -1; }
  __syncthreads();
  int ymin = im.H, ymax = -1, xmin = im.W, xmax = -1;
  for (int y = blockIdx.x; y < im.H; y += gridDim.x)
    for (int x = tid; x < im.W; x += THREADS) {
      bool nz = false;
      for (int c = 0; c < im.C; ++c) nz |= load_px<DT>(im, c, y, x) != 0.f;   // NaN != 0, as in numpy
      if (nz) { ymin = min(ymin, y); ymax = max(ymax, y); xmin = min(xmin, x); xmax = max(xmax, x); }
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ymin = min(ymin, __shfl_xor(ymin, o)); ymax = max(ymax, __shfl_xor(ymax, o));
    xmin = min(xmin, __shfl_xor(xmin, o)); xmax = max(xmax, __shfl_xor(xmax, o));
  }
  if ((tid & 63) == 0 && ymax >= 0) { atomicMin(&sh[0], ymin); atomicMax(&sh[1], ymax); atomicMin(&sh[2], xmin); atomicMax(&sh[3], xmax); }
  __syncthreads();
  if (tid == 0 && sh[1] >= 0) { atomicMin(&raw[0], sh[0]); atomicMax(&raw[1], sh[1]); atomicMin(&raw[2], sh[2]); atomicMax(&raw[3], sh[3]); }
}

// ---- (b) crop statistics ----------------------------------------------------------------------------------------------------------------------
// one record per (channel, workgroup) in the workspace and per channel in the result: sum, sum of squares (uint64 bit patterns for uint8 input,
// float64 for float32 input), min, max (float64)
struct StatRec { unsigned long long sum, sumsq; double mn, mx; };
static_assert(sizeof(StatRec) == 32, "ldiff_op_case_stats: 32 bytes per channel");

template <int DT> struct Acc { using T = typename std::conditional<DT == DT_U8, unsigned long long, double>::type; };

template <int DT>
__global__ __launch_bounds__(THREADS) void case_stats_kernel(Img im, Box b, StatRec* part) {
  using T = typename Acc<DT>::T;
  __shared__ T s1[THREADS], s2[THREADS];
  __shared__ float smn[THREADS], smx[THREADS];
  const int tid = threadIdx.x, c = blockIdx.y, rows = b.y1 - b.y0;
  const int per = (rows + STATS_BLOCKS - 1) / STATS_BLOCKS;          // a fixed slice of rows per workgroup: the order depends on the shape alone
  const int r0 = b.y0 + blockIdx.x * per, r1 = min(b.y1, r0 + per);
  T a1 = 0, a2 = 0;
  float mn = INFINITY, mx = -INFINITY;
  for (int y = r0; y < r1; ++y)
    for (int x = b.x0 + tid; x < b.x1; x += THREADS) {
      const float v = load_px<DT>(im, c, y, x);
      if constexpr (DT == DT_U8) { const unsigned long long u = (unsigned long long)v; a1 += u; a2 += u * u; }
      else { const double d = (double)v; a1 += d; a2 += d * d; }
      mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
  s1[tid] = a1; s2[tid] = a2; smn[tid] = mn; smx[tid] = mx;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {                          // fixed tree
    if (tid < o) { s1[tid] += s1[tid + o]; s2[tid] += s2[tid + o]; smn[tid] = fminf(smn[tid], smn[tid + o]); smx[tid] = fmaxf(smx[tid], smx[tid + o]); }
    __syncthreads();
  }
  if (tid == 0) {
    StatRec r;
    r.sum = __builtin_bit_cast(unsigned long long, s1[0]); r.sumsq = __builtin_bit_cast(unsigned long long, s2[0]);
    r.mn = (double)smn[0]; r.mx = (double)smx[0];
    part[c * STATS_BLOCKS + blockIdx.x] = r;
  }
}

template <int DT>
__global__ void case_stats_final_kernel(const StatRec* part, StatRec* out, int C) {
  using T = typename Acc<DT>::T;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  T a1 = 0, a2 = 0;
  double mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < STATS_BLOCKS; ++i) {                             // index order
    const StatRec r = part[c * STATS_BLOCKS + i];
    a1 += __builtin_bit_cast(T, r.sum); a2 += __builtin_bit_cast(T, r.sumsq);
    mn = fmin(mn, r.mn); mx = fmax(mx, r.mx);
  }
  StatRec r;
  r.sum = __builtin_bit_cast(unsigned long long, a1); r.sumsq = __builtin_bit_cast(unsigned long long, a2); r.mn = mn; r.mx = mx;
  out[c] = r;
}

// ---- (c) label counts per row -----------------------------------------------------------------------------------------------------------------
struct Lab { const uint8_t* p; long long stride; };

__global__ __launch_bounds__(THREADS) void case_counts_kernel(Lab lab, Box b, int n_heads, unsigned* row_counts) {
  __shared__ unsigned hist[WAVES][MAX_HEADS + 2];   // n_heads + 1 bins; the ignore form counts its label as one more class
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rows = b.y1 - b.y0, w = b.x1 - b.x0;
  unsigned* h = hist[wave];
  for (int r0 = blockIdx.x * WAVES; r0 < rows; r0 += gridDim.x * WAVES) {      // a wave owns its row and its histogram; uniform trip counts throughout
    const int r = r0 + wave;
    const bool valid = r < rows;
    if (lane <= n_heads) h[lane] = 0;
    __syncthreads();
    const uint8_t* row = lab.p + (long long)(b.y0 + (valid ? r : 0)) * lab.stride + b.x0;
    for (int x0 = 0; x0 < w; x0 += 64) {
      const bool act = valid && x0 + lane < w;
      int bin = 0;
      if (act) { const int v = row[x0 + lane]; bin = v < n_heads ? v : n_heads; }
      unsigned long long todo = __ballot(act);
      while (todo) {                                                            // one LDS add per distinct bin of the 64 pixels
        const int first = __ffsll((long long)todo) - 1;
        const int b0 = __shfl(bin, first);
        const unsigned long long same = __ballot(act && bin == b0);
        if (lane == first) atomicAdd(&h[b0], (unsigned)__popcll(same));
        todo &= ~same;
      }
    }
    __syncthreads();
    if (valid && lane <= n_heads) row_counts[(long long)r * (n_heads + 1) + lane] = h[lane];
    __syncthreads();   // the next row zeroes the histogram
  }
}

// selector s in [0, n_heads): label == s; s == n_heads: label > 0 (labels >= n_heads included: the caller refuses such a case before it asks).
// prefix[s, r] = number of selected pixels in rows [0, r) of the box, r = 0 .. rows; totals[s] = prefix[s, rows]; totals[n_heads + 1] = labels >= n_heads.
// A grid of n_heads + 3 workgroups adds the selector `label < n_classes` ("the label is a class" of a map whose highest value is an ignore label):
// prefix row n_heads + 1, totals[n_heads + 2].
__global__ __launch_bounds__(THREADS) void case_prefix_kernel(const unsigned* row_counts, int rows, int n_heads, int n_classes, unsigned* prefix, unsigned* totals) {
  __shared__ unsigned sh[THREADS];
  __shared__ unsigned carry;
  const int s = blockIdx.x, tid = threadIdx.x, nb = n_heads + 1;
  if (tid == 0) carry = 0;
  __syncthreads();
  const bool has_row = s <= n_heads || s == n_heads + 2;
  unsigned* out = prefix + (long long)(s <= n_heads ? s : n_heads + 1) * (rows + 1);
  for (int r0 = 0; r0 < rows; r0 += THREADS) {
    const int r = r0 + tid;
    unsigned v = 0;
    if (r < rows) {
      if (s < n_heads) v = row_counts[(long long)r * nb + s];
      else if (s == n_heads) { for (int c = 1; c < nb; ++c) v += row_counts[(long long)r * nb + c]; }
      else if (s == n_heads + 1) v = row_counts[(long long)r * nb + n_heads];
      else { for (int c = 0; c < n_classes; ++c) v += row_counts[(long long)r * nb + c]; }
    }
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < THREADS; o <<= 1) {                                     // inclusive scan of the chunk
      const unsigned add = tid >= o ? sh[tid - o] : 0;
      __syncthreads();
      sh[tid] += add;
      __syncthreads();
    }
    const unsigned base = carry;
    if (r < rows && has_row) out[r] = base + sh[tid] - v;
    __syncthreads();
    if (tid == THREADS - 1) carry = base + sh[tid];
    __syncthreads();
  }
  if (tid == 0) {
    if (has_row) out[rows] = carry;
    totals[s] = carry;
  }
}

// ---- (d) apply --------------------------------------------------------------------------------------------------------------------------------
struct ApplyParams {
  Img im; Lab lab; Box b;
  float sub[MAX_CH], div[MAX_CH];
  float* raw; float* coef;       // destination planes [C, h, stride] (coef may be null)
  uint8_t* labels; int stride, label_stride;
};

template <int DT>
__global__ __launch_bounds__(THREADS) void case_apply_kernel(ApplyParams q) {
  const int h = q.b.y1 - q.b.y0, w = q.b.x1 - q.b.x0;
  const int y = blockIdx.x, plane = blockIdx.y;   // plane C: the labels
  if (y >= h) return;
  if (plane == q.im.C) {
    const uint8_t* src = q.lab.p + (long long)(q.b.y0 + y) * q.lab.stride + q.b.x0;
    for (int x = threadIdx.x; x < w; x += THREADS) q.labels[(long long)y * q.label_stride + x] = src[x];
    return;
  }
  const float sub = q.sub[plane], div = q.div[plane];
  const long long o = ((long long)plane * h + y) * q.stride;
  for (int x = threadIdx.x; x < w; x += THREADS) {
    const float v = (load_px<DT>(q.im, plane, q.b.y0 + y, q.b.x0 + x) - sub) / div;   // two IEEE operations, each rounded once
    q.raw[o + x] = v;
    if (q.coef) q.coef[o + x] = v;
  }
}

// ---- (e) rank to coordinate -------------------------------------------------------------------------------------------------------------------
struct RankParams {
  Lab lab; Box b; int selector;            // >= 0: label == selector; -1: label > 0; -1 - m: label < m
  const unsigned* prefix;                  // [rows + 1]
  const long long* ranks; long long n;
  int* coords;                             // [n, 2]
  Img im; void* values;                    // [n, C] of the image's dtype, or null
};

template <int DT>
__global__ __launch_bounds__(THREADS) void case_rank_kernel(RankParams q) {
  const int lane = threadIdx.x & 63, rows = q.b.y1 - q.b.y0, w = q.b.x1 - q.b.x0;
  const long long waves = (long long)gridDim.x * WAVES;
  for (long long i = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6); i < q.n; i += waves) {   // wave-uniform
    const long long rank = q.ranks[i];
    int row = -1, col = -1;
    if (rank >= 0 && rank < (long long)q.prefix[rows]) {
      int lo = 0, hi = rows - 1;                      // the last row whose exclusive prefix is <= rank
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)q.prefix[mid] <= rank) lo = mid; else hi = mid - 1;
      }
      row = lo;
      unsigned k = (unsigned)(rank - q.prefix[row]);   // the k-th selected pixel of that row
      const uint8_t* p = q.lab.p + (long long)(q.b.y0 + row) * q.lab.stride + q.b.x0;
      for (int x0 = 0; x0 < w; x0 += 64) {
        bool sel = false;
        if (x0 + lane < w) { const int v = p[x0 + lane]; sel = q.selector >= 0 ? v == q.selector : q.selector == -1 ? v > 0 : v < -1 - q.selector; }
        const unsigned long long m = __ballot(sel);
        const unsigned cnt = (unsigned)__popcll(m);
        if (k < cnt) {
          const unsigned below = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
          const unsigned long long hit = __ballot(sel && below == k);
          col = x0 + __ffsll((long long)hit) - 1;
          break;
        }
        k -= cnt;
      }
      if (col < 0) row = -1;   // the prefix and the labels disagree: report no pixel, read nothing
    }
    if (lane == 0) { q.coords[2 * i] = row; q.coords[2 * i + 1] = col; }
    if (q.values && lane < q.im.C) {
      using T = typename std::conditional<DT == DT_U8, uint8_t, float>::type;
      T v = 0;
      if (row >= 0) v = static_cast<const T*>(q.im.p)[(long long)lane * q.im.plane_stride + (long long)(q.b.y0 + row) * q.im.row_stride + q.b.x0 + col];
      static_cast<T*>(q.values)[i * q.im.C + lane] = v;
    }
  }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------------
Img checked_img(const char* who, const void* img, int dtype, int C, int H, int W, long long row_stride, long long plane_stride) {
  LDIFF_CHECK(dtype == DT_U8 || dtype == DT_F32, LDIFF_ERR_INVALID, "%s: dtype %d (0 uint8, 1 float32)", who, dtype);
  LDIFF_CHECK(C >= 1 && C <= MAX_CH, LDIFF_ERR_INVALID, "%s: %d channels out of range [1,%d]", who, C, MAX_CH);
  LDIFF_CHECK(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, LDIFF_ERR_INVALID, "%s: extent %d x %d out of range [1,32768]", who, H, W);
  LDIFF_CHECK(row_stride >= W, LDIFF_ERR_INVALID, "%s: row_stride %lld below W = %d", who, row_stride, W);
  LDIFF_CHECK(C == 1 || plane_stride >= (long long)(H - 1) * row_stride + W, LDIFF_ERR_INVALID, "%s: plane_stride %lld: planes overlap", who, plane_stride);
  LDIFF_CHECK(img, LDIFF_ERR_INVALID, "%s: null argument img", who);
  LDIFF_CHECK(dtype == DT_U8 || (reinterpret_cast<uintptr_t>(img) & 3) == 0, LDIFF_ERR_INVALID, "%s: float32 img not aligned to 4 bytes", who);
  return Img{img, C, H, W, row_stride, plane_stride};
}

Box checked_box(const char* who, int H, int W, int y0, int y1, int x0, int x1) {
  LDIFF_CHECK(0 <= y0 && y0 < y1 && y1 <= H && 0 <= x0 && x0 < x1 && x1 <= W, LDIFF_ERR_INVALID, "%s: box (%d, %d, %d, %d) is empty or leaves the %d x %d case", who, y0,
              y1, x0, x1, H, W);
  return Box{y0, y1, x0, x1};
}

Lab checked_lab(const char* who, const void* label, int W, long long label_stride) {
  LDIFF_CHECK(label, LDIFF_ERR_INVALID, "%s: null argument label", who);
  LDIFF_CHECK(label_stride >= W, LDIFF_ERR_INVALID, "%s: label_stride %lld below W = %d", who, label_stride, W);
  return Lab{static_cast<const uint8_t*>(label), label_stride};
}

}  // namespace

void launch_case_bbox(const void* img, int dtype, int C, int H, int W, long long row_stride, long long plane_stride, int* box, hipStream_t s) {
  const Img im = checked_img("case_bbox", img, dtype, C, H, W, row_stride, plane_stride);
  LDIFF_CHECK(box && (reinterpret_cast<uintptr_t>(box) & 3) == 0, LDIFF_ERR_INVALID, "case_bbox: box null or not aligned to 4 bytes");
  ProfScope prof("case_bbox", 0.0, (double)C * H * W * (dtype == DT_U8 ? 1.0 : 4.0), s);
  hipLaunchKernelGGL(case_bbox_init_kernel, dim3(1), dim3(1), 0, s, box, H, W);
  const int grid = H < BBOX_GRID ? H : BBOX_GRID;
  if (dtype == DT_U8) hipLaunchKernelGGL(case_bbox_kernel<DT_U8>, dim3(grid), dim3(THREADS), 0, s, im, box);
  else hipLaunchKernelGGL(case_bbox_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, s, im, box);
  hipLaunchKernelGGL(case_bbox_final_kernel, dim3(1), dim3(1), 0, s, box, H, W);
  HIP_CHECK(hipGetLastError());
}

long long case_stats_ws_bytes(int C) { return (C >= 1 && C <= MAX_CH) ? (long long)C * STATS_BLOCKS * (long long)sizeof(StatRec) : 0; }

void launch_case_stats(const void* img, int dtype, int C, int H, int W, long long row_stride, long long plane_stride, int y0, int y1, int x0, int x1, void* stats,
                       void* ws, long long ws_bytes, hipStream_t s) {
  const Img im = checked_img("case_stats", img, dtype, C, H, W, row_stride, plane_stride);
  const Box b = checked_box("case_stats", H, W, y0, y1, x0, x1);
  LDIFF_CHECK(stats && (reinterpret_cast<uintptr_t>(stats) & 7) == 0, LDIFF_ERR_INVALID, "case_stats: stats null or not aligned to 8 bytes");
  LDIFF_CHECK(ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && ws_bytes >= case_stats_ws_bytes(C), LDIFF_ERR_INVALID,
              "case_stats: workspace of %lld bytes, ldiff_op_case_stats_ws_bytes asks for %lld (8-byte aligned)", ws_bytes, case_stats_ws_bytes(C));
  ProfScope prof("case_stats", 0.0, (double)C * (y1 - y0) * (x1 - x0) * (dtype == DT_U8 ? 1.0 : 4.0), s);
  StatRec* part = static_cast<StatRec*>(ws);
  if (dtype == DT_U8) {
    hipLaunchKernelGGL(case_stats_kernel<DT_U8>, dim3(STATS_BLOCKS, C), dim3(THREADS), 0, s, im, b, part);
    hipLaunchKernelGGL(case_stats_final_kernel<DT_U8>, dim3(1), dim3(64), 0, s, part, static_cast<StatRec*>(stats), C);
  } else {
    hipLaunchKernelGGL(case_stats_kernel<DT_F32>, dim3(STATS_BLOCKS, C), dim3(THREADS), 0, s, im, b, part);
    hipLaunchKernelGGL(case_stats_final_kernel<DT_F32>, dim3(1), dim3(64), 0, s, part, static_cast<StatRec*>(stats), C);
  }
  HIP_CHECK(hipGetLastError());
}

void launch_case_counts(const void* label, int H, int W, long long label_stride, int y0, int y1, int x0, int x1, int n_heads, int n_classes, unsigned* row_counts,
                        unsigned* row_prefix, unsigned* totals, hipStream_t s) {
  LDIFF_CHECK(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, LDIFF_ERR_INVALID, "case_counts: extent %d x %d out of range [1,32768]", H, W);
  const int max_heads = MAX_HEADS + (n_classes > 0 ? 1 : 0);   // with the class selector the ignore label may be counted as one more class
  LDIFF_CHECK(n_heads >= 1 && n_heads <= max_heads, LDIFF_ERR_INVALID, "case_counts: n_heads %d out of range [1,%d]", n_heads, max_heads);
  LDIFF_CHECK(n_classes >= 0 && n_classes <= n_heads, LDIFF_ERR_INVALID, "case_counts: n_classes %d out of range [1,%d]", n_classes, n_heads);
  const Lab lab = checked_lab("case_counts", label, W, label_stride);
  const Box b = checked_box("case_counts", H, W, y0, y1, x0, x1);
  LDIFF_CHECK(row_counts && row_prefix && totals, LDIFF_ERR_INVALID, "case_counts: null output");
  LDIFF_CHECK(((reinterpret_cast<uintptr_t>(row_counts) | reinterpret_cast<uintptr_t>(row_prefix) | reinterpret_cast<uintptr_t>(totals)) & 3) == 0, LDIFF_ERR_INVALID,
              "case_counts: outputs not aligned to 4 bytes");
  const int rows = y1 - y0;
  ProfScope prof("case_counts", 0.0, (double)rows * (x1 - x0), s);
  const int grid = (rows + WAVES - 1) / WAVES;
  hipLaunchKernelGGL(case_counts_kernel, dim3(grid < 1024 ? grid : 1024), dim3(THREADS), 0, s, lab, b, n_heads, row_counts);
  hipLaunchKernelGGL(case_prefix_kernel, dim3(n_heads + 2 + (n_classes > 0 ? 1 : 0)), dim3(THREADS), 0, s, row_counts, rows, n_heads, n_classes, row_prefix, totals);
  HIP_CHECK(hipGetLastError());
}

void launch_case_apply(const void* img, int dtype, int C, int H, int W, long long row_stride, long long plane_stride, const void* label, long long label_stride, int y0, int y1,
                       int x0, int x1, const float* sub, const float* div, void* arena, long long arena_bytes, const ldiff_seg_case* row, int write_coef, hipStream_t s) {
  ApplyParams q{};
  q.im = checked_img("case_apply", img, dtype, C, H, W, row_stride, plane_stride);
  q.lab = checked_lab("case_apply", label, W, label_stride);
  q.b = checked_box("case_apply", H, W, y0, y1, x0, x1);
  LDIFF_CHECK(sub && div && arena && row, LDIFF_ERR_INVALID, "case_apply: null argument");
  const int h = y1 - y0, w = x1 - x0;
  LDIFF_CHECK(row->H == h && row->W == w, LDIFF_ERR_INVALID, "case_apply: the table row is %d x %d, the box %d x %d", row->H, row->W, h, w);
  LDIFF_CHECK(row->stride >= w && row->label_stride >= w, LDIFF_ERR_INVALID, "case_apply: the table row's strides (%d, %d) are below its width %d", row->stride,
              row->label_stride, w);
  const long long plane_bytes = (long long)C * h * row->stride * 4, label_bytes = (long long)h * row->label_stride;
  auto inside = [&](long long off, long long bytes) { return off >= 0 && bytes <= arena_bytes && off <= arena_bytes - bytes; };
  LDIFF_CHECK(inside(row->raw_off, plane_bytes) && inside(row->label_off, label_bytes) && (!write_coef || inside(row->coef_off, plane_bytes)), LDIFF_ERR_INVALID,
              "case_apply: the table row leaves the arena of %lld bytes", arena_bytes);
  LDIFF_CHECK((reinterpret_cast<uintptr_t>(arena) & 3) == 0 && row->raw_off % 4 == 0 && (!write_coef || row->coef_off % 4 == 0), LDIFF_ERR_INVALID,
              "case_apply: a float offset is no multiple of 4");
  for (int c = 0; c < C; ++c) { q.sub[c] = sub[c]; q.div[c] = div[c]; }
  char* base = static_cast<char*>(arena);
  q.raw = reinterpret_cast<float*>(base + row->raw_off);
  q.coef = write_coef ? reinterpret_cast<float*>(base + row->coef_off) : nullptr;
  q.labels = reinterpret_cast<uint8_t*>(base + row->label_off);
  q.stride = row->stride; q.label_stride = row->label_stride;
  ProfScope prof("case_apply", 0.0, (double)C * h * w * ((dtype == DT_U8 ? 1.0 : 4.0) + (write_coef ? 8.0 : 4.0)) + 2.0 * h * w, s);
  if (dtype == DT_U8) hipLaunchKernelGGL(case_apply_kernel<DT_U8>, dim3(h, C + 1), dim3(THREADS), 0, s, q);
  else hipLaunchKernelGGL(case_apply_kernel<DT_F32>, dim3(h, C + 1), dim3(THREADS), 0, s, q);
  HIP_CHECK(hipGetLastError());
}

void launch_case_rank_to_coord(const void* label, int H, int W, long long label_stride, int y0, int y1, int x0, int x1, int selector, const unsigned* row_prefix,
                               const long long* ranks, long long n, int* coords, const void* img, int dtype, int C, long long row_stride, long long plane_stride, void* values,
                               hipStream_t s) {
  LDIFF_CHECK(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, LDIFF_ERR_INVALID, "case_rank_to_coord: extent %d x %d out of range [1,32768]", H, W);
  LDIFF_CHECK(n >= 0, LDIFF_ERR_INVALID, "case_rank_to_coord: negative n");
  LDIFF_CHECK(selector >= -256 && selector < 256, LDIFF_ERR_INVALID, "case_rank_to_coord: selector %d (a class 0..255, -1 for label > 0, -1 - m for label < m <= 255)",
              selector);
  if (n == 0) return;
  RankParams q{};
  q.lab = checked_lab("case_rank_to_coord", label, W, label_stride);
  q.b = checked_box("case_rank_to_coord", H, W, y0, y1, x0, x1);
  LDIFF_CHECK(row_prefix && ranks && coords, LDIFF_ERR_INVALID, "case_rank_to_coord: null argument");
  LDIFF_CHECK((reinterpret_cast<uintptr_t>(row_prefix) & 3) == 0 && (reinterpret_cast<uintptr_t>(coords) & 3) == 0 && (reinterpret_cast<uintptr_t>(ranks) & 7) == 0,
              LDIFF_ERR_INVALID, "case_rank_to_coord: row_prefix / coords / ranks not aligned to their element size");
  q.selector = selector; q.prefix = row_prefix; q.ranks = ranks; q.n = n; q.coords = coords;
  if (values) {
    q.im = checked_img("case_rank_to_coord", img, dtype, C, H, W, row_stride, plane_stride);
    LDIFF_CHECK(dtype == DT_U8 || (reinterpret_cast<uintptr_t>(values) & 3) == 0, LDIFF_ERR_INVALID, "case_rank_to_coord: float32 values not aligned to 4 bytes");
    q.values = values;
  }
  ProfScope prof("case_rank_to_coord", 0.0, (double)n * (x1 - x0), s);
  const long long blocks = (n + WAVES - 1) / WAVES;
  const int grid = (int)(blocks < 65536 ? blocks : 65536);
  if (values && dtype == DT_F32) hipLaunchKernelGGL(case_rank_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, s, q);
  else hipLaunchKernelGGL(case_rank_kernel<DT_U8>, dim3(grid), dim3(THREADS), 0, s, q);
  HIP_CHECK(hipGetLastError());
}
