// Connected components of label maps and nnU-Net's "remove all but the largest connected component" (postprocessing/remove_connected_components.py:22-34), on the
// device: include/ldiff.h "Postprocessing".  N uint8 label maps [N, H, W], each on its own; membership = table[seg] (256 device bytes), the binary mask is never stored.
//
// A component's label is the SMALLEST linear pixel index (y W + x, per image) in it: every union links the larger root under the smaller one, so the result does not
// depend on scheduling.  Launches, in order (what one workgroup stores is read by another only behind a launch boundary):
//   1 cc_local     union-find of a CC_TH x CC_TW tile in LDS; parent[p] = the tile-local root as a linear index of the image, -1 outside the mask
//   2 cc_merge     the seams: the row under each horizontal seam against the row above it, the column right of each vertical seam against the column left of it (the
//                  diagonals across tile corners are among them).  Every read of `parent` is an agent-scope atomic load, every update an atomicMin; no waiting on
//                  another workgroup: a union loop ends because parents only decrease
//   3 cc_flatten   root[p] = find(p) (parent is read-only here)
//   4 memset + cc_count   size[root] += 1, integer atomics, one per workgroup for the workgroup's smallest root
//   5 cc_winner    per image max over roots of cc_winner_key (the tie rule, below)
//   6 cc_filter / cc_export
#include "common.h"

constexpr int CC_TH = LDIFF_CC_TILE_H, CC_TW = LDIFF_CC_TILE_W, CC_THREADS = 256;
constexpr int CC_TILE = CC_TH * CC_TW;

// ---- the tie rule, in one place: the largest component wins; among components of equal largest size the one whose first pixel in raster order comes first, that is the
// one with the smallest label.  As one 64-bit key whose maximum is the winner: size in the high word, the complement of the label in the low word.  (UNPINNED: the
// reference calls acvl_utils, restated as skimage.measure.label + argmax of the sizes)  Key 0 = no component: an empty mask.
__device__ __forceinline__ unsigned long long cc_winner_key(int size, int root) { return ((unsigned long long)(unsigned)size << 32) | (unsigned)~(unsigned)root; }
__device__ __forceinline__ int cc_winner_root(unsigned long long key) { return key == 0 ? -1 : (int)~(unsigned)(key & 0xffffffffull); }

struct CcWs {
  int* a;                     // [N][HW]: parent (launches 1-3), then the sizes at the roots
  unsigned long long* keys;   // [N]
  int* root;                  // [N][HW]
};

// ---- 1. tile-local union-find in LDS ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* L, int x) {
  while (true) {
    const int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
  while (true) {
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;   // a had stopped being a root: go on with what it hangs under
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const uint8_t* __restrict__ seg, const uint8_t* __restrict__ table, int H, int W, int tiles_x,
                                                              int tiles_per_image, int* __restrict__ parent) {
  __shared__ int L[CC_TILE];
  __shared__ uint8_t M[CC_TILE];
  const int n = blockIdx.x / tiles_per_image, t = blockIdx.x % tiles_per_image;
  const int y0 = (t / tiles_x) * CC_TH, x0 = (t % tiles_x) * CC_TW;
  const long long base = (long long)n * H * W;
  for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
    const int y = y0 + i / CC_TW, x = x0 + i % CC_TW;
    M[i] = (y < H && x < W) ? table[seg[base + (long long)y * W + x]] : 0;
    L[i] = i;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
    if (!M[i]) continue;
    const int ly = i / CC_TW, lx = i % CC_TW;
    // of the four neighbours that come earlier in raster order only those whose link does not follow from the neighbours' own links
    if (ly > 0 && M[i - CC_TW]) {
      lds_union(L, i, i - CC_TW);
    } else {
      if (lx > 0 && M[i - 1]) lds_union(L, i, i - 1);
      else if (lx > 0 && ly > 0 && M[i - CC_TW - 1]) lds_union(L, i, i - CC_TW - 1);
      if (ly > 0 && lx < CC_TW - 1 && M[i - CC_TW + 1]) lds_union(L, i, i - CC_TW + 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
    const int y = y0 + i / CC_TW, x = x0 + i % CC_TW;
    if (y >= H || x >= W) continue;
    int r = -1;
    if (M[i]) {
      const int l = lds_find(L, i);
      r = (y0 + l / CC_TW) * W + x0 + l % CC_TW;
    }
    parent[base + (long long)y * W + x] = r;
  }
}

// ---- 2. the seams --------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_find_atomic(int* parent, int x) {
  while (true) {
    const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}
// A stale root costs a turn of the loop, never the result: atomicMin returns what the parent really was, and whatever it was stays linked to both sides.
__device__ __forceinline__ void cc_union_atomic(int* parent, int a, int b) {
  while (true) {
    a = cc_find_atomic(parent, a);
    b = cc_find_atomic(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const uint8_t* __restrict__ seg, const uint8_t* __restrict__ table, int H, int W, int n_hseams,
                                                              int n_vseams, int blocks_per_image, int* parent_all) {
  const int n = blockIdx.x / blocks_per_image;
  const long long j = (long long)(blockIdx.x % blocks_per_image) * CC_THREADS + threadIdx.x;
  const long long base = (long long)n * H * W, n_h = (long long)n_hseams * W, n_v = (long long)n_vseams * H;
  if (j >= n_h + n_v) return;
  const uint8_t* s = seg + base;
  int* parent = parent_all + base;
  auto member = [&](int y, int x) { return y >= 0 && y < H && x >= 0 && x < W && table[s[(long long)y * W + x]]; };
  if (j < n_h) {   // the row under a horizontal seam against the three pixels above it
    const int y = (int)(j / W + 1) * CC_TH, x = (int)(j % W);
    if (!member(y, x)) return;
    for (int dx = -1; dx <= 1; ++dx)
      if (member(y - 1, x + dx)) cc_union_atomic(parent, y * W + x, (y - 1) * W + x + dx);
  } else {         // the column right of a vertical seam against the three pixels left of it
    const long long k = j - n_h;
    const int x = (int)(k / H + 1) * CC_TW, y = (int)(k % H);
    if (!member(y, x)) return;
    for (int dy = -1; dy <= 1; ++dy)
      if (member(y + dy, x - 1)) cc_union_atomic(parent, y * W + x, (y + dy) * W + x - 1);
  }
}

// ---- 3 .. 5 --------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const int* __restrict__ parent_all, int HW, int blocks_per_image, int* __restrict__ root_all) {
  const int n = blockIdx.x / blocks_per_image;
  const long long p = (long long)(blockIdx.x % blocks_per_image) * CC_THREADS + threadIdx.x;
  if (p >= HW) return;
  const int* parent = parent_all + (long long)n * HW;
  int x = parent[p];
  if (x >= 0)
    while (true) {
      const int q = parent[x];
      if (q == x) break;
      x = q;
    }
  root_all[(long long)n * HW + p] = x;
}

__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const int* __restrict__ root_all, int HW, int blocks_per_image, int* size_all) {
  __shared__ int s_root, s_count;
  const int n = blockIdx.x / blocks_per_image;
  const long long p = (long long)(blockIdx.x % blocks_per_image) * CC_THREADS + threadIdx.x;
  if (threadIdx.x == 0) { s_root = 0x7fffffff; s_count = 0; }
  __syncthreads();
  const int r = p < HW ? root_all[(long long)n * HW + p] : -1;
  if (r >= 0) atomicMin(&s_root, r);
  __syncthreads();
  int* size = size_all + (long long)n * HW;
  if (r >= 0) {
    if (r == s_root) atomicAdd(&s_count, 1);
    else atomicAdd(&size[r], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_count > 0) atomicAdd(&size[s_root], s_count);
}

__global__ __launch_bounds__(CC_THREADS) void cc_winner_kernel(const int* __restrict__ root_all, const int* __restrict__ size_all, int HW, int blocks_per_image,
                                                               unsigned long long* keys) {
  __shared__ unsigned long long s_key;
  const int n = blockIdx.x / blocks_per_image;
  const long long p = (long long)(blockIdx.x % blocks_per_image) * CC_THREADS + threadIdx.x;
  if (threadIdx.x == 0) s_key = 0;
  __syncthreads();
  if (p < HW && root_all[(long long)n * HW + p] == (int)p) atomicMax(&s_key, cc_winner_key(size_all[(long long)n * HW + p], (int)p));
  __syncthreads();
  if (threadIdx.x == 0 && s_key != 0) atomicMax(&keys[n], s_key);
}

// ---- 6. the results ------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const uint8_t* __restrict__ seg, const uint8_t* __restrict__ table, const int* __restrict__ root_all,
                                                               const unsigned long long* __restrict__ keys, int HW, int blocks_per_image, int background,
                                                               uint8_t* __restrict__ out) {
  const int n = blockIdx.x / blocks_per_image;
  const long long p = (long long)(blockIdx.x % blocks_per_image) * CC_THREADS + threadIdx.x;
  if (p >= HW) return;
  const long long i = (long long)n * HW + p;
  const uint8_t v = seg[i];
  out[i] = (table[v] && root_all[i] != cc_winner_root(keys[n])) ? (uint8_t)background : v;
}

__global__ __launch_bounds__(CC_THREADS) void cc_export_kernel(const int* __restrict__ root_all, const int* __restrict__ size_all, long long total,
                                                               int* __restrict__ labels, int* __restrict__ sizes) {
  const long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= total) return;
  labels[i] = root_all[i] + 1;   // -1 outside the mask
  sizes[i] = size_all[i];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------------
static long long cc_pad2(long long n) { return (n + 1) & ~1ll; }

long long keep_largest_component_ws_bytes(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1 || (long long)H * W > (1ll << 30)) return 0;
  const long long px = cc_pad2((long long)N * H * W);
  return px * 4 + (long long)N * 8 + px * 4;
}

static CcWs cc_components(const char* what, const uint8_t* seg, int N, int H, int W, const uint8_t* table, void* ws, long long ws_bytes, hipStream_t s) {
  LDIFF_CHECK(N >= 1, LDIFF_ERR_INVALID, "%s: N=%d below 1", what, N);
  LDIFF_CHECK(H >= 1, LDIFF_ERR_INVALID, "%s: H=%d below 1", what, H);
  LDIFF_CHECK(W >= 1, LDIFF_ERR_INVALID, "%s: W=%d below 1", what, W);
  LDIFF_CHECK((long long)H * W <= (1ll << 30), LDIFF_ERR_INVALID, "%s: H * W = %lld above 2^30 (H=%d W=%d)", what, (long long)H * W, H, W);
  const int HW = H * W, tiles_x = (W + CC_TW - 1) / CC_TW, tiles_y = (H + CC_TH - 1) / CC_TH, bpi = (HW + CC_THREADS - 1) / CC_THREADS;
  const long long tiles_per_image = (long long)tiles_x * tiles_y;
  LDIFF_CHECK((long long)N * bpi < (1ll << 31) && (long long)N * tiles_per_image < (1ll << 31), LDIFF_ERR_INVALID,
              "%s: N=%d images of %d x %d make more workgroups than one launch takes", what, N, H, W);
  LDIFF_CHECK(seg && table && ws, LDIFF_ERR_INVALID, "%s: null argument", what);
  LDIFF_CHECK(((uintptr_t)ws & 7) == 0, LDIFF_ERR_INVALID, "%s: ws is not 8-byte aligned", what);
  LDIFF_CHECK(ws_bytes >= keep_largest_component_ws_bytes(N, H, W), LDIFF_ERR_INVALID, "%s: ws_bytes=%lld, %lld needed (ldiff_op_keep_largest_component_ws_bytes)",
              what, ws_bytes, keep_largest_component_ws_bytes(N, H, W));
  const long long total = (long long)N * HW, px = cc_pad2(total);
  CcWs w;
  w.a = (int*)ws;
  w.keys = (unsigned long long*)(w.a + px);
  w.root = (int*)(w.keys + N);
  hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)(N * tiles_per_image)), dim3(CC_THREADS), 0, s, seg, table, H, W, tiles_x, (int)tiles_per_image, w.a);
  HIP_CHECK(hipGetLastError());
  const int n_hseams = (H - 1) / CC_TH, n_vseams = (W - 1) / CC_TW;
  const long long seam_px = (long long)n_hseams * W + (long long)n_vseams * H;
  if (seam_px > 0) {
    const int bpi_m = (int)((seam_px + CC_THREADS - 1) / CC_THREADS);   // <= 2 bpi-ish: fewer seam pixels than pixels
    hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)((long long)N * bpi_m)), dim3(CC_THREADS), 0, s, seg, table, H, W, n_hseams, n_vseams, bpi_m, w.a);
    HIP_CHECK(hipGetLastError());
  }
  const dim3 grid((unsigned)((long long)N * bpi));
  hipLaunchKernelGGL(cc_flatten_kernel, grid, dim3(CC_THREADS), 0, s, (const int*)w.a, HW, bpi, w.root);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemsetAsync(w.a, 0, (size_t)(px * 4 + (long long)N * 8), s));   // the parents are done with: sizes and winner keys start at zero
  hipLaunchKernelGGL(cc_count_kernel, grid, dim3(CC_THREADS), 0, s, (const int*)w.root, HW, bpi, w.a);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(cc_winner_kernel, grid, dim3(CC_THREADS), 0, s, (const int*)w.root, (const int*)w.a, HW, bpi, w.keys);
  HIP_CHECK(hipGetLastError());
  return w;
}

static bool cc_overlap(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

void launch_keep_largest_component(const uint8_t* seg_in, uint8_t* seg_out, int N, int H, int W, const uint8_t* table, int background_label, void* ws,
                                   long long ws_bytes, hipStream_t s) {
  const char* what = "op_keep_largest_component";
  LDIFF_CHECK(seg_out, LDIFF_ERR_INVALID, "%s: null argument seg_out", what);
  LDIFF_CHECK(background_label >= 0 && background_label <= 255, LDIFF_ERR_INVALID, "%s: background_label=%d does not fit a uint8 label map", what, background_label);
  if (seg_in && N >= 1 && H >= 1 && W >= 1 && (long long)H * W <= (1ll << 30))
    LDIFF_CHECK(!cc_overlap(seg_in, (long long)N * H * W, seg_out, (long long)N * H * W), LDIFF_ERR_INVALID,
                "%s: seg_out overlaps seg_in (in-place operation is refused: seg_in is not modified)", what);
  const CcWs w = cc_components(what, seg_in, N, H, W, table, ws, ws_bytes, s);
  const int HW = H * W, bpi = (HW + CC_THREADS - 1) / CC_THREADS;
  hipLaunchKernelGGL(cc_filter_kernel, dim3((unsigned)((long long)N * bpi)), dim3(CC_THREADS), 0, s, seg_in, table, (const int*)w.root,
                     (const unsigned long long*)w.keys, HW, bpi, background_label, seg_out);
  HIP_CHECK(hipGetLastError());
}

void launch_cc_label(const uint8_t* seg, int N, int H, int W, const uint8_t* table, int* labels, int* sizes, void* ws, long long ws_bytes, hipStream_t s) {
  const char* what = "op_cc_label";
  LDIFF_CHECK(labels, LDIFF_ERR_INVALID, "%s: null argument labels", what);
  LDIFF_CHECK(sizes, LDIFF_ERR_INVALID, "%s: null argument sizes", what);
  const CcWs w = cc_components(what, seg, N, H, W, table, ws, ws_bytes, s);
  const long long total = (long long)N * H * W;
  hipLaunchKernelGGL(cc_export_kernel, dim3((unsigned)((total + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, s, (const int*)w.root, (const int*)w.a, total,
                     labels, sizes);
  HIP_CHECK(hipGetLastError());
}
