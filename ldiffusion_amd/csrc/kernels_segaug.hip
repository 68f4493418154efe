// Training data of the nnU-Net tissue head (include/ldiff.h "Tissue head, training data"): what nnUNetDataLoader2D and the transforms of
// nnUNetTrainer.get_training_transforms do to a batch, from cases that stay on the device.  Two launches per batch, no host synchronisation.
//
// seg_sample_kernel     resampled data planes (f32 NCHW), the full-resolution label map and every deep-supervision label map of a batch
//   work      one thread = one output pixel of one scale; a sample's pixels of all scales are one index space (scale 0 first), the patch row
//             contiguous, so stores coalesce.  blockIdx.y = sample: the copy / resample branch is uniform per workgroup.
//   data      patch index -> case coordinate by the sample's 2 x 3 matrix (rotation, scale, mirror and centre folded in on the host: no
//             trigonometry here); cubic B-spline of the case's prefiltered coefficients, 4 x 4 taps mirrored at whole samples, 0 where the
//             coordinate leaves [0, n - 1].  One thread forms its 4 + 4 weights once and reuses them over the C channels; the taps are reads
//             of a case that sits in L2 / Infinity Cache.
//   labels    bilinear vote: per label the sum of the four weights on it, the highest label whose sum reaches 0.5 wins, else 0; 0 outside.
//             Scale k asks for full-resolution pixel (2^k i + 2^(k-1), 2^k j + 2^(k-1)) and evaluates it with the same arithmetic.
//   copy      a sample without rotation / scale carries an integer translation (and +-1 steps for the mirror) and reads the raw normalised
//             image and the label map directly: exact.
//
// seg_intensity_kernel  noise, blur, brightness, contrast and the two gammas, in place, ONE workgroup per (sample, channel) plane for the whole
//   chain.  Every mean / std / min / max is reduced inside the workgroup in a fixed order: a thread's partial over its strided walk (16-byte loads
//   where a plane is a multiple of 4 elements), a 64-lane butterfly, then the 16 wave partials added in wave order by every thread.  The blur's two
//   passes go plane -> workspace -> plane with workgroup barriers between.  No atomics, no inter-workgroup traffic: a replay is bit-identical.
//   A plane whose table row has everything off returns after reading the row.
//   <VEC, LR = true> (ldiff_op_seg_intensity_lr) adds SimulateLowResolutionTransform between contrast and the gammas: order-0 down-sampling into the
//   plane's workspace with a 12-sample edge pad, the cubic B-spline prefilter below, order-3 up-sampling back into the data, clipped.
//
// spline_prefilter_kernel  scipy.ndimage.spline_filter(order=3, mode='mirror') of a plane by one workgroup, in place (ldiff_op_spline_prefilter).
#include "common.h"

#include <math.h>

namespace {

constexpr int MAX_SCALES = 8, ST = 256;
constexpr int IT = 1024, IW = IT / 64, MAX_RADIUS = 7;

struct SampleParams {
  const unsigned char* arena; long long arena_bytes;
  const ldiff_seg_case* cases; int n_cases;
  const ldiff_seg_sample* samples;
  int B, C, h, w, n_scales;
  float* data; uint8_t* target;
  int first[MAX_SCALES + 1];           // first pixel of scale k in a sample's index space; first[n_scales] = pixels per sample over all scales
  long long target_off[MAX_SCALES];    // byte offset of scale k's [B, 1, h_k, w_k] block in `target`
};

__device__ __forceinline__ int mirror_index(int i, int n) {   // whole-sample mirror: -i -> i, n - 1 + i -> n - 1 - i (clamped: tiny cases)
  i = i < 0 ? -i : i;
  i = i > n - 1 ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

__device__ __forceinline__ void bspline3(float t, float w[4]) {
  const float s = 1.f - t, t2 = t * t, s2 = s * s;
  w[0] = s2 * s * (1.f / 6.f);
  w[1] = (4.f - 6.f * t2 + 3.f * t2 * t) * (1.f / 6.f);
  w[2] = (4.f - 6.f * s2 + 3.f * s2 * s) * (1.f / 6.f);
  w[3] = t2 * t * (1.f / 6.f);
}

__device__ __forceinline__ bool inside(float y, float x, int H, int W) {   // false for NaN
  return y >= 0.f && y <= (float)(H - 1) && x >= 0.f && x <= (float)(W - 1);
}

// interpolate_img(is_seg=True, order=1) at one point: the highest label whose bilinear indicator reaches 0.5
__device__ __forceinline__ unsigned vote_label(const uint8_t* lab, int H, int W, int ls, float y, float x) {
  if (!inside(y, x, H, W)) return 0u;
  const float fy = floorf(y), fx = floorf(x), ty = y - fy, tx = x - fx;
  const int y0 = (int)fy, x0 = (int)fx, y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);   // the clamped neighbour has weight 0
  const unsigned l[4] = {lab[(long long)y0 * ls + x0], lab[(long long)y0 * ls + x1], lab[(long long)y1 * ls + x0], lab[(long long)y1 * ls + x1]};
  const float wt[4] = {(1.f - ty) * (1.f - tx), (1.f - ty) * tx, ty * (1.f - tx), ty * tx};
  unsigned best = 0u;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += l[k] == l[a] ? wt[k] : 0.f;
    if (s >= 0.5f && l[a] > best) best = l[a];
  }
  return best;
}

__global__ __launch_bounds__(ST) void seg_sample_kernel(SampleParams q) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * ST + threadIdx.x;
  if (p >= q.first[q.n_scales]) return;
  int k = 0;
  while (k + 1 < q.n_scales && p >= q.first[k + 1]) ++k;
  const int hk = q.h >> k, wk = q.w >> k, r = p - q.first[k];
  const int i = r / wk, j = r - i * wk;
  const int fi = k ? (i << k) + (1 << (k - 1)) : i, fj = k ? (j << k) + (1 << (k - 1)) : j;   // the full-resolution pixel this output is
  uint8_t* tgt = q.target + q.target_off[k] + (long long)b * hk * wk + r;
  float* dat = q.data + (long long)b * q.C * q.h * q.w + r;   // scale 0 only
  const long long plane = (long long)q.h * q.w;

  const ldiff_seg_sample sp = q.samples[b];
  bool ok = sp.case_index >= 0 && sp.case_index < q.n_cases;
  ldiff_seg_case cs{};
  if (ok) {
    cs = q.cases[sp.case_index];
    const long long fbytes = (long long)q.C * cs.H * cs.stride * 4, lbytes = (long long)cs.H * cs.label_stride;
    ok = cs.H >= 1 && cs.W >= 1 && cs.stride >= cs.W && cs.label_stride >= cs.W && cs.coef_off >= 0 && cs.raw_off >= 0 && cs.label_off >= 0 &&
         ((cs.coef_off | cs.raw_off) & 3) == 0 &&
         cs.coef_off + fbytes <= q.arena_bytes && cs.raw_off + fbytes <= q.arena_bytes && cs.label_off + lbytes <= q.arena_bytes;
  }
  if (!ok) {   // a table row that points outside the arena reads nothing
    *tgt = 0;
    if (k == 0) for (int c = 0; c < q.C; ++c) dat[c * plane] = 0.f;
    return;
  }
  const int H = cs.H, W = cs.W;
  const uint8_t* lab = q.arena + cs.label_off;
  const long long cplane = (long long)H * cs.stride;

  if (sp.copy) {
    const int y = (int)sp.m[0] * fi + (int)sp.m[2], x = (int)sp.m[4] * fj + (int)sp.m[5];
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    *tgt = in ? lab[(long long)y * cs.label_stride + x] : (uint8_t)0;
    if (k == 0) {
      const float* raw = reinterpret_cast<const float*>(q.arena + cs.raw_off) + (long long)y * cs.stride + x;
      for (int c = 0; c < q.C; ++c) dat[c * plane] = in ? raw[c * cplane] : 0.f;
    }
    return;
  }

  const float y = fmaf(sp.m[0], (float)fi, fmaf(sp.m[1], (float)fj, sp.m[2]));
  const float x = fmaf(sp.m[3], (float)fi, fmaf(sp.m[4], (float)fj, sp.m[5]));
  *tgt = (uint8_t)vote_label(lab, H, W, cs.label_stride, y, x);
  if (k != 0) return;
  if (!inside(y, x, H, W)) {
    for (int c = 0; c < q.C; ++c) dat[c * plane] = 0.f;
    return;
  }
  const float fy = floorf(y), fx = floorf(x);
  float wy[4], wx[4];
  bspline3(y - fy, wy);
  bspline3(x - fx, wx);
  int iy[4], ix[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) { iy[a] = mirror_index((int)fy - 1 + a, H) * cs.stride; ix[a] = mirror_index((int)fx - 1 + a, W); }
  const float* coef = reinterpret_cast<const float*>(q.arena + cs.coef_off);
  for (int c = 0; c < q.C; ++c) {
    const float* cp = coef + c * cplane;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float row = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) row = fmaf(wx[t], cp[iy[a] + ix[t]], row);
      acc = fmaf(wy[a], row, acc);
    }
    dat[c * plane] = acc;
  }
}

// ---- intensity chain ---------------------------------------------------------------------------------------------------------------------
struct IntensityParams {
  float* data; const ldiff_seg_sample* samples; const ldiff_seg_chan* chans;
  int B, C, h, w;
  const float* normal; unsigned long long seed;
  float* ws;
};

template <bool VEC, class F>
__device__ __forceinline__ void map_plane(float* p, int n, F f) {   // p[i] = f(p[i], i)
  if constexpr (VEC) {
    float4* q = reinterpret_cast<float4*>(p);
    for (int v = threadIdx.x; v < n / 4; v += IT) {
      float4 x = q[v];
      x.x = f(x.x, 4 * v); x.y = f(x.y, 4 * v + 1); x.z = f(x.z, 4 * v + 2); x.w = f(x.w, 4 * v + 3);
      q[v] = x;
    }
  } else {
    for (int i = threadIdx.x; i < n; i += IT) p[i] = f(p[i], i);
  }
}
template <bool VEC, class F>
__device__ __forceinline__ void visit_plane(const float* p, int n, F f) {   // f(p[i]) in the thread's walk order
  if constexpr (VEC) {
    const float4* q = reinterpret_cast<const float4*>(p);
    for (int v = threadIdx.x; v < n / 4; v += IT) {
      const float4 x = q[v];
      f(x.x); f(x.y); f(x.z); f(x.w);
    }
  } else {
    for (int i = threadIdx.x; i < n; i += IT) f(p[i]);
  }
}

enum { R_SUM = 0, R_MIN = 1, R_MAX = 2 };
template <int OP> __device__ __forceinline__ float combine(float a, float b) { return OP == R_SUM ? a + b : (OP == R_MIN ? fminf(a, b) : fmaxf(a, b)); }
// every thread returns the same value: butterfly over the wave, then the wave partials in wave order
template <int OP>
__device__ __forceinline__ float block_reduce(float v, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = combine<OP>(v, __shfl_xor(v, o));
  __syncthreads();   // the previous reduction's readers are done with `red`
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int wv = 1; wv < IW; ++wv) r = combine<OP>(r, red[wv]);
  return r;
}

template <bool VEC>
__device__ __forceinline__ void plane_sum_min_max(const float* p, int n, float* red, float& sum, float& lo, float& hi) {
  float s = 0.f, a = INFINITY, z = -INFINITY;
  visit_plane<VEC>(p, n, [&](float x) { s += x; a = fminf(a, x); z = fmaxf(z, x); });
  sum = block_reduce<R_SUM>(s, red);
  lo = block_reduce<R_MIN>(a, red);
  hi = block_reduce<R_MAX>(z, red);
}
template <bool VEC>
__device__ __forceinline__ float plane_sum(const float* p, int n, float* red) {
  float s = 0.f;
  visit_plane<VEC>(p, n, [&](float x) { s += x; });
  return block_reduce<R_SUM>(s, red);
}
template <bool VEC>
__device__ __forceinline__ float plane_std(const float* p, int n, float mean, float* red) {   // population std about a given mean
  float s = 0.f;
  visit_plane<VEC>(p, n, [&](float x) { const float d = x - mean; s = fmaf(d, d, s); });
  return sqrtf(block_reduce<R_SUM>(s, red) / (float)n);
}

__device__ __forceinline__ int reflect_index(int i, int n) {   // scipy 'reflect': (d c b a | a b c d | d c b a)
  while (i < 0 || i >= n) {
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
  }
  return i;
}

// four standard normals of one Philox counter: Box-Muller on (words 0, 1) and (words 2, 3)
__device__ __forceinline__ void normal4(unsigned long long ctr, unsigned long long key, float z[4]) {
  unsigned r[4];
  philox4x32_10(ctr, key, r);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float u1 = (float)((r[2 * k] >> 8) + 1u) * (1.0f / 16777216.0f);   // (0, 1]
    const float u2 = (float)(r[2 * k + 1] >> 8) * (1.0f / 16777216.0f);      // [0, 1)
    const float rad = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincospif(2.f * u2, &sn, &cs);
    z[2 * k] = rad * cs;
    z[2 * k + 1] = rad * sn;
  }
}

// GammaTransform(retain_stats=True) of one plane
template <bool VEC>
__device__ __forceinline__ void gamma_plane(float* p, int n, float gamma, bool invert, float* red) {
  __syncthreads();
  if (invert) { map_plane<VEC>(p, n, [](float x, int) { return -x; }); __syncthreads(); }
  float sum, lo, hi;
  plane_sum_min_max<VEC>(p, n, red, sum, lo, hi);
  const float m = sum / (float)n;
  const float s = plane_std<VEC>(p, n, m, red);
  const float r = hi - lo, den = r + 1e-7f;
  __syncthreads();
  map_plane<VEC>(p, n, [=](float x, int) { return fmaf(powf((x - lo) / den, gamma), r, lo); });
  __syncthreads();
  const float m2 = plane_sum<VEC>(p, n, red) / (float)n;
  const float d2 = plane_std<VEC>(p, n, m2, red) + 1e-8f;
  __syncthreads();
  map_plane<VEC>(p, n, [=](float x, int) {
    const float y = fmaf((x - m2) / d2, s, m);
    return invert ? -y : y;
  });
  __syncthreads();
}

// ---- cubic B-spline prefilter of one plane by one workgroup ------------------------------------------------------------------------------
// scipy.ndimage.spline_filter(order=3, mode='mirror') in place on P [H, W] (row stride `stride`), axis 0 then axis 1; nnunet_data.spline_coefficients
// is its float64 statement.  Per line of n >= 2 samples (n == 1: untouched), pole z = sqrt(3) - 2:
//   c+[0] = 6 sum_k wgt(k) x[k]          n > 64: wgt(k) = z^k, k < 64;  n <= 64: the mirrored signal's exact periodic sum, wgt(0) = 1,
//                                        wgt(n-1) = z^(n-1), wgt(k) = z^k + z^(2n-2-k), the whole over 1 - z^(2n-2)
//   c+[k] = 6 x[k] + z c+[k-1]
//   c[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]),   c[k] = z (c[k+1] - c+[k])
// Axis 0: one thread per column walks it serially (neighbouring threads read neighbouring addresses); the SPLINE_WALK loads of the next group are
// issued ahead of the dependent fmas of this one (the pass is bound by the loads' latency, not by the fma chain).  Axis 1: one wave per row, lanes along the row, so the loads coalesce too; both recursions are
// first-order linear scans, y[k] = v[k] + z y[k-1], done per 64-sample chunk by six shuffle steps (y += z^d shifted(y, d), d = 1 .. 32) plus
// z^(lane+1) times the carry of the chunk before.  Only that last fma depends on the chunk before, so SPLINE_GROUP chunks are loaded and scanned
// together and then chained; a line of at most 64 SPLINE_GROUP samples stays in registers from its load to its one store.  The anti-causal pass is
// the mirrored scan over the same chunks from the last one down.  `pw`: z^k, k < 128, in LDS.
constexpr int SPLINE_PAD = 12, SPLINE_HORIZON = 64, SPLINE_POWERS = 128, SPLINE_WALK = 8, SPLINE_GROUP = 5;
constexpr float SPLINE_POLE = -0.26794919243112270647f, SPLINE_GAIN = 6.f, SPLINE_LAST = 0.28867513459481288225f;   // z, (1 - z)(1 - 1/z), z / (z^2 - 1)

__device__ __forceinline__ void spline_powers(float* pw) {   // ends with a barrier
  if (threadIdx.x < SPLINE_POWERS) {
    double v = 1.0;
    for (int k = 0; k < (int)threadIdx.x; ++k) v *= -0.26794919243112270647;
    pw[threadIdx.x] = (float)v;
  }
  __syncthreads();
}

__device__ __forceinline__ float spline_init_weight(int k, int n, const float* pw) {   // k < min(n, SPLINE_HORIZON)
  if (n > SPLINE_HORIZON || k == 0) return pw[k];
  return k == n - 1 ? pw[k] : pw[k] + pw[2 * n - 2 - k];
}
__device__ __forceinline__ float spline_init_scale(int n, const float* pw) {
  return n > SPLINE_HORIZON ? SPLINE_GAIN : SPLINE_GAIN / (1.f - pw[2 * n - 2]);
}

// y[lane] = sum_d z^d v[lane - d] over the chunk's lanes below (DOWN: v[lane + d], the lanes above); the caller adds the carry's share
template <bool DOWN>
__device__ __forceinline__ float spline_wave_scan(float v, const float* pw, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float t = DOWN ? __shfl_down(v, d) : __shfl_up(v, d);
    if (DOWN ? lane + d < 64 : lane >= d) v = fmaf(pw[d], t, v);
  }
  return v;
}

__device__ void spline_prefilter_plane(float* P, int H, int W, int stride, const float* pw) {
  if (H >= 2) {   // axis 0
    const int n = H, hz = min(n, SPLINE_HORIZON);
    const float scale = spline_init_scale(n, pw);
    for (int j = threadIdx.x; j < W; j += IT) {
      float* c = P + j;   // H * stride < 2^30: every index below fits 32 bits
      float s = 0.f;
      for (int k = 0; k < hz; ++k) s = fmaf(spline_init_weight(k, n, pw), c[k * stride], s);
      float cur = s * scale, before = 0.f;
      c[0] = cur;
      float x[SPLINE_WALK], nx[SPLINE_WALK];
#pragma unroll
      for (int u = 0; u < SPLINE_WALK; ++u) x[u] = 1 + u < n ? c[(1 + u) * stride] : 0.f;
      for (int k0 = 1; k0 < n; k0 += SPLINE_WALK) {
#pragma unroll
        for (int u = 0; u < SPLINE_WALK; ++u)   // the next group, none of it written yet
          nx[u] = k0 + SPLINE_WALK + u < n ? c[(k0 + SPLINE_WALK + u) * stride] : 0.f;
#pragma unroll
        for (int u = 0; u < SPLINE_WALK; ++u)
          if (k0 + u < n) {
            before = cur;
            cur = fmaf(SPLINE_POLE, cur, SPLINE_GAIN * x[u]);
            c[(k0 + u) * stride] = cur;
          }
#pragma unroll
        for (int u = 0; u < SPLINE_WALK; ++u) x[u] = nx[u];
      }
      cur = SPLINE_LAST * fmaf(SPLINE_POLE, before, cur);
      c[(n - 1) * stride] = cur;
#pragma unroll
      for (int u = 0; u < SPLINE_WALK; ++u) x[u] = n - 2 - u >= 0 ? c[(n - 2 - u) * stride] : 0.f;
      for (int k0 = n - 2; k0 >= 0; k0 -= SPLINE_WALK) {
#pragma unroll
        for (int u = 0; u < SPLINE_WALK; ++u)   // still the causal pass's values
          nx[u] = k0 - SPLINE_WALK - u >= 0 ? c[(k0 - SPLINE_WALK - u) * stride] : 0.f;
#pragma unroll
        for (int u = 0; u < SPLINE_WALK; ++u)
          if (k0 - u >= 0) {
            cur = SPLINE_POLE * (cur - x[u]);
            c[(k0 - u) * stride] = cur;
          }
#pragma unroll
        for (int u = 0; u < SPLINE_WALK; ++u) x[u] = nx[u];
      }
    }
  }
  __syncthreads();
  if (W >= 2) {   // axis 1
    const int n = W, hz = min(n, SPLINE_HORIZON), lane = threadIdx.x & 63, chunks = (n + 63) >> 6;
    const bool resident = chunks <= SPLINE_GROUP;   // the whole line stays in registers between the two passes
    const float scale = spline_init_scale(n, pw);
    const float wup = pw[lane + 1], wdown = pw[64 - lane];   // z^distance to the last sample of the chunk below, the first of the chunk above
    for (int row = threadIdx.x >> 6; row < H; row += IW) {   // uniform per wave: every shuffle below runs with all 64 lanes
      float* c = P + row * stride;
      float v[SPLINE_GROUP];   // chunk c0 + g of the current group; a chunk past the line's end holds zeros and stores nothing
#pragma unroll
      for (int g = 0; g < SPLINE_GROUP; ++g) v[g] = (g << 6) + lane < n ? c[(g << 6) + lane] : 0.f;
      float s = lane < hz ? spline_init_weight(lane, n, pw) * v[0] : 0.f;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
      const float first = s * scale;
      float carry = 0.f, last = 0.f, before = 0.f;
      for (int c0 = 0; c0 < chunks; c0 += SPLINE_GROUP) {
#pragma unroll
        for (int g = 0; g < SPLINE_GROUP; ++g) {
          const int k = ((c0 + g) << 6) + lane;
          if (c0 > 0) v[g] = k < n ? c[k] : 0.f;
          v[g] = k == 0 ? first : SPLINE_GAIN * v[g];
        }
#pragma unroll
        for (int g = 0; g < SPLINE_GROUP; ++g) v[g] = spline_wave_scan<false>(v[g], pw, lane);
#pragma unroll
        for (int g = 0; g < SPLINE_GROUP; ++g) {
          const int ci = c0 + g, k = (ci << 6) + lane;
          v[g] = fmaf(wup, carry, v[g]);
          if (!resident && k < n) c[k] = v[g];
          carry = __shfl(v[g], 63);
          if (ci == (n - 1) >> 6) last = __shfl(v[g], (n - 1) & 63);
          if (ci == (n - 2) >> 6) before = __shfl(v[g], (n - 2) & 63);
        }
      }
      const float end = SPLINE_LAST * fmaf(SPLINE_POLE, before, last);
      carry = 0.f;
      // the same groups and chunks from the last one down: a lane re-reads only what it wrote itself, or nothing at all
      for (int c0 = (chunks - 1) / SPLINE_GROUP * SPLINE_GROUP; c0 >= 0; c0 -= SPLINE_GROUP) {
#pragma unroll
        for (int g = 0; g < SPLINE_GROUP; ++g) {
          const int k = ((c0 + g) << 6) + lane;
          if (!resident) v[g] = k < n ? c[k] : 0.f;
          v[g] = k == n - 1 ? end : (k < n ? -SPLINE_POLE * v[g] : 0.f);
        }
#pragma unroll
        for (int g = 0; g < SPLINE_GROUP; ++g) v[g] = spline_wave_scan<true>(v[g], pw, lane);
#pragma unroll
        for (int g = SPLINE_GROUP - 1; g >= 0; --g) {
          const int k = ((c0 + g) << 6) + lane;
          v[g] = fmaf(wdown, carry, v[g]);
          if (k < n) c[k] = v[g];
          carry = __shfl(v[g], 0);
        }
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(IT) void spline_prefilter_kernel(float* planes, int H, int W, int stride) {
  __shared__ float pw[SPLINE_POWERS];
  spline_powers(pw);
  spline_prefilter_plane(planes + (long long)blockIdx.x * H * stride, H, W, stride, pw);
}

// SimulateLowResolutionTransform's target extent of one axis: rint(n zoom) in float32, half to even.  nnunet_data.lowres_shape is the same expression.
__device__ __forceinline__ int lowres_extent(int n, float zoom) { return (int)rintf((float)n * zoom); }

// augment_linear_downsampling_scipy on one plane p [h, w]: order-0 resize to [m0, m1], order-3 resize back (skimage.transform.resize(mode='edge',
// anti_aliasing=False) = scipy.ndimage.zoom(mode='nearest', grid_mode=True) and a clip to the input's range).  P: (m0 + 24) x (m1 + 24) floats.
__device__ void lowres_plane(float* p, int h, int w, int m0, int m1, float* P, const float* pw, float* red) {
  const int Hp = m0 + 2 * SPLINE_PAD, Wp = m1 + 2 * SPLINE_PAD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float lo = INFINITY, hi = -INFINITY;
  // the down-sampled plane d and its edge pad in one walk, a wave per row: P[i, j] = d[clamp(i - 12), clamp(j - 12)], d[i, j] = p[iy(i), ix(j)].
  // (2 i + 1) n stays below 2^31 for n <= 16384 (the launcher's limit); the row's index is formed once per row, the column's once per element.
  for (int i = wave; i < Hp; i += IW) {
    const int di = min(max(i - SPLINE_PAD, 0), m0 - 1);
    const float* src = p + ((2 * di + 1) * h) / (2 * m0) * w;
    for (int j = lane; j < Wp; j += 64) {
      const int dj = min(max(j - SPLINE_PAD, 0), m1 - 1);
      const float v = src[((2 * dj + 1) * w) / (2 * m1)];
      P[i * Wp + j] = v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  lo = block_reduce<R_MIN>(lo, red);
  hi = block_reduce<R_MAX>(hi, red);   // its barriers also order the walk above before the filter
  spline_prefilter_plane(P, Hp, Wp, Wp, pw);
  // the source coordinate of output index i is (i + 1/2) m / n - 1/2 = num / (2 n): floor and fraction in integers (num > -2 n)
  for (int i = wave; i < h; i += IW) {
    int ny = (2 * i + 1) * m0 - h, fy = 0;
    if (ny < 0) { fy = -1; ny += 2 * h; } else { fy = ny / (2 * h); ny -= fy * 2 * h; }
    float wy[4];
    bspline3((float)ny / (float)(2 * h), wy);
    const float* r[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) r[a] = P + min(max(fy - 1 + a + SPLINE_PAD, 0), Hp - 1) * Wp;   // the pad keeps every tap inside; the clamp is the guard
    for (int j = lane; j < w; j += 64) {
      int nx = (2 * j + 1) * m1 - w, fx = 0;
      if (nx < 0) { fx = -1; nx += 2 * w; } else { fx = nx / (2 * w); nx -= fx * 2 * w; }
      float wx[4];
      bspline3((float)nx / (float)(2 * w), wx);
      int col[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) col[t] = min(max(fx - 1 + t + SPLINE_PAD, 0), Wp - 1);
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        float row = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) row = fmaf(wx[t], r[a][col[t]], row);
        acc = fmaf(wy[a], row, acc);
      }
      p[i * w + j] = fminf(fmaxf(acc, lo), hi);
    }
  }
}

// LR: the chain with SimulateLowResolutionTransform between contrast and the gammas; a plane's workspace is then (h + 24) (w + 24) floats.
template <bool VEC, bool LR = false>
__global__ __launch_bounds__(IT) void seg_intensity_kernel(IntensityParams q) {
  __shared__ float red[IW];
  __shared__ float taps[2 * MAX_RADIUS + 1];
  const int pl = blockIdx.x, b = pl / q.C, c = pl - b * q.C, n = q.h * q.w;
  const float noise = q.samples[b].noise_sigma;
  const ldiff_seg_chan ch = q.chans[pl];
  // gaussian_filter's radius; 0 (sigma < 0.125) is the identity there, and beyond MAX_RADIUS (sigma >= 1.875) the row counts as off
  const int radius = ch.blur_sigma > 0.f ? (int)fminf(4.f * ch.blur_sigma + 0.5f, 1e6f) : 0;
  const bool do_noise = noise > 0.f, do_blur = radius >= 1 && radius <= MAX_RADIUS, do_bright = ch.brightness != 1.f, do_contrast = ch.contrast > 0.f,
             do_gi = ch.gamma_inverted > 0.f, do_g = ch.gamma > 0.f;
  int m0 = 0, m1 = 0;
  bool do_lr = false;
  if constexpr (LR) {   // off: zoom outside (0, 1] or NaN, an empty target, or the target is the plane's own shape
    if (ch.lowres_zoom > 0.f && ch.lowres_zoom <= 1.f) {
      m0 = lowres_extent(q.h, ch.lowres_zoom);
      m1 = lowres_extent(q.w, ch.lowres_zoom);
      do_lr = m0 >= 1 && m1 >= 1 && !(m0 == q.h && m1 == q.w);
    }
  }
  if (!(do_noise || do_blur || do_bright || do_contrast || do_lr || do_gi || do_g)) return;
  float* p = q.data + (long long)pl * n;
  float* wsp = q.ws + (long long)pl * (LR ? (q.h + 2 * SPLINE_PAD) * (q.w + 2 * SPLINE_PAD) : n);   // this plane's own workspace

  if (do_noise) {   // GaussianNoiseTransform: x + N(0, sigma), sigma used as the scale
    if (q.normal) {
      const float* z = q.normal + (long long)pl * n;
      map_plane<VEC>(p, n, [=](float x, int i) { return fmaf(noise, z[i], x); });
    } else {
      const unsigned long long off = q.samples[b].philox_offset;
      const long long e0 = (long long)c * n;   // element index inside the sample
      if constexpr (VEC) {
        float4* v4 = reinterpret_cast<float4*>(p);
        for (int v = threadIdx.x; v < n / 4; v += IT) {   // n % 4 == 0: a float4 is one counter
          float z[4];
          normal4(off + (unsigned long long)((e0 >> 2) + v), q.seed, z);
          float4 x = v4[v];
          x.x = fmaf(noise, z[0], x.x); x.y = fmaf(noise, z[1], x.y); x.z = fmaf(noise, z[2], x.z); x.w = fmaf(noise, z[3], x.w);
          v4[v] = x;
        }
      } else {
        for (int i = threadIdx.x; i < n; i += IT) {
          float z[4];
          const long long e = e0 + i;
          normal4(off + (unsigned long long)(e >> 2), q.seed, z);
          p[i] = fmaf(noise, z[e & 3], p[i]);
        }
      }
    }
  }

  if (do_blur) {   // scipy.ndimage.gaussian_filter(x, sigma): axis 0 then axis 1, 'reflect'
    if ((int)threadIdx.x <= 2 * radius) {
      const float d = (float)((int)threadIdx.x - radius) / ch.blur_sigma;
      taps[threadIdx.x] = expf(-0.5f * d * d);
    }
    __syncthreads();
    float tsum = 0.f;
    for (int k = 0; k <= 2 * radius; ++k) tsum += taps[k];
    const float inv = 1.f / tsum;
    float* tmp = wsp;
    const int h = q.h, w = q.w;
    for (int e = threadIdx.x; e < n; e += IT) {
      const int i = e / w, j = e - i * w;
      float acc = 0.f;
      for (int k = -radius; k <= radius; ++k) acc = fmaf(taps[k + radius] * inv, p[reflect_index(i + k, h) * w + j], acc);
      tmp[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += IT) {
      const int i = e / w, j = e - i * w;
      float acc = 0.f;
      for (int k = -radius; k <= radius; ++k) acc = fmaf(taps[k + radius] * inv, tmp[i * w + reflect_index(j + k, w)], acc);
      p[e] = acc;
    }
  }

  if (do_bright) {   // BrightnessMultiplicativeTransform
    __syncthreads();
    const float mult = ch.brightness;
    map_plane<VEC>(p, n, [=](float x, int) { return x * mult; });
  }

  if (do_contrast) {   // ContrastAugmentationTransform(preserve_range=True)
    __syncthreads();
    float sum, lo, hi;
    plane_sum_min_max<VEC>(p, n, red, sum, lo, hi);
    const float m = sum / (float)n, f = ch.contrast;
    __syncthreads();
    map_plane<VEC>(p, n, [=](float x, int) { return fminf(fmaxf(fmaf(x - m, f, m), lo), hi); });
  }

  if constexpr (LR) {
    if (do_lr) {   // SimulateLowResolutionTransform: order 0 down, order 3 up, clipped to the down-sampled plane's range
      __shared__ float pw[SPLINE_POWERS];
      spline_powers(pw);   // its barrier also puts the steps above before the walk over the plane
      lowres_plane(p, q.h, q.w, m0, m1, wsp, pw, red);
    }
  }

  if (do_gi) gamma_plane<VEC>(p, n, ch.gamma_inverted, true, red);
  if (do_g) gamma_plane<VEC>(p, n, ch.gamma, false, red);
}

}  // namespace

void launch_seg_sample(const void* arena, long long arena_bytes, const ldiff_seg_case* cases, int n_cases, const ldiff_seg_sample* samples, int B, int C, int h,
                       int w, int n_scales, float* data, uint8_t* target, hipStream_t s) {
  LDIFF_CHECK(B >= 0 && C >= 1 && h >= 1 && w >= 1 && n_cases >= 1 && arena_bytes >= 0, LDIFF_ERR_INVALID, "seg_sample: bad extents (B %d, C %d, patch %d x %d, %d cases)",
              B, C, h, w, n_cases);
  LDIFF_CHECK(n_scales >= 1 && n_scales <= MAX_SCALES, LDIFF_ERR_INVALID, "seg_sample: n_scales %d out of range [1,%d]", n_scales, MAX_SCALES);
  const int div = 1 << (n_scales - 1);
  LDIFF_CHECK(h % div == 0 && w % div == 0, LDIFF_ERR_INVALID, "seg_sample: patch %d x %d is not divisible by 2^(n_scales - 1) = %d", h, w, div);
  LDIFF_CHECK((long long)h * w < (1ll << 30) && B <= 65535, LDIFF_ERR_INVALID, "seg_sample: patch %d x %d or batch %d too large", h, w, B);
  if (B == 0) return;
  LDIFF_CHECK(arena && cases && samples && data && target, LDIFF_ERR_INVALID, "seg_sample: null argument");
  LDIFF_CHECK((reinterpret_cast<uintptr_t>(arena) & 15) == 0 && (reinterpret_cast<uintptr_t>(data) & 3) == 0, LDIFF_ERR_INVALID, "seg_sample: arena / data misaligned");
  SampleParams q{};
  q.arena = static_cast<const unsigned char*>(arena); q.arena_bytes = arena_bytes; q.cases = cases; q.n_cases = n_cases; q.samples = samples;
  q.B = B; q.C = C; q.h = h; q.w = w; q.n_scales = n_scales; q.data = data; q.target = target;
  long long off = 0;
  int first = 0;
  for (int k = 0; k < n_scales; ++k) {
    q.first[k] = first;
    q.target_off[k] = off;
    first += (h >> k) * (w >> k);
    off += (long long)B * (h >> k) * (w >> k);
  }
  for (int k = n_scales; k <= MAX_SCALES; ++k) q.first[k] = first;
  ProfScope prof("seg_sample", 0.0, (double)B * h * w * (C * 4.0 * 17 + 6.0), s);
  hipLaunchKernelGGL(seg_sample_kernel, dim3((first + ST - 1) / ST, B), dim3(ST), 0, s, q);
  HIP_CHECK(hipGetLastError());
}

long long seg_intensity_ws_bytes(int B, int C, int h, int w) { return (long long)B * C * h * w * 4; }
long long seg_intensity_lr_ws_bytes(int B, int C, int h, int w) { return (long long)B * C * (h + 2 * SPLINE_PAD) * (w + 2 * SPLINE_PAD) * 4; }

void launch_seg_intensity(float* data, const ldiff_seg_sample* samples, const ldiff_seg_chan* chans, int B, int C, int h, int w, const float* normal,
                          unsigned long long seed, void* ws, long long ws_bytes, hipStream_t s, bool lowres) {
  const char* name = lowres ? "seg_intensity_lr" : "seg_intensity";
  LDIFF_CHECK(B >= 0 && C >= 1 && h >= 1 && w >= 1 && (long long)h * w < (1ll << 30) && (long long)B * C < (1ll << 31), LDIFF_ERR_INVALID,
              "%s: bad extents (B %d, C %d, patch %d x %d)", name, B, C, h, w);
  // the low-resolution step forms (2 i + 1) n and indexes its padded plane in 32 bits
  LDIFF_CHECK(!lowres || (h <= 16384 && w <= 16384), LDIFF_ERR_INVALID, "%s: patch %d x %d too large (16384 per axis)", name, h, w);
  if (B == 0) return;
  LDIFF_CHECK(data && samples && chans && ws, LDIFF_ERR_INVALID, "%s: null argument", name);
  const long long need = lowres ? seg_intensity_lr_ws_bytes(B, C, h, w) : seg_intensity_ws_bytes(B, C, h, w);
  LDIFF_CHECK(ws_bytes >= need, LDIFF_ERR_INVALID, "%s: workspace of %lld bytes, %lld needed (ldiff_op_%s_ws_bytes)", name, ws_bytes, need, name);
  LDIFF_CHECK((reinterpret_cast<uintptr_t>(data) & 3) == 0 && (reinterpret_cast<uintptr_t>(ws) & 3) == 0 && (reinterpret_cast<uintptr_t>(normal) & 3) == 0,
              LDIFF_ERR_INVALID, "%s: data / workspace / normal not aligned to float", name);
  IntensityParams q{data, samples, chans, B, C, h, w, normal, seed, static_cast<float*>(ws)};
  const bool vec = (h * w) % 4 == 0 && (reinterpret_cast<uintptr_t>(data) & 15) == 0;   // every plane then starts on a 16-byte boundary
  ProfScope prof(name, 0.0, (double)B * C * h * w * 8.0, s);
  if (lowres) {
    if (vec) hipLaunchKernelGGL((seg_intensity_kernel<true, true>), dim3(B * C), dim3(IT), 0, s, q);
    else hipLaunchKernelGGL((seg_intensity_kernel<false, true>), dim3(B * C), dim3(IT), 0, s, q);
  } else {
    if (vec) hipLaunchKernelGGL(seg_intensity_kernel<true>, dim3(B * C), dim3(IT), 0, s, q);
    else hipLaunchKernelGGL(seg_intensity_kernel<false>, dim3(B * C), dim3(IT), 0, s, q);
  }
  HIP_CHECK(hipGetLastError());
}

void launch_spline_prefilter(float* planes, int n_planes, int H, int W, int stride, hipStream_t s) {
  LDIFF_CHECK(n_planes >= 0, LDIFF_ERR_INVALID, "spline_prefilter: n_planes %d is negative", n_planes);
  LDIFF_CHECK(H >= 1, LDIFF_ERR_INVALID, "spline_prefilter: H %d must be at least 1", H);
  LDIFF_CHECK(W >= 1, LDIFF_ERR_INVALID, "spline_prefilter: W %d must be at least 1", W);
  LDIFF_CHECK(stride >= W, LDIFF_ERR_INVALID, "spline_prefilter: stride %d is below W %d", stride, W);
  LDIFF_CHECK((long long)H * stride < (1ll << 30), LDIFF_ERR_INVALID, "spline_prefilter: H * stride = %lld must stay below 2^30", (long long)H * stride);
  if (n_planes == 0) return;
  LDIFF_CHECK(planes, LDIFF_ERR_INVALID, "spline_prefilter: null argument planes_f32");
  LDIFF_CHECK((reinterpret_cast<uintptr_t>(planes) & 3) == 0, LDIFF_ERR_INVALID, "spline_prefilter: planes_f32 not aligned to float");
  ProfScope prof("spline_prefilter", 0.0, (double)n_planes * H * W * 24.0, s);
  hipLaunchKernelGGL(spline_prefilter_kernel, dim3(n_planes), dim3(IT), 0, s, planes, H, W, stride);
  HIP_CHECK(hipGetLastError());
}
