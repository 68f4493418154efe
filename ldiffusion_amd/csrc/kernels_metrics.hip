// Mask scoring (include/ldiff.h "Metrics"): per-image confusion matrices on the device, and the reference's four metrics from one matrix on the host.
//
// confusion<PRED, TGT, LUTS>: conf[b, t, p] += #{pixels of image b with target t and prediction p} (evaluate.py:32-35 `hist`), dropped[b] += the pixels
// whose target or prediction is no class.  Memory-bound: 2 bytes per pixel in mask form, 4 C + 1 in logit form.
//   work     one unit = a contiguous chunk of ONE image; units are dealt to a grid capped at GRID_PER_CU workgroups per CU
//   loads    mask form: a scalar head up to the prediction's 16-byte boundary, 16 pixels (one 16-byte load per operand) per lane on the body, a scalar tail;
//            where target and prediction disagree on that boundary (views at different offsets) the whole chunk takes the scalar walk.
//            logit form: the C planes of a run of 4 (f32) / 8 (f16) pixels per lane, one 16-byte load per plane, where the planes share a 16-byte phase
//            (H W a multiple of the run); else one pixel per lane, which is still one coalesced load per plane.  The arg-max stays in registers.
//   counting per-wave LDS histograms of C*C + 1 uint32 bins (the last one = dropped).  Masks are large constant regions, the worst case for LDS atomics
//            (64 lanes on one bin), so a wave whose lanes agree (ballot against the first active lane's bin) adds its lane count from one lane; a lane
//            whose 16 pixels are one bin in a wave of such lanes adds 16 x the lane count.  Other waves use plain LDS atomic adds.
//   flush    once per unit: the waves' histograms are summed in LDS and every NON-ZERO bin becomes one 64-bit integer atomicAdd.  Integer adds commute:
//            the matrix is exact and bitwise reproducible whatever the arrival order.
#include "common.h"

#include <math.h>
#include <type_traits>

namespace {

constexpr int MAX_C = 32, THREADS = 256, WAVES = THREADS / 64, BINS_MAX = MAX_C * MAX_C + 1;
constexpr int GRID_PER_CU = 4;
constexpr long long MIN_CHUNK = 8192;   // pixels: two body iterations of the mask form; a flush (<= C*C atomics) per this many pixels is noise
enum { PRED_U8 = 0, PRED_F32 = 1, PRED_F16 = 2, TGT_U8 = 0, TGT_I64 = 1 };

struct ConfusionParams {
  const void* pred; const void* target;
  const uint8_t* pred_lut; const uint8_t* target_lut;
  int B, C;
  long long HW, chunk;      // pixels per image / per unit
  int chunks;               // units per image
  long long units;          // B * chunks
  unsigned long long* conf; unsigned long long* dropped;
};

// One pixel slot of every lane: `bin` in [0, C*C] (C*C = dropped), `active` lanes only.
__device__ __forceinline__ void count_slot(unsigned* hist, int bin, bool active, unsigned weight) {
  const unsigned long long mask = __ballot(active);
  if (mask == 0) return;
  const int first = __ffsll((long long)mask) - 1;
  const int b0 = __shfl(bin, first);
  if (__ballot(active && bin == b0) == mask) {
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[b0], weight * (unsigned)__popcll(mask));
  } else if (active) {
    atomicAdd(&hist[bin], weight);
  }
}

__device__ __forceinline__ int bin_of(unsigned t, unsigned p, int C) { return (t < (unsigned)C && p < (unsigned)C) ? (int)(t * C + p) : C * C; }

template <int TGT, bool LUTS>
__device__ __forceinline__ unsigned load_target(const void* target, long long i, const uint8_t* tl) {
  if constexpr (TGT == TGT_U8) {
    const unsigned t = static_cast<const uint8_t*>(target)[i];
    return LUTS ? tl[t] : t;
  } else {
    const unsigned long long t = static_cast<const unsigned long long*>(target)[i];   // negative labels compare as huge
    return t < (unsigned long long)MAX_C ? (unsigned)t : 0xffu;
  }
}

// argmax_u8_kernel's rule (kernels_elem.hip), bit for bit: the first maximal class; a pixel with any NaN or +inf logit is class 0
struct ArgMax {
  float best; int bi; bool bad;
  __device__ __forceinline__ void first(float v) { best = v; bi = 0; bad = v != v || v == INFINITY; }
  __device__ __forceinline__ void next(float v, int c) { bad |= v != v || v == INFINITY; if (v > best) { best = v; bi = c; } }
  __device__ __forceinline__ unsigned label() const { return bad ? 0u : (unsigned)bi; }
};

template <int PRED, int TGT, bool LUTS>
__global__ __launch_bounds__(THREADS) void confusion_kernel(ConfusionParams q) {
  __shared__ unsigned hist[WAVES * BINS_MAX];
  __shared__ uint8_t luts[LUTS ? 512 : 1];
  const int C = q.C, bins = C * C + 1, tid = threadIdx.x;
  unsigned* wh = hist + (tid >> 6) * bins;
  const uint8_t* pl = luts;
  const uint8_t* tl = luts + (LUTS ? 256 : 0);
  if constexpr (LUTS) {
    luts[tid] = q.pred_lut ? q.pred_lut[tid] : (uint8_t)tid;       // THREADS == 256 entries; an absent table is the identity
    luts[256 + tid] = q.target_lut ? q.target_lut[tid] : (uint8_t)tid;
  }
  for (long long u = blockIdx.x; u < q.units; u += gridDim.x) {
    for (int i = tid; i < WAVES * bins; i += THREADS) hist[i] = 0;
    __syncthreads();
    const int b = (int)(u / q.chunks);
    const long long start = (u - (long long)b * q.chunks) * q.chunk;
    const long long n = (q.HW - start < q.chunk) ? q.HW - start : q.chunk;   // >= 1: chunks = ceil(HW / chunk)
    const long long tbase = (long long)b * q.HW + start;                      // first pixel of the unit in the target (and in a mask prediction)

    if constexpr (PRED == PRED_U8) {
      const uint8_t* pp = static_cast<const uint8_t*>(q.pred) + tbase;
      auto scalar_walk = [&](long long lo, long long hi) {   // pixels [lo, hi) of the unit, one per lane
        for (long long i0 = lo; i0 < hi; i0 += THREADS) {     // uniform trip count: the ballots see whole waves
          const long long i = i0 + tid;
          const bool act = i < hi;
          int bin = 0;
          if (act) {
            const unsigned p = LUTS ? pl[pp[i]] : pp[i];
            bin = bin_of(load_target<TGT, LUTS>(q.target, tbase + i, tl), p, C);
          }
          count_slot(wh, bin, act, 1u);
        }
      };
      if constexpr (TGT == TGT_U8) {
        const uint8_t* tp = static_cast<const uint8_t*>(q.target) + tbase;
        long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(pp) & 15)) & 15);
        if (head > n) head = n;
        const bool same_phase = ((reinterpret_cast<uintptr_t>(pp) ^ reinterpret_cast<uintptr_t>(tp)) & 15) == 0;
        const long long vecs = same_phase ? (n - head) / 16 : 0;
        scalar_walk(0, head);
        for (long long v0 = 0; v0 < vecs; v0 += THREADS) {
          const long long v = v0 + tid;
          const bool act = v < vecs;
          uint4 pv = make_uint4(0, 0, 0, 0), tv = make_uint4(0, 0, 0, 0);
          if (act) {
            pv = *reinterpret_cast<const uint4*>(pp + head + v * 16);
            tv = *reinterpret_cast<const uint4*>(tp + head + v * 16);
          }
          const unsigned pw[4] = {pv.x, pv.y, pv.z, pv.w}, tw[4] = {tv.x, tv.y, tv.z, tv.w};
          // a lane whose 16 pixels are one (target, prediction) pair: the common case inside a constant region
          const unsigned ps = (pw[0] & 255u) * 0x01010101u, ts = (tw[0] & 255u) * 0x01010101u;
          const bool flat = pw[0] == ps && pw[1] == ps && pw[2] == ps && pw[3] == ps && tw[0] == ts && tw[1] == ts && tw[2] == ts && tw[3] == ts;
          const unsigned long long am = __ballot(act);
          if (__ballot(act && flat) == am) {
            const unsigned p = pw[0] & 255u, t = tw[0] & 255u;
            count_slot(wh, bin_of(LUTS ? tl[t] : t, LUTS ? pl[p] : p, C), act, 16u);
          } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
              const unsigned p = (pw[j >> 2] >> (8 * (j & 3))) & 255u, t = (tw[j >> 2] >> (8 * (j & 3))) & 255u;
              count_slot(wh, bin_of(LUTS ? tl[t] : t, LUTS ? pl[p] : p, C), act, 1u);
            }
          }
        }
        scalar_walk(head + vecs * 16, n);
      } else {
        // int64 labels: 16 bytes = two labels per lane on the body, the prediction's two bytes beside them
        const unsigned long long* tp = static_cast<const unsigned long long*>(q.target) + tbase;
        long long head = (reinterpret_cast<uintptr_t>(tp) & 15) ? 1 : 0;   // labels are 8-byte aligned (checked by the launcher)
        if (head > n) head = n;
        const long long pairs = (n - head) / 2;
        scalar_walk(0, head);
        for (long long v0 = 0; v0 < pairs; v0 += THREADS) {
          const long long v = v0 + tid;
          const bool act = v < pairs;
          int bin0 = 0, bin1 = 0;
          if (act) {
            const ulonglong2 t2 = *reinterpret_cast<const ulonglong2*>(tp + head + v * 2);
            const unsigned p0 = pp[head + v * 2], p1 = pp[head + v * 2 + 1];
            bin0 = bin_of(t2.x < (unsigned long long)MAX_C ? (unsigned)t2.x : 0xffu, p0, C);
            bin1 = bin_of(t2.y < (unsigned long long)MAX_C ? (unsigned)t2.y : 0xffu, p1, C);
          }
          count_slot(wh, bin0, act, 1u);
          count_slot(wh, bin1, act, 1u);
        }
        scalar_walk(head + pairs * 2, n);
      }
    } else {
      using T = typename std::conditional<PRED == PRED_F32, float, f16>::type;
      constexpr int RUN = 16 / (int)sizeof(T);   // pixels of one 16-byte load
      const T* lp = static_cast<const T*>(q.pred) + (long long)b * C * q.HW + start;   // plane 0 of the unit; plane c is c * HW further
      auto scalar_walk = [&](long long lo, long long hi) {
        for (long long i0 = lo; i0 < hi; i0 += THREADS) {
          const long long i = i0 + tid;
          const bool act = i < hi;
          int bin = 0;
          if (act) {
            ArgMax a;
            a.first((float)lp[i]);
            for (int c = 1; c < C; ++c) a.next((float)lp[(long long)c * q.HW + i], c);
            bin = bin_of(load_target<TGT, LUTS>(q.target, tbase + i, tl), a.label(), C);
          }
          count_slot(wh, bin, act, 1u);
        }
      };
      // every plane has plane 0's 16-byte phase only where a plane is a whole number of runs
      const bool planes_in_phase = q.HW % RUN == 0;   // (the launcher checked that the logits are aligned to their element)
      long long head = (long long)(((16 - (reinterpret_cast<uintptr_t>(lp) & 15)) & 15) / sizeof(T));
      if (head > n) head = n;
      const long long vecs = planes_in_phase ? (n - head) / RUN : 0;
      scalar_walk(0, head);
      for (long long v0 = 0; v0 < vecs; v0 += THREADS) {
        const long long v = v0 + tid;
        const bool act = v < vecs;
        int bin[RUN];
#pragma unroll
        for (int j = 0; j < RUN; ++j) bin[j] = 0;
        if (act) {
          const long long i = head + v * RUN;
          ArgMax a[RUN];
          for (int c = 0; c < C; ++c) {
            const uint4 raw = *reinterpret_cast<const uint4*>(lp + (long long)c * q.HW + i);
            float x[RUN];
            if constexpr (PRED == PRED_F32) {
              x[0] = __builtin_bit_cast(float, raw.x); x[1] = __builtin_bit_cast(float, raw.y);
              x[2] = __builtin_bit_cast(float, raw.z); x[3] = __builtin_bit_cast(float, raw.w);
            } else {
              const f16x8 h = __builtin_bit_cast(f16x8, raw);
#pragma unroll
              for (int j = 0; j < RUN; ++j) x[j] = (float)h[j];
            }
#pragma unroll
            for (int j = 0; j < RUN; ++j) { if (c == 0) a[j].first(x[j]); else a[j].next(x[j], c); }
          }
#pragma unroll
          for (int j = 0; j < RUN; ++j) bin[j] = bin_of(load_target<TGT, LUTS>(q.target, tbase + i + j, tl), a[j].label(), C);
        }
#pragma unroll
        for (int j = 0; j < RUN; ++j) count_slot(wh, bin[j], act, 1u);
      }
      scalar_walk(head + vecs * RUN, n);
    }

    __syncthreads();
    for (int i = tid; i < bins; i += THREADS) {
      unsigned long long s = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) s += hist[w * bins + i];
      if (s == 0) continue;
      if (i < C * C) atomicAdd(q.conf + (long long)b * C * C + i, s);
      else if (q.dropped) atomicAdd(q.dropped + b, s);
    }
    __syncthreads();   // the next unit zeroes the histograms
  }
}

int metrics_num_cus() {
  int dev = 0, n = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  return n > 0 ? n : 256;
}

template <int PRED, int TGT, bool LUTS>
void launch_one(const ConfusionParams& q, int grid, hipStream_t s) {
  hipLaunchKernelGGL((confusion_kernel<PRED, TGT, LUTS>), dim3(grid), dim3(THREADS), 0, s, q);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_confusion(const void* pred, int pred_kind, const void* target, int target_kind, const uint8_t* pred_lut, const uint8_t* target_lut, int B, int C, int H, int W,
                      int64_t* conf, int64_t* dropped, hipStream_t s) {
  LDIFF_CHECK(C >= 1 && C <= MAX_C, LDIFF_ERR_INVALID, "confusion: class count %d out of range [1,%d]", C, MAX_C);
  LDIFF_CHECK(pred_kind >= PRED_U8 && pred_kind <= PRED_F16, LDIFF_ERR_INVALID, "confusion: pred_kind %d (0 u8 mask, 1 f32 logits, 2 f16 logits)", pred_kind);
  LDIFF_CHECK(target_kind == TGT_U8 || target_kind == TGT_I64, LDIFF_ERR_INVALID, "confusion: target_kind %d (0 u8, 1 i64)", target_kind);
  LDIFF_CHECK(B >= 0 && H >= 0 && W >= 0, LDIFF_ERR_INVALID, "confusion: negative extent");
  LDIFF_CHECK(!(target_kind == TGT_I64 && (pred_lut || target_lut)), LDIFF_ERR_INVALID, "confusion: a LUT maps 8-bit grey levels; int64 targets take none");
  LDIFF_CHECK(!(pred_kind != PRED_U8 && pred_lut), LDIFF_ERR_INVALID, "confusion: a prediction LUT needs the mask form");
  const long long HW = (long long)H * W;
  if ((long long)B * HW == 0) return;   // empty batch: nothing to count (pointers may be null)
  LDIFF_CHECK(pred && target && conf, LDIFF_ERR_INVALID, "confusion: null pointer");
  LDIFF_CHECK(target_kind != TGT_I64 || (reinterpret_cast<uintptr_t>(target) & 7) == 0, LDIFF_ERR_INVALID, "confusion: int64 target not 8-byte aligned");
  LDIFF_CHECK((reinterpret_cast<uintptr_t>(conf) & 7) == 0 && (reinterpret_cast<uintptr_t>(dropped) & 7) == 0, LDIFF_ERR_INVALID, "confusion: conf / dropped not 8-byte aligned");
  LDIFF_CHECK(pred_kind == PRED_U8 || (reinterpret_cast<uintptr_t>(pred) & (pred_kind == PRED_F32 ? 3 : 1)) == 0, LDIFF_ERR_INVALID, "confusion: logits not aligned to their element size");

  ConfusionParams q{};
  q.pred = pred; q.target = target; q.pred_lut = pred_lut; q.target_lut = target_lut;
  q.B = B; q.C = C; q.HW = HW;
  q.conf = reinterpret_cast<unsigned long long*>(conf);          // two's complement: an unsigned add is the signed add
  q.dropped = reinterpret_cast<unsigned long long*>(dropped);
  const long long cap = (long long)GRID_PER_CU * metrics_num_cus();
  long long per_image = cap / B < 1 ? 1 : cap / B;
  const long long want = (HW + MIN_CHUNK - 1) / MIN_CHUNK;
  if (per_image > want) per_image = want;
  q.chunk = ((HW + per_image - 1) / per_image + 63) / 64 * 64;
  q.chunks = (int)((HW + q.chunk - 1) / q.chunk);
  q.units = (long long)B * q.chunks;
  // a unit's pixels all fit one uint32 bin (x 1: every pixel is counted once)
  LDIFF_CHECK(q.chunk < (1ll << 32), LDIFF_ERR_INVALID, "confusion: %lld pixels per workgroup overflow a 32-bit bin", q.chunk);
  const int grid = (int)(q.units < cap ? q.units : cap);
  const bool luts = pred_lut || target_lut;
  ProfScope prof("confusion", 0.0, (double)B * HW * ((pred_kind == PRED_U8 ? 1.0 : (pred_kind == PRED_F32 ? 4.0 : 2.0) * C) + (target_kind == TGT_U8 ? 1.0 : 8.0)), s);
  if (pred_kind == PRED_U8) {
    if (target_kind == TGT_I64) launch_one<PRED_U8, TGT_I64, false>(q, grid, s);
    else if (luts) launch_one<PRED_U8, TGT_U8, true>(q, grid, s);
    else launch_one<PRED_U8, TGT_U8, false>(q, grid, s);
  } else if (pred_kind == PRED_F32) {
    if (target_kind == TGT_I64) launch_one<PRED_F32, TGT_I64, false>(q, grid, s);
    else if (luts) launch_one<PRED_F32, TGT_U8, true>(q, grid, s);
    else launch_one<PRED_F32, TGT_U8, false>(q, grid, s);
  } else {
    if (target_kind == TGT_I64) launch_one<PRED_F16, TGT_I64, false>(q, grid, s);
    else if (luts) launch_one<PRED_F16, TGT_U8, true>(q, grid, s);
    else launch_one<PRED_F16, TGT_U8, false>(q, grid, s);
  }
}

// ---- host: the reference's four metrics from ONE C x C matrix --------------------------------------------------------------------------------
// Each restates the reference's arithmetic in the reference's number format, one IEEE operation per python / torch operator (volatile keeps the
// compiler from contracting or widening them), on counts the reference forms by summing 0/1 floats or integers.
int seg_metrics_host(const int64_t* conf, int C, ldiff_seg_metrics_out* out) {
  if (!conf || !out || C < 1 || C > MAX_C) {
    ldiff_set_error("seg_metrics: %s", (!conf || !out) ? "null argument" : "class count out of range [1,32]");
    return LDIFF_ERR_INVALID;
  }
  for (int i = 0; i < C * C; ++i)
    if (conf[i] < 0) { ldiff_set_error("seg_metrics: negative count at [%d,%d]", i / C, i % C); return LDIFF_ERR_INVALID; }
  *out = ldiff_seg_metrics_out{};
  out->num_classes = C;
  int64_t row[MAX_C] = {}, col[MAX_C] = {}, total = 0;
  for (int t = 0; t < C; ++t)
    for (int p = 0; p < C; ++p) { row[t] += conf[t * C + p]; col[p] += conf[t * C + p]; total += conf[t * C + p]; }
  // Dice (utils.py:55-82): float32 sums of 0/1 products; 2 TP / (2 TP + FP + FN) in float32; absent from both: 1.  torch.mean of the float32 tensor: the
  // sum in double rounded once, which every float32 summation order of <= 32 values in [0, 1] meets within an ulp
  {
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
      const int64_t tp = conf[c * C + c];
      float d = 1.f;
      if (row[c] != 0 || col[c] != 0) {
        const volatile float TP = (float)tp, FP = (float)(col[c] - tp), FN = (float)(row[c] - tp);
        const volatile float two_tp = 2.f * TP;
        const volatile float den1 = two_tp + FP;
        const volatile float den = den1 + FN;
        d = two_tp / den;   // TP + FP + FN > 0 here: the reference's `== 0` branch (:75-76) is unreachable behind its first test
      }
      out->dice[c] = d;
      acc += (double)d;
    }
    out->dice_mean = (float)(acc / C);
  }
  // IoU (utils.py:84-104): python ints divided as doubles; empty union: skipped (NaN here, flagged); mean over the rest, 1.0 if none
  {
    double acc = 0.0;
    int n = 0;
    for (int c = 0; c < C; ++c) {
      const int64_t inter = conf[c * C + c], uni = row[c] + col[c] - inter;
      if (uni == 0) { out->iou[c] = NAN; out->iou_skipped[c] = 1; continue; }
      out->iou[c] = (double)inter / (double)uni;
      acc += out->iou[c];   // python's sum(): left to right in double
      ++n;
    }
    out->iou_mean = n ? acc / n : 1.0;
  }
  // pixel accuracy (evaluate.py:11-27): TP / |target == c| in double, 1.0 for an absent class, mean over C
  {
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
      out->pa[c] = row[c] == 0 ? 1.0 : (double)conf[c * C + c] / (double)row[c];
      acc += out->pa[c];
    }
    out->pa_mean = acc / C;
  }
  // frequency-weighted IoU (evaluate.py:29-45): float32 matrix and arithmetic; freq is NOT renormalised when class 0 is left out
  {
    const volatile float tot = (float)total;   // hist.sum(): exact below 2^24 pixels, as every float32 sum here
    volatile float all = 0.f, fg = 0.f;
    for (int c = 0; c < C; ++c) {
      const volatile float r = (float)row[c], cl = (float)col[c], d = (float)conf[c * C + c];
      const volatile float freq = r / tot;
      const volatile float s1 = r + cl;
      const volatile float s2 = s1 - d;
      const volatile float den = s2 + 1e-10f;
      const volatile float iu = d / den;
      const volatile float term = freq * iu;
      all = all + term;
      if (c >= 1) fg = fg + term;
    }
    out->fw_iou = all;
    out->fw_iou_fg = fg;
  }
  return LDIFF_OK;
}
