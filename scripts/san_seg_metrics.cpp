// Sanitizer check of the host routine ldiff_seg_metrics (kernels_metrics.hip seg_metrics_host): a stand-alone program that feeds it the edge matrices
// and both ends of the class range under AddressSanitizer + UndefinedBehaviorSanitizer.  Host code only: no kernel is launched and no device is needed.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         ldiffusion_amd/csrc/kernels_metrics.hip scripts/san_seg_metrics.cpp -o san_seg_metrics && ./san_seg_metrics
//
// Prints "san_seg_metrics: ok" and exits 0; any sanitizer report, or a wrong figure, ends it with a non-zero status.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ldiffusion_amd/csrc/common.h"

// what kernels_metrics.hip takes from the rest of the library
static char g_err[512];
void ldiff_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
bool prof_on(const char*) { return false; }
void prof_begin(const char*, double, double, hipStream_t) {}
void prof_end(hipStream_t) {}

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "san_seg_metrics: %s failed (line %d)\n", #cond, __LINE__); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

// the output record between two guard blocks that must come back untouched
struct Guarded {
  unsigned char before[64];
  ldiff_seg_metrics_out out;
  unsigned char after[64];
};

static void run(const std::vector<int64_t>& conf, int C, ldiff_seg_metrics_out* out, int want_rc) {
  // an exact-size heap copy: a read past C * C entries is a heap-buffer-overflow
  int64_t* m = (int64_t*)malloc(conf.size() * sizeof(int64_t) + (conf.empty() ? 1 : 0));
  if (!conf.empty()) memcpy(m, conf.data(), conf.size() * sizeof(int64_t));
  Guarded* g = (Guarded*)malloc(sizeof(Guarded));
  memset(g, 0xA5, sizeof(Guarded));
  REQUIRE(seg_metrics_host(m, C, &g->out) == want_rc);
  for (int i = 0; i < 64; ++i) REQUIRE(g->before[i] == 0xA5 && g->after[i] == 0xA5);
  *out = g->out;
  free(g);
  free(m);
}

int main() {
  ldiff_seg_metrics_out o;
  // C = 1
  run({9}, 1, &o, LDIFF_OK);
  REQUIRE(o.num_classes == 1 && o.dice[0] == 1.f && o.dice_mean == 1.f && o.iou[0] == 1.0 && o.iou_mean == 1.0 && o.pa_mean == 1.0 && o.fw_iou == 1.f && o.fw_iou_fg == 0.f);
  run({0}, 1, &o, LDIFF_OK);
  REQUIRE(o.dice[0] == 1.f && o.iou_skipped[0] == 1 && isnan(o.iou[0]) && o.iou_mean == 1.0 && o.pa[0] == 1.0 && isnan(o.fw_iou) && o.fw_iou_fg == 0.f);
  // the hand-made 3 x 3 matrix: ignore_background, an absent class
  run({5, 1, 0, 3, 2, 0, 0, 0, 0}, 3, &o, LDIFF_OK);
  REQUIRE(fabsf(o.dice[0] - 10.f / 14.f) < 1e-7f && o.dice[1] == 0.5f && o.dice[2] == 1.f);
  REQUIRE(o.iou_skipped[0] == 0 && o.iou_skipped[1] == 0 && o.iou_skipped[2] == 1 && isnan(o.iou[2]) && fabs(o.iou_mean - (5.0 / 9 + 2.0 / 6) / 2) < 1e-12);
  REQUIRE(fabs(o.pa_mean - (5.0 / 6 + 2.0 / 5 + 1) / 3) < 1e-12);
  REQUIRE(fabsf(o.fw_iou_fg - (5.f / 11) * (2.f / 6)) < 1e-7f && fabsf(o.fw_iou - ((6.f / 11) * (5.f / 9) + (5.f / 11) * (2.f / 6))) < 1e-7f);
  // the empty matrix
  run(std::vector<int64_t>(16, 0), 4, &o, LDIFF_OK);
  REQUIRE(o.dice_mean == 1.f && o.iou_mean == 1.0 && o.pa_mean == 1.0 && isnan(o.fw_iou) && isnan(o.fw_iou_fg));
  // C = 32: every entry of the per-class arrays, and counts beyond 2^24 and 2^32 (the float32 conversions and the int64 sums)
  {
    std::vector<int64_t> big(32 * 32);
    for (int i = 0; i < 32 * 32; ++i) big[i] = (int64_t)i * 3000000007ll + (i % 33 == 0 ? (1ll << 40) : 0);
    run(big, 32, &o, LDIFF_OK);
    REQUIRE(o.num_classes == 32);
    for (int c = 0; c < 32; ++c) REQUIRE(o.dice[c] > 0.f && o.dice[c] <= 1.f && o.iou[c] > 0.0 && o.iou[c] <= 1.0 && o.pa[c] > 0.0 && o.pa[c] <= 1.0 && !o.iou_skipped[c]);
    REQUIRE(o.fw_iou > 0.f && o.fw_iou <= 1.f && o.fw_iou_fg <= o.fw_iou);
    std::vector<int64_t> huge(32 * 32, INT64_MAX / (32 * 32));   // the total stays below 2^63
    run(huge, 32, &o, LDIFF_OK);
    REQUIRE(fabs(o.iou_mean - 1.0 / 63) < 1e-12);
  }
  // refusals: nothing is read or written
  run({}, 0, &o, LDIFF_ERR_INVALID);
  run({}, 33, &o, LDIFF_ERR_INVALID);
  run({1, -1, 0, 1}, 2, &o, LDIFF_ERR_INVALID);
  REQUIRE(seg_metrics_host(nullptr, 3, &o) == LDIFF_ERR_INVALID && strstr(g_err, "null"));
  {
    int64_t one = 1;
    REQUIRE(seg_metrics_host(&one, 1, nullptr) == LDIFF_ERR_INVALID);
  }
  printf("san_seg_metrics: ok\n");
  return 0;
}
