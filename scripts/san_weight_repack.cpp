// Sanitizer check of the checkpoint loader's host repack functions (ldiffusion_amd/csrc/weight_store.hip: repack_rows, repack_tconv, repack_f32,
// repack_rows3): a stand-alone program that runs each on the smallest shape that exercises its index rule, from F32, F16 and BF16 input, under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Host code only: no HIP call is made and no device is needed.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         ldiffusion_amd/csrc/weight_store.hip scripts/san_weight_repack.cpp -o san_weight_repack && ./san_weight_repack
//
// Prints "san_weight_repack: ok" and exits 0; any sanitizer report, or a wrong element, ends it with a non-zero status.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ldiffusion_amd/csrc/model.h"

// what weight_store.hip takes from the rest of the library
static char g_err[512];
void ldiff_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define REQUIRE(cond)                                                              \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      fprintf(stderr, "san_weight_repack: %s failed (line %d)\n", #cond, __LINE__); \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

// A source tensor of n elements in `dtype`, in an exact-size heap block (a read past it is a heap-buffer-overflow), and the value of each element as a
// float.  The values are no fp16 numbers, so the fp16 rounding and the wl = f16(w - wh) term both matter.
struct Src {
  void* p;
  std::vector<float> val;
  Src(int dtype, size_t n) : val(n) {
    const size_t es = dtype == LDIFF_F32 ? 4 : 2;
    p = malloc(n * es);
    for (size_t i = 0; i < n; ++i) {
      const float f = 0.0137f * (float)(i + 1) * ((i % 3) ? 1.f : -1.f) + 1e-4f * (float)(i % 7);
      if (dtype == LDIFF_F32) { ((float*)p)[i] = f; val[i] = f; }
      else if (dtype == LDIFF_F16) { ((f16*)p)[i] = (f16)f; val[i] = (float)(f16)f; }
      else {
        uint32_t u;
        memcpy(&u, &f, 4);
        ((uint16_t*)p)[i] = (uint16_t)(u >> 16);
        u &= 0xffff0000u;
        memcpy(&val[i], &u, 4);
      }
    }
  }
  ~Src() { free(p); }
};

// n elements of T between two 64-byte guard blocks, filled with a pattern that is neither zero nor an expected value
template <class T> struct Guarded {
  unsigned char* raw;
  size_t n;
  explicit Guarded(size_t n_) : n(n_) {
    raw = (unsigned char*)malloc(128 + n * sizeof(T));
    memset(raw, 0xA5, 128 + n * sizeof(T));
    memset(raw + 64, 0x5A, n * sizeof(T));
  }
  T* data() { return (T*)(raw + 64); }
  void check_guards() {
    for (int i = 0; i < 64; ++i) REQUIRE(raw[i] == 0xA5 && raw[64 + n * sizeof(T) + i] == 0xA5);
  }
  ~Guarded() { free(raw); }
};

static bool same(f16 a, f16 b) { return memcmp(&a, &b, 2) == 0; }
static bool same(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// x rows 16j..16j+15 at 32j.., gate rows 16j.. at 32j+16..
static int naive_geglu_row(int r, int half) {
  const bool gate = r >= half;
  const int q = gate ? r - half : r;
  return 32 * (q / 16) + (gate ? 16 : 0) + q % 16;
}

static void check_dtype(int dtype) {
  {   // conv [3, 2, 3, 3] into Cin_pad = 8
    const int rows = 3, Cin = 2, taps = 9, Cp = 8, K = taps * Cp;
    Src s(dtype, (size_t)rows * Cin * taps);
    Guarded<f16> d((size_t)rows * K);
    repack_rows(s.p, dtype, rows, Cin, taps, Cp, K, 0, d.data());
    d.check_guards();
    for (int r = 0; r < rows; ++r)
      for (int t = 0; t < taps; ++t)
        for (int c = 0; c < Cp; ++c) {
          const f16 want = c < Cin ? (f16)s.val[(size_t)(r * Cin + c) * taps + t] : (f16)0.f;
          REQUIRE(same(d.data()[(size_t)r * K + t * Cp + c], want));
        }
  }
  {   // GEGLU projection of 64 rows (half = 32), Linear(6 -> 64) into Cin_pad = 8, and its bias
    const int rows = 64, half = 32, Cin = 6, Cp = 8, K = Cp;
    Src s(dtype, (size_t)rows * Cin);
    Guarded<f16> d((size_t)rows * K);
    repack_rows(s.p, dtype, rows, Cin, 1, Cp, K, half, d.data());
    d.check_guards();
    std::vector<int> seen(rows, 0);
    for (int r = 0; r < rows; ++r) {
      const int dr = naive_geglu_row(r, half);
      REQUIRE(dr >= 0 && dr < rows && !seen[dr]);
      seen[dr] = 1;
      for (int c = 0; c < Cp; ++c) REQUIRE(same(d.data()[(size_t)dr * K + c], c < Cin ? (f16)s.val[(size_t)r * Cin + c] : (f16)0.f));
    }
    Src b(dtype, rows);
    Guarded<float> db(rows);
    repack_f32(b.p, dtype, rows, half, db.data());
    db.check_guards();
    for (int r = 0; r < rows; ++r) REQUIRE(same(db.data()[naive_geglu_row(r, half)], b.val[r]));
    Guarded<float> dp(rows);   // and a plain fp32 tensor
    repack_f32(b.p, dtype, rows, 0, dp.data());
    dp.check_guards();
    for (int r = 0; r < rows; ++r) REQUIRE(same(dp.data()[r], b.val[r]));
  }
  {   // transposed conv [2, 3, 2, 2] into [tap][Cout][Cin_pad = 8]
    const int Cin = 2, Cout = 3, taps = 4, K = 8;
    Src s(dtype, (size_t)Cin * Cout * taps);
    Guarded<f16> d((size_t)taps * Cout * K);
    repack_tconv(s.p, dtype, Cin, Cout, taps, Cout, K, d.data());
    d.check_guards();
    for (int t = 0; t < taps; ++t)
      for (int n = 0; n < Cout; ++n)
        for (int c = 0; c < K; ++c) REQUIRE(same(d.data()[(size_t)(t * Cout + n) * K + c], c < Cin ? (f16)s.val[(size_t)(c * Cout + n) * taps + t] : (f16)0.f));
  }
  {   // three-block linear [5, 4] at row offset 16 of a 21-row operand: the rows in front stay untouched
    const int rows = 5, K = 4, off = 16;
    Src s(dtype, (size_t)rows * K);
    Guarded<f16> d((size_t)(off + rows) * 3 * K);
    repack_rows3(s.p, dtype, rows, K, d.data() + (size_t)off * 3 * K);
    d.check_guards();
    const unsigned char* bytes = (const unsigned char*)d.data();
    for (size_t i = 0; i < (size_t)off * 3 * K * sizeof(f16); ++i) REQUIRE(bytes[i] == 0x5A);
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < K; ++k) {
        const float w = s.val[(size_t)r * K + k];
        const f16 wh = (f16)w, wl = (f16)(w - (float)wh);
        const f16* row = d.data() + (size_t)(off + r) * 3 * K;
        REQUIRE(same(row[k], wh) && same(row[K + k], wh) && same(row[2 * K + k], wl));
      }
  }
}

int main() {
  for (int dtype : {LDIFF_F32, LDIFF_F16, LDIFF_BF16}) check_dtype(dtype);
  printf("san_weight_repack: ok\n");
  return 0;
}
