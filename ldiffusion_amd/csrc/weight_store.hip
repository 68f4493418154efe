// WeightStore: the checkpoint loader of every handle family (contract: model.h).  Two layers: host repack functions that turn a torch tensor into the
// device layout without a HIP call (scripts/san_weight_repack.cpp runs them under the sanitizers), and WeightStore::load, which looks the name up, checks
// dtype and shape, repacks and copies.
#include <string.h>

#include <algorithm>

#include "model.h"

// ---- host repack ---------------------------------------------------------------------------------
static float host_to_float(const void* p, int dtype, size_t i) {   // element i of a host tensor of dtype LDIFF_F32 / F16 / BF16
  if (dtype == LDIFF_F32) return ((const float*)p)[i];
  if (dtype == LDIFF_F16) return (float)((const f16*)p)[i];
  uint32_t u = (uint32_t)((const uint16_t*)p)[i] << 16;  // bf16
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static inline int geglu_row(int r, int half) { const int q = r < half ? r : r - half; return (q / 16) * 32 + (r < half ? 0 : 16) + q % 16; }

void repack_rows(const void* src, int dtype, int rows, int Cin, int taps, int Cin_pad, int K, int geglu_half, f16* dst) {
  std::fill(dst, dst + (size_t)rows * K, (f16)0.f);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < Cin; ++c)
      for (int t = 0; t < taps; ++t)
        dst[(size_t)(geglu_half ? geglu_row(r, geglu_half) : r) * K + (size_t)t * Cin_pad + c] = (f16)host_to_float(src, dtype, ((size_t)r * Cin + c) * taps + t);
}
void repack_tconv(const void* src, int dtype, int Cin, int Cout, int taps, int rows_t, int K, f16* dst) {
  std::fill(dst, dst + (size_t)taps * rows_t * K, (f16)0.f);
  for (int c = 0; c < Cin; ++c)
    for (int n = 0; n < Cout; ++n)
      for (int t = 0; t < taps; ++t) dst[((size_t)t * rows_t + n) * K + c] = (f16)host_to_float(src, dtype, ((size_t)c * Cout + n) * taps + t);
}
void repack_f32(const void* src, int dtype, size_t n, int geglu_half, float* dst) {
  for (size_t i = 0; i < n; ++i) dst[geglu_half ? (size_t)geglu_row((int)i, geglu_half) : i] = host_to_float(src, dtype, i);
}
void repack_rows3(const void* src, int dtype, int rows, int K, f16* dst) {
  for (int r = 0; r < rows; ++r)
    for (int k = 0; k < K; ++k) {
      const float w = host_to_float(src, dtype, (size_t)r * K + k);
      const f16 wh = (f16)w;
      f16* d = dst + (size_t)r * 3 * K + k;
      d[0] = wh; d[K] = wh; d[2 * K] = (f16)(w - (float)wh);
    }
}

// ---- allocation and registration -------------------------------------------------------------------
WeightStore::~WeightStore() {
  for (void* p : allocs_) (void)hipFree(p);
}
void* WeightStore::alloc_zeroed(size_t bytes) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes));
  allocs_.push_back(p);
  HIP_CHECK(hipMemset(p, 0, bytes));
  return p;
}
f16* WeightStore::alloc_mat(int Nrows, int K) { return (f16*)alloc_zeroed((size_t)Nrows * K * sizeof(f16)); }
float* WeightStore::alloc_vec(size_t n) { return (float*)alloc_zeroed(n * sizeof(float)); }

LoadSpec& WeightStore::add(const std::string& name, LoadSpec::Kind kind, std::vector<int64_t> shape) {
  LoadSpec& sp = specs_[name];
  sp = LoadSpec();
  sp.kind = kind;
  sp.shape = std::move(shape);
  order_.push_back(name);
  return sp;
}
void WeightStore::add_tensor(const std::string& name, std::vector<int64_t> shape, float* dst, int off) {
  LoadSpec& sp = add(name, LoadSpec::TENSOR, std::move(shape));
  sp.vec = dst; sp.vec_off = off;
}
void WeightStore::add_host(const std::string& name, std::vector<int64_t> shape) { add(name, LoadSpec::HOST, std::move(shape)); }
void WeightStore::add_rows(const std::string& wname, const std::string& bname, f16* mat, int K, int ks, int Cin, int Cin_pad, int row_off,
                           int rows, float* bias_vec, bool has_bias) {
  LoadSpec& w = add(wname, LoadSpec::MATRIX, {rows, Cin, ks, ks});
  w.mat = mat; w.row_off = row_off; w.K = K; w.ks = ks; w.Cin_pad = Cin_pad;
  if (has_bias) add_tensor(bname, {rows}, bias_vec, row_off);
}
void WeightStore::add_rows3(const std::string& wname, const std::string& bname, f16* mat, int K, int row_off, int rows, float* bias_vec) {
  add_rows(wname, bname, mat, K, 1, K, K, row_off, rows, bias_vec, true);
  specs_[wname].rows3 = true;
}
MatW WeightStore::add_conv(const std::string& prefix, int Cin, int Cout, int ks, bool bias, int Cin_pad, int min_rows, bool geglu) {
  if (Cin_pad < 0) Cin_pad = roundup(Cin, 8);
  MatW m;
  m.N = Cout; m.Nrows = roundup(std::max(Cout, min_rows), 16); m.ks = ks; m.Cin = Cin_pad; m.K = ks * ks * Cin_pad;
  m.Cin_logical = 2 * Cin <= Cin_pad ? Cin : 0;   // hi | lo of a <= 4-channel input fit into the 8 padded channels
  m.w = alloc_mat(m.Nrows, m.K);
  m.b = bias ? alloc_vec(m.Nrows) : nullptr;
  add_rows(prefix + ".weight", prefix + ".bias", m.w, m.K, ks, Cin, Cin_pad, 0, Cout, m.b, bias);
  if (geglu) {   // Linear(C, 2*half) whose output is [x | gate]: store x rows 16j..16j+15 at 32j.., gate rows 16j.. at 32j+16..
    LDIFF_CHECK(Cout % 32 == 0, LDIFF_ERR_INVALID, "geglu projection width %d must be a multiple of 32", Cout);
    m.geglu = true;
    specs_[prefix + ".weight"].geglu_half = Cout / 2;
    if (bias) specs_[prefix + ".bias"].geglu_half = Cout / 2;
  }
  return m;
}
NormW WeightStore::add_norm(const std::string& prefix, int C) {
  NormW n;
  n.C = C; n.g = alloc_vec(C); n.b = alloc_vec(C);
  add_tensor(prefix + ".weight", {C}, n.g);
  add_tensor(prefix + ".bias", {C}, n.b);
  return n;
}
MatW WeightStore::add_tconv(const std::string& prefix, int Cin, int Cout, int k) {
  MatW m;
  m.N = Cout; m.Nrows = Cout; m.ks = k; m.Cin = roundup(Cin, 8); m.K = m.Cin;
  m.w = alloc_mat(k * k * m.Nrows, m.K);
  m.b = alloc_vec(m.Nrows);
  LoadSpec& w = add(prefix + ".weight", LoadSpec::MATRIX, {Cin, Cout, k, k});
  w.mat = m.w; w.K = m.K; w.ks = k; w.Cin_pad = m.Cin; w.tconv = true; w.tconv_rows = m.Nrows;
  add_tensor(prefix + ".bias", {Cout}, m.b);
  return m;
}
void WeightStore::alias(const std::string& alias_name, const std::string& name) { alias_[alias_name] = name; }

// ---- loading ---------------------------------------------------------------------------------------
void WeightStore::check_tensor(const char* name_c, const void* host, int dtype, const int64_t* shape, int ndim) const {
  LDIFF_CHECK(name_c && host && (shape || ndim == 0), LDIFF_ERR_INVALID, "%s: null argument", who);
  LDIFF_CHECK(dtype == LDIFF_F32 || dtype == LDIFF_F16 || dtype == LDIFF_BF16, LDIFF_ERR_INVALID, "%s(%s): unsupported dtype %d", who, name_c, dtype);
}
[[noreturn]] static void throw_shape_mismatch(const char* who, const char* name, const int64_t* shape, int ndim, const std::vector<int64_t>& want) {
  std::string got, exp;
  for (int i = 0; i < ndim; ++i) got += (i ? "," : "") + std::to_string((long long)shape[i]);
  for (size_t i = 0; i < want.size(); ++i) exp += (i ? "," : "") + std::to_string((long long)want[i]);
  ldiff_set_error("%s(%s): shape [%s] does not match expected [%s]", who, name, got.c_str(), exp.c_str());
  throw LdiffError{LDIFF_ERR_INVALID};
}

void WeightStore::load(const char* name_c, const void* host, int dtype, const int64_t* shape, int ndim) {
  check_tensor(name_c, host, dtype, shape, ndim);
  std::string name(name_c);
  auto al = alias_.find(name);
  if (al != alias_.end()) name = al->second;
  auto it = specs_.find(name);
  LDIFF_CHECK(it != specs_.end(), LDIFF_ERR_INVALID, "%s: unexpected tensor name '%s'", who, name_c);
  LoadSpec& sp = it->second;
  size_t numel = 1;
  for (auto d : sp.shape) numel *= (size_t)d;
  bool ok;
  if (sp.kind == LoadSpec::MATRIX) {   // element count and the first two extents; rank 4, or rank 2 for a 1x1
    size_t got = 1;
    for (int i = 0; i < ndim; ++i) got *= (size_t)shape[i];
    ok = got == numel && ndim >= 2 && shape[0] == sp.shape[0] && shape[1] == sp.shape[1] && (ndim == 4 || (ndim == 2 && sp.ks == 1));
  } else {                             // exact
    ok = ndim == (int)sp.shape.size();
    for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == sp.shape[i];
  }
  if (!ok) throw_shape_mismatch(who, name_c, shape, ndim, sp.shape);
  // the wait rule: an earlier forward may still read a tensor that was loaded before; nothing can have read one that was not
  auto to_device = [&](void* dst, const void* src, size_t bytes) {
    if (sp.loaded) HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  };
  if (sp.kind == LoadSpec::HOST) {
    sp.host.resize(numel);
    repack_f32(host, dtype, numel, 0, sp.host.data());
    if (!sp.fresh) ++n_fresh_;
    sp.fresh = true;
  } else if (sp.kind == LoadSpec::TENSOR) {
    std::vector<float> tmp(numel);
    repack_f32(host, dtype, numel, sp.geglu_half, tmp.data());
    to_device(sp.vec + sp.vec_off, tmp.data(), numel * sizeof(float));
  } else if (sp.tconv) {
    const int taps = sp.ks * sp.ks;
    std::vector<f16> tmp((size_t)taps * sp.tconv_rows * sp.K);
    repack_tconv(host, dtype, (int)sp.shape[0], (int)sp.shape[1], taps, sp.tconv_rows, sp.K, tmp.data());
    to_device(sp.mat, tmp.data(), tmp.size() * sizeof(f16));
  } else if (sp.rows3) {
    const int rows = (int)sp.shape[0];
    std::vector<f16> tmp((size_t)rows * 3 * sp.K);
    repack_rows3(host, dtype, rows, sp.K, tmp.data());
    to_device(sp.mat + (size_t)sp.row_off * 3 * sp.K, tmp.data(), tmp.size() * sizeof(f16));
  } else {
    const int rows = (int)sp.shape[0];
    std::vector<f16> tmp((size_t)rows * sp.K);
    repack_rows(host, dtype, rows, (int)sp.shape[1], sp.ks * sp.ks, sp.Cin_pad, sp.K, sp.geglu_half, tmp.data());
    to_device(sp.mat + (size_t)sp.row_off * sp.K, tmp.data(), tmp.size() * sizeof(f16));
  }
  sp.loaded = true;
  ++generation;
}
int WeightStore::missing() const {
  missing_cache_.clear();
  for (auto& n : order_)
    if (!specs_.at(n).loaded) missing_cache_.push_back(n);
  return (int)missing_cache_.size();
}
const char* WeightStore::missing_name(int i) const {
  if (i < 0 || i >= (int)missing_cache_.size()) return "";
  return missing_cache_[i].c_str();
}

// ---- host-staged tensors ---------------------------------------------------------------------------
bool WeightStore::loaded(const std::string& name) const { return specs_.at(name).loaded; }
const std::vector<float>* WeightStore::fresh(const std::string& name) const {
  const LoadSpec& sp = specs_.at(name);
  return sp.fresh ? &sp.host : nullptr;
}
void WeightStore::consume(const std::string& name) {
  LoadSpec& sp = specs_.at(name);
  if (!sp.fresh) return;
  sp.fresh = false;
  std::vector<float>().swap(sp.host);
  --n_fresh_;
}
