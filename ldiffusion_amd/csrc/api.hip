// extern "C" boundary of libldiff_hip.so (see include/ldiff.h for the contract of every entry point).
#include <string.h>

#include <cmath>
#include <exception>
#include <map>
#include <mutex>

#include "model.h"

const char* ldiff_error_message();

// non-finite detector, reporting rule (b) of include/ldiff.h: an entry point that finds the flag of EARLIER, completed work set reports it once
// the VAE's handles add the cure for the decoder (include/ldiff.h "Non-finite detection")
#define VAE_RANGE_HINT " For the VAE decoder: ldiff_vae_set_range_shift (python: AutoencoderKL.set_range_shift / fit_range_shift) stores its activations times 2^-k."
static void report_nonfinite(NonFiniteFlag& nf, const char* what, const char* hint = "") {
  LDIFF_CHECK(!nf.test_and_clear(), LDIFF_ERR_NONFINITE,
              "%s: a non-finite activation (fp16 overflow: |x| > 65504, or NaN) was detected in work enqueued earlier on this handle; its results are invalid. "
              "Activations are stored as fp16 in every precision mode (set_precision 1 / 2 add mantissa bits, not range): rescale the input / checkpoint, "
              "and use LDIFF_TRACE_ABSMAX=1 to see which stage overflows.%s", what, hint);
}

#define API_BEGIN try {
#define API_END                                                  \
  }                                                              \
  catch (const LdiffError& e) { return e.code; }                 \
  catch (const std::exception& e) {                              \
    ldiff_set_error("internal error: %s", e.what());             \
    return LDIFF_ERR_RUNTIME;                                    \
  }                                                              \
  return LDIFF_OK;

// ---- what the handle families (unet, controlnet, vae, segnet, resnet, textenc) share ----
template <class H> static int device_of(const H* h) { return h->device; }
static int device_of(const ldiff_controlnet* c) { return c->trunk.device; }
template <class H> static NonFiniteFlag& flag_of(H* h) { return h->nf; }
static NonFiniteFlag& flag_of(ldiff_controlnet* c) { return c->trunk.nf; }
template <class H> static WeightStore& store_of(H* h) { return h->ws; }
static WeightStore& store_of(ldiff_controlnet* c) { return c->trunk.ws; }
// *_load (the contract: model.h, WeightStore): the classifier and the text encoder have a step of their own in front of the store's
template <class H> static void load_into(H* h, const char* name, const void* host, int dtype, const int64_t* shape, int ndim) { store_of(h).load(name, host, dtype, shape, ndim); }
static void load_into(ldiff_resnet* r, const char* name, const void* host, int dtype, const int64_t* shape, int ndim) { r->load(name, host, dtype, shape, ndim); }
static void load_into(ldiff_textenc* t, const char* name, const void* host, int dtype, const int64_t* shape, int ndim) { t->load(name, host, dtype, shape, ndim); }
template <class H> static int load(H* h, const char* who, const char* name, const void* host, int dtype, const int64_t* shape, int ndim) {
  API_BEGIN
  LDIFF_CHECK(h, LDIFF_ERR_INVALID, "%s: null handle", who);
  HIP_CHECK(hipSetDevice(device_of(h)));
  load_into(h, name, host, dtype, shape, ndim);
  API_END
}
template <class H> static int missing(H* h) { return h ? store_of(h).missing() : -1; }
template <class H> static const char* missing_name(H* h, int i) { return h ? store_of(h).missing_name(i) : ""; }

static void select_device(const char* who, int device) {   // of a *_create
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  LDIFF_CHECK(device >= 0 && device < ndev, LDIFF_ERR_INVALID, "%s: device %d not available (%d devices)", who, device, ndev);
  HIP_CHECK(hipSetDevice(device));
}
// *_check_finite: `synced` runs between the synchronisation and the report (the VAE's side stream, the UNet's attached ControlNet)
template <class H, class F> static int check_finite(H* h, void* stream, const char* who, const char* hint, F synced) {
  API_BEGIN
  LDIFF_CHECK(h, LDIFF_ERR_INVALID, "%s: null handle", who);
  HIP_CHECK(hipSetDevice(device_of(h)));
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  synced();
  report_nonfinite(flag_of(h), who, hint);
  API_END
}
template <class H> static int check_finite(H* h, void* stream, const char* who) { return check_finite(h, stream, who, "", [] {}); }
// *_destroy: `release` frees what the handle's destructor does not
template <class H, class F> static void destroy(H* h, F release) {
  if (!h) return;
  (void)hipSetDevice(device_of(h));
  (void)hipDeviceSynchronize();
  release();
  delete h;
}
template <class H> static void destroy(H* h) { destroy(h, [] {}); }
template <class H> static int set_graph(H* h, int on, const char* who) {
  API_BEGIN
  LDIFF_CHECK(h, LDIFF_ERR_INVALID, "%s: null handle", who);
  HIP_CHECK(hipSetDevice(h->device));
  h->gc.set_enabled(on != 0);   // (off: waits for the device before the graph goes)
  API_END
}

extern "C" {

int ldiff_version(void) { return LDIFF_VERSION; }
const char* ldiff_last_error(void) { return ldiff_error_message(); }

// ---- UNet ----
int ldiff_unet_create(ldiff_unet** out, const ldiff_unet_cfg* cfg, int device) {
  API_BEGIN
  LDIFF_CHECK(out && cfg, LDIFF_ERR_INVALID, "unet_create: null argument");
  select_device("unet_create", device);
  ldiff_unet* u = new ldiff_unet();
  u->cfg = *cfg;
  u->device = device;
  try { u->build(); } catch (...) { delete u; throw; }
  *out = u;
  API_END
}
int ldiff_unet_load(ldiff_unet* u, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) { return load(u, "unet_load", name, host_ptr, dtype, shape, ndim); }
int ldiff_unet_set_precision(ldiff_unet* u, int mode) {
  API_BEGIN
  LDIFF_CHECK(u && mode >= PREC_FAST && mode <= PREC_FULL, LDIFF_ERR_INVALID, "unet_set_precision: mode must be 0, 1 or 2");
  u->precision = mode;
  API_END
}
int ldiff_unet_set_plan_batch(ldiff_unet* u, int n) {
  API_BEGIN
  LDIFF_CHECK(u, LDIFF_ERR_INVALID, "unet_set_plan_batch: null handle");
  LDIFF_CHECK(n >= 0, LDIFF_ERR_INVALID, "unet_set_plan_batch: n = %d must be >= 0 (0 = off)", n);
  u->set_plan_batch(n);
  API_END
}
int ldiff_unet_set_graph(ldiff_unet* u, int on) { return set_graph(u, on, "unet_set_graph"); }
int64_t ldiff_unet_graph_replays(ldiff_unet* u) { return u ? (int64_t)u->gc.replays : -1; }
int64_t ldiff_unet_graph_nodes(ldiff_unet* u) { return u ? (int64_t)u->gc.nodes : -1; }
int ldiff_unet_missing(ldiff_unet* u) { return missing(u); }
const char* ldiff_unet_missing_name(ldiff_unet* u, int i) { return missing_name(u, i); }
int ldiff_unet_set_context(ldiff_unet* u, const void* ctx_dev, int B_ctx, int L, void* stream) {
  API_BEGIN
  LDIFF_CHECK(u, LDIFF_ERR_INVALID, "unet_set_context: null handle");
  u->set_context((const float*)ctx_dev, B_ctx, L, (hipStream_t)stream);
  API_END
}
int ldiff_unet_forward(ldiff_unet* u, const void* sample_dev, int B, int h, int w, float timestep, void* out_dev, void* stream) {
  API_BEGIN
  LDIFF_CHECK(u, LDIFF_ERR_INVALID, "unet_forward: null handle");
  report_nonfinite(u->nf, "unet_forward");
  u->forward((const float*)sample_dev, B, h, w, timestep, (float*)out_dev, (hipStream_t)stream);
  API_END
}
int ldiff_unet_set_additional_residuals(ldiff_unet* u, const void* const* down_dev, int n_down, const void* mid_dev) {
  API_BEGIN
  LDIFF_CHECK(u, LDIFF_ERR_INVALID, "set_additional_residuals: null handle");
  LDIFF_CHECK(n_down == 0 || (down_dev && n_down == u->n_skips()), LDIFF_ERR_INVALID,
              "set_additional_residuals: %d down-block residuals given, this UNet has %d skip tensors", n_down, u->n_skips());
  u->extra_down.clear();
  for (int i = 0; i < n_down; ++i) {
    LDIFF_CHECK(down_dev[i], LDIFF_ERR_INVALID, "set_additional_residuals: residual %d is null", i);
    u->extra_down.push_back((const float*)down_dev[i]);
  }
  u->extra_mid = (const float*)mid_dev;
  API_END
}
int ldiff_unet_check_finite(ldiff_unet* u, void* stream) {
  return check_finite(u, stream, "unet_check_finite", "", [u] {
    const bool cn_bad = u->cn && u->cn->trunk.nf.test_and_clear();   // an attached ControlNet's blocks ran inside this handle's forwards
    if (cn_bad) (void)u->nf.test_and_clear();                        // (the UNet's own blocks inherit the overflow through the skips: one report for both)
    LDIFF_CHECK(!cn_bad, LDIFF_ERR_NONFINITE, "unet_check_finite: a non-finite activation (fp16 overflow: |x| > 65504, or NaN) was detected in the attached ControlNet; "
                "the results of that forward are invalid.  LDIFF_TRACE_ABSMAX=1 shows which stage overflows.");
  });
}
void ldiff_unet_destroy(ldiff_unet* u) {
  destroy(u, [u] { if (u->ctx_buf) (void)hipFree(u->ctx_buf); });
}

// ---- ControlNet ----
int ldiff_controlnet_create(ldiff_controlnet** out, const ldiff_unet_cfg* trunk_cfg, int conditioning_channels, const int* embedding_channels, int n_embedding, int device) {
  API_BEGIN
  LDIFF_CHECK(out && trunk_cfg && embedding_channels && n_embedding >= 1 && n_embedding <= LDIFF_MAX_BLOCKS, LDIFF_ERR_INVALID, "controlnet_create: bad arguments");
  select_device("controlnet_create", device);
  ldiff_controlnet* c = new ldiff_controlnet();
  c->trunk.cfg = *trunk_cfg;
  c->trunk.device = device;
  c->cond_channels = conditioning_channels;
  c->emb_ch.assign(embedding_channels, embedding_channels + n_embedding);
  try { c->build(); } catch (...) { delete c; throw; }
  *out = c;
  API_END
}
int ldiff_controlnet_load(ldiff_controlnet* c, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) { return load(c, "controlnet_load", name, host_ptr, dtype, shape, ndim); }
int ldiff_controlnet_missing(ldiff_controlnet* c) { return missing(c); }
const char* ldiff_controlnet_missing_name(ldiff_controlnet* c, int i) { return missing_name(c, i); }
int ldiff_controlnet_set_precision(ldiff_controlnet* c, int mode) {
  API_BEGIN
  LDIFF_CHECK(c && mode >= PREC_FAST && mode <= PREC_FULL, LDIFF_ERR_INVALID, "controlnet_set_precision: mode must be 0, 1 or 2");
  c->trunk.precision = mode;
  API_END
}
int ldiff_controlnet_set_plan_batch(ldiff_controlnet* c, int n) {
  API_BEGIN
  LDIFF_CHECK(c, LDIFF_ERR_INVALID, "controlnet_set_plan_batch: null handle");
  LDIFF_CHECK(n >= 0, LDIFF_ERR_INVALID, "controlnet_set_plan_batch: n = %d must be >= 0 (0 = off)", n);
  c->set_plan_batch(n);
  API_END
}
int ldiff_controlnet_set_context(ldiff_controlnet* c, const void* ctx_dev, int B_ctx, int L, void* stream) {
  API_BEGIN
  LDIFF_CHECK(c, LDIFF_ERR_INVALID, "controlnet_set_context: null handle");
  c->trunk.set_context((const float*)ctx_dev, B_ctx, L, (hipStream_t)stream);
  API_END
}
int ldiff_controlnet_set_cond(ldiff_controlnet* c, const void* cond_dev, int B, int H, int W, void* stream) {
  API_BEGIN
  LDIFF_CHECK(c, LDIFF_ERR_INVALID, "controlnet_set_cond: null handle");
  c->set_cond((const float*)cond_dev, B, H, W, (hipStream_t)stream);
  API_END
}
int ldiff_controlnet_forward(ldiff_controlnet* c, const void* sample_dev, int B, int h, int w, float timestep, float conditioning_scale, void* const* down_out, int n_down,
                             void* mid_out, void* stream) {
  API_BEGIN
  LDIFF_CHECK(c, LDIFF_ERR_INVALID, "controlnet_forward: null handle");
  report_nonfinite(c->trunk.nf, "controlnet_forward");
  c->forward((const float*)sample_dev, B, h, w, timestep, conditioning_scale, reinterpret_cast<float* const*>(down_out), n_down, (float*)mid_out, (hipStream_t)stream);
  API_END
}
int ldiff_controlnet_check_finite(ldiff_controlnet* c, void* stream) { return check_finite(c, stream, "controlnet_check_finite"); }
void ldiff_controlnet_destroy(ldiff_controlnet* c) { destroy(c); }
// ---- nnU-Net tissue head ----
int ldiff_segnet_create(ldiff_segnet** out, int in_channels, int n_stages, const int* features, const int* strides, const int* n_conv_encoder, const int* n_conv_decoder,
                        int n_heads, int device) {
  API_BEGIN
  LDIFF_CHECK(out && features && strides && n_conv_encoder && n_conv_decoder && n_stages >= 2 && n_stages <= 16, LDIFF_ERR_INVALID, "segnet_create: null argument or n_stages outside 2..16");
  select_device("segnet_create", device);
  ldiff_segnet* n = new ldiff_segnet();
  n->device = device;
  n->in_ch = in_channels; n->n_stages = n_stages; n->n_heads = n_heads;
  n->features.assign(features, features + n_stages);
  n->strides.assign(strides, strides + n_stages);
  n->nce.assign(n_conv_encoder, n_conv_encoder + n_stages);
  n->ncd.assign(n_conv_decoder, n_conv_decoder + n_stages - 1);
  try { n->build(); } catch (...) { delete n; throw; }
  *out = n;
  API_END
}
int ldiff_segnet_load(ldiff_segnet* n, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) { return load(n, "segnet_load", name, host_ptr, dtype, shape, ndim); }
int ldiff_segnet_missing(ldiff_segnet* n) { return missing(n); }
const char* ldiff_segnet_missing_name(ldiff_segnet* n, int i) { return missing_name(n, i); }
int ldiff_segnet_set_graph(ldiff_segnet* n, int on) { return set_graph(n, on, "segnet_set_graph"); }
int64_t ldiff_segnet_graph_replays(ldiff_segnet* n) { return n ? n->gc.replays : -1; }
int ldiff_segnet_forward(ldiff_segnet* n, const void* x_dev, int B, int H, int W, void* logits_dev, int out_dtype, void* stream) {
  API_BEGIN
  LDIFF_CHECK(n, LDIFF_ERR_INVALID, "segnet_forward: null handle");
  report_nonfinite(n->nf, "segnet_forward");
  n->forward((const float*)x_dev, B, H, W, logits_dev, out_dtype, (hipStream_t)stream);
  API_END
}
int ldiff_segnet_check_finite(ldiff_segnet* n, void* stream) { return check_finite(n, stream, "segnet_check_finite"); }
void ldiff_segnet_destroy(ldiff_segnet* n) { destroy(n); }
// ---- instance classifier of the cell head ----
int ldiff_resnet_create(ldiff_resnet** out, const int* layers, int width, int adapter_channels, int num_classes, int device) {
  API_BEGIN
  LDIFF_CHECK(out && layers, LDIFF_ERR_INVALID, "resnet_create: null argument");
  select_device("resnet_create", device);
  ldiff_resnet* r = new ldiff_resnet();
  r->device = device;
  for (int i = 0; i < 4; ++i) r->layers[i] = layers[i];
  r->width = width; r->adapter_ch = adapter_channels; r->n_classes = num_classes;
  try { r->build(); } catch (...) { delete r; throw; }
  *out = r;
  API_END
}
int ldiff_resnet_load(ldiff_resnet* r, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) { return load(r, "resnet_load", name, host_ptr, dtype, shape, ndim); }
int ldiff_resnet_missing(ldiff_resnet* r) { return missing(r); }
const char* ldiff_resnet_missing_name(ldiff_resnet* r, int i) { return missing_name(r, i); }
int ldiff_resnet_set_graph(ldiff_resnet* r, int on) { return set_graph(r, on, "resnet_set_graph"); }
int64_t ldiff_resnet_graph_replays(ldiff_resnet* r) { return r ? r->gc.replays : -1; }
int ldiff_resnet_forward(ldiff_resnet* r, const void* crops, int B, int S, void* logits, void* labels, void* stream) {
  API_BEGIN
  LDIFF_CHECK(r, LDIFF_ERR_INVALID, "resnet_forward: null handle");
  report_nonfinite(r->nf, "resnet_forward");
  r->forward((const f16*)crops, B, S, (float*)logits, (int*)labels, (hipStream_t)stream);
  API_END
}
int ldiff_resnet_set_train(ldiff_resnet* r, int on) {
  API_BEGIN
  LDIFF_CHECK(r, LDIFF_ERR_INVALID, "resnet_set_train: null handle");
  r->set_train(on != 0);
  API_END
}
int64_t ldiff_resnet_bn_channels(ldiff_resnet* r) { return r ? r->bn_total : -1; }
int ldiff_resnet_bn_entry(ldiff_resnet* r, int i, const char** name, int64_t* offset, int* channels) {
  API_BEGIN
  LDIFF_CHECK(r && name && offset && channels, LDIFF_ERR_INVALID, "resnet_bn_entry: null argument");
  LDIFF_CHECK(i >= 0 && i < (int)r->bn_order.size(), LDIFF_ERR_INVALID, "resnet_bn_entry: index %d outside the %d BatchNorms of this network", i, (int)r->bn_order.size());
  const ClsConvW& c = r->convs[r->bn_order[i]];
  *name = c.bn.c_str(); *offset = c.bn_off; *channels = c.Cout;
  API_END
}
int ldiff_resnet_forward_train(ldiff_resnet* r, const void* crops, int B, int S, void* batch_stats, void* features, void* logits, void* labels, void* stream) {
  API_BEGIN
  LDIFF_CHECK(r, LDIFF_ERR_INVALID, "resnet_forward_train: null handle");
  report_nonfinite(r->nf, "resnet_forward_train");
  r->forward_train((const f16*)crops, B, S, (float*)batch_stats, (float*)features, (float*)logits, (int*)labels, (hipStream_t)stream);
  API_END
}
int ldiff_resnet_check_finite(ldiff_resnet* r, void* stream) { return check_finite(r, stream, "resnet_check_finite"); }
void ldiff_resnet_destroy(ldiff_resnet* r) { destroy(r); }
// ---- CLIP text encoder of the prompt path ----
int ldiff_textenc_create(ldiff_textenc** out, const ldiff_textenc_cfg* cfg, int device) {
  API_BEGIN
  LDIFF_CHECK(out && cfg, LDIFF_ERR_INVALID, "textenc_create: null argument");
  select_device("textenc_create", device);
  ldiff_textenc* t = new ldiff_textenc();
  t->cfg = *cfg;
  t->device = device;
  try { t->build(); } catch (...) { delete t; throw; }
  *out = t;
  API_END
}
int ldiff_textenc_load(ldiff_textenc* t, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) { return load(t, "textenc_load", name, host_ptr, dtype, shape, ndim); }
int ldiff_textenc_missing(ldiff_textenc* t) { return missing(t); }
const char* ldiff_textenc_missing_name(ldiff_textenc* t, int i) { return missing_name(t, i); }
int ldiff_textenc_set_graph(ldiff_textenc* t, int on) { return set_graph(t, on, "textenc_set_graph"); }
int64_t ldiff_textenc_graph_replays(ldiff_textenc* t) { return t ? (int64_t)t->gc.replays : -1; }
int64_t ldiff_textenc_graph_nodes(ldiff_textenc* t) { return t ? (int64_t)t->gc.nodes : -1; }
int ldiff_textenc_forward(ldiff_textenc* t, const int32_t* ids_host, int B, int L, int project, void* out_dev, int out_dtype, void* stream) {
  API_BEGIN
  LDIFF_CHECK(t, LDIFF_ERR_INVALID, "textenc_forward: null handle");
  report_nonfinite(t->nf, "textenc_forward");
  t->forward(ids_host, B, L, project, out_dev, out_dtype, (hipStream_t)stream);
  API_END
}
int ldiff_textenc_check_finite(ldiff_textenc* t, void* stream) { return check_finite(t, stream, "textenc_check_finite"); }
void ldiff_textenc_destroy(ldiff_textenc* t) { destroy(t); }
int ldiff_op_text_attention(const void* qkv, int ld, int hidden, void* o, int ldo, int B, int heads, int L, int d, float scale, void* stream) {
  API_BEGIN
  LDIFF_CHECK(qkv && o, LDIFF_ERR_INVALID, "op_text_attention: null argument");
  launch_text_attention((const f16*)qkv, ld, hidden, (f16*)o, ldo, 0, B, heads, L, d, scale, (hipStream_t)stream);
  API_END
}
int ldiff_op_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, void* stream) {
  API_BEGIN
  launch_maxpool3x3s2((const f16*)x, (f16*)y, B, H, W, C, (hipStream_t)stream);
  API_END
}
int ldiff_op_crop_resize_norm(const void* rgb_u8, int H, int W, const void* boxes_i32, int n, const void* lut_u8, int S, const double* mean3, const double* std3, void* out_f16,
                              void* stream) {
  API_BEGIN
  launch_crop_resize_norm((const uint8_t*)rgb_u8, H, W, (const int*)boxes_i32, n, (const uint8_t*)lut_u8, S, mean3, std3, (f16*)out_f16, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_resize_u8_ws_bytes(int B, int Hs, int Ws, int C, int Ho, int Wo, int to_float) { return resize_u8_ws_bytes(B, Hs, Ws, C, Ho, Wo, to_float); }
int ldiff_op_resize_u8(const void* x_u8, int B, int Hs, int Ws, int C, int Ho, int Wo, const void* hbounds_i32, const void* hcoef_i32, int htaps, const void* vbounds_i32,
                       const void* vcoef_i32, int vtaps, const void* lut_f32_or_null, void* out, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  launch_resize_u8((const uint8_t*)x_u8, B, Hs, Ws, C, Ho, Wo, (const int*)hbounds_i32, (const int*)hcoef_i32, htaps, (const int*)vbounds_i32, (const int*)vcoef_i32, vtaps,
                   (const float*)lut_f32_or_null, out, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_label_table_u8(const void* src_u8, void* dst_u8, int64_t n, const void* table_u8, void* stream) {
  API_BEGIN
  launch_label_table_u8((const uint8_t*)src_u8, (uint8_t*)dst_u8, n, (const uint8_t*)table_u8, (hipStream_t)stream);
  API_END
}
int ldiff_op_gather_labels(const void* cache_u8, int N, int H, int W, const void* idx_i32, int B, void* label_u8, void* mask_i64, void* stream) {
  API_BEGIN
  launch_gather_labels((const uint8_t*)cache_u8, N, H, W, (const int*)idx_i32, B, (uint8_t*)label_u8, (long long*)mask_i64, (hipStream_t)stream);
  API_END
}
int ldiff_op_warmup_labels_supported(int H, int W, int oh, int ow) { return warmup_labels_supported(H, W, oh, ow); }
int ldiff_op_warmup_labels(const void* cache_u8, int N, int H, int W, const void* idx_i32, int B, int oh, int ow, void* out_u8, void* stream) {
  API_BEGIN
  launch_warmup_labels((const uint8_t*)cache_u8, N, H, W, (const int*)idx_i32, B, oh, ow, (uint8_t*)out_u8, (hipStream_t)stream);
  API_END
}
int ldiff_op_warmup_images(const void* cache_u8, int N, int Hs, int Ws, const void* idx_i32, int B, const void* table_f32, const void* ybounds_i32, const void* yweights_f32, int ytaps,
                           const void* xbounds_i32, const void* xweights_f32, int xtaps, int oh, int ow, void* out_f32, void* stream) {
  API_BEGIN
  launch_warmup_images((const uint8_t*)cache_u8, N, Hs, Ws, (const int*)idx_i32, B, (const float*)table_f32, (const int*)ybounds_i32, (const float*)yweights_f32, ytaps,
                       (const int*)xbounds_i32, (const float*)xweights_f32, xtaps, oh, ow, (float*)out_f32, (hipStream_t)stream);
  API_END
}
int ldiff_op_cls_head(const void* x, int B, int HW, int A, int ldx, const void* w_f32, const void* bias_f32, int C, void* logits_f32, void* labels_i32_or_null, void* stream) {
  API_BEGIN
  launch_cls_head((const f16*)x, B, HW, A, ldx, (const float*)w_f32, (const float*)bias_f32, C, (float*)logits_f32, (int*)labels_i32_or_null, (hipStream_t)stream);
  API_END
}
int ldiff_op_cls_head_feat(const void* x, int B, int HW, int A, int ldx, const void* w_f32, const void* bias_f32, int C, void* logits_f32_or_null, void* labels_i32_or_null,
                           void* features_f32_or_null, void* stream) {
  API_BEGIN
  launch_cls_head_feat((const f16*)x, B, HW, A, ldx, (const float*)w_f32, (const float*)bias_f32, C, (float*)logits_f32_or_null, (int*)labels_i32_or_null, (float*)features_f32_or_null,
                       (hipStream_t)stream);
  API_END
}
int ldiff_unet_attach_controlnet(ldiff_unet* u, ldiff_controlnet* c, float conditioning_scale) {
  API_BEGIN
  LDIFF_CHECK(u, LDIFF_ERR_INVALID, "unet_attach_controlnet: null handle");
  if (c) {
    const ldiff_unet_cfg &a = u->cfg, &b = c->trunk.cfg;
    bool same = a.n_blocks == b.n_blocks && a.layers_per_block == b.layers_per_block && a.in_channels == b.in_channels && u->device == c->trunk.device;
    std::string sa, sb;
    for (int i = 0; i < a.n_blocks; ++i) sa += (i ? "," : "") + std::to_string(a.block_out_channels[i]);
    for (int i = 0; i < b.n_blocks; ++i) sb += (i ? "," : "") + std::to_string(b.block_out_channels[i]);
    LDIFF_CHECK(same && sa == sb, LDIFF_ERR_INVALID,
                "unet_attach_controlnet: the UNet has widths [%s], %d layers per block, %d input channels (device %d); the ControlNet [%s], %d, %d (device %d)", sa.c_str(),
                a.layers_per_block, a.in_channels, u->device, sb.c_str(), b.layers_per_block, b.in_channels, c->trunk.device);
  }
  u->cn = c;
  u->cn_scale = conditioning_scale;
  ++u->cn_epoch;
  API_END
}

// ---- VAE ----
int ldiff_vae_create(ldiff_vae** out, const ldiff_vae_cfg* cfg, int device) {
  API_BEGIN
  LDIFF_CHECK(out && cfg, LDIFF_ERR_INVALID, "vae_create: null argument");
  select_device("vae_create", device);
  ldiff_vae* v = new ldiff_vae();
  v->cfg = *cfg;
  v->device = device;
  try { v->build(); } catch (...) { delete v; throw; }
  *out = v;
  API_END
}
int ldiff_vae_load(ldiff_vae* v, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) { return load(v, "vae_load", name, host_ptr, dtype, shape, ndim); }
int ldiff_vae_set_precision(ldiff_vae* v, int encoder_mode, int decoder_mode) {
  API_BEGIN
  LDIFF_CHECK(v && encoder_mode >= PREC_FAST && encoder_mode <= PREC_FULL && decoder_mode >= PREC_FAST && decoder_mode <= PREC_FULL, LDIFF_ERR_INVALID,
              "vae_set_precision: modes must be 0, 1 or 2");
  v->prec_enc = encoder_mode; v->prec_dec = decoder_mode;
  API_END
}
int ldiff_vae_set_range_shift(ldiff_vae* v, int k) {
  API_BEGIN
  LDIFF_CHECK(v && k >= 0 && k <= 16, LDIFF_ERR_INVALID, "vae_set_range_shift: k = %d outside 0..16", k);
  v->set_range_shift(k);
  API_END
}
int ldiff_vae_set_plan_batch(ldiff_vae* v, int n) {
  API_BEGIN
  LDIFF_CHECK(v, LDIFF_ERR_INVALID, "vae_set_plan_batch: null handle");
  LDIFF_CHECK(n >= 0, LDIFF_ERR_INVALID, "vae_set_plan_batch: n = %d must be >= 0 (0 = off)", n);
  v->set_plan_batch(n);
  API_END
}
int ldiff_vae_missing(ldiff_vae* v) { return missing(v); }
const char* ldiff_vae_missing_name(ldiff_vae* v, int i) { return missing_name(v, i); }
int ldiff_vae_encode(ldiff_vae* v, const void* x_dev, int B, int H, int W, void* moments_dev, void* stream) {
  API_BEGIN
  LDIFF_CHECK(v, LDIFF_ERR_INVALID, "vae_encode: null handle");
  report_nonfinite(v->nf, "vae_encode", VAE_RANGE_HINT);
  v->encode((const float*)x_dev, B, H, W, (float*)moments_dev, (hipStream_t)stream);
  API_END
}
int ldiff_vae_decode(ldiff_vae* v, const void* z_dev, int B, int h, int w, float z_scale, void* sample_nchw, void* image_nhwc, void* rgb_u8,
                     void* luma_u8, int n_slots, int slot, void* stream) {
  API_BEGIN
  LDIFF_CHECK(v, LDIFF_ERR_INVALID, "vae_decode: null handle");
  report_nonfinite(v->nf, "vae_decode", VAE_RANGE_HINT);
  v->wait_side((hipStream_t)stream);   // a sampler with a deferred join may still be decoding on the side stream (same workspace)
  v->decode((const float*)z_dev, B, h, w, z_scale, (float*)sample_nchw, (float*)image_nhwc, (uint8_t*)rgb_u8, (uint8_t*)luma_u8, n_slots, slot,
            (hipStream_t)stream);
  API_END
}
int ldiff_vae_check_finite(ldiff_vae* v, void* stream) {
  return check_finite(v, stream, "vae_check_finite", VAE_RANGE_HINT, [v] {
    if (v->side_stream) HIP_CHECK(hipStreamSynchronize(v->side_stream));
  });
}
void ldiff_vae_destroy(ldiff_vae* v) {
  destroy(v, [v] {
    if (v->ev_side) (void)hipEventDestroy(v->ev_side);
    if (v->side_stream) (void)hipStreamDestroy(v->side_stream);
  });
}

// ---- sampler arithmetic ----
int ldiff_pndm_step(const float* coef, const void* const* ops, int nops, void* out, int64_t n, void* stream) {
  API_BEGIN
  LDIFF_CHECK(coef && ops && out && n >= 0, LDIFF_ERR_INVALID, "pndm_step: bad arguments");
  launch_lincomb(coef, ops, nops, (float*)out, n, (hipStream_t)stream);
  API_END
}
int ldiff_pndm_coeffs(float a_t, float a_prev, float* sample_coeff, float* eps_coeff) {
  // PNDMScheduler._get_prev_sample in float32, one IEEE operation per python operator:
  //   prev = sqrt(a_prev/a_t)*sample - (a_prev-a_t)*eps / (a_t*sqrt(1-a_prev) + sqrt(a_t*(1-a_t)*a_prev))
  if (!sample_coeff || !eps_coeff || !(a_t > 0.f) || !(a_prev > 0.f)) { ldiff_set_error("pndm_coeffs: bad arguments"); return LDIFF_ERR_INVALID; }
  const volatile float b_t = 1.f - a_t, b_prev = 1.f - a_prev;
  const volatile float sc = sqrtf(a_prev / a_t);
  const volatile float d1 = a_t * sqrtf(b_prev);
  const volatile float d2 = sqrtf((a_t * b_t) * a_prev);
  const volatile float denom = d1 + d2;
  *sample_coeff = sc;
  *eps_coeff = -(a_prev - a_t) / denom;
  return LDIFF_OK;
}
int ldiff_pndm_alphas_cumprod(float* out_host, int n) {
  API_BEGIN
  LDIFF_CHECK(out_host && n == 1000, LDIFF_ERR_INVALID, "alphas_cumprod: n must be 1000");
  pndm_alphas_cumprod(out_host);
  API_END
}
int ldiff_laplace_add(const void* z0, float scale, const void* u, uint64_t seed, uint64_t offset, void* out, int64_t n, void* stream) {
  API_BEGIN
  LDIFF_CHECK(z0 && out && n >= 0, LDIFF_ERR_INVALID, "laplace_add: bad arguments");
  LDIFF_CHECK(scale >= 0.f, LDIFF_ERR_INVALID, "laplace_add: scale must be >= 0 (got %g)", (double)scale);
  launch_laplace_add((const float*)z0, scale, (const float*)u, seed, offset, (float*)out, n, (hipStream_t)stream);
  API_END
}
int ldiff_argmax_u8(const void* logits, int B, int C, int H, int W, void* mask_u8, void* stream) {
  API_BEGIN
  LDIFF_CHECK(B >= 0 && H >= 0 && W >= 0, LDIFF_ERR_INVALID, "argmax: negative extent");
  if ((long long)B * H * W == 0) return LDIFF_OK;   // empty batch: nothing to do (pointers may be null)
  LDIFF_CHECK(logits && mask_u8, LDIFF_ERR_INVALID, "argmax: null pointer");
  launch_argmax_u8((const float*)logits, B, C, H, W, (uint8_t*)mask_u8, (hipStream_t)stream);
  API_END
}
int ldiff_confusion(const void* pred, int pred_kind, const void* target, int target_kind, const uint8_t* pred_lut_or_null, const uint8_t* target_lut_or_null, int B, int C, int H,
                    int W, int64_t* conf, int64_t* dropped_or_null, void* stream) {
  API_BEGIN
  launch_confusion(pred, pred_kind, target, target_kind, pred_lut_or_null, target_lut_or_null, B, C, H, W, conf, dropped_or_null, (hipStream_t)stream);
  API_END
}
int ldiff_seg_metrics(const int64_t* conf_host, int C, ldiff_seg_metrics_out* out) { return seg_metrics_host(conf_host, C, out); }
int ldiff_probe_argmax_u8(const void* features_u8, int B, int N, int H, int W, const void* weight, const void* bias_or_null, float scale, int C, void* mask_u8,
                          void* stream) {
  API_BEGIN
  LDIFF_CHECK(B >= 0 && H >= 0 && W >= 0, LDIFF_ERR_INVALID, "probe_argmax: negative extent");
  if ((long long)B * H * W == 0) return LDIFF_OK;
  LDIFF_CHECK(features_u8 && weight && mask_u8, LDIFF_ERR_INVALID, "probe_argmax: null pointer");
  launch_probe_argmax_u8((const uint8_t*)features_u8, B, N, H, W, (const float*)weight, (const float*)bias_or_null, scale, C, (uint8_t*)mask_u8, (hipStream_t)stream);
  API_END
}
int ldiff_window_accumulate(void* acc, void* cnt, const void* pred, const void* weight_or_null, int C, int H, int W, int th, int tw, int y0, int x0, int dtypes,
                            void* stream) {
  API_BEGIN
  LDIFF_CHECK(acc && cnt && pred, LDIFF_ERR_INVALID, "window_accumulate: null argument");
  launch_window_accumulate(acc, cnt, pred, weight_or_null, C, H, W, th, tw, y0, x0, dtypes, (hipStream_t)stream);
  API_END
}
// batched sliding window of the tissue head (kernels_segwin.hip); the launchers hold every refusal, so that nothing is enqueued on a bad argument
int ldiff_op_window_gather(const void* img_f32, int C, int h, int w, int64_t row_stride, int64_t plane_stride, int pad_top, int pad_left, int Hp, int Wp,
                           const ldiff_window_tiles* tiles, int th, int tw, void* x_f32, void* stream) {
  API_BEGIN
  LDIFF_CHECK(img_f32 && tiles && x_f32, LDIFF_ERR_INVALID, "window_gather: null argument");
  launch_window_gather((const float*)img_f32, C, h, w, row_stride, plane_stride, pad_top, pad_left, Hp, Wp, *tiles, th, tw, (float*)x_f32, (hipStream_t)stream);
  API_END
}
int ldiff_op_window_accumulate_batch(void* acc, void* cnt, const void* pred, const void* weight_or_null, int heads, int Hp, int Wp, int th, int tw,
                                     const ldiff_window_tiles* tiles, int dtypes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(acc && cnt && pred && tiles, LDIFF_ERR_INVALID, "window_accumulate_batch: null argument");
  launch_window_accumulate_batch(acc, cnt, pred, weight_or_null, heads, Hp, Wp, th, tw, *tiles, dtypes, (hipStream_t)stream);
  API_END
}
int ldiff_op_window_finish(const void* acc, const void* cnt, int heads, int Hp, int Wp, int y0, int x0, int h, int w, int acc_f16, void* logits_or_null,
                           void* mask_or_null, int mask_H, int mask_W, int mask_y0, int mask_x0, int32_t* inf_flag, void* stream) {
  API_BEGIN
  LDIFF_CHECK(acc && cnt && inf_flag, LDIFF_ERR_INVALID, "window_finish: null argument");
  launch_window_finish(acc, cnt, heads, Hp, Wp, y0, x0, h, w, acc_f16, logits_or_null, (uint8_t*)mask_or_null, mask_H, mask_W, mask_y0, mask_x0, inf_flag,
                       (hipStream_t)stream);
  API_END
}
int ldiff_op_window_finish_ensemble(const void* const* acc, int n_folds, const void* cnt_or_null, int heads, int Hp, int Wp, int y0, int x0, int h, int w,
                                    int acc_f16, void* logits_or_null, void* mask_or_null, int mask_H, int mask_W, int mask_y0, int mask_x0, int32_t* inf_flag,
                                    void* stream) {
  API_BEGIN
  LDIFF_CHECK(acc && inf_flag, LDIFF_ERR_INVALID, "window_finish_ensemble: null argument");
  launch_window_finish_ensemble(acc, n_folds, cnt_or_null, heads, Hp, Wp, y0, x0, h, w, acc_f16, logits_or_null, (uint8_t*)mask_or_null, mask_H, mask_W, mask_y0,
                                mask_x0, inf_flag, (hipStream_t)stream);
  API_END
}
int ldiff_luma_float(const void* rgb_nchw, void* gray, int B, int H, int W, void* stream) {
  API_BEGIN
  LDIFF_CHECK(rgb_nchw && gray, LDIFF_ERR_INVALID, "luma_float: null argument");
  launch_luma_float((const float*)rgb_nchw, (float*)gray, B, H, W, (hipStream_t)stream);
  API_END
}
int ldiff_bilinear_resize(const void* x_nchw, void* y_nchw, int B, int C, int H, int W, int out_h, int out_w, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x_nchw && y_nchw, LDIFF_ERR_INVALID, "bilinear_resize: null argument");
  LDIFF_CHECK(B >= 0 && C >= 1 && H >= 1 && W >= 1 && out_h >= 1 && out_w >= 1, LDIFF_ERR_INVALID, "bilinear_resize: bad shape");
  launch_bilinear_resize((const float*)x_nchw, (float*)y_nchw, B, C, H, W, out_h, out_w, (hipStream_t)stream);
  API_END
}

// ---- fused sampler ----
int ldiff_pipeline_create(ldiff_pipeline** out, ldiff_unet* u, ldiff_vae* v) {
  API_BEGIN
  LDIFF_CHECK(out && u && v, LDIFF_ERR_INVALID, "pipeline_create: null argument");
  LDIFF_CHECK(u->device == v->device, LDIFF_ERR_INVALID, "pipeline_create: unet and vae live on different devices");
  LDIFF_CHECK(u->cfg.in_channels == v->cfg.latent_channels && u->cfg.out_channels == v->cfg.latent_channels, LDIFF_ERR_INVALID,
              "pipeline_create: unet channels do not match the vae latent channels");
  ldiff_pipeline* p = new ldiff_pipeline();
  p->unet = u;
  p->vae = v;
  pndm_alphas_cumprod(p->abar);
  HIP_CHECK(hipSetDevice(u->device));
  if (!v->side_stream) {   // one side stream per VAE: all feature-only decodes of all samplers on it serialise (one decoder workspace)
    HIP_CHECK(hipStreamCreateWithFlags(&v->side_stream, hipStreamNonBlocking));   // (stream priorities made no difference: 46.1-46.3 patches/s)
    HIP_CHECK(hipEventCreateWithFlags(&v->ev_side, hipEventDisableTiming));
  }
  HIP_CHECK(hipEventCreateWithFlags(&p->ev_latents, hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&p->ev_decoded, hipEventDisableTiming));
  *out = p;
  API_END
}
// CU-restricted streams (experiment): bit i of the mask is set where lo32 <= i % 32 < hi32, so every XCD keeps the same share of
// its 32 CUs whichever way the runtime numbers them (interleaved over the XCDs or XCD by XCD) as long as lo32 / hi32 are multiples of 8.
static void make_cu_share_stream(int lo32, int hi32, hipStream_t* out) {
  LDIFF_CHECK(lo32 >= 0 && hi32 <= 32 && lo32 < hi32 && (lo32 & 7) == 0 && (hi32 & 7) == 0, LDIFF_ERR_INVALID,
              "cu share: need 0 <= lo32 < hi32 <= 32, both multiples of 8");
  int dev = 0, cus = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const uint32_t word = (hi32 == 32 ? 0xffffffffu : ((1u << hi32) - 1u)) & ~((1u << lo32) - 1u);
  std::vector<uint32_t> mask((size_t)((cus + 31) / 32), word);
  HIP_CHECK(hipExtStreamCreateWithCUMask(out, (uint32_t)mask.size(), mask.data()));
}
int ldiff_stream_create_cu_share(int lo32, int hi32, void** stream_out) {
  API_BEGIN
  LDIFF_CHECK(stream_out, LDIFF_ERR_INVALID, "stream_create_cu_share: null argument");
  hipStream_t s = nullptr;
  make_cu_share_stream(lo32, hi32, &s);
  *stream_out = (void*)s;
  API_END
}
int ldiff_stream_destroy(void* stream) {
  API_BEGIN
  if (stream) HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
  API_END
}
int ldiff_vae_set_side_cu_share(ldiff_vae* v, int lo32, int hi32) {
  API_BEGIN
  LDIFF_CHECK(v, LDIFF_ERR_INVALID, "vae_set_side_cu_share: null vae");
  HIP_CHECK(hipSetDevice(v->device));
  hipStream_t s = nullptr;
  if (lo32 == 0 && hi32 == 32) HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  else make_cu_share_stream(lo32, hi32, &s);
  if (v->side_stream) {
    HIP_CHECK(hipStreamSynchronize(v->side_stream));
    HIP_CHECK(hipStreamDestroy(v->side_stream));
  } else {
    HIP_CHECK(hipEventCreateWithFlags(&v->ev_side, hipEventDisableTiming));
  }
  v->side_stream = s;
  API_END
}
int ldiff_pipeline_set_overlap(ldiff_pipeline* p, int mode) {
  API_BEGIN
  LDIFF_CHECK(p && mode >= 0 && mode <= 2, LDIFF_ERR_INVALID, "set_overlap: mode must be 0, 1 or 2");
  LDIFF_CHECK(!p->join_pending, LDIFF_ERR_STATE, "set_overlap: a deferred join is pending; call ldiff_pipeline_join first");
  p->overlap = mode;
  API_END
}
int ldiff_pipeline_join(ldiff_pipeline* p, void* stream) {
  API_BEGIN
  LDIFF_CHECK(p, LDIFF_ERR_INVALID, "join: null pipeline");
  if (p->join_pending) {
    HIP_CHECK(hipSetDevice(p->unet->device));
    HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, p->ev_decoded, 0));
    p->join_pending = false;
  }
  API_END
}
int ldiff_pipeline_set_alphas_cumprod(ldiff_pipeline* p, const float* abar_host, int n) {
  API_BEGIN
  LDIFF_CHECK(p && abar_host && n == 1000, LDIFF_ERR_INVALID, "set_alphas_cumprod: need 1000 float32 values");
  for (int i = 0; i < n; ++i) LDIFF_CHECK(abar_host[i] > 0.f && abar_host[i] <= 1.f, LDIFF_ERR_INVALID, "set_alphas_cumprod: value %d out of (0,1]", i);
  memcpy(p->abar, abar_host, sizeof(float) * 1000);
  API_END
}
int ldiff_plms_timesteps(int n_passes, int64_t* out, int cap) {
  try { return plms_timesteps(n_passes, out, cap); } catch (const LdiffError& e) { return e.code; }
}

int ldiff_sample(ldiff_pipeline* p, const void* images, int B, int H, int W, int n_passes, void* latents_out, void* features_u8, void* rgb_u8,
                 void* stream) {
  API_BEGIN
  LDIFF_CHECK(p && images, LDIFF_ERR_INVALID, "sample: null argument");
  hipStream_t s = (hipStream_t)stream;
  ldiff_unet* u = p->unet;
  ldiff_vae* v = p->vae;
  HIP_CHECK(hipSetDevice(u->device));
  report_nonfinite(u->nf, "sample (unet)");
  report_nonfinite(v->nf, "sample (vae)");
  int64_t ts[1024];
  const int nts = plms_timesteps(n_passes, ts, 1024);
  const int f = 1 << (v->cfg.n_blocks - 1), lat = v->cfg.latent_channels;
  LDIFF_CHECK(B >= 1 && H >= f && W >= f && H % f == 0 && W % f == 0, LDIFF_ERR_INVALID, "sample: bad batch/image size (B=%d, %dx%d)", B, H, W);
  const int h = H / f, w = W / f;
  const size_t nlat = (size_t)B * lat * h * w;
  // workspace: moments (2x), latents ping-pong (2), cur_sample, eps history (4), fresh eps, one latent snapshot per pass
  p->arena.reserve((2 + 2 + 1 + 4 + 1 + (size_t)nts) * nlat * sizeof(float) + (16 + (size_t)nts) * 256);
  p->arena.reset();
  auto buf = [&]() { return (float*)p->arena.alloc(nlat * sizeof(float)); };
  float* moments = (float*)p->arena.alloc(2 * nlat * sizeof(float));
  float* z = buf();
  float* znext = buf();
  float* cur_sample = buf();
  float* ets[4] = {buf(), buf(), buf(), buf()};
  float* eps_new = buf();

  // this pipeline's previous call may still be decoding from its latent snapshots (deferred join): its buffers are reused now
  if (p->join_pending) { HIP_CHECK(hipStreamWaitEvent(s, p->ev_decoded, 0)); p->join_pending = false; }
  if (p->overlap == 0) v->wait_side(s);   // decodes on the caller's stream share the decoder workspace with the side stream
  // z = vae.encode(x).latent_dist.mean   (no scaling_factor: pixel_latent_vector.py:73)
  v->encode((const float*)images, B, H, W, moments, s);
  HIP_CHECK(hipMemcpy2DAsync(z, (size_t)lat * h * w * 4, moments, (size_t)2 * lat * h * w * 4, (size_t)lat * h * w * 4, B, hipMemcpyDeviceToDevice, s));

  // Two streams: the UNet / PLMS chain stays on the caller's stream; the VAE decode of pass k (it only feeds the feature
  // tensor, nothing downstream in the loop) runs on the pipeline's side stream beside the UNet pass k+1, whose deep levels
  // (16x16 / 8x8 maps: tens of workgroups per launch) leave most CUs idle.  Each decode reads its own snapshot of the
  // latents, so the chain never waits for it; the caller's stream joins the side stream before returning.
  const bool overlap = p->overlap != 0;
  hipStream_t sd = overlap ? v->side_stream : s;
  bool decoded_any = false;

  const int n_sched = n_passes == 1 ? 1 : n_passes - 1;
  const int ratio = 1000 / n_sched;
  int n_ets = 0, counter = 0;  // ets[0] is the oldest kept entry
  for (int i = 0; i < nts; ++i) {
    int t = (int)ts[i];
    u->forward(z, B, h, w, (float)t, eps_new, s);
    // ---- PNDMScheduler.step_plms ----
    int prev_t = t - ratio;
    const float* sample = z;
    // weights on {eps_new (when not stored), ets[-1], ets[-2], ets[-3], ets[-4]}; kept in double and folded into the
    // float32 eps coefficient with ONE rounding, exactly like the python scheduler shim (fp16 activations amplify a
    // 1-ulp coefficient difference into ~1e-4 latent differences, so the two drivers must agree bit for bit)
    double wts[5] = {0, 0, 0, 0, 0};
    const float* opsrc[5] = {eps_new, nullptr, nullptr, nullptr, nullptr};
    if (counter != 1) {
      // ets = ets[-3:] + [eps_new]: rotate the ring so that ets[n_ets-1] is the newest
      if (n_ets == 4) { float* old = ets[0]; ets[0] = ets[1]; ets[1] = ets[2]; ets[2] = ets[3]; ets[3] = old; n_ets = 3; }
      std::swap(ets[n_ets], eps_new);     // store without copying; eps_new now names a free buffer
      ++n_ets;
    } else {
      prev_t = t;
      t = t + ratio;
    }
    int nops = 0;
    float coef[6];
    const void* ops[6];
    if (n_ets == 1 && counter == 0) {
      wts[1] = 1.0;
      HIP_CHECK(hipMemcpyAsync(cur_sample, z, nlat * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else if (n_ets == 1 && counter == 1) {
      wts[0] = 0.5; wts[1] = 0.5;       // (model_output + ets[-1]) / 2
      sample = cur_sample;
    } else if (n_ets == 2) { wts[1] = 3.0 / 2; wts[2] = -1.0 / 2; }
    else if (n_ets == 3) { wts[1] = 23.0 / 12; wts[2] = -16.0 / 12; wts[3] = 5.0 / 12; }
    else { wts[1] = 55.0 / 24; wts[2] = -59.0 / 24; wts[3] = 37.0 / 24; wts[4] = -9.0 / 24; }
    for (int k = 1; k <= 4; ++k) opsrc[k] = (n_ets - k >= 0) ? ets[n_ets - k] : nullptr;
    // ---- _get_prev_sample: prev = sqrt(a_prev/a_t)*sample - (a_prev-a_t)*eps/(a_t*sqrt(1-a_prev)+sqrt(a_t*(1-a_t)*a_prev)) ----
    const float a_t = p->abar[t], a_prev = prev_t >= 0 ? p->abar[prev_t] : p->abar[0];
    float sample_coeff, ce;
    ldiff_pndm_coeffs(a_t, a_prev, &sample_coeff, &ce);
    coef[nops] = sample_coeff; ops[nops++] = sample;
    for (int k = 0; k < 5; ++k)
      if (wts[k] != 0.0) { coef[nops] = (float)((double)ce * wts[k]); ops[nops++] = opsrc[k]; }
    static const bool debug = getenv("LDIFF_DEBUG") != nullptr;   // read once per process
    if (debug) {
      fprintf(stderr, "[ldiff_sample] pass %d t=%d prev_t=%d n_ets=%d nops=%d coef:", i, t, prev_t, n_ets, nops);
      for (int k = 0; k < nops; ++k) fprintf(stderr, " %.9g", (double)coef[k]);
      fprintf(stderr, "\n");
    }
    launch_lincomb(coef, ops, nops, znext, (long long)nlat, s);
    std::swap(z, znext);
    ++counter;
    // ---- decode_latents + numpy_to_pil + convert("L") ----
    const bool last = i == nts - 1;
    if (features_u8 || (last && rgb_u8)) {
      const float* zdec = z;
      if (overlap) {
        float* snap = buf();
        HIP_CHECK(hipMemcpyAsync(snap, z, nlat * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipEventRecord(p->ev_latents, s));
        HIP_CHECK(hipStreamWaitEvent(sd, p->ev_latents, 0));   // also orders the first decode behind the encode (same VAE workspace)
        zdec = snap;
      }
      v->ex_dec.short_runs = overlap;   // beside the next UNet pass: persistent conv kernels walk short runs (ConvParams::short_runs); alone on the chip: one workgroup per CU
      v->decode(zdec, B, h, w, 1.0f / v->cfg.scaling_factor, nullptr, nullptr, last ? (uint8_t*)rgb_u8 : nullptr, (uint8_t*)features_u8, nts, i, sd);
      v->ex_dec.short_runs = false;
      decoded_any = true;
    }
  }
  if (overlap && decoded_any) {
    HIP_CHECK(hipEventRecord(p->ev_decoded, sd));
    HIP_CHECK(hipEventRecord(v->ev_side, sd));
    v->side_used = true;
    if (p->overlap == 1) HIP_CHECK(hipStreamWaitEvent(s, p->ev_decoded, 0));
    else p->join_pending = true;   // mode 2: the caller joins (ldiff_pipeline_join) before it reads features / rgb
  }
  if (latents_out) HIP_CHECK(hipMemcpyAsync(latents_out, z, nlat * sizeof(float), hipMemcpyDeviceToDevice, s));
  API_END
}
int ldiff_pipeline_check_finite(ldiff_pipeline* p, void* stream) {
  API_BEGIN
  LDIFF_CHECK(p, LDIFF_ERR_INVALID, "pipeline_check_finite: null pipeline");
  HIP_CHECK(hipSetDevice(p->unet->device));
  if (p->join_pending) { HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, p->ev_decoded, 0)); p->join_pending = false; }
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  if (p->vae->side_stream) HIP_CHECK(hipStreamSynchronize(p->vae->side_stream));
  const bool bad_u = p->unet->nf.test_and_clear(), bad_v = p->vae->nf.test_and_clear();
  LDIFF_CHECK(!bad_u && !bad_v, LDIFF_ERR_NONFINITE,
              "pipeline_check_finite: a non-finite activation (fp16 overflow: |x| > 65504, or NaN) was detected in the %s graph; the results of that call are invalid. "
              "Activations are stored as fp16 in every precision mode (set_precision 1 / 2 add mantissa bits, not range): rescale the input / checkpoint, "
              "and use LDIFF_TRACE_ABSMAX=1 to see which stage overflows.%s", bad_u && bad_v ? "UNet and VAE" : bad_u ? "UNet" : "VAE", bad_v ? VAE_RANGE_HINT : "");
  API_END
}
void ldiff_pipeline_destroy(ldiff_pipeline* p) {
  if (!p) return;
  (void)hipDeviceSynchronize();
  if (p->ev_latents) (void)hipEventDestroy(p->ev_latents);
  if (p->ev_decoded) (void)hipEventDestroy(p->ev_decoded);
  delete p;
}

// ---- single-kernel entry points ----
// grow-only scratch per (device, stream, slot) for the handle-less op entry points
static void* op_scratch(hipStream_t st, int slot, size_t bytes) {
  struct Buf { void* p = nullptr; size_t cap = 0; };
  static std::mutex mu;
  static std::map<std::tuple<int, hipStream_t, int>, Buf> bufs;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  Buf& b = bufs[std::make_tuple(dev, st, slot)];
  if (bytes > b.cap) {
    if (b.p) { HIP_CHECK(hipStreamSynchronize(st)); HIP_CHECK(hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    HIP_CHECK(hipMalloc(&b.p, bytes));
    b.cap = bytes;
  }
  return b.p;
}
static void conv_args_to_params(const ldiff_conv_args* a, ConvParams& p) {
  LDIFF_CHECK(a && a->x && a->w && a->y, LDIFF_ERR_INVALID, "op_conv: null argument");
  memset(&p, 0, sizeof(p));
  p.x = (const f16*)a->x; p.x2 = (const f16*)a->x2; p.C1 = a->C1; p.C2 = a->C2;
  p.B = a->B; p.Hin = a->Hin; p.Win = a->Win; p.Hout = a->Hout; p.Wout = a->Wout;
  p.ks = a->ks; p.stride = a->stride; p.pad_t = a->pad_t; p.pad_l = a->pad_l; p.ups = a->ups;
  LDIFF_CHECK((p.ks == 1 || p.ks == 3 || (a->tconv && p.ks == 2) || ((a->relu_out || a->cls_conv > 0) && p.ks == 7)) && (p.stride == 1 || p.stride == 2) && (p.ups == 0 || p.ups == 1), LDIFF_ERR_INVALID,
              "op_conv: unsupported ks=%d stride=%d ups=%d", p.ks, p.stride, p.ups);
  p.w = (const f16*)a->w; p.N = a->N; p.Nrows = a->Nrows; p.K = a->ks * a->ks * (a->C1 + a->C2);
  p.n_real = a->n_real > 0 && a->n_real <= a->N ? a->n_real : 0;
  p.c3d_ups = a->c3d_ups;
  p.gn_scale = (const float*)a->gn_scale; p.gn_shift = (const float*)a->gn_shift; p.silu_in = a->silu_in;
  p.bias = (const float*)a->bias; p.temb = (const float*)a->temb; p.ld_temb = a->ld_temb;
  p.res = (const f16*)a->res; p.ld_res = a->ld_res;
  p.y = a->y; p.ldy = a->ldy; p.out_f32 = a->out_f32;
  p.ld1 = a->ld1; p.ld2 = a->ld2; p.res_lo = a->res_lo; p.y_lo = a->y_lo;
  p.short_runs = a->short_runs != 0;
  p.M = a->B * a->Hout * a->Wout;
  p.stats = (float*)a->stats;
  p.geglu = a->geglu != 0;
  p.lo8_slab0 = a->lo8_slab0; p.lo8_sa = (const int*)a->lo8_scale; p.lo8_sb = a->lo8_slab0 ? 127 - LO8_SHIFT : 0;
  p.df_force = a->gemm_df;
  p.xs = (const f16*)a->sc_x; p.Cs = a->sc_x ? a->sc_C : 0; p.lds = a->sc_x ? a->sc_ld : 0;
  p.out_shift = a->out_shift;   // (plan_conv checks 0..16)
  p.silu_out = a->silu_out != 0;
  p.cond_force = a->cond_conv;
  p.lrelu_in = a->lrelu_in; p.tconv = a->tconv; p.seg_conv = a->seg_conv;
  p.relu_out = a->relu_out != 0; p.cls_force = a->cls_conv;
  p.act_out = a->act_out;   // (plan_conv checks 0 | 1 | 2 and the route)
  p.bn_stats = (float*)a->bn_stats;   // (plan_conv: the classifier's conv family on request, or refused)
  if (p.tconv) p.K = a->C1;   // one GEMM over the coarse map: the four taps are column blocks, not K
}
int ldiff_op_conv_pb(const ldiff_conv_args* a, int plan_batch, void* stream) {
  API_BEGIN
  ConvParams p;
  conv_args_to_params(a, p);
  LDIFF_CHECK(plan_batch >= 0, LDIFF_ERR_INVALID, "op_conv: plan_batch = %d must be >= 0 (0 = off)", plan_batch);
  if (plan_batch > 0) { p.plan_B = plan_batch; p.plan_M = plan_batch * a->Hout * a->Wout; }   // (plan_conv refuses B > plan_batch)
  if (a->splitk)   // an explicit split count (tests, timing), taken as the executors' plans are
    LDIFF_CHECK(a->splitk >= 2 && a->splitk <= 16 && !p.out_f32 && !p.geglu && !p.ups && !p.xs && !p.lo8_slab0 && p.df_force <= 0, LDIFF_ERR_INVALID,
                "op_conv: splitk = %d needs 2..16 splits, an fp16 output and a plain 3x3 / 1x1 / strided launch", a->splitk);
  const bool df_asked = p.df_force > 0;
  ConvAsk ask;
  ask.splitk = a->splitk ? a->splitk : (p.stats || p.xs || df_asked) ? 1 : 0;   // no planned split beside fused statistics, a folded shortcut or a forced gemm_df
  ask.stats = p.stats != nullptr;
  ask.fold_gn = a->fold_gn != 0;
  const ConvPlan pl = plan_conv(p, ask);
  LDIFF_CHECK(!p.stats || p.stats_R > 0, LDIFF_ERR_INVALID, "op_conv: fused statistics are not supported for this shape");
  LDIFF_CHECK(!p.xs || (a->sc_w && pl.kernel == ConvKernel::C3_DATAFLOW), LDIFF_ERR_INVALID, "op_conv: a folded shortcut (sc_x) needs sc_w and a launch the dataflow conv3x3 kernel takes");
  if (df_asked) LDIFF_CHECK(pl.kernel == ConvKernel::GEMM_DF, LDIFF_ERR_INVALID, "op_conv: gemm_df asked for a launch the dataflow GEMM does not take");
  // This test/bench entry point has no handle to own the derived weights and the scratch, so it keeps one grow-only buffer per (device, stream):
  // reuse is stream-ordered, and two streams or devices never share one.
  hipStream_t st = (hipStream_t)stream;
  if (pl.parity) {
    f16* wpar = (f16*)op_scratch(st, 0, parity_weights_bytes(p));
    pack_parity_weights(p, wpar, st);
    p.w_par = wpar;
  }
  if (pl.weights != ConvWeights::PLAIN) {   // the executors cache these per layer (Exec::derived); here per call, by the same recipes (conv_route.hip)
    // LDIFF_OP_CACHE_FRAG=1 (timing scripts only): the dataflow GEMM's copy is packed once per (matrix address, shape) -- stale as soon as the caller
    // rewrites the matrix in place, which the tests do
    static const bool cache = [] { const char* e = getenv("LDIFF_OP_CACHE_FRAG"); return e && atoi(e) != 0; }();
    static std::mutex mu;
    static std::map<std::tuple<const void*, int, int>, f16*> packed;
    const size_t bytes = packed_weights_bytes(pl.weights, p);
    f16* wf = nullptr;
    bool pack = true;
    if (cache && pl.weights == ConvWeights::GEMM_FRAG) {
      std::lock_guard<std::mutex> lock(mu);
      f16*& kept = packed[std::make_tuple((const void*)p.w, p.Nrows, p.K)];
      pack = !kept;
      if (!kept) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&kept), bytes));
      wf = kept;
    } else {
      wf = (f16*)op_scratch(st, 3, bytes);
    }
    if (pack) pack_weights(pl.weights, p, (const f16*)a->sc_w, wf, st);
    p.w_frag = wf;
    if (pl.weights == ConvWeights::FRAG_SC) {   // the two biases summed
      float* bsum = (float*)op_scratch(st, 5, (size_t)p.Nrows * sizeof(float));
      pack_shortcut_bias(p, (const float*)a->sc_bias, bsum, st);
      p.bias = bsum;
    }
  }
  if (pl.fold_gn) {   // the executor's two launches (model.hip): per-image weights and biases, then the plain GEMM on them
    f16* wfold = (f16*)op_scratch(st, 6, (size_t)p.B * p.Nrows * p.K * sizeof(f16));
    float* bfold = (float*)op_scratch(st, 7, (size_t)p.B * p.Nrows * sizeof(float));
    launch_fold_gn_weights(p.w, p.bias, (const float*)a->gn_scale, (const float*)a->gn_shift, wfold, bfold, p.B, p.Nrows, p.K, st);
    p.w = wfold; p.bias = bfold;
  }
  if (p.splitk > 1) p.splitk_ws = (float*)op_scratch(st, 1, (size_t)p.splitk * p.M * p.N * sizeof(float));
  launch_igemm(p, pl, st);
  API_END
}
int ldiff_op_conv(const ldiff_conv_args* a, void* stream) { return ldiff_op_conv_pb(a, 0, stream); }
int ldiff_op_in_finalize(const void* part, int R, const void* x_f16, int ldx, int B, int HW, int C, float eps, const void* gamma, const void* beta, void* scale, void* shift,
                         int ld_ss, int ss_off, int ident, void* stream) {
  API_BEGIN
  LDIFF_CHECK((part || x_f16) && gamma && beta && scale && shift && B >= 1 && HW >= 1 && C >= 1 && ident >= 0 && ss_off >= ident && ss_off + C <= ld_ss && (part == nullptr || R >= 1) &&
                  (x_f16 == nullptr || ldx >= C),
              LDIFF_ERR_INVALID, "op_in_finalize: null argument, empty shape, or a row of %d entries that does not hold %d identity + %d channels at offset %d", ld_ss, ident, C, ss_off);
  launch_in_finalize((const float*)part, R, (const f16*)x_f16, ldx, B, HW, C, eps, (const float*)gamma, (const float*)beta, (float*)scale, (float*)shift, ld_ss, ss_off, ident,
                     (hipStream_t)stream, nullptr);
  API_END
}
int ldiff_op_conv_stats_blocks(const ldiff_conv_args* a) {
  try {
    ConvParams p;
    conv_args_to_params(a, p);
    ConvAsk ask;   // as ldiff_op_conv plans a launch with statistics
    ask.splitk = a->splitk > 1 ? a->splitk : 1;
    ask.stats = true;
    plan_conv(p, ask);
    return p.stats_R;
  } catch (const LdiffError& e) { return e.code; }
}
int ldiff_op_conv_bn_stats_blocks(const ldiff_conv_args* a) {
  try {
    ConvParams p;
    conv_args_to_params(a, p);
    float placeholder[2];
    if (!p.bn_stats) p.bn_stats = reinterpret_cast<float*>(((uintptr_t)placeholder + 7) & ~(uintptr_t)7);   // (read as null / non-null and for its alignment only)
    plan_conv(p, ConvAsk());
    return cls_conv_bn_stats_blocks(p);
  } catch (const LdiffError& e) { return e.code; }
}
int ldiff_op_bn_finalize(const void* part_f32, int R, int N, int64_t n, const void* gamma_f32, const void* beta_f32, void* scale_f32, void* shift_f32, void* batch_stats_f32,
                         int64_t offset, int64_t T, void* stream) {
  API_BEGIN
  launch_bn_finalize((const float*)part_f32, R, N, n, (const float*)gamma_f32, (const float*)beta_f32, (float*)scale_f32, (float*)shift_f32, (float*)batch_stats_f32, offset, T,
                     (hipStream_t)stream);
  API_END
}
int ldiff_op_bn_apply(const void* x_f16, int64_t M, int N, const void* scale_f32, const void* shift_f32, const void* id_f16_or_null, const void* id_scale_f32_or_null,
                      const void* id_shift_f32_or_null, int relu, void* y_f16, void* nonfinite_i32_or_null, void* stream) {
  API_BEGIN
  launch_bn_apply((const f16*)x_f16, M, N, (const float*)scale_f32, (const float*)shift_f32, (const f16*)id_f16_or_null, (const float*)id_scale_f32_or_null,
                  (const float*)id_shift_f32_or_null, relu, (f16*)y_f16, (int*)nonfinite_i32_or_null, (hipStream_t)stream);
  API_END
}
int ldiff_op_gn_finalize(const void* part1, int R1, int C1, const void* part2, int R2, int C2, int B, int HW, int groups, float eps,
                         const void* gamma, const void* beta, void* scale, void* shift, void* stream) {
  API_BEGIN
  LDIFF_CHECK(part1 && gamma && beta && scale && shift && B >= 1 && HW >= 1 && groups >= 1, LDIFF_ERR_INVALID, "op_gn_finalize: bad arguments");
  launch_gn_finalize((const float*)part1, R1, C1, (const float*)part2, R2, C2, B, HW, groups, eps, (const float*)gamma, (const float*)beta,
                     (float*)scale, (float*)shift, (hipStream_t)stream);
  API_END
}
int ldiff_op_attention_pb(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int B, int heads, int Lq,
                          int Lk, int d, int64_t q_bstride, int64_t kv_bstride, int64_t o_bstride, float scale, int plan_batch, void* stream) {
  API_BEGIN
  LDIFF_CHECK(q && k && v && o && B >= 1 && heads >= 1 && plan_batch >= 0, LDIFF_ERR_INVALID, "op_attention: bad arguments");
  AttnParams p;
  p.q = (const f16*)q; p.ldq = ldq; p.k = (const f16*)k; p.ldk = ldk; p.v = (const f16*)v; p.ldv = ldv; p.o = (f16*)o; p.ldo = ldo;
  p.B = B; p.heads = heads; p.Lq = Lq; p.Lk = Lk; p.d = d;
  p.q_bstride = q_bstride; p.kv_bstride = kv_bstride; p.o_bstride = o_bstride; p.scale = scale;
  p.plan_B = plan_batch;   // (launch_attention refuses B > plan_batch > 0)
  launch_attention(p, (hipStream_t)stream);
  API_END
}
int ldiff_op_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int B, int heads, int Lq,
                       int Lk, int d, int64_t q_bstride, int64_t kv_bstride, int64_t o_bstride, float scale, void* stream) {
  return ldiff_op_attention_pb(q, ldq, k, ldk, v, ldv, o, ldo, B, heads, Lq, Lk, d, q_bstride, kv_bstride, o_bstride, scale, 0, stream);
}
int ldiff_op_attention_prescaled(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int B, int heads, int Lq,
                                 int Lk, int d, int64_t q_bstride, int64_t kv_bstride, int64_t o_bstride, void* stream) {
  API_BEGIN
  LDIFF_CHECK(q && k && v && o && B >= 1 && heads >= 1, LDIFF_ERR_INVALID, "op_attention_prescaled: bad arguments");
  LDIFF_CHECK(attention_prescale_supported(d), LDIFF_ERR_INVALID, "op_attention_prescaled: head dim %d has no prescaled kernel (40 and 80 do)", d);
  AttnParams p;
  p.q = (const f16*)q; p.ldq = ldq; p.k = (const f16*)k; p.ldk = ldk; p.v = (const f16*)v; p.ldv = ldv; p.o = (f16*)o; p.ldo = ldo;
  p.B = B; p.heads = heads; p.Lq = Lq; p.Lk = Lk; p.d = d;
  p.q_bstride = q_bstride; p.kv_bstride = kv_bstride; p.o_bstride = o_bstride; p.scale = 1.0f; p.prescaled = 1;
  launch_attention(p, (hipStream_t)stream);
  API_END
}
int ldiff_op_gn_stats_pb(const void* x, int C1, int ld1, int lo1, const void* x2, int C2, int ld2, int lo2, int B, int HW, int groups, float eps,
                         const void* gamma, const void* beta, void* scale, void* shift, int plan_batch, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && gamma && beta && scale && shift && B >= 1 && HW >= 1 && groups >= 1 && plan_batch >= 0, LDIFF_ERR_INVALID, "op_gn_stats: bad arguments");
  const size_t bytes = gn_partial_bytes(B, HW, C1 + C2);
  float* partial = (float*)op_scratch((hipStream_t)stream, 2, bytes);
  launch_gn_stats(SrcView{(const f16*)x, C1, ld1, lo1}, SrcView{(const f16*)x2, C2, ld2, lo2}, B, HW, groups, eps, (const float*)gamma,
                  (const float*)beta, partial, bytes, (float*)scale, (float*)shift, (hipStream_t)stream, nullptr, plan_batch);
  API_END
}
int ldiff_op_gn_stats(const void* x, int C1, int ld1, int lo1, const void* x2, int C2, int ld2, int lo2, int B, int HW, int groups, float eps,
                      const void* gamma, const void* beta, void* scale, void* shift, void* stream) {
  return ldiff_op_gn_stats_pb(x, C1, ld1, lo1, x2, C2, ld2, lo2, B, HW, groups, eps, gamma, beta, scale, shift, 0, stream);
}
int ldiff_op_layernorm(const void* x, int ldx, int x_lo, void* y, int rows, int C, const void* gamma, const void* beta, float eps, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && y && gamma && beta, LDIFF_ERR_INVALID, "op_layernorm: null argument");
  launch_layernorm(SrcView{(const f16*)x, C, ldx, x_lo}, (f16*)y, rows, (const float*)gamma, (const float*)beta, eps, (hipStream_t)stream);
  API_END
}
int ldiff_op_ln_linear(const void* x, int ldx, int x_lo, int rows, int Cc, const void* gamma, const void* beta, float eps, const void* w, int N, int Nrows,
                       const void* bias, int geglu, void* y, int ldy, int qcols, float qscale, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && gamma && beta && w && y && rows >= 0, LDIFF_ERR_INVALID, "op_ln_linear: null argument");
  if (rows == 0) return LDIFF_OK;
  LDIFF_CHECK(lngemm_eligible(Cc, N, ldx ? ldx : Cc, x_lo, ldy, geglu != 0) && Nrows >= N, LDIFF_ERR_INVALID, "op_ln_linear: unsupported shape (C=%d N=%d Nrows=%d)", Cc, N, Nrows);
  // the executors keep the tiled weight copy per layer; this handle-less entry point tiles per call into stream-ordered scratch
  f16* wt = (f16*)op_scratch((hipStream_t)stream, 4, (size_t)N * Cc * sizeof(f16));
  launch_lngemm_tile_weights((const f16*)w, wt, N, Cc, (hipStream_t)stream);
  launch_lngemm((const f16*)x, ldx ? ldx : Cc, x_lo, rows, Cc, (const float*)gamma, (const float*)beta, eps, wt, N, (const float*)bias, geglu != 0,
                (f16*)y, ldy, (hipStream_t)stream, qcols, qscale);
  API_END
}
int ldiff_op_norm_apply(const void* x, int C1, int ld1, int lo1, const void* x2, int C2, int ld2, int lo2, int B, int HW, const void* scale,
                        const void* shift, int silu, void* y, int ldy, int y_lo, void* stream) {
  API_BEGIN
  launch_norm_apply(SrcView{(const f16*)x, C1, ld1, lo1}, SrcView{(const f16*)x2, C2, ld2, lo2}, B, HW, (const float*)scale, (const float*)shift, silu,
                    (f16*)y, ldy, y_lo, 0, (hipStream_t)stream);
  API_END
}
int ldiff_op_norm_apply_lo8(const void* x, int C1, int ld1, int lo1, int B, int HW, const void* scale, const void* shift, int silu, void* y, void* stream) {
  API_BEGIN
  launch_norm_apply(SrcView{(const f16*)x, C1, ld1, lo1}, SrcView{nullptr, 0, 0, 0}, B, HW, (const float*)scale, (const float*)shift, silu,
                    (f16*)y, C1 + C1 / 2, C1, 1, (hipStream_t)stream);
  API_END
}
int ldiff_op_lo8_weights(const void* w, void* wd, void* scale_out, int Nrows, int taps, int Cin, void* stream) {
  API_BEGIN
  launch_lo8_weights((const f16*)w, wd, (int*)scale_out, Nrows, taps, Cin, (hipStream_t)stream);
  API_END
}
int ldiff_op_dup_weights(const void* w, void* wd, int Nrows, int taps, int src_tap_stride, int Ca, int Cb, int dst_tap_stride, void* stream) {
  API_BEGIN
  LDIFF_CHECK(w && wd, LDIFF_ERR_INVALID, "op_dup_weights: null argument");
  launch_dup_weights((const f16*)w, (f16*)wd, Nrows, taps, src_tap_stride, Ca, Cb, dst_tap_stride, (hipStream_t)stream);
  API_END
}
// ---- backward-pass primitives (kernels_bwd.hip) ----
int ldiff_op_im2col_t(const void* x, void* out, int B, int H, int W, int Cc, int ks, int stride, int pad, int ups, int Ho, int Wo, int Mpad, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && out, LDIFF_ERR_INVALID, "op_im2col_t: null argument");
  launch_im2col_t((const f16*)x, (f16*)out, B, H, W, Cc, ks, stride, pad, ups, Ho, Wo, Mpad, (hipStream_t)stream);
  API_END
}
int ldiff_op_transpose(const void* x, void* out, int M, int N, int ldx, int Mpad, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && out, LDIFF_ERR_INVALID, "op_transpose: null argument");
  launch_transpose_rows((const f16*)x, (f16*)out, M, N, ldx, Mpad, (hipStream_t)stream);
  API_END
}
int ldiff_op_colsum(const void* dy, void* db_f32, int M, int N, int ld, void* stream) {
  API_BEGIN
  LDIFF_CHECK(dy && db_f32, LDIFF_ERR_INVALID, "op_colsum: null argument");
  launch_colsum((const f16*)dy, (float*)db_f32, M, N, ld, (hipStream_t)stream);
  API_END
}
int ldiff_op_gn_train_fwd(const void* x, void* y, const void* gamma, const void* beta, void* mean, void* rstd, int B, int HW, int Cc, int groups, float eps,
                          int silu, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && y && gamma && beta && mean && rstd, LDIFF_ERR_INVALID, "op_gn_train_fwd: null argument");
  launch_gn_train_fwd((const f16*)x, (f16*)y, (const float*)gamma, (const float*)beta, (float*)mean, (float*)rstd, B, HW, Cc, groups, eps, silu,
                      (hipStream_t)stream);
  API_END
}
int ldiff_op_gn_train_bwd(const void* x, const void* dy, const void* gamma, const void* beta, const void* mean, const void* rstd, void* dx, void* dgamma,
                          void* dbeta, int B, int HW, int Cc, int groups, int silu, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && dy && gamma && beta && mean && rstd && dx && dgamma && dbeta, LDIFF_ERR_INVALID, "op_gn_train_bwd: null argument");
  launch_gn_train_bwd((const f16*)x, (const f16*)dy, (const float*)gamma, (const float*)beta, (const float*)mean, (const float*)rstd, (f16*)dx,
                      (float*)dgamma, (float*)dbeta, B, HW, Cc, groups, silu, (hipStream_t)stream);
  API_END
}
int ldiff_op_ln_bwd(const void* x, const void* dy, const void* gamma, void* dx, void* dgamma, void* dbeta, int rows, int Cc, float eps, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && dy && gamma && dx && dgamma && dbeta, LDIFF_ERR_INVALID, "op_ln_bwd: null argument");
  launch_ln_bwd((const f16*)x, (const f16*)dy, (const float*)gamma, (f16*)dx, (float*)dgamma, (float*)dbeta, rows, Cc, eps, (hipStream_t)stream);
  API_END
}
int ldiff_op_geglu_bwd(const void* x, const void* dy, void* dx, int64_t M, int C4, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && dy && dx, LDIFF_ERR_INVALID, "op_geglu_bwd: null argument");
  launch_geglu_bwd((const f16*)x, (const f16*)dy, (f16*)dx, M, C4, (hipStream_t)stream);
  API_END
}
int ldiff_op_silu(const void* x, void* y, int64_t n, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && y && n >= 0, LDIFF_ERR_INVALID, "op_silu: bad arguments");
  launch_silu_f16((const f16*)x, (f16*)y, n, (hipStream_t)stream);
  API_END
}
int ldiff_op_silu_bwd(const void* x, const void* dy, void* dx, int64_t n, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && dy && dx && n >= 0, LDIFF_ERR_INVALID, "op_silu_bwd: bad arguments");
  launch_silu_bwd_f16((const f16*)x, (const f16*)dy, (f16*)dx, n, (hipStream_t)stream);
  API_END
}
int ldiff_op_attention_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* dO, int ldo, void* dq, void* dk, void* dv,
                           int B, int heads, int Lq, int Lk, int d, int64_t q_bstride, int64_t kv_bstride, int64_t o_bstride, float scale, void* stream) {
  API_BEGIN
  LDIFF_CHECK(q && k && v && dO && dq && dk && dv && B >= 0 && heads >= 1, LDIFF_ERR_INVALID, "op_attention_bwd: bad arguments");
  AttnParams p;
  p.q = (const f16*)q; p.ldq = ldq; p.k = (const f16*)k; p.ldk = ldk; p.v = (const f16*)v; p.ldv = ldv; p.o = nullptr; p.ldo = ldo;
  p.B = B; p.heads = heads; p.Lq = Lq; p.Lk = Lk; p.d = d;
  p.q_bstride = q_bstride; p.kv_bstride = kv_bstride; p.o_bstride = o_bstride; p.scale = scale;
  launch_attn_bwd(p, (const f16*)dO, (f16*)dq, (f16*)dk, (f16*)dv, (hipStream_t)stream);
  API_END
}
int ldiff_op_adamw(void* p, const void* g, void* m, void* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   void* stream) {
  API_BEGIN
  LDIFF_CHECK(p && g && m && v && n >= 0, LDIFF_ERR_INVALID, "op_adamw: bad arguments");
  launch_adamw((float*)p, (const float*)g, (float*)m, (float*)v, n, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
  API_END
}
int ldiff_op_infonce(const void* features, int B, int n, int64_t HW, const void* bi, const void* ai, const void* pi, const void* ni, int T, const void* T_dev,
                     int K, float temperature, void* loss, void* dfeatures, void* stream) {
  API_BEGIN
  LDIFF_CHECK(features && loss && dfeatures && B >= 1 && HW >= 1 && T >= 0 && (T == 0 || (bi && ai && pi && ni)), LDIFF_ERR_INVALID, "op_infonce: bad arguments");
  launch_infonce((const float*)features, B, n, HW, (const int*)bi, (const int*)ai, (const int*)pi, (const int*)ni, T, (const int*)T_dev, K, temperature, (float*)loss,
                 (float*)dfeatures, (hipStream_t)stream);
  API_END
}
int ldiff_op_pack_weight(const void* w_f32, void* dst_f16, int Cout, int Cin, int k, int rows, int Cpad, int mode, void* stream) {
  API_BEGIN
  LDIFF_CHECK(w_f32 && dst_f16 && Cout >= 1 && Cin >= 1 && (k == 1 || k == 3) && (mode == 0 || mode == 1) && rows >= (mode ? Cin : Cout) &&
                  Cpad >= (mode ? Cout : Cin) && Cpad % 2 == 0, LDIFF_ERR_INVALID, "op_pack_weight: bad arguments (Cpad must be even and cover the channels)");
  launch_pack_weight((const float*)w_f32, (f16*)dst_f16, Cout, Cin, k, rows, Cpad, mode, (hipStream_t)stream);
  API_END
}
int ldiff_op_pack_weight_multi(const void* entries, const void* tile_prefix, int n_entries, int n_tiles, void* stream) {
  API_BEGIN
  LDIFF_CHECK(n_entries >= 0 && n_tiles >= 0 && (n_entries == 0 || (entries && tile_prefix)), LDIFF_ERR_INVALID, "op_pack_weight_multi: bad arguments");
  launch_pack_weight_multi((const PackEntry*)entries, (const int*)tile_prefix, n_entries, n_tiles, (hipStream_t)stream);
  API_END
}
int ldiff_op_unpack_wgrad(const void* g_f32, void* dw_f32, int Cout, int Cin, int k, int Cx, int ldg, void* stream) {
  API_BEGIN
  LDIFF_CHECK(g_f32 && dw_f32 && Cout >= 1 && Cin >= 1 && (k == 1 || k == 3) && Cx >= Cin && ldg >= k * k * Cx, LDIFF_ERR_INVALID, "op_unpack_wgrad: bad arguments");
  launch_unpack_wgrad((const float*)g_f32, (float*)dw_f32, Cout, Cin, k, Cx, ldg, (hipStream_t)stream);
  API_END
}
int ldiff_op_adamw_multi(const void* tensors, const void* grads, const void* chunks, int64_t nchunks, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int step, void* stream) {
  API_BEGIN
  LDIFF_CHECK(nchunks >= 0 && (nchunks == 0 || (tensors && grads && chunks)), LDIFF_ERR_INVALID, "op_adamw_multi: bad arguments");
  launch_adamw_multi((const AdamTensor*)tensors, (const float* const*)grads, (const AdamChunk*)chunks, nchunks, lr, beta1, beta2, eps, weight_decay, step,
                     (hipStream_t)stream);
  API_END
}
// ---- training form of the nnU-Net tissue head (kernels_segtrain.hip) ----
int64_t ldiff_op_in_train_ws_bytes(int B, int HW, int Cc) {
  if (B < 1 || HW < 1 || Cc < 8 || Cc % 8 != 0) return 0;
  return in_train_ws_floats(B, HW, Cc) * 4;
}
int ldiff_op_in_train_fwd(const void* x, void* y, const void* gamma, const void* beta, void* mean, void* rstd, int B, int HW, int Cc, float eps, float slope,
                          void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && y && gamma && beta && mean && rstd && ws, LDIFF_ERR_INVALID, "op_in_train_fwd: null argument");
  launch_in_train_fwd((const f16*)x, (f16*)y, (const float*)gamma, (const float*)beta, (float*)mean, (float*)rstd, B, HW, Cc, eps, slope, (float*)ws, ws_bytes,
                      (hipStream_t)stream);
  API_END
}
int ldiff_op_in_train_bwd(const void* x, const void* dy, const void* gamma, const void* beta, const void* mean, const void* rstd, void* dx, void* dgamma,
                          void* dbeta, int B, int HW, int Cc, float slope, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && dy && gamma && beta && mean && rstd && dx && dgamma && dbeta && ws, LDIFF_ERR_INVALID, "op_in_train_bwd: null argument");
  launch_in_train_bwd((const f16*)x, (const f16*)dy, (const float*)gamma, (const float*)beta, (const float*)mean, (const float*)rstd, (f16*)dx, (float*)dgamma,
                      (float*)dbeta, B, HW, Cc, slope, (float*)ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_dice_ce_ws_bytes(int B, int64_t HW, int n_heads) {
  if (B < 1 || HW < 1 || n_heads < 2 || n_heads > 32) return 0;
  return dice_ce_ws_bytes(B, HW, n_heads, false);
}
int ldiff_op_dice_ce(const void* logits, int ld, int n_heads, const void* target, int target_i64, int B, int64_t HW, int batch_dice, float smooth, float weight,
                     float grad_scale, void* loss, void* dlogits, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && target && loss && dlogits && ws, LDIFF_ERR_INVALID, "op_dice_ce: null argument");
  launch_dice_ce((const f16*)logits, ld, n_heads, std::nullopt, target, target_i64, B, HW, batch_dice, smooth, weight, grad_scale, (float*)loss, (f16*)dlogits, ws,
                 ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_dice_ce_stats(const void* logits, int ld, int n_heads, const void* target, int target_i64, int B, int64_t HW, int batch_dice, void* sums, void* ws,
                           int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && target && sums && ws, LDIFF_ERR_INVALID, "op_dice_ce_stats: null argument");
  launch_dice_ce_stats((const f16*)logits, ld, n_heads, std::nullopt, target, target_i64, B, HW, batch_dice, (double*)sums, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_dice_ce_from_sums(const void* logits, int ld, int n_heads, const void* target, int target_i64, int B, int64_t HW, int batch_dice, float smooth,
                               float weight, float grad_scale, const void* dice_sums, const void* local_sums, int world, void* loss, void* dlogits, void* ws,
                               int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && target && dice_sums && local_sums && loss && dlogits && ws, LDIFF_ERR_INVALID, "op_dice_ce_from_sums: null argument");
  launch_dice_ce_from_sums((const f16*)logits, ld, n_heads, std::nullopt, target, target_i64, B, HW, batch_dice, smooth, weight, grad_scale,
                           (const double*)dice_sums, (const double*)local_sums, world, (float*)loss, (f16*)dlogits, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_dice_ce_ignore_ws_bytes(int B, int64_t HW, int n_heads) {
  if (B < 1 || HW < 1 || n_heads < 2 || n_heads > 32) return 0;
  return dice_ce_ws_bytes(B, HW, n_heads, true);
}
int ldiff_op_dice_ce_ignore_nacc(int n_heads) { return (n_heads < 2 || n_heads > 32) ? 0 : dice_ce_nacc(n_heads, true); }
int ldiff_op_dice_ce_ignore(const void* logits, int ld, int n_heads, int ignore_label, const void* target, int target_i64, int B, int64_t HW, int batch_dice,
                            float smooth, float weight, float grad_scale, void* loss, void* dlogits, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && target && loss && dlogits && ws, LDIFF_ERR_INVALID, "op_dice_ce_ignore: null argument");
  launch_dice_ce((const f16*)logits, ld, n_heads, ignore_label, target, target_i64, B, HW, batch_dice, smooth, weight, grad_scale, (float*)loss, (f16*)dlogits, ws,
                 ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_dice_ce_ignore_stats(const void* logits, int ld, int n_heads, int ignore_label, const void* target, int target_i64, int B, int64_t HW, int batch_dice,
                                  void* sums, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && target && sums && ws, LDIFF_ERR_INVALID, "op_dice_ce_ignore_stats: null argument");
  launch_dice_ce_stats((const f16*)logits, ld, n_heads, ignore_label, target, target_i64, B, HW, batch_dice, (double*)sums, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_dice_ce_ignore_from_sums(const void* logits, int ld, int n_heads, int ignore_label, const void* target, int target_i64, int B, int64_t HW,
                                      int batch_dice, float smooth, float weight, float grad_scale, const void* sums, void* loss, void* dlogits, void* ws,
                                      int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && target && sums && loss && dlogits && ws, LDIFF_ERR_INVALID, "op_dice_ce_ignore_from_sums: null argument");
  // one process: the Dice sums are the local ones (the data-parallel exchange of the ignore form is not built)
  launch_dice_ce_from_sums((const f16*)logits, ld, n_heads, ignore_label, target, target_i64, B, HW, batch_dice, smooth, weight, grad_scale, (const double*)sums,
                           (const double*)sums, 1, (float*)loss, (f16*)dlogits, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_dice_focal_ws_bytes(int B, int64_t HW, int n_regions) {
  if (B < 1 || HW < 1 || n_regions < 1 || n_regions > 24) return 0;
  return dice_focal_ws_bytes(B, HW, n_regions);
}
int ldiff_op_dice_focal_nacc(int n_regions) { return (n_regions < 1 || n_regions > 24) ? 0 : dice_focal_nacc(n_regions); }
int ldiff_op_dice_focal(const void* logits, int ld, int n_regions, const void* table, const void* target, int target_i64, int use_ignore, int bce, int B, int64_t HW,
                        int batch_dice, float smooth, float weight, float grad_scale, void* loss, void* dlogits, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && table && target && loss && dlogits && ws, LDIFF_ERR_INVALID, "op_dice_focal: null argument");
  launch_dice_focal((const f16*)logits, ld, n_regions, (const unsigned*)table, target, target_i64, use_ignore, bce, B, HW, batch_dice, smooth, weight, grad_scale,
                    (float*)loss, (f16*)dlogits, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_dice_focal_stats(const void* logits, int ld, int n_regions, const void* table, const void* target, int target_i64, int use_ignore, int bce, int B,
                              int64_t HW, int batch_dice, void* sums, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && table && target && sums && ws, LDIFF_ERR_INVALID, "op_dice_focal_stats: null argument");
  launch_dice_focal_stats((const f16*)logits, ld, n_regions, (const unsigned*)table, target, target_i64, use_ignore, bce, B, HW, batch_dice, (double*)sums, ws, ws_bytes,
                          (hipStream_t)stream);
  API_END
}
int ldiff_op_dice_focal_from_sums(const void* logits, int ld, int n_regions, const void* table, const void* target, int target_i64, int use_ignore, int bce, int B,
                                  int64_t HW, int batch_dice, float smooth, float weight, float grad_scale, const void* dice_sums, const void* local_sums, int world,
                                  void* loss, void* dlogits, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && table && target && dice_sums && local_sums && loss && dlogits && ws, LDIFF_ERR_INVALID, "op_dice_focal_from_sums: null argument");
  launch_dice_focal_from_sums((const f16*)logits, ld, n_regions, (const unsigned*)table, target, target_i64, use_ignore, bce, B, HW, batch_dice, smooth, weight,
                              grad_scale, (const double*)dice_sums, (const double*)local_sums, world, (float*)loss, (f16*)dlogits, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_region_counts_ws_bytes(int B, int64_t HW, int n_regions) {
  if (B < 1 || HW < 1 || n_regions < 1 || n_regions > 24) return 0;
  return region_counts_ws_bytes(B, HW, n_regions);
}
int ldiff_op_region_counts(const void* logits, int ld, int n_regions, const void* table, const void* target, int target_i64, int B, int64_t HW, float threshold,
                           void* counts, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && table && target && counts && ws, LDIFF_ERR_INVALID, "op_region_counts: null argument");
  launch_region_counts((const f16*)logits, ld, n_regions, (const unsigned*)table, target, target_i64, B, HW, threshold, (long long*)counts, ws, ws_bytes,
                       (hipStream_t)stream);
  API_END
}
int ldiff_op_region_mask_u8(const void* logits, int logits_f32, int n_regions, int H, int W, const int* regions_class_order, float threshold, void* mask, int mask_H,
                            int mask_W, int mask_y0, int mask_x0, void* stream) {
  API_BEGIN
  LDIFF_CHECK(logits && regions_class_order && mask, LDIFF_ERR_INVALID, "op_region_mask_u8: null argument");
  launch_region_mask_u8(logits, logits_f32, n_regions, H, W, regions_class_order, threshold, (uint8_t*)mask, mask_H, mask_W, mask_y0, mask_x0, (hipStream_t)stream);
  API_END
}
// ---- connected components and the largest-component filter (kernels_segpost.hip) ----
int64_t ldiff_op_keep_largest_component_ws_bytes(int N, int H, int W) { return keep_largest_component_ws_bytes(N, H, W); }
int ldiff_op_keep_largest_component(const void* seg_in, void* seg_out, int N, int H, int W, const void* table, int background_label, void* ws, int64_t ws_bytes,
                                    void* stream) {
  API_BEGIN
  launch_keep_largest_component((const uint8_t*)seg_in, (uint8_t*)seg_out, N, H, W, (const uint8_t*)table, background_label, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_cc_label(const void* seg, int N, int H, int W, const void* table, void* labels_i32, void* sizes_i32, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  launch_cc_label((const uint8_t*)seg, N, H, W, (const uint8_t*)table, (int*)labels_i32, (int*)sizes_i32, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_bucket_pack(const void* grads, const void* offsets, const void* chunks, int64_t nchunks, void* bucket, void* stream) {
  API_BEGIN
  LDIFF_CHECK(nchunks >= 0 && (nchunks == 0 || (grads && offsets && chunks && bucket)), LDIFF_ERR_INVALID, "op_bucket_pack: bad arguments");
  launch_bucket_pack((const float* const*)grads, (const long long*)offsets, (const AdamChunk*)chunks, nchunks, (float*)bucket, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_sumsq_ws_bytes(int64_t n) { return sumsq_ws_bytes(n); }
int ldiff_op_sumsq(const void* x, int64_t n, void* out_f32, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && out_f32 && ws, LDIFF_ERR_INVALID, "op_sumsq: null argument");
  launch_sumsq((const float*)x, n, (float*)out_f32, (float*)ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_sgd_nesterov_multi(const void* tensors, const void* grads, const void* chunks, int64_t nchunks, float lr, float momentum, float weight_decay,
                                int first, const void* inv_scale, const void* clip_coef, void* stream) {
  API_BEGIN
  LDIFF_CHECK(nchunks >= 0 && inv_scale && clip_coef && (nchunks == 0 || (tensors && grads && chunks)), LDIFF_ERR_INVALID, "op_sgd_nesterov_multi: bad arguments");
  launch_sgd_nesterov_multi((const SgdTensor*)tensors, (const float* const*)grads, (const AdamChunk*)chunks, nchunks, lr, momentum, weight_decay, first,
                            (const float*)inv_scale, (const float*)clip_coef, (hipStream_t)stream);
  API_END
}
// ---- direct weight / bias gradients of the tissue head's convs (kernels_wgrad.hip) ----
int64_t ldiff_op_conv_wgrad_ws_bytes(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) { return conv_wgrad_ws_bytes(B, Ho, Wo, Cx, Cy, k, wgs); }
int ldiff_op_conv_wgrad(const void* x, const void* dy, void* dw_f32, int B, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout, int Cin, int k, int stride, int wgs,
                        void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x, LDIFF_ERR_INVALID, "op_conv_wgrad: null argument x");
  LDIFF_CHECK(dy, LDIFF_ERR_INVALID, "op_conv_wgrad: null argument dy");
  LDIFF_CHECK(dw_f32, LDIFF_ERR_INVALID, "op_conv_wgrad: null argument dw_f32");
  LDIFF_CHECK(ws, LDIFF_ERR_INVALID, "op_conv_wgrad: null argument ws");
  launch_conv_wgrad((const f16*)x, (const f16*)dy, (float*)dw_f32, B, H, W, Cx, Ho, Wo, Cy, Cout, Cin, k, stride, wgs, (float*)ws, ws_bytes, (hipStream_t)stream);
  API_END
}
// the wide convs: both channel counts blocked (the same kernel of kernels_wgrad.hip under the wide entry's limits and plan)
int64_t ldiff_op_conv_wgrad_wide_ws_bytes(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs) { return conv_wgrad_wide_ws_bytes(B, Ho, Wo, Cx, Cy, k, wgs); }
int ldiff_op_conv_wgrad_wide(const void* x, const void* dy, void* dw_f32, int B, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout, int Cin, int k, int stride,
                             int wgs, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x, LDIFF_ERR_INVALID, "op_conv_wgrad_wide: null argument x");
  LDIFF_CHECK(dy, LDIFF_ERR_INVALID, "op_conv_wgrad_wide: null argument dy");
  LDIFF_CHECK(dw_f32, LDIFF_ERR_INVALID, "op_conv_wgrad_wide: null argument dw_f32");
  LDIFF_CHECK(ws, LDIFF_ERR_INVALID, "op_conv_wgrad_wide: null argument ws");
  launch_conv_wgrad_wide((const f16*)x, (const f16*)dy, (float*)dw_f32, B, H, W, Cx, Ho, Wo, Cy, Cout, Cin, k, stride, wgs, (float*)ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_colsum_slabs_ws_bytes(int64_t M, int N) { return colsum_slabs_ws_bytes(M, N); }
int ldiff_op_colsum_slabs(const void* dy, void* db_f32, int64_t M, int N, int ld, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  LDIFF_CHECK(dy, LDIFF_ERR_INVALID, "op_colsum_slabs: null argument dy");
  LDIFF_CHECK(db_f32, LDIFF_ERR_INVALID, "op_colsum_slabs: null argument db_f32");
  LDIFF_CHECK(ws, LDIFF_ERR_INVALID, "op_colsum_slabs: null argument ws");
  launch_colsum_slabs((const f16*)dy, (float*)db_f32, M, N, ld, (float*)ws, ws_bytes, (hipStream_t)stream);
  API_END
}
// ---- training data of the tissue head (kernels_segaug.hip) ----
int ldiff_op_seg_sample(const void* arena, int64_t arena_bytes, const ldiff_seg_case* cases, int n_cases, const ldiff_seg_sample* samples, int B, int Cc, int h,
                        int w, int n_scales, void* data, void* target, void* stream) {
  API_BEGIN
  launch_seg_sample(arena, arena_bytes, cases, n_cases, samples, B, Cc, h, w, n_scales, (float*)data, (uint8_t*)target, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_seg_intensity_ws_bytes(int B, int Cc, int h, int w) {
  if (B < 1 || Cc < 1 || h < 1 || w < 1) return 0;
  return seg_intensity_ws_bytes(B, Cc, h, w);
}
int ldiff_op_seg_intensity(void* data, const ldiff_seg_sample* samples, const ldiff_seg_chan* chans, int B, int Cc, int h, int w, const void* normal_or_null,
                           uint64_t seed, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  launch_seg_intensity((float*)data, samples, chans, B, Cc, h, w, (const float*)normal_or_null, seed, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_seg_intensity_lr_ws_bytes(int B, int Cc, int h, int w) {
  if (B < 1 || Cc < 1 || h < 1 || w < 1) return 0;
  return seg_intensity_lr_ws_bytes(B, Cc, h, w);
}
int ldiff_op_seg_intensity_lr(void* data, const ldiff_seg_sample* samples, const ldiff_seg_chan* chans, int B, int Cc, int h, int w, const void* normal_or_null,
                              uint64_t seed, void* ws, int64_t ws_bytes, void* stream) {
  API_BEGIN
  launch_seg_intensity((float*)data, samples, chans, B, Cc, h, w, (const float*)normal_or_null, seed, ws, ws_bytes, (hipStream_t)stream, true);
  API_END
}
int ldiff_op_spline_prefilter(void* planes_f32, int n_planes, int H, int W, int stride, void* stream) {
  API_BEGIN
  launch_spline_prefilter((float*)planes_f32, n_planes, H, W, stride, (hipStream_t)stream);
  API_END
}
// ---- plan and preprocess of the tissue head's cases (kernels_segprep.hip) ----
int ldiff_op_case_bbox(const void* img, int dtype, int Cc, int H, int W, int64_t row_stride, int64_t plane_stride, int32_t* box, void* stream) {
  API_BEGIN
  launch_case_bbox(img, dtype, Cc, H, W, row_stride, plane_stride, box, (hipStream_t)stream);
  API_END
}
int64_t ldiff_op_case_stats_ws_bytes(int Cc) { return case_stats_ws_bytes(Cc); }
int ldiff_op_case_stats(const void* img, int dtype, int Cc, int H, int W, int64_t row_stride, int64_t plane_stride, int y0, int y1, int x0, int x1, void* stats, void* ws,
                        int64_t ws_bytes, void* stream) {
  API_BEGIN
  launch_case_stats(img, dtype, Cc, H, W, row_stride, plane_stride, y0, y1, x0, x1, stats, ws, ws_bytes, (hipStream_t)stream);
  API_END
}
int ldiff_op_case_counts(const void* label_u8, int H, int W, int64_t label_stride, int y0, int y1, int x0, int x1, int n_heads, uint32_t* row_counts, uint32_t* row_prefix,
                         uint32_t* totals, void* stream) {
  API_BEGIN
  launch_case_counts(label_u8, H, W, label_stride, y0, y1, x0, x1, n_heads, 0, row_counts, row_prefix, totals, (hipStream_t)stream);
  API_END
}
int ldiff_op_case_counts_classes(const void* label_u8, int H, int W, int64_t label_stride, int y0, int y1, int x0, int x1, int n_heads, int n_classes,
                                 uint32_t* row_counts, uint32_t* row_prefix, uint32_t* totals, void* stream) {
  API_BEGIN
  LDIFF_CHECK(n_classes >= 1, LDIFF_ERR_INVALID, "op_case_counts_classes: n_classes %d below 1", n_classes);
  launch_case_counts(label_u8, H, W, label_stride, y0, y1, x0, x1, n_heads, n_classes, row_counts, row_prefix, totals, (hipStream_t)stream);
  API_END
}
int ldiff_op_case_apply(const void* img, int dtype, int Cc, int H, int W, int64_t row_stride, int64_t plane_stride, const void* label_u8, int64_t label_stride, int y0, int y1,
                        int x0, int x1, const float* sub, const float* div, void* arena, int64_t arena_bytes, const ldiff_seg_case* row, int write_coef, void* stream) {
  API_BEGIN
  launch_case_apply(img, dtype, Cc, H, W, row_stride, plane_stride, label_u8, label_stride, y0, y1, x0, x1, sub, div, arena, arena_bytes, row, write_coef, (hipStream_t)stream);
  API_END
}
int ldiff_op_case_rank_to_coord(const void* label_u8, int H, int W, int64_t label_stride, int y0, int y1, int x0, int x1, int selector, const uint32_t* row_prefix,
                                const int64_t* ranks, int64_t n, int32_t* coords, const void* img_or_null, int dtype, int Cc, int64_t row_stride, int64_t plane_stride,
                                void* values_or_null, void* stream) {
  API_BEGIN
  launch_case_rank_to_coord(label_u8, H, W, label_stride, y0, y1, x0, x1, selector, row_prefix, (const long long*)ranks, n, coords, img_or_null, dtype, Cc, row_stride,
                            plane_stride, values_or_null, (hipStream_t)stream);
  API_END
}
int ldiff_op_geglu(const void* x, void* y, int64_t M, int C4, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x && y, LDIFF_ERR_INVALID, "op_geglu: null argument");
  launch_geglu((const f16*)x, (f16*)y, M, C4, (hipStream_t)stream);
  API_END
}
int ldiff_op_nchw_to_nhwc(const void* x_f32, void* y_f16, int B, int C, int H, int W, int Cpad, int lo_off, void* stream) {
  API_BEGIN
  LDIFF_CHECK(x_f32 && y_f16, LDIFF_ERR_INVALID, "op_nchw_to_nhwc: null argument");
  launch_nchw_f32_to_nhwc_f16((const float*)x_f32, (f16*)y_f16, B, C, H, W, Cpad, (hipStream_t)stream, lo_off);
  API_END
}

}  // extern "C"
