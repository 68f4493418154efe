// ldiff_textenc: the CLIP text encoder of the prompt path (include/ldiff.h) -- transformers' CLIPTextModel up to last_hidden_state, plus the optional prompt
// projection.  Executor over the same Exec / plan_conv / GraphCache as the other graphs; kernels of its own in kernels_text.hip.
//
// One pass at (B, L), M = B L rows, per layer 7 launches (more where plan_conv splits K: each split GEMM adds its reduce):
//   text_embed                                      ids -> x (split hi | lo)
//   per layer:  text_ln (LN1)                       -> n   split
//               GEMM q/k/v fused (+bias)            -> qkv [M, 3 hidden] fp16      the attention kernel's operands
//               text_attn<d>                        -> a   split                   causal, whole-row fp32 softmax
//               GEMM out_proj (+bias, +x, split out) -> x
//               text_ln (LN2)                       -> n   split
//               GEMM fc1 (+bias, quick_gelu | gelu) -> f   split                   act_out epilogue
//               GEMM fc2 (+bias, +x, split out)     -> x
//   text_ln (final)                                 -> last_hidden_state fp32 | fp16, or the split operand of
//   GEMM proj (fp32 out) [+ f32_to_f16]             -> [M, cross_attention_dim]   (project = 1)
// Every GEMM contracts a split activation read as [hi | lo | hi] (two sources over one buffer) against [wh | wh | wl]: fp16 MFMA operands, but neither the
// activation's nor the weight's fp16 rounding enters the sum.  With single fp16 operands the encoder missed 1e-3 of max |ref| against fp32 transformers (the weights'
// rounding alone is 6e-4 .. 8e-4 after 2-3 layers: DESIGN.md section 7); what is left is the rounding of q, k, v and of the probabilities inside the attention.
// The GEMM rows are M = 5, 20, 77, 231, ...: the LDS-DMA GEMM clamps the rows of its last tile (kernels_gemm.hip), as for ldiff_unet_set_context's L = 77
// projections, so no buffer is padded.
#include <string.h>

#include <algorithm>

#include "model.h"

void ldiff_textenc::build() {
  const ldiff_textenc_cfg& c = cfg;
  LDIFF_CHECK(c.vocab_size >= 1 && c.vocab_size <= (1 << 20), LDIFF_ERR_INVALID, "textenc_create: vocab_size = %d outside 1..2^20", c.vocab_size);
  LDIFF_CHECK(c.heads >= 1 && c.hidden >= 64 && c.hidden <= 2048 && c.hidden % 64 == 0 && c.hidden % c.heads == 0, LDIFF_ERR_INVALID,
              "textenc_create: hidden = %d must be a multiple of 64 in 64..2048 and of heads = %d", c.hidden, c.heads);
  const int d = c.hidden / c.heads;
  LDIFF_CHECK(d % 16 == 0 && d <= 128, LDIFF_ERR_INVALID, "textenc_create: head dim %d (hidden / heads) must be a multiple of 16 up to 128", d);
  LDIFF_CHECK(c.intermediate >= 64 && c.intermediate <= 16384 && c.intermediate % 64 == 0, LDIFF_ERR_INVALID, "textenc_create: intermediate = %d must be a multiple of 64 in 64..16384 (FC2 on the LDS-DMA GEMM)", c.intermediate);
  LDIFF_CHECK(c.layers >= 1 && c.layers <= 64, LDIFF_ERR_INVALID, "textenc_create: layers = %d outside 1..64", c.layers);
  LDIFF_CHECK(c.max_positions >= 1 && c.max_positions <= 128, LDIFF_ERR_INVALID, "textenc_create: max_positions = %d outside 1..128", c.max_positions);
  LDIFF_CHECK(c.act == 0 || c.act == 1, LDIFF_ERR_INVALID, "textenc_create: act = %d must be 0 (quick_gelu) or 1 (gelu)", c.act);
  LDIFF_CHECK(c.ln_eps > 0.f && c.ln_eps < 1.f, LDIFF_ERR_INVALID, "textenc_create: ln_eps = %g outside (0, 1)", (double)c.ln_eps);
  nf.create();
  ws.who = "textenc_load";
  ex.weights_gen = &ws.generation;
  ex.nonfinite = nf.words;
  ex.trace_tag = "textenc";
  const int H = c.hidden;
  // the two tables stay fp32: the embedding sum is the reference's, to fp32 round-off
  tok = ws.alloc_vec((size_t)c.vocab_size * H);
  pos = ws.alloc_vec((size_t)c.max_positions * H);
  ws.add_tensor("text_model.embeddings.token_embedding.weight", {c.vocab_size, H}, tok);
  ws.add_tensor("text_model.embeddings.position_embedding.weight", {c.max_positions, H}, pos);
  layers.resize(c.layers);
  for (int i = 0; i < c.layers; ++i) {
    const std::string p = "text_model.encoder.layers." + std::to_string(i);
    TextLayerW& l = layers[i];
    l.ln1 = ws.add_norm(p + ".layer_norm1", H);
    l.qkv = add_lin("", H, 3 * H);   // fused q/k/v, rows in that order
    add_part(l.qkv, p + ".self_attn.q_proj", 0, H);
    add_part(l.qkv, p + ".self_attn.k_proj", H, H);
    add_part(l.qkv, p + ".self_attn.v_proj", 2 * H, H);
    l.out = add_lin(p + ".self_attn.out_proj", H, H);
    l.ln2 = ws.add_norm(p + ".layer_norm2", H);
    l.fc1 = add_lin(p + ".mlp.fc1", H, c.intermediate);
    l.fc2 = add_lin(p + ".mlp.fc2", c.intermediate, H);
  }
  final_ln = ws.add_norm("text_model.final_layer_norm", H);
}

// a linear layer's three-block operand and bias; with a prefix, its one checkpoint matrix
TextLinW ldiff_textenc::add_lin(const std::string& prefix, int K, int N) {
  TextLinW l;
  l.N = N; l.Nrows = (N + 15) / 16 * 16; l.K = K;
  l.w3 = ws.alloc_mat(l.Nrows, 3 * K);
  l.b = ws.alloc_vec(l.Nrows);
  if (!prefix.empty()) add_part(l, prefix, 0, N);
  return l;
}
void ldiff_textenc::add_part(TextLinW& l, const std::string& prefix, int row_off, int rows) {
  ws.add_rows3(prefix + ".weight", prefix + ".bias", l.w3, l.K, row_off, rows, l.b);
}

// the one step of a load that is the text encoder's own: the optional prompt projection is registered by its first tensor, which states the width
void ldiff_textenc::load(const char* name_c, const void* host, int dtype, const int64_t* shape, int ndim) {
  const std::string name(name_c ? name_c : "");
  if ((name == "proj.weight" || name == "proj.bias") && proj_dim == 0) {
    const bool is_w = name == "proj.weight";
    ws.check_tensor(name_c, host, dtype, shape, ndim);
    LDIFF_CHECK(is_w ? (ndim == 2 && shape[1] == cfg.hidden) : ndim == 1, LDIFF_ERR_INVALID, "textenc_load(%s): expected %s", name_c, is_w ? "[cross_attention_dim, hidden]" : "[cross_attention_dim]");
    LDIFF_CHECK(shape[0] >= 8 && shape[0] <= 8192 && shape[0] % 8 == 0, LDIFF_ERR_INVALID, "textenc_load(%s): cross_attention_dim = %lld must be a multiple of 8 in 8..8192", name_c, (long long)shape[0]);
    // dtype, rank and both extents are checked above, so the load below cannot refuse the tensor that registered the projection
    proj = add_lin("proj", cfg.hidden, (int)shape[0]);
    proj_dim = (int)shape[0];
  }
  ws.load(name_c, host, dtype, shape, ndim);
}

Act ldiff_textenc::layernorm(const Act& x, const NormW& w) {
  Act y = ex.new_act(x.B, x.H, x.W, x.C, true);
  launch_text_ln(x.p, (int)x.rows(), x.C, w.g, w.b, cfg.ln_eps, nullptr, 0, y.p, nullptr, ex.s);
  return y;
}

Act ldiff_textenc::linear(const TextLinW& w, const Act& x, const Act* res, bool split_out, int act_out, float* out_f32) {
  LDIFF_CHECK(x.split && !x.lo8 && x.C == w.K, LDIFF_ERR_INVALID, "textenc linear: input has %d channels, weight expects %d", x.C, w.K);
  const int M = (int)x.rows();
  ConvParams p;
  memset(&p, 0, sizeof(p));
  p.x = x.p; p.C1 = 2 * w.K; p.ld1 = 2 * w.K;   // hi | lo
  p.x2 = x.p; p.C2 = w.K; p.ld2 = 2 * w.K;       // hi again, against wl
  p.B = 1; p.Hin = 1; p.Win = M; p.Hout = 1; p.Wout = M; p.ks = 1; p.stride = 1;
  p.w = w.w3; p.N = w.N; p.Nrows = w.Nrows; p.K = 3 * w.K; p.bias = w.b; p.M = M;
  p.act_out = act_out;
  p.df_force = -1;   // (no fragment-packed copy of these operands for the dataflow GEMM)
  if (res) {
    LDIFF_CHECK(res->rows() == M && res->C == w.N && res->split, LDIFF_ERR_INVALID, "textenc linear: residual shape mismatch");
    p.res = res->p; p.ld_res = res->ld(); p.res_lo = res->lo();
  }
  Act y;
  if (out_f32) { p.y = out_f32; p.ldy = w.N; p.out_f32 = 1; }
  else {
    y = ex.new_act(1, 1, M, w.N, split_out);
    p.y = y.p; p.ldy = y.ld(); p.y_lo = y.lo();
  }
  ConvAsk ask;
  const ConvPlan pl = plan_conv(p, ask);
  if (p.splitk) p.splitk_ws = ex.tmp<float>((size_t)p.splitk * M * p.N);
  launch_igemm(p, pl, ex.s);
  if (p.splitk_ws) ex.arena.free(p.splitk_ws);   // stream-ordered reuse
  return y;
}

void ldiff_textenc::forward_impl(const int* ids, int B, int L, int project, void* out, int out_dtype, hipStream_t s) {
  HIP_CHECK(hipSetDevice(device));
  const int H = cfg.hidden, I = cfg.intermediate, M = B * L, heads = cfg.heads, d = H / heads;
  ex.s = s;
  ex.arena.reset();
  // live at once, at most: two split streams, a normalised copy, q/k/v or the FC1 output, and the fp32 partials of a split GEMM (<= 16 splits)
  const size_t widest = (size_t)std::max(std::max(3 * H, I), proj_dim);
  ex.arena.reserve((size_t)M * ((size_t)12 * H + 2 * widest) * sizeof(f16) + (size_t)16 * M * widest * sizeof(float) + (size_t)M * widest * sizeof(float) + (4u << 20));
  const float scale = 1.0f / sqrtf((float)d);

  Act x = ex.new_act(1, 1, M, H, true);
  launch_text_embed(ids, tok, pos, x.p, M, L, H, cfg.vocab_size, s);
  ex.trace("embeddings", x);
  for (int li = 0; li < cfg.layers; ++li) {
    const TextLayerW& l = layers[li];
    Act n = layernorm(x, l.ln1);
    Act qkv = linear(l.qkv, n, nullptr, false, 0, nullptr);
    ex.release(n);
    Act a = ex.new_act(1, 1, M, H, true);
    launch_text_attention(qkv.p, qkv.ld(), H, a.p, a.ld(), a.lo(), B, heads, L, d, scale, s);
    ex.release(qkv);
    Act x1 = linear(l.out, a, &x, true, 0, nullptr);
    ex.release(a);
    ex.release(x);
    n = layernorm(x1, l.ln2);
    Act f = linear(l.fc1, n, nullptr, true, cfg.act == 0 ? 1 : 2, nullptr);
    ex.release(n);
    x = linear(l.fc2, f, &x1, true, 0, nullptr);
    ex.release(f);
    ex.release(x1);
    ex.trace(("layer" + std::to_string(li)).c_str(), x);
  }
  if (!project) {
    launch_text_ln(x.p, M, H, final_ln.g, final_ln.b, cfg.ln_eps, out, out_dtype == LDIFF_F16, nullptr, ex.nonfinite, s);
  } else {
    Act y = ex.new_act(1, 1, M, H, true);
    launch_text_ln(x.p, M, H, final_ln.g, final_ln.b, cfg.ln_eps, nullptr, 0, y.p, ex.nonfinite, s);
    float* o32 = out_dtype == LDIFF_F16 ? ex.tmp<float>((size_t)M * proj_dim) : (float*)out;
    linear(proj, y, nullptr, false, 0, o32);
    ex.release(y);
    if (out_dtype == LDIFF_F16) {
      launch_f32_to_f16(o32, (f16*)out, (long long)M * proj_dim, s);
      ex.arena.free(o32);
    }
  }
  ex.release(x);
}

void ldiff_textenc::forward(const int32_t* ids_host, int B, int L, int project, void* out, int out_dtype, hipStream_t s) {
  LDIFF_CHECK(ids_host && out, LDIFF_ERR_INVALID, "textenc_forward: null pointer");
  LDIFF_CHECK(B >= 1 && B <= 4096, LDIFF_ERR_INVALID, "textenc_forward: B = %d outside 1..4096", B);
  LDIFF_CHECK(L >= 1 && L <= cfg.max_positions, LDIFF_ERR_INVALID, "textenc_forward: L = %d outside 1..max_positions = %d", L, cfg.max_positions);
  LDIFF_CHECK(out_dtype == LDIFF_F32 || out_dtype == LDIFF_F16, LDIFF_ERR_INVALID, "textenc_forward: out_dtype = %d must be LDIFF_F32 or LDIFF_F16", out_dtype);
  const int M = B * L;
  for (int i = 0; i < M; ++i)
    LDIFF_CHECK(ids_host[i] >= 0 && ids_host[i] < cfg.vocab_size, LDIFF_ERR_INVALID, "textenc_forward: ids[%d][%d] = %d outside 0..vocab_size - 1 = %d", i / L, i % L, (int)ids_host[i],
                cfg.vocab_size - 1);
  LDIFF_CHECK(ws.missing() == 0, LDIFF_ERR_STATE, "textenc: %d weight tensors not loaded (first: %s)", ws.missing(), ws.missing_name(0));
  LDIFF_CHECK(!project || proj_dim > 0, LDIFF_ERR_STATE, "textenc_forward: project = 1 needs proj.weight / proj.bias loaded");
  HIP_CHECK(hipSetDevice(device));
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (s) (void)hipStreamIsCapturing(s, &cs);
  LDIFF_CHECK(cs == hipStreamCaptureStatusNone, LDIFF_ERR_STATE, "textenc_forward: the ids are host data copied at call time; the call cannot run inside a stream capture");
  // the ids always pass through the handle's staging buffer: the eager forward and a replayed graph read them there
  const size_t n_ids = (size_t)M * sizeof(int), n_out = (size_t)M * (project ? proj_dim : cfg.hidden) * (out_dtype == LDIFF_F16 ? 2 : 4);
  st_ids.ensure(n_ids);
  HIP_CHECK(hipMemcpyAsync(st_ids.p, ids_host, n_ids, hipMemcpyHostToDevice, s));
  if (gc.bypass(s)) {
    forward_impl(st_ids.as<int>(), B, L, project, out, out_dtype, s);
    return;
  }
  gc.run(s, [&] { return GraphCache::Key{B, L, project, out_dtype, ws.generation, (long long)ex.arena.capacity(), (long long)reinterpret_cast<uintptr_t>(st_ids.p)}; },
         {{&st_ids, n_ids}, {&st_out, n_out}},
         [&] { forward_impl(st_ids.as<int>(), B, L, project, out, out_dtype, s); },
         [&](hipStream_t cap) { forward_impl(st_ids.as<int>(), B, L, project, st_out.p, out_dtype, cap); },
         [&] {},
         [&] { HIP_CHECK(hipMemcpyAsync(out, st_out.p, n_out, hipMemcpyDeviceToDevice, s)); });
}
