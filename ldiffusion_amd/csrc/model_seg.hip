// ldiff_segnet: the nnU-Net v2 PlainConvUNet (2-D) of the tissue head (include/ldiff.h; /root/reference/segmentor.py:463-488 builds it through
// nnUNetPredictor.initialize_from_trained_model_folder -> get_network_from_plans).  Executor over the same Exec / WeightStore / plan_conv as the UNet and the VAE.
#include <string.h>

#include <algorithm>

#include "model.h"

static const float IN_EPS = 1e-5f;   // InstanceNorm2d's eps in every nnU-Net plans file (norm_op_kwargs)

void ldiff_segnet::build() {
  LDIFF_CHECK(n_stages >= 2 && n_stages <= 16, LDIFF_ERR_INVALID, "segnet_create: n_stages = %d outside 2..16", n_stages);
  LDIFF_CHECK(in_ch >= 1 && in_ch <= 8, LDIFF_ERR_INVALID, "segnet_create: in_channels = %d outside 1..8", in_ch);
  LDIFF_CHECK(n_heads >= 1 && n_heads <= 64, LDIFF_ERR_INVALID, "segnet_create: n_heads = %d outside 1..64", n_heads);
  for (int s = 0; s < n_stages; ++s) {
    LDIFF_CHECK(features[s] >= 16 && features[s] % 16 == 0, LDIFF_ERR_INVALID, "segnet_create: features[%d] = %d must be a multiple of 16", s, features[s]);
    LDIFF_CHECK(strides[s] == 1 || strides[s] == 2, LDIFF_ERR_INVALID, "segnet_create: strides[%d] = %d (1 or 2 in both axes)", s, strides[s]);
    LDIFF_CHECK(nce[s] >= 1 && nce[s] <= 8, LDIFF_ERR_INVALID, "segnet_create: n_conv_per_stage[%d] = %d outside 1..8", s, nce[s]);
    if (s > 0) LDIFF_CHECK(strides[s] == 2, LDIFF_ERR_INVALID, "segnet_create: strides[%d] = 1: the transposed conv of a decoder stage has kernel = stride = 2 here", s);
  }
  LDIFF_CHECK(strides[0] == 1, LDIFF_ERR_INVALID, "segnet_create: strides[0] = %d: the first stage keeps the resolution", strides[0]);
  for (int j = 0; j < n_stages - 1; ++j) LDIFF_CHECK(ncd[j] >= 1 && ncd[j] <= 8, LDIFF_ERR_INVALID, "segnet_create: n_conv_per_stage_decoder[%d] = %d outside 1..8", j, ncd[j]);
  nf.create();
  ex.weights_gen = &ws.generation;
  ex.nonfinite = nf.words;
  ex.trace_tag = "segnet";
  enc.resize(n_stages);
  for (int s = 0; s < n_stages; ++s) {
    int cin = s == 0 ? in_ch : features[s - 1];
    for (int i = 0; i < nce[s]; ++i) {
      const std::string pre = "encoder.stages." + std::to_string(s) + ".0.convs." + std::to_string(i);
      SegConvW c;
      c.conv = ws.add_conv(pre + ".conv", cin, features[s], 3);
      c.norm = ws.add_norm(pre + ".norm", features[s]);
      enc[s].push_back(c);
      cin = features[s];
    }
  }
  dec.resize(n_stages - 1);
  for (int j = 0; j < n_stages - 1; ++j) {
    const int below = features[n_stages - 1 - j], skip = features[n_stages - 2 - j];
    up.push_back(ws.add_tconv("decoder.transpconvs." + std::to_string(j), below, skip, 2));
    int cin = 2 * skip;
    for (int i = 0; i < ncd[j]; ++i) {
      const std::string pre = "decoder.stages." + std::to_string(j) + ".convs." + std::to_string(i);
      SegConvW c;
      c.conv = ws.add_conv(pre + ".conv", cin, skip, 3);
      c.norm = ws.add_norm(pre + ".norm", skip);
      dec[j].push_back(c);
      cin = skip;
    }
  }
  head = ws.add_conv("decoder.seg_layers." + std::to_string(n_stages - 2), features[0], n_heads, 1);
}

GNss ldiff_segnet::in_ss(const Act& a, const NormW& w, int ident) {
  LDIFF_CHECK(a.C == w.C && !a.split, LDIFF_ERR_INVALID, "instance norm: %d channels, weight has %d", a.C, w.C);
  GNss g;
  const int ld = ident + a.C;
  g.scale = ex.tmp<float>((size_t)a.B * ld);
  g.shift = ex.tmp<float>((size_t)a.B * ld);
  launch_in_finalize(a.st, a.st_R, a.p, a.ld(), a.B, a.H * a.W, a.C, IN_EPS, w.g, w.b, g.scale, g.shift, ld, ident, ident, ex.s, ex.nonfinite);
  return g;
}

// The 2x2 transposed conv of a decoder stage on the raw output of the stage below (its InstanceNorm + LeakyReLU in the prologue)
static Act seg_tconv(Exec& ex, const MatW& w, const Act& x, const GNss& g) {
  ConvParams p;
  memset(&p, 0, sizeof(p));
  LDIFF_CHECK(x.C == w.Cin && !x.split, LDIFF_ERR_INVALID, "tconv: input has %d channels, weight expects %d", x.C, w.Cin);
  p.x = x.p; p.C1 = x.C;
  p.B = x.B; p.Hin = x.H; p.Win = x.W; p.Hout = 2 * x.H; p.Wout = 2 * x.W;
  p.ks = 2; p.stride = 2; p.tconv = 1;
  p.w = w.w; p.N = w.N; p.Nrows = w.Nrows; p.K = w.K;
  p.bias = w.b;
  p.gn_scale = g.scale; p.gn_shift = g.shift; p.lrelu_in = 1;
  p.M = x.B * p.Hout * p.Wout;
  p.ldy = w.N;
  const ConvPlan pl = plan_conv(p, ConvAsk{});
  Act y = ex.new_act(x.B, p.Hout, p.Wout, w.N);
  p.y = y.p;
  launch_igemm(p, pl, ex.s);
  return y;
}

void ldiff_segnet::forward_impl(const float* x, int B, int H, int W, void* out, int out_dtype, hipStream_t s) {
  LDIFF_CHECK(x && out && B >= 1 && H >= 1 && W >= 1, LDIFF_ERR_INVALID, "segnet_forward: null pointer or empty shape");
  LDIFF_CHECK(out_dtype == LDIFF_F32 || out_dtype == LDIFF_F16, LDIFF_ERR_INVALID, "segnet_forward: out dtype %d (LDIFF_F32 or LDIFF_F16)", out_dtype);
  int div = 1;
  for (int st : strides) div *= st;
  LDIFF_CHECK(H % div == 0 && W % div == 0, LDIFF_ERR_INVALID, "segnet_forward: %dx%d must be divisible by the product of the strides, %d", H, W, div);
  LDIFF_CHECK(ws.missing() == 0, LDIFF_ERR_STATE, "segnet: %d weight tensors not loaded (first: %s)", ws.missing(), ws.missing_name(0));
  LDIFF_CHECK((long long)B * H * W * features[0] < (1ll << 31), LDIFF_ERR_INVALID, "segnet_forward: B * H * W * features[0] exceeds 2^31");
  HIP_CHECK(hipSetDevice(device));
  ex.s = s;
  ex.arena.reset();
  // live at once: the skip of every stage (2 x the first one's bytes in all), the running tensors, their partial sums (1/8 of a tensor), split-K partials
  ex.arena.reserve((size_t)B * H * W * features[0] * 2 * 12 + (64u << 20));

  Act cur = ex.new_act(B, H, W, roundup(in_ch, 8));
  launch_nchw_f32_to_nhwc_f16(x, cur.p, B, in_ch, H, W, cur.C, s);
  const NormW* cur_norm = nullptr;   // the InstanceNorm `cur` (a raw conv output) still has to pass through
  auto conv_block = [&](const SegConvW& c, const Act& a, const Act* a2, const NormW* norm, int stride) {
    ConvOpts o;
    o.stride = stride;
    o.want_stats = true;
    o.splitk_per_image = true;
    o.seg_conv = 1;   // (the first conv has no prologue: the narrow kernel on request)
    GNss g;
    if (norm) {
      g = in_ss(a2 ? *a2 : a, *norm, a2 ? a.C : 0);
      o.gn = &g; o.lrelu = a2 ? 2 : 1;
    }
    Act y = ex.conv(c.conv, a, a2, o);
    if (norm) ex.release(g);
    return y;
  };
  std::vector<Act> skips(n_stages);
  std::vector<const NormW*> skip_norm(n_stages);
  for (int st = 0; st < n_stages; ++st) {
    for (int i = 0; i < nce[st]; ++i) {
      Act y = conv_block(enc[st][i], cur, nullptr, cur_norm, i == 0 ? strides[st] : 1);
      const bool is_skip = st > 0 && i == 0;   // `cur` is then the output of the stage above: kept for the decoder
      if (!is_skip) ex.release(cur);
      cur = y;
      cur_norm = &enc[st][i].norm;
    }
    ex.trace(("encoder." + std::to_string(st)).c_str(), cur);
    skips[st] = cur; skip_norm[st] = cur_norm;
  }
  for (int j = 0; j < n_stages - 1; ++j) {
    GNss g = in_ss(cur, *cur_norm, 0);
    Act upx = seg_tconv(ex, up[j], cur, g);
    ex.release(g);
    ex.release(cur);
    Act& skip = skips[n_stages - 2 - j];
    LDIFF_CHECK(skip.H == upx.H && skip.W == upx.W, LDIFF_ERR_INVALID, "segnet: skip %dx%d against upsampled %dx%d", skip.H, skip.W, upx.H, upx.W);
    cur = conv_block(dec[j][0], upx, &skip, skip_norm[n_stages - 2 - j], 1);
    ex.release(upx);
    ex.release(skip);
    cur_norm = &dec[j][0].norm;
    for (int i = 1; i < ncd[j]; ++i) {
      Act y = conv_block(dec[j][i], cur, nullptr, cur_norm, 1);
      ex.release(cur);
      cur = y;
      cur_norm = &dec[j][i].norm;
    }
    ex.trace(("decoder." + std::to_string(j)).c_str(), cur);
  }
  // segmentation head: 1x1 conv on lrelu(in(cur)), fp32, then NHWC -> NCHW in the caller's dtype
  const int ldl = roundup(n_heads, 4);
  float* logits = ex.tmp<float>((size_t)B * H * W * ldl);
  {
    GNss g = in_ss(cur, *cur_norm, 0);
    ConvOpts o;
    o.gn = &g; o.lrelu = 1;
    o.splitk_per_image = true;
    o.out_f32 = logits; o.ldy_f32 = ldl;
    ex.conv(head, cur, nullptr, o);
    ex.release(g);
    ex.release(cur);
  }
  launch_nhwc_f32_to_nchw(logits, out, B, n_heads, H, W, ldl, out_dtype == LDIFF_F16 ? 1 : 0, s);
  ex.arena.free(logits);
}

void ldiff_segnet::forward(const float* x, int B, int H, int W, void* out, int out_dtype, hipStream_t s) {
  if (!x || !out || B < 1 || H < 1 || W < 1 || (out_dtype != LDIFF_F32 && out_dtype != LDIFF_F16) || gc.bypass(s)) {
    forward_impl(x, B, H, W, out, out_dtype, s);   // (argument errors are reported by forward_impl)
    return;
  }
  HIP_CHECK(hipSetDevice(device));
  const size_t n_in = (size_t)B * in_ch * H * W * sizeof(float), n_out = (size_t)B * n_heads * H * W * (out_dtype == LDIFF_F16 ? 2 : 4);
  gc.run(s, [&] { return GraphCache::Key{B, H, W, out_dtype, ws.generation, (long long)ex.arena.capacity()}; }, {{&st_in, n_in}, {&st_out, n_out}},
         [&] { forward_impl(x, B, H, W, out, out_dtype, s); },
         [&](hipStream_t cs) { forward_impl(st_in.as<float>(), B, H, W, st_out.p, out_dtype, cs); },
         [&] { HIP_CHECK(hipMemcpyAsync(st_in.p, x, n_in, hipMemcpyDeviceToDevice, s)); },
         [&] { HIP_CHECK(hipMemcpyAsync(out, st_out.p, n_out, hipMemcpyDeviceToDevice, s)); });
}
