// ldiff_resnet: the instance classifier of the cell head (include/ldiff.h) -- torchvision's ResNet trunk (v1.5 bottlenecks), adapter conv, mean, linear head.
// Executor over the same Exec / plan_conv as the other graphs; the weights are its own: a conv and its BatchNorm are folded on the host in double.
#include <string.h>

#include <algorithm>

#include "model.h"

static const double BN_EPS = 1e-5;   // torchvision's BatchNorm2d default, eval mode (running statistics)

static std::vector<std::string> group_names(const ClsConvW& c) {   // the checkpoint tensors folded into one conv: the weight first
  std::vector<std::string> names = {c.conv + ".weight"};
  if (c.bn.empty()) names.push_back(c.conv + ".bias");
  else
    for (const char* v : {".weight", ".bias", ".running_mean", ".running_var"}) names.push_back(c.bn + v);
  return names;
}

static int add_conv(ldiff_resnet& r, const std::string& conv, const std::string& bn, int Cin, int Cout, int ks, int stride) {
  ClsConvW c;
  c.conv = conv; c.bn = bn; c.Cin = Cin; c.Cout = Cout; c.ks = ks; c.stride = stride;
  c.Cin_pad = (Cin + 7) / 8 * 8;
  c.w = r.ws.alloc_mat(Cout, ks * ks * c.Cin_pad);
  c.b = r.ws.alloc_vec(Cout);
  const std::vector<std::string> names = group_names(c);
  r.ws.add_host(names[0], {Cout, Cin, ks, ks});
  for (size_t i = 1; i < names.size(); ++i) r.ws.add_host(names[i], {Cout});
  r.convs.push_back(c);
  return (int)r.convs.size() - 1;
}

void ldiff_resnet::build() {
  for (int i = 0; i < 4; ++i) LDIFF_CHECK(layers[i] >= 1 && layers[i] <= 64, LDIFF_ERR_INVALID, "resnet_create: layers[%d] = %d outside 1..64", i, layers[i]);
  LDIFF_CHECK(width >= 16 && width <= 256 && width % 16 == 0, LDIFF_ERR_INVALID, "resnet_create: width = %d must be a multiple of 16 in 16..256", width);
  LDIFF_CHECK(adapter_ch >= 16 && adapter_ch <= 8192 && adapter_ch % 16 == 0, LDIFF_ERR_INVALID, "resnet_create: adapter_channels = %d must be a multiple of 16 in 16..8192", adapter_ch);
  LDIFF_CHECK(n_classes >= 2 && n_classes <= 4096, LDIFF_ERR_INVALID, "resnet_create: num_classes = %d outside 2..4096", n_classes);
  nf.create();
  ws.who = "resnet_load";
  ex.weights_gen = &ws.generation;
  ex.nonfinite = nf.words;
  ex.trace_tag = "resnet";
  stem = add_conv(*this, "encoder.0", "encoder.1", 3, width, 7, 2);
  int inpl = width;
  for (int L = 0; L < 4; ++L) {
    const int planes = width << L;
    for (int b = 0; b < layers[L]; ++b) {
      const std::string pre = "encoder." + std::to_string(4 + L) + "." + std::to_string(b);
      const int stride = (b == 0 && L > 0) ? 2 : 1;
      ClsBlockW k;
      k.c1 = add_conv(*this, pre + ".conv1", pre + ".bn1", inpl, planes, 1, 1);
      k.c2 = add_conv(*this, pre + ".conv2", pre + ".bn2", planes, planes, 3, stride);   // v1.5: the stride sits on the 3x3 conv
      k.c3 = add_conv(*this, pre + ".conv3", pre + ".bn3", planes, 4 * planes, 1, 1);
      if (b == 0) k.down = add_conv(*this, pre + ".downsample.0", pre + ".downsample.1", inpl, 4 * planes, 1, stride);
      blocks.push_back(k);
      inpl = 4 * planes;
    }
  }
  adapter = add_conv(*this, "adapter", "", inpl, adapter_ch, 3, 1);
  fc_w = ws.alloc_vec((size_t)n_classes * adapter_ch);
  fc_b = ws.alloc_vec(n_classes);
  ws.add_tensor("classifier.weight", {n_classes, adapter_ch}, fc_w);
  ws.add_tensor("classifier.bias", {n_classes}, fc_b);
  for (size_t i = 0; i < convs.size(); ++i)
    if (!convs[i].bn.empty()) { convs[i].bn_off = bn_total; bn_total += convs[i].Cout; bn_order.push_back((int)i); }
}

// Before the first load: fold() consumes the host tensors, and the un-folded matrices can only be made from them.
void ldiff_resnet::set_train(bool on) {
  if (on == train) return;
  LDIFF_CHECK(ws.generation == 0, LDIFF_ERR_STATE,
              "resnet_set_train: tensors were loaded already; training mode is chosen before the load, because the fold of a conv with its BatchNorm consumes the host tensors "
              "the un-folded matrices are made from");
  HIP_CHECK(hipSetDevice(device));
  if (on)
    for (ClsConvW& c : convs)
      if (!c.bn.empty() && !c.w_raw) {
        c.w_raw = ws.alloc_mat(c.Cout, c.ks * c.ks * c.Cin_pad);
        c.gamma = ws.alloc_vec(c.Cout);
        c.beta = ws.alloc_vec(c.Cout);
      }
  train = on;
}

void ldiff_resnet::load(const char* name, const void* host, int dtype, const int64_t* shape, int ndim) {
  static const std::string nbt = "num_batches_tracked";
  const size_t n = name ? strlen(name) : 0;
  if (n >= nbt.size() && nbt.compare(name + n - nbt.size()) == 0) return;   // BatchNorm's step counter: not a parameter of the eval-mode forward
  ws.load(name, host, dtype, shape, ndim);
}

// w'[n][tap][c] = fp16(w[n][c][tap] * gamma[n] / sqrt(var[n] + eps)), b'[n] = fp32(beta[n] - mean[n] * gamma[n] / sqrt(var[n] + eps)), in double, one rounding each
void ldiff_resnet::fold() {
  if (ws.n_fresh() == 0) return;
  HIP_CHECK(hipDeviceSynchronize());   // (earlier forwards may still read the matrices)
  for (ClsConvW& c : convs) {
    const std::vector<std::string> names = group_names(c);
    size_t n_fresh = 0, n_have = 0;
    std::vector<const std::vector<float>*> v;
    for (auto& n : names) { v.push_back(ws.fresh(n)); n_fresh += v.back() ? 1 : 0; n_have += ws.loaded(n) ? 1 : 0; }
    if (n_fresh == 0 || n_have < names.size()) continue;   // nothing new, or still incomplete (missing() names it)
    LDIFF_CHECK(n_fresh == names.size(), LDIFF_ERR_STATE, "resnet: '%s' was folded with its BatchNorm already; reloading part of the group needs all of %s.* and %s.* again",
                c.conv.c_str(), c.conv.c_str(), c.bn.empty() ? c.conv.c_str() : c.bn.c_str());
    const std::vector<float>& w = *v[0];
    const int taps = c.ks * c.ks, K = taps * c.Cin_pad;
    std::vector<f16> wf((size_t)c.Cout * K, (f16)0.f);
    std::vector<float> bf(c.Cout);
    for (int n = 0; n < c.Cout; ++n) {
      double scale = 1.0, shift;
      if (c.bn.empty()) shift = (*v[1])[n];
      else {
        const double g = (*v[1])[n], be = (*v[2])[n], mu = (*v[3])[n], var = (*v[4])[n];
        scale = g / std::sqrt(var + BN_EPS);
        shift = be - mu * scale;
      }
      bf[n] = (float)shift;
      for (int ci = 0; ci < c.Cin; ++ci)
        for (int t = 0; t < taps; ++t) wf[(size_t)n * K + (size_t)t * c.Cin_pad + ci] = (f16)((double)w[((size_t)n * c.Cin + ci) * taps + t] * scale);
    }
    HIP_CHECK(hipMemcpy(c.w, wf.data(), wf.size() * sizeof(f16), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(c.b, bf.data(), bf.size() * sizeof(float), hipMemcpyHostToDevice));
    if (train && !c.bn.empty()) {   // the un-folded matrix: w rounded once, the same layout; gamma / beta as they are
      std::fill(wf.begin(), wf.end(), (f16)0.f);
      for (int n = 0; n < c.Cout; ++n)
        for (int ci = 0; ci < c.Cin; ++ci)
          for (int t = 0; t < taps; ++t) wf[(size_t)n * K + (size_t)t * c.Cin_pad + ci] = (f16)w[((size_t)n * c.Cin + ci) * taps + t];
      HIP_CHECK(hipMemcpy(c.w_raw, wf.data(), wf.size() * sizeof(f16), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(c.gamma, v[1]->data(), (size_t)c.Cout * sizeof(float), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(c.beta, v[2]->data(), (size_t)c.Cout * sizeof(float), hipMemcpyHostToDevice));
    }
    c.folded = true;
    for (auto& n : names) ws.consume(n);
  }
}

Act ldiff_resnet::conv(const ClsConvW& c, const Act& x, const Act* res, bool relu) {
  ConvParams p;
  memset(&p, 0, sizeof(p));
  LDIFF_CHECK(x.C == c.Cin_pad && !x.split, LDIFF_ERR_INVALID, "resnet conv %s: input has %d channels, weight expects %d", c.conv.c_str(), x.C, c.Cin_pad);
  p.x = x.p; p.C1 = x.C;
  p.B = x.B; p.Hin = x.H; p.Win = x.W;
  p.ks = c.ks; p.stride = c.stride; p.pad_t = c.ks / 2; p.pad_l = c.ks / 2;
  p.Hout = (x.H - 1) / c.stride + 1; p.Wout = (x.W - 1) / c.stride + 1;
  p.w = c.w; p.N = c.Cout; p.Nrows = c.Cout; p.K = c.ks * c.ks * c.Cin_pad;
  p.bias = c.b;
  p.M = x.B * p.Hout * p.Wout;
  p.ldy = c.Cout;
  p.relu_out = relu ? 1 : 0;
  p.cls_force = 1;   // (the downsample and adapter convs carry no ReLU: the family on request)
  p.nonfinite = ex.nonfinite;
  if (res) {
    LDIFF_CHECK(res->rows() == p.M && res->C == p.N && !res->split, LDIFF_ERR_INVALID, "resnet conv %s: identity shape mismatch", c.conv.c_str());
    p.res = res->p; p.ld_res = res->ld();
  }
  Act y = ex.new_act(x.B, p.Hout, p.Wout, c.Cout);
  p.y = y.p;   // (before the plan: the family's eligibility test looks at every pointer's alignment)
  ConvAsk ask;
  ask.splitk = 1;   // never split: the K order of a sum must not depend on the batch
  const ConvPlan pl = plan_conv(p, ask);
  LDIFF_CHECK(pl.kernel == ConvKernel::CLSCONV, LDIFF_ERR_INVALID, "resnet conv %s: not taken by the classifier's conv family", c.conv.c_str());
  launch_igemm(p, pl, ex.s);
  return y;
}

void ldiff_resnet::forward_impl(const f16* crops, int B, int S, float* logits, int* labels, hipStream_t s) {
  HIP_CHECK(hipSetDevice(device));
  ex.s = s;
  ex.arena.reset();
  // live at once, at most (first block of layer 1): the pooled map, two quarter-size tensors, the downsampled identity and the block's output: < 3 x the stem's output
  const size_t unit = (size_t)B * (S / 2) * (S / 2) * width * sizeof(f16);
  ex.arena.reserve(4 * unit + (8u << 20));

  Act in;
  in.p = const_cast<f16*>(crops); in.B = B; in.H = S; in.W = S; in.C = 8; in.borrowed = true;
  Act a = conv(convs[stem], in, nullptr, true);
  ex.trace("stem", a);
  Act cur = ex.new_act(B, (a.H - 1) / 2 + 1, (a.W - 1) / 2 + 1, width);
  launch_maxpool3x3s2(a.p, cur.p, B, a.H, a.W, width, s);
  ex.release(a);
  int bi = 0;
  for (int L = 0; L < 4; ++L) {
    for (int b = 0; b < layers[L]; ++b, ++bi) {
      const ClsBlockW& k = blocks[bi];
      Act t1 = conv(convs[k.c1], cur, nullptr, true);
      Act t2 = conv(convs[k.c2], t1, nullptr, true);
      ex.release(t1);
      Act idn = cur;
      if (k.down >= 0) idn = conv(convs[k.down], cur, nullptr, false);
      Act out = conv(convs[k.c3], t2, &idn, true);   // relu(bn3(conv3) + identity)
      ex.release(t2);
      if (k.down >= 0) ex.release(idn);
      ex.release(cur);
      cur = out;
    }
    ex.trace(("layer" + std::to_string(L + 1)).c_str(), cur);
  }
  Act ad = conv(convs[adapter], cur, nullptr, false);
  ex.release(cur);
  ex.trace("adapter", ad);
  launch_cls_head(ad.p, B, ad.H * ad.W, adapter_ch, ad.ld(), fc_w, fc_b, n_classes, logits, labels, s);
  ex.release(ad);
}

void ldiff_resnet::forward(const f16* crops, int B, int S, float* logits, int* labels, hipStream_t s) {
  LDIFF_CHECK(crops && logits, LDIFF_ERR_INVALID, "resnet_forward: null pointer");
  LDIFF_CHECK(B >= 1, LDIFF_ERR_INVALID, "resnet_forward: B = %d must be at least 1", B);
  LDIFF_CHECK(S >= 32 && S <= 1024 && S % 32 == 0, LDIFF_ERR_INVALID, "resnet_forward: S = %d must be a multiple of 32 in 32..1024", S);
  LDIFF_CHECK((long long)B * (S / 2) * (S / 2) * width < (1ll << 31), LDIFF_ERR_INVALID, "resnet_forward: B * (S / 2)^2 * width exceeds 2^31 (B = %d, S = %d)", B, S);
  LDIFF_CHECK(ws.missing() == 0, LDIFF_ERR_STATE, "resnet: %d weight tensors not loaded (first: %s)", ws.missing(), ws.missing_name(0));
  HIP_CHECK(hipSetDevice(device));
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (s) (void)hipStreamIsCapturing(s, &cs);
  if (cs == hipStreamCaptureStatusNone) fold();
  LDIFF_CHECK(ws.n_fresh() == 0, LDIFF_ERR_STATE, "resnet_forward: weights were loaded but not folded yet; the first forward after a load cannot run inside a stream capture");
  if (gc.bypass(s)) {
    forward_impl(crops, B, S, logits, labels, s);
    return;
  }
  const size_t n_in = (size_t)B * S * S * 8 * sizeof(f16), n_log = (size_t)B * n_classes * sizeof(float), n_lab = (size_t)B * sizeof(int);
  gc.run(s, [&] { return GraphCache::Key{B, S, ws.generation, (long long)ex.arena.capacity()}; }, {{&st_in, n_in}, {&st_logits, n_log}, {&st_labels, n_lab}},
         [&] { forward_impl(crops, B, S, logits, labels, s); },
         [&](hipStream_t cap) { forward_impl(st_in.as<f16>(), B, S, st_logits.as<float>(), st_labels.as<int>(), cap); },
         [&] { HIP_CHECK(hipMemcpyAsync(st_in.p, crops, n_in, hipMemcpyDeviceToDevice, s)); },
         [&] {
           HIP_CHECK(hipMemcpyAsync(logits, st_logits.p, n_log, hipMemcpyDeviceToDevice, s));
           if (labels) HIP_CHECK(hipMemcpyAsync(labels, st_labels.p, n_lab, hipMemcpyDeviceToDevice, s));
         });
}

// ---- training mode: conv -> batch statistics -> scale / shift, then one apply launch that carries the ReLU and the block's identity ----
ClsBnOut ldiff_resnet::conv_bn(const ClsConvW& c, const Act& x, float* batch_stats) {
  ConvParams p;
  memset(&p, 0, sizeof(p));
  LDIFF_CHECK(x.C == c.Cin_pad && !x.split, LDIFF_ERR_INVALID, "resnet conv %s: input has %d channels, weight expects %d", c.conv.c_str(), x.C, c.Cin_pad);
  p.x = x.p; p.C1 = x.C;
  p.B = x.B; p.Hin = x.H; p.Win = x.W;
  p.ks = c.ks; p.stride = c.stride; p.pad_t = c.ks / 2; p.pad_l = c.ks / 2;
  p.Hout = (x.H - 1) / c.stride + 1; p.Wout = (x.W - 1) / c.stride + 1;
  p.w = c.w_raw; p.N = c.Cout; p.Nrows = c.Cout; p.K = c.ks * c.ks * c.Cin_pad;
  p.M = x.B * p.Hout * p.Wout;
  p.ldy = c.Cout;
  p.cls_force = 1;
  p.nonfinite = ex.nonfinite;
  ClsBnOut o;
  o.raw = ex.new_act(x.B, p.Hout, p.Wout, c.Cout);
  p.y = o.raw.p;
  const int R = cls_conv_bn_stats_blocks(p);
  float* part = ex.tmp<float>((size_t)c.Cout * R * 2);
  p.bn_stats = part;
  ConvAsk ask;
  ask.splitk = 1;
  const ConvPlan pl = plan_conv(p, ask);
  LDIFF_CHECK(pl.kernel == ConvKernel::CLSCONV, LDIFF_ERR_INVALID, "resnet conv %s: not taken by the classifier's conv family", c.conv.c_str());
  launch_igemm(p, pl, ex.s);
  o.scale = ex.tmp<float>(c.Cout);
  o.shift = ex.tmp<float>(c.Cout);
  launch_bn_finalize(part, R, c.Cout, p.M, c.gamma, c.beta, o.scale, o.shift, batch_stats, c.bn_off, bn_total, ex.s);
  ex.arena.free(part);   // (stream order: the next writer of these bytes runs behind the finalize)
  return o;
}

Act ldiff_resnet::bn_apply(ClsBnOut& a, const Act* id_plain, ClsBnOut* id_bn, bool relu) {
  const Act* id = id_bn ? &id_bn->raw : id_plain;
  LDIFF_CHECK(!id || (id->rows() == a.raw.rows() && id->C == a.raw.C && !id->split), LDIFF_ERR_INVALID, "resnet bn_apply: identity shape mismatch");
  Act y = ex.new_act(a.raw.B, a.raw.H, a.raw.W, a.raw.C);
  launch_bn_apply(a.raw.p, a.raw.rows(), a.raw.C, a.scale, a.shift, id ? id->p : nullptr, id_bn ? id_bn->scale : nullptr, id_bn ? id_bn->shift : nullptr, relu ? 1 : 0, y.p,
                  ex.nonfinite, ex.s);
  for (ClsBnOut* o : {&a, id_bn}) {
    if (!o) continue;
    ex.release(o->raw);
    ex.arena.free(o->scale); ex.arena.free(o->shift);
    o->scale = o->shift = nullptr;
  }
  return y;
}

void ldiff_resnet::forward_train(const f16* crops, int B, int S, float* batch_stats, float* features, float* logits, int* labels, hipStream_t s) {
  LDIFF_CHECK(train, LDIFF_ERR_STATE, "resnet_forward_train: the handle was not put in training mode (ldiff_resnet_set_train(h, 1) before the tensors are loaded; python: ResNetClassifier(train=True))");
  LDIFF_CHECK(crops && batch_stats && features, LDIFF_ERR_INVALID, "resnet_forward_train: null pointer");
  LDIFF_CHECK(B >= 1, LDIFF_ERR_INVALID, "resnet_forward_train: B = %d must be at least 1", B);
  LDIFF_CHECK(S >= 32 && S <= 1024 && S % 32 == 0, LDIFF_ERR_INVALID, "resnet_forward_train: S = %d must be a multiple of 32 in 32..1024", S);
  LDIFF_CHECK((long long)B * (S / 2) * (S / 2) * width < (1ll << 31), LDIFF_ERR_INVALID, "resnet_forward_train: B * (S / 2)^2 * width exceeds 2^31 (B = %d, S = %d)", B, S);
  LDIFF_CHECK(ws.missing() == 0, LDIFF_ERR_STATE, "resnet: %d weight tensors not loaded (first: %s)", ws.missing(), ws.missing_name(0));
  {   // every BatchNorm needs more than one value per channel (torch: "Expected more than 1 value per channel when training"): checked for the whole network before any launch
    int h = S / 4, bi = 0;   // the map behind the pooling
    for (int L = 0; L < 4; ++L)
      for (int b = 0; b < layers[L]; ++b, ++bi) {
        const int ho = (b == 0 && L > 0) ? (h - 1) / 2 + 1 : h;
        const ClsBlockW& k = blocks[bi];
        const std::pair<int, int> at[4] = {{k.c1, h}, {k.c2, ho}, {k.c3, ho}, {k.down, ho}};
        for (const auto& e : at)
          LDIFF_CHECK(e.first < 0 || (long long)B * e.second * e.second >= 2, LDIFF_ERR_INVALID,
                      "resnet_forward_train: expected more than 1 value per channel when training: BatchNorm %s sees B * H * W = %d * %d * %d = 1 (S = %d)", e.first < 0 ? "" : convs[e.first].bn.c_str(),
                      B, e.second, e.second, S);
        h = ho;
      }
  }
  HIP_CHECK(hipSetDevice(device));
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (s) (void)hipStreamIsCapturing(s, &cs);
  LDIFF_CHECK(cs == hipStreamCaptureStatusNone, LDIFF_ERR_STATE, "resnet_forward_train: runs eagerly (B differs from image to image), not inside a stream capture");
  fold();
  ex.s = s;
  ex.arena.reset();
  // live at once, at most (first block of layer 1): the block's input and conv2's output (a quarter of the stem's output each), the raw downsample and conv3 tensors and the block's
  // output (one each), plus a conv's partials (at most a quarter of its raw tensor) and scale / shift vectors
  const size_t unit = (size_t)B * (S / 2) * (S / 2) * width * sizeof(f16);
  ex.arena.reserve(6 * unit + (16u << 20));

  Act in;
  in.p = const_cast<f16*>(crops); in.B = B; in.H = S; in.W = S; in.C = 8; in.borrowed = true;
  ClsBnOut st = conv_bn(convs[stem], in, batch_stats);
  Act a = bn_apply(st, nullptr, nullptr, true);
  ex.trace("stem", a);
  Act cur = ex.new_act(B, (a.H - 1) / 2 + 1, (a.W - 1) / 2 + 1, width);
  launch_maxpool3x3s2(a.p, cur.p, B, a.H, a.W, width, s);
  ex.release(a);
  int bi = 0;
  for (int L = 0; L < 4; ++L) {
    for (int b = 0; b < layers[L]; ++b, ++bi) {
      const ClsBlockW& k = blocks[bi];
      ClsBnOut r1 = conv_bn(convs[k.c1], cur, batch_stats);
      Act t1 = bn_apply(r1, nullptr, nullptr, true);
      ClsBnOut r2 = conv_bn(convs[k.c2], t1, batch_stats);
      ex.release(t1);
      Act t2 = bn_apply(r2, nullptr, nullptr, true);
      ClsBnOut r3 = conv_bn(convs[k.c3], t2, batch_stats);
      ex.release(t2);
      Act out;
      if (k.down >= 0) {
        ClsBnOut rd = conv_bn(convs[k.down], cur, batch_stats);
        out = bn_apply(r3, nullptr, &rd, true);   // relu(bn3(conv3) + bn_d(downsample))
      } else {
        out = bn_apply(r3, &cur, nullptr, true);  // relu(bn3(conv3) + identity)
      }
      ex.release(cur);
      cur = out;
    }
    ex.trace(("layer" + std::to_string(L + 1)).c_str(), cur);
  }
  Act ad = conv(convs[adapter], cur, nullptr, false);   // (bias, no BatchNorm: as in eval mode)
  ex.release(cur);
  ex.trace("adapter", ad);
  launch_cls_head_feat(ad.p, B, ad.H * ad.W, adapter_ch, ad.ld(), fc_w, fc_b, n_classes, logits, labels, features, s);
  ex.release(ad);
}
