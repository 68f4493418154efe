"""Float64 restatements for the tests of the tissue head's training step (TEST INFRASTRUCTURE ONLY): nnU-Net's deep-supervision Dice + cross-entropy
loss, InstanceNorm + LeakyReLU with the error bound of ldiff_op_in_train_fwd / _bwd, and the PlainConvUNet with deep supervision on a float64 tape whose
stored tensors can be rounded to fp16 in both passes (the fp16-storage model the whole-step tests use as their yardstick).

The loss follows the public algorithm of nnunetv2's DC_and_CE_loss(MemoryEfficientSoftDiceLoss(do_bg=False, smooth=1e-5, batch_dice), CrossEntropyLoss)
under DeepSupervisionWrapper; tests/test_cpu_nnunet_train.py pins it to values recorded from those modules (tests/golden/reference_dc_ce_loss.npz)."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24      # unit roundoff of fp32
U16 = 2.0 ** -11    # of fp16
SUB16 = 2.0 ** -25  # half a subnormal step of fp16
IN_ROWS = 32        # csrc/kernels_segtrain.hip: at most this many terms per fp32 accumulator, the rest of every sum is added in double


def gamma(n):
    return 2.0 * n * U


# ---- the loss -------------------------------------------------------------------------------------------------------------------------------------
def dc_ce_loss(logits, target, batch_dice, do_bg=False, smooth=1e-5):
    """logits [B, n, H, W] (any float dtype, differentiable), target integer [B, H, W] -> CE_mean - mean_c dc_c."""
    B, n = logits.shape[:2]
    p = torch.softmax(logits, 1)
    onehot = F.one_hot(target.long(), n).permute(0, 3, 1, 2).to(logits.dtype)
    first = 0 if do_bg else 1
    p, onehot = p[:, first:], onehot[:, first:]
    intersect, sum_pred, sum_gt = (p * onehot).sum((2, 3)), p.sum((2, 3)), onehot.sum((2, 3))
    if batch_dice:
        intersect, sum_pred, sum_gt = intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)
    dc = (2 * intersect + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)
    ce = F.cross_entropy(logits, target.long())
    return ce - dc.mean()


def first_pass_dice_loss(logits, target, keep, loss, ce):
    """A WRONG loss the bounds must reject: the cross-entropy `ce(logits, target)` of the whole batch, the Dice term of `loss` from samples < keep alone
    (what the finalize's first pass over its [sample][accumulator] slots covers).  `loss`, `ce`: callables on (logits [b, n, H, W], target [b, H, W])."""
    return ce(logits, target) + loss(logits[:keep], target[:keep]) - ce(logits[:keep], target[:keep])


def deep_supervision_loss(outputs, targets, weights, batch_dice, **kw):
    return sum(w * dc_ce_loss(o, t, batch_dice, **kw) for o, t, w in zip(outputs, targets, weights) if w != 0.0)


def label_maps(B, n_heads, size, n_scales, seed):
    """Smooth label maps with every class present: arg-max over n_heads smooth random fields, then the lower scales by 2x sub-sampling."""
    g = torch.Generator().manual_seed(seed)
    f = F.avg_pool2d(torch.randn((B, n_heads, size + 6, size + 6), generator=g), 7, 1)
    top = f.argmax(1)
    step = 2 ** (n_scales - 1)          # every class present in every image at every scale: one pixel each on the coarsest grid, should the fields miss one
    for c in range(n_heads):
        top[:, (c * step) % size, (c * step) // size * step] = c
    return [top[:, ::2 ** i, ::2 ** i].contiguous() for i in range(n_scales)]


# ---- InstanceNorm + LeakyReLU: float64 values and the kernel's error bound -------------------------------------------------------------------------
def in_lrelu_reference(x, dy, gm, bt, eps, slope, batch_stats=False):
    """x, dy [B, HW, C] float64 (fp16-exact values), gm / bt [C] float64.  Returns a dict of float64 tensors: y, dx, dgamma, dbeta and the intermediate
    quantities the bound needs.  batch_stats: the (wrong) statistics over the batch as well."""
    dims = (0, 1) if batch_stats else (1,)
    mu = x.mean(dims, keepdim=True)
    var = x.var(dims, unbiased=False, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * r
    a = xh * gm + bt
    y = torch.where(a > 0, a, a * slope)
    da = dy * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))
    m1, m2 = da.mean(1, keepdim=True), (da * xh).mean(1, keepdim=True)
    dx = r * gm * (da - m1 - xh * m2)
    return dict(mu=mu, var=var, r=r, xh=xh, a=a, y=y, da=da, m1=m1, m2=m2, dx=dx, dgamma=(da * xh).sum((0, 1)), dbeta=da.sum((0, 1)))


def in_lrelu_bounds(x, dy, gm, bt, eps, slope):
    """Per-element bounds on |kernel - float64| for y and dx, per-channel bounds for dgamma / dbeta, and the mask of elements whose float64 pre-activation
    is smaller than the fp32 evaluation error of that value (they may take either branch).  u = 2^-24, gamma(n) = 2 n u.

    Statistics.  A sum over the HW pixels of an image is formed from fp32 accumulators of at most IN_ROWS terms (error gamma(IN_ROWS) of the sum of
    magnitudes), one fp32 rounding of each workgroup's partial, a double sum, one fp32 rounding of the result: gamma(IN_ROWS + 2) =: gs of the sum of
    magnitudes; a sum of products carries one more rounding, gq = gamma(IN_ROWS + 3).
        |d mu| <= gs E|x|;    |d var| <= gq E[x^2] + 2 |mu| gs E|x| <= 3 gq E[x^2];    e_r = |d rstd| / rstd <= 1.5 gq E[x^2] / (var + eps) + u
    Values.   xhat = fl((x - mu) rstd):  |d xhat| <= |xhat| (2u + e_r) + rstd |d mu|;   a = fma(xhat, gamma, beta):  |d a| <= |gamma| |d xhat| + u |a|;
        y = fl16(fl(a s)), s = 1 or slope:  |d y| <= s |d a| + u |y| + 2^-11 |y| (1 + 2u) + 2^-25.
    Backward, with A = the elements that may take either branch: da = fl(dy s) (|d da| <= u |da| off A);  m1 = mean da, m2 = mean(da xhat):
        |d m1| <= (gs + u) E|da| + sum_A |dy| (1 - slope) / HW;    |d m2| <= (gq + u) E|da xhat| + E(|da| |d xhat|) + sum_A |dy xhat| (1 - slope) / HW
        dx = fl16(rstd gamma (da - m1 - xhat m2)):  |d dx| <= |rstd gamma| ((4u + e_r) (|da| + |m1| + |xhat m2|) + |d m1| + |xhat| |d m2| + |m2| |d xhat|)
                                                              + 2^-11 |dx| (1 + 4u) + 2^-25
        dgamma, dbeta: HW times the m2 / m1 bounds, summed over the batch, plus one fp32 rounding of the result."""
    ref = in_lrelu_reference(x, dy, gm, bt, eps, slope)
    HW = x.shape[1]
    gs, gq = gamma(IN_ROWS + 2), gamma(IN_ROWS + 3)
    Ex, Ex2 = x.abs().mean(1, keepdim=True), (x * x).mean(1, keepdim=True)
    d_mu = gs * Ex
    e_r = 1.5 * gq * Ex2 / (ref["var"] + eps) + U
    xh, a, r = ref["xh"], ref["a"], ref["r"]
    d_xh = xh.abs() * (2 * U + e_r) + r * d_mu
    d_a = gm.abs() * d_xh + U * a.abs()
    amb = a.abs() <= d_a
    s = torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))
    y = ref["y"]
    tol_y = s * d_a + U * y.abs() + U16 * y.abs() * (1 + 2 * U) + SUB16
    da = ref["da"]
    flip = torch.where(amb, dy.abs() * abs(1.0 - slope), torch.zeros_like(dy))
    d_m1 = (gs + U) * da.abs().mean(1, keepdim=True) + flip.sum(1, keepdim=True) / HW
    d_m2 = (gq + U) * (da * xh).abs().mean(1, keepdim=True) + (da.abs() * d_xh).mean(1, keepdim=True) + (flip * (xh.abs() + d_xh)).sum(1, keepdim=True) / HW
    m1, m2, dx = ref["m1"], ref["m2"], ref["dx"]
    tol_dx = (r * gm).abs() * ((4 * U + e_r) * (da.abs() + m1.abs() + (xh * m2).abs()) + d_m1 + xh.abs() * d_m2 + m2.abs() * d_xh) + U16 * dx.abs() * (1 + 4 * U) + SUB16
    tol_dgamma = (HW * d_m2).sum((0, 1)) + U * ref["dgamma"].abs()
    tol_dbeta = (HW * d_m1).sum((0, 1)) + U * ref["dbeta"].abs()
    return ref, dict(y=tol_y, dx=tol_dx, dgamma=tol_dgamma, dbeta=tol_dbeta, ambiguous=amb)


def in_layout(HW, C):
    """csrc/kernels_segtrain.hip's in_layout restated: a row is C8 = C / 8 vectors, G = min(C8, 256) threads cover it (C8 > 256: in several passes), nrl =
    256 // G row lanes take alternate rows (256 - nrl G threads idle), a workgroup owns a slab of S = nrl IN_ROWS rows, an image has R slabs.  The two
    finalize kernels add an image's R partials 64 at a time.  tests/test_cpu_nnunet_train.py pins this to the library's workspace size."""
    C8 = C // 8
    G = min(C8, 256)
    nrl = 256 // G
    S = nrl * IN_ROWS
    return dict(C8=C8, G=G, nrl=nrl, S=S, R=-(-HW // S))


def in_lrelu_first_pass_reference(x, dy, gm, bt, eps, slope, rows):
    """What the kernels would hand out if each finalize stopped after its first pass over the slabs (a WRONG reference the bounds must reject): every sum over
    the pixels of an image runs over pixels < `rows` only and is still divided by HW.  Returns mu, var, r [B, 1, C] and dgamma, dbeta [C], float64."""
    HW = x.shape[1]
    xs = x[:, :rows]
    mu = xs.sum(1, keepdim=True) / HW
    var = ((xs * xs).sum(1, keepdim=True) / HW - mu * mu).clamp_min(0.0)
    r = 1.0 / torch.sqrt(var + eps)
    xh = (xs - mu) * r
    a = xh * gm + bt
    da = dy[:, :rows] * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))
    return dict(mu=mu, var=var, r=r, dgamma=(da * xh).sum((0, 1)), dbeta=da.sum((0, 1)))


# ---- the network with deep supervision on a float64 tape -------------------------------------------------------------------------------------------
class _Store16(torch.autograd.Function):
    """A tensor that lives in memory as fp16, in both passes: the value is rounded on the way forward, its gradient on the way back."""

    @staticmethod
    def forward(ctx, t):
        return t.to(torch.float16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.float16).to(g.dtype)


def store16(t):
    return _Store16.apply(t)


def weight16(t):
    """A parameter the kernels read as fp16 while its gradient stays fp32: rounded forward, the gradient passes as it is."""
    return t + (t.to(torch.float16).to(t.dtype) - t).detach()


def _block(sd, prefix, x, stride, slope, store, wstore):
    y = store(F.conv2d(x, wstore(sd[prefix + ".conv.weight"]), sd[prefix + ".conv.bias"], stride=stride, padding=1))
    y = F.instance_norm(y, weight=sd[prefix + ".norm.weight"], bias=sd[prefix + ".norm.bias"], eps=1e-5)
    return store(F.leaky_relu(y, slope))


def forward_deep_supervision(sd, spec, x, slope=0.01, storage16=False):
    """sd: float64 leaves (requires_grad as the caller set it) under nnunet.param_shapes(spec, deep_supervision=True).  x [B, C, H, W] float64.
    Returns the heads' logits [B, n_heads, h, w], highest resolution first.  storage16: every tensor a layer hands on is rounded to fp16, and so is its
    gradient on the way back (at whatever loss scale the caller multiplies the loss by); weights are read as fp16."""
    store = store16 if storage16 else (lambda t: t)
    wstore = weight16 if storage16 else (lambda t: t)
    h = x.to(torch.float16).to(x.dtype) if storage16 else x
    n = spec["n_stages"]
    skips = []
    for s in range(n):
        for i in range(spec["n_conv_encoder"][s]):
            h = _block(sd, f"encoder.stages.{s}.0.convs.{i}", h, spec["strides"][s] if i == 0 else 1, slope, store, wstore)
        skips.append(h)
    outs = []
    for j in range(n - 1):
        st = spec["strides"][n - 1 - j]
        up = store(F.conv_transpose2d(h, wstore(sd[f"decoder.transpconvs.{j}.weight"]), sd[f"decoder.transpconvs.{j}.bias"], stride=st))
        h = torch.cat((up, skips[n - 2 - j]), 1)
        for i in range(spec["n_conv_decoder"][j]):
            h = _block(sd, f"decoder.stages.{j}.convs.{i}", h, 1, slope, store, wstore)
        outs.append(store(F.conv2d(h, wstore(sd[f"decoder.seg_layers.{j}.weight"]), sd[f"decoder.seg_layers.{j}.bias"])))
    return outs[::-1]


def synthetic_state_dict(spec, seed):
    """nnunet_ref.synthetic_state_dict's recipe over the deep-supervision name set."""
    from ldiffusion_amd import nnunet
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in nnunet.param_shapes(spec, deep_supervision=True).items():
        if name.endswith("norm.weight"):
            t = 1.0 + 0.2 * torch.randn(shape, generator=g)
        elif name.endswith("bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif "transpconvs" in name:
            t = torch.randn(shape, generator=g) * (1.0 / shape[0]) ** 0.5
        else:
            t = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        sd[name] = t.to(torch.float16).float()
    return sd


def step_gradients(sd, spec, x, targets, weights, batch_dice, slope, storage16=False, loss_scale=1.0):
    """(loss, {name: d loss / d parameter}) in float64; a parameter the loss does not reach maps to None.  With storage16 the backward runs at `loss_scale`
    (the rounding of the stored gradients happens at that scale) and the result is unscaled."""
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    outs = forward_deep_supervision(leaves, spec, x.double(), slope, storage16)
    loss = deep_supervision_loss(outs, targets, weights, batch_dice)
    names = list(leaves)
    grads = torch.autograd.grad(loss * loss_scale, [leaves[k] for k in names], allow_unused=True)
    return float(loss.detach()), {k: (None if g is None else g / loss_scale) for k, g in zip(names, grads)}
