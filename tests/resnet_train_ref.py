"""The cell head's instance classifier in TRAINING mode, restated in plain torch on top of tests/resnet_ref.py (helper of the cell-training tests; TEST
INFRASTRUCTURE ONLY).

Every BatchNorm of the trunk normalises with the statistics of the batch it is given (F.batch_norm(..., training=True), eps 1e-5) and moves its running
statistics with momentum 0.1 and the unbiased batch variance, as torch.nn.BatchNorm2d does in `.train()`; the adapter conv, the pooling and the linear head
are those of the eval-mode restatement.  `store` is resnet_ref's hook: `resnet_ref.fp16_storage` makes it the fp16-storage model (float64 arithmetic, every
tensor a module hands on rounded to fp16 once).

`bn_layout(layers, width)` is the order the library reports (ResNetClassifier.bn_layout): the stem's BatchNorm, then per block bn1, bn2, bn3 and, in a layer's
first block, downsample.1 behind them; offsets on one flat channel axis."""
import torch
import torch.nn.functional as F

from resnet_ref import EPS

MOMENTUM = 0.1


def bn_layout(layers, width):
    """[(checkpoint prefix, offset, channels)] and the total T."""
    out, off = [], 0

    def add(prefix, ch):
        nonlocal off
        out.append((prefix, off, ch))
        off += ch

    add("encoder.1", width)
    for li, nblocks in enumerate(layers):
        planes = width << li
        for b in range(nblocks):
            p = f"encoder.{4 + li}.{b}"
            add(p + ".bn1", planes)
            add(p + ".bn2", planes)
            add(p + ".bn3", 4 * planes)
            if b == 0:
                add(p + ".downsample.1", 4 * planes)
    return out, off


def forward_train(sd, layers, x, dtype=torch.float64, store=None, momentum=MOMENTUM):
    """x [B, 3, S, S] -> dict(features [B, A], logits [B, C], mean [T], var [T] (UNBIASED batch variance), running: name -> tensor (the running statistics and
    num_batches_tracked after this forward)), all of it in `dtype` but the counters."""
    store = store or (lambda t: t)
    width = sd["encoder.0.weight"].shape[0]
    layout, T = bn_layout(layers, width)
    offs = {p: (o, c) for p, o, c in layout}
    mean, var = torch.zeros(T, dtype=dtype), torch.zeros(T, dtype=dtype)
    running = {}
    counters = {k: v for k, v in sd.items() if k.endswith("num_batches_tracked")}
    sd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}

    def conv(p, t, stride, pad):
        return store(F.conv2d(t, store(sd[p + ".weight"]), sd.get(p + ".bias"), stride=stride, padding=pad))

    def bn(p, t):
        o, c = offs[p]
        mean[o:o + c] = t.mean((0, 2, 3))
        var[o:o + c] = t.var((0, 2, 3), unbiased=True)
        rm, rv = sd[p + ".running_mean"].clone(), sd[p + ".running_var"].clone()
        y = F.batch_norm(t, rm, rv, sd[p + ".weight"], sd[p + ".bias"], True, momentum, EPS)   # (moves rm / rv in place, as the module does)
        running[p + ".running_mean"], running[p + ".running_var"] = rm, rv
        running[p + ".num_batches_tracked"] = counters.get(p + ".num_batches_tracked", torch.zeros((), dtype=torch.int64)).to(torch.int64) + 1
        return store(y)

    h = store(x.to(dtype))
    h = store(F.relu(bn("encoder.1", conv("encoder.0", h, 2, 3))))
    h = F.max_pool2d(h, 3, 2, 1)
    for li, nblocks in enumerate(layers):
        for b in range(nblocks):
            p = f"encoder.{4 + li}.{b}"
            stride = 2 if (b == 0 and li > 0) else 1
            t = store(F.relu(bn(p + ".bn1", conv(p + ".conv1", h, 1, 0))))
            t = store(F.relu(bn(p + ".bn2", conv(p + ".conv2", t, stride, 1))))
            t = bn(p + ".bn3", conv(p + ".conv3", t, 1, 0))
            idn = h
            if p + ".downsample.0.weight" in sd:
                idn = bn(p + ".downsample.1", conv(p + ".downsample.0", h, stride, 0))
            h = store(F.relu(t + idn))
    h = conv("adapter", h, 1, 1)
    feat = store(h.mean((2, 3)))
    return dict(features=feat, logits=F.linear(feat, sd["classifier.weight"], sd["classifier.bias"]), mean=mean, var=var, running=running)


def train_loop(sd, layers, images, fit_classifier, epochs, lr, dtype=torch.float64):
    """The trainer's own loop on the restatement: `images` = list of (crops [N, 3, S, S] or None for an image without instances, targets [N] int64).  Per image
    one training-mode forward, the running-statistics update and, with fit_classifier, one AdamW step on classifier.{weight, bias} with the cross-entropy over
    the targets >= 1.  Returns (state dict after the loop, per-epoch mean cross-entropy, the first image's cross-entropy in front of any update)."""
    sd = {k: v.clone() for k, v in sd.items()}
    W = sd["classifier.weight"].to(dtype).clone().requires_grad_(True)
    b = sd["classifier.bias"].to(dtype).clone().requires_grad_(True)
    opt = torch.optim.AdamW([W, b], lr=lr)
    means, first = [], None
    cache = {}
    for _ in range(epochs):
        losses = []
        for i, (crops, targets) in enumerate(images):
            if crops is None:
                continue
            if i not in cache:   # (no trunk weight moves: the features and the batch statistics of an image never change)
                cache[i] = forward_train(sd, layers, crops, dtype)
            out = cache[i]
            layout, _ = bn_layout(layers, sd["encoder.0.weight"].shape[0])
            for p, o, c in layout:
                for name, batch in (("running_mean", out["mean"]), ("running_var", out["var"])):
                    sd[f"{p}.{name}"] = MOMENTUM * batch[o:o + c] + (1 - MOMENTUM) * sd[f"{p}.{name}"].to(dtype)
                k = f"{p}.num_batches_tracked"
                sd[k] = sd.get(k, torch.zeros((), dtype=torch.int64)) + 1
            sel = targets >= 1
            if fit_classifier and bool(sel.any()):
                opt.zero_grad()
                loss = F.cross_entropy(out["features"][sel].detach() @ W.t() + b, targets[sel])
                loss.backward()
                opt.step()
                losses.append(loss.item())
                first = loss.item() if first is None else first
        means.append(sum(losses) / len(losses) if losses else 0.0)
    sd["classifier.weight"], sd["classifier.bias"] = W.detach().clone(), b.detach().clone()
    return sd, means, first
