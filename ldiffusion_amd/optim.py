"""What follows a backward pass, each piece stated once: the dynamic loss-scale rule, the two clip coefficients, and the multi-tensor launches of
libldiff_hip.so (AdamW, SGD with Nesterov momentum, the gradient bucket, its norm).  No tape in here; the library is loaded on first use.
A multi-tensor launch reads three device tables (csrc/common.h): one row per tensor ({p, m, v, n}, {p, buf, n} or an offset), one gradient pointer per
tensor, and one AdamChunk {int32 tensor, int32 pad, int64 first} per workgroup of ADAMW_CHUNK elements.  Rows and chunks are built once per set of
live tensors and cached in the caller's state dict; only the gradient pointers are uploaded at every launch."""
from __future__ import annotations

import math
from itertools import accumulate

import torch

from . import _lib

ADAMW_CHUNK = 16384   # elements per workgroup of ldiff_op_adamw_multi (csrc/common.h)
LOSS_SCALE = 1024.0   # initial loss scale of the backward pass: activation gradients are stored in float16 (the reference trains in fp32,
                      # ldiffusion.py:172 `fp16.enabled: False`); unscaled, 0.5 % of the non-negligible parameter-gradient entries underflow to zero
LOSS_SCALE_GROWTH_INTERVAL = 200   # consecutive finite steps before a lowered loss scale doubles again (never above LOSS_SCALE)


def update_loss_scale(state, total) -> bool:
    """Dynamic loss scaling on `total`, the exchanged gradient norm (identical on every rank, so the decision is rank-uniform).  Non-finite: the
    caller skips the update (False) -- `state["loss_scale"]` is halved, never below 1, and the run of finite steps starts over.  Finite (True):
    after LOSS_SCALE_GROWTH_INTERVAL finite steps in a row a lowered scale doubles, up to the initial LOSS_SCALE -- one transient overflow must
    not pin the scale low for the rest of the run (the underflow LOSS_SCALE exists to avoid would come back)."""
    if not math.isfinite(total):
        state["skipped_steps"] = state.get("skipped_steps", 0) + 1
        state["loss_scale"] = max(1.0, state.get("loss_scale", LOSS_SCALE) * 0.5)
        state["finite_steps"] = 0
        return False
    state["finite_steps"] = state.get("finite_steps", 0) + 1
    if state["finite_steps"] >= LOSS_SCALE_GROWTH_INTERVAL and state.get("loss_scale", LOSS_SCALE) < LOSS_SCALE:
        state["loss_scale"] = min(LOSS_SCALE, state["loss_scale"] * 2.0)
        state["finite_steps"] = 0
    return True


def clip_coef_deepspeed(total, max_norm):
    """DeepSpeed's `gradient_clipping` (ldiffusion.py:187: 1.0): max_norm / max(global L2 norm, max_norm); 1 without a max_norm."""
    return 1.0 if max_norm is None else float(max_norm) / max(total, float(max_norm))


def clip_coef_torch(norm, max_norm):
    """torch's clip_grad_norm_: max_norm / (norm + 1e-6), at most 1."""
    return min(1.0, max_norm / (norm + 1e-6))


def chunk_list(sizes, chunk=ADAMW_CHUNK):
    """[(tensor, first)]: one entry per workgroup of a multi-tensor launch over tensors of `sizes` elements, `chunk` elements each."""
    return [(t, first) for t, n in enumerate(sizes) for first in range(0, int(n), chunk)]


def _tables(state, slot, specs, dev):
    """The cached device tables of a call's launches.  specs: per launch (key, make) -- `make()` gives the flat int64 per-tensor rows and the tensors'
    element counts.  A table is (key, rows on the device, chunks on the device, number of chunks); one whose key `state[slot]` already holds is
    reused, and `state[slot]` holds exactly this call's tables afterwards."""
    old, tabs = state.get(slot) or [], []
    for key, make in specs:
        tab = next((t for t in old if t[0] == key), None)
        if tab is None:
            rows, sizes = make()
            chunks = chunk_list(sizes)   # {int32 tensor, int32 pad} packed into one int64 (little endian), then int64 first
            tab = (key, torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(chunks, dtype=torch.int64).reshape(-1).to(dev), len(chunks))
        tabs.append(tab)
    state[slot] = tabs
    return tabs


def _grad_ptrs(grads, dev):
    """The gradient-pointer table of one launch, uploaded: (table, what must outlive the asynchronous launch)."""
    gs = [g.detach().to(torch.float32).contiguous() for g in grads]
    gptr = torch.tensor([g.data_ptr() for g in gs], dtype=torch.int64).to(dev)
    return gptr, (gs, gptr)


def _live(what, params, grads):
    """[(index, parameter, gradient)] of the tensors whose gradient is not None."""
    live = [(i, p, g) for i, (p, g) in enumerate(zip(params, grads)) if g is not None]
    if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for _, p, _ in live):
        raise ValueError(f"{what}: parameters must be contiguous float32 CUDA tensors")
    return live


def _launch_groups(state, groups, row, launch, keep):
    """One launch per (tag, members) of an optimizer step: `row(i, p)` is a tensor's row of the table, `launch(tag, rows, grads, chunks, nchunks)` the
    library call on the device tables.  `keep` (with the uploads added) outlives the asynchronous launches in state["_keep"]."""
    dev = groups[0][1][0][1].device
    specs = [(tuple((i, p.data_ptr(), p.numel()) for i, p, _ in m), lambda m=m: ([v for i, p, _ in m for v in row(i, p)], [p.numel() for _, p, _ in m]))
             for _, m in groups]
    for (tag, members), tab in zip(groups, _tables(state, "_tables", specs, dev)):
        gptr, alive = _grad_ptrs([g for _, _, g in members], dev)
        _lib.check(launch(tag, tab[1].data_ptr(), gptr.data_ptr(), tab[2].data_ptr(), tab[3]))
        keep.append(alive)
    state["_keep"] = keep


def adamw_step(params, grads, state, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
    """One AdamW update (torch.optim.AdamW semantics; the reference's DeepSpeed config, ldiffusion.py:168-171) of float32 CUDA
    parameters, in place, ALL tensors in one launch (ldiff_op_adamw_multi).  `state` is a dict the caller keeps: the step count, the two
    moment buffers per parameter and the device tables of the launch (parameter / moment pointers and the chunk list are built once;
    only the gradient pointers change from step to step).  As in torch, a tensor whose gradient is None is skipped and its own step count
    (the bias correction) does not advance; tensors whose counts differ are updated by one launch per count."""
    lib = _lib.load()
    live = _live("adamw_step", params, grads)
    if not live:
        return   # nothing to update: the bias-correction step count must not advance either
    state["step"] = state.get("step", 0) + 1
    steps = state.setdefault("_steps", {})   # per-tensor step counts
    groups = {}
    for i, p, g in live:
        if i not in state:
            state[i] = (torch.zeros_like(p), torch.zeros_like(p))
        steps[i] = steps.get(i, 0) + 1
        groups.setdefault(steps[i], []).append((i, p, g))
    _launch_groups(state, sorted(groups.items()), lambda i, p: (p.data_ptr(), state[i][0].data_ptr(), state[i][1].data_ptr(), p.numel()),
                   lambda step, rows, gptr, chunks, n: lib.ldiff_op_adamw_multi(rows, gptr, chunks, n, float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                                                float(weight_decay), int(step), _lib.stream_ptr()), [])


def sgd_nesterov_step(params, grads, state, lr, weight_decay=0.0, momentum=0.99, inv_scale=1.0, clip_coef=1.0):
    """One torch.optim.SGD(momentum, nesterov=True, weight_decay) update of float32 CUDA parameters, in place, all tensors in one launch
    (ldiff_op_sgd_nesterov_multi; a second launch for tensors that meet their first gradient later than the others: their buffer starts as g).
    The gradient enters as inv_scale * clip_coef * grad: floats, or float32 device scalars (0-dim / 1-element tensors, read by the kernel).
    As in torch, a tensor whose gradient is None is left untouched: no weight decay, no buffer.  `state` is the caller's dict: momentum buffers
    by parameter index, the device tables."""
    lib = _lib.load()
    live = _live("sgd_nesterov_step", params, grads)
    if not live:
        return

    def scalar(name, v):
        if torch.is_tensor(v):
            if not (v.is_cuda and v.dtype == torch.float32 and v.numel() == 1):
                raise ValueError(f"sgd_nesterov_step: {name} must be a float or a float32 CUDA scalar")
            return v
        return torch.tensor([float(v)], dtype=torch.float32, device=live[0][1].device)

    s_inv, s_clip = scalar("inv_scale", inv_scale), scalar("clip_coef", clip_coef)
    bufs = state.setdefault("momentum_buffer", {})
    groups = {0: [], 1: []}   # 1: the tensors that meet their first gradient
    for i, p, g in live:
        groups[int(i not in bufs)].append((i, p, g))
        if i not in bufs:
            bufs[i] = torch.empty_like(p)
    _launch_groups(state, [(f, m) for f, m in groups.items() if m], lambda i, p: (p.data_ptr(), bufs[i].data_ptr(), p.numel()),
                   lambda first, rows, gptr, chunks, n: lib.ldiff_op_sgd_nesterov_multi(rows, gptr, chunks, n, float(lr), float(momentum), float(weight_decay), first,
                                                                                        s_inv.data_ptr(), s_clip.data_ptr(), _lib.stream_ptr()), [s_inv, s_clip])
    state["step"] = state.get("step", 0) + 1


def bucket_pack(grads, state=None, out=None):
    """ldiff_op_bucket_pack: the float32 CUDA gradients that are not None, flattened in order into one buffer in ONE launch (torch.cat's result).
    `state`: a dict the caller keeps; the offset and chunk tables are built once per set of sizes.  Returns (bucket, offsets): offsets[j] is the start of
    the j-th live gradient, offsets[-1] the length."""
    lib = _lib.load()
    live = [g for g in grads if g is not None]
    if not live:
        raise ValueError("bucket_pack: no gradient")
    dev = live[0].device
    if not all(g.is_cuda and g.dtype == torch.float32 for g in live):
        raise ValueError("bucket_pack: gradients must be float32 CUDA tensors")
    key = tuple(g.numel() for g in live)
    offsets = [0, *accumulate(key)]
    state = state if state is not None else {}
    (tab,) = _tables(state, "_pack", [(key, lambda: (offsets, key))], dev)
    if out is None:
        out = torch.empty(offsets[-1], dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == offsets[-1]):
        raise ValueError(f"bucket_pack: out must be a contiguous float32 CUDA tensor of {offsets[-1]} elements")
    gptr, alive = _grad_ptrs(live, dev)
    _lib.check(lib.ldiff_op_bucket_pack(gptr.data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), tab[3], out.data_ptr(), _lib.stream_ptr()))
    state["_pack_keep"] = alive   # the launch is asynchronous
    return out, offsets


SUMSQ_CHAIN = 27   # dependent fp32 roundings on the longest path into one partial of ldiff_op_sumsq (csrc/kernels_segtrain.hip: 16 + 1 + 2 + 6 + 2)


def sumsq_plan(n):
    """(chain, partials) of ldiff_op_sumsq on n elements: fp32 roundings per partial, and the most partials the double finalize adds."""
    return SUMSQ_CHAIN, max(1, (((int(n) + 3) // 4) + ADAMW_CHUNK // 4 - 1) // (ADAMW_CHUNK // 4))


def sumsq(x, out=None):
    """ldiff_op_sumsq: sqrt(sum x^2) of a contiguous float32 CUDA tensor as a float32 device scalar [1] (no read-back here)."""
    lib = _lib.load()
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() >= 1):
        raise ValueError("sumsq: a non-empty contiguous float32 CUDA tensor is expected")
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=x.device)
    nb = lib.ldiff_op_sumsq_ws_bytes(x.numel())
    ws = torch.empty(nb // 4, dtype=torch.float32, device=x.device)
    _lib.check(lib.ldiff_op_sumsq(x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), nb, _lib.stream_ptr()))
    return out
