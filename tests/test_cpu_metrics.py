"""CPU (-m "not gpu"): the host half of mask scoring -- `ldiff_seg_metrics` (the reference's four metrics from one confusion matrix) against the
reference's recorded values (tests/golden/reference_metrics.json, written by the reference's own python), its edge rules and refusals, the label
LUTs, the struct mirror's layout and `parallel.reduce_confusion` on two gloo ranks.  No kernel is launched here.

Tolerances are those tests/test_cpu_oracle.py already uses against the same file: 1e-7 for Dice and the frequency-weighted IoU (float32 arithmetic),
1e-12 for the mean IoU and the pixel accuracy (double), None for exactly the recorded classes."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from ldiffusion_amd import _lib, metrics, parallel
from metrics_ref import check_against_fixture, fixture_cases, numpy_confusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "reference_metrics.json")


def test_seg_metrics_reproduce_the_references_recorded_values(lib):
    cases = fixture_cases()
    assert [tuple(c["shape"]) for c, _, _ in cases] == [(1, 7, 32, 32), (2, 6, 17, 23), (1, 11, 8, 8), (1, 3, 4, 4)]
    for c, logits, target in cases:
        n = c["shape"][1]
        conf = numpy_confusion(torch.argmax(logits, 1).numpy(), target.numpy(), n)
        assert conf.sum() == target.numel()
        check_against_fixture(c, metrics.from_confusion(conf))
        check_against_fixture(c, metrics.from_confusion(torch.from_numpy(conf)))
    # case 3 (force_class0): classes 1 and 2 are absent from target and prediction -> Dice 1, IoU None, pixel accuracy 1
    m = metrics.from_confusion(numpy_confusion(torch.argmax(cases[3][1], 1).numpy(), cases[3][2].numpy(), 3))
    assert m.dice_per_class.tolist() == [1.0, 1.0, 1.0] and m.iou_per_class == {0: 1.0, 1: None, 2: None} and m.pa_per_class == [1.0, 1.0, 1.0]


def test_seg_metrics_edge_rules(lib):
    # rows = targets.  class 0: 5 right, 1 taken for class 1; class 1: 2 right, 3 taken for class 0; class 2: in neither
    conf = np.array([[5, 1, 0], [3, 2, 0], [0, 0, 0]], np.int64)
    m = metrics.from_confusion(conf)
    f = np.float32
    hist = conf.astype(f)
    freq = hist.sum(1) / hist.sum()
    iu = np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist) + f(1e-10))
    assert iu.dtype == f and freq.dtype == f
    assert m.fw_iou == pytest.approx(float((freq * iu).sum()), abs=1e-7)
    assert m.fw_iou_fg == pytest.approx(float((freq[1:] * iu[1:]).sum()), abs=1e-7)      # ignore_background: class 0 left out, freq NOT renormalised
    assert m.fw_iou_fg == pytest.approx((5 / 11) * (2 / 6), abs=1e-7) and m.fw_iou == pytest.approx((6 / 11) * (5 / 9) + (5 / 11) * (2 / 6), abs=1e-7)
    assert m.dice_per_class.tolist() == pytest.approx([10 / 14, 4 / 8, 1.0], abs=1e-7) and m.dice == pytest.approx((10 / 14 + 0.5 + 1) / 3, abs=1e-7)
    assert m.iou_per_class == {0: 5 / 9, 1: 2 / 6, 2: None} and m.miou == pytest.approx((5 / 9 + 2 / 6) / 2, abs=1e-12)
    assert m.pa_per_class == [5 / 6, 2 / 5, 1.0] and m.pixel_accuracy == pytest.approx((5 / 6 + 2 / 5 + 1) / 3, abs=1e-12)
    # a class present in the target only: Dice 0, IoU 0, accuracy 0 (not the "absent" rule)
    m = metrics.from_confusion(np.array([[0, 4], [0, 0]], np.int64))
    assert m.dice_per_class.tolist() == [0.0, 0.0] and m.iou_per_class == {0: 0.0, 1: 0.0} and m.pa_per_class == [0.0, 1.0]
    # the empty matrix: every class absent -> Dice 1, IoU all skipped -> 1.0, accuracy 1, and the reference's float32 0 / 0 for the weighted IoU
    m = metrics.from_confusion(np.zeros((4, 4), np.int64))
    assert m.dice == 1.0 and m.miou == 1.0 and set(m.iou_per_class.values()) == {None} and m.pixel_accuracy == 1.0
    assert math.isnan(m.fw_iou) and math.isnan(m.fw_iou_fg)
    # both ends of the class range, and a stack of matrices is scored as their sum (the reference flattens the batch)
    m = metrics.from_confusion(np.array([[9]], np.int64))
    assert (m.dice, m.miou, m.pixel_accuracy, m.fw_iou, m.fw_iou_fg) == (1.0, 1.0, 1.0, 1.0, 0.0)
    big = np.arange(32 * 32, dtype=np.int64).reshape(32, 32)
    m = metrics.from_confusion(np.stack([big, 2 * big]))
    assert m.num_classes == 32 and m.pa_per_class[31] == pytest.approx(3 * 1023 / (3 * big[31].sum()), abs=1e-12)


def test_seg_metrics_and_confusion_refuse_bad_class_counts(lib):
    rec = _lib.SegMetricsOut()
    buf = (C.c_int64 * (33 * 33))()
    for bad in (0, 33, -1):
        assert lib.ldiff_seg_metrics(buf, bad, C.byref(rec)) == -1 and b"class count" in lib.ldiff_last_error()
        # nothing is enqueued (there is no device here to enqueue on): the class count is refused before anything else is looked at
        assert lib.ldiff_confusion(None, 0, None, 0, None, None, 1, bad, 4, 4, None, None, None) == -1 and b"class count" in lib.ldiff_last_error()
    assert lib.ldiff_seg_metrics(None, 3, C.byref(rec)) == -1 and lib.ldiff_seg_metrics(buf, 3, None) == -1
    buf[4] = -1
    assert lib.ldiff_seg_metrics(buf, 3, C.byref(rec)) == -1 and b"negative" in lib.ldiff_last_error()
    assert lib.ldiff_confusion(None, 3, None, 0, None, None, 1, 7, 4, 4, None, None, None) == -1 and b"pred_kind" in lib.ldiff_last_error()
    assert lib.ldiff_confusion(None, 0, None, 2, None, None, 1, 7, 4, 4, None, None, None) == -1 and b"target_kind" in lib.ldiff_last_error()
    lut = (C.c_uint8 * 256)()
    assert lib.ldiff_confusion(None, 0, None, 1, None, lut, 1, 7, 4, 4, None, None, None) == -1 and b"LUT" in lib.ldiff_last_error()
    with pytest.raises(ValueError):
        metrics.from_confusion(np.zeros((33, 33), np.int64))
    with pytest.raises(ValueError):
        metrics.from_confusion(np.zeros((3, 4), np.int64))
    with pytest.raises(ValueError):
        metrics.from_confusion(np.zeros((3, 3), np.float32))


def test_label_luts_equal_the_references_tables():
    with open(GOLD) as f:
        luts = json.load(f)["luts"]
    for level, key in (("tissue", "pixel_to_label"), ("cell", "pixel_to_label_cell")):
        lut = metrics.label_lut(level)
        assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256,)
        want = np.zeros(256, np.uint8)
        for grey, label in luts[key].items():
            want[int(grey)] = label
        assert np.array_equal(lut.numpy(), want)                 # 0 elsewhere, as convert_labels leaves unlisted grey levels
    with pytest.raises(ValueError):
        metrics.label_lut("organ")


def test_seg_metrics_struct_mirror_has_the_headers_layout(tmp_path):
    """ldiff_seg_metrics_out against _lib.SegMetricsOut: same size, same offsets, same field order, as gcc lays the header out."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldiff.h")).read(), flags=re.S)
    body = re.search(r"typedef struct ldiff_seg_metrics_out\s*{([^}]*)}\s*ldiff_seg_metrics_out\s*;", hdr).group(1)
    names = [re.search(r"(\w+)\s*(?:\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    fields = [f[0] for f in _lib.SegMetricsOut._fields_]
    assert names == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ldiff.h"', 'int main(void) {', '  printf(". %zu\\n", sizeof(ldiff_seg_metrics_out));']
    lines += [f'  printf("{n} %zu\\n", offsetof(ldiff_seg_metrics_out, {n}));' for n in fields]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}"]))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["."]) == C.sizeof(_lib.SegMetricsOut)
    for n in fields:
        assert int(got[n]) == getattr(_lib.SegMetricsOut, n).offset, n


def test_reduce_confusion_is_the_identity_without_a_group():
    conf = torch.arange(2 * 3 * 3, dtype=torch.int64).view(2, 3, 3)
    assert parallel.reduce_confusion(conf) is conf and torch.equal(conf, torch.arange(18).view(2, 3, 3))


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
from ldiffusion_amd import parallel
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
assert world == 2
def matrix(r):                                          # what rank r counted: every rank can rebuild both
    g = torch.Generator().manual_seed(100 + r)
    return torch.randint(0, 1 << 40, (3, 7, 7), generator=g, dtype=torch.int64)
mine = matrix(rank)
got = parallel.reduce_confusion(mine)
assert got is mine and got.dtype == torch.int64 and torch.equal(got, matrix(0) + matrix(1)), rank
try:
    parallel.reduce_confusion(torch.zeros((2, 2), dtype=torch.int32))
    raise SystemExit("expected ValueError")
except ValueError:
    pass
dist.barrier()
dist.destroy_process_group()
open(os.path.join({out!r}, "rank%d.ok" % rank), "w").write("ok")
"""


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_reduce_confusion_world_size_2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, out=str(tmp_path)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "rank0.ok").exists() and (tmp_path / "rank1.ok").exists(), r.stdout[-2000:] + r.stderr[-2000:]
