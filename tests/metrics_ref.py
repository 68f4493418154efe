"""Shared by tests/test_cpu_metrics.py and tests/test_gpu_metrics.py: the cases of tests/golden/reference_metrics.json rebuilt from their seeds, the
numpy confusion matrix every device count is compared with, and the comparison of a metric record with the reference's recorded values."""
import json
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_metrics.json")


def fixture_cases():
    """(case, logits, target) of the fixture, rebuilt from the seeds exactly as tests/test_cpu_oracle.py does."""
    with open(GOLD) as f:
        fx = json.load(f)
    out = []
    for c in fx["metrics"]:
        B, Cc, H, W = c["shape"]
        g = torch.Generator().manual_seed(c["seed"])
        logits = torch.randn((B, Cc, H, W), generator=g)
        target = torch.randint(0, Cc, (B, H, W), generator=g)
        if c["force_class0"]:
            target[:] = 0
            logits[:, 0] += 100
        out.append((c, logits, target))
    return out


def numpy_confusion(pred, target, n):
    """[n, n] int64, rows = targets; labels outside [0, n) are in no cell."""
    pred, target = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(target).reshape(-1).astype(np.int64)
    ok = (pred >= 0) & (pred < n) & (target >= 0) & (target < n)
    return np.bincount(target[ok] * n + pred[ok], minlength=n * n).reshape(n, n)


def check_against_fixture(c, m):
    assert m.dice_per_class.dtype == np.float32
    assert m.dice_per_class.tolist() == pytest.approx(c["dice_per_class"], abs=1e-7) and m.dice == pytest.approx(c["dice"], abs=1e-7)
    assert m.miou == pytest.approx(c["miou"], abs=1e-12)
    want = {int(k): v for k, v in c["iou_per_class"].items()}
    assert {k for k, v in m.iou_per_class.items() if v is None} == {k for k, v in want.items() if v is None}
    for k, v in want.items():
        assert v is None or m.iou_per_class[k] == pytest.approx(v, abs=1e-12)
    assert m.pixel_accuracy == pytest.approx(c["pixel_accuracy"], abs=1e-12)
    assert m.fw_iou == pytest.approx(c["fw_iou"], abs=1e-7)
