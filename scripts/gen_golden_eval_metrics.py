"""Generate tests/golden/reference_eval_metrics.json by running the REFERENCE's own `compute_metrics` (evaluation/evaluate_predictions.py:89-120) on a handful
of tiny (reference, prediction) label maps, loaded as scripts/gen_golden_dc_ce_loss_ignore.py loads its modules.
usage: python scripts/gen_golden_eval_metrics.py <the reference's model/nnunetv2 folder>

`evaluate_predictions` imports file helpers of `batchgenerators` and nnU-Net's readers and plans handling at module level; none of them takes part in
`compute_metrics`, so they are stubbed here, and the reader the function asks for is a small in-script object that hands out the arrays by name.
Cases: plain labels (two pairs), one pair with an ignore label, one with regions (tuples and a single label), one with a class absent from both masks
(Dice and IoU nan).  The file holds inputs and outputs only; the reference is never read at test time.  The pooled `compute_metrics_on_folder` and
`determine_postprocessing` cannot run in this setting (spawn pools; the second needs acvl_utils): ldiffusion_amd.nnunet_post restates them."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _unused(*a, **k):
    raise RuntimeError("a stubbed helper was called: compute_metrics should not need it")


for pkg in ["batchgenerators", "batchgenerators.utilities", "nnunetv2", "nnunetv2.imageio", "nnunetv2.utilities", "nnunetv2.utilities.plans_handling",
            "nnunetv2.evaluation"]:
    _stub(pkg)
_stub("batchgenerators.utilities.file_and_folder_operations", subfiles=_unused, join=os.path.join, save_json=_unused, load_json=_unused, isfile=os.path.isfile)
_stub("nnunetv2.configuration", default_num_processes=1)
_stub("nnunetv2.imageio.base_reader_writer", BaseReaderWriter=object)
_stub("nnunetv2.imageio.reader_writer_registry", determine_reader_writer_from_dataset_json=_unused, determine_reader_writer_from_file_ending=_unused)
_stub("nnunetv2.imageio.simpleitk_reader_writer", SimpleITKIO=object)
_stub("nnunetv2.utilities.json_export", recursive_fix_for_json_export=_unused)
_stub("nnunetv2.utilities.plans_handling.plans_handler", PlansManager=object)

spec = importlib.util.spec_from_file_location("nnunetv2.evaluation.evaluate_predictions", os.path.join(REF, "evaluation", "evaluate_predictions.py"))
ep = importlib.util.module_from_spec(spec)
sys.modules[spec.name] = ep
spec.loader.exec_module(ep)


class Reader:
    """read_seg(name) -> ([1, H, W] label map, properties), as a BaseReaderWriter answers."""

    def __init__(self):
        self.arrays = {}

    def read_seg(self, name):
        return self.arrays[name][None], {"spacing": (999, 1, 1)}


rng = np.random.RandomState(2024)


def blocks(h, w, values, cell=2):
    """A label map of cell x cell blocks drawn from `values`."""
    coarse = rng.choice(values, size=((h + cell - 1) // cell, (w + cell - 1) // cell))
    return np.kron(coarse, np.ones((cell, cell), np.int64))[:h, :w].astype(np.uint8)


def noisy(ref, values, p):
    out = ref.copy()
    flip = rng.rand(*ref.shape) < p
    out[flip] = rng.choice(values, size=int(flip.sum()))
    return out


CASES = []
ref = blocks(9, 11, [0, 1, 2, 3])
CASES.append(("plain_a", [1, 2, 3], None, ref, noisy(ref, [0, 1, 2, 3], 0.3)))
ref = blocks(8, 8, [0, 1, 2], cell=3)
CASES.append(("plain_b", [1, 2], None, ref, noisy(ref, [0, 1, 2], 0.5)))
ref = blocks(10, 7, [0, 1, 2, 3])   # 3 = the ignore label
CASES.append(("ignore", [1, 2], 3, ref, noisy(np.where(ref == 3, 1, ref).astype(np.uint8), [0, 1, 2], 0.3)))
ref = blocks(9, 9, [0, 1, 2, 3])
CASES.append(("regions", [(1, 2, 3), (2, 3), 3], None, ref, noisy(ref, [0, 1, 2, 3], 0.35)))
ref = blocks(7, 10, [0, 1, 2])
CASES.append(("absent", [1, 2, 3], None, ref, noisy(ref, [0, 1, 2], 0.25)))   # class 3 in neither mask: Dice and IoU nan

reader = Reader()
out = []
for name, lors, ignore, r, p in CASES:
    reader.arrays = {"ref": r, "pred": p}
    res = ep.compute_metrics("ref", "pred", reader, lors, ignore)
    metrics = {ep.label_or_region_to_key(k): {m: (float(v) if m in ("Dice", "IoU") else int(v)) for m, v in d.items()} for k, d in res["metrics"].items()}
    out.append({"name": name, "labels_or_regions": [list(k) if isinstance(k, tuple) else k for k in lors], "ignore_label": ignore, "ref": r.tolist(), "pred": p.tolist(),
                "metrics": metrics})
    print(name, {k: round(d["Dice"], 4) for k, d in metrics.items()})

path = os.path.join(ROOT, "tests", "golden", "reference_eval_metrics.json")
with open(path, "w") as f:
    json.dump(out, f)
print("wrote", path, os.path.getsize(path), "bytes")
