"""Generate tests/golden/reference_fold_ensemble.npz by running the REFERENCE's own fold ensemble
(/root/reference/model/nnunetv2/inference/predict_from_raw_data.py:459-494 `predict_logits_from_preprocessed_data`: per entry of `list_of_parameters`
`network.load_state_dict`, the sliding window, `prediction += ...` on the float16 logits, then `prediction /= len(list_of_parameters)`) over three state
dicts of a tiny stand-in head, with `_internal_predict_sliding_window_return_logits` and `_internal_maybe_mirror_and_predict` underneath, in the build
container, the absent third-party imports stubbed as in scripts/gen_golden_sliding_window.py.  Only inputs, the per-fold weights and the output logits are
committed; /root/reference is never read at test time."""
import importlib.util
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/model"


class _Stub(MagicMock):
    pass


for name in ["acvl_utils", "acvl_utils.cropping_and_padding", "acvl_utils.cropping_and_padding.padding", "batchgenerators",
             "batchgenerators.dataloading", "batchgenerators.dataloading.multi_threaded_augmenter", "batchgenerators.utilities",
             "batchgenerators.utilities.file_and_folder_operations", "nnunetv2.configuration", "nnunetv2.inference.data_iterators",
             "nnunetv2.inference.export_prediction", "nnunetv2.utilities.file_path_utilities", "nnunetv2.utilities.find_class_by_name",
             "nnunetv2.utilities.helpers", "nnunetv2.utilities.json_export", "nnunetv2.utilities.label_handling",
             "nnunetv2.utilities.label_handling.label_handling", "nnunetv2.utilities.plans_handling",
             "nnunetv2.utilities.plans_handling.plans_handler", "nnunetv2.utilities.utils", "cv2", "tifffile", "nnunetv2.paths", "torchvision", "torchvision.transforms",
             "torchvision.models", "torchvision.models.segmentation", "torchvision.models.segmentation.deeplabv3"]:
    if name not in sys.modules:
        sys.modules[name] = _Stub()
for pkg, path in [("nnunetv2", REF + "/nnunetv2"), ("nnunetv2.inference", REF + "/nnunetv2/inference"), ("nnunetv2.utilities", REF + "/nnunetv2/utilities")]:
    m = types.ModuleType(pkg)
    m.__path__ = [path]
    sys.modules[pkg] = m


def _load(modname, path):
    spec = importlib.util.spec_from_file_location(modname, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


sw = _load("nnunetv2.inference.sliding_window_prediction", REF + "/nnunetv2/inference/sliding_window_prediction.py")
sys.modules["nnunetv2.utilities.helpers"].empty_cache = lambda d: None
sys.modules["nnunetv2.utilities.helpers"].dummy_context = __import__("contextlib").nullcontext
pr = _load("nnunetv2.inference.predict_from_raw_data", REF + "/nnunetv2/inference/predict_from_raw_data.py")
pr.default_num_processes = 8          # the stubbed nnunetv2.configuration has no number to compare the thread count with
P = pr.nnUNetPredictor

C_IN, C_OUT, FOLDS = 3, 4, 3


class Head(torch.nn.Module):
    """[1, C_IN, h, w] -> [1, C_OUT, h, w]: a 1x1 conv with integer weights (exact in fp32 on any device) plus a column ramp of the fold's own slope;
    NOT mirror-equivariant, so TTA changes the result.  tests/fold_ensemble_ref.py `stand_in_network` restates it."""

    def __init__(self):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(C_OUT, C_IN))
        self.slope = torch.nn.Parameter(torch.zeros(()))

    def forward(self, x):
        ramp = torch.arange(x.shape[-1], dtype=torch.float32, device=x.device) * self.slope
        return torch.einsum("oc,bchw->bohw", self.weight, x.float()) + ramp[None, None, None, :]


g = torch.Generator().manual_seed(5)
params = [{"weight": torch.randint(-3, 4, (C_OUT, C_IN), generator=g).float(), "slope": torch.tensor(0.125 * (k + 1))} for k in range(FOLDS)]

out = {}
inexact = 0
for tag, (H, Wd, tile, step, mirror) in {"a": (40, 56, (32, 32), 0.5, (0, 1)), "b": (64, 64, (32, 32), 1.0, None), "c": (33, 70, (32, 32), 0.5, (1,))}.items():
    data = torch.randint(0, 16, (C_IN, H, Wd), generator=g).float()      # integer-valued "image"
    fake = types.SimpleNamespace(
        network=Head(), device=torch.device("cpu"), verbose=False, allow_tqdm=False, use_gaussian=True, use_mirroring=mirror is not None,
        allowed_mirroring_axes=mirror, tile_step_size=step, perform_everything_on_device=True, list_of_parameters=params,
        configuration_manager=types.SimpleNamespace(patch_size=list(tile)), label_manager=types.SimpleNamespace(num_segmentation_heads=C_OUT))
    fake._internal_maybe_mirror_and_predict = lambda x, f=fake: P._internal_maybe_mirror_and_predict(f, x)
    # predict_sliding_window_return_logits without its padding step (acvl_utils is absent, and no case is smaller than the tile)
    fake.predict_sliding_window_return_logits = lambda d, f=fake: P._internal_predict_sliding_window_return_logits(
        f, d, P._internal_get_sliding_window_slicers(f, d.shape[1:]), True)
    data4 = data[:, None]                                    # nnU-Net's 2-D configurations carry a dummy z axis: [C, 1, H, W]
    with torch.no_grad():
        logits = P.predict_logits_from_preprocessed_data(fake, data4)[:, 0]
        single = []
        for p in params:
            fake.network.load_state_dict(p)
            single.append(fake.predict_sliding_window_return_logits(data4)[:, 0])
    assert logits.dtype == torch.half
    for k, s in enumerate(single):
        assert not torch.equal(s, logits), f"case {tag}: the ensemble equals fold {k}"
    total = single[0].clone()
    for s in single[1:]:
        total += s
    inexact_here = int(((total.double() / FOLDS).half().double() != total.double() / FOLDS).sum())
    inexact += inexact_here
    out[f"{tag}_image"] = data.numpy()
    out[f"{tag}_logits_f16"] = logits.numpy()
    out[f"{tag}_cfg"] = np.array([tile[0], tile[1], step, -1 if mirror is None else sum(1 << m for m in mirror)], np.float64)
    print(tag, tuple(data.shape), "logits", tuple(logits.shape), float(logits.float().abs().max()), "sum / 3 not representable at", inexact_here, "elements")
assert inexact > 0, "no element exercises the rounding of the last division"
out["fold_weights"] = torch.stack([p["weight"] for p in params]).numpy()
out["fold_slopes"] = torch.stack([p["slope"] for p in params]).numpy()
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "reference_fold_ensemble.npz"), **out)
print("wrote reference_fold_ensemble.npz")
