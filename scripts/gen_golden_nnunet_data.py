"""Generate tests/golden/nnunet_class_locations.npz by running the REFERENCE's own DefaultPreprocessor._sample_foreground_locations
(/root/reference/model/nnunetv2/preprocessing/preprocessors/default_preprocessor.py:152-178) on a 48 x 48 label map with three foreground classes, one of
them absent.  The module's imports (batchgenerators, tqdm, the rest of nnunetv2) are stubbed: the static method needs numpy alone.  Only the label map and
the recorded locations are committed; /root/reference is never read at test time."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/model/nnunetv2/preprocessing/preprocessors/default_preprocessor.py"


class _Stub(types.ModuleType):
    __all__ = []
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return object


for name in ["nnunetv2", "nnunetv2.paths", "nnunetv2.preprocessing", "nnunetv2.preprocessing.cropping", "nnunetv2.preprocessing.cropping.cropping",
             "nnunetv2.preprocessing.resampling", "nnunetv2.preprocessing.resampling.default_resampling", "nnunetv2.utilities",
             "nnunetv2.utilities.dataset_name_id_conversion", "nnunetv2.utilities.find_class_by_name", "nnunetv2.utilities.plans_handling",
             "nnunetv2.utilities.plans_handling.plans_handler", "nnunetv2.utilities.utils", "batchgenerators", "batchgenerators.utilities",
             "batchgenerators.utilities.file_and_folder_operations", "tqdm"]:
    sys.modules.setdefault(name, _Stub(name))
# `from batchgenerators.utilities.file_and_folder_operations import *` is where the module gets typing.List from
import typing  # noqa: E402
_ffo = sys.modules["batchgenerators.utilities.file_and_folder_operations"]
_ffo.List = typing.List
_ffo.__all__ = ["List"]

spec = importlib.util.spec_from_file_location("reference_default_preprocessor", REF)
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)

# blobs: class 1 a disc, class 3 a bar and a few single pixels, class 2 absent
yy, xx = np.mgrid[:48, :48]
seg = np.zeros((48, 48), np.uint8)
seg[(yy - 17) ** 2 + (xx - 20) ** 2 <= 81] = 1
seg[30:41, 5:44] = 3
seg[3, 40] = seg[45, 2] = seg[44, 46] = 3
classes = [1, 2, 3]
locs = mod.DefaultPreprocessor._sample_foreground_locations(seg[None, None], classes, seed=1234)   # [1, 1, H, W] as the preprocessor holds a 2-D case
out = {"seg": seg, "classes": np.array(classes)}
for c in classes:
    out[f"locations_{c}"] = np.asarray(locs[c], dtype=np.int64).reshape(-1, 4)
    print(c, out[f"locations_{c}"].shape)
path = os.path.join(ROOT, "tests", "golden", "nnunet_class_locations.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
