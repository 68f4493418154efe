"""Generate tests/golden/nnunet_class_locations_ignore.npz by running the REFERENCE's own DefaultPreprocessor._sample_foreground_locations
(model/nnunetv2/preprocessing/preprocessors/default_preprocessor.py:152-178) the way run_case_npy calls it for a dataset with an ignore label
(:96-107): the foreground classes, then one more entry, the list of ALL labels (background included) -- the annotated pixels.  Two 40 x 36 label maps with
three classes and the ignore label 3: `a` partly annotated (class 2 a few pixels only), `b` without any annotated pixel.  The module's imports are
stubbed as scripts/gen_golden_nnunet_data.py stubs them.  Only the label maps and the recorded locations are committed; the reference is never read
at test time.  usage: python scripts/gen_golden_nnunet_data_ignore.py <the reference's model/nnunetv2 folder>"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(sys.argv[1], "preprocessing", "preprocessors", "default_preprocessor.py")


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
import typing  # noqa: E402
_ffo = sys.modules["batchgenerators.utilities.file_and_folder_operations"]
_ffo.List = typing.List
_ffo.__all__ = ["List"]

spec = importlib.util.spec_from_file_location("reference_default_preprocessor", REF)
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)

N_HEADS, IGNORE, H, W = 3, 3, 40, 36
yy, xx = np.mgrid[:H, :W]
a = np.full((H, W), IGNORE, np.uint8)          # strokes on an unlabelled slide: a background region, a disc of class 1, three pixels of class 2
a[4:15, 3:30] = 0
a[(yy - 26) ** 2 + (xx - 14) ** 2 <= 49] = 1
a[8, 8] = a[30, 33] = a[38, 1] = 2
b = np.full((H, W), IGNORE, np.uint8)          # nothing annotated
foreground, all_labels = [1, 2], [0, 1, 2]
collect = foreground + [all_labels]            # run_case_npy :96-102
out = {"n_heads": np.int64(N_HEADS), "ignore": np.int64(IGNORE), "classes": np.array(foreground)}
for name, seg in (("a", a), ("b", b)):
    locs = mod.DefaultPreprocessor._sample_foreground_locations(seg[None, None], collect, seed=1234)   # [1, 1, H, W] as the preprocessor holds a 2-D case
    assert list(locs) == foreground + [tuple(all_labels)]
    out[f"{name}.seg"] = seg
    for key in locs:
        tag = "annotated" if isinstance(key, tuple) else str(key)
        out[f"{name}.locations_{tag}"] = np.asarray(locs[key], dtype=np.int64).reshape(-1, 4)
        print(name, key, out[f"{name}.locations_{tag}"].shape)
path = os.path.join(ROOT, "tests", "golden", "nnunet_class_locations_ignore.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
