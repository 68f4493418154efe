"""CPU (-m "not gpu"): the text encoder's host side -- config refusals, the checkpoint key map, the ctypes mirrors of what the ABI gained.
No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from ldiffusion_amd import _lib, models, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=77,
            hidden_act="quick_gelu", layer_norm_eps=1e-5)


@pytest.mark.parametrize("change, field", [
    (dict(hidden_act="relu"), "hidden_act"),
    (dict(hidden_size=64, num_attention_heads=3), "num_attention_heads"),
    (dict(hidden_size=64, num_attention_heads=8), "head dim"),            # d = 8: not a multiple of 16
    (dict(hidden_size=1152, num_attention_heads=8), "head dim"),          # d = 144 > 128
    (dict(hidden_size=96, num_attention_heads=2), "hidden_size"),         # d = 48 is fine, 96 is no multiple of 64
    (dict(max_position_embeddings=129), "max_position_embeddings"),
    (dict(intermediate_size=100), "intermediate_size"),
])
def test_config_refusals_name_their_field(change, field):
    """Validation happens in Python before the library is touched: each refusal is a ValueError naming the config field, raised by the
    validator and by the class alike (which therefore never reaches the GPU check)."""
    cfg = dict(GOOD, **change)
    with pytest.raises(ValueError, match=field):
        weights.clip_text_config(cfg)
    with pytest.raises(ValueError, match=field):
        models.CLIPTextModel(cfg, {})
    assert weights.clip_text_config(GOOD)["hidden_size"] == 64
    assert weights.clip_text_config({})["hidden_act"] == "quick_gelu"   # transformers' defaults fill a trimmed config.json


def test_attention_mask_is_refused_by_name():
    enc = object.__new__(models.CLIPTextModel)   # the argument check comes before anything that needs a handle
    with pytest.raises(ValueError, match="attention_mask"):
        enc(torch.zeros((1, 5), dtype=torch.long), attention_mask=torch.ones((1, 5)))
    enc._h = None


def test_every_state_dict_key_maps_to_one_loader_name():
    """The loader names are transformers' own keys: every key of CLIPTextModel(cfg).state_dict() maps to exactly one (position_ids, a buffer
    older versions save, is the one key that is dropped), with the shape the library expects, and the library expects nothing else."""
    from transformers import CLIPTextConfig, CLIPTextModel
    for act, heads, layers in (("quick_gelu", 4, 2), ("gelu", 1, 3)):
        cfg = CLIPTextConfig(vocab_size=50, hidden_size=64, intermediate_size=192, num_hidden_layers=layers, num_attention_heads=heads, max_position_embeddings=33,
                             hidden_act=act, bos_token_id=0, eos_token_id=1, pad_token_id=1)
        sd = CLIPTextModel(cfg).state_dict()
        shapes = weights.clip_text_param_shapes(cfg.to_dict())
        for layout in (sd, {"text_model." + k: v for k, v in sd.items()}):   # the installed transformers' keys, and the 4.x layout of the checkpoints in circulation
            names = [weights.clip_text_loader_name(k) for k in layout]
            kept = [n for n in names if n is not None]
            assert len(kept) == len(set(kept)) == len(shapes) and len(names) - len(kept) <= 1
            assert set(kept) == set(shapes), set(kept) ^ set(shapes)
            for k, v in layout.items():
                n = weights.clip_text_loader_name(k)
                assert n is None or tuple(v.shape) == shapes[n], k
            assert list(weights.normalize_clip_text_keys(layout)) == kept
    assert weights.clip_text_loader_name("text_model.embeddings.position_ids") is None and weights.clip_text_loader_name("embeddings.position_ids") is None
    with pytest.raises(ValueError, match="second time"):
        weights.normalize_clip_text_keys({"final_layer_norm.weight": torch.ones(64), "text_model.final_layer_norm.weight": torch.ones(64)})
    assert list(weights.clip_text_param_shapes(cfg.to_dict(), 40))[-2:] == ["proj.weight", "proj.bias"]
    assert weights.clip_text_param_shapes(cfg.to_dict(), 40)["proj.weight"] == (40, 64)


def test_abi_mirrors_of_the_text_encoder(tmp_path):
    """ldiff_conv_args gained act_out (last field, as the header appends it), and ldiff_textenc_cfg's ctypes mirror has the header's layout."""
    assert _lib.ConvArgs._fields_[-1] == ("act_out", C.c_int)
    fields = [f[0] for f in _lib.TextEncCfg._fields_]
    assert fields == ["vocab_size", "hidden", "intermediate", "layers", "heads", "max_positions", "act", "ln_eps"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ldiff.h"', 'int main(void) {', '  printf(". %zu\\n", sizeof(ldiff_textenc_cfg));']
    lines += [f'  printf("{f} %zu\\n", offsetof(ldiff_textenc_cfg, {f}));' for f in fields]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}"]))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["."]) == C.sizeof(_lib.TextEncCfg)
    for f in fields:
        assert int(got[f]) == getattr(_lib.TextEncCfg, f).offset, f
    hdr = open(os.path.join(ROOT, "include", "ldiff.h")).read()
    assert re.search(r"int act_out;", hdr) and "ldiff_textenc_forward" in _lib.SIGNATURES
