"""-m "not gpu": the forward-attention error bound of tests/attention_bound.py, judged on the CPU where its verdicts are known.

On peaky rows (regime R2: N(0, 1) scores plus one key 7 - 12 nats higher in the first key tile, d = 40, 4,096 and 16,384 keys) the bound must
accept torch's fp32 SDPA and an emulated online softmax, and reject the emulated fixed-reference arithmetic attn<40,fixref> had (first tile's
maximum + 4 binades, P packed toward zero into fp16, row sum from the same rounded P).  The same arithmetic with P rounded to nearest, the
kernel's current form, must pass."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_bound as ab


@pytest.mark.parametrize("Lk", [4096, 16384])
def test_bound_on_peaky_rows(Lk):
    d, rows = 40, 48
    q, k, v = (t[0] for t in ab.make_operands(1, 1, 1, rows, Lk, d, "R2", Lk))
    scale = 1.0 / math.sqrt(d)
    o, tol = ab.reference(q, k, v, scale, "attn<40,fixref>")
    verdicts = {
        "fp32 SDPA": ab.ratio(F.scaled_dot_product_attention(q[None], k[None], v[None])[0].half(), o, tol),
        "online softmax, fp32 row sums": ab.ratio(ab.online_emulation(q, k, v, scale), o, tol),
        "online softmax, rounded-P row sums": ab.ratio(ab.online_emulation(q, k, v, scale, ones=True), o, tol),
        "fixed reference, P to nearest": ab.ratio(ab.fixref_emulation(q, k, v, scale, rtz=False).half(), o, tol),
    }
    fixref_rtz = ab.ratio(ab.fixref_emulation(q, k, v, scale), o, tol)
    print(f"[attn-bound] Lk={Lk}: " + ", ".join(f"{n} {r:.3f}" for n, r in verdicts.items()) + f"; fixed reference, P toward zero {fixref_rtz:.3f}")
    for n, r in verdicts.items():
        assert r <= 1.0, f"Lk={Lk}: the bound rejects {n} ({r:.3f} of it)"
    assert fixref_rtz > 1.0, f"Lk={Lk}: the bound accepts the round-toward-zero fixed-reference arithmetic ({fixref_rtz:.3f} of it)"
    for name, wo, wt in ab.wrong_references(q, k, v, scale, "attn<40,fixref>"):
        assert ab.ratio(o, wo, wt) > 1.0, f"Lk={Lk}: the bound does not reject the wrong reference '{name}'"


def test_kernel_classification():
    """w = |v - o| exactly where the row sum comes from the rounded P (launch_attn_cfg: d < DV; attn<40,fixref>'s ones row)."""
    assert ab.ones_row_sum("attn<40,fixref>", 40) and ab.ones_row_sum("attn<64,48>", 40) and ab.ones_row_sum("attn<32,16>", 8)
    assert not ab.ones_row_sum("attn<96,80>", 80) and not ab.ones_row_sum("attn<160,160>", 160) and not ab.ones_row_sum("attn<64,48>", 48)
    assert not ab.ones_row_sum("xattn<short-kv>", 40) and not ab.ones_row_sum("attn<512,128q>", 512) and not ab.ones_row_sum("attn<512,512>", 256)
    assert ab.key_tile("attn<512,128q>", 4096) == 32 and ab.key_tile("attn<40,fixref>", 4096) == 64 and ab.key_tile("xattn<short-kv>", 6) == 6


def test_rtz_pack_emulation():
    """_rtz16 is fp16 rounding toward zero with subnormals kept, and an overflow clamps to 65504 (v_cvt_pkrtz)."""
    e = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 7 * 2.0 ** -12, 2.0 ** -20 * 1.9, 70000.0, 0.0], dtype=torch.float32)
    h = ab._rtz16(e).double()
    assert h.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -10, 2.0 ** -20 * 1.875, 65504.0, 0.0]
