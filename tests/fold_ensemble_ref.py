"""Host twin of ldiff_op_window_finish_ensemble (include/ldiff.h): the reference's fold ensemble in torch CPU ops of the accumulators' dtype, in the kernel's
order -- per fold `acc / cnt` (one correctly rounded division; no count plane: the inputs are logits), the inf look per fold, `s = l_0; s += l_k` in fold
order, `s /= K` when K > 1.  torch's CPU half `+=` and `/= K` are rn16 of the float32 operation, which is the correctly rounded result
(24 >= 2 * 11 + 2 bits), so they are a bit-exact oracle; tests/test_cpu_fold_ensemble.py pins the twin to the reference's own recorded ensemble
(tests/golden/reference_fold_ensemble.npz, scripts/gen_golden_fold_ensemble.py)."""
import torch

import window_twin


def stand_in_network(weight, slope):
    """The fixture's stand-in head of one fold: integer 1x1 weights plus a column ramp of the fold's slope, float32 out."""
    weight, slope = torch.as_tensor(weight, dtype=torch.float32), float(slope)

    def network(x):
        ramp = torch.arange(x.shape[-1], dtype=torch.float32, device=x.device) * slope
        return torch.einsum("oc,bchw->bohw", weight.to(x.device), x.float()) + ramp[None, None, None, :]
    return network


def ensemble(accs, cnt=None, box=None):
    """accs: host tensors [heads, Hp, Wp] of one dtype, cnt [Hp, Wp] or None, box = (y0, x0, h, w) or None (everything)
    -> (logits [heads, h, w], mask uint8 [h, w], inf flag)."""
    if box is not None:
        y0, x0, h, w = box
        accs = [a[:, y0:y0 + h, x0:x0 + w] for a in accs]
        cnt = None if cnt is None else cnt[y0:y0 + h, x0:x0 + w]
    logits = [a / cnt if cnt is not None else a.clone() for a in accs]
    flag = int(any(bool(torch.isinf(l).any()) for l in logits))
    s = logits[0].clone()
    for l in logits[1:]:
        s += l
    if len(logits) > 1:
        s /= len(logits)
    return s, window_twin.argmax_rule(s), flag
