"""Pins the nnU-Net tissue head's key layout and one forward pass against the package that owns them.

Needs `dynamic_network_architectures` (and torch); the test-suite's machines have neither it nor a network, so this script is run by a maintainer
where the package is installed.  It builds PlainConvUNet exactly as nnU-Net's get_network_from_plans does for the fixture plans
(tests/golden/nnunet_plans_2d.json, configuration 2d_reduced), and
  1. compares its state-dict keys, after ldiffusion_amd.nnunet.clean_state_dict, with ldiffusion_amd.nnunet.param_shapes (names and shapes);
  2. runs one seeded float64 forward and compares it with tests/nnunet_ref.forward on the same weights;
  3. writes tests/golden/nnunet_pinned.npz (the seeded input, the logits, the sorted key list) for a test to consume.
usage: python scripts/gen_golden_nnunet.py
"""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from dynamic_network_architectures.architectures.unet import PlainConvUNet   # the import this script exists for
    import nnunet_ref
    from ldiffusion_amd import nnunet
    golden = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(golden, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(golden, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    n = spec["n_stages"]
    net = PlainConvUNet(input_channels=spec["in_channels"], n_stages=n, features_per_stage=spec["features"], conv_op=nn.Conv2d, kernel_sizes=[[3, 3]] * n,
                        strides=[[s, s] for s in spec["strides"]], n_conv_per_stage=spec["n_conv_encoder"], num_classes=spec["n_heads"],
                        n_conv_per_stage_decoder=spec["n_conv_decoder"], conv_bias=True, norm_op=nn.InstanceNorm2d, norm_op_kwargs={"eps": 1e-5, "affine": True},
                        dropout_op=None, dropout_op_kwargs=None, nonlin=nn.LeakyReLU, nonlin_kwargs={"inplace": True}, deep_supervision=False).double().eval()
    torch.manual_seed(0)
    for p in net.parameters():
        p.data.normal_(0.0, 0.1)
    sd = nnunet.clean_state_dict(net.state_dict(), spec)
    want = nnunet.param_shapes(spec)
    assert set(sd) == set(want), (sorted(set(sd) - set(want))[:5], sorted(set(want) - set(sd))[:5])
    assert all(tuple(sd[k].shape) == tuple(want[k]) for k in want)
    x = torch.randn((1, spec["in_channels"], 64, 64), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with torch.no_grad():
        y = net(x)
    ref = nnunet_ref.forward(sd, spec, x, torch.float64)
    err = (y - ref).abs().max().item() / ref.abs().max().item()
    print(f"keys: {len(sd)} canonical of {len(net.state_dict())}; forward: max |package - restatement| = {err:.2e} of max |logit|")
    assert err <= 1e-12
    np.savez_compressed(os.path.join(golden, "nnunet_pinned.npz"), x=x.numpy(), logits=y.numpy(), keys=np.array(sorted(net.state_dict())))


if __name__ == "__main__":
    main()
