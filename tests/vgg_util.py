"""Shared by the VGG16 tests and tests/golden/make_golden_vgg.py: the seeded weight rule (VGG16's 59 MB of weights are
regenerated, not stored) and a small torch restatement of the backbone that tests/test_vgg_host.py pins to the reference's own
outputs (g20) and the GPU tests lean on."""
import math

import torch
import torch.nn.functional as F

# (stage, convs, in, out): wsovod/modeling/backbone/vgg.py:145-205
PLAN = (("plain1", 2, 3, 64), ("plain2", 2, 64, 128), ("plain3", 3, 128, 256), ("plain4", 3, 256, 512), ("plain5", 3, 512, 512))
SEED_BASE = 2000


def vgg_keys_shapes(prefix=""):
    """State-dict keys and shapes in module order: plain{i}.0.conv{j}.{weight,bias}."""
    out = []
    for name, n, cin, cout in PLAN:
        for j in range(n):
            out.append((f"{prefix}{name}.0.conv{j + 1}.weight", (cout, cin if j == 0 else cout, 3, 3)))
            out.append((f"{prefix}{name}.0.conv{j + 1}.bias", (cout,)))
    return out


def vgg_seeded_state(prefix="", dtype=torch.float32):
    """THE rule: the i-th tensor of vgg_keys_shapes() is drawn from torch.Generator().manual_seed(SEED_BASE + i) as fp32
    standard normals times sqrt(2 / fan_in) (weights, fan_in = 9 Cin: ReLU-preserving scale) or times 0.1 (biases, so that
    a bias is never a no-op)."""
    sd = {}
    for i, (k, shape) in enumerate(vgg_keys_shapes(prefix)):
        g = torch.Generator().manual_seed(SEED_BASE + i)
        t = torch.randn(shape, generator=g, dtype=torch.float32)
        sd[k] = (t * (math.sqrt(2.0 / (9 * shape[1])) if len(shape) == 4 else 0.1)).to(dtype)
    return sd


def vgg_inputs():
    """The fixture's two normalised float inputs: 3x48x64 (every pool even) and 3x41x55 (every pool floors; plain4's
    stride-1 pool takes its row and column off an odd map)."""
    return [torch.randn((1, 3, h, w), generator=torch.Generator().manual_seed(3000 + i)) * 2.0
            for i, (h, w) in enumerate(((48, 64), (41, 55)))]


def vgg16_ref(sd, x, conv5_dilation=2, prefix="", stages=None):
    """vgg.py:103-121,215-222 in torch ops, in x's dtype (fp32 / fp64): -> plain5 (or {stage: map} for `stages`)."""
    out = {}
    for name, n, _, _ in PLAN:
        d = conv5_dilation if name == "plain5" else 1
        for j in range(n):
            k = f"{prefix}{name}.0.conv{j + 1}."
            x = F.relu(F.conv2d(x, sd[k + "weight"].to(x.dtype), sd[k + "bias"].to(x.dtype), 1, d, d))
        if name != "plain5":
            x = F.max_pool2d(x, 2, 1 if (name == "plain4" and conv5_dilation == 2) else 2, 0)
        out[name] = x
    return out["plain5"] if stages is None else {s: out[s] for s in stages}
