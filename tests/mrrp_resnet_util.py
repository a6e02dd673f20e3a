"""Shared by the MRRP ResNet tests: a plain fp32 torch restatement of the reference's MRRP WSL ResNet (resnet_wsl_mrrp.py:
stem and res2 - res4 as the plain net; every block of res5 once per branch dilation with the same weights, block 0 of every
branch reading the same res4 map; `torch.cat` along N) on top of the oracle's blocks, and the seeded weights and inputs of
tests/golden/g22_resnet_mrrp.npz (regenerated here, not stored)."""
import torch

from oracle import wsovod_ref as R
from tests.golden import gen

DILATIONS = (1, 2, 4)
RES4_CHANNELS = {18: 256, 50: 1024}
RES5_CHANNELS = {18: 512, 50: 2048}
RES4_MAP = {18: (1, 4, 5), 50: (1, 3, 4)}   # (N, H, W) of the seeded res4 maps of g22
KEEP_EVERY = {18: 16, 50: 64}               # g22 keeps every n-th channel of the whole-backbone outputs (file size)


def resnet_seeded_state(depth, seed=2200):
    """{"backbone.<key>": tensor} for the plain WSL ResNet's keys (= the MRRP one's), seeded as tests/golden/gen.py does."""
    from wsovod_amd.modeling.backbone import build_wsl_resnet_backbone
    from wsovod_amd.structures import ShapeSpec
    from wsovod_amd.testing import hot_path_cfg

    net = build_wsl_resnet_backbone(hot_path_cfg(depth=depth, device="cpu"), ShapeSpec(channels=3))
    return gen.seeded_state({"backbone." + k: tuple(v.shape) for k, v in net.state_dict().items()}, seed + depth)


def res4_map(depth):
    n, h, w = RES4_MAP[depth]
    return torch.relu(torch.randn((n, RES4_CHANNELS[depth], h, w), generator=torch.Generator().manual_seed(2300 + depth)))


def image_batch():
    """The normalised 2 x 3 x 96 x 128 float batch of the whole-backbone outputs."""
    return torch.randn((2, 3, 96, 128), generator=torch.Generator().manual_seed(2400))


def res5_mrrp_ref(sd, x4, depth, dilations=DILATIONS, prefix="backbone."):
    """res5 of the MRRP net on the res4 map x4 (N, C4, H, W) -> (len(dilations) * N, C5, H, W), branch-major."""
    block = R.basic_block if depth in (18, 34) else R.bottleneck_block
    outs = []
    for d in dilations:
        y = x4
        for b in range(R._BLOCKS[depth][3]):
            y = block(y, sd, f"{prefix}res5.{b}.", d, False, 1)
        outs.append(y)
    return torch.cat(outs)


def resnet_mrrp_ref(sd, x, depth, dilations=DILATIONS, prefix="backbone."):
    """The whole MRRP backbone on normalised float images x (N, 3, H, W) -> (len(dilations) * N, C5, H / 8, W / 8)."""
    x4 = R.backbone_forward(sd, x, depth=depth, res5_dilation=2, prefix=prefix)["res4"]
    return res5_mrrp_ref(sd, x4, depth, dilations, prefix)
