"""Shared by the MRRP VGG16 tests: a torch restatement of the reference's MRRP backbone (vgg_mrrp.py: plain1 - plain4 as the
plain VGG16, plain5 once per branch dilation with the same weights, `torch.cat` along N) on top of tests/vgg_util.py."""
import torch
import torch.nn.functional as F

from vgg_util import vgg16_ref


def vgg16_mrrp_ref(sd, x, dilations=(1, 2, 4), conv5_dilation=2, prefix=""):
    """-> (len(dilations) * N, 512, H, W), branch-major, in x's dtype."""
    x4 = vgg16_ref(sd, x, conv5_dilation=conv5_dilation, prefix=prefix, stages=("plain4",))["plain4"]
    outs = []
    for d in dilations:
        y = x4
        for j in range(3):
            k = f"{prefix}plain5.0.conv{j + 1}."
            y = F.relu(F.conv2d(y, sd[k + "weight"].to(y.dtype), sd[k + "bias"].to(y.dtype), 1, d, d))
        outs.append(y)
    return torch.cat(outs)
