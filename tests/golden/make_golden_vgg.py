"""Generate tests/golden/g20_vgg16.npz by running the REFERENCE's own VGG16 (wsovod/modeling/backbone/vgg.py), loaded by path
over the stand-in modules of make_golden.py.

    python tests/golden/make_golden_vgg.py

Stored: the state-dict key names and shapes, `output_shape()` strides / channels and `_out_features` for CONV5_DILATION 2 and 1,
and the plain5 outputs of both models on the two seeded inputs of tests/vgg_util.py.  The 59 MB of weights are NOT stored:
every parameter (biases too) is filled from the per-tensor seed rule tests/vgg_util.py:vgg_seeded_state, which the tests
re-run."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import vgg_util  # noqa: E402
from tests.golden import make_golden as MG  # noqa: E402


class _FrozenBN(MG.FrozenBatchNorm2d):
    @classmethod
    def convert_frozen_batchnorm(cls, module):  # detectron2's walks the tree for BatchNorm layers: VGG16 has none
        assert not any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in module.modules())
        return module


def main():
    MG.install_shims()
    sys.modules["detectron2.layers"].FrozenBatchNorm2d = _FrozenBN
    ref = MG.load_ref("wsovod.modeling.backbone.vgg", "wsovod/modeling/backbone/vgg.py")
    torch.manual_seed(0)
    sd = vgg_util.vgg_seeded_state()
    xs = vgg_util.vgg_inputs()
    arrays = {}
    for d in (2, 1):
        net = ref.VGG16(d, 5).eval()
        ref_sd = net.state_dict()
        assert [(k, tuple(v.shape)) for k, v in ref_sd.items()] == vgg_util.vgg_keys_shapes()
        assert not any(p.requires_grad for p in net.parameters())
        net.load_state_dict(sd, strict=True)
        if d == 2:
            arrays["keys"] = np.array(list(ref_sd.keys()))
            arrays["shapes"] = np.array([str(tuple(v.shape)) for v in ref_sd.values()])
        shape = net.output_shape()
        arrays[f"d{d}_out_features"] = np.array(list(net._out_features))
        arrays[f"d{d}_out_strides"] = np.array([shape[f].stride for f in net._out_features])
        arrays[f"d{d}_out_channels"] = np.array([shape[f].channels for f in net._out_features])
        arrays[f"d{d}_all_strides"] = np.array([net._out_feature_strides[f"plain{i}"] for i in range(1, 6)])
        arrays[f"d{d}_all_channels"] = np.array([net._out_feature_channels[f"plain{i}"] for i in range(1, 6)])
        with torch.no_grad():
            for i, x in enumerate(xs):
                arrays[f"d{d}_plain5_{i}"] = net(x.clone())["plain5"]
    MG.save("g20_vgg16", **arrays)


if __name__ == "__main__":
    main()
