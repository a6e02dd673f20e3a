"""CPU: the VGG16 DC5 backbone's host side -- config keys, the reference's own V_16 YAML files, the module surface against
the reference's (g20), the refusals, and the torch restatement tests/vgg_util.py:vgg16_ref against the reference's outputs."""
import os
import re

import numpy as np
import pytest
import torch

from tests import vgg_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G20 = np.load(os.path.join(ROOT, "tests", "golden", "g20_vgg16.npz"), allow_pickle=False)
REF_CONFIGS = "/root/reference/configs"
V16 = ("PascalVOC-Detection/WSOVOD_V_16_DC5_1x.yaml", "PascalVOC-Detection/WSOVOD_V_16_DC5_VOC12_1x.yaml",
       "COCO-Detection/WSOVOD_V_16_DC5_1x.yaml")


def test_config_defaults_are_the_references():
    from wsovod_amd.config import get_cfg

    cfg = get_cfg()
    assert cfg.MODEL.VGG.DEPTH == 16 and cfg.MODEL.VGG.CONV5_DILATION == 1


@pytest.mark.skipif(not os.path.exists(REF_CONFIGS), reason="reference checkout absent")
@pytest.mark.parametrize("rel", V16)
def test_reference_v16_config_files_load(rel):
    from wsovod_amd.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(REF_CONFIGS, rel))
    assert cfg.MODEL.BACKBONE.NAME == "build_vgg_backbone" and cfg.MODEL.BACKBONE.FREEZE_AT == 5
    assert cfg.MODEL.VGG.DEPTH == 16 and cfg.MODEL.VGG.CONV5_DILATION == 2
    assert cfg.MODEL.ROI_HEADS.IN_FEATURES == ["plain5"]
    assert cfg.MODEL.PIXEL_MEAN == [103.939, 116.779, 123.68]


def test_hot_path_vgg16_model_builds_on_cpu():
    from wsovod_amd.modeling import build_model
    from wsovod_amd.modeling.backbone_vgg import VGG16
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(backbone="vgg16", device="cpu")
    assert cfg.MODEL.VGG.CONV5_DILATION == 2 and cfg.SOLVER.BIAS_LR_FACTOR == 2.0 and cfg.SOLVER.WEIGHT_DECAY_BIAS == 0.0
    model = build_model(cfg)
    bb = model.backbone
    assert isinstance(bb, VGG16) and not bb.has_trainable_stage and bb.compute_dtype == torch.bfloat16
    assert not any(p.requires_grad for p in bb.parameters())
    assert bb.output_shape()["plain5"].stride == 8 and bb.output_shape()["plain5"].channels == 512
    assert tuple(model.roi_heads.box_head.fcs[0].weight.shape) == (4096, 25088)  # the neck's fc1, as for WSR_18
    # the default backbone of the helpers is unchanged
    assert hot_path_cfg(device="cpu").MODEL.BACKBONE.NAME == "build_wsl_resnet_backbone"


@pytest.mark.parametrize("dilation", [2, 1])
def test_surface_equals_the_references(dilation):
    from wsovod_amd.modeling.backbone_vgg import VGG16

    net = VGG16(dilation, 5)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in G20["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in G20["shapes"]]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == vgg_util.vgg_keys_shapes()
    assert list(net._out_features) == [str(f) for f in G20[f"d{dilation}_out_features"]] == ["plain5"]
    shape = net.output_shape()
    assert [shape[f].stride for f in net._out_features] == G20[f"d{dilation}_out_strides"].tolist()
    assert [shape[f].channels for f in net._out_features] == G20[f"d{dilation}_out_channels"].tolist()
    names = [f"plain{i}" for i in range(1, 6)]
    assert list(net.stage_names) == names
    assert [net._out_feature_strides[n] for n in names] == G20[f"d{dilation}_all_strides"].tolist()
    assert [net._out_feature_channels[n] for n in names] == G20[f"d{dilation}_all_channels"].tolist()
    for n in names:  # each stage an nn.Sequential of one block
        stage = getattr(net, n)
        assert isinstance(stage, torch.nn.Sequential) and len(stage) == 1
    assert not any(p.requires_grad for p in net.parameters())
    net.load_state_dict(vgg_util.vgg_seeded_state(), strict=True)


def test_refusals():
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(backbone="vgg16", device="cpu", freeze_at=4)
    with pytest.raises(NotImplementedError, match="FREEZE_AT"):
        build_model(cfg)
    cfg = hot_path_cfg(backbone="vgg16", device="cpu")
    cfg.MODEL.VGG.DEPTH = 19
    with pytest.raises(NotImplementedError, match="DEPTH"):
        build_model(cfg)


def test_rpn_in_features_of_the_reference_yaml_is_named_in_the_error():
    """The reference's V_16 YAML keeps RPN.IN_FEATURES = ["res5"] from its base: no VGG map has that name."""
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(backbone="vgg16", device="cpu", rpn=True)
    cfg.MODEL.RPN.IN_FEATURES = ["res5"]
    with pytest.raises(KeyError, match=r"MODEL\.RPN\.IN_FEATURES.*plain5"):
        build_model(cfg)
    cfg.MODEL.RPN.IN_FEATURES = ["plain5"]
    model = build_model(cfg)
    assert model.proposal_generator is not None and model.proposal_generator.in_features == ["plain5"]


@pytest.mark.parametrize("dilation", [2, 1])
def test_restatement_matches_the_references_outputs(dilation):
    """vgg16_ref (what the GPU tests compare with) against the reference's own VGG16 on the seeded weights: 1e-5."""
    sd = vgg_util.vgg_seeded_state()
    for i, x in enumerate(vgg_util.vgg_inputs()):
        want = torch.from_numpy(G20[f"d{dilation}_plain5_{i}"])
        for dt in (torch.float32, torch.float64):
            got = vgg_util.vgg16_ref(sd, x.to(dt), dilation)
            assert got.shape == want.shape
            err = float((got.double() - want.double()).abs().max())
            print(f"dilation {dilation} input {i} {dt}: max |err| {err:.3e} (max |want| {float(want.abs().max()):.3f})")
            assert err <= 1e-5 * max(1.0, float(want.abs().max()))
    h, w = vgg_util.vgg_inputs()[1].shape[-2:]
    if dilation == 2:  # 41 x 55: floors 20x27 -> 10x13 -> 5x6, then the stride-1 pool's -1
        assert tuple(G20["d2_plain5_1"].shape[-2:]) == (h // 8 - 1, w // 8 - 1) == (4, 5)


def test_abi_and_new_symbols():
    from wsovod_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "wsovod_hip.h")).read()
    declared = set(re.findall(r"\b(wsovod_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    assert _lib.ABI_VERSION == 9 and L.wsovod_abi_version() == 9
    for name in ("wsovod_stem_conv1_s1", "wsovod_stem_conv1_s1_x2", "wsovod_stem_im2col_ex"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    # argument validation before any launch: the f16mx pool takes whole 32-value groups, the im2col strides 1 and 2
    assert L.wsovod_maxpool2x2_nhwc(None, _lib.F16MX, 1, 4, 4, 48, 2, 0, None, None) == 1
    assert b"multiple of 32" in L.wsovod_last_error()
    assert L.wsovod_stem_im2col_ex(None, None, None, None, 1, 8, 8, 3, None, _lib.F32, None) == 1
    assert b"stride" in L.wsovod_last_error()
