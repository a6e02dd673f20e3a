"""CPU: the MRRP WSL ResNet backbone's host side -- the registered builder, the module surface (key for key the plain ResNet's),
the refusals, the reference's own MRRP WSR YAML files, the exported `_ex` entries, and the torch restatement
tests/mrrp_resnet_util.py against the reference's own outputs (g22: tests/golden/make_golden_mrrp_resnet.py)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import mrrp_resnet_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G22 = np.load(os.path.join(ROOT, "tests", "golden", "g22_resnet_mrrp.npz"), allow_pickle=False)
REF_CONFIGS = "/root/reference/configs"


def _cfg(depth=18, **mrrp):
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(depth=depth, mrrp=True, device="cpu")
    for k, v in mrrp.items():
        setattr(cfg.MODEL.MRRP, k, v)
    return cfg


def _build(cfg):
    from wsovod_amd.config import BACKBONE_REGISTRY
    from wsovod_amd.structures import ShapeSpec

    return BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, ShapeSpec(channels=3))


def _plain(depth):
    from wsovod_amd.modeling.backbone import build_wsl_resnet_backbone
    from wsovod_amd.structures import ShapeSpec
    from wsovod_amd.testing import hot_path_cfg

    return build_wsl_resnet_backbone(hot_path_cfg(depth=depth, device="cpu"), ShapeSpec(channels=3))


@pytest.mark.parametrize("depth", [18, 50])
def test_builder_is_registered_and_the_surface_is_the_plain_models(depth):
    from wsovod_amd.modeling.backbone import BasicBlock, BottleneckBlock, ResNet
    from wsovod_amd.modeling.backbone_resnet_mrrp import MRRPBasicBlock, MRRPBottleneckBlock, MRRPResNet

    cfg = _cfg(depth)
    assert cfg.MODEL.BACKBONE.NAME == "build_mrrp_wsl_resnet_backbone"
    net, plain = _build(cfg), _plain(depth)
    assert isinstance(net, MRRPResNet) and isinstance(net, ResNet)
    mrrp_cls, plain_cls = (MRRPBasicBlock, BasicBlock) if depth == 18 else (MRRPBottleneckBlock, BottleneckBlock)
    assert all(isinstance(b, mrrp_cls) for b in net.res5) and len(net.res5) == len(plain.res5)
    for stage in (net.res2, net.res3, net.res4):
        assert all(type(b) is plain_cls for b in stage)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(v.shape)) for k, v in plain.state_dict().items()]
    spec = net.output_shape()["res5"]
    assert spec.stride == 8 and spec.channels == U.RES5_CHANNELS[depth] and list(net.output_shape()) == ["res5"]
    assert net.mrrp_stacked is True and net.mrrp_num_branch == 3
    assert [b.shared_input for b in net.res5] == [True] + [False] * (len(net.res5) - 1)
    assert [b.concat_output for b in net.res5] == [False] * (len(net.res5) - 1) + [True]
    for b in net.res5:
        assert b.dilations == (1, 2, 4) and not b.has_pool and b.stride == 1
        assert all(c.stride == 1 for c in b.convs()) and (b.shortcut is None) == (b is not net.res5[0])
    assert not any(p.requires_grad for p in net.parameters())


@pytest.mark.parametrize("depth", [18, 50])
def test_checkpoints_of_the_plain_and_the_mrrp_model_are_interchangeable(depth):
    sd = {k[len("backbone."):]: v for k, v in U.resnet_seeded_state(depth).items()}
    plain, mrrp = _plain(depth), _build(_cfg(depth))
    plain.load_state_dict(sd, strict=True)
    mrrp.load_state_dict(plain.state_dict(), strict=True)
    back = _plain(depth)
    back.load_state_dict(mrrp.state_dict(), strict=True)
    assert all(torch.equal(back.state_dict()[k], v) for k, v in sd.items())


@pytest.mark.parametrize("depth", [18, 50])
def test_surface_equals_g22(depth):
    net, tag = _build(_cfg(depth)), f"r{depth}_"
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in G22[tag + "keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(x) for x in G22[tag + "shapes"]]
    shape = net.output_shape()
    assert list(net._out_features) == [str(f) for f in G22[tag + "out_features"]] == ["res5"]
    assert [shape[f].stride for f in net._out_features] == G22[tag + "out_strides"].tolist() == [8]
    assert [shape[f].channels for f in net._out_features] == G22[tag + "out_channels"].tolist()


@pytest.mark.parametrize("change,key", [(dict(MRRP_STAGE="res4"), "MRRP_STAGE"), (dict(MRRP_STAGE="res2"), "MRRP_STAGE"),
                                        (dict(TEST_BRANCH_IDX=1), "TEST_BRANCH_IDX"), (dict(TEST_BRANCH_IDX=0), "TEST_BRANCH_IDX"),
                                        (dict(BRANCH_DILATIONS=[1, 2]), "BRANCH_DILATIONS"),
                                        (dict(NUM_BRANCH=5, BRANCH_DILATIONS=[1, 2, 3, 4, 5]), "NUM_BRANCH")])
def test_mrrp_refusals_name_their_key(change, key):
    with pytest.raises(NotImplementedError, match=key):
        _build(_cfg(**change))


@pytest.mark.parametrize("depth", [18, 50])
def test_other_refusals_name_their_key(depth):
    cfg = _cfg(depth)
    cfg.MODEL.BACKBONE.FREEZE_AT = 4
    with pytest.raises(NotImplementedError, match="FREEZE_AT"):
        _build(cfg)
    cfg = _cfg(depth)
    cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False, False, False, True]
    with pytest.raises(NotImplementedError, match="DEFORM_ON_PER_STAGE"):
        _build(cfg)
    cfg = _cfg(depth)
    cfg.MODEL.RESNETS.NUM_GROUPS = 2
    with pytest.raises(NotImplementedError, match="NUM_GROUPS"):
        _build(cfg)


def test_four_branches_are_built():
    net = _build(_cfg(NUM_BRANCH=4, BRANCH_DILATIONS=[1, 2, 3, 4]))
    assert net.mrrp_num_branch == 4 and net.res5[1].dilations == (1, 2, 3, 4)


@pytest.mark.skipif(not os.path.exists(REF_CONFIGS), reason="reference checkout absent")
def test_reference_mrrp_wsr_config_files_load():
    """Every WSOVOD_MRRP_WSR_* file merges; with precomputed proposals the PascalVOC 1x pair builds the whole model, unchanged
    otherwise (the MRRP RPN is another refusal; of the mixed-dataset files only the backbone is built here)."""
    from wsovod_amd.config import get_cfg
    from wsovod_amd.modeling import build_model

    files = sorted(glob.glob(os.path.join(REF_CONFIGS, "*", "WSOVOD_MRRP_WSR_*.yaml")))
    assert len(files) == 8
    for f in files:
        cfg = get_cfg()
        cfg.merge_from_file(f)
        assert cfg.MODEL.BACKBONE.NAME == "build_mrrp_wsl_resnet_backbone" and cfg.MODEL.MRRP.MRRP_ON
        assert cfg.MODEL.MRRP.MRRP_STAGE == "res5" and cfg.MODEL.MRRP.TEST_BRANCH_IDX == -1
        assert len(cfg.MODEL.MRRP.BRANCH_DILATIONS) == cfg.MODEL.MRRP.NUM_BRANCH <= 4
        net = _build(cfg)
        assert net.mrrp_num_branch == cfg.MODEL.MRRP.NUM_BRANCH and cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE == "ROILoopPool"
    for depth in (18, 50):
        cfg = get_cfg()
        cfg.merge_from_file(os.path.join(REF_CONFIGS, "PascalVOC-Detection", f"WSOVOD_MRRP_WSR_{depth}_DC5_1x.yaml"))
        hot = _cfg(depth)  # (the class embeddings' file of the test builder: the reference's path is not on this machine)
        # (BBOX_REFINE -- SAM in the training step -- is refused for every config, MRRP or not: off, as in the hot-path files)
        cfg.merge_from_list(["MODEL.PROPOSAL_GENERATOR.NAME", "PrecomputedProposals", "MODEL.DEVICE", "cpu", "WSOVOD.BBOX_REFINE.ENABLE", False,
                             "MODEL.ROI_BOX_HEAD.OPEN_VOCABULARY.WEIGHT_PATH_TRAIN", hot.MODEL.ROI_BOX_HEAD.OPEN_VOCABULARY.WEIGHT_PATH_TRAIN,
                             "MODEL.ROI_BOX_HEAD.OPEN_VOCABULARY.WEIGHT_PATH_TEST", hot.MODEL.ROI_BOX_HEAD.OPEN_VOCABULARY.WEIGHT_PATH_TEST])
        model = build_model(cfg)
        assert model.backbone.mrrp_num_branch == 3 and model.roi_heads.mrrp_on and model.proposal_generator is None


def test_new_entries_are_declared_bound_and_the_abi_version_stays():
    from wsovod_amd import _lib

    assert _lib.ABI_VERSION == 9
    header = open(os.path.join(ROOT, "include", "wsovod_hip.h")).read()
    for name in ("wsovod_gemm_conv_branches_ex", "wsovod_gemm_f16mx_conv_branches_ex"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header)
    assert len(_lib.SIGNATURES["wsovod_gemm_conv_branches_ex"]) == len(_lib.SIGNATURES["wsovod_gemm_conv_branches"]) + 1
    assert len(_lib.SIGNATURES["wsovod_gemm_f16mx_conv_branches_ex"]) == len(_lib.SIGNATURES["wsovod_gemm_f16mx_conv_branches"]) + 1


@pytest.mark.parametrize("depth", [18, 50])
def test_restatement_matches_the_references_outputs(depth):
    """res5_mrrp_ref / resnet_mrrp_ref (what the GPU tests compare with) against the reference's own MRRP ResNet on the seeded
    weights: 1e-5 of the largest value, the project's CPU bar."""
    sd = U.resnet_seeded_state(depth)
    want = torch.from_numpy(G22[f"r{depth}_res5"])
    n, h, w = U.RES4_MAP[depth]
    assert tuple(want.shape) == (3 * n, U.RES5_CHANNELS[depth], h, w)
    got = U.res5_mrrp_ref(sd, U.res4_map(depth), depth)
    err = float((got - want).abs().max())
    print(f"R{depth} res5: max |err| {err:.3e} (max |want| {float(want.abs().max()):.3f})")
    assert got.shape == want.shape and err <= 1e-5 * max(1.0, float(want.abs().max()))
    want = torch.from_numpy(G22[f"r{depth}_backbone"])
    assert tuple(want.shape) == (6, U.RES5_CHANNELS[depth] // U.KEEP_EVERY[depth], 12, 16)
    got = U.resnet_mrrp_ref(sd, U.image_batch(), depth)
    assert tuple(got.shape) == (6, U.RES5_CHANNELS[depth], 12, 16)
    got = got[:, ::U.KEEP_EVERY[depth]]
    err = float((got - want).abs().max())
    print(f"R{depth} backbone: max |err| {err:.3e} (max |want| {float(want.abs().max()):.3f})")
    assert err <= 1e-5 * max(1.0, float(want.abs().max()))
    # branch order: chunk b is the plain net with res5 dilation d_b (chunk 1 = the shipped RES5_DILATION 2 model)
    plain = U.R.backbone_forward(sd, U.image_batch(), depth=depth, res5_dilation=2)["res5"][:, ::U.KEEP_EVERY[depth]]
    assert torch.equal(got[2:4], plain)


@pytest.mark.parametrize("depth", [18, 50])
def test_hot_path_mrrp_model_builds_on_cpu(depth):
    from wsovod_amd.modeling import build_model
    from wsovod_amd.modeling.backbone_resnet_mrrp import MRRPResNet
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(depth=depth, mrrp=True, device="cpu")
    assert cfg.MODEL.MRRP.MRRP_ON and cfg.MODEL.MRRP.BRANCH_DILATIONS == [1, 2, 4] and cfg.MODEL.MRRP.TEST_BRANCH_IDX == -1
    assert cfg.MODEL.PROPOSAL_GENERATOR.NAME == "PrecomputedProposals" and cfg.MODEL.RESNETS.DEPTH == depth
    model = build_model(cfg)
    assert isinstance(model.backbone, MRRPResNet) and model.backbone.mrrp_num_branch == 3
    assert model.roi_heads.mrrp_on and model.roi_heads.mrrp_num_branch == 3 and model.proposal_generator is None
    assert model.data_aware_head is None or model.data_aware_head.mrrp_on
    assert not hot_path_cfg(depth=depth, device="cpu").MODEL.MRRP.MRRP_ON  # the option defaults to off


def test_mrrp_on_and_the_backbone_must_agree():
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(device="cpu")  # a plain ResNet under MRRP_ON
    cfg.MODEL.MRRP.MRRP_ON = True
    with pytest.raises(NotImplementedError, match="MRRP"):
        build_model(cfg)
    cfg = hot_path_cfg(mrrp=True, device="cpu")  # an MRRP backbone whose heads would read branch 0 only
    cfg.MODEL.MRRP.MRRP_ON = False
    with pytest.raises(NotImplementedError, match="MRRP_ON"):
        build_model(cfg)


def test_the_mrrp_rpn_keeps_raising_with_the_resnet_backbone():
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(rpn=True, device="cpu")
    cfg.merge_from_list(["MODEL.BACKBONE.NAME", "build_mrrp_wsl_resnet_backbone", "MODEL.MRRP.MRRP_ON", True, "MODEL.MRRP.MRRP_STAGE",
                         "res5", "MODEL.MRRP.TEST_BRANCH_IDX", -1, "MODEL.MRRP.BRANCH_DILATIONS", [1, 2, 4]])
    with pytest.raises(NotImplementedError, match="MRRP RPN"):
        build_model(cfg)


def test_the_one_launch_table_and_its_override(monkeypatch):
    from wsovod_amd.modeling import backbone_resnet_mrrp as M

    monkeypatch.delenv("WSOVOD_BRANCH_BATCHED", raising=False)
    assert M.MRRPBasicBlock.KIND == "basic" and M.MRRPBottleneckBlock.KIND == "bottleneck"
    for kind in ("basic", "bottleneck"):
        for fmt, mx in (("bf16x2", False), ("f16mx", True)):
            up_to = M.BATCHED_UP_TO[kind][fmt]
            assert M.branch_batched_default(kind, mx, up_to + 1) is False
            assert up_to == 0 or M.branch_batched_default(kind, mx, up_to) is True
    monkeypatch.setenv("WSOVOD_BRANCH_BATCHED", "1")
    assert M.branch_batched_default("basic", False, 10 ** 6) is True
    monkeypatch.setenv("WSOVOD_BRANCH_BATCHED", "0")
    assert M.branch_batched_default("bottleneck", True, 1) is False
