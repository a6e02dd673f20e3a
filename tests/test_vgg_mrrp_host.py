"""CPU: the MRRP VGG16 backbone's host side -- the registered builder, the module surface (key for key the plain VGG16's), the
refusals, the reference's own MRRP V_16 YAML files, the exported entries, and the torch restatement tests/mrrp_util.py."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import mrrp_util, vgg_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G21 = np.load(os.path.join(ROOT, "tests", "golden", "g21_vgg16_mrrp.npz"), allow_pickle=False)
REF_CONFIGS = "/root/reference/configs"


def _cfg(**mrrp):
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(backbone="vgg16", device="cpu")
    cfg.MODEL.BACKBONE.NAME = "build_mrrp_vgg_backbone"
    cfg.MODEL.MRRP.MRRP_STAGE = "plain5"
    cfg.MODEL.MRRP.BRANCH_DILATIONS = [1, 2, 4]
    cfg.MODEL.MRRP.TEST_BRANCH_IDX = -1
    for k, v in mrrp.items():
        setattr(cfg.MODEL.MRRP, k, v)
    return cfg


def _build(cfg):
    from wsovod_amd.config import BACKBONE_REGISTRY
    from wsovod_amd.structures import ShapeSpec

    return BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, ShapeSpec(channels=3))


def test_builder_is_registered_and_the_surface_is_the_plain_models():
    from wsovod_amd.modeling.backbone_vgg import PlainBlock, VGG16
    from wsovod_amd.modeling.backbone_vgg_mrrp import MRRPPlainBlock, MRRPVGG16

    net = _build(_cfg())
    assert isinstance(net, MRRPVGG16) and isinstance(net, VGG16) and isinstance(net.plain5[0], MRRPPlainBlock)
    assert all(isinstance(getattr(net, f"plain{i}")[0], PlainBlock) for i in range(1, 5))
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == vgg_util.vgg_keys_shapes()
    spec = net.output_shape()["plain5"]
    assert spec.stride == 8 and spec.channels == 512 and list(net.output_shape()) == ["plain5"]
    assert net.plain5[0].dilations == (1, 2, 4) and net.mrrp_num_branch == 3 and not net.plain5[0].has_pool
    assert not any(p.requires_grad for p in net.parameters())
    # the reference's `name in self.mrrp_stage` test: another stage name leaves the plain block
    plain = _build(_cfg(MRRP_STAGE="res4"))
    assert isinstance(plain.plain5[0], PlainBlock) and plain.mrrp_num_branch == 1


def test_checkpoints_of_the_plain_and_the_mrrp_model_are_interchangeable():
    from wsovod_amd.modeling.backbone_vgg import VGG16

    sd = vgg_util.vgg_seeded_state()
    plain, mrrp = VGG16(2, 5), _build(_cfg())
    plain.load_state_dict(sd, strict=True)
    mrrp.load_state_dict(plain.state_dict(), strict=True)
    back = VGG16(2, 5)
    back.load_state_dict(mrrp.state_dict(), strict=True)
    assert all(torch.equal(back.state_dict()[k], v) for k, v in sd.items())


@pytest.mark.parametrize("change,key", [(dict(TEST_BRANCH_IDX=1), "TEST_BRANCH_IDX"), (dict(TEST_BRANCH_IDX=0), "TEST_BRANCH_IDX"),
                                        (dict(BRANCH_DILATIONS=[1, 2]), "BRANCH_DILATIONS"),
                                        (dict(NUM_BRANCH=5, BRANCH_DILATIONS=[1, 2, 3, 4, 5]), "NUM_BRANCH")])
def test_refusals_name_their_key(change, key):
    with pytest.raises(NotImplementedError, match=key):
        _build(_cfg(**change))


def test_a_trainable_stage_is_refused_as_for_the_plain_vgg():
    cfg = _cfg()
    cfg.MODEL.BACKBONE.FREEZE_AT = 4
    with pytest.raises(NotImplementedError, match="FREEZE_AT"):
        _build(cfg)


@pytest.mark.skipif(not os.path.exists(REF_CONFIGS), reason="reference checkout absent")
def test_reference_mrrp_v16_config_files_load():
    from wsovod_amd.config import get_cfg

    files = sorted(glob.glob(os.path.join(REF_CONFIGS, "*", "WSOVOD_MRRP_V_16_*.yaml")))
    assert len(files) >= 3
    for f in files[:3]:
        cfg = get_cfg()
        cfg.merge_from_file(f)
        assert cfg.MODEL.BACKBONE.NAME == "build_mrrp_vgg_backbone" and cfg.MODEL.MRRP.MRRP_ON
        assert "plain5" in cfg.MODEL.MRRP.MRRP_STAGE and cfg.MODEL.MRRP.TEST_BRANCH_IDX == -1
        assert len(cfg.MODEL.MRRP.BRANCH_DILATIONS) == cfg.MODEL.MRRP.NUM_BRANCH <= 4
        net = _build(cfg)
        assert net.mrrp_num_branch == cfg.MODEL.MRRP.NUM_BRANCH


def test_new_entries_are_declared_bound_and_the_abi_version_stays():
    from wsovod_amd import _lib

    assert _lib.ABI_VERSION == 9
    header = open(os.path.join(ROOT, "include", "wsovod_hip.h")).read()
    for name in ("wsovod_gemm_conv_branches", "wsovod_gemm_f16mx_conv_branches"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header)
    assert [n for n, _ in _lib.ConvBranches._fields_] == ["n_branch", "dil", "pad", "shared_input"]
    m = re.search(r"typedef struct \{\s*int n_branch;\s*int dil\[4\], pad\[4\];\s*int shared_input;\s*\} wsovod_conv_branches;", header)
    assert m, "wsovod_conv_branches layout"


@pytest.mark.parametrize("dils", [(1, 2, 4), (1, 2, 3)])
def test_restatement_matches_the_references_outputs(dils):
    """vgg16_mrrp_ref (what the GPU tests compare with) against the reference's own MRRP VGG16 on the seeded weights: 1e-5 of
    the largest value, the bar tests/test_vgg_host.py sets for g20."""
    sd = vgg_util.vgg_seeded_state()
    tag = "".join(str(d) for d in dils)
    for i, x in enumerate(vgg_util.vgg_inputs()):
        want = torch.from_numpy(G21[f"d{tag}_plain5_{i}"])
        assert tuple(want.shape) == (3, 512) + ((5, 7), (4, 5))[i]
        for dt in (torch.float32, torch.float64):
            got = mrrp_util.vgg16_mrrp_ref(sd, x.to(dt), dilations=dils)
            assert got.shape == want.shape
            err = float((got.double() - want.double()).abs().max())
            print(f"dilations {dils} input {i} {dt}: max |err| {err:.3e} (max |want| {float(want.abs().max()):.3f})")
            assert err <= 1e-5 * max(1.0, float(want.abs().max()))


def test_surface_equals_g21():
    net = _build(_cfg())
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in G21["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(x) for x in G21["shapes"]]
    shape = net.output_shape()
    assert list(net._out_features) == [str(f) for f in G21["out_features"]] == ["plain5"]
    assert [shape[f].stride for f in net._out_features] == G21["out_strides"].tolist() == [8]
    assert [shape[f].channels for f in net._out_features] == G21["out_channels"].tolist() == [512]


def test_rewritten_batch_indices_reproduce_the_reference_poolers_routing():
    """The reference pooled box r from chunk level_ids[r] // 1000 of the map (three same-scale levels, `index_put_`); the
    index rewrite pools it from image branch * N + n of the concatenated map in ONE single-level call: same values."""
    from oracle import wsovod_ref as R
    from oracle import roi_ops
    from wsovod_amd.modeling.roi_heads import mrrp_route_rois

    fmap = torch.from_numpy(G21["route_map"])
    boxes, ids = torch.from_numpy(G21["route_boxes"]), torch.from_numpy(G21["route_level_ids"])
    assert set(ids.flatten().tolist()) <= {0, 3, 1000, 1002, 2001} and len(set((ids // 1000).flatten().tolist())) == 3
    rois = mrrp_route_rois(R.pooler_format(list(boxes)), ids.flatten(), boxes.shape[0], 3)
    assert rois[:, 0].tolist() == [float(int(l) // 1000 * 2 + n) for n in range(2) for l in ids[n]]
    got = roi_ops.roi_pool_forward(fmap, rois, 0.125, (7, 7))[0]
    assert torch.equal(got, torch.from_numpy(G21["routed_pool"]))
    with pytest.raises(ValueError, match="level_ids"):
        mrrp_route_rois(rois, torch.full((24,), 3000), 2, 3)


def test_hot_path_vgg16_mrrp_model_builds_on_cpu():
    from wsovod_amd.modeling import build_model
    from wsovod_amd.modeling.backbone_vgg_mrrp import MRRPVGG16
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(backbone="vgg16", mrrp=True, device="cpu")
    assert cfg.MODEL.MRRP.MRRP_ON and cfg.MODEL.MRRP.BRANCH_DILATIONS == [1, 2, 4] and cfg.MODEL.MRRP.TEST_BRANCH_IDX == -1
    assert cfg.MODEL.PROPOSAL_GENERATOR.NAME == "PrecomputedProposals"
    model = build_model(cfg)
    assert isinstance(model.backbone, MRRPVGG16) and model.backbone.mrrp_num_branch == 3
    assert model.roi_heads.mrrp_on and model.roi_heads.mrrp_num_branch == 3 and model.proposal_generator is None
    assert model.data_aware_head is None or model.data_aware_head.mrrp_on
    assert not hot_path_cfg(backbone="vgg16", device="cpu").MODEL.MRRP.MRRP_ON  # the option defaults to off


def test_mrrp_on_and_the_backbone_must_agree():
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(backbone="vgg16", device="cpu")  # a plain backbone under MRRP_ON
    cfg.MODEL.MRRP.MRRP_ON = True
    with pytest.raises(NotImplementedError, match="MRRP"):
        build_model(cfg)
    cfg = hot_path_cfg(backbone="vgg16", mrrp=True, device="cpu")  # an MRRP backbone whose heads would read branch 0 only
    cfg.MODEL.MRRP.MRRP_ON = False
    with pytest.raises(NotImplementedError, match="MRRP_ON"):
        build_model(cfg)


def test_the_mrrp_rpn_keeps_raising():
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(backbone="vgg16", rpn=True, device="cpu")
    cfg.merge_from_list(["MODEL.BACKBONE.NAME", "build_mrrp_vgg_backbone", "MODEL.MRRP.MRRP_ON", True, "MODEL.MRRP.MRRP_STAGE",
                         "plain5", "MODEL.MRRP.TEST_BRANCH_IDX", -1])
    with pytest.raises(NotImplementedError, match="MRRP RPN"):
        build_model(cfg)
