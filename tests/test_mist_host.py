"""MIST pseudo-GT mining (WSOVOD.INSTANCE_REFINEMENT.REFINE_MIST), the parts that need no GPU: the torch restatement the
kernels are compared with reproduces the reference's own outputs (tests/golden/g24_mist.npz, direct calls of get_pgt_mist
and label_and_sample_proposals_wsl) exactly; the host side of the feature (config, constructor, refusals, bindings)."""
import pytest
import torch

from tests import mist_util as U
from tests.helpers import load_golden

K, THR = 20, 0.5


@pytest.fixture(scope="module")
def g24():
    return load_golden("g24_mist")


def direct_names(g):
    return [str(n) for n in g["direct/names"]]


def test_golden_holds_the_issues_images(g24):
    names = direct_names(g24)
    assert names == ["r120_c1", "r120_c2", "r120_c3", "r97", "half_small", "all_small", "one_valid", "all_below_floor",
                     "grid2000_c3"]
    assert g24["direct/grid2000_c3/t_classes"].numel() > 128           # more targets than the top-1 kernel's LDS holds
    assert g24["direct/all_small/t_boxes"].tolist() == [[-10000.0, -10000.0, 10000.0, 10000.0]]
    assert g24["direct/all_below_floor/t_classes"].numel() == 3        # rank 0 of each class only
    for n in names:                                                    # the weight is the candidate's own score
        assert torch.equal(g24[f"direct/{n}/t_weights"], g24[f"direct/{n}/t_scores"]), n


def test_restatement_reproduces_the_reference_exactly(g24):
    for n in direct_names(g24):
        p = f"direct/{n}/"
        boxes, scores, classes = g24[p + "boxes"], g24[p + "scores"], g24[p + "classes"]
        t = U.mine(boxes, scores, classes)
        assert torch.equal(t["gt_classes"], g24[p + "t_classes"]), n   # classes, order and count
        assert torch.equal(t["gt_boxes"], g24[p + "t_boxes"]), n       # copies: bit for bit
        assert torch.equal(t["gt_scores"], g24[p + "t_scores"]), n
        assert torch.equal(t["gt_weights"], g24[p + "t_weights"]), n
        if n != "all_small":
            assert torch.equal(boxes[t["index"]], t["gt_boxes"]) and torch.equal(scores[t["index"], t["gt_classes"]], t["gt_scores"])
        lab = U.label(boxes, t, K, THR)
        assert torch.equal(lab["gt_classes"], g24[p + "l_classes"]), n
        assert torch.equal(lab["gt_boxes"], g24[p + "l_boxes"]), n
        assert torch.equal(lab["gt_scores"], g24[p + "l_scores"]), n
        assert torch.equal(lab["gt_weights"], g24[p + "l_weights"]), n


def test_candidate_count_helper_equals_pythons():
    from wsovod_amd.layers import hip_ops as H

    for n in range(0, 14001):
        assert H.mist_k(n) == max(int(n * 0.15), 1) == U.mist_k(n), n
    assert H.mist_k(120) == 18 and H.mist_k(5024) == 753 and H.mist_k(13659) == 2048 and H.mist_k(13660) == 2049


def test_the_mist_yaml_builds_plain_and_mixed_heads():
    from wsovod_amd.testing import build_hot_path_model, build_mixed_model

    cfg, model = build_hot_path_model(mist=True, device="cpu", precision="fp32")
    assert cfg.WSOVOD.INSTANCE_REFINEMENT.REFINE_MIST is True and model.roi_heads.refine_mist is True
    cfg, model = build_mixed_model(mist=True, device="cpu", precision="fp32")
    assert type(model.roi_heads).__name__ == "WSOVODMixedDatasetsROIHeads" and model.roi_heads.refine_mist is True
    _, model = build_hot_path_model(device="cpu", precision="fp32")
    assert model.roi_heads.refine_mist is False


def test_sam_and_train_on_pred_boxes_still_raise():
    from wsovod_amd.modeling import build_model
    from wsovod_amd.modeling.roi_heads import WSOVODROIHeads
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(mist=True, device="cpu")
    cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES = True
    with pytest.raises(NotImplementedError, match="TRAIN_ON_PRED_BOXES"):
        build_model(cfg)
    cfg = hot_path_cfg(mist=True, device="cpu")
    cfg.WSOVOD.BBOX_REFINE.ENABLE = True
    with pytest.raises(NotImplementedError, match="SAM"):
        build_model(cfg)
    with pytest.raises(NotImplementedError, match="SAM"):  # the constructor's own refusal, past from_config's
        WSOVODROIHeads.__init__(WSOVODROIHeads.__new__(WSOVODROIHeads), box_in_features=["res5"], box_pooler=None,
                                box_head=None, object_miner=None, sam=object(), num_classes=K, batch_size_per_image=512,
                                positive_fraction=0.25, proposal_matcher=None, pixel_mean=[0.0], pixel_std=[1.0])


def test_capacity_refusals_name_their_numbers():
    from wsovod_amd.layers import hip_ops as H

    z = torch.zeros(1)
    with pytest.raises(RuntimeError, match=r"22 image-level classes x 753 candidates per class = 16566.*10176"):
        H.mist_mine_and_label(z, z, z, z, z, 80, 0.5, max_rows=5024, max_classes=22)  # (above the issue's 16384)
    with pytest.raises(RuntimeError, match=r"14 image-level classes x 753 candidates per class = 10542.*10176"):
        H.mist_mine_and_label(z, z, z, z, z, 80, 0.5, max_rows=5024, max_classes=14)  # (above what the NMS scan really holds)
    assert H.NMS_SEGMENT_MAX == 159 * 64  # 2 chunks x 64 rows x W 8-byte words <= 159 KiB of LDS (csrc/proposals.hip)
    with pytest.raises(RuntimeError, match=r"k_cap = 2049.*13660.*2048 pairs"):
        H.mist_mine_and_label(z, z, z, z, z, 80, 0.5, max_rows=13660, max_classes=1)


def test_new_entries_are_declared_and_bound_and_the_abi_version_stays():
    import os
    import re

    from wsovod_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wsovod_hip.h")).read()
    for name, nargs in (("wsovod_mist_select", 16), ("wsovod_mist_merge", 19), ("wsovod_mist_label", 27)):
        assert len(_lib.SIGNATURES[name]) == nargs, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl is not None and decl.group(1).count(",") + 1 == nargs, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.ABI_VERSION == 9 == _lib.lib().wsovod_abi_version()


def test_pseudo_targets_cut_rows_by_the_results_own_starts():
    """MIST's target rows are capacity-padded: PseudoTargets takes the starts from the result, not from the class offsets."""
    from wsovod_amd.modeling.roi_heads import PseudoTargets

    boxes = torch.arange(40, dtype=torch.float32).view(10, 4)
    o = dict(pgt_boxes=boxes, pgt_classes=torch.arange(10), pgt_scores=torch.arange(10.0), pgt_weights=torch.arange(10.0),
             pgt_count=torch.tensor([3, 1], dtype=torch.int32), pgt_start=torch.tensor([0, 6], dtype=torch.int32))
    t = PseudoTargets(o, torch.tensor([0, 2, 3], dtype=torch.int32), [(8, 8), (8, 8)])
    assert t.packed[1] is o["pgt_start"] and len(t) == 2
    assert t[0].gt_classes.tolist() == [0, 1, 2] and t[1].gt_classes.tolist() == [6]
    assert torch.equal(t[1].gt_boxes.tensor, boxes[6:7])
    del o["pgt_start"]  # top-1 mining: one row per class slot, the class offsets are the starts
    t = PseudoTargets(o, torch.tensor([0, 2, 3], dtype=torch.int32), [(8, 8), (8, 8)])
    assert t.packed[1].tolist() == [0, 2] and t[1].gt_classes.tolist() == [2]
