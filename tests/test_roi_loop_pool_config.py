"""POOLER_TYPE ROILoopPool under the "parity" family on the host: which carrier the ROI heads ask the pooler for, that the
hot-path config builds, and that the fused entry is declared and registered (no GPU)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("precision", ["parity", "parity_mx", "parity_mx_train"])
def test_hot_path_config_with_the_loop_pool_builds(precision):
    from wsovod_amd.modeling.poolers import ROILoopPool
    from wsovod_amd.testing import build_hot_path_model

    cfg, model = build_hot_path_model(seed=0, precision=precision, pooler="ROILoopPool", device="cpu")
    assert cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE == "ROILoopPool" and model.roi_heads.pooler_type == "ROILoopPool"
    assert isinstance(model.roi_heads.box_pooler.level_poolers[0], ROILoopPool)
    assert model.roi_heads.precision == "parity" and model.mx == (precision != "parity")


def test_pool_dtype_follows_the_rows_fc1_sees(monkeypatch):
    """`_pool_dtype_for` takes the row count of the pooled matrix: 3R for ROILoopPool.  Under "parity_mx" the f16mx carrier
    starts at MX_MIN_ROWS of THOSE rows -- 1366 boxes (4098 rows) take it, 1365 (4095 rows) keep bf16x2, as 4095 rows of the
    one-output pool do; without the f16mx mode it is bf16x2 at any count; outside the "parity" family the compute dtype."""
    import torch

    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.modeling.roi_heads import WSOVODROIHeads
    from wsovod_amd.testing import build_hot_path_model

    monkeypatch.setattr(WSOVODROIHeads, "MX_MIN_ROWS", 4096)
    loop = build_hot_path_model(seed=0, precision="parity_mx", pooler="ROILoopPool", device="cpu")[1].roi_heads
    plain = build_hot_path_model(seed=0, precision="parity_mx", pooler="ROIPool", device="cpu")[1].roi_heads
    with H.x3_mode("x2"), H.mx_mode(True):
        assert loop._pool_dtype_for(3 * 1366) == H.MX and loop._pool_dtype_for(3 * 1365) == H.X2
        assert plain._pool_dtype_for(4096) == H.MX and plain._pool_dtype_for(4095) == H.X2
    with H.x3_mode("x2"), H.mx_mode(False):
        assert loop._pool_dtype_for(3 * 5000) == H.X2
    bf = build_hot_path_model(seed=0, precision="bf16", pooler="ROILoopPool", device="cpu")[1].roi_heads
    f3 = build_hot_path_model(seed=0, precision="bf16x3f", pooler="ROILoopPool", device="cpu")[1].roi_heads
    assert bf._pool_dtype_for(3 * 5000) == torch.bfloat16 and f3._pool_dtype_for(3 * 5000) == torch.float32


def test_pool_features_counts_three_rows_per_box(monkeypatch):
    """The ROI heads hand `_pool_dtype_for` 3R for ROILoopPool and R otherwise, and pass the scale to the pooler: no
    NotImplementedError, no torch multiply (the pooler and the rois kernel are stubbed: host only)."""
    import torch

    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.structures import Boxes, Instances
    from wsovod_amd.testing import build_hot_path_model

    seen = {}
    rois = torch.zeros(10, 5)
    scale = torch.ones(10)
    monkeypatch.setattr(H, "format_rois", lambda boxes, seg, obj=None: (rois, scale))
    for pooler, rows in (("ROILoopPool", 30), ("ROIPool", 10)):
        rh = build_hot_path_model(seed=0, precision="parity", pooler=pooler, device="cpu")[1].roi_heads

        def pool_dtype(n, rh=rh):
            seen["rows"] = n
            return torch.float32

        class PoolerStub(torch.nn.Module):
            def forward(self, feats, boxes, roi_scale=None, out_dtype=None, rois=None, rows=rows):
                seen["scale"], seen["out_dtype"] = roi_scale, out_dtype
                return torch.zeros(rows, 4, 7, 7)

        monkeypatch.setattr(rh, "_pool_dtype_for", pool_dtype)
        monkeypatch.setattr(rh, "box_pooler", PoolerStub())
        props = [Instances((64, 64), proposal_boxes=Boxes(torch.zeros(10, 4)), objectness_logits=torch.zeros(10))]
        with H.x3_mode("x2"):
            out = rh.pool_features({f: torch.zeros(1, 4, 8, 8) for f in rh.box_in_features}, props)
        assert out.shape[0] == rows and seen["rows"] == rows and seen["scale"] is scale and seen["out_dtype"] == torch.float32


def test_fused_entry_is_declared_and_registered():
    from wsovod_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "wsovod_hip.h")).read()
    m = re.search(r"\bint\s+wsovod_roi_loop_pool_forward_ex\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, "wsovod_roi_loop_pool_forward_ex is not declared in include/wsovod_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert "wsovod_roi_loop_pool_forward_ex" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wsovod_roi_loop_pool_forward_ex"]) == len(args) == 19
    assert any(a.endswith("roi_scale") for a in args) and any(a.endswith("out_hi") for a in args)
    assert _lib.ABI_VERSION == 9  # an additive entry: the ABI version stays
