"""GPU: the MRRP VGG16 model above the backbone -- the uint8 entry against the restatement, the heads' routing of boxes to
branches against the reference pooler's golden (g21), the data-aware head against the reference's (g21), the all-zero
level_ids case against the same model fed the map sliced to branch 0, and one trainer step with the range guard raising."""
import os

import numpy as np
import pytest
import torch

from oracle import wsovod_ref as R
from tests import mrrp_util
from tests.golden import gen
from tests.helpers import to_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G21 = np.load(os.path.join(ROOT, "tests", "golden", "g21_vgg16_mrrp.npz"), allow_pickle=False)
K = 20
V16_MEAN = (103.939, 116.779, 123.68)


def _build(precision, pooler="ROIPool"):
    from wsovod_amd.testing import build_hot_path_model

    cfg, model = build_hot_path_model(seed=0, backbone="vgg16", mrrp=True, K=K, precision=precision, pooler=pooler, device="cuda:0")
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    return cfg, model


def _batch():
    return gen.seeded_batch(2, 64, K, 96, 128, seed=21)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "parity", "parity_mx"])
def test_uint8_entry_matches_the_restatement(gpu, precision, monkeypatch):
    """forward_uint8 and the float entry: (3 * 2, 512, 11, 15), branch-major; fp32, parity and parity_mx against vgg16_mrrp_ref with the
    backbone-map bar of tests/test_gpu_vgg_model.py (rtol 1e-3 / atol 3e-4); bf16 (8 mantissa bits through 13 conv layers)
    is held to the shape, finiteness and the branch order: chunk 1 (dilation 2) is the plain bf16 model's map, bit for bit."""
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.testing import build_hot_path_model

    if precision == "parity_mx":  # (two small images: the f16mx run from plain3 on needs the gate lowered, as the VGG tests do)
        from wsovod_amd.modeling.backbone_vgg import VGG16

        monkeypatch.setattr(VGG16, "MX_MIN_TILES", 1)
    cfg, model = _build(precision)
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    inputs = to_inputs(_batch())
    canvas, sizes_t, _ = model._canvas(inputs)
    with torch.no_grad(), model._entered():
        got = model.backbone.forward_uint8(canvas, sizes_t, model._mean, model._std)["plain5"].float().cpu().contiguous()
    assert tuple(got.shape) == (6, 512, 11, 15) and bool(torch.isfinite(got).all())
    if precision == "bf16":
        _, plain = build_hot_path_model(seed=0, backbone="vgg16", K=K, precision="bf16", device="cuda:0")
        plain.backbone.load_state_dict(model.backbone.state_dict(), strict=True)
        with torch.no_grad():
            want = plain.backbone.forward_uint8(canvas, sizes_t, model._mean, model._std)["plain5"].float().cpu()
        assert torch.equal(got[2:4], want)
        return
    x = R.preprocess_image([b["image"] for b in _batch()], V16_MEAN, (1.0, 1.0, 1.0))
    want = mrrp_util.vgg16_mrrp_ref(sd, x, dilations=(1, 2, 4), prefix="backbone.")
    print(precision, "max |err|", float((got - want).abs().max()), "max |ref|", float(want.abs().max()))
    torch.testing.assert_close(got, want, rtol=1e-3, atol=3e-4)
    xf = model.preprocess_image(inputs).tensor
    torch.testing.assert_close(model.backbone(xf)["plain5"].float().cpu().contiguous(), want, rtol=1e-3, atol=3e-4)


def _routing_proposals(gpu, zero_ids=False):
    from wsovod_amd.structures import Boxes, Instances

    boxes, ids = torch.from_numpy(G21["route_boxes"]), torch.from_numpy(G21["route_level_ids"])
    return [Instances((72, 88), proposal_boxes=Boxes(boxes[n].to(gpu)), objectness_logits=torch.zeros(12, device=gpu),
                      level_ids=(torch.zeros_like(ids[n]) if zero_ids else ids[n]).to(gpu)) for n in range(2)]


def test_roi_pool_routing_equals_the_reference_poolers_golden(gpu):
    """RoIPool in fp32 is max over cells: exact against the reference's `ROIPooler(level_ids=...)` over the chunked map."""
    cfg, model = _build("fp32")
    fmap = torch.from_numpy(G21["route_map"]).to(gpu).contiguous(memory_format=torch.channels_last)
    got = model.roi_heads.pool_features({"plain5": fmap}, _routing_proposals(gpu))
    assert torch.equal(got.float().cpu().reshape(24, 32, 7, 7), torch.from_numpy(G21["routed_pool"]))


@pytest.mark.parametrize("pooler", ["ROIPool", "ROIAlignV2", "ROILoopPool"])
def test_pooled_features_equal_the_per_branch_oracle_pooling(gpu, pooler):
    """Mixed level_ids: box r against the oracle pooler on ITS branch's chunk of the map (RoIPool / ROILoopPool: maxima, exact;
    ROIAlignV2: bilinear sums in fp32, 1e-5 relative to the map's largest value).  All ids zero: bit for bit the same heads
    without MRRP on the map sliced to branch 0."""
    cfg, model = _build("fp32", pooler=pooler)
    rh = model.roi_heads
    fmap_cpu = torch.from_numpy(G21["route_map"])
    fmap = fmap_cpu.to(gpu).contiguous(memory_format=torch.channels_last)
    boxes, ids = torch.from_numpy(G21["route_boxes"]), torch.from_numpy(G21["route_level_ids"])
    got = rh.pool_features({"plain5": fmap}, _routing_proposals(gpu)).float().cpu()
    parts = 3 if pooler == "ROILoopPool" else 1
    got = got.reshape(parts, 24, 32, 7, 7)
    per_branch = [R.roi_pooler(chunk, list(boxes), pooler).reshape(parts, 24, 32, 7, 7) for chunk in torch.chunk(fmap_cpu, 3)]
    branch = (ids // 1000).flatten()
    want = torch.stack([per_branch[int(b)][:, r] for r, b in enumerate(branch)], dim=1)
    if pooler == "ROIAlignV2":
        assert float((got - want).abs().max()) <= 1e-5 * float(fmap_cpu.abs().max())
    else:
        assert torch.equal(got, want)
    zero = rh.pool_features({"plain5": fmap}, _routing_proposals(gpu, zero_ids=True)).clone()
    rh.mrrp_on = False
    try:
        sliced = rh.pool_features({"plain5": fmap[:2].contiguous(memory_format=torch.channels_last)}, _routing_proposals(gpu, zero_ids=True))
    finally:
        rh.mrrp_on = True
    assert torch.equal(zero, sliced)


def test_data_aware_features_equal_the_references(gpu):
    """The mean over the branches' GAP rows against the reference head's mean over the branch maps before its GAP: fp32
    sums of 99 cells in another order, 1e-5 relative."""
    from wsovod_amd.modeling.class_heads import DataAwareFeaturesHead
    from wsovod_amd.structures import ShapeSpec

    head = DataAwareFeaturesHead({"plain5": ShapeSpec(channels=32)}, datasets_prototype_num=5, features_dim=24,
                                 cls_in_features=["plain5"], mrrp_on=True, mrrp_num_branch=3)
    head.load_state_dict({k[len("daf_sd."):]: torch.from_numpy(G21[k]) for k in G21.files if k.startswith("daf_sd.")}, strict=True)
    head = head.to(gpu)
    fmap = torch.from_numpy(G21["route_map"]).to(gpu).contiguous(memory_format=torch.channels_last)
    nums = G21["daf_nums"].tolist()
    with torch.no_grad():
        got = head({"plain5": fmap}, [range(n) for n in nums]).float().cpu()
    want = torch.from_numpy(G21["daf"])
    assert got.shape == want.shape == (sum(nums), 24)
    assert float((got - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


def _lower_mx(monkeypatch):
    from wsovod_amd.modeling.backbone_vgg import VGG16
    from wsovod_amd.modeling.roi_heads import WSOVODROIHeads

    monkeypatch.setattr(VGG16, "MX_MIN_TILES", 1)
    monkeypatch.setattr(WSOVODROIHeads, "MX_MIN_ROWS", 1)


def _mixed_ids(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([0, 3, 1000, 1002, 2001])[torch.randint(0, 5, (n,), generator=g)]


_ORACLE = {}


def _oracle_heads(sd, batch, ids):
    """vgg16_mrrp_ref -> oracle.roi_pooler per branch (box r from the chunk level_ids[r] // 1000) -> neck_forward ->
    (+ data-aware features of the branch mean) -> mining_forward -> ov_classifier_forward.  Computed once per weight set."""
    key = float(sd["backbone.plain3.0.conv1.weight"].double().sum())
    if key not in _ORACLE:
        with torch.no_grad():
            x = R.preprocess_image([b["image"] for b in batch], V16_MEAN, (1.0, 1.0, 1.0))
            fmap = mrrp_util.vgg16_mrrp_ref(sd, x, dilations=(1, 2, 4), prefix="backbone.")
            boxes = [b["boxes"] for b in batch]
            nums = [len(b) for b in boxes]
            per_branch = [R.roi_pooler(c, boxes, "ROIPool", 7, 0.125, 0) for c in torch.chunk(fmap, 3)]
            branch = torch.cat(ids) // 1000
            pooled = torch.stack([per_branch[int(b)][r] for r, b in enumerate(branch)])
            pooled = pooled * torch.cat([b["objectness"] + 1 for b in batch]).view(-1, 1, 1, 1)
            feat = R.neck_forward(sd, pooled)
            daf = R.data_aware_forward(sd, torch.stack(torch.chunk(fmap, 3)).mean(0))
            feat = feat + torch.cat([daf[i].repeat(n, 1) for i, n in enumerate(nums)])
            _ORACLE[key] = (R.mining_forward(sd, feat, nums),
                            R.ov_classifier_forward(sd, feat, "roi_heads.box_refinery_0.cls.", 50.0))
    return _ORACLE[key]


@pytest.mark.parametrize("precision", ["parity", "parity_mx"])
def test_whole_model_logits_hold_the_bar_with_mixed_level_ids(gpu, precision, monkeypatch):
    """Two images of 256 x 352 (the second ragged), 64 / 57 proposals, `level_ids` from {0, 3, 1000, 1002, 2001} set on the
    proposals before the heads: mining scores and refinement logits within the project's 1e-3 bar of the oracle composition;
    labels and pseudo-GT exact when the oracle mines from the HIP path's own scores.
    Measured: parity 7.0e-9 (scores) / 8.0e-5 (logits); parity_mx 1.8e-8 / 1.3e-4."""
    from wsovod_amd.testing import capture_full_step

    if precision == "parity_mx":
        _lower_mx(monkeypatch)
    cfg, model = _build(precision)
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    batch = gen.seeded_batch(2, 64, K, 256, 352, seed=31)
    ids = [_mixed_ids(len(b["boxes"]), 500 + i) for i, b in enumerate(batch)]
    assert len({int(v) // 1000 for t in ids for v in t}) == 3
    inputs = to_inputs(batch)
    dev_inputs = [{**x, "image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu)} for x in inputs]
    plain = model._proposals

    def with_ids(batched_inputs):  # the ids an MRRP proposal generator would have set (rcnn_wsovod.py:177-197)
        props = plain(batched_inputs)
        for p, t in zip(props, ids):
            p.level_ids = t.to(gpu)
        return props

    monkeypatch.setattr(model, "_proposals", with_ids)
    out = capture_full_step(model, dev_inputs)
    want_scores, want_logits = _oracle_heads(sd, batch, ids)
    e_score = float((out["mining_scores"] - want_scores).abs().max())
    e_logit = float((out["refine_logits"] - want_logits).abs().max())
    print(f"{precision}: max |score err| {e_score:.3e}, max |logit err| {e_logit:.3e}")
    assert e_score < 1e-3 and e_logit < 1e-3
    nums = [len(b["boxes"]) for b in batch]
    gt_int, _ = R.get_image_level_gt([b["gt_classes"] for b in batch], K)
    tg = R.get_pgt_top_k([b["boxes"] for b in batch], list(out["mining_scores"].split(nums)), gt_int, out["img_scores"], K)
    lab = R.label_and_sample_proposals_wsl([b["boxes"] for b in batch], tg, K)
    assert out["pgt_num"] == [len(t["gt_classes"]) for t in tg]
    assert torch.equal(out["pgt_boxes"], torch.cat([t["gt_boxes"] for t in tg]))
    assert torch.equal(out["pgt_classes"], torch.cat([t["gt_classes"] for t in tg]))
    assert torch.equal(out["gt_classes"], torch.cat([l["gt_classes"] for l in lab]))
    assert torch.equal(out["gt_boxes"], torch.cat([l["gt_boxes"] for l in lab]))


def _train_run(gpu, monkeypatch, precision, step_graph, branches, steps, guard=False, state=None, data_aware=True):
    from wsovod_amd.engine import HotPathTrainer, build_optimizer
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    monkeypatch.setenv("WSOVOD_STEP_GRAPH", step_graph)
    cfg = hot_path_cfg(backbone="vgg16", mrrp=True, K=K, precision=precision, device="cuda:0")
    cfg.MODEL.MRRP.NUM_BRANCH, cfg.MODEL.MRRP.BRANCH_DILATIONS = len(branches), list(branches)
    cfg.MODEL.ROI_BOX_HEAD.OPEN_VOCABULARY.DATA_AWARE = data_aware
    if guard:
        cfg.MODEL.HIP.MX_RANGE_GUARD = "raise"
    torch.manual_seed(0)
    model = build_model(cfg)
    with torch.no_grad():
        model.backbone.plain1[0].conv1.weight.mul_(1.0 / 64.0)
    if state is not None:
        model.load_state_dict(state, strict=True)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    cfg.SOLVER.BASE_LR = 1e-3
    from wsovod_amd.data import make_batch

    batch = make_batch(2, 64, K, H=96, W=128, seed=140)  # (equal image shapes: the layout a step graph is keyed on)
    tr = HotPathTrainer(model, build_optimizer(cfg, model))
    hist = []
    try:
        for _ in range(steps):
            losses = tr.run_step(batch)
            pgt = model.roi_heads._last_pgt
            rows = sum(len(x["proposals"]) for x in batch)
            hist.append(({k: float(v.detach()) for k, v in losses.items()}, pgt["gt_classes"][:rows].cpu().clone()))
        graphs = [type(g).__name__ for g in tr._graphs.values()]
        tr.flush()
        torch.cuda.synchronize()
        params = {k: v.detach().clone() for k, v in model.named_parameters() if v.requires_grad}
    finally:
        tr.close()
    return hist, params, graphs, start


@pytest.mark.parametrize("precision", ["parity", "parity_mx"])
def test_whole_step_graph_replay_equals_eager(gpu, precision, monkeypatch):
    """HotPathTrainer on the hot_path_vgg16_mrrp model, dropout on, five steps: the whole-step HIP graph (captured on the
    third step, replayed after; the routing rewrite is inside it) against WSOVOD_STEP_GRAPH=0 -- labels equal step by step,
    losses and trained parameters to the bounds of tests/test_gpu_graph.py::test_whole_step_graph_reproduces_the_eager_steps.
    parity_mx runs with the range guard in `raise` mode: a step that ends is a clean step."""
    from wsovod_amd.layers import hip_ops as H

    monkeypatch.setattr(H, "DETERMINISTIC", True)
    monkeypatch.setenv("WSOVOD_BACKBONE_GRAPH", "0")
    mx = precision == "parity_mx"
    if mx:
        _lower_mx(monkeypatch)
    eager = _train_run(gpu, monkeypatch, precision, "0", (1, 2, 4), 5, guard=mx)
    graph = _train_run(gpu, monkeypatch, precision, "1", (1, 2, 4), 5, guard=mx)
    assert eager[2] == [] and graph[2] == ["_StepGraph"]
    for s, (e, g) in enumerate(zip(eager[0], graph[0])):
        assert torch.equal(e[1], g[1]), s
        for k in e[0]:
            assert abs(e[0][k] - g[0][k]) <= 2e-5 * max(abs(e[0][k]), 1e-3), (s, k, e[0][k], g[0][k])
    for k, v in eager[1].items():
        torch.testing.assert_close(graph[1][k], v, rtol=1e-5, atol=2e-6 * float(v.abs().max()) + 1e-9, msg=lambda m: f"{k}: {m}")


def test_zero_level_ids_train_like_the_branch_0_map_bit_for_bit(gpu, monkeypatch):
    """Without a proposal generator every level id is 0 (rcnn_wsovod.py:198-203): every box pools from branch 0.  Three steps
    under the whole-step graph of the three-branch model against the SAME weights on a backbone that emits branch 0's map
    alone (NUM_BRANCH 1, dilation 1): losses, labels and updated head weights are equal bit for bit.  The data-aware head is
    off in both: its input is by definition the mean over ALL branches (data_aware_features_head.py:110-111), which a map
    sliced to branch 0 does not carry."""
    from wsovod_amd.layers import hip_ops as H

    monkeypatch.setattr(H, "DETERMINISTIC", True)
    monkeypatch.setenv("WSOVOD_BACKBONE_GRAPH", "0")
    three = _train_run(gpu, monkeypatch, "parity", "1", (1, 2, 4), 4, data_aware=False)
    one = _train_run(gpu, monkeypatch, "parity", "1", (1,), 4, state=three[3], data_aware=False)
    assert three[2] == one[2] == ["_StepGraph"]
    for (la, ga), (lb, gb) in zip(three[0], one[0]):
        assert la == lb and torch.equal(ga, gb)
    assert three[1].keys() == one[1].keys() and all(torch.equal(v, one[1][k]) for k, v in three[1].items())
