"""GPU: the MRRP ResNet models (hot_path_r18_mrrp / hot_path_r50_mrrp) above the kernels -- the uint8 entry against the
restatement tests/mrrp_resnet_util.py, the heads with mixed `level_ids` against the oracle composition (RoIPool and
ROILoopPool, the pooler the WSR MRRP configs select), the all-zero ids case against the map sliced to branch 0, the whole-step
HIP graph against the eager steps, and the two forms of the branched convs against each other."""
import pytest
import torch

from oracle import wsovod_ref as R
from tests import mrrp_resnet_util as U
from tests.golden import gen
from tests.helpers import to_inputs

pytestmark = pytest.mark.gpu
K = 20


def _lower_mx(monkeypatch):
    """Two small images: the f16mx run of res4 / res5 and of the heads needs its gates lowered, as the existing tests do."""
    from wsovod_amd.modeling.backbone import FrozenForwardMixin
    from wsovod_amd.modeling.roi_heads import WSOVODROIHeads

    monkeypatch.setattr(FrozenForwardMixin, "MX_MIN_TILES", 1)
    monkeypatch.setattr(WSOVODROIHeads, "MX_MIN_ROWS", 1)


def _build(precision, depth=18, pooler="ROIPool"):
    from wsovod_amd.testing import build_hot_path_model

    cfg, model = build_hot_path_model(seed=0, depth=depth, mrrp=True, K=K, precision=precision, pooler=pooler, device="cuda:0")
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    return cfg, model


def _batch():
    return gen.seeded_batch(2, 64, K, 96, 128, seed=22)


def _state(model):
    return {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}


def _backbone_map(model, batch):
    inputs = to_inputs(batch)
    canvas, sizes_t, _ = model._canvas(inputs)
    with torch.no_grad(), model._entered():
        return model.backbone.forward_uint8(canvas, sizes_t, model._mean, model._std)["res5"].float().cpu().contiguous()


def _restated_map(model, sd, batch, depth):
    x = R.preprocess_image([b["image"] for b in batch], tuple(model._mean), tuple(model._std))
    with torch.no_grad():
        return U.resnet_mrrp_ref(sd, x, depth)


@pytest.mark.parametrize("depth,precision", [(18, "fp32"), (18, "parity"), (18, "parity_mx"), (50, "parity"), (50, "parity_mx")])
def test_uint8_entry_matches_the_restatement(gpu, monkeypatch, depth, precision):
    """forward_uint8 on two 96 x 128 images: (3 * 2, C, 12, 16), branch-major, against resnet_mrrp_ref on the model's own weights.
    R18: the backbone-map bar of the VGG form, element by element (rtol 1e-3 / atol 3e-4).  R50: the bar the project holds the
    plain WSR_50 backbone to (tests/test_gpu_model_parity.py::test_r50_backbone_matches_reference_golden): 1e-3 of the map's
    peak value -- through 16 Bottlenecks a value next to the ReLU threshold is a cancelling sum of terms of the map's
    magnitude, so its error scales with the map, not with the element.
    Measured: R18 fp32 3.4e-5, parity 3.0e-4, parity_mx 5.4e-4 (peak 19.4); R50 parity 3.6e-3, parity_mx 7.8e-3 (peak 146:
    2.5e-5 / 5.3e-5 of it)."""
    if precision == "parity_mx":
        _lower_mx(monkeypatch)
    cfg, model = _build(precision, depth)
    got = _backbone_map(model, _batch())
    assert tuple(got.shape) == (6, U.RES5_CHANNELS[depth], 12, 16) and bool(torch.isfinite(got).all())
    want = _restated_map(model, _state(model), _batch(), depth)
    print(f"R{depth} {precision}: max |err| {float((got - want).abs().max()):.3e}, max |ref| {float(want.abs().max()):.3e}")
    if depth == 50:
        assert float((got - want).abs().max()) < 1e-3 * float(want.abs().max())
    else:
        torch.testing.assert_close(got, want, rtol=1e-3, atol=3e-4)


@pytest.mark.parametrize("precision", ["parity", "parity_mx"])
def test_both_forms_of_the_branched_convs_give_the_same_bits(gpu, monkeypatch, precision):
    """WSOVOD_BRANCH_BATCHED = 0 (the loop over the single-dilation launches) and = 1 (one launch per branched conv) on the
    uint8 entry of the R18 model: the same bits in the map that leaves the backbone."""
    if precision == "parity_mx":
        _lower_mx(monkeypatch)
    cfg, model = _build(precision)
    outs = {}
    for form in ("0", "1"):
        monkeypatch.setenv("WSOVOD_BRANCH_BATCHED", form)
        outs[form] = _backbone_map(model, _batch())
    diff = (outs["0"] - outs["1"]).abs()
    print(f"{precision}: loop against one launch: max |diff| {float(diff.max()):.3e}, differing values {int((diff > 0).sum())} of {diff.numel()}")
    assert torch.equal(outs["0"].view(torch.int32), outs["1"].view(torch.int32))


def _mixed_ids(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([0, 3, 1000, 1002, 2001])[torch.randint(0, 5, (n,), generator=g)]


def _oracle_heads(sd, fmap, batch, ids, pooler):
    """restatement map -> oracle.roi_pooler per branch (box r from the chunk level_ids[r] // 1000) -> neck_forward (+ the
    data-aware features of the branch mean) -> the mining head -> the open-vocabulary classifier."""
    with torch.no_grad():
        boxes = [b["boxes"] for b in batch]
        nums = [len(b) for b in boxes]
        rows, parts = sum(nums), 3 if pooler == "ROILoopPool" else 1
        per_branch = [R.roi_pooler(c, boxes, pooler, 7, 0.125, 0).reshape(parts, rows, -1, 7, 7) for c in torch.chunk(fmap, 3)]
        branch = torch.cat(ids) // 1000
        pooled = torch.stack([per_branch[int(b)][:, r] for r, b in enumerate(branch)], dim=1)  # (parts, rows, C, 7, 7)
        pooled = pooled * torch.cat([b["objectness"] + 1 for b in batch]).view(1, -1, 1, 1, 1)
        feats = [R.neck_forward(sd, p) for p in pooled]
        if any(k.startswith("data_aware_head.") for k in sd):
            daf = R.data_aware_forward(sd, torch.stack(torch.chunk(fmap, 3)).mean(0))
            rep = torch.cat([daf[i].repeat(n, 1) for i, n in enumerate(nums)])
            feats = [f + rep for f in feats]
        scores = R.mining_forward_contextlocnet(sd, *feats, nums) if parts == 3 else R.mining_forward(sd, feats[0], nums)
        return scores, R.ov_classifier_forward(sd, feats[0], "roi_heads.box_refinery_0.cls.", 50.0)


@pytest.mark.parametrize("pooler", ["ROIPool", "ROILoopPool"])
@pytest.mark.parametrize("precision", ["parity", "parity_mx"])
def test_whole_model_logits_hold_the_bar_with_mixed_level_ids(gpu, precision, pooler, monkeypatch):
    """Two images of 96 x 128, 64 proposals each, `level_ids` from {0, 3, 1000, 1002, 2001} set on the proposals before the heads:
    mining scores and refinement logits within the project's 1e-3 bar of the oracle composition; labels and pseudo-GT exact when
    the oracle mines from the HIP path's own scores."""
    from wsovod_amd.testing import capture_full_step

    if precision == "parity_mx":
        _lower_mx(monkeypatch)
    cfg, model = _build(precision, pooler=pooler)
    sd, batch = _state(model), _batch()
    ids = [_mixed_ids(len(b["boxes"]), 600 + i) for i, b in enumerate(batch)]
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
    want_scores, want_logits = _oracle_heads(sd, _restated_map(model, sd, batch, 18), batch, ids, pooler)
    e_score = float((out["mining_scores"] - want_scores).abs().max())
    e_logit = float((out["refine_logits"] - want_logits).abs().max())
    print(f"{precision} {pooler}: max |score err| {e_score:.3e}, max |logit err| {e_logit:.3e}")
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
    from wsovod_amd.data import make_batch
    from wsovod_amd.engine import HotPathTrainer, build_optimizer
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    monkeypatch.setenv("WSOVOD_STEP_GRAPH", step_graph)
    cfg = hot_path_cfg(depth=18, mrrp=True, K=K, precision=precision, device="cuda:0")
    cfg.MODEL.MRRP.NUM_BRANCH, cfg.MODEL.MRRP.BRANCH_DILATIONS = len(branches), list(branches)
    cfg.MODEL.ROI_BOX_HEAD.OPEN_VOCABULARY.DATA_AWARE = data_aware
    if guard:
        cfg.MODEL.HIP.MX_RANGE_GUARD = "raise"
    torch.manual_seed(0)
    model = build_model(cfg)
    with torch.no_grad():
        model.backbone.stem.conv1.norm.weight.fill_(1.0 / 64.0)
    if state is not None:
        model.load_state_dict(state, strict=True)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    cfg.SOLVER.BASE_LR = 1e-3
    batch = make_batch(2, 64, K, H=96, W=128, seed=141)  # (equal image shapes: the layout a step graph is keyed on)
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
    """HotPathTrainer on the hot_path_r18_mrrp model, dropout on, five steps: the whole-step HIP graph (captured on the third
    step, replayed after; the routing rewrite is inside it) against WSOVOD_STEP_GRAPH=0 -- labels equal step by step, losses and
    trained parameters to the bounds of tests/test_gpu_graph.py::test_whole_step_graph_reproduces_the_eager_steps.  parity_mx
    runs with the range guard in `raise` mode: a step that ends is a clean step."""
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
    """Without a proposal generator every level id is 0: every box pools from branch 0.  Four steps under the whole-step graph of
    the three-branch model against the SAME weights on a backbone that emits branch 0's map alone (NUM_BRANCH 1, dilation 1):
    losses, labels and updated head weights are equal bit for bit.  The data-aware head is off in both: its input is by
    definition the mean over ALL branches, which a map sliced to branch 0 does not carry."""
    from wsovod_amd.layers import hip_ops as H

    monkeypatch.setattr(H, "DETERMINISTIC", True)
    monkeypatch.setenv("WSOVOD_BACKBONE_GRAPH", "0")
    three = _train_run(gpu, monkeypatch, "parity", "1", (1, 2, 4), 4, data_aware=False)
    one = _train_run(gpu, monkeypatch, "parity", "1", (1,), 4, state=three[3], data_aware=False)
    assert three[2] == one[2] == ["_StepGraph"]
    for (la, ga), (lb, gb) in zip(three[0], one[0]):
        assert la == lb and torch.equal(ga, gb)
    assert three[1].keys() == one[1].keys() and all(torch.equal(v, one[1][k]) for k, v in three[1].items())
