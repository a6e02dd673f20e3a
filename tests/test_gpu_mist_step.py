"""-m gpu: whole training steps with WSOVOD.INSTANCE_REFINEMENT.REFINE_MIST on the HIP path against the reference's own
steps (tests/golden/g24_mist.npz: g8's shapes, REFINE_NUM 1 and 2), the mixed-dataset heads against the restatement, and
the mining + labelling call without a host read."""
import pytest
import torch

from tests import mist_util as U
from tests.conftest import *  # noqa: F401,F403
from tests.golden import gen
from tests.helpers import load_golden, to_inputs

pytestmark = pytest.mark.gpu

K = 20


def set_refine_num(cfg, n):  # (as tests/golden/make_golden_mist.py sets it for the reference)
    cfg.WSOVOD.INSTANCE_REFINEMENT.REFINE_NUM = n
    cfg.WSOVOD.INSTANCE_REFINEMENT.REFINE_REG = [True] * n
    cfg.WSOVOD.SAMPLING.IOU_THRESHOLDS = [[0.5]] * n
    cfg.WSOVOD.SAMPLING.IOU_LABELS = [[0, 1]] * n
    cfg.WSOVOD.SAMPLING.BATCH_SIZE_PER_IMAGE = [4096] * n
    cfg.WSOVOD.SAMPLING.POSITIVE_FRACTION = [1.0] * n


def build_mist_model(precision, refine_num):
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(mist=True, precision=precision, device="cuda:0")
    set_refine_num(cfg, refine_num)
    cfg.MODEL.PIXEL_STD = list(gen.PIXEL_STD)
    torch.manual_seed(0)
    model = build_model(cfg)
    assert model.roi_heads.refine_mist and model.roi_heads.refine_K == refine_num
    model._std = [float(v) for v in gen.PIXEL_STD]
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(gen.seeded_state(shapes, seed=1), strict=True)
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    return model


def run_capturing(model, batch):
    """One forward + backward; -> (losses, [(head k's mining inputs, result dict)])."""
    rh, calls = model.roi_heads, []
    orig = rh.mine_and_label

    def wrapped(k, scores, boxes, proposals, seg, nums):
        o, pk = orig(k, scores, boxes, proposals, seg, nums)
        calls.append(((k, scores, boxes, proposals, seg, nums), o))
        return o, pk

    rh.mine_and_label = wrapped
    try:
        losses = model(to_inputs(batch))
    finally:
        del rh.mine_and_label
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return losses, calls


def targets_of(o):
    """The capacity-padded target rows of a MIST result, concatenated image by image."""
    start, count = o["pgt_start"].cpu().tolist(), o["pgt_count"].cpu().tolist()
    rows = torch.cat([torch.arange(s, s + c) for s, c in zip(start, count)])
    return count, {k: o[k].cpu()[rows] for k in ("pgt_boxes", "pgt_classes", "pgt_scores", "pgt_weights", "pgt_index")}


def check_step_against_golden(precision, refine_num, monkeypatch):
    g = load_golden("g24_mist")
    if precision == "parity_mx":  # the small golden case: lower the thresholds so that the f16mx kernels are what runs
        from wsovod_amd.modeling.backbone import ResNet
        from wsovod_amd.modeling.roi_heads import WSOVODROIHeads

        monkeypatch.setattr(ResNet, "MX_MIN_TILES", 1)
        monkeypatch.setattr(WSOVODROIHeads, "MX_MIN_ROWS", 1)
    model = build_mist_model(precision, refine_num)
    p = f"step{refine_num}/"
    batch = gen.seeded_batch(4, 64, K, 320, 416, seed=int(g[p + "batch_seed"]))
    losses, calls = run_capturing(model, batch)
    assert len(calls) == refine_num
    for h, ((_, scores, boxes, _, seg, _), o) in enumerate(calls):
        q = p + f"head{h}/"
        count, t = targets_of(o)
        assert count == g[q + "pgt_num"].tolist(), (h, count)
        assert torch.equal(t["pgt_classes"], g[q + "pgt_classes"]), h
        assert torch.equal(o["gt_classes"].cpu(), g[q + "gt_classes"]), h  # every proposal's label
        if h == 0:  # the first head mines the loaded proposals themselves: copies, bit for bit
            assert torch.equal(t["pgt_boxes"], g[q + "pgt_boxes"]) and torch.equal(o["gt_boxes"].cpu(), g[q + "gt_boxes"])
        else:
            # later heads mine the boxes the previous head regressed: floats the fp32 forward reproduces to ~5e-3 px, held
            # to the 1e-2 px bar this tree holds regressed pseudo-GT boxes to (g23).  WHICH boxes are mined, their classes
            # and order, and every label are exact: the generator asserts that the golden's decisions sit 2e-3 in IoU away
            # from such a move and survive a 1e-2 px perturbation (tests/golden/make_golden_mist.py:check_conditions)
            torch.testing.assert_close(t["pgt_boxes"], g[q + "pgt_boxes"], rtol=1e-3, atol=1e-2)
            torch.testing.assert_close(o["gt_boxes"].cpu(), g[q + "gt_boxes"], rtol=1e-3, atol=1e-2)
            # and, on this head's own device inputs, the restatement bit for bit
            sg = seg.cpu().tolist()
            want = U.mine_and_label([boxes[sg[i]:sg[i + 1]].cpu() for i in range(4)],
                                    [scores[sg[i]:sg[i + 1]].float().cpu() for i in range(4)],
                                    [torch.unique(b["gt_classes"]) for b in batch], K, 0.5,
                                    proposal_boxes=[b["boxes"] for b in batch])
            assert torch.equal(o["gt_classes"].cpu(), torch.cat([w[1]["gt_classes"] for w in want]))
            assert torch.equal(o["gt_boxes"].cpu(), torch.cat([w[1]["gt_boxes"] for w in want]))
            assert torch.equal(t["pgt_index"].long(), torch.cat([w[0]["index"] for w in want]))
        torch.testing.assert_close(t["pgt_scores"], g[q + "pgt_scores"], rtol=1e-3, atol=1e-5)
        torch.testing.assert_close(o["gt_weights"].cpu(), g[q + "gt_weights"], rtol=1e-3, atol=1e-5)
        assert torch.equal(t["pgt_weights"], t["pgt_scores"])
    names = ["loss_cls_object_mining"] + [f"loss_{n}_r{h}" for h in range(refine_num) for n in ("cls", "box_reg")]
    for k in names:  # tests/test_gpu_model_parity.py's bars for g8 under fp32 / parity / parity_mx
        torch.testing.assert_close(losses[k].detach().cpu(), g[p + "loss/" + k], rtol=1e-3, atol=1e-5, msg=lambda m: f"{k}: {m}")


@pytest.mark.parametrize("refine_num", [1, 2])
def test_fp32_mist_step_matches_the_reference(gpu, refine_num, monkeypatch):
    check_step_against_golden("fp32", refine_num, monkeypatch)


@pytest.mark.parametrize("precision", ["parity", "parity_mx"])
def test_parity_modes_mist_step_matches_the_reference(gpu, precision, monkeypatch):
    check_step_against_golden(precision, 2, monkeypatch)


def test_mixed_dataset_heads_mine_with_their_sources_class_count(gpu):
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import mixed_datasets_cfg

    Ks = (20, 20, 80)
    cfg = mixed_datasets_cfg(Ks=Ks, precision="fp32", device="cuda:0", mist=True)
    torch.manual_seed(0)
    model = build_model(cfg)
    assert type(model.roi_heads).__name__ == "WSOVODMixedDatasetsROIHeads" and model.roi_heads.refine_mist
    model._std = [float(v) for v in gen.PIXEL_STD]
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(gen.mixed_seeded_state(shapes, seed=17), strict=True)
    model.train()
    for source_id in (2, 0):
        Ksrc = Ks[source_id]
        batch = gen.seeded_batch(2, 40, Ksrc, 256, 352, seed=19 + source_id)
        for b in batch:
            b["dataset_id"] = source_id
        model.zero_grad(set_to_none=True)
        losses, calls = run_capturing(model, batch)
        assert all(bool(torch.isfinite(v)) for v in losses.values())
        (_, scores, boxes, _, seg, nums), o = calls[0]
        assert scores.shape[1] == Ksrc
        seg = seg.cpu().tolist()
        count, t = targets_of(o)
        classes = [torch.unique(b["gt_classes"]) for b in batch]
        want = U.mine_and_label([boxes[seg[i]:seg[i + 1]].cpu() for i in range(2)],
                                [scores[seg[i]:seg[i + 1]].float().cpu() for i in range(2)], classes, Ksrc, 0.5)
        assert count == [len(w[0]["gt_classes"]) for w in want]
        assert torch.equal(t["pgt_classes"], torch.cat([w[0]["gt_classes"] for w in want]))
        assert torch.equal(t["pgt_index"].long(), torch.cat([w[0]["index"] for w in want]))
        assert torch.equal(t["pgt_boxes"], torch.cat([w[0]["gt_boxes"] for w in want]))
        assert torch.equal(o["gt_classes"].cpu(), torch.cat([w[1]["gt_classes"] for w in want]))
        assert torch.equal(o["gt_boxes"].cpu(), torch.cat([w[1]["gt_boxes"] for w in want]))
        assert torch.equal(o["gt_weights"].cpu(), torch.cat([w[1]["gt_weights"] for w in want]))
        assert int(o["gt_classes"].max()) <= Ksrc


def _sync_debug_mode_is_enforced():
    """Whether torch raises on a synchronising call under set_sync_debug_mode("error") on this build."""
    x = torch.ones(4, device="cuda")
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.sum().item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(prev)


def test_mining_and_labelling_read_nothing_back(gpu):
    model = build_mist_model("fp32", 2)
    _, calls = run_capturing(model, gen.seeded_batch(4, 64, K, 320, 416, seed=2))
    (k, scores, boxes, proposals, seg, nums), eager = calls[1]
    rh = model.roi_heads
    keys = ("pgt_boxes", "pgt_classes", "pgt_scores", "pgt_index", "pgt_count", "gt_classes", "gt_boxes", "gt_weights", "matched")
    if _sync_debug_mode_is_enforced():
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            o, _ = rh.mine_and_label(k, scores, boxes, proposals, seg, nums)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        for name in keys:
            assert torch.equal(o[name], eager[name]), name
        return
    # this torch does not enforce the mode here: a captured graph cannot contain a host read, and a replay on fresh
    # scores must equal the eager call bit for bit
    static_scores = scores.clone()
    fresh = torch.softmax(torch.randn(scores.shape, generator=torch.Generator().manual_seed(9)) * 3, dim=1).to(scores.device)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rh.mine_and_label(k, static_scores, boxes, proposals, seg, nums)  # (warm-up: one-time function attributes)
        with torch.cuda.graph(graph, stream=side):
            o, _ = rh.mine_and_label(k, static_scores, boxes, proposals, seg, nums)
    torch.cuda.current_stream().wait_stream(side)
    static_scores.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    want, _ = rh.mine_and_label(k, fresh, boxes, proposals, seg, nums)
    for name in keys:
        assert torch.equal(o[name], want[name]), name
    assert not torch.equal(want["gt_classes"], eager["gt_classes"]) or not torch.equal(want["pgt_index"], eager["pgt_index"])
