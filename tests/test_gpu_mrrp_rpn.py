"""-m gpu: the MRRP RPN model (hot_path_r18_mrrp_rpn.yaml) against the reference's golden step g23, with the bars
tests/test_gpu_rpn.py uses for g12; eval inference; the VGG16 form; two optimizer steps."""
import numpy as np
import pytest
import torch

from tests.conftest import *  # noqa: F401,F403
from tests.golden import gen
from tests.helpers import load_golden, to_inputs
from tests.test_gpu_rpn import first_k_keys, match_fraction

pytestmark = pytest.mark.gpu


def build_model(precision="fp32", backbone="resnet", golden=None):
    from wsovod_amd.modeling import build_model as build
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(precision=precision, device="cuda:0", rpn=True, mrrp=True, backbone=backbone)
    cfg.SOLVER.MAX_ITER = 4000
    torch.manual_seed(0)
    model = build(cfg)
    if golden is not None:
        model._std = [float(v) for v in gen.PIXEL_STD]
        shapes = {str(k): eval(str(s)) for k, s in zip(golden["keys"], golden["shapes"])}
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
        model.load_state_dict(gen.seeded_state(shapes, 41), strict=True)
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    model.roi_heads.iter = 1000
    return cfg, model


def golden_step(model, g, monkeypatch):
    first_k_keys(model, monkeypatch)
    drawn = iter([g["loaded0/level_ids"], g["loaded1/level_ids"]])

    def fixed(rpn_ids, n):  # the ids the golden script drew for the loaded boxes
        return next(drawn).to(rpn_ids.device)

    monkeypatch.setattr(model, "_loaded_level_ids", fixed)
    losses = model(to_inputs(gen.seeded_batch(2, 40, 20, 256, 352, seed=int(g["batch_seed"]))))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return losses


@pytest.mark.parametrize("route", ["hip", "torch"])
def test_mrrp_rpn_step_matches_reference_golden(gpu, monkeypatch, route):
    from wsovod_amd.layers import hip_ops as H

    monkeypatch.setattr(H, "RPN_TOPK_ROUTE", route)
    g = load_golden("g23_mrrp_rpn")
    cfg, model = build_model("fp32", golden=g)
    losses = golden_step(model, g, monkeypatch)
    pg = model.proposal_generator
    assert len(pg.pred_objectness_logits) == 3 and len(pg.anchors) == 3
    print("label differences", int((pg.sampled_labels.cpu() != g["anchor_labels"]).sum()))
    assert (pg.sampled_labels.cpu() != g["anchor_labels"]).sum() <= 4
    for l in range(3):
        torch.testing.assert_close(pg.pred_objectness_logits[l].detach().cpu(), g[f"rpn_logits{l}"], rtol=1e-4, atol=2e-4)
    deltas = torch.cat([d.detach().cpu() for d in pg.pred_anchor_deltas], dim=1)
    torch.testing.assert_close(gen.strided_sample(deltas, 8192), g["rpn_deltas_sample"], rtol=1e-4, atol=2e-4)
    for i, p in enumerate(model.rpn_proposals):
        ref_b, ref_id = g[f"prop{i}/boxes"], g[f"prop{i}/level_ids"]
        got_b, got_id = p.proposal_boxes.tensor.cpu(), p.level_ids.cpu()
        assert got_id.dtype == torch.int64
        print("proposals", len(got_b), len(ref_b), match_fraction(ref_b, got_b), match_fraction(got_b, ref_b))
        assert abs(len(got_b) - len(ref_b)) <= 2
        assert match_fraction(ref_b, got_b) >= 0.95 and match_fraction(got_b, ref_b) >= 0.95
        d = (got_b[:, None, :] - ref_b[None, :, :]).abs().amax(dim=2)  # every matched box carries the golden's level id
        near = d < 0.05
        assert bool(((got_id[:, None] == ref_id[None, :]) & near).any(dim=1)[near.any(dim=1)].all())
        assert float(p.objectness_logits.max()) <= 0.25 + 1e-6
    for i, t in enumerate(model.roi_heads.proposal_targets):
        torch.testing.assert_close(t.gt_boxes.tensor.cpu(), g[f"target{i}/gt_boxes"], rtol=1e-4, atol=1e-2)
        assert torch.equal(t.gt_classes.cpu(), g[f"target{i}/gt_classes"])
    for k in ("loss_cls_object_mining", "loss_cls_r0", "loss_box_reg_r0", "loss_rpn_cls", "loss_rpn_loc"):
        print(k, float(losses[k]), float(g["loss/" + k]))
        torch.testing.assert_close(losses[k].detach().cpu(), g["loss/" + k], rtol=5e-3, atol=1e-5, msg=lambda m: f"{k}: {m}")
    for k, q in model.named_parameters():
        if q.requires_grad:
            ref, got = float(g["gradnorm/" + k]), float(q.grad.double().norm())
            assert abs(got - ref) <= 1e-2 * ref + 1e-6, (k, got, ref)


def test_parity_mode_mrrp_rpn_step_is_finite_and_close(gpu, monkeypatch):
    """The same g23 step in the parity precision (the branch-major trunk on bf16x2 maps, the RPN head on the fp32 map through
    the hi/lo operand split, L levels stacked along N), by the bars of tests/test_gpu_rpn.py's parity test of g12."""
    from tests import mrrp_rpn_util as U

    g = load_golden("g23_mrrp_rpn")
    cfg, model = build_model("parity", golden=g)
    losses = golden_step(model, g, monkeypatch)
    pg = model.proposal_generator
    for l in range(3):
        torch.testing.assert_close(pg.pred_objectness_logits[l].detach().cpu(), g[f"rpn_logits{l}"], rtol=1e-3, atol=1e-3)
    for k in ("loss_cls_object_mining", "loss_cls_r0", "loss_box_reg_r0"):
        print(k, float(losses[k]), float(g["loss/" + k]))
        torch.testing.assert_close(losses[k].detach().cpu(), g["loss/" + k], rtol=1e-2, atol=1e-5, msg=lambda m: f"{k}: {m}")
    targets = model.roi_heads.proposal_targets
    for i, t in enumerate(targets):
        assert torch.equal(t.gt_classes.cpu(), g[f"target{i}/gt_classes"])
        torch.testing.assert_close(t.gt_boxes.tensor.cpu(), g[f"target{i}/gt_boxes"], rtol=0, atol=0.1)
    same = torch.equal(pg.sampled_labels.cpu(), g["anchor_labels"])
    print("labels equal the golden's:", same, {k: float(losses[k]) for k in ("loss_rpn_cls", "loss_rpn_loc")})
    if same:
        for k in ("loss_rpn_cls", "loss_rpn_loc"):
            torch.testing.assert_close(losses[k].detach().cpu(), g["loss/" + k], rtol=1e-2, atol=1e-5, msg=lambda m: f"{k}: {m}")
    else:  # as the g12 test: labels and losses against the restatement on the model's OWN pseudo-GT boxes
        cls, loc, ref_labels = U.rpn_losses([a.tensor.cpu() for a in pg.anchors],
                                            [x.detach().float().cpu() for x in pg.pred_objectness_logits],
                                            [x.detach().float().cpu() for x in pg.pred_anchor_deltas],
                                            [t.gt_boxes.tensor.cpu() for t in targets], pg.box2box_transform, pg.anchor_matcher,
                                            gen.first_k_subsample, pg.batch_size_per_image, pg.positive_fraction)
        assert torch.equal(pg.sampled_labels.cpu().to(ref_labels.dtype), ref_labels)
        torch.testing.assert_close(losses["loss_rpn_cls"].detach().cpu(), cls, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(losses["loss_rpn_loc"].detach().cpu(), loc, rtol=1e-4, atol=1e-6)
    for k, q in model.named_parameters():
        if q.requires_grad:
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), k


def test_eval_inference_returns_level_ids(gpu):
    g = load_golden("g23_mrrp_rpn")
    cfg, model = build_model("fp32", golden=g)
    model.eval()
    inputs = to_inputs(gen.seeded_batch(2, 40, 20, 256, 352, seed=int(g["batch_seed"])))
    for x in inputs:
        x.pop("instances", None)
    out = model(inputs, classifier=torch.randn(20, 512, device="cuda"))
    assert len(out) == 2
    allowed = {l * 1000 + a for l in range(3) for a in range(6)}
    for p in model.rpn_proposals:
        assert len(p) > 0 and set(p.level_ids.tolist()) <= allowed and p.level_ids.dtype == torch.int64


def test_vgg16_mrrp_rpn_trains_and_the_rpn_weights_move(gpu):
    from wsovod_amd.data import make_batch
    from wsovod_amd.engine import build_optimizer, run_step
    from wsovod_amd.testing import build_hot_path_model

    cfg, model = build_hot_path_model(seed=0, precision="bf16", device="cuda:0", backbone="vgg16", mrrp=True, rpn=True)
    model.train()
    opt = build_optimizer(cfg, model)
    before = {k: v.detach().clone() for k, v in model.proposal_generator.named_parameters()}
    batch = make_batch(2, 64, 20, H=192, W=256, seed=3)
    for _ in range(2):
        losses = run_step(model, opt, batch)
        assert all(np.isfinite(float(v)) for v in losses.values()), losses
    assert {"loss_rpn_cls", "loss_rpn_loc"} <= set(losses)
    moved = [k for k, v in model.proposal_generator.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert "rpn_head.objectness_logits.weight" in moved and "rpn_head.conv.weight" in moved
