"""A resume -- model and optimizer state dicts loaded into a HotPathTrainer's model / optimizer -- continues exactly as a fresh
load does, in every precision, with eager steps and with whole-step HIP graphs (WSOVOD_STEP_GRAPH).

What a checkpoint does NOT hold, as in the reference (its checkpointer saves the model and the optimizer, the iteration comes
back through `resume_or_load` / start_iter): the neck's dropout step counters (`box_head._step`, set through `set_step`) and
`roi_heads.iter`.  Dropout is off here, so the counters draw no mask; they are set to the checkpoint's step anyway, so that the
runs compared hold the same host state."""
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

CKPT_STEPS = 3


def _batches(gpu, n, seed):
    from wsovod_amd.data import make_batch

    out = []
    for s in range(n):
        b = make_batch(2, 64, 20, H=160, W=224, seed=seed + s)
        out.append([{"image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu), "instances": x["instances"],
                     "height": x["height"], "width": x["width"]} for x in b])
    return out


def _trainer(monkeypatch, precision, fused, graph):
    from wsovod_amd.engine import HotPathTrainer, build_optimizer
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.testing import build_hot_path_model

    monkeypatch.setattr(H, "DETERMINISTIC", True)
    monkeypatch.setenv("WSOVOD_BACKBONE_GRAPH", "0")
    monkeypatch.setenv("WSOVOD_FUSED_SGD", "1" if fused else "0")
    monkeypatch.setenv("WSOVOD_STEP_GRAPH", "1" if graph else "0")
    if precision == "parity_mx":  # (two small images: below the mode's tile-count thresholds -- lowered, the f16mx kernels run)
        from wsovod_amd.modeling.backbone import ResNet
        from wsovod_amd.modeling.roi_heads import WSOVODROIHeads

        monkeypatch.setattr(ResNet, "MX_MIN_TILES", 1)
        monkeypatch.setattr(WSOVODROIHeads, "MX_MIN_ROWS", 1)
    cfg, model = build_hot_path_model(seed=0, precision=precision, device="cuda:0")
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    cfg.SOLVER.BASE_LR = 1e-3
    tr = HotPathTrainer(model, build_optimizer(cfg, model))
    assert bool(tr._fused) == fused
    return model, tr


def _run(tr, batches, first_step):
    """Steps under a moving learning rate: a scheduler sets the LIVE param groups before every step."""
    losses = []
    for s, b in enumerate(batches):
        for grp in tr.optimizer.param_groups:
            grp["lr"] = 2e-3 * (1 + 0.5 * (first_step + s))
        losses.append({k: float(v) for k, v in tr.run_step(b).items()})
    return losses


def _load(model, tr, ckpt, step):
    sd, osd = torch.load(io.BytesIO(ckpt), map_location="cpu")  # (CPU tensors, as a checkpoint file gives them)
    model.load_state_dict(sd)
    tr.optimizer.load_state_dict(osd)
    tr.iter = step  # the counters the checkpoint does not hold (module docstring)
    model.roi_heads.iter = step
    for m in model.modules():
        if hasattr(m, "set_step"):
            m.set_step(step)


def _result(model, tr, losses):
    tr.flush()
    fc1 = model.roi_heads.box_head.fc1.weight
    out = {"params": {k: v.detach().clone() for k, v in model.named_parameters() if v.requires_grad},
           "mom_fc1": tr.optimizer.state[fc1]["momentum_buffer"].clone(), "losses": losses,
           "calls": tr._fused[0]._fused_update.calls if tr._fused else 0, "graphs": len(tr._graphs)}
    tr.close()
    return out


def _assert_same(a, b, what):
    for s, (sa, sb) in enumerate(zip(a["losses"], b["losses"])):
        for k in sa:
            assert abs(sa[k] - sb[k]) <= 2e-5 * max(abs(sb[k]), 1e-3), (what, s, k, sa[k], sb[k])
    for k, v in b["params"].items():
        torch.testing.assert_close(a["params"][k], v, rtol=1e-5, atol=2e-6 * float(v.abs().max()) + 1e-9,
                                   msg=lambda m: f"{what} {k}: {m}")
    torch.testing.assert_close(a["mom_fc1"], b["mom_fc1"], rtol=1e-5, atol=1e-6 * float(b["mom_fc1"].abs().max()) + 1e-12,
                               msg=lambda m: f"{what} fc1 momentum: {m}")


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("precision", ["bf16", "parity", "parity_mx"])
def test_resume_equals_a_fresh_load(gpu, monkeypatch, precision, graph):
    """Checkpoint C = model + optimizer state dicts after three steps, through torch.save / torch.load.
    (1) Load before the first step (the reference's resume_or_load order: trainer first, checkpoint afterwards): the trainer
    with fc1 / fc2's update fused into their weight-gradient kernels against WSOVOD_FUSED_SGD=0 -- the fused update must follow
    the LIVE param groups (load_state_dict replaces the group dicts; the scheduler moves the new ones).
    (2) Load into a trainer that has already run (and, with step graphs, captured and replayed) five steps of its own: its
    pending update and its graphs belong to the weights and momentum buffers before the load -- it must continue as (1)."""
    model, tr = _trainer(monkeypatch, precision, True, graph)
    _run(tr, _batches(gpu, CKPT_STEPS, 900), 0)
    buf = io.BytesIO()
    torch.save((model.state_dict(), tr.optimizer.state_dict()), buf)  # (state-dict pre-hooks apply the pending update)
    ckpt = buf.getvalue()
    tr.close()
    del model, tr
    after = _batches(gpu, 5, 950)  # eager, eager, capture, replay, replay (graph)

    runs = {}
    for fused in (True, False):
        model, tr = _trainer(monkeypatch, precision, fused, graph)
        _load(model, tr, ckpt, CKPT_STEPS)
        runs[fused] = _result(model, tr, _run(tr, after, CKPT_STEPS))
        del model, tr
    assert runs[True]["calls"] > 0 and (runs[True]["graphs"] == 1) == graph
    _assert_same(runs[True], runs[False], "fused vs two-kernel step after a load")

    model, tr = _trainer(monkeypatch, precision, True, graph)
    _run(tr, _batches(gpu, 5, 700), 0)  # (its own history: the update of the last step still pending)
    assert (len(tr._graphs) == 1) == graph
    _load(model, tr, ckpt, CKPT_STEPS)
    late = _result(model, tr, _run(tr, after, CKPT_STEPS))
    _assert_same(late, runs[True], "load after own steps vs fresh load")
