"""-m gpu: the range guard of the f16mx operands (MODEL.HIP.MX_RANGE_GUARD).  The audit kernel (wsovod_f16mx_range) against
torch on the carrier's own bytes, counters EXACTLY equal; then the guard on the model at 2 images with the f16mx kernels forced
on: silent and bit-neutral on the synthetic model, a trip by a scaled FrozenBN (saturated cross terms, then a non-finite hi)
under every mode in inference and training, and the trainer's arming schedule next to its captured step graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PLANTED = [0.0, -0.0, 416.0, -416.0, 431.9, -431.9, 432.0, -432.0, 448.0, -448.0, 1e3, -1e3, 65504.0, -65504.0, 65520.0,
           -65520.0, 1e5, -1e5, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 3e-6, -3e-6, 2.0 ** -10]


def _expect(car2d):
    """[values, non-finite hi, q at the top code, largest finite |hi| as fp16 bits] of a 2-D f16mx carrier view, from its bytes."""
    rows, cols = car2d.shape
    if rows == 0:
        return [0, 0, 0, 0]
    raw = car2d.contiguous().view(torch.uint8).view(rows, cols // 32, 128).cpu()
    hi = raw[:, :, :64].contiguous().view(torch.float16)
    fin = torch.isfinite(hi)
    q = raw[:, :, 64:96].contiguous().to(torch.int32)
    bits = hi.view(torch.int16).to(torch.int32) & 0x7FFF
    return [rows * cols, int((~fin).sum()), int(((q & 0x7F) >= 0x7E).sum()), int(bits[fin].max()) if bool(fin.any()) else 0]


def _planted(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.logspace(-3, 2.5, max(cols, 1))[None]
    flat = x.view(-1)
    n = flat.numel()
    if n:
        vals = torch.tensor(PLANTED)
        pos = torch.arange(0, n, 2) if n <= 64 else torch.randperm(n, generator=g)[: max(n // 5, len(PLANTED))]
        flat[pos] = vals[torch.arange(pos.numel()) % len(PLANTED)]
    return x


def _counters(gpu):
    return torch.zeros(4, dtype=torch.int64, device=gpu)


@pytest.mark.parametrize("shape", [(1, 32), (3, 96), (257, 32), (300, 4096), (0, 64)], ids=str)
def test_audit_kernel_equals_torch_on_the_carriers_bytes(gpu, shape):
    """Unit-scale carriers of fp32 matrices planted with the values around every threshold (416 .. 448, the fp16 limit, inf,
    NaN, denormals, signed zeros); (3, 96) is a column block of a wider carrier (ld > cols).  Two calls on one counter row add
    up (the maximum stays)."""
    from wsovod_amd.layers import carrier
    from wsovod_amd.layers import hip_ops as H

    rows, cols = shape
    if shape == (3, 96):
        wide, _ = H.mx_encode(_planted(rows, 160, 5).to(gpu), unit=True)
        car = carrier.like(wide, wide[:, 32:128])
        assert car.stride(0) == 160 and not car.is_contiguous()
    else:
        car, _ = H.mx_encode(_planted(rows, cols, rows + cols).to(gpu), unit=True)
    want = _expect(car)
    if rows:
        assert want[1] > 0 and want[2] > 0 and want[3] > 0, want  # (the planted values did land in every counter)
    c = _counters(gpu)
    assert H.mx_range(car, c) is c
    got = c.cpu().tolist()
    print(f"{shape}: kernel {got} torch {want}")
    assert got == want
    H.mx_range(car, c)
    assert c.cpu().tolist() == [2 * want[0], 2 * want[1], 2 * want[2], want[3]]


def test_maximum_is_kept_across_calls_and_sees_the_largest_finite_half(gpu):
    from wsovod_amd.layers import hip_ops as H

    c = _counters(gpu)
    small = torch.full((5, 64), 3.0)
    big = torch.full((5, 64), 7.0)
    big[4, 63] = -65504.0  # the last value of the last row: the largest finite half
    big[0, 0] = float("inf")
    for x in (big, small):
        car, _ = H.mx_encode(x.to(gpu), unit=True)
        H.mx_range(car, c)
    assert c.cpu().tolist() == [640, 1, 2, 0x7BFF]  # (q: inf and -65504 are clamped to the top code)


def test_scaled_weight_operand_with_too_small_a_scale_byte(gpu):
    """A weight operand encoded with ONE scale byte three binades too small: the q plane saturates, the audit counts exactly
    the bytes torch counts, hi (unscaled) stays finite; the operand carrier is taken explicitly, never by a tag."""
    from wsovod_amd.layers import hip_ops as H

    g = torch.Generator().manual_seed(3)
    w = (torch.rand(96, 256, generator=g) * 2 - 1).to(gpu)  # |w| < 1: the fitting scale is 2^-7 (256 > 128 |w|)
    fit = torch.tensor([127 - 7], dtype=torch.uint8, device=gpu)
    small = torch.tensor([127 - 10], dtype=torch.uint8, device=gpu)
    for byte, saturates in ((fit, False), (small, True)):
        car, scales = H.mx_encode(w, tensor_byte=byte)
        assert H.carrier.fmt_of(car) is None
        with pytest.raises(RuntimeError, match="f16mx"):
            H.mx_range(car, _counters(gpu))
        c = _counters(gpu)
        H.mx_range(car, c, operand=True)
        want = _expect(car)
        model = int((w.abs() * 2.0 ** 10 >= 432).sum()) if saturates else 0
        print(f"byte {int(byte)}: kernel {c.cpu().tolist()} torch {want}; |w| 2^10 >= 432: {model}")
        assert c.cpu().tolist() == want and want[1] == 0 and (want[2] > 0) == saturates
        assert want[2] == model  # (e4m3 rounds |w| 2^10 to 448 from the midpoint 432 up, ties to the even code, and clamps beyond)


def test_untagged_and_wrongly_tagged_tensors_are_refused(gpu):
    from wsovod_amd.layers import hip_ops as H

    c = _counters(gpu)
    with pytest.raises(RuntimeError, match="f16mx"):
        H.mx_range(torch.zeros(4, 32, device=gpu), c)
    with pytest.raises(RuntimeError, match="f16mx"):
        H.mx_range(H.x2_encode(torch.zeros(4, 32, device=gpu)), c)
    car, _ = H.mx_encode(torch.zeros(4, 32, device=gpu), unit=True)
    with pytest.raises(RuntimeError, match="counters"):
        H.mx_range(car, torch.zeros(4, dtype=torch.int32, device=gpu))
    assert c.cpu().tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the guard on the model
# ---------------------------------------------------------------------------------------------------------------------
def _lower_mx_thresholds(monkeypatch):
    from wsovod_amd.modeling.backbone import ResNet
    from wsovod_amd.modeling.roi_heads import WSOVODROIHeads

    monkeypatch.setattr(ResNet, "MX_MIN_TILES", 1)
    monkeypatch.setattr(WSOVODROIHeads, "MX_MIN_ROWS", 1)


def _build(precision, guard="off", period=100, bn_scale=None):
    """build_hot_path_model with the guard keys set; bn_scale: the factor on the FrozenBN weight / bias of res4's last conv."""
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(precision=precision, device="cuda:0")
    cfg.MODEL.HIP.MX_RANGE_GUARD = guard
    cfg.MODEL.HIP.MX_RANGE_GUARD_PERIOD = period
    torch.manual_seed(0)
    model = build_model(cfg)
    with torch.no_grad():
        model.backbone.stem.conv1.norm.weight.fill_(1.0 / 64.0)
        if bn_scale is not None:
            norm = _res4_last_conv(model).norm
            norm.weight.mul_(bn_scale)
            norm.bias.mul_(bn_scale)
    return cfg, model


def _res4_last_conv(model):
    bb = model.backbone
    stage = bb.stages[bb.stage_names.index("res4")]
    return list(stage.children())[-1].conv2


def _res4_site(model):
    return {id(m): n for n, m in model.named_modules()}[id(_res4_last_conv(model))]


def _batch(gpu, seed=11):
    from wsovod_amd.data import make_batch

    return [{"image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu), "instances": x["instances"],
             "height": x["height"], "width": x["width"]} for x in make_batch(2, 64, 20, H=160, W=224, seed=seed)]


def _tensors(o):
    if torch.is_tensor(o):
        return [o]
    if isinstance(o, (list, tuple)):
        return [t for v in o for t in _tensors(v)]
    return []


def _infer(model, batch):
    """Everything inference returns, as a flat list of host tensors: the detections, every refinement's scores, the boxes."""
    model.eval()
    res, scores, boxes = model.inference(batch, do_postprocess=False)
    out = [t for r in res for t in (r.pred_boxes.tensor, r.scores, r.pred_classes)] + _tensors(scores) + _tensors(boxes)
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in out]


def _same_bytes(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(
        x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def _count(monkeypatch, name):
    from wsovod_amd.layers import hip_ops as H

    calls, orig = [0], getattr(H, name)

    def counted(*a, **k):
        calls[0] += 1
        return orig(*a, **k)

    monkeypatch.setattr(H, name, counted)
    return calls


@pytest.fixture(scope="module")
def unscaled(gpu):
    """The synthetic model's reported maximum at res4's last conv under the guard (shared: the scaled cases derive their
    factors from it), with everything the silent run recorded."""
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.layers.mx_guard import MxRangeGuard
    from wsovod_amd.modeling.backbone import ResNet
    from wsovod_amd.modeling.roi_heads import WSOVODROIHeads

    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(ResNet, "MX_MIN_TILES", 1)
        mp.setattr(WSOVODROIHeads, "MX_MIN_ROWS", 1)
        seen, orig = {}, MxRangeGuard.audit

        def recording(self, site, tensor, operand=False):
            if self.armed():
                name = site if isinstance(site, str) else self.names[id(site)]
                seen.setdefault(name, []).append(tensor.detach().clone())
            return orig(self, site, tensor, operand=operand)

        mp.setattr(MxRangeGuard, "audit", recording)
        batch = _batch(gpu)
        _, model = _build("parity_mx", "raise")
        out = _infer(model, batch)
        report = dict(model.mx_guard.last)
        site = _res4_site(model)
        decoded = {n: (sum(t.numel() for t in ts), max(float(_finite_max(H.mx_decode(_rows_of_groups(t))[0])) for t in ts)) for n, ts in seen.items()}
        _, off = _build("parity_mx", "off")
        out_off = _infer(off, batch)
    finally:
        mp.undo()
    return {"report": report, "site": site, "decoded": decoded, "out": out, "out_off": out_off, "polls": model.mx_guard.polls}


def _rows_of_groups(t):
    """(the pooled tensor's groups of 32 run along its flattened rows)"""
    return t if t.shape[-1] % 32 == 0 else t.reshape(t.shape[0], -1)


def _finite_max(hi):
    a = hi.abs()
    a = a[torch.isfinite(a)]
    return a.max() if a.numel() else torch.zeros(())


def test_synthetic_model_does_not_trip_and_the_guard_changes_no_bit(unscaled):
    """(a) guard "raise" on the unscaled synthetic model: no trip; every site audited once with its element count, its
    reported maximum the decoded carrier's; inference returns the bytes of guard "off"."""
    rep, dec = unscaled["report"], unscaled["decoded"]
    for n, r in rep.items():
        print(n, r)
    assert unscaled["polls"] == 1 and set(rep) == set(dec) and len(rep) >= 6
    for want in ("backbone.mx_from_x2", "roi_heads.pooled", "roi_heads.box_head.fc1", unscaled["site"]):
        assert want in rep, (want, list(rep))
    assert "roi_heads.box_head.fc2" not in rep  # (the last FC layer hands bf16x2 to the heads)
    for n, r in rep.items():
        assert r.nonfinite == 0 and r.top_code == 0 and r.audited == dec[n][0] > 0 and r.max_abs == dec[n][1], (n, r, dec[n])
        assert r.max_abs > 0
    assert _same_bytes(unscaled["out"], unscaled["out_off"])


def test_guard_off_launches_no_audit(gpu, monkeypatch):
    """(b) with the default "off", inference and a training step never reach hip_ops.mx_range (the f16mx kernels do run)."""
    from wsovod_amd.engine import build_optimizer
    from wsovod_amd.engine.trainer import run_step

    _lower_mx_thresholds(monkeypatch)
    audits, gemms = _count(monkeypatch, "mx_range"), _count(monkeypatch, "gemm_mx")
    cfg, model = _build("parity_mx")
    assert model.mx_guard is None
    _infer(model, _batch(gpu))
    model.train()
    run_step(model, build_optimizer(cfg, model), _batch(gpu, seed=12))
    torch.cuda.synchronize()
    assert gemms[0] > 0 and audits[0] == 0


def _factor(unscaled, target):
    m0 = unscaled["report"][unscaled["site"]].max_abs
    return target / m0


def test_saturated_cross_terms_trip_every_mode(gpu, monkeypatch, unscaled):
    """(c) the FrozenBN weight / bias of res4's last conv scaled so that its map passes 448 (asserted on the guard's own
    report): "raise" raises naming that site, "warn" returns the bytes of "off", "fallback" returns the bytes of the same
    model built with PRECISION = "parity" and stays fallen back."""
    from wsovod_amd.layers.mx_guard import MxRangeError

    _lower_mx_thresholds(monkeypatch)
    f = _factor(unscaled, 8192.0)
    batch, site = _batch(gpu), unscaled["site"]
    _, warn = _build("parity_mx", "warn", bn_scale=f)
    out_warn = _infer(warn, batch)
    r = warn.mx_guard.last[site]
    print(f"factor {f:.4g}: {site} {r}")
    assert r.max_abs > 448 and r.top_code > 0 and not warn.mx_guard.fallen_back
    first = [n for n, v in warn.mx_guard.last.items() if v.nonfinite or v.top_code][0]
    assert first == site  # (nothing upstream of the scaled conv trips)
    _, off = _build("parity_mx", "off", bn_scale=f)
    assert _same_bytes(out_warn, _infer(off, batch))
    _, rz = _build("parity_mx", "raise", bn_scale=f)
    with pytest.raises(MxRangeError) as e:
        _infer(rz, batch)
    assert e.value.site == site and e.value.report[site].top_code == r.top_code and site in str(e.value)
    _, parity = _build("parity", bn_scale=f)
    out_parity = _infer(parity, batch)
    _, fb = _build("parity_mx", "fallback", bn_scale=f)
    gemms = _count(monkeypatch, "gemm_mx")
    out_fb = _infer(fb, batch)
    assert gemms[0] > 0 and fb.mx_guard.fallen_back and not fb.mx_on
    assert _same_bytes(out_fb, out_parity)
    assert not _same_bytes(out_fb, out_warn)  # (the f16mx result of this batch was discarded, not returned)
    n, polls = gemms[0], fb.mx_guard.polls
    assert _same_bytes(_infer(fb, batch), out_parity) and gemms[0] == n and fb.mx_guard.polls == polls  # sticky: straight to bf16x2


def test_nonfinite_hi_trips_inference_and_raises_in_training(gpu, monkeypatch, unscaled):
    """(d) scaled past 65504: the non-finite count is reported, "fallback" inference still equals "parity", and a training
    step raises under "warn", "raise" and "fallback" alike (its update is already applied)."""
    from wsovod_amd.engine import build_optimizer
    from wsovod_amd.engine.trainer import run_step
    from wsovod_amd.layers.mx_guard import MxRangeError

    _lower_mx_thresholds(monkeypatch)
    f = _factor(unscaled, 2.0 ** 22)
    batch, site = _batch(gpu), unscaled["site"]
    _, warn = _build("parity_mx", "warn", bn_scale=f)
    _infer(warn, batch)
    r = warn.mx_guard.last[site]
    print(f"factor {f:.4g}: {site} {r}")
    assert r.nonfinite > 0
    _, parity = _build("parity", bn_scale=f)
    _, fb = _build("parity_mx", "fallback", bn_scale=f)
    assert _same_bytes(_infer(fb, batch), _infer(parity, batch)) and fb.mx_guard.fallen_back
    for mode in ("warn", "raise", "fallback"):
        cfg, model = _build("parity_mx", mode, bn_scale=f)
        model.train()
        with pytest.raises(MxRangeError, match="non-finite") as e:
            run_step(model, build_optimizer(cfg, model), _batch(gpu, seed=12))
        assert e.value.site == site and e.value.report[site].nonfinite > 0, mode
        assert not model.mx_guard.armed()


def _count_graph_steps(monkeypatch):
    """-> [(graph object, replayed)]: every _StepGraph.step call from now on (replayed: it did run the step)."""
    from wsovod_amd.engine.trainer import _StepGraph

    calls, orig = [], _StepGraph.step

    def counted(self, batched_inputs):
        out = orig(self, batched_inputs)
        calls.append((self, out is not None))
        return out

    monkeypatch.setattr(_StepGraph, "step", counted)
    return calls


def _trainer_run(gpu, monkeypatch, guard, n_steps=6):
    from wsovod_amd.engine import HotPathTrainer, build_optimizer
    from wsovod_amd.layers import hip_ops as H

    graph_steps = _count_graph_steps(monkeypatch)

    monkeypatch.setattr(H, "DETERMINISTIC", True)
    monkeypatch.setenv("WSOVOD_BACKBONE_GRAPH", "0")
    monkeypatch.setenv("WSOVOD_STEP_GRAPH", "1")
    _lower_mx_thresholds(monkeypatch)
    cfg, model = _build("parity_mx", guard, period=3)
    model.train()
    cfg.SOLVER.BASE_LR = 1e-3
    tr = HotPathTrainer(model, build_optimizer(cfg, model))
    armed = []
    g = model.mx_guard
    if g is not None:
        orig = g.begin_step

        def begin():
            armed.append(orig())
            return armed[-1]

        g.begin_step = begin
    losses, per_step = [], []
    for s in range(n_steps):
        out = tr.run_step(_batch(gpu, seed=700 + s))
        losses.append({k: float(v) for k, v in out.items()})
        per_step.append((sum(1 for _, ran in graph_steps if ran), dict(g.totals) if g is not None else None,
                         g.polls if g is not None else 0,
                         g.table.cpu().clone() if g is not None and g.table is not None else None))
    tr.flush()
    params = {k: v.detach().clone() for k, v in model.named_parameters() if v.requires_grad}
    graphs = [bool(v) for v in tr._graphs.values()]
    tr.close()
    return {"losses": losses, "params": params, "armed": armed, "per_step": per_step, "graphs": graphs,
            "last": dict(g.last) if g is not None else None}


def test_trainer_arms_every_period_next_to_its_step_graph(gpu, monkeypatch):
    """(e) HotPathTrainer, period 3, six steps of one layout with step graphs enabled: steps 0 and 3 are audited and run on
    eager launches, the layout is still captured and replayed by the others; losses and trained parameters equal the
    guard-"off" run to the graph-vs-eager tolerance of tests/test_gpu_graph.py; every site's audited count advanced exactly
    twice, the trained weights' operands among them."""
    off = _trainer_run(gpu, monkeypatch, "off")
    on = _trainer_run(gpu, monkeypatch, "raise")
    assert on["armed"] == [True, False, False, True, False, False]
    assert off["graphs"] == [True] and on["graphs"] == [True]  # the layout's whole-step graph was captured in both runs
    polls = [p[2] for p in on["per_step"]]
    assert polls == [1, 1, 1, 2, 2, 2]
    # steps served by the captured graph, cumulative (a layout is captured at its third unaudited sighting): the audited steps
    # 0 and 3 never went through it, the steps after the capture all did
    assert [p[0] for p in off["per_step"]] == [0, 0, 1, 2, 3, 4]
    assert [p[0] for p in on["per_step"]] == [0, 0, 0, 0, 1, 2]
    # the DEVICE table moves in audited steps only: no audit kernel was captured into the graph or launched unarmed
    tables = [p[3] for p in on["per_step"]]
    assert int(tables[0][:, 0].sum()) > 0
    assert torch.equal(tables[1], tables[0]) and torch.equal(tables[2], tables[0])
    assert torch.equal(tables[4], tables[3]) and torch.equal(tables[5], tables[3])
    assert torch.equal(tables[3][:, 0], tables[0][:, 0])  # (cleared when armed: one step's counts, not two)
    first, second = on["per_step"][0][1], on["per_step"][5][1]
    assert first and set(first) == set(second)
    for want in ("backbone.mx_from_x2", "roi_heads.pooled", "roi_heads.box_head.fc1", "weight:roi_heads.box_head.fc1.weight",
                 "weight:roi_heads.box_head.fc2.weight"):
        assert want in first, (want, list(first))
    for n, v in first.items():
        assert v > 0 and on["per_step"][2][1][n] == v and second[n] == 2 * v, n
    assert all(r.nonfinite == 0 and r.top_code == 0 for r in on["last"].values())
    for s, (e, g) in enumerate(zip(off["losses"], on["losses"])):
        for k in e:
            print(f"step {s} {k}: off {e[k]!r} guard {g[k]!r}")
            assert abs(e[k] - g[k]) <= 2e-5 * max(abs(e[k]), 1e-3), (s, k, e[k], g[k])
    for k, v in off["params"].items():
        torch.testing.assert_close(on["params"][k], v, rtol=1e-5, atol=2e-6 * float(v.abs().max()) + 1e-9, msg=lambda m: f"{k}: {m}")


def test_fallback_tripped_in_inference_drops_the_trainers_captured_graphs(gpu, monkeypatch, unscaled):
    """A layout is captured and replayed under guard "fallback"; then an eval call between steps (the trainer's supported
    use) meets saturating activations and falls back.  The next training step must not replay the graph that captured the
    f16mx kernels: that graph object is never stepped again and is gone from the trainer, and no f16mx contraction is
    launched by the step (or by the capture that replaces the graph)."""
    from wsovod_amd.engine import HotPathTrainer, build_optimizer
    from wsovod_amd.layers import hip_ops as H

    monkeypatch.setattr(H, "DETERMINISTIC", True)
    monkeypatch.setenv("WSOVOD_BACKBONE_GRAPH", "0")
    monkeypatch.setenv("WSOVOD_STEP_GRAPH", "1")
    _lower_mx_thresholds(monkeypatch)
    graph_steps = _count_graph_steps(monkeypatch)
    cfg, model = _build("parity_mx", "fallback", period=100)
    model.train()
    cfg.SOLVER.BASE_LR = 1e-3
    tr = HotPathTrainer(model, build_optimizer(cfg, model))
    for s in range(5):  # 0 audited, 1 - 2 eager, 3 captured, 4 replayed
        tr.run_step(_batch(gpu, seed=700 + s))
    old = [g for g in tr._graphs.values() if g]
    assert len(old) == 1 and [ran for _, ran in graph_steps] == [True, True] and not model.mx_guard.fallen_back
    with torch.no_grad():  # the checkpoint's magnitudes grow: res4's last map passes 448
        norm = _res4_last_conv(model).norm
        f = _factor(unscaled, 8192.0)
        norm.weight.mul_(f)
        norm.bias.mul_(f)
        _res4_last_conv(model).weight.mul_(1.0)  # (the folded weight is cached by the conv weight's version, as a load moves it)
    _infer(model, _batch(gpu))
    assert model.mx_guard.fallen_back and not model.mx_on
    assert model.mx_guard.last[unscaled["site"]].max_abs > 448
    model.train()
    n = len(graph_steps)
    gemms = _count(monkeypatch, "gemm_mx")
    tr.run_step(_batch(gpu, seed=705))
    tr.flush()
    torch.cuda.synchronize()
    assert gemms[0] == 0
    assert all(g is not old[0] for g in tr._graphs.values()) and all(g is not old[0] for g, _ in graph_steps[n:])
    # the layout starts over on the bf16x2 kernels: eager sightings first, then ONE new capture that replays
    for s in range(6, 10):
        tr.run_step(_batch(gpu, seed=700 + s))
    new = [g for g in tr._graphs.values()]
    assert gemms[0] == 0 and len(new) == 1 and bool(new[0]) and new[0] is not old[0]
    # (steps 5 and 6 are the eager sightings, step 7 captures, 8 and 9 replay)
    assert [g is new[0] and ran for g, ran in graph_steps[n:]] == [True, True, True]
    tr.close()
