"""-m gpu: MODEL.HIP.PRECISION = "parity_mx_train" -- the "parity_mx" forward (f16mx kernels) with a backward whose
input-gradient contractions keep the hi/lo split (layers/functions.py:_Linear).  Kernel by kernel (the masked gradient written
as bf16x2, the transposed bf16x2 weight, the f16mx decoder, the dX contraction built of them), then the mode as a whole: the
five-step trajectory against the oracle's at the north star's 1e-3, the forward's identity with "parity_mx", fc1's fused
update, the whole-step graph."""
import pytest
import torch

from tests.util import bits, odd_view, outside_intact, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _lower_mx_thresholds(monkeypatch):
    """Two small images are below the mode's tile / row thresholds: lowered, so that the f16mx kernels run."""
    from wsovod_amd.modeling.backbone import ResNet
    from wsovod_amd.modeling.roi_heads import WSOVODROIHeads

    monkeypatch.setattr(ResNet, "MX_MIN_TILES", 1)
    monkeypatch.setattr(WSOVODROIHeads, "MX_MIN_ROWS", 1)


def _count_gemm_mx(monkeypatch):
    """-> [n]: the number of hip_ops.gemm_mx calls from now on (the f16mx kernels ran: no pass on the bf16x2 hand-over)."""
    from wsovod_amd.layers import hip_ops as H

    calls, orig = [0], H.gemm_mx

    def counted(*a, **k):
        calls[0] += 1
        return orig(*a, **k)

    monkeypatch.setattr(H, "gemm_mx", counted)
    return calls


def _to_dev(host, gpu):
    return [{"image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu), "instances": x["instances"],
             "height": x["height"], "width": x["width"]} for x in host]


def _x2_planes(t, rows, cols):
    """(hi, lo) bf16 matrices (rows, cols) of an interleaved bf16x2 carrier with cols a multiple of 32 (host tensors)."""
    raw = t.contiguous().view(BF).view(rows, cols // 32, 2, 32).cpu()
    return raw[:, :, 0, :].reshape(rows, cols), raw[:, :, 1, :].reshape(rows, cols)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the mode: five optimizer steps against the oracle's trajectory
# ---------------------------------------------------------------------------------------------------------------------
def test_five_step_trajectory_stays_within_1e_3_of_the_oracles(gpu, monkeypatch):
    """The five-step harness of tests/test_gpu_full_size.py (2 x 800x600 x 512 proposals per step, the reference's warm-up
    learning rates, HotPathTrainer + HipSGD against the oracle's five SGD steps) under "parity_mx_train" with the f16mx
    kernels forced on: labels and pseudo-GT of every step exact, every loss within 1e-3 relative, and after the five updates
    the MIL-head logits within the north star's 1e-3 -- the gate "parity_train" gets, which "parity_mx" (plain bf16 backward,
    6.8e-3) is not held to.  The harness applies the 1e-3 logit gate to every precision name but "parity" / "parity_mx".
    MEASURED on an MI355X: 5.1e-4 on the default bf16x2 dX route, 5.4e-4 with WSOVOD_PT_DX=x3 ("parity_train": 4.0e-4)."""
    from tests import test_gpu_full_size as FS

    _lower_mx_thresholds(monkeypatch)
    calls = _count_gemm_mx(monkeypatch)
    FS.test_five_step_training_trajectory_stays_on_the_oracles(gpu, "parity_mx_train", monkeypatch)
    assert calls[0] > 0, "the f16mx kernels did not run"


def _trainer_steps(gpu, monkeypatch, precision, n_steps=1, graph=False):
    from wsovod_amd.data import make_batch
    from wsovod_amd.engine import HotPathTrainer, build_optimizer
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.layers import operand_cache
    from wsovod_amd.testing import build_hot_path_model

    monkeypatch.setattr(H, "DETERMINISTIC", True)
    monkeypatch.setenv("WSOVOD_BACKBONE_GRAPH", "0")
    monkeypatch.setenv("WSOVOD_STEP_GRAPH", "1" if graph else "0")
    _lower_mx_thresholds(monkeypatch)
    cfg, model = build_hot_path_model(seed=0, precision=precision, device="cuda:0")
    model.train()
    cfg.SOLVER.BASE_LR = 1e-3
    tr = HotPathTrainer(model, build_optimizer(cfg, model))
    hist = []
    for s in range(n_steps):
        b = _to_dev(make_batch(2, 64, 20, H=160, W=224, seed=700 + s), gpu)
        losses = tr.run_step(b)
        pgt = model.roi_heads._last_pgt
        t = int(sum(len(torch.unique(x["instances"].gt_classes)) for x in b))  # (a step graph pads the pseudo-GT arrays)
        hist.append(({k: v.detach().clone() for k, v in losses.items()}, pgt["gt_classes"][:128].clone(),
                     torch.stack([pgt["pgt_index"][:t], pgt["pgt_classes"][:t]]).clone()))
    tr.flush()
    bh = model.roi_heads.box_head
    out = {"hist": hist, "fc1_grad": bh.fc1.weight.grad, "fused_calls": [p._fused_update.calls for p in tr._fused],
           "graphs": len(tr._graphs), "params": {k: v.detach().clone() for k, v in model.named_parameters() if v.requires_grad},
           "x2t_fc2": operand_cache.current(bh.fc2.weight, "x2t")}
    tr.close()
    return out


def test_first_step_is_parity_mx_forward_and_fc1_keeps_its_fused_update(gpu, monkeypatch):
    """One trainer step from the same weights on the same batch under "parity_mx" and "parity_mx_train".  The forward is the
    same kernels on the same inputs: the step's losses, labels and pseudo-GT are equal bit for bit, with the same number of
    f16mx launches.  fc1 has no split contraction to run (the pooled tensor takes no gradient under a frozen backbone): it
    keeps the ordinary backward, so its gradient never reaches memory (`grad is None`: the fused dW + optimizer kernel ran,
    once, as under "parity_mx"), and fc2's does not either (the bf16x2 dX route replaces ONE contraction of the ordinary
    backward).  The updated fc1 WEIGHT is not "parity_mx"'s on the model: its kernels are, but its incoming gradient is
    fc2's dX, the one quantity the mode computes differently.  "Same kernels, same inputs -> the same updated weight" is
    pinned on the layer, through the fused dW + optimizer kernel and with one upstream gradient for both modes, by
    test_fused_update_of_a_layer_is_the_parity_mx_one below."""
    calls = _count_gemm_mx(monkeypatch)
    a = _trainer_steps(gpu, monkeypatch, "parity_mx")
    n_mx = calls[0]
    b = _trainer_steps(gpu, monkeypatch, "parity_mx_train")
    assert n_mx > 0 and calls[0] == 2 * n_mx  # the same f16mx launches, no bf16x2 hand-over
    for k, v in a["hist"][0][0].items():
        assert torch.equal(b["hist"][0][0][k], v), (k, float(v), float(b["hist"][0][0][k]))
    assert torch.equal(a["hist"][0][1], b["hist"][0][1]) and torch.equal(a["hist"][0][2], b["hist"][0][2])
    assert a["fc1_grad"] is None and b["fc1_grad"] is None
    assert a["fused_calls"] == [1, 1] and b["fused_calls"] == [1, 1]  # fc1 AND fc2
    assert b["x2t_fc2"] is None  # (the transposed operand was encoded from the weights before the update: dropped with it)


def test_forward_logits_equal_parity_mx_bit_for_bit(gpu, monkeypatch):
    """Forward identity on the model: losses, mining scores and refinement logits of a training forward under
    "parity_mx_train" are torch.equal to "parity_mx"'s on the same weights and batch (the f16mx kernels counted)."""
    from wsovod_amd.data import make_batch
    from wsovod_amd.testing import build_hot_path_model, capture_step

    _lower_mx_thresholds(monkeypatch)
    calls = _count_gemm_mx(monkeypatch)
    batch = _to_dev(make_batch(2, 64, 20, H=160, W=224, seed=11), gpu)
    got = {}
    for precision in ("parity_mx", "parity_mx_train"):
        cfg, model = build_hot_path_model(seed=0, precision=precision, device="cuda:0")
        model.train()
        got[precision] = capture_step(model, batch)
        del model
    assert calls[0] > 0 and calls[0] % 2 == 0
    (la, ma, ra), (lb, mb, rb) = got["parity_mx"], got["parity_mx_train"]
    for k in la:
        assert torch.equal(la[k], lb[k]), k
    assert torch.equal(ma, mb) and torch.equal(ra, rb)


def test_whole_step_graph_replays_equal_the_eager_steps(gpu, monkeypatch):
    """HotPathTrainer under "parity_mx_train", dropout on, six steps of one layout: the whole-step HIP graph (captured on the
    third step, replayed three times) against WSOVOD_STEP_GRAPH=0 with the unsplit (fixed-order) weight-gradient tiles --
    labels, pseudo-GT, losses and every trained tensor equal bit for bit.  The transposed bf16x2 operand of fc2 is encoded
    INSIDE the graph from the weights before the update: after a replay it is not offered as current."""
    e = _trainer_steps(gpu, monkeypatch, "parity_mx_train", n_steps=6, graph=False)
    g = _trainer_steps(gpu, monkeypatch, "parity_mx_train", n_steps=6, graph=True)
    assert e["graphs"] == 0 and g["graphs"] == 1 and g["x2t_fc2"] is None
    for s, (he, hg) in enumerate(zip(e["hist"], g["hist"])):
        assert torch.equal(he[1], hg[1]) and torch.equal(he[2], hg[2]), s
        for k in he[0]:
            print(f"step {s} {k}: eager {float(he[0][k])!r} graph {float(hg[0][k])!r}")
    for k, v in e["params"].items():
        print(f"{k}: max |eager - graph| {float((g['params'][k] - v).abs().max()):.3e}")
    for s, (he, hg) in enumerate(zip(e["hist"], g["hist"])):
        for k in he[0]:
            assert torch.equal(he[0][k], hg[0][k]), (s, k, float(he[0][k]), float(hg[0][k]))
    for k, v in e["params"].items():
        assert torch.equal(g["params"][k], v), k


def test_trainable_backbone_stage_is_refused_with_the_reason(gpu):
    """Out of the mode's scope: a trainable residual stage.  The step raises and says why."""
    from wsovod_amd.data import make_batch
    from wsovod_amd.testing import build_hot_path_model

    cfg, model = build_hot_path_model(seed=0, precision="parity_mx_train", device="cuda:0", freeze_at=4)
    model.train()
    with pytest.raises(NotImplementedError, match="frozen backbone"):
        model(_to_dev(make_batch(1, 16, 20, H=160, W=224, seed=1), gpu))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the layer: _Linear with an f16mx input under a backward split
# ---------------------------------------------------------------------------------------------------------------------
def _mx_linear_case(gpu, M, K, N, seed, out_fmt):
    """An FC layer of the f16mx chain on its own: x as the previous producer leaves it (unit-scale f16mx + its plain bf16
    rounding), an fp32 master weight and bias, an upstream gradient.  -> (x32, x carrier factory, w, b, dy)."""
    from wsovod_amd.layers import carrier
    from wsovod_amd.layers import hip_ops as H

    g = _gen(seed)
    x32 = torch.randn(M, K, generator=g).to(gpu)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(gpu)
    b = (torch.randn(N, generator=g) * 0.1).to(gpu)
    dy = torch.randn(M, N, generator=g).to(gpu)

    def make_x(requires_grad):
        x, _ = H.mx_encode(x32, unit=True)
        carrier.tag(x, H.MX, H.mx_to_f32(x).to(BF))
        return x.requires_grad_(requires_grad)

    return x32, make_x, w, b, dy


def _run_linear(make_x, w, b, dy, out_fmt, *, split, x_grad, env, monkeypatch, dropout_p=0.0):
    from wsovod_amd.layers import functions as Fn
    from wsovod_amd.layers import hip_ops as H

    for k in ("WSOVOD_PT_SPLIT", "WSOVOD_PT_DX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wp = w.clone().requires_grad_(True)
    bp = b.clone().requires_grad_(True)
    x = make_x(x_grad)
    with H.x3_mode("x2"), H.mx_mode(True), Fn.backward_split(split):
        y = Fn.linear(x, wp, bp, relu=True, dropout_p=dropout_p, seed=1234, out_dtype=out_fmt)
    assert H.carrier.fmt_of(y) == out_fmt
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), x.grad, wp.grad, bp.grad


@pytest.mark.parametrize("out_fmt", ["f16mx", "bf16x2"], ids=["mask-from-bf16-copy", "mask-from-bf16x2-output"])
def test_linear_without_a_split_contraction_is_the_parity_mx_layer(gpu, monkeypatch, out_fmt):
    """fc1's case: an f16mx input that takes no gradient under WSOVOD_PT_SPLIT=dx.  The same kernels on the same inputs as
    without the backward split: output, dW and db equal bit for bit (and with an input gradient wanted, dW and db still are:
    only dX changes)."""
    x32, make_x, w, b, dy = _mx_linear_case(gpu, 320, 512, 256, 5, out_fmt)
    ya, _, dwa, dba = _run_linear(make_x, w, b, dy, out_fmt, split=False, x_grad=False, env={}, monkeypatch=monkeypatch)
    yb, dxb, dwb, dbb = _run_linear(make_x, w, b, dy, out_fmt, split=True, x_grad=False, env={}, monkeypatch=monkeypatch)
    assert dxb is None and same_bits(ya.cpu(), yb.cpu()) and torch.equal(dwa, dwb) and torch.equal(dba, dbb)
    _, dxp, dwp, dbp = _run_linear(make_x, w, b, dy, out_fmt, split=False, x_grad=True, env={}, monkeypatch=monkeypatch)
    for env in ({}, {"WSOVOD_PT_DX": "x3"}):
        _, dxs, dws, dbs = _run_linear(make_x, w, b, dy, out_fmt, split=True, x_grad=True, env=env, monkeypatch=monkeypatch)
        assert torch.equal(dws, dwa) and torch.equal(dwp, dwa), env
        torch.testing.assert_close(dbs, dba, rtol=0, atol=320 * U * float((dy.abs()).sum(0).max()))  # (summed from fp32 either way)
        # dX against the fp64 contraction of the masked gradient and the fp32 master: the split routes beat the plain one
        dA = torch.where(_decoded(ya, out_fmt) > 0, dy, torch.zeros_like(dy)).double()
        ref = dA @ w.double()
        es, ep = float((dxs.double() - ref).abs().max()), float((dxp.double() - ref).abs().max())
        print(f"{out_fmt} {env}: max |dX - fp64| split {es:.3e} plain bf16 {ep:.3e}")
        assert es < ep


@pytest.mark.parametrize("x_grad", [False, True], ids=["fc1-no-input-gradient", "fc2-input-gradient"])
@pytest.mark.parametrize("out_fmt", ["f16mx", "bf16x2"])
def test_fused_update_of_a_layer_is_the_parity_mx_one(gpu, monkeypatch, out_fmt, x_grad):
    """An FC layer of the f16mx chain with the trainer's fused dW + optimizer kernel on its weight (engine/trainer.py:
    _FusedUpdate, armed as inside the trainer's own backward), ONE upstream gradient, without and with the backward split.
    The same kernels on the same inputs: the fused kernel runs once either way, no gradient reaches memory, and the updated
    weight and its momentum are equal bit for bit -- for fc1 (no input gradient: the ordinary backward)
    and for fc2 (the bf16x2 dX route replaces one contraction; the weight gradient's operand is mask_x2's plain bf16 copy).
    The input gradient itself is taken from the weights BEFORE the update under both."""
    from wsovod_amd.engine.trainer import HipSGD, _FusedUpdate
    from wsovod_amd.layers import functions as Fn
    from wsovod_amd.layers import hip_ops as H

    monkeypatch.setattr(H, "DETERMINISTIC", True)
    for k in ("WSOVOD_PT_SPLIT", "WSOVOD_PT_DX"):
        monkeypatch.delenv(k, raising=False)
    x32, make_x, w, b, dy = _mx_linear_case(gpu, 320, 512, 256, 13, out_fmt)
    got = {}
    for split in (False, True):
        wp = torch.nn.Parameter(w.clone())
        bp = b.clone().requires_grad_(True)
        opt = HipSGD([{"params": [wp], "lr": 1e-2, "weight_decay": 1e-4}], 1e-2, momentum=0.9)
        wp._fused_update = fu = _FusedUpdate(opt, wp, 4096)
        x = make_x(x_grad)
        with H.x3_mode("x2"), H.mx_mode(True), Fn.backward_split(split):
            y = Fn.linear(x, wp, bp, relu=True, dropout_p=0.5, seed=99, out_dtype=out_fmt)
        fu.armed = True
        y.backward(dy)
        fu.armed = False
        torch.cuda.synchronize()
        assert fu.calls == 1 and wp.grad is None, split
        got[split] = (wp.detach().clone(), opt.state[wp]["momentum_buffer"].clone(), bp.grad.clone(), x.grad)
    assert not torch.equal(got[False][0], w)  # (a step was taken)
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    if x_grad:
        # (the bias gradient: the same fp32 values summed by mask_x2 instead of mask_transpose, 320 terms per column)
        torch.testing.assert_close(got[True][2], got[False][2], rtol=0, atol=320 * U * 2.0 * float(dy.abs().sum(0).max()))
        dA = torch.where(_decoded(y.detach(), out_fmt) > 0, dy * 2.0, torch.zeros_like(dy)).double()
        ref = dA @ w.double()  # the weights before the update
        es, ep = float((got[True][3].double() - ref).abs().max()), float((got[False][3].double() - ref).abs().max())
        assert es < ep, (es, ep)
    else:
        assert torch.equal(got[True][2], got[False][2]) and got[True][3] is None and got[False][3] is None


def _decoded(y, fmt):
    from wsovod_amd.layers import carrier
    from wsovod_amd.layers import hip_ops as H

    return H.mx_to_f32(y) if fmt == "f16mx" else H.x2_decode(carrier.tag(y.clone(), H.X2))


def test_split_weight_gradient_of_an_f16mx_input(gpu, monkeypatch):
    """WSOVOD_PT_SPLIT=dw,dx with an f16mx input: the saved carrier is decoded on the device (wsovod_f16mx_to_f32) and dW =
    dA^T X runs on the split operands -- finite, and within the "parity_train" gradient tolerance (5e-3 of the tensor's norm,
    tests/test_gpu_full_size.py) of the fp64 gradient; closer to it than the plain bf16 dW on the same inputs."""
    for out_fmt in ("f16mx", "bf16x2"):
        x32, make_x, w, b, dy = _mx_linear_case(gpu, 320, 512, 256, 7, out_fmt)
        env = {"WSOVOD_PT_SPLIT": "dw,dx"}
        y, dx, dw, db = _run_linear(make_x, w, b, dy, out_fmt, split=True, x_grad=True, env=env, monkeypatch=monkeypatch)
        _, _, dwp, _ = _run_linear(make_x, w, b, dy, out_fmt, split=False, x_grad=True, env={}, monkeypatch=monkeypatch)
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(db).all())
        from wsovod_amd.layers import hip_ops as H

        xv = H.mx_to_f32(make_x(False)).double()  # the values the forward contracted
        dA = torch.where(_decoded(y, out_fmt) > 0, dy, torch.zeros_like(dy)).double()
        ref = dA.t() @ xv
        rel = float((dw.double().norm() - ref.norm()).abs() / ref.norm())
        es, ep = float((dw.double() - ref).abs().max()), float((dwp.double() - ref).abs().max())
        print(f"{out_fmt}: dW norm error {rel:.3e}; max |dW - fp64| split {es:.3e} plain bf16 {ep:.3e}")
        assert rel < 5e-3 and es < ep


def test_split_weight_gradient_of_the_model_matches_the_oracle(gpu, monkeypatch):
    """The same on the model: WSOVOD_PT_SPLIT=dw,dx under "parity_mx_train" at the headline size (2 x 800x600 x 512
    proposals, f16mx kernels forced on) against the oracle's step -- every gradient finite and every gradient norm within
    the "parity_train" tolerance (grad_tol 5e-3, tests/test_gpu_full_size.py)."""
    from tests import test_gpu_full_size as FS

    _lower_mx_thresholds(monkeypatch)
    calls = _count_gemm_mx(monkeypatch)
    monkeypatch.setenv("WSOVOD_PT_SPLIT", "dw,dx")
    rep = FS._oracle_vs_hip(gpu, "parity_mx_train", n_images=2, proposals=512, classes=20)
    assert calls[0] > 0
    assert rep["max_rel_gradnorm_err"] == rep["max_rel_gradnorm_err"] and rep["max_rel_gradnorm_err"] < 5e-3, rep
    assert rep["max_abs_logit_err"] < 1e-3 and rep["labels_exact"] and rep["pgt_exact"], rep


# ---------------------------------------------------------------------------------------------------------------------
# 3. the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ykind", ["bf16", "x2", "f32", None])
def test_mask_x2_writes_the_masked_gradient_as_bf16x2(gpu, ykind):
    """wsovod_mask_bf16x2 against the torch composition: mask (y > 0 on the stored mask source: +-0, NaN and denormals
    included), scale, .bfloat16(), residual .bfloat16() -- hi and lo bit for bit, the padding columns zero, the plain bf16
    copy of hi equal to hi, nothing written outside; M not a multiple of 64, N not a multiple of 8 (32 for a bf16x2 y),
    unaligned dy / y rows.  Column sums: M fp32 terms per column in a fixed order, within M u of the sum of magnitudes (the
    bound of tests/test_gpu_elementwise.py::test_mask_transpose), ADDED to what colsum held, the same bits twice."""
    from wsovod_amd.layers import hip_ops as H

    scale = 0.37
    shapes = [(1, 1), (65, 9), (150, 1204), (64, 64), (1000, 4096)]
    if ykind == "x2":
        shapes = [(1, 32), (65, 96), (150, 1216), (1000, 4096)]
    for M, N in shapes:
        g = _gen(M * 5 + N)
        dy = torch.randn(M, N, generator=g)
        Np = (N + 31) // 32 * 32
        if ykind is None:
            y_dev, active = None, torch.ones(M, N, dtype=torch.bool)
        else:
            y = torch.randn(M, N, generator=g)
            flat = y.view(-1)
            for k, v in enumerate((0.0, -0.0, float("nan"), 1e-40, -1e-40)):
                flat[k % flat.numel()::13 + k] = v
            if ykind in ("bf16", "x2"):
                y = y.to(BF)
            if ykind == "x2":
                y_dev = H.x2_encode(y.float().to(gpu))
                active = _x2_planes(y_dev, M, N)[0].float() > 0
            else:
                yv, ybuf = odd_view((M, N), y.dtype, N + 7, 1, gpu)
                yv.copy_(y)
                y_dev, active = yv, y.float() > 0
        masked = torch.where(active, dy * torch.tensor(scale, dtype=torch.float32), torch.zeros(()))
        hi = masked.bfloat16()
        lo = (masked - hi.float()).bfloat16()
        dyv, dybuf = odd_view((M, N), torch.float32, N + 3, 1, gpu)
        dyv.copy_(dy)
        pre = torch.randn(N, generator=g)
        cs = pre.clone().to(gpu)
        out, plain = H.mask_x2(dyv, y_dev, scale, colsum=cs, y_x2=ykind == "x2", want_hi=True, ld_hi=(N + 7) // 8 * 8)
        assert H.carrier.fmt_of(out) == H.X2 and out.shape == (M, Np) and plain.shape == (M, (N + 7) // 8 * 8)
        ghi, glo = _x2_planes(out, M, Np)
        tag = (ykind, M, N)
        assert same_bits(ghi[:, :N], hi) and same_bits(glo[:, :N], lo), tag
        assert bool((bits(ghi[:, N:]) == 0).all()) and bool((bits(glo[:, N:]) == 0).all()), tag
        assert same_bits(plain.cpu()[:, :N], hi) and bool((bits(plain.cpu()[:, N:]) == 0).all()), tag
        assert outside_intact(dybuf, dyv) and (ykind in (None, "x2") or outside_intact(ybuf, yv)), tag
        ref, mag = masked.double().sum(0), masked.double().abs().sum(0)
        got = cs.cpu().double() - pre.double()
        assert bool(((got - ref).abs() <= M * U * mag + 2 * U * (pre.double().abs() + ref.abs())).all()), tag
        cs0 = torch.zeros(N, device=gpu)
        out2, none = H.mask_x2(dy.to(gpu), y_dev, scale, colsum=cs0, y_x2=ykind == "x2")
        assert none is None and torch.equal(out2.view(torch.int32), out.view(torch.int32)), tag
        assert bool(((cs0.cpu().double() - ref).abs() <= M * U * mag).all()), tag
        assert same_bits(cs.cpu(), pre + cs0.cpu()), tag
        # the decoded carrier is what gemm_nt(x2=True) contracts: hi + lo of the masked fp32 values
        assert same_bits(H.x2_decode(out).cpu()[:, :N], hi.float() + lo.float()), tag


def test_transposed_bf16x2_weight_and_its_cache(gpu):
    """wsovod_bf16x2_encode_t: the bytes of x2_encode(w.t().contiguous()) in the first N columns, zeros up to the next multiple
    of 32; cached on the weight under "x2t": a second call hits, an in-place update misses (and no other format's entry is
    touched)."""
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.layers import operand_cache

    for N, K in ((64, 96), (96, 40), (37, 70), (4096, 1024), (1, 1)):
        w = torch.randn(N, K, generator=_gen(N + K)).to(gpu)
        w[0, 0] = float("inf")
        Np = (N + 31) // 32 * 32
        got = H.x2_encode_t(w)
        assert got.shape == (K, Np) and H.carrier.fmt_of(got) == H.X2
        wt = torch.zeros(K, Np, device=gpu)
        wt[:, :N] = w.t()
        want = H.x2_encode(wt)  # (zero columns encode as zero bytes)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (N, K)
        if N % 32 == 0:
            assert torch.equal(got.view(torch.int32), H.x2_encode(w.t().contiguous()).view(torch.int32)), (N, K)
        ghi, glo = _x2_planes(got, K, Np)
        assert bool((bits(ghi[:, N:]) == 0).all()) and bool((bits(glo[:, N:]) == 0).all())
    # a strided source (a row block of a wider matrix)
    wide = torch.randn(64, 200, generator=_gen(3)).to(gpu)
    assert torch.equal(H.x2_encode_t(wide[:, 8:136]).view(torch.int32), H.x2_encode(wide[:, 8:136].t().contiguous()).view(torch.int32))
    w = torch.nn.Parameter(torch.randn(128, 96, generator=_gen(9)).to(gpu))
    x2 = H.x2_cached(w)
    a = H.x2t_cached(w)
    assert H.x2t_cached(w) is a and operand_cache.current(w, "x2t") is a and operand_cache.current(w, "x2") is x2
    with torch.no_grad():
        w.mul_(0.5)
    assert operand_cache.current(w, "x2t") is None
    b = H.x2t_cached(w)
    assert b is not a and torch.equal(b.view(torch.int32), H.x2_encode(w.detach().t().contiguous()).view(torch.int32))
    operand_cache.wrote(w, None)  # an update kernel wrote the weight: the transposed operand is not refreshed by any
    assert operand_cache.current(w, "x2t") is None and H.x2t_cached(w) is not b


@pytest.mark.parametrize("shape", [(16384, 4096, 4096), (333, 129, 200)], ids=["fc2", "ragged"])
def test_split_input_gradient_contraction(gpu, shape):
    """dX = dA W as gemm_nt(x2) on mask_x2's carrier and the transposed bf16x2 weight, at fc2's shape (32 images x 512
    proposals) and at a ragged one.  Against the fp64 contraction of the decoded hi + lo operands: within the x2 GEMM's bound
    of tests/test_gpu_bf16x2.py (3e-5 of sum |a||b|; the three-product model 2e-6).  Against the fp64 contraction of the
    UNROUNDED operands: closer than the plain bf16 dX (bf16 dA, bf16 W^T) on the same inputs."""
    from wsovod_amd.layers import hip_ops as H

    M, N, K = shape  # the layer's rows, outputs, inputs: dA (M, N), W (N, K), dX (M, K)
    g = torch.Generator(device="cuda").manual_seed(M + N)
    dy = torch.randn(M, N, device=gpu, generator=g)
    y = torch.randn(M, N, device=gpu, generator=g).to(BF)
    w = torch.randn(N, K, device=gpu, generator=g) * N ** -0.5
    a2, a16 = H.mask_x2(dy, y, 2.0, want_hi=True, ld_hi=(N + 7) // 8 * 8)
    wt2 = H.x2_encode_t(w)
    dx = H.gemm_nt(a2, wt2, x2=True, out_dtype=torch.float32)
    assert dx.shape == (M, K)
    dA = torch.where(y.float() > 0, dy * 2.0, torch.zeros_like(dy))
    plain = H.gemm_nt(a16, H.transpose_cast(w, BF, ld_dst=a16.shape[1]), out_dtype=torch.float32)
    wd = H.x2_decode(wt2)[:, :N].double()  # (K, N) = W^T as encoded
    worst = [0.0, 0.0, 0.0, 0.0]
    for r0 in range(0, M, 2048):  # fp64 in row blocks
        sl = slice(r0, min(M, r0 + 2048))
        ad = H.x2_decode(a2[sl].contiguous())[:, :N].double()
        ref_dec = ad @ wd.t()
        scale = ad.abs() @ wd.abs().t()
        worst[0] = max(worst[0], float(((dx[sl].double() - ref_dec).abs() / scale.clamp_min(1e-300)).max()))
        hi_a, hi_w = dA[sl].to(BF).double(), w.to(BF).double()
        model = hi_a @ hi_w + hi_a @ (w - w.to(BF).float()).to(BF).double() + (dA[sl] - dA[sl].to(BF).float()).to(BF).double() @ hi_w
        worst[1] = max(worst[1], float(((dx[sl].double() - model).abs() / scale.clamp_min(1e-300)).max()))
        ref = dA[sl].double() @ w.double()
        worst[2] = max(worst[2], float((dx[sl].double() - ref).abs().max()))
        worst[3] = max(worst[3], float((plain[sl].double() - ref).abs().max()))
    print(f"{shape}: split dX vs decoded fp64 {worst[0]:.3e} (of sum |a||b|), vs the three-product model {worst[1]:.3e}; "
          f"max |dX - fp64(unrounded)| split {worst[2]:.3e}, plain bf16 {worst[3]:.3e}")
    assert worst[0] < 3e-5 and worst[1] < 2e-6
    assert worst[2] < worst[3]


def test_f16mx_decode_kernel_equals_the_torch_composition(gpu):
    """wsovod_f16mx_to_f32 against hip_ops.mx_to_f32 (hi + ql 2^-11 composed in torch), torch.equal: encoded random values
    over the fp16 range, values beyond it (+-inf in the hi plane), hand-written bytes -- saturated e4m3 (+-448), e4m3
    denormals, +-0 --, a row of ONE group, a 4-D carrier.  Only a tensor recorded as f16mx is taken."""
    from wsovod_amd.layers import carrier
    from wsovod_amd.layers import hip_ops as H

    for rows, cols in ((1, 32), (7, 96), (513, 4096)):
        x = torch.randn(rows, cols, generator=_gen(rows)) * torch.logspace(-5, 5, cols)[None]
        x.view(-1)[::11] = 1e6    # beyond fp16: hi = inf
        x.view(-1)[5::17] = -1e6
        x.view(-1)[3::19] = 0.0
        car, _ = H.mx_encode(x.to(gpu), unit=True)
        raw = car.view(torch.uint8).view(rows, cols // 32, 128)
        raw[:, :, 96] = 0x7E  # +448, the largest e4m3 value (what a saturating encoder writes)
        raw[:, :, 97] = 0xFE  # -448
        raw[:, :, 98] = 0x01  # the smallest e4m3 denormal, 2^-9
        raw[:, :, 99] = 0x80  # -0
        got, want = H.f16mx_to_f32(car), H.mx_to_f32(car)
        assert bool(torch.isinf(want).any()) and not bool(torch.isnan(want).any())
        assert got.shape == want.shape and torch.equal(got, want), (rows, cols)
        assert same_bits(got.cpu(), want.cpu()), (rows, cols)
    nd = carrier.tag(H.mx_encode(torch.randn(6 * 4 * 4, 64, generator=_gen(1)).to(gpu), unit=True)[0].view(6, 4, 4, 64), H.MX)
    assert torch.equal(H.f16mx_to_f32(nd), H.mx_to_f32(nd))
    with pytest.raises(RuntimeError, match="f16mx"):
        H.f16mx_to_f32(torch.zeros(4, 32, device=gpu))  # untagged
    with pytest.raises(RuntimeError, match="f16mx"):
        H.f16mx_to_f32(H.x2_encode(torch.zeros(4, 32, device=gpu)))  # tagged bf16x2
