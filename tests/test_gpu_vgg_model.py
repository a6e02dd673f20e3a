"""-m gpu: the VGG16 DC5 model (wsovod_amd/modeling/backbone_vgg.py) end to end against the oracle.  The oracle's backbone is
the ResNet restatement; these tests put tests/vgg_util.py:vgg16_ref -- pinned to the reference's own VGG16 by
tests/test_vgg_host.py -- in its place (`R.backbone_forward`), everything downstream of the map is the oracle's own code.

Two ragged images (96 x 128 and 88 x 112), 64 / 57 proposals, K = 20, the synthetic calibrated model of
wsovod_amd.testing (conv1_1 scaled by 1/64: every activation from plain3 on is below 1.2 on this batch -- measured with
vgg16_ref on the CPU -- far inside f16mx's exact range, 432)."""
import pytest
import torch

from oracle import wsovod_ref as R
from tests import vgg_util
from tests.golden import gen
from tests.helpers import to_inputs

pytestmark = pytest.mark.gpu

K = 20
V16_MEAN = (103.939, 116.779, 123.68)
_CACHE = {}


def _batch():
    return gen.seeded_batch(2, 64, K, 96, 128, seed=21)


def _build(precision, rpn=False, dilation=2):
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import build_hot_path_model, hot_path_cfg

    if dilation == 2:
        cfg, model = build_hot_path_model(seed=0, backbone="vgg16", K=K, precision=precision, device="cuda:0", rpn=rpn)
    else:
        cfg = hot_path_cfg(backbone="vgg16", K=K, precision=precision, device="cuda:0")
        cfg.MODEL.VGG.CONV5_DILATION = dilation
        torch.manual_seed(0)
        model = build_model(cfg)
        with torch.no_grad():
            model.backbone.plain1[0].conv1.weight.mul_(1.0 / 64.0)
    assert tuple(cfg.MODEL.PIXEL_MEAN) == V16_MEAN
    model.train()
    for m in model.modules():  # dropout RNG streams cannot match the reference's: off on both sides
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    return cfg, model, sd


def _vgg_oracle(monkeypatch, dilation=2):
    monkeypatch.setattr(R, "backbone_forward",
                        lambda sd, x, depth=18, **kw: {"res5": vgg_util.vgg16_ref(sd, x, dilation, prefix="backbone.")})


def _reference(monkeypatch, sd):
    """The oracle's training forward on the seeded VGG model: computed once, shared (every precision starts from the same
    seeded weights), never modified."""
    if "train" not in _CACHE:
        _vgg_oracle(monkeypatch)
        with torch.no_grad():
            _CACHE["train"] = R.train_forward(sd, _batch(), num_classes=K, pixel_mean=V16_MEAN)
        _CACHE["w0"] = sd["backbone.plain3.0.conv1.weight"].clone()
    assert torch.equal(_CACHE["w0"], sd["backbone.plain3.0.conv1.weight"])
    return _CACHE["train"]


def _lower_mx_thresholds(monkeypatch):
    from wsovod_amd.modeling.backbone_vgg import VGG16
    from wsovod_amd.modeling.roi_heads import WSOVODROIHeads

    monkeypatch.setattr(VGG16, "MX_MIN_TILES", 1)
    monkeypatch.setattr(WSOVODROIHeads, "MX_MIN_ROWS", 1)


def _plain5(model, inputs, **kw):
    canvas, sizes_t, _ = model._canvas(inputs)
    from wsovod_amd.layers import hip_ops as H

    with torch.no_grad(), H.mx_mode(model.mx_on):
        return model.backbone.forward_uint8(canvas, sizes_t, model._mean, model._std, **kw)["plain5"]


def test_fp32_step_matches_the_oracle(gpu, monkeypatch):
    """plain5, pooled features, mining scores, refinement logits and the losses.  Tolerances: those of
    tests/test_gpu_model_parity.py::test_fp32_intermediates_match_oracle -- the backbone map rtol 1e-3 / atol 3e-4, losses
    rtol 1e-3 / atol 1e-5, the MIL-head logits 1e-3 absolute (that file's fp32 bar); the pooled tensor is the map's own
    elements times (objectness + 1) <= 2, hence twice the map's absolute term."""
    from wsovod_amd.testing import capture_full_step

    cfg, model, sd = _build("fp32")
    ref_losses, inter = _reference(monkeypatch, sd)
    inputs = to_inputs(_batch())
    got = _plain5(model, inputs).float().cpu().contiguous()
    assert got.shape == inter["res5"].shape == (2, 512, 96 // 8 - 1, 128 // 8 - 1)
    print("fp32 plain5 max |err|", float((got - inter["res5"]).abs().max()), "max |ref|", float(inter["res5"].abs().max()))
    torch.testing.assert_close(got, inter["res5"], rtol=1e-3, atol=3e-4)
    x = model.preprocess_image(inputs).tensor  # the generic float entry (reference signature) gives the same map
    torch.testing.assert_close(model.backbone(x)["plain5"].float().cpu().contiguous(), inter["res5"], rtol=1e-3, atol=3e-4)
    dev_inputs = [{**x, "image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu)} for x in inputs]
    st = model.forward_frozen(dev_inputs)
    torch.testing.assert_close(st["pooled"].float().cpu().reshape(inter["pooled"].shape), inter["pooled"], rtol=1e-3, atol=6e-4)
    out = capture_full_step(model, dev_inputs)
    print("fp32 logits", float((out["refine_logits"] - inter["refine_logits"]).abs().max()),
          "scores", float((out["mining_scores"] - inter["mining_scores"]).abs().max()))
    assert float((out["mining_scores"] - inter["mining_scores"]).abs().max()) < 1e-3
    assert float((out["refine_logits"] - inter["refine_logits"]).abs().max()) < 1e-3
    for k, v in ref_losses.items():
        torch.testing.assert_close(torch.tensor(out["losses"][k]), v.detach().float(), rtol=1e-3, atol=1e-5, msg=lambda m: f"{k}: {m}")


def test_fp32_undilated_map_matches_the_oracle(gpu):
    """CONV5_DILATION = 1: plain4 ends in MaxPool2d(2, 2), stride 16; the backbone map alone."""
    cfg, model, sd = _build("fp32", dilation=1)
    inputs = to_inputs(_batch())
    x = R.preprocess_image([b["image"] for b in _batch()], V16_MEAN, (1.0, 1.0, 1.0))
    want = vgg_util.vgg16_ref(sd, x, 1, prefix="backbone.")
    got = _plain5(model, inputs).float().cpu().contiguous()
    assert got.shape == want.shape == (2, 512, 96 // 16, 128 // 16)
    torch.testing.assert_close(got, want, rtol=1e-3, atol=3e-4)


def _launched():
    from wsovod_amd import _lib

    return {e["name"] for e in _lib.profile_collect() if e["launches"] > 0}


@pytest.mark.parametrize("precision", ["parity", "parity_mx"])
def test_parity_precisions_hold_the_logit_bar(gpu, precision, monkeypatch):
    """MIL-head logits (mining scores, refinement logits) within 1e-3 of the oracle; labels and pseudo-GT exact when the
    oracle mines from the HIP path's own scores.  parity_mx: thresholds lowered so that the f16mx convs (plain3 on), the
    f16mx pools and f16mx fc1 / fc2 run -- asserted from the library's launch profile -- and an f16mx_range audit of the
    crossing map and of every f16mx producer shows no top code and no non-finite value."""
    from wsovod_amd import _lib
    from wsovod_amd.layers import hip_ops as H, mx_guard
    from wsovod_amd.testing import capture_full_step

    mx = precision == "parity_mx"
    if mx:
        _lower_mx_thresholds(monkeypatch)
    cfg, model, sd = _build(precision)
    ref_losses, inter = _reference(monkeypatch, sd)
    batch = _batch()
    inputs = to_inputs(batch)
    dev_inputs = [{**x, "image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu)} for x in inputs]
    if mx:  # which kernels run, and the range audit of what they wrote (the guard's own table, armed by hand)
        guard = mx_guard.MxRangeGuard("warn")
        guard.names.update({id(m): n for n, m in model.named_modules() if n})
        guard.arm()
        _lib.profile_reset()
        _lib.profile_enable(True)
        try:
            with mx_guard.active(guard):
                canvas, sizes_t, _ = model._canvas(inputs)
                with torch.no_grad(), H.x3_mode("x2"), H.mx_mode(True):
                    feats = model.backbone.forward_uint8(canvas, sizes_t, model._mean, model._std)
            names = _launched()
        finally:
            _lib.profile_enable(False)
        assert "conv_igemm_f16mx_256x256_8ph" in names and "maxpool2x2_nhwc_f16mx" in names, names
        assert "stem_conv1_s1_fused_bf16x2" in names and "f16mx_from_bf16x2" in names, names
        rep = guard.poll()
        print({k: tuple(v) for k, v in rep.items()})
        assert "backbone.mx_from_x2" in rep and any(k.startswith("backbone.plain5.0.conv") for k in rep)
        assert any(k == "backbone.plain3.0" for k in rep)  # (the f16mx pool's output)
        for site, r in rep.items():
            assert r.audited > 0 and r.nonfinite == 0 and r.top_code == 0 and r.max_abs < 432, (site, r)
        _lib.profile_reset()
        _lib.profile_enable(True)
    try:
        out = capture_full_step(model, dev_inputs)
        if mx:
            names = _launched()
            assert "gemm_nt_f16mx_256x256_8ph" in names, names  # fc1 / fc2
    finally:
        if mx:
            _lib.profile_enable(False)
    e_logit = float((out["refine_logits"] - inter["refine_logits"]).abs().max())
    e_score = float((out["mining_scores"] - inter["mining_scores"]).abs().max())
    print(f"{precision}: max |logit err| {e_logit:.3e}, max |score err| {e_score:.3e}")
    assert e_logit < 1e-3 and e_score < 1e-3
    # proposal indexing: exact GIVEN identical scores -- the oracle mines from the HIP path's own scores
    nums = [len(b["boxes"]) for b in batch]
    gt_int, _ = R.get_image_level_gt([b["gt_classes"] for b in batch], K)
    tg = R.get_pgt_top_k([b["boxes"] for b in batch], list(out["mining_scores"].split(nums)), gt_int, out["img_scores"], K)
    lab = R.label_and_sample_proposals_wsl([b["boxes"] for b in batch], tg, K)
    assert out["pgt_num"] == [len(t["gt_classes"]) for t in tg]
    assert torch.equal(out["pgt_boxes"], torch.cat([t["gt_boxes"] for t in tg]))
    assert torch.equal(out["pgt_classes"], torch.cat([t["gt_classes"] for t in tg]))
    assert torch.equal(out["gt_classes"], torch.cat([l["gt_classes"] for l in lab]))
    assert torch.equal(out["gt_boxes"], torch.cat([l["gt_boxes"] for l in lab]))


def test_parity_mx_below_its_thresholds_is_the_parity_forward(gpu):
    """Two small images are far below MX_MIN_TILES: every layer stays on bf16x2 and the map is "parity"'s, bit for bit."""
    inputs = to_inputs(_batch())
    maps = []
    for precision in ("parity", "parity_mx"):
        cfg, model, sd = _build(precision)
        assert model.mx == (precision == "parity_mx")
        maps.append(_plain5(model, inputs).clone())
    assert maps[0].dtype == torch.float32 and torch.equal(maps[0], maps[1])


@pytest.mark.parametrize("precision", ["bf16", "parity"])
def test_image_blocks_equal_the_unblocked_run(gpu, precision, monkeypatch):
    """CONV_MAX_OPERAND_BYTES lowered so that the full-resolution plain1 map goes through conv1_2 in blocks of one image
    (at 800 x 600 that is the normal path from 18 images up)."""
    from wsovod_amd.modeling import conv as B

    cfg, model, sd = _build(precision)
    g = torch.Generator().manual_seed(5)
    inputs = [{"image": torch.randint(0, 256, (3, 48, 64), dtype=torch.uint8, generator=g)} for _ in range(3)]
    want = _plain5(model, inputs).clone()
    esize = 2 if precision == "bf16" else 4
    monkeypatch.setattr(B, "CONV_MAX_OPERAND_BYTES", 48 * 64 * 64 * esize + 1)  # one image of the plain1 map
    got = _plain5(model, inputs)
    assert got.shape == want.shape == (3, 512, 5, 7) and torch.equal(got, want)
    monkeypatch.setattr(B, "CONV_MAX_OPERAND_BYTES", 1)  # (every conv in blocks of one image)
    assert torch.equal(_plain5(model, inputs), want)


@pytest.mark.parametrize("precision", ["bf16", "parity"])
def test_backbone_graph_replay_equals_eager(gpu, precision):
    cfg, model, sd = _build(precision)
    bb = model.backbone
    g = torch.Generator().manual_seed(7)
    batches = [[{"image": torch.randint(0, 256, (3, 96, 128), dtype=torch.uint8, generator=g).to(gpu)} for _ in range(2)]
               for _ in range(2)]
    eager = [_plain5(model, b).clone() for b in batches]
    bb.graph_max_batch = 8
    try:
        for _ in range(bb.GRAPH_AFTER - 1):  # a shape is captured on its GRAPH_AFTER-th call
            assert torch.equal(_plain5(model, batches[0], allow_graph=True), eager[0]) and not bb.__dict__.get("_graphs")
        got = [_plain5(model, b, allow_graph=True).clone() for b in batches]
        assert len(bb._graphs) == 1 and all(bb._graphs.values())  # captured, not refused
        assert all(torch.equal(a, b) for a, b in zip(got, eager))
        assert _plain5(model, batches[0], allow_graph=True).data_ptr() == _plain5(model, batches[1], allow_graph=True).data_ptr()
    finally:
        bb.graph_max_batch = 0


def test_inference_tail_matches_the_oracle(gpu):
    """model.inference on the VGG model: threshold + per-class NMS + top-k on the HIP path's own scores and boxes give the
    oracle tail's boxes, classes and proposal ids (the form of test_eval_tail_matches_oracle)."""
    cfg, model, sd = _build("fp32")
    model.eval()
    batch = gen.seeded_batch(2, 120, K, 96, 128, seed=23)
    torch.manual_seed(3)
    results, all_scores, all_boxes = model.inference(to_inputs(batch), do_postprocess=False,
                                                     classifier=torch.randn(K, 512, device=gpu))
    pred = model.roi_heads.box_refinery[-1]
    checked = 0
    for b, res, sc, bx in zip(batch, results, all_scores, all_boxes):
        rb, rs, rc, ri = R.fast_rcnn_inference_single_image(bx[0].cpu(), sc[0].cpu(), tuple(b["image"].shape[-2:]),
                                                            pred.test_score_thresh, pred.test_nms_thresh,
                                                            pred.test_topk_per_image)
        assert torch.equal(res.pred_classes.cpu(), rc) and torch.equal(res.pred_inds.cpu(), ri)
        assert torch.equal(res.pred_boxes.tensor.cpu(), rb) and torch.equal(res.scores.cpu(), rs)
        checked += len(rc)
    assert checked > 0


def test_rpn_branch_on_plain5_matches_the_oracle(gpu, monkeypatch):
    """IN_FEATURES = ["plain5"]: one fp32 training step with the RPN branch; given the HIP path's own RPN boxes every loss
    agrees with the oracle's train_forward(rpn=...) (the form and tolerances of
    tests/test_gpu_rpn.py::test_rpn_head_gradients_match_oracle)."""
    cfg, model, sd = _build("fp32", rpn=True)
    assert model.proposal_generator.in_features == ["plain5"]
    cur, max_iter = 1000, 4000
    model.cfg.SOLVER.MAX_ITER = max_iter  # (the objectness ramp iter / MAX_ITER = 0.25, as in tests/test_gpu_rpn.py)
    model.roi_heads.iter = cur
    monkeypatch.setattr(model.proposal_generator, "_sample_keys",
                        lambda B, A, dev: torch.arange(A, device=dev, dtype=torch.float32).expand(B, A))
    batch = _batch()
    losses = model(to_inputs(batch))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    ramp = cur / max_iter
    props = []
    for p in model.rpn_proposals:  # undo sigmoid * ramp: the oracle applies it itself
        s = p.objectness_logits.cpu() / ramp
        props.append((p.proposal_boxes.tensor.cpu(), torch.log(s / (1 - s))))
    _vgg_oracle(monkeypatch)
    with torch.no_grad():
        ref_losses, inter = R.train_forward(sd, batch, num_classes=K, pixel_mean=V16_MEAN,
                                            rpn=dict(cur_iter=cur, max_iter=max_iter, subsample=gen.first_k_subsample,
                                                     proposals=props))
    assert set(ref_losses) >= {"loss_rpn_cls", "loss_rpn_loc"}
    for name, v in ref_losses.items():
        torch.testing.assert_close(losses[name].detach().cpu(), v.detach(), rtol=2e-3, atol=1e-5, msg=lambda m: f"{name}: {m}")
    for k, q in model.named_parameters():
        if k.startswith("proposal_generator."):
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), k
