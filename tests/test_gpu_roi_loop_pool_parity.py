"""-m gpu: POOLER_TYPE ROILoopPool + the contextlocnet mining head under MODEL.HIP.PRECISION "parity", "parity_mx" and
"parity_mx_train", against the oracle on identical seeded parameters (the harness of
tests/test_gpu_model_parity.py::test_roi_loop_pool_contextlocnet_step_matches_oracle).

The bound is the project's standing one: mining scores and refinement logits within 1e-3 absolute of the oracle's, labels
and pseudo-GT classes exact, every trainable gradient finite.

MEASURED on an MI355X:     parity           2 x 40 boxes    mining scores 1.1e-05   refinement logits 1.6e-04
    parity_mx        2 x 700 boxes   mining scores 1.2e-05   refinement logits 2.2e-04   (pooled carrier f16mx, 4179 rows)
    parity_mx        2 x 40 boxes    bf16x2 route, bit-identical to "parity"
    parity (eval)    2 x 40 boxes    all_scores 2.3e-05
    parity_mx_train  2 x 700 boxes   forward bit-identical to "parity_mx"
(2 images of 256 x 352, max |HIP - oracle|; the bar is 1e-3)
"""
import pytest
import torch

from oracle import wsovod_ref as R
from tests.golden import gen
from tests.helpers import build_seeded_hip_model, to_inputs

pytestmark = pytest.mark.gpu

BAR = 1e-3  # the north star: MIL-head logits within 1e-3 of the reference
_REF = {}


def _batch(n_props):
    return gen.seeded_batch(2, n_props, 20, 256, 352, seed=61)


def _oracle(n_props, sd, classifier=None):
    """The oracle's step on the seeded parameters: computed once per (proposal count, classifier) and left unchanged."""
    key = (n_props, classifier is not None)
    if key not in _REF:
        sdc = {k: v.clone() for k, v in sd.items()}
        with torch.no_grad():
            _, inter = R.train_forward(sdc, _batch(n_props), depth=18, num_classes=20, pixel_std=gen.PIXEL_STD,
                                       pooler_type="ROILoopPool", classifier=classifier)
        _REF[key] = {"mining_scores": inter["mining_scores"], "refine_logits": inter["refine_logits"],
                     "gt_classes": torch.cat([l["gt_classes"] for l in inter["labelled"]]),
                     "gt_boxes": torch.cat([l["gt_boxes"] for l in inter["labelled"]])}
    return _REF[key]


def _step(model, batch):
    """One training forward + backward -> (losses, mining scores, refinement logits, pseudo-GT dict, pooled tensor)."""
    captured = {}
    rh = model.roi_heads
    orig_m, orig_r, orig_p = rh.object_miner.forward, rh.box_refinery[0].forward, rh.pool_features

    def cap(name, fn):
        def w(*a, **k):
            o = fn(*a, **k)
            captured[name] = o
            return o
        return w

    rh.object_miner.forward, rh.box_refinery[0].forward = cap("miner", orig_m), cap("refine", orig_r)
    rh.pool_features = cap("pooled", orig_p)
    try:
        losses = model(to_inputs(batch))
    finally:
        rh.object_miner.forward, rh.box_refinery[0].forward, rh.pool_features = orig_m, orig_r, orig_p
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return ({k: v.detach() for k, v in losses.items()}, captured["miner"][0].detach(), captured["refine"][0].detach(),
            rh._last_pgt, captured["pooled"])


def _check_against_oracle(tag, model, sd, n_props, scores, logits, pgt):
    ref = _oracle(n_props, sd)
    es = float((scores.cpu() - ref["mining_scores"]).abs().max())
    el = float((logits.cpu() - ref["refine_logits"]).abs().max())
    print(f"{tag}: max |mining scores - oracle| = {es:.3e}, max |refinement logits - oracle| = {el:.3e}")
    assert es < BAR and el < BAR, (tag, es, el)
    assert torch.equal(pgt["gt_classes"].cpu(), ref["gt_classes"]), tag
    assert torch.equal(pgt["gt_boxes"].cpu(), ref["gt_boxes"]), tag  # (the pseudo-GT box every proposal was matched to)
    for k, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (tag, k)


def test_parity_step_matches_the_oracle(gpu):
    """"parity": the pooler writes planar bf16x2 for the three parts at once (training: with its hi plane as fc1's weight-
    gradient operand), the neck runs on 3R rows, the miner on the three row blocks of its bf16x2 output."""
    from wsovod_amd.layers import hip_ops as H

    cfg, model, sd = build_seeded_hip_model("parity", pooler="ROILoopPool")
    batch = _batch(40)
    losses, scores, logits, pgt, pooled = _step(model, batch)
    rows = 3 * sum(len(b["boxes"]) for b in batch)
    assert pooled.shape[0] == rows and H.carrier.fmt_of(pooled) in (H.X2, H.carrier.X2P) and H.x2_hi_pop(pooled) is not None
    _check_against_oracle("parity 2 x 40", model, sd, 40, scores, logits, pgt)


def test_parity_mx_step_above_the_row_threshold_runs_on_f16mx(gpu):
    """"parity_mx" with 3R >= MX_MIN_ROWS: the pooled carrier IS f16mx (else this would pass on the bf16x2 route and show
    nothing), fc1 and fc2 contract it on the f16mx kernels, and the step meets the same bar."""
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.modeling.roi_heads import WSOVODROIHeads

    cfg, model, sd = build_seeded_hip_model("parity_mx", pooler="ROILoopPool")
    batch = _batch(700)
    rows = 3 * sum(len(b["boxes"]) for b in batch)
    assert sum(len(b["boxes"]) for b in batch) < WSOVODROIHeads.MX_MIN_ROWS <= rows  # only the 3R count crosses it
    losses, scores, logits, pgt, pooled = _step(model, batch)
    assert pooled.shape[0] == rows and H.mx_of(pooled), H.carrier.fmt_of(pooled)
    _check_against_oracle("parity_mx 2 x 700", model, sd, 700, scores, logits, pgt)


def test_parity_mx_below_the_row_threshold_is_the_parity_step(gpu):
    """"parity_mx" with 3R < MX_MIN_ROWS keeps the bf16x2 output (its split-K GEMM forms win at few rows): the carrier is
    bf16x2 and the step's scores, logits and losses are "parity"'s bit for bit."""
    from wsovod_amd.layers import hip_ops as H

    batch = _batch(40)
    got = {}
    for precision in ("parity", "parity_mx"):
        cfg, model, sd = build_seeded_hip_model(precision, pooler="ROILoopPool")
        got[precision] = _step(model, batch)
        del model
    pooled = got["parity_mx"][4]
    assert not H.mx_of(pooled) and H.carrier.fmt_of(pooled) in (H.X2, H.carrier.X2P)
    assert torch.equal(got["parity"][1], got["parity_mx"][1]) and torch.equal(got["parity"][2], got["parity_mx"][2])
    for k, v in got["parity"][0].items():
        assert torch.equal(v, got["parity_mx"][0][k]), k


def test_parity_inference_matches_the_oracles_all_scores(gpu):
    """Eval mode under "parity": no argmax, no bf16 copy, the refinement head reads the region rows.  all_scores =
    softmax of the oracle's refinement logits on the same class embeddings (REFINE_NUM = 1), within 1e-3."""
    cfg, model, sd = build_seeded_hip_model("parity", pooler="ROILoopPool")
    model.eval()
    batch = _batch(40)
    clf = torch.randn(20, 512, generator=torch.Generator().manual_seed(3))
    ref = torch.softmax(_oracle(40, sd, classifier=clf)["refine_logits"], dim=-1)
    results, all_scores, all_boxes = model.inference(to_inputs(batch), do_postprocess=False, classifier=clf.to(gpu))
    got = torch.cat([s[0] for s in all_scores]).cpu()
    assert got.shape == ref.shape
    err = float((got - ref).abs().max())
    print(f"parity eval 2 x 40: max |all_scores - oracle| = {err:.3e}")
    assert err < BAR
    assert all(bool(torch.isfinite(b[0]).all()) for b in all_boxes) and len(results) == 2


def test_parity_mx_train_forward_is_parity_mx_bit_for_bit(gpu):
    """"parity_mx_train" at the above-threshold size: the same forward kernels on the same inputs as "parity_mx" -- losses,
    mining scores and refinement logits torch.equal, the pooled carrier f16mx -- and a backward that leaves every trainable
    gradient finite."""
    from wsovod_amd.layers import hip_ops as H

    batch = _batch(700)
    got = {}
    for precision in ("parity_mx", "parity_mx_train"):
        cfg, model, sd = build_seeded_hip_model(precision, pooler="ROILoopPool")
        got[precision] = _step(model, batch)
        for k, p in model.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (precision, k)
        del model
    assert H.mx_of(got["parity_mx"][4]) and H.mx_of(got["parity_mx_train"][4])
    assert torch.equal(got["parity_mx"][1], got["parity_mx_train"][1])
    assert torch.equal(got["parity_mx"][2], got["parity_mx_train"][2])
    for k, v in got["parity_mx"][0].items():
        assert torch.equal(v, got["parity_mx_train"][0][k]), k
