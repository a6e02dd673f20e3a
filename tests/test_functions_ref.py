"""CPU only: the fp64 restatements of tests/functions_ref.py against the C oracle and against brute force, before the GPU
files rely on them."""
import pytest
import torch

from oracle import roi_ops as O
from tests import functions_ref as FR

N, Hh, Ww = FR.MAP


@pytest.mark.parametrize("size", FR.POOL_SIZES)
def test_pool_scatter_is_the_oracles_backward(size):
    """RoIPool and the 3-output pool: argmax and values of the C oracle at the shared cases (empty bins -1, the identical
    rois equal), and the fp64 scatter through that argmax equal to the oracle's fp32 scatter within its own rounding,
    (n_max + 1) 2^-24 B -- with and without a scale (the oracle takes none: it is folded into the gradient, exactly
    representable here)."""
    rois, sc = FR.pooler_rois(), FR.pooler_scale()
    feat = FR.pooler_map(8, torch.float32, 1, nonneg=True)
    g = torch.randn(24, 8, *size, generator=torch.Generator().manual_seed(2))
    out, arg = O.roi_pool_forward(feat, rois, FR.SCALE, size)
    assert bool((arg[4] == -1).all()) and bool((out[4] == 0).all())      # wholly outside
    assert torch.equal(arg[0], arg[1]) and bool((arg[2] >= 0).all())       # identical rois; the whole map has no empty bin
    assert len(set(rois[:, 0].tolist())) == 2 and rois[:, 0].tolist() != sorted(rois[:, 0].tolist())
    flat = feat.view(N, 8, -1)
    ok = arg >= 0
    n = rois[:, 0].long().view(-1, 1, 1, 1).expand_as(arg)
    c = torch.arange(8).view(1, -1, 1, 1).expand_as(arg)
    assert torch.equal(flat[n[ok], c[ok], arg[ok].long()], out[ok])        # the value IS the cell argmax names
    for scale in (None, sc):
        gi, B, n_max = FR.roi_pool_backward(g, arg, rois, scale, feat.shape)
        gs = g.double() if scale is None else (g.double() * scale.double().view(-1, 1, 1, 1))
        assert n_max >= 2 and bool((B > 0).any()) and bool((B == 0).any())
        if scale is None:
            want = O.roi_pool_backward(g, rois, arg, feat.shape).double()
            assert bool(((gi - want).abs() <= (n_max + 1) * FR.U32 * B).all())
        assert bool((gi[B == 0] == 0).all())
        assert abs(float(gi.sum()) - float(gs[ok].sum())) <= 1e-9 * float(gs.abs().sum())  # nothing lost, nothing twice
    out3, arg3 = O.roi_loop_pool_forward(feat, rois, FR.SCALE, size)
    g3 = torch.randn(72, 8, *size, generator=torch.Generator().manual_seed(3))
    gi3, B3, _ = FR.loop_pool_backward(g3, arg3, rois, None, feat.shape)
    want3 = O.roi_pool_backward(g3, rois.repeat(3, 1), arg3, feat.shape).double()
    assert bool(((gi3 - want3).abs() <= 1e-5 * (1 + B3)).all())
    # with distinct scales, repeating them the wrong way changes the result: the GPU test can tell the two apart
    a = FR.loop_pool_backward(g3, arg3, rois, sc, feat.shape)[0]
    b = FR.pool_scatter(g3, arg3, rois[:, 0].repeat(3), sc.repeat_interleave(3), feat.shape)[0]
    assert float((a - b).abs().max()) > 1e-2


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("sampling_ratio", [0, 2])
@pytest.mark.parametrize("size", FR.POOL_SIZES)
def test_roi_align_restatement_matches_the_oracle(size, sampling_ratio, aligned):
    """The separable fp64 restatement against the fp32 C restatement of torchvision's roi_align.  The oracle's own error:
    its sample coordinates are off by at most delta (functions_ref._align_rois), each of a sample's four weights by at most
    3 delta, the average over the samples by no more; plus a handful of fp32 roundings of the weighted sum.  No sample of
    the shared cases lies near the border where a sample turns invalid."""
    rois = FR.pooler_rois()
    feat = FR.pooler_map(6, torch.float32, 4)
    assert FR.roi_align_margin(rois, FR.SCALE, size, sampling_ratio, aligned, Hh, Ww) > 1e-3
    want = O.roi_align_forward(feat, rois, FR.SCALE, size, sampling_ratio, aligned).double()
    got = FR.roi_align(feat.double(), rois, FR.SCALE, size, sampling_ratio, aligned)
    delta = max(d for *_, d in FR._align_rois(rois, FR.SCALE, size, sampling_ratio, aligned, Hh, Ww))
    tol = (4 * 3 * delta + 16 * FR.U32) * float(feat.abs().max())
    assert float((got - want).abs().max()) <= tol, (float((got - want).abs().max()), tol)
    assert bool((got[4] == 0).all()) and float(got.abs().max()) > 0.1
    # the backward helper: autograd's gradient, the magnitude map and the reach map are consistent
    g = torch.randn(24, 6, *size, generator=torch.Generator().manual_seed(5))
    gi, B, D, n_max = FR.roi_align_backward(g, rois, FR.pooler_scale(), FR.SCALE, sampling_ratio, aligned, feat.shape)
    want_gi = O.roi_align_backward(g * FR.pooler_scale().view(-1, 1, 1, 1), rois, FR.SCALE, sampling_ratio, aligned,
                                   feat.shape).double()
    assert bool(((gi - want_gi).abs() <= (n_max + 4) * FR.U32 * B + 3 * D + 1e-30).all())
    assert bool((gi.abs() <= B * (1 + 1e-12)).all()) and bool((D[B > 0] > 0).all()) and n_max >= 4


def _label_case():
    """12 anchors, 3 images with [2, 0, 3] boxes, integer coordinates, thresholds 0.25 / 0.5: IoU exactly on both thresholds,
    a tie for a box's best below thr_lo, an anchor that ties another box's best, a box that overlaps nothing."""
    anchors = torch.tensor([[0, 0, 16, 32], [0, 0, 16, 16], [0, 0, 8, 16], [100, 100, 108, 108], [124, 124, 132, 132],
                            [200, 0, 232, 16], [232, 0, 264, 16], [200, 0, 232, 7], [300, 300, 316, 316],
                            [308, 300, 324, 316], [400, 400, 410, 410], [0, 40, 16, 56]], dtype=torch.float32)
    gt = torch.tensor([[0, 0, 16, 32], [100, 100, 132, 132],
                       [200, 0, 232, 7], [216, 0, 248, 16], [1000, 1000, 1010, 1010]], dtype=torch.float32)
    return anchors, gt, torch.tensor([0, 2, 2], dtype=torch.int32), torch.tensor([2, 0, 3], dtype=torch.int32)


def test_label_restatement_matches_brute_force():
    anchors, gt, start, count = _label_case()
    lab, best_gt, best_iou, unique = FR.label_anchors(anchors, gt, start, count, 0.25, 0.5)
    blab, biou = FR.label_anchors_brute(anchors, gt, start, count, 0.25, 0.5)
    assert torch.equal(lab, blab) and torch.equal(best_iou, biou)
    # image 0: the thresholds and the tie
    assert best_iou[0, :3].tolist() == [1.0, 0.5, 0.25] and lab[0, :3].tolist() == [1, 1, -1]
    assert best_iou[0, 3] == best_iou[0, 4] == 0.0625 and lab[0, 3] == lab[0, 4] == 1     # both attain box 1's best
    assert lab[0, 8:].tolist() == [0, 0, 0, 0] and best_gt[0, 1] == 0 and best_gt[0, 3] == 1
    # image 1: no boxes
    assert bool((lab[1] == 0).all()) and bool((best_gt[1] == -1).all())
    # image 2: anchor 5's own best is box 2 (0.4375, between the thresholds), it ties anchor 6 for box 3's best (1/3);
    # box 4 overlaps nothing: its best IoU is 0, and every anchor that has IoU 0 with it -- all of them -- is positive
    assert best_gt[2, 5] == 2 and float(best_iou[2, 5]) == 0.4375 and best_gt[2, 6] == 3
    assert bool((lab[2] == 1).all())
    lab2, _, _, _ = FR.label_anchors(anchors, gt[:4], start, torch.tensor([2, 0, 2], dtype=torch.int32), 0.25, 0.5)
    assert lab2[2].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0]   # without box 4: anchor 5 positive by the tie alone
    assert bool(unique[0, :5].all()) and not bool(unique[2, 8])      # (image 2, anchor 8: all three boxes at IoU 0)


def test_small_restatements():
    """cosine_logits with and without normalize, the zero row and the row below eps; GAP; add_group_rows."""
    g = torch.Generator().manual_seed(7)
    z = torch.relu(torch.randn(5, 16, generator=g, dtype=torch.float64))
    z[1] = 0
    z[2] = 1e-14 * z[0]
    wn = torch.nn.functional.normalize(torch.randn(4, 16, generator=g, dtype=torch.float64), dim=1)
    wn[3] = 0
    dl = torch.randn(5, 4, generator=g, dtype=torch.float64)
    ref = FR.cosine_reference(z, wn, 50.0, True, torch.zeros(4, dtype=torch.float64), dl)
    assert bool((ref["logits"][1] == 0).all()) and bool((ref["logits"][:, 3] == 0).all())
    # clamped rows: d/dz of T z / eps is T dl wn / eps, no projection term
    want = 50.0 / 1e-12 * (dl[1:3] @ wn)
    assert torch.allclose(ref["dz"][1:3], want, rtol=1e-12, atol=0)
    assert bool((ref["dz"].abs() <= ref["B_dz"] * (1 + 1e-9)).all()) and bool((ref["logits"].abs() <= ref["B_logits"] * (1 + 1e-9)).all())
    assert torch.equal(ref["db"], dl.sum(0))
    plain = FR.cosine_reference(z, wn, 50.0, False, None, dl)
    assert torch.allclose(plain["dz"], dl @ wn) and plain["db"] is None
    x = torch.randn(2, 5, 7, 3, generator=g)
    assert torch.allclose(FR.gap(x), x.sum((1, 2)) / 35)
    rg = torch.tensor([0, 0, 2, 3], dtype=torch.int32)
    assert torch.equal(FR.add_group_rows(torch.zeros(4, 2), torch.arange(8.0).view(4, 2), rg)[:, 0], torch.tensor([0.0, 0.0, 4.0, 6.0]))
