"""-m gpu: the MIST mining kernels (wsovod_mist_select, wsovod_mist_merge, wsovod_mist_label around wsovod_nms_segments)
against the torch restatement of tests/mist_util.py (anchored to the reference by tests/test_mist_host.py), all exact.

The select sweep is a thinned product, not the full cross of R x C x images: every (pattern, valid fraction, floor) case
walks all twelve R with C cycling through (1, 2, 5, 20), all four C at R = 257, and three 3-image batches of unequal R."""
import pytest
import torch

from tests import mist_util as U
from tests.conftest import *  # noqa: F401,F403
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

K = 20
RS = (1, 6, 7, 13, 14, 20, 63, 64, 65, 257, 1000, 5024)   # the small ones walk k over 1, 1, 1, 2, 3
CS = (1, 2, 5, 20)
TRIPLES = ((7, 65, 257), (1, 1000, 14), (64, 5024, 20))    # three images of unequal R


def bits(t):
    return t.contiguous().view(torch.int32)


def make_boxes(r, valid, gen):
    x0, y0 = torch.rand(r, generator=gen) * 300, torch.rand(r, generator=gen) * 200
    b = torch.stack([x0, y0, x0 + 6 + torch.rand(r, generator=gen) * 80, y0 + 6 + torch.rand(r, generator=gen) * 60], 1)
    tiny = torch.cat([b[:, :2], b[:, :2] + 2.0 + 2.0 * torch.rand(r, 2, generator=gen)], 1)  # area in (4, 16)
    if valid == "half":
        b[::2] = tiny[::2]
    elif valid == "one":
        keep = r // 2
        tiny[keep] = b[keep]
        b = tiny
    elif valid == "none":
        b = tiny
    return b


def make_scores(pattern, floor, r, gen):
    if pattern == "random":
        x = torch.rand(r, K, generator=gen)
    elif pattern == "levels":  # 5 distinct values: ties by position straddle the k-th
        x = torch.randint(0, 5, (r, K), generator=gen).float() / 4
    elif pattern == "equal":
        x = torch.full((r, K), 0.375)
    else:  # "special": +-0, +-inf and the canonical NaN among few distinct values
        x = torch.randint(0, 3, (r, K), generator=gen).float() / 2
        pick = torch.randint(0, 8, (r, K), generator=gen)
        for code, v in ((0, 0.0), (1, -0.0), (2, float("inf")), (3, float("-inf")), (4, float("nan"))):
            x = torch.where(pick == code, torch.full_like(x, v), x)
    if floor == "below":
        return x * 0.04
    if floor == "above":
        return x * 0.9 + 0.06
    return x * 0.12  # mixed: the floor cuts some ranks and not others


def to_device(images, dev, wide=0):
    """[(boxes, scores, classes)] -> the kernels' inputs.  wide > 0: the scores are a column block of a wider matrix."""
    nums = [len(b) for b, _, _ in images]
    seg = torch.tensor([0] + torch.tensor(nums).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    boxes = torch.cat([b for b, _, _ in images]).to(dev)
    scores = torch.cat([s for _, s, _ in images])
    if wide:
        full = torch.full((scores.size(0), scores.size(1) + 2 * wide), 7.0)
        full[:, wide:wide + scores.size(1)] = scores
        scores = full.to(dev)[:, wide:wide + K]
        assert not scores.is_contiguous()
    else:
        scores = scores.to(dev)
    gt_cat = torch.cat([c for _, _, c in images]).to(dev)
    gt_off = torch.tensor([0] + torch.tensor([len(c) for _, _, c in images]).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    return scores, boxes, seg, gt_cat, gt_off, max(nums), max(len(c) for _, _, c in images)


def check_select(images, dev, wide=0):
    from wsovod_amd.layers import hip_ops as H

    scores, boxes, seg, gt_cat, gt_off, max_rows, _ = to_device(images, dev, wide)
    k_cap = H.mist_k(max_rows)
    s, i, n = (t.cpu() for t in H.mist_select(scores, boxes, seg, gt_cat, gt_off, K, k_cap))
    t = 0
    for b, sc, cl in images:
        for want_s, want_i in U.select(b, sc, cl):
            tag = (len(b), cl.tolist(), t)
            assert int(n[t]) == len(want_s), tag
            assert torch.equal(bits(s[t, :len(want_s)]), bits(want_s)), tag
            assert torch.equal(i[t, :len(want_s)].long(), want_i), tag
            t += 1


@pytest.mark.parametrize("floor", ["below", "above", "mixed"])
@pytest.mark.parametrize("valid", ["all", "half", "one", "none"])
@pytest.mark.parametrize("pattern", ["random", "levels", "equal", "special"])
def test_select_equals_the_restatement(gpu, pattern, valid, floor):
    gen = torch.Generator().manual_seed(sum(map(ord, pattern + valid + floor)))
    one = lambda r, c: (make_boxes(r, valid, gen), make_scores(pattern, floor, r, gen),  # noqa: E731
                        torch.randperm(K, generator=gen)[:c].sort()[0])
    for n, r in enumerate(RS):
        check_select([one(r, CS[n % 4])], gpu)
    for c in CS:
        check_select([one(257, c)], gpu)
    for n, rs in enumerate(TRIPLES):
        check_select([one(r, CS[(n + j) % 4]) for j, r in enumerate(rs)], gpu)


def test_select_reads_a_column_block_of_a_wider_matrix(gpu):
    gen = torch.Generator().manual_seed(5)
    images = [(make_boxes(r, "half", gen), make_scores("random", "mixed", r, gen), torch.tensor([1, 4, 19])) for r in (65, 300)]
    check_select(images, gpu, wide=3)


def test_select_refuses_a_capacity_above_the_sort(gpu):
    from wsovod_amd.layers import hip_ops as H

    images = [(make_boxes(8, "all", torch.Generator().manual_seed(1)), torch.rand(8, K), torch.tensor([2]))]
    scores, boxes, seg, gt_cat, gt_off, _, _ = to_device(images, gpu)
    with pytest.raises(RuntimeError, match="k_cap 2049 is above the 2048"):
        H.mist_select(scores, boxes, seg, gt_cat, gt_off, K, 2049)


# ---- merge + NMS + label ------------------------------------------------------------------------------------------------
def run_hip(images, dev, iou_thr=0.5):
    from wsovod_amd.layers import hip_ops as H

    scores, boxes, seg, gt_cat, gt_off, max_rows, max_classes = to_device(images, dev)
    o = H.mist_mine_and_label(scores, boxes, seg, gt_cat, gt_off, K, iou_thr, max_rows=max_rows, max_classes=max_classes)
    torch.cuda.synchronize()
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}, seg.cpu().tolist()


def check_against_restatement(images, dev, iou_thr=0.5):
    o, seg = run_hip(images, dev, iou_thr)
    counts = []
    for g, ((b, s, c), (t, lab)) in enumerate(zip(images, U.mine_and_label(*zip(*images), K, iou_thr))):
        n, r0 = len(t["gt_classes"]), int(o["pgt_start"][g])
        assert int(o["pgt_count"][g]) == n, g
        assert torch.equal(o["pgt_classes"][r0:r0 + n], t["gt_classes"]), g
        assert torch.equal(o["pgt_index"][r0:r0 + n].long(), t["index"]), g
        for k in ("boxes", "scores", "weights"):
            assert torch.equal(bits(o["pgt_" + k][r0:r0 + n]), bits(t["gt_" + k])), (g, k)
        sl = slice(seg[g], seg[g + 1])
        assert torch.equal(o["gt_classes"][sl], lab["gt_classes"]), g
        assert torch.equal(o["matched"][sl].long(), lab["matched"]), g
        for k in ("boxes", "scores", "weights"):
            assert torch.equal(bits(o["gt_" + k][sl]), bits(lab["gt_" + k])), (g, k)
        counts.append(n)
    return counts


def grid_image(n_valid, classes, gen, tiny=40):
    """n_valid boxes of ~9 x 9 on a jittered grid of pitch 16 (no two overlap: every candidate survives the NMS) + `tiny`
    boxes of area 16 inside grid boxes (no candidates, but proposals to label); scores above the floor, every class's
    best rows on its own residue of the row index, so that no two classes select the same box."""
    cols = 100
    i = torch.arange(n_valid)
    x0 = (i % cols).float() * 16 + torch.rand(n_valid, generator=gen) * 4
    y0 = (i // cols).float() * 16 + torch.rand(n_valid, generator=gen) * 4
    b = torch.stack([x0, y0, x0 + 9 + torch.rand(n_valid, generator=gen), y0 + 9 + torch.rand(n_valid, generator=gen)], 1)
    inner = b[torch.randint(0, n_valid, (tiny,), generator=gen)]
    inner = torch.stack([inner[:, 0] + 2, inner[:, 1] + 2, inner[:, 0] + 6, inner[:, 1] + 6], 1)
    boxes = torch.cat([b, inner])
    s = 0.06 + 0.3 * torch.rand(len(boxes), K, generator=gen)
    for j, c in enumerate(classes):
        rows = torch.arange(j, n_valid, len(classes))
        s[rows, c] += 0.5
    return boxes, s, torch.tensor(classes)


def tiny_image(r, classes, gen):
    return make_boxes(r, "none", gen), torch.rand(r, K, generator=gen), torch.tensor(classes)


@pytest.mark.parametrize("want,n_valid", [(1, 6), (127, 847), (128, 854), (129, 861), (300, 2001), (1025, 6834)])
def test_target_counts_at_the_chunk_edges(gpu, want, n_valid):
    gen = torch.Generator().manual_seed(want)
    assert check_against_restatement([grid_image(n_valid, [3], gen)], gpu) == [want]


def test_three_images_with_the_dummy_in_the_middle(gpu):
    gen = torch.Generator().manual_seed(3)
    images = [grid_image(430, [0, 7], gen), tiny_image(50, [2, 5, 9], gen), grid_image(667, [1, 4, 19], gen)]
    assert check_against_restatement(images, gpu) == [128, 1, 300]


def test_equal_scores_across_classes_keep_the_flattening_order(gpu):
    gen = torch.Generator().manual_seed(11)
    boxes, _, classes = grid_image(200, [2, 6, 13], gen, tiny=8)
    s = torch.randint(1, 4, (len(boxes), K), generator=gen).float() / 4  # 3 levels, all above the floor
    counts = check_against_restatement([(boxes, s, classes)], gpu)
    assert 30 < counts[0] <= 90  # (classes that pick the same box at equal scores: the order decides which entry survives)


def test_first_maximum_among_equidistant_targets(gpu):
    a, b, p = [0.0, 0.0, 10.0, 10.0], [20.0, 0.0, 30.0, 10.0], [5.0, 0.0, 25.0, 10.0]  # IoU(p, a) = IoU(p, b) = 0.2
    far = [[100.0 + 20 * i, 100.0, 110.0 + 20 * i, 110.0] for i in range(11)]
    boxes = torch.tensor([a, b, p] + far)
    s = torch.full((14, K), 0.2)
    s[0, 4], s[1, 4], s[2, 4] = 0.8, 0.9, 0.1  # k = int(14 * 0.15) = 2: targets b, a in this order
    o, _ = run_hip([(boxes, s, torch.tensor([4]))], gpu, iou_thr=0.1)
    assert o["pgt_index"][:2].tolist() == [1, 0] and int(o["pgt_count"][0]) == 2
    assert int(o["matched"][2]) == 0 and o["gt_boxes"][2].tolist() == b and int(o["gt_classes"][2]) == 4
    check_against_restatement([(boxes, s, torch.tensor([4]))], gpu, iou_thr=0.1)


def test_g24_direct_calls_end_to_end(gpu):
    g = load_golden("g24_mist")
    names = [str(n) for n in g["direct/names"]]
    images = [(g[f"direct/{n}/boxes"], g[f"direct/{n}/scores"], g[f"direct/{n}/classes"]) for n in names]
    o, seg = run_hip(images, gpu)
    for i, n in enumerate(names):
        p = f"direct/{n}/"
        cnt, r0 = int(o["pgt_count"][i]), int(o["pgt_start"][i])
        assert cnt == g[p + "t_classes"].numel(), n
        assert torch.equal(o["pgt_classes"][r0:r0 + cnt], g[p + "t_classes"]), n
        for k in ("boxes", "scores", "weights"):
            assert torch.equal(bits(o["pgt_" + k][r0:r0 + cnt]), bits(g[p + "t_" + k])), (n, k)
        sl = slice(seg[i], seg[i + 1])
        assert torch.equal(o["gt_classes"][sl], g[p + "l_classes"]), n
        for k in ("boxes", "scores", "weights"):
            assert torch.equal(bits(o["gt_" + k][sl]), bits(g[p + "l_" + k])), (n, k)
