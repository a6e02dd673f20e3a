"""-m gpu: `hip_ops.rpn_label_anchors` (csrc/proposals.hip: rpn_match_kernel + rpn_label_kernel) called directly, against the
oracle's Matcher restatement (tests/functions_ref.py: label_anchors).

Integer box coordinates: every area and intersection is an exact integer, every IoU one correctly rounded fp32 quotient on
both sides, so labels and best IoUs are compared with torch.equal.  best_gt is compared wherever ONE box attains the anchor's
best IoU; at a tie the kernel keeps the first box of the image (`iou > best`), torch's max may name another."""
import pytest
import torch

from tests import functions_ref as FR

pytestmark = pytest.mark.gpu

LO, HI = 0.25, 0.5

# Hand-made anchors and boxes (tests/test_functions_ref.py checks the same geometry against brute force):
#   box 0 (0,0,16,32):     anchor 0 IoU 1; anchor 1 IoU 256/512 = thr_hi exactly and NOT the box's best -> positive by `>=` alone;
#                          anchor 2 IoU 128/512 = thr_lo exactly -> ignored (-1), not background
#   box 1 (100..132)^2:    anchors 3 and 4 tie for its best at 1/16 < thr_lo -> both positive by the low-quality rule
#   box 2 (200,0,232,7):   anchor 7 IoU 1; anchor 5's own best (0.4375, between the thresholds)
#   box 3 (216,0,248,16):  anchors 5 and 6 tie for its best at 1/3: anchor 5 turns positive though its own best is box 2
#   box 4 (1000..1010)^2:  overlaps nothing: its best IoU is 0, which EVERY anchor attains -> the whole image positive
HAND_ANCHORS = [[0, 0, 16, 32], [0, 0, 16, 16], [0, 0, 8, 16], [100, 100, 108, 108], [124, 124, 132, 132],
                [200, 0, 232, 16], [232, 0, 264, 16], [200, 0, 232, 7]]
BOX = [[0, 0, 16, 32], [100, 100, 132, 132], [200, 0, 232, 7], [216, 0, 248, 16], [1000, 1000, 1010, 1010],
       [8, 304, 40, 328]]  # (box 5 lies on the filler grid)


def _anchors(A):
    """16 x 16 filler anchors on a stride-8 grid below y = 304 (far from boxes 0 - 4), the hand-made ones spread over the index
    range, first and last index included: the last workgroup's ragged tail holds one."""
    i = torch.arange(A)
    x0, y0 = 8.0 * (i % 40), 304.0 + 8.0 * (i // 40)
    a = torch.stack([x0, y0, x0 + 16, y0 + 16], 1)
    n = min(A, len(HAND_ANCHORS))
    at = torch.linspace(0, A - 1, n).round().long() if n > 1 else torch.zeros(1, dtype=torch.long)
    if n == len(HAND_ANCHORS):
        a[at] = torch.tensor(HAND_ANCHORS, dtype=torch.float32)
    else:
        a[at] = torch.tensor(HAND_ANCHORS[:n], dtype=torch.float32)
    return a, at


def _run(gpu, anchors, boxes, counts, lo=LO, hi=HI):
    from wsovod_amd.layers import hip_ops as H

    gt = torch.tensor(boxes, dtype=torch.float32).view(-1, 4)
    count = torch.tensor(counts, dtype=torch.int32)
    start = (torch.cumsum(count, 0) - count).to(torch.int32)
    assert int(count.sum()) == gt.size(0)
    lab, best_gt, best_iou = H.rpn_label_anchors(anchors.to(gpu), gt.to(gpu), start.to(gpu), count.to(gpu), lo, hi)
    ref = FR.label_anchors(anchors, gt, start, count, lo, hi)
    lab, best_gt, best_iou = lab.cpu(), best_gt.cpu(), best_iou.cpu()
    assert lab.dtype == torch.int8 and lab.shape == (len(counts), anchors.size(0))
    assert torch.equal(lab, ref[0])
    has = (count > 0).view(-1, 1).expand_as(lab)
    assert torch.equal(best_iou[has], ref[2][has])
    assert bool((best_gt[~has] == -1).all()) and bool((lab[~has] == 0).all())
    assert torch.equal(best_gt[ref[3]], ref[1][ref[3]])
    inside = (best_gt[has] >= start.view(-1, 1).expand_as(lab)[has]) & \
             (best_gt[has] < (start + count).view(-1, 1).expand_as(lab)[has])
    assert bool(inside.all())  # a tie still names a box of the anchor's own image
    return lab, best_gt, best_iou, ref


@pytest.mark.parametrize("A", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("counts", [[2, 0, 3], [0, 0, 1]], ids=["2-0-3", "0-0-1"])
def test_thresholds_ties_and_empty_images(gpu, A, counts):
    """An image without boxes between two that have some; IoU exactly on thr_lo and on thr_hi; the low-quality rule on ties;
    A below, on and above the workgroup size."""
    anchors, at = _anchors(A)
    boxes = [BOX[0], BOX[1], BOX[2], BOX[3], BOX[5]] if counts == [2, 0, 3] else [BOX[0]]
    lab, best_gt, best_iou, _ = _run(gpu, anchors, boxes, counts)
    if A >= len(HAND_ANCHORS):
        a = at.tolist()
        if counts == [2, 0, 3]:
            assert [float(best_iou[0, a[i]]) for i in (0, 1, 2)] == [1.0, HI, LO]
            assert [int(lab[0, a[i]]) for i in (0, 1, 2, 3, 4)] == [1, 1, -1, 1, 1]
            assert float(best_iou[0, a[3]]) == float(best_iou[0, a[4]]) == 0.0625
            assert int(best_gt[2, a[5]]) == 2 and float(best_iou[2, a[5]]) == 0.4375 and int(lab[2, a[5]]) == 1
            assert int(lab[2, a[6]]) == 1 and int(lab[2, a[0]]) == 0
            assert int((lab[0] == 0).sum()) >= A - len(HAND_ANCHORS)  # the filler is background for image 0
        else:
            assert [int(lab[2, a[i]]) for i in (0, 1, 2, 3)] == [1, 1, -1, 0]


def test_no_boxes_at_all(gpu):
    anchors, _ = _anchors(300)
    lab, best_gt, _, _ = _run(gpu, anchors, [], [0, 0])
    assert bool((lab == 0).all()) and bool((best_gt == -1).all())


def test_a_box_that_overlaps_no_anchor(gpu):
    """Matcher's low-quality rule compares with the box's best IoU, 0 here: every anchor of THAT image is positive (the
    restatement and detectron2 agree); the neighbouring image, whose rows lie next to it in gt_boxes, is untouched."""
    anchors, at = _anchors(257)
    lab, _, _, _ = _run(gpu, anchors, [BOX[0], BOX[4], BOX[0], BOX[1]], [2, 2])
    assert bool((lab[0] == 1).all())
    assert int(lab[1, at[2]]) == -1 and int((lab[1] == 0).sum()) >= 257 - len(HAND_ANCHORS)


def test_best_iou_cells_do_not_leak_between_images(gpu):
    """Adjacent rows of gt_boxes, the same box in both images, but image 1 sees it next to a box that anchor 5 overlaps more:
    whatever one image's pass writes for its rows must not decide the other's low-quality matches."""
    anchors, at = _anchors(600)
    lab, _, _, _ = _run(gpu, anchors, [BOX[3], BOX[2], BOX[3], BOX[1]], [1, 3])
    assert int(lab[0, at[5]]) == 1 and int(lab[0, at[6]]) == 1 and int(lab[0, at[3]]) == 0
    assert int(lab[1, at[3]]) == 1 and int(lab[1, at[4]]) == 1


def test_seeded_random_case(gpu):
    """A = 600, up to 5 boxes per image, coordinates on a grid of 8: ties and exact thresholds come by themselves."""
    g = torch.Generator().manual_seed(17)
    A = 600
    xy = torch.randint(0, 40, (A, 2), generator=g) * 8.0
    wh = torch.randint(1, 9, (A, 2), generator=g) * 8.0
    anchors = torch.cat([xy, xy + wh], 1)
    counts = [5, 0, 3, 1, 4]
    n = sum(counts)
    bxy = torch.randint(0, 40, (n, 2), generator=g) * 8.0
    bwh = torch.randint(1, 9, (n, 2), generator=g) * 8.0
    boxes = torch.cat([bxy, bxy + bwh], 1)
    lab, _, best_iou, ref = _run(gpu, anchors, boxes.tolist(), counts)
    assert not bool(ref[3].all())                                       # ties for an anchor's best occur
    assert bool((best_iou == LO).any()) or bool((best_iou == HI).any())  # so does an IoU exactly on a threshold
    assert {int(v) for v in lab.unique()} == {-1, 0, 1}
