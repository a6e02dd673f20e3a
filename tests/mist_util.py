"""Restatement of the reference's MIST mining in plain torch ops: get_pgt_mist (roi_heads.py:910-1040, no SAM) and the
matching of label_and_sample_proposals_wsl (:1722-1825), written from what they compute.  It runs on whatever device its
inputs live on: the CPU for the tests (anchored to the reference by tests/golden/g24_mist.npz), the GPU as the torch-op
formulation tools/mist_step.py times the kernels against.

This tree's tie rule where the reference has none worth copying (torch.topk): equal scores go by ascending proposal index;
among the candidates of an image equal scores go by ascending rank, then ascending class slot (the reference's flattening
order, which a stable sort inside the NMS keeps).  Every float expression is fp32 in the kernels' operation order."""
import torch

TOP_PRO, THRES, NMS_IOU = 0.15, 0.05, 0.2


def mist_k(n, top_pro=TOP_PRO):
    return max(int(n * top_pro), 1)


def _area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def sort_key(x):
    """Order and equality of the kernels' top-k as one int64 per score: every NaN one value above +inf, -0.0 == +0.0."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    key = torch.where(u >= 0x80000000, 0xffffffff - u, u | 0x80000000)
    key = torch.where(x == 0, torch.full_like(key, 0x80000000), key)
    return torch.where(x != x, torch.full_like(key, 0xffffffff), key)


def select(boxes, scores, classes, top_pro=TOP_PRO, thres=THRES):
    """Steps 1-5 for one image: -> per class (kept scores, kept proposal indices), descending, after the floor."""
    valid = torch.nonzero(_area(boxes) > 20).flatten()
    n = int(valid.numel())
    out = []
    for c in classes.tolist():
        if n == 0:
            out.append((scores.new_zeros((0,)), valid.new_zeros((0,))))
            continue
        col = scores[valid, c]
        order = torch.sort(sort_key(col), descending=True, stable=True)[1][:min(mist_k(n, top_pro), n)]
        s = col[order]
        keep = s >= thres
        keep[0] = True
        out.append((s[keep], valid[order][keep]))
    return out


def candidates(boxes, lists, classes):
    """Step 5-6 (input side): the image's class lists as one list by descending score; equal scores by rank, then slot."""
    s = torch.cat([l[0] for l in lists])
    idx = torch.cat([l[1] for l in lists])
    dev = s.device
    rank = torch.cat([torch.arange(len(l[0]), device=dev) for l in lists])
    slot = torch.cat([torch.full((len(l[0]),), j, device=dev, dtype=torch.int64) for j, l in enumerate(lists)])
    flat = rank * max(len(lists), 1) + slot                     # position in the reference's rank-major flattening
    order = torch.sort(flat, stable=True)[1]
    order = order[torch.sort(sort_key(s[order]), descending=True, stable=True)[1]]
    return boxes[idx[order]], s[order], classes[slot[order]], idx[order]


def nms(boxes, thr):
    """Greedy NMS over boxes already in visiting order: kept positions, ascending."""
    n = boxes.size(0)
    if n == 0:
        return torch.zeros((0,), dtype=torch.int64, device=boxes.device)
    area = _area(boxes)
    w = (torch.min(boxes[:, None, 2], boxes[None, :, 2]) - torch.max(boxes[:, None, 0], boxes[None, :, 0])).clamp(min=0)
    h = (torch.min(boxes[:, None, 3], boxes[None, :, 3]) - torch.max(boxes[:, None, 1], boxes[None, :, 1])).clamp(min=0)
    inter = w * h
    over = (inter / (area[:, None] + area[None, :] - inter) > thr).cpu()
    removed = torch.zeros((n,), dtype=torch.bool)
    kept = []
    for i in range(n):
        if not removed[i]:
            kept.append(i)
            removed |= over[i]
    return torch.tensor(kept, dtype=torch.int64, device=boxes.device)


def mine(boxes, scores, classes, top_pro=TOP_PRO, thres=THRES, nms_iou=NMS_IOU):
    """get_pgt_mist for one image -> dict(gt_boxes, gt_classes, gt_scores, gt_weights, index)."""
    lists = select(boxes, scores, classes, top_pro, thres)
    if sum(len(l[0]) for l in lists) == 0:  # no valid box: the dummy target of get_pgt_top_k's fallback (:1181-1207)
        return dict(gt_boxes=boxes.new_tensor([[-10000.0, -10000.0, 10000.0, 10000.0]]),
                    gt_classes=classes.new_zeros((1,)), gt_scores=scores.new_ones((1,)), gt_weights=scores.new_ones((1,)),
                    index=classes.new_full((1,), -1))
    b, s, c, idx = candidates(boxes, lists, classes)
    keep = nms(b, nms_iou)
    return dict(gt_boxes=b[keep], gt_classes=c[keep], gt_scores=s[keep], gt_weights=s[keep], index=idx[keep])


def label(boxes, t, K, iou_thr):
    """label_and_sample_proposals_wsl's matching for one image -> dict(gt_classes, gt_boxes, gt_scores, gt_weights, matched)."""
    tb = t["gt_boxes"]
    w = (torch.min(boxes[:, None, 2], tb[None, :, 2]) - torch.max(boxes[:, None, 0], tb[None, :, 0])).clamp(min=0)
    h = (torch.min(boxes[:, None, 3], tb[None, :, 3]) - torch.max(boxes[:, None, 1], tb[None, :, 1])).clamp(min=0)
    inter = w * h
    iou = torch.where(inter > 0, inter / (_area(tb)[None, :] + _area(boxes)[:, None] - inter), torch.zeros_like(inter))
    best = iou.max(dim=1)[0]
    j = (iou == best[:, None]).to(torch.int64).argmax(dim=1)  # the first maximum
    cls = torch.where(best >= iou_thr, t["gt_classes"][j], torch.full_like(j, K))
    return dict(gt_classes=cls, gt_boxes=tb[j], gt_scores=t["gt_scores"][j], gt_weights=t["gt_weights"][j], matched=j)


def mine_and_label(boxes_list, scores_list, classes_list, K, iou_thr, proposal_boxes=None, **kw):
    """Per image: (targets, labels).  proposal_boxes: the boxes that are labelled, where they are not the mined ones (the
    reference labels the proposals, and mines a later head's targets from the previous head's predictions)."""
    out = []
    for i, (b, s, c) in enumerate(zip(boxes_list, scores_list, classes_list)):
        t = mine(b, s, c, **kw)
        out.append((t, label(b if proposal_boxes is None else proposal_boxes[i], t, K, iou_thr)))
    return out
