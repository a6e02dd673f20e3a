"""fp64 restatements of what wsovod_amd/layers/functions.py hands to autograd, shared by tests/test_functions_ref.py (CPU)
and the three GPU files test_gpu_pooler_autograd.py, test_gpu_head_autograd.py and test_gpu_rpn_label_anchors.py.  Plain torch
on the CPU; the HIP library is never touched here.

Tolerances are |got - ref| <= c * u * B: B is the reference evaluated over magnitudes (the sum of the magnitudes of all terms
of an element), u the unit of the number format, c a count of roundings read off the code path and written beside each use
(the convention of tests/conv_backward_ref.py).
"""
import json
import os

import torch
import torch.nn.functional as F

from oracle import wsovod_ref as R

U32, UBF, UX2 = 2.0 ** -24, 2.0 ** -9, 2.0 ** -17
RATIOS = {}  # test id -> observed max(err / (u * B)); written by the GPU files' module fixtures


def record(key, err, bound_per_c):
    """Observed max(err / (u * B)) over the elements with B > 0 (the others are asserted exactly)."""
    ok = bound_per_c > 0
    worst = float((err[ok] / bound_per_c[ok]).max()) if bool(ok.any()) else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    return worst


def write_ratios():
    """WSOVOD_FUNCTIONS_AUTOGRAD_BOUNDS=<file>: merge the ratios observed so far into that JSON file."""
    path = os.environ.get("WSOVOD_FUNCTIONS_AUTOGRAD_BOUNDS")
    if path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        old.update(RATIOS)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def bf16_ulp(x):
    """One unit in the last place of the bf16 neighbours of |x| (8 significant bits); 0 at 0."""
    x = x.abs().double()
    e = torch.floor(torch.log2(x.clamp_min(2.0 ** -126)))
    return torch.where(x > 0, torch.exp2(e - 7), torch.zeros_like(x))


# ---- max pools: the gradient through a GIVEN argmax -------------------------------------------------------------------
def pool_scatter(grad_out, argmax, batch_index, scale, shape):
    """grad_in[n, c, argmax] += grad_out * scale[row] for every output element with argmax >= 0, in fp64.
    grad_out (Q, C, ph, pw); argmax int32, -1 = empty bin; batch_index (Q) image of every row; scale (Q) or None.
    -> (grad_in (N, C, H, W), B: the same scatter over |grad_out * scale|, n_max: most contributions any cell receives)."""
    N, C, H, W = shape
    g = grad_out.detach().double().cpu()
    if scale is not None:
        g = g * scale.detach().double().cpu().view(-1, 1, 1, 1)
    am = argmax.detach().cpu().long()
    ok = am >= 0
    assert bool((am[ok] < H * W).all())
    n = batch_index.detach().cpu().long().view(-1, 1, 1, 1).expand_as(am)
    c = torch.arange(C).view(1, -1, 1, 1).expand_as(am)
    flat = ((n * C + c) * (H * W) + am)[ok]
    out = torch.zeros(N * C * H * W, dtype=torch.float64)
    mag = torch.zeros_like(out)
    cnt = torch.zeros_like(out)
    out.index_add_(0, flat, g[ok])
    mag.index_add_(0, flat, g[ok].abs())
    cnt.index_add_(0, flat, torch.ones_like(g[ok]))
    return out.view(shape), mag.view(shape), int(cnt.max())


def loop_pool_backward(grad_out, argmax, rois, scale, shape):
    """The 3-output pool: row q of the (3R, C, ph, pw) output is roi q mod R, so its image and its scale are those."""
    s3 = None if scale is None else scale.detach().cpu().repeat(3)
    return pool_scatter(grad_out, argmax, rois.detach().cpu()[:, 0].repeat(3), s3, shape)


def roi_pool_backward(grad_out, argmax, rois, scale, shape):
    return pool_scatter(grad_out, argmax, rois.detach().cpu()[:, 0], scale, shape)


# ---- RoIAlign: torchvision roi_align / `decode_align` + `bilinear_setup` of csrc/roi_pool.hip ---------------------------
class _AlignAxis:
    """One axis of one roi: the (bins, cells) matrix of summed bilinear weights of the valid samples, and the same with every
    weight replaced by 1 on the two cells a sample touches and on their two outer neighbours (`reach`)."""

    def __init__(self, start, length, bins, grid, size):
        bin_sz = length / bins
        p = torch.arange(bins, dtype=torch.float64).view(-1, 1)
        i = torch.arange(grid, dtype=torch.float64).view(1, -1)
        y = start + p * bin_sz + (i + 0.5) * bin_sz / grid  # (bins, grid)
        self.valid = ~((y < -1.0) | (y > size))
        # distance of any sample to the two discontinuities of `valid` (a sample there may flip between the kernel's fp32 and
        # this fp64 and takes its whole weight with it: the cases keep clear of them, test_functions_ref asserts it)
        self.margin = float(torch.minimum((y + 1.0).abs(), (y - size).abs()).min()) if y.numel() else float("inf")
        y = y.clamp_min(0.0)
        lo = y.floor().long()
        top = lo >= size - 1
        lo = torch.where(top, torch.full_like(lo, size - 1), lo)
        hi = torch.where(top, lo, lo + 1)
        y = torch.where(top, lo.double(), y)
        ly = y - lo.double()
        hy = 1.0 - ly
        v = self.valid.double()
        self.w = torch.zeros(bins, size, dtype=torch.float64)
        self.w.scatter_add_(1, lo, hy * v)
        self.w.scatter_add_(1, hi, ly * v)
        self.reach = torch.zeros(bins, size, dtype=torch.float64)
        for idx in (lo - 1, lo, hi, hi + 1):
            self.reach.scatter_add_(1, idx.clamp(0, size - 1), v)


def _align_rois(rois, spatial_scale, output_size, sampling_ratio, aligned, H, W):
    """Per roi (image, inv_count, y axis, x axis, delta).  The box is decoded in fp32 as the kernel decodes it (a product with
    a power of two and a subtraction of 0.5: exact for the cases' quarter-pixel coordinates, FMA or not) so that the sample
    grid ceil(size / bins) is the kernel's; everything behind it is fp64.  delta bounds |kernel's fp32 sample coordinate - the
    exact one|: at most 8 roundings (the bin size, its products with the bin and sample index, the quotient by the grid, two
    sums; a fused multiply-add only removes some) of values no larger than the box's far edge."""
    ph, pw = output_size
    rois = rois.detach().cpu().float()
    off = 0.5 if aligned else 0.0
    out = []
    for r in range(rois.size(0)):
        b = rois[r, 1:] * torch.tensor(spatial_scale, dtype=torch.float32) - off
        rw, rh = b[2] - b[0], b[3] - b[1]
        if not aligned:
            rw, rh = rw.clamp_min(1.0), rh.clamp_min(1.0)
        gh = sampling_ratio if sampling_ratio > 0 else int(torch.ceil(rh / ph))
        gw = sampling_ratio if sampling_ratio > 0 else int(torch.ceil(rw / pw))
        inv = 1.0 / max(gh * gw, 1)
        ya = _AlignAxis(float(b[1]), float(rh), ph, max(gh, 0), H)
        xa = _AlignAxis(float(b[0]), float(rw), pw, max(gw, 0), W)
        delta = 8 * U32 * max(1.0, float(b.abs().max()), float(b[0] + rw), float(b[1] + rh))
        out.append((int(rois[r, 0]), inv, ya, xa, delta))
    return out


def roi_align(feat, rois, spatial_scale, output_size, sampling_ratio, aligned):
    """(R, C, ph, pw) fp64, differentiable in `feat` (N, C, H, W) fp64.  The bilinear weights of a sample are a product of a
    row and a column weight and its validity a product too, so a roi's output is Wy @ feat[n] @ Wx^T / count."""
    N, C, H, W = feat.shape
    out = []
    for n, inv, ya, xa, _ in _align_rois(rois, spatial_scale, output_size, sampling_ratio, aligned, H, W):
        out.append(torch.einsum("ph,chw,qw->cpq", ya.w, feat[n], xa.w) * inv)
    return torch.stack(out) if out else feat.new_zeros((0, C) + tuple(output_size))


def roi_align_margin(rois, spatial_scale, output_size, sampling_ratio, aligned, H, W):
    return min(min(ya.margin, xa.margin) for _, _, ya, xa, _ in
               _align_rois(rois, spatial_scale, output_size, sampling_ratio, aligned, H, W) if ya.valid.any() and xa.valid.any())


def roi_align_backward(grad_out, rois, scale, spatial_scale, sampling_ratio, aligned, shape):
    """-> (grad_in fp64 by autograd through `roi_align`, B over magnitudes, D, n_max).
    D[cell] = sum over the samples that can reach the cell (their four cells and the ring around them, should the fp32
    coordinate fall on the other side of a cell border) of delta * |grad_out * scale| / count: a weight is a product of two
    numbers in [0, 1] that each move by at most delta, so it moves by at most 2 delta + delta^2 <= 3 delta.
    n_max: the most atomic adds one cell can receive (counted over the same reach)."""
    N, C, H, W = shape
    g = grad_out.detach().double().cpu()
    if scale is not None:
        g = g * scale.detach().double().cpu().view(-1, 1, 1, 1)
    ph, pw = g.shape[2:]
    feat = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    out = roi_align(feat, rois, spatial_scale, (ph, pw), sampling_ratio, aligned)
    (gi,) = torch.autograd.grad(out, feat, g, retain_graph=True)
    (B,) = torch.autograd.grad(out, feat, g.abs())  # (every weight is >= 0)
    D = torch.zeros(shape, dtype=torch.float64)
    cnt = torch.zeros((N, H, W), dtype=torch.float64)
    for r, (n, inv, ya, xa, delta) in enumerate(_align_rois(rois, spatial_scale, (ph, pw), sampling_ratio, aligned, H, W)):
        D[n] += torch.einsum("ph,cpq,qw->chw", ya.reach, g[r].abs(), xa.reach) * (inv * delta)
        cnt[n] += torch.einsum("ph,qw->hw", ya.reach, xa.reach)
    return gi, B, D, int(cnt.max())


# ---- the cosine classifier ------------------------------------------------------------------------------------------
def cosine_logits(z, wn, temperature, normalize, bias):
    """T * F.normalize(z, dim=1, eps=1e-12) @ wn.T + bias (open_vocabulary_classifier.py:91-104), or without normalize."""
    x = temperature * F.normalize(z, p=2, dim=1, eps=1e-12) if normalize else z
    y = x @ wn.t()
    return y if bias is None else y + bias


def cosine_reference(z, wn, temperature, normalize, bias, dl):
    """fp64 values and autograd gradients, and their magnitudes.
    -> dict(logits, dz, db or None, B_logits, B_dz, B_db).  Magnitudes: logits s |z| |wn|^T + |bias| with s = T / max(||z||, eps);
    dz = s (v - z (z . v) / ||z||^2) with v = dl @ wn: s (|v| + |z| (|z| . |v|) / ||z||^2), |v| = |dl| @ |wn| (clamped rows and
    normalize off: s |v|)."""
    z64 = z.detach().double().cpu().requires_grad_(True)
    w64 = wn.detach().double().cpu()
    b64 = None if bias is None else bias.detach().double().cpu().requires_grad_(True)
    dl64 = dl.detach().double().cpu()
    y = cosine_logits(z64, w64, temperature, normalize, b64)
    grads = torch.autograd.grad(y, [z64] + ([b64] if b64 is not None else []), dl64)
    with torch.no_grad():
        za = z64.abs()
        nrm = z64.norm(dim=1, keepdim=True)
        s = temperature / nrm.clamp_min(1e-12) if normalize else torch.ones_like(nrm)
        B_logits = s * (za @ w64.abs().t()) + (0 if b64 is None else b64.abs())
        v = dl64.abs() @ w64.abs()
        proj = za * (za * v).sum(1, keepdim=True) / (nrm * nrm).clamp_min(1e-300)
        B_dz = s * (v + (proj if normalize else 0) * (nrm > 1e-12))
    return dict(logits=y.detach(), dz=grads[0], db=grads[1] if b64 is not None else None, B_logits=B_logits, B_dz=B_dz,
                B_db=dl64.abs().sum(0))


def c_cosine_forward(D, u, operand_roundings=0.0):
    """`_CosineLogits.forward`: the D-term dot in fp32 (acc) + the row scale T / max(sqrt(sum z^2), eps) -- a D-term sum of
    squares (D), its root, the quotient (1 each), counted once more for the square it is the root of -- + the two epilogue
    stages (times row_scale, plus bias) + what the operands lose when they are encoded (bf16x2: see the caller)."""
    return operand_roundings + (2.0 * D + (D + 3) + 2) * U32 / u


def c_cosine_backward(D, K1p, u, roundings):
    """`_CosineLogits._backward`: `roundings` units for the operands rounded to the contraction's format + the K1p-term dot
    v = dA @ wnT (acc) + row_l2norm_backward: the D-term dots z . v (acc) and z . z (D), the quotient, the product with z, the
    difference, s (D + 3 as in the forward) and the product with it (4 single operations)."""
    return roundings + (2.0 * K1p + 2.0 * D + D + (D + 3) + 4) * U32 / u


# ---- the data-aware features head -------------------------------------------------------------------------------------
def data_aware_reference(gap, W1, b1, W2, b2, E, ddaf):
    """fp64 autograd through tanh(relu(gap W1^T + b1) W2^T + b2) @ E (oracle/wsovod_ref.py: data_aware_forward) and the
    magnitudes of its five gradients, as tests/test_gpu_elementwise.py::test_data_aware_backward derives them (the fp32
    forward's rounding of h1 and h2 reaches the gradients through tanh's slope).  -> (daf, grads, mags)."""
    gap, W1, b1, W2, b2, E, ddaf = [t.detach().double().cpu() for t in (gap, W1, b1, W2, b2, E, ddaf)]
    for t in (W1, b1, W2, b2, E):
        t.requires_grad_(True)
    h1 = torch.relu(gap @ W1.t() + b1)
    h2 = torch.tanh(h1 @ W2.t() + b2)
    daf = h2 @ E
    g = torch.autograd.grad(daf, [W1, b1, W2, b2, E], ddaf)
    grads = dict(zip(("dW1", "db1", "dW2", "db2", "dE"), g))
    with torch.no_grad():
        live = (h1 > 0).double()
        m_h1 = (gap.abs() @ W1.abs().t() + b1.abs()) * live
        m_pre2 = m_h1 @ W2.abs().t() + b2.abs()
        sens = 1 - h2 * h2
        m_h2 = h2.abs() + sens * m_pre2
        m_dpre2 = (ddaf.abs() @ E.abs().t()) * ((1 + h2 * h2) + 2 * h2.abs() * sens * m_pre2)
        m_dh1 = (m_dpre2 @ W2.abs()) * live
        mags = dict(dE=m_h2.t() @ ddaf.abs(), dW2=m_dpre2.t() @ m_h1, db2=m_dpre2.sum(0), dW1=m_dh1.t() @ gap.abs(),
                    db1=m_dh1.sum(0), daf=m_h2 @ E.abs())
    return daf.detach(), grads, mags


def data_aware_case(N, C, Hd, P, Fd, g):
    """The inputs of test_data_aware_backward: gap >= 0; every third hidden unit dead for every image (negative weights and
    bias), the others alive and far from the ReLU's kink, so fp32 and fp64 agree on every mask; prototype 0 saturates tanh at
    +1, prototype 1 at -1, the others stay in its bend."""
    gap = torch.rand(N, C, generator=g)
    W1 = torch.rand(Hd, C, generator=g) * (2.0 / C) + 1e-3
    b1 = torch.rand(Hd, generator=g) * 0.1 + 0.05
    dead = torch.arange(Hd) % 3 == 1
    W1[dead], b1[dead] = -W1[dead], -b1[dead]
    W2 = torch.randn(P, Hd, generator=g) * (1.0 / Hd ** 0.5)
    b2 = torch.randn(P, generator=g) * 0.3
    b2[0], b2[1] = 40.0, -40.0
    return gap, W1, b1, W2, b2, torch.randn(P, Fd, generator=g), torch.randn(N, Fd, generator=g)


def data_aware_terms(N, C, Hd, P, Fd):
    """The longest reduction chain behind every gradient (test_data_aware_backward: `terms`), + 8 single operations."""
    chain = dict(dE=N, dW2=Fd + N, db2=Fd + N, dW1=Fd + P + N, db1=Fd + P + N)
    return {k: v + C + Hd + 8 for k, v in chain.items()}


# ---- small ones -------------------------------------------------------------------------------------------------------
def gap(x):
    return x.mean((1, 2))


def add_group_rows(x, add, row_group):
    return x + add[row_group.long()]


# ---- RPN anchor labels ------------------------------------------------------------------------------------------------
def label_anchors(anchors, gt_boxes, gt_start, gt_count, thr_lo, thr_hi):
    """fp32 on the CPU, per image: the oracle's restatement behind R.rpn_losses -- `pairwise_iou` in detectron2's operation
    order, Matcher([lo, hi], [0, -1, 1], allow_low_quality_matches=True).  An image without boxes: labels 0, best_gt -1.
    -> (labels (B, A) int8, best_gt (B, A) int32 row of gt_boxes, best_iou (B, A) fp32 (-1 without boxes),
        unique (B, A) bool: exactly one box of the image attains the anchor's best IoU)."""
    anchors, gt_boxes = anchors.detach().cpu().float(), gt_boxes.detach().cpu().float()
    A = anchors.size(0)
    labels, best_gt, best_iou, unique = [], [], [], []
    for s, n in zip(gt_start.tolist(), gt_count.tolist()):
        if n == 0:
            labels.append(torch.zeros(A, dtype=torch.int8))
            best_gt.append(torch.full((A,), -1, dtype=torch.int32))
            best_iou.append(torch.full((A,), -1.0))
            unique.append(torch.ones(A, dtype=torch.bool))
            continue
        gt = gt_boxes[s:s + n]
        matches, lab = R.rpn_match_anchors(anchors, gt, thresholds=(thr_lo, thr_hi))
        iou = R.pairwise_iou(gt, anchors)
        vals = iou.max(dim=0).values
        labels.append(lab.to(torch.int8))
        best_gt.append((matches + s).to(torch.int32))
        best_iou.append(vals)
        unique.append((iou == vals[None]).sum(0) == 1)
    return torch.stack(labels), torch.stack(best_gt), torch.stack(best_iou), torch.stack(unique)


def label_anchors_brute(anchors, gt_boxes, gt_start, gt_count, thr_lo, thr_hi):
    """The same by a double loop over Python floats rounded to fp32 after every operation (small cases only)."""
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))
    a, g = anchors.tolist(), gt_boxes.tolist()
    labels, best = [], []

    def iou(p, q):
        w = max(f(min(p[2], q[2]) - max(p[0], q[0])), 0.0)
        h = max(f(min(p[3], q[3]) - max(p[1], q[1])), 0.0)
        inter = f(w * h)
        ap, aq = f(f(p[2] - p[0]) * f(p[3] - p[1])), f(f(q[2] - q[0]) * f(q[3] - q[1]))
        return f(inter / f(f(ap + aq) - inter)) if inter > 0 else 0.0

    for s, n in zip(gt_start.tolist(), gt_count.tolist()):
        m = [[iou(g[s + j], a[i]) for i in range(len(a))] for j in range(n)]
        lab, bi = [], []
        for i in range(len(a)):
            if n == 0:
                lab.append(0)
                bi.append(-1.0)
                continue
            v = max(m[j][i] for j in range(n))
            l = 1 if v >= thr_hi else (-1 if v >= thr_lo else 0)
            for j in range(n):
                if m[j][i] == max(m[j]):  # the low-quality rule: this anchor attains box j's best IoU
                    l = 1
            lab.append(l)
            bi.append(v)
        labels.append(lab)
        best.append(bi)
    return torch.tensor(labels, dtype=torch.int8).view(len(labels), len(a)), torch.tensor(best, dtype=torch.float32).view(len(best), len(a))


# ---- inputs shared by the CPU and GPU pooler tests -------------------------------------------------------------------------
MAP = (2, 20, 26)       # (images, H, W) of the feature map; spatial_scale 1/8: images of 160 x 208 pixels
SCALE = 0.125
POOL_SIZES = ((7, 7), (3, 5))


def pooler_rois(seed=5):
    """R = 24 rois [image, x0, y0, x1, y1] on a quarter-pixel grid: two identical ones (atomics on the same cells), the
    whole map, one cell wide, wholly outside the map (empty bins, argmax -1; every RoIAlign sample invalid and far from the
    border), the rest seeded; the image index is not sorted."""
    g = torch.Generator().manual_seed(seed)
    R = 24
    x0 = torch.randint(0, 4 * 150, (R,), generator=g) / 4.0
    y0 = torch.randint(0, 4 * 110, (R,), generator=g) / 4.0
    w = torch.randint(4 * 9, 4 * 120, (R,), generator=g) / 4.0
    h = torch.randint(4 * 9, 4 * 90, (R,), generator=g) / 4.0
    rois = torch.stack([torch.randint(0, 2, (R,), generator=g).float(), x0, y0, (x0 + w).clamp(max=200.0),
                        (y0 + h).clamp(max=152.0)], 1)
    rois[0] = torch.tensor([1.0, 16.0, 24.0, 120.0, 100.0])
    rois[1] = rois[0]                                           # identical
    rois[2] = torch.tensor([0.0, 0.0, 0.0, 207.0, 159.0])       # the whole map
    rois[3] = torch.tensor([1.0, 40.0, 16.0, 43.0, 120.0])      # one cell wide
    rois[4] = torch.tensor([0.0, 300.0, 300.0, 400.0, 380.0])   # wholly outside
    rois[5, 0], rois[6, 0] = 1.0, 0.0
    return rois


def pooler_scale(R=24):
    """Distinct entries in [1, 2): objectness + 1 (roi_heads.py); repeat and repeat_interleave of it differ everywhere."""
    return 1.0 + (torch.arange(R, dtype=torch.float32) * 7 % R) / R + 1.0 / 64


def pooler_map(C, dtype, seed, nonneg=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(MAP[0], C, MAP[1], MAP[2], generator=g)
    return (torch.relu(x) if nonneg else x).to(dtype)
