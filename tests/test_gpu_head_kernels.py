"""GPU parity of the individual head kernels against the oracle / plain torch fp32 on the CPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle import wsovod_ref as R

pytestmark = pytest.mark.gpu


def _seg(nums, dev):
    o = [0]
    for n in nums:
        o.append(o[-1] + n)
    return torch.tensor(o, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("nums,K", [([64, 57, 1, 30], 20), ([512], 80), ([300, 212], 1203), ([5], 2)])
def test_mil_forward_backward(gpu, nums, K):
    from wsovod_amd.layers import functions as Fn

    torch.manual_seed(0)
    M = sum(nums)
    logits = torch.randn(M, 2 * K) * 3
    y = (torch.rand(len(nums), K) < 0.1).float()
    lc = logits.clone().requires_grad_(True)
    scores_ref = torch.cat([F.softmax(c, 1) * F.softmax(d, 0)
                            for c, d in zip(lc[:, :K].split(nums), lc[:, K:].split(nums))])
    loss_ref = R.mining_loss(scores_ref, nums, y)
    loss_ref.backward()
    lg = logits.clone().to(gpu).requires_grad_(True)
    seg = _seg(nums, gpu)
    scores = Fn.mil_scores(lg, seg, K)
    loss, img = Fn.image_bce(scores, seg, y.to(gpu), float(len(nums) * K))
    loss.backward()
    torch.testing.assert_close(scores.detach().cpu(), scores_ref.detach(), rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(loss.detach().cpu(), loss_ref.detach(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(img.cpu(), R.predict_probs_img(scores_ref.detach(), nums), rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(lg.grad.cpu(), lc.grad, rtol=2e-3, atol=1e-7)


def test_mil_k1_special_case(gpu):
    from tests.helpers import seeded_sd
    from wsovod_amd.modeling.fast_rcnn_open_vocabulary import ObjectMiningOutputLayers
    from wsovod_amd.modeling.box_regression import Box2BoxTransform

    torch.manual_seed(1)
    layer = ObjectMiningOutputLayers(4096, box2box_transform=Box2BoxTransform((10., 10., 5., 5.)), num_classes=1).to(gpu)
    x = torch.randn(40, 4096)
    sd = {"p.cls.weight": layer.cls.weight.detach().cpu(), "p.cls.bias": layer.cls.bias.detach().cpu(),
          "p.det.weight": layer.det.weight.detach().cpu(), "p.det.bias": layer.det.bias.detach().cpu()}
    ref = R.mining_forward(sd, x, [25, 15], prefix="p.")

    class P:  # only len() is used
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

    scores, _ = layer(x.to(gpu), [P(25), P(15)])
    torch.testing.assert_close(scores.detach().cpu(), ref, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("K1,weighted", [(21, True), (81, True), (1201, True), (21, False)])
def test_weighted_cross_entropy(gpu, K1, weighted):
    from wsovod_amd.layers import functions as Fn

    torch.manual_seed(2)
    M = 333
    logits = torch.randn(M, K1) * 4
    gt = torch.randint(-1, K1, (M,))
    gt[:5] = -1
    w = torch.rand(M)
    w[7] = 0.0
    lc = logits.clone().requires_grad_(True)
    ref_c, _ = R.refinement_losses(lc, torch.zeros(M, 4), gt, w, torch.tensor([[0., 0., 10., 10.]]).repeat(M, 1),
                                   torch.tensor([[0., 0., 10., 10.]]).repeat(M, 1), K1 - 1,
                                   cross_entropy_weighted=weighted)
    (ref_c * 0.7).backward()
    lg = logits.clone().to(gpu).requires_grad_(True)
    loss = Fn.weighted_cross_entropy(lg, gt.to(gpu), w.to(gpu), weighted)
    (loss * 0.7).backward()
    torch.testing.assert_close(loss.detach().cpu(), ref_c.detach(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(lg.grad.cpu(), lc.grad, rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize("beta,kind", [(0.0, "smooth_l1_weighted"), (0.5, "smooth_l1_weighted"), (0.0, "smooth_l1")])
def test_weighted_l1_box_loss(gpu, beta, kind):
    from wsovod_amd.layers import functions as Fn

    torch.manual_seed(3)
    M, K = 257, 20
    pb = torch.rand(M, 4) * 100
    pb[:, 2:] += pb[:, :2] + 5
    gb = torch.rand(M, 4) * 100
    gb[:, 2:] += gb[:, :2] + 5
    gt = torch.randint(-1, K + 1, (M,))
    w = torch.rand(M)
    pred = torch.randn(M, 4)
    pc = pred.clone().requires_grad_(True)
    _, ref = R.refinement_losses(torch.randn(M, K + 1), pc, gt, w, pb, gb, K, beta=beta, box_loss_type=kind)
    ref.backward()
    pg = pred.clone().to(gpu).requires_grad_(True)
    wk = w.clone()
    wk[gt == -1] = 0
    loss = Fn.weighted_l1_box_loss(pg, pb.to(gpu), gb.to(gpu), gt.to(gpu), wk.to(gpu), K, (10., 10., 5., 5.), beta,
                                   weighted=kind == "smooth_l1_weighted")
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), ref.detach(), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(pg.grad.cpu(), pc.grad, rtol=1e-4, atol=1e-8)


def test_weighted_l1_nan_guard(gpu):
    from wsovod_amd.layers import functions as Fn

    pb = torch.tensor([[0., 0., 10., 10.], [5., 5., 20., 20.]])
    gb = torch.tensor([[0., 0., 10., 10.], [8., 8., 8., 30.]])  # zero-width target -> log(0) = -inf, not NaN
    gb[1] = torch.tensor([9., 9., 5., 30.])  # negative width -> log(<0) = NaN
    gt = torch.tensor([1, 2])
    pred = torch.zeros(2, 4, device=gpu, requires_grad=True)
    loss = Fn.weighted_l1_box_loss(pred, pb.to(gpu), gb.to(gpu), gt.to(gpu), torch.ones(2, device=gpu), 20,
                                   (10., 10., 5., 5.), 0.0)
    loss.backward()
    assert float(loss) == 0.0 and torch.all(pred.grad == 0)  # reference guard: fast_rcnn_open_vocabulary.py:868-871


@pytest.mark.parametrize("case", ["normal", "all_small", "single"])  # images without GT labels never reach this code: the reference filters them (engine/trainer.py:47-50) and its get_pgt_top_k cannot reshape them
def test_pgt_mining_and_labelling_exact(gpu, case):
    from wsovod_amd.layers import hip_ops as H

    torch.manual_seed(4)
    K = 20
    nums = [60, 45, 1] if case != "single" else [1]
    boxes_list, scores_list, gts = [], [], []
    for i, n in enumerate(nums):
        x0, y0 = torch.rand(n) * 300, torch.rand(n) * 200
        b = torch.stack([x0, y0, x0 + 10 + torch.rand(n) * 200, y0 + 10 + torch.rand(n) * 150], 1)
        if case == "all_small" and i == 1:
            b[:, 2:] = b[:, :2] + 3.0  # every box has area 9 <= 20
        if n > 3:
            b[2] = b[1]  # duplicate boxes: IoU ties
        boxes_list.append(b)
        scores_list.append(torch.rand(n, K) * 0.05)
        gts.append(torch.tensor([], dtype=torch.int64) if (case == "no_gt" and i == 0)
                   else torch.unique(torch.randint(0, K, (2,))))
    img_logits = torch.rand(len(nums), K).clamp(1e-6, 1 - 1e-6)
    targets = R.get_pgt_top_k(boxes_list, scores_list, gts, img_logits, K)
    lab = R.label_and_sample_proposals_wsl(boxes_list, targets, K)
    dev = gpu
    seg = torch.tensor([0] + list(torch.tensor(nums).cumsum(0)), dtype=torch.int32, device=dev)
    goff = torch.tensor([0] + list(torch.tensor([len(g) for g in gts]).cumsum(0)), dtype=torch.int32, device=dev)
    o = H.pgt_mine_and_label(torch.cat(scores_list).to(dev), torch.cat(boxes_list).to(dev), seg,
                             torch.cat(gts).to(dev), goff, img_logits.to(dev), K, 0.5)
    torch.cuda.synchronize()
    assert o["pgt_count"].cpu().tolist() == [len(t["gt_classes"]) for t in targets]
    assert torch.equal(o["gt_classes"].cpu(), torch.cat([l["gt_classes"] for l in lab]))
    assert torch.equal(o["gt_boxes"].cpu(), torch.cat([l["gt_boxes"] for l in lab]))
    assert torch.equal(o["gt_weights"].cpu(), torch.cat([l["gt_weights"] for l in lab]))
    assert torch.equal(o["gt_scores"].cpu(), torch.cat([l["gt_scores"] for l in lab]))
    assert torch.equal(o["matched"].cpu().long(), torch.cat([l["matched_idxs"] for l in lab]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_linear_fn_forward_backward(gpu, dtype):
    from wsovod_amd.layers import functions as Fn

    torch.manual_seed(5)
    M, K, N = 150, 256, 44
    x = torch.randn(M, K).to(dtype)
    w = torch.randn(N, K) * 0.1
    b = torch.randn(N)
    xr = x.float().clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    wq = w.to(dtype).float() if dtype == torch.bfloat16 else wr
    yr = F.relu(F.linear(xr, wr if dtype == torch.float32 else wq.requires_grad_(True), br))
    g = torch.randn(M, N)
    yr.backward(g)
    xg = x.to(gpu).requires_grad_(True)
    wg, bg = w.to(gpu).requires_grad_(True), b.to(gpu).requires_grad_(True)
    y = Fn.linear(xg, wg, bg, relu=True, out_dtype=torch.float32)
    y.backward(g.to(gpu))
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(y.detach().cpu(), yr.detach(), **tol)
    wref = wr.grad if dtype == torch.float32 else wq.grad
    torch.testing.assert_close(wg.grad.cpu(), wref, **(tol if dtype == torch.float32 else dict(rtol=5e-2, atol=0.3)))
    torch.testing.assert_close(bg.grad.cpu(), br.grad, **(tol if dtype == torch.float32 else dict(rtol=5e-2, atol=0.3)))
    torch.testing.assert_close(xg.grad.float().cpu(), xr.grad, **(tol if dtype == torch.float32 else dict(rtol=5e-2, atol=0.1)))


def test_dropout_linear_backward_uses_same_mask(gpu):
    from wsovod_amd.layers import functions as Fn

    x = torch.randn(64, 128, device=gpu).abs().requires_grad_(True)
    w = torch.rand(96, 128, device=gpu).requires_grad_(True)
    y = Fn.linear(x, w, None, relu=True, dropout_p=0.5, seed=42)
    kept = (y > 0)
    assert 0.4 < kept.float().mean().item() < 0.6
    y.sum().backward()
    # d/dx of sum(y) = 2 * kept @ w   (inverted dropout scale 2, relu always active: inputs and weights positive)
    torch.testing.assert_close(x.grad, 2.0 * kept.float() @ w.detach(), rtol=1e-4, atol=1e-3)


def test_elementwise_kernels(gpu):
    from wsovod_amd.layers import hip_ops as H

    torch.manual_seed(6)
    # 2x2 max pools incl. the zero-padded stride-1 variant
    x = torch.randn(2, 9, 11, 64)
    for stride, pad in [(2, False), (1, True)]:
        xc = x.permute(0, 3, 1, 2)
        ref = F.max_pool2d(F.pad(xc, (0, 1, 0, 1)) if pad else xc, 2, stride).permute(0, 2, 3, 1)
        for dt in (torch.float32, torch.bfloat16):
            out = H.maxpool2x2_nhwc(x.to(dt).to(gpu).contiguous(), stride, zero_pad_br=pad)
            torch.testing.assert_close(out.float().cpu(), ref.to(dt).float())
    # GAP
    torch.testing.assert_close(H.global_avgpool_nhwc(x.to(gpu)).cpu(), x.mean(dim=(1, 2)), rtol=1e-5, atol=1e-6)
    # preprocess + stem im2col
    img = torch.randint(0, 256, (2, 3, 21, 30), dtype=torch.uint8)
    sizes = torch.tensor([[21, 30], [17, 25]], dtype=torch.int32)
    mean, std = [102.9801, 115.9465, 122.7717], [57.375, 57.12, 58.395]
    ref = R.preprocess_image([img[0], img[1][:, :17, :25]], mean, std)
    out = H.preprocess_image(img.to(gpu), sizes.to(gpu), mean, std)
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-6, atol=1e-6)
    a, ho, wo = H.stem_im2col(img.to(gpu), sizes.to(gpu), mean, std, torch.float32)
    cols = F.unfold(ref, 3, padding=1, stride=2)  # (N, 27 [c,r,q], L)
    cols = cols.view(2, 3, 9, -1).permute(0, 3, 2, 1).reshape(2 * ho * wo, 27)  # -> k = (r*3+q)*3 + c
    torch.testing.assert_close(a.cpu()[:, :27], cols, rtol=1e-6, atol=1e-6)
    assert torch.all(a.cpu()[:, 27:] == 0)
    # data-aware head vs oracle
    from tests.helpers import seeded_sd

    sd = seeded_sd()
    fm = torch.randn(3, 512, 6, 7)
    ref = R.data_aware_forward(sd, fm)
    gap = H.global_avgpool_nhwc(fm.permute(0, 2, 3, 1).contiguous().to(gpu))
    p = "data_aware_head."
    daf, _, _ = H.data_aware_forward(gap, *(sd[p + k].to(gpu) for k in
                                            ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
                                             "datasets_feat.weight")))
    torch.testing.assert_close(daf.cpu(), ref, rtol=1e-4, atol=1e-5)


def test_subsample_labels_matches_reference_golden(gpu):
    """G16 = the reference's _sample_proposals_wsl with the first-k stand-in for subsample_labels; the kernel with
    keys = row index is that rule: labels bit-exact, incl. R = 5024 > 4096 (the shipped RPN form)."""
    from tests.helpers import load_golden
    from wsovod_amd.layers import hip_ops as H

    g = load_golden("g16_subsample")
    i = 0
    while f"case{i}/params" in g:
        R_, num, frac, K = g[f"case{i}/params"].tolist()
        lab = g[f"case{i}/labels_in"].to(gpu)
        seg = torch.tensor([0, int(R_)], dtype=torch.int32, device=gpu)
        out = H.subsample_labels(lab, torch.arange(int(R_), dtype=torch.float32, device=gpu), seg, int(R_), int(num), frac,
                                 int(K))
        assert torch.equal(out.cpu(), g[f"case{i}/labels_out"]), i
        i += 1
    assert i == 5
    # two of the cases (same quota) as ragged segments of one launch, an empty segment between them
    a, b = g["case0/labels_in"], g["case4/labels_in"]
    seg = torch.tensor([0, len(a), len(a), len(a) + len(b)], dtype=torch.int32, device=gpu)
    keys = torch.cat([torch.arange(len(a)), torch.arange(len(b))]).float().to(gpu)
    out = H.subsample_labels(torch.cat([a, b]).to(gpu), keys, seg, max(len(a), len(b)), 4096, 1.0, 20).cpu()
    assert torch.equal(out, torch.cat([g["case0/labels_out"], g["case4/labels_out"]]))


def test_subsample_labels_random_keys(gpu):
    """Random keys: (i) the kernel equals the oracle's keyed subsample_labels on the same keys (ties broken by row);
    (ii) quotas of detectron2's subsample_labels hold; (iii) every positive / negative is drawn with the same
    frequency (uniform without replacement, what randperm does in the reference)."""
    from wsovod_amd.layers import hip_ops as H

    g = torch.Generator().manual_seed(5)
    K, n, num, frac = 20, 300, 64, 0.25
    lab = torch.full((n,), K, dtype=torch.int64)
    lab[torch.randperm(n, generator=g)[:40]] = 3
    lab[torch.randperm(n, generator=g)[:5]] = -1
    pos, neg = (lab != K) & (lab != -1), lab == K
    seg = torch.tensor([0, n], dtype=torch.int32, device=gpu)
    hits = torch.zeros(n)
    trials = 400
    for t in range(trials):
        keys = torch.rand(n, generator=g)
        if t == 0:
            keys[10:20] = keys[10]  # exact ties
        out = H.subsample_labels(lab.to(gpu), keys.to(gpu), seg, n, num, frac, K).cpu()
        p_idx, n_idx = R.subsample_labels_keyed(lab, num, frac, K, keys)
        want = torch.full_like(lab, -1)
        want[torch.cat([p_idx, n_idx])] = lab[torch.cat([p_idx, n_idx])]
        assert torch.equal(out, want)
        kept = out != -1
        assert int((kept & pos).sum()) == min(int(pos.sum()), int(num * frac))
        assert int((kept & neg).sum()) == min(int(neg.sum()), num - int((kept & pos).sum()))
        hits += kept.float()
    for grp in (pos, neg):
        f = hits[grp] / trials
        p = float(f.mean())
        sigma = (p * (1 - p) / trials) ** 0.5
        assert float((f - p).abs().max()) < 5 * sigma + 1e-9


def test_training_step_reductions_are_run_to_run_bit_identical(gpu):
    """The reductions of the training step that once met by fp32 atomic adds -- the K slices of split weight-gradient
    tiles (few output tiles: every tile split; a partly filled last round: its tiles split), the bias-gradient column sums
    of the Linear backward prologue and the two refinement-loss sums -- are written as partials and added in a fixed
    order: repeated launches on the same inputs give the same bits (and the values of an fp64 reference)."""
    from wsovod_amd.layers import functions as Fn
    from wsovod_amd.layers import hip_ops as H

    torch.manual_seed(31)
    for Mred, NI, NJ in ((16384, 512, 1024), (4096, 256 * 17, 256 * 16)):  # 8 tiles x 8 slices; 272 tiles = 256 + 16 split
        P = (torch.rand(Mred, NI, device=gpu) - 0.5).to(torch.bfloat16)
        Q = (torch.rand(Mred, NJ, device=gpu) - 0.5).to(torch.bfloat16)
        first = H.gemm_tn(P, Q)
        for _ in range(5):
            assert torch.equal(H.gemm_tn(P, Q), first)
        torch.testing.assert_close(first.double(), P.double().t() @ Q.double(), rtol=1e-4, atol=1e-3)
        acc = torch.randn(NI, NJ, device=gpu)
        again = H.gemm_tn(P, Q, out=acc.clone(), alpha=0.5, accumulate=True)
        assert torch.equal(H.gemm_tn(P, Q, out=acc.clone(), alpha=0.5, accumulate=True), again)
        del P, Q, first, acc, again
    M, N = 8192, 1024
    dy = torch.randn(M, N, device=gpu)
    y = torch.randn(M, N, device=gpu)
    sums = []
    for _ in range(5):
        cs = torch.zeros(N, device=gpu)
        H.mask_transpose(dy, y, 0.5, torch.bfloat16, want_t=False, colsum=cs)
        sums.append(cs)
    assert all(torch.equal(c, sums[0]) for c in sums)
    want = (dy.double() * (y > 0) * 0.5).sum(0)
    torch.testing.assert_close(sums[0].double(), want, rtol=1e-5, atol=1e-4)
    M, K = 16384, 20
    logits = torch.randn(M, K + 1, device=gpu) * 4
    gt = torch.randint(-1, K + 1, (M,), device=gpu)
    w = torch.rand(M, device=gpu)
    ce = [Fn.weighted_cross_entropy(logits, gt, w, True) for _ in range(5)]
    assert all(torch.equal(c, ce[0]) for c in ce)
    pb = torch.rand(M, 4, device=gpu) * 100
    pb[:, 2:] += pb[:, :2] + 5
    gb = torch.rand(M, 4, device=gpu) * 100
    gb[:, 2:] += gb[:, :2] + 5
    pred = torch.randn(M, 4, device=gpu)
    wk = torch.where(gt == -1, torch.zeros_like(w), w)
    l1 = [Fn.weighted_l1_box_loss(pred, pb, gb, gt, wk, K, (10., 10., 5., 5.), 0.0) for _ in range(5)]
    assert all(torch.equal(v, l1[0]) for v in l1)


def test_column_sums_are_run_to_run_bit_identical(gpu):
    """segment_colsum / the NHWC global average pool are fixed-order two-stage reductions (per-chunk fp32 partials, then
    one pass in chunk order): the same input gives the same bits whatever the launch timing, with no quantisation.  (With
    fp32 atomics the pooled statistics moved in their last bits between runs; through near-tied mining scores that
    flipped a pseudo ground-truth box on ~15 % of cold starts of the RPN golden test.  Round 2's 64-bit fixed-point
    atomics fixed that but quantised at 2^-30 ABSOLUTE: gradient sums of magnitude 1e-8 lost everything, sums past 8.6e9
    wrapped.)  Checked against fp64 at magnitudes 1e-8, 1 and 1e+9, for ragged segments incl. empty ones, segments
    shorter than a chunk, and non-finite inputs."""
    from wsovod_amd.layers import hip_ops as H

    torch.manual_seed(21)
    x = (torch.randn(8, 75 * 100, 512, device=gpu) * 3).to(torch.bfloat16)
    first = H.global_avgpool_nhwc(x.view(8, 75, 100, 512))
    for _ in range(30):
        assert torch.equal(H.global_avgpool_nhwc(x.view(8, 75, 100, 512)), first)
    torch.testing.assert_close(first.double().cpu(), x.double().mean(1).cpu(), rtol=2e-6, atol=1e-7)
    bounds = [0, 1, 4000, 4000, 4003, 4100, 4101, 9000]  # 1-row, empty, 3-row, sub-chunk and multi-chunk segments
    seg = torch.tensor(bounds, dtype=torch.int32, device=gpu)
    base = torch.rand(9000, 200, device=gpu) + 0.5  # positive: the sum's magnitude is the natural error scale
    for scale in (1e-8, 1.0, 1e9):
        rows = base * scale
        s0 = H.segment_colsum(rows, seg)
        for _ in range(10):
            assert torch.equal(H.segment_colsum(rows, seg), s0)
        want = torch.stack([rows[a:b].double().sum(0) for a, b in zip(bounds[:-1], bounds[1:])])
        torch.testing.assert_close(s0.double().cpu(), want.cpu(), rtol=2e-6, atol=0.0)
    mixed = torch.randn(9000, 200, device=gpu)  # mixed signs: error relative to the sum of magnitudes
    got = H.segment_colsum(mixed, seg).double().cpu()
    want = torch.stack([mixed[a:b].double().sum(0) for a, b in zip(bounds[:-1], bounds[1:])]).cpu()
    mag = torch.stack([mixed[a:b].double().abs().sum(0) for a, b in zip(bounds[:-1], bounds[1:])]).cpu()
    assert float(((got - want).abs() / mag.clamp(min=1e-30)).max()) < 2e-6
    acc = torch.full((7, 200), 2.0, device=gpu)  # accumulate adds to the existing values
    H.segment_colsum(mixed, seg, out=acc, accumulate=True)
    torch.testing.assert_close(acc.double().cpu(), want + 2.0, rtol=1e-5, atol=1e-4)
    bad = base.clone()
    bad[4500, 7] = float("nan")
    bad[10, 3] = float("inf")
    sb = H.segment_colsum(bad, seg).cpu()
    assert torch.isnan(sb[6, 7]) and torch.isinf(sb[1, 3]) and torch.isfinite(sb[0]).all()  # non-finite values propagate
    rows_bf = (base * 3).to(torch.bfloat16)  # bf16 input form (8 columns per lane)
    torch.testing.assert_close(H.segment_colsum(rows_bf, seg).double().cpu(),
                               torch.stack([rows_bf[a:b].double().sum(0) for a, b in zip(bounds[:-1], bounds[1:])]).cpu(),
                               rtol=2e-6, atol=0.0)


@pytest.mark.parametrize("kind", ["full_model", "norm", "value"])
@pytest.mark.parametrize("wire", [False, True])
def test_hip_sgd_gradient_clipping_matches_torch(gpu, kind, wire):
    """SOLVER.CLIP_GRADIENTS on the fused optimizer (engine/defaults.py:292-323): "full_model" = clip_grad_norm_ over all
    parameters at once (the reference's FullModelGradientClippingOptimizer), "norm" / "value" = detectron2's per-parameter
    forms.  Norms and coefficients stay on the device; compared with torch's clip + SGD over three steps (fp32 gradients
    and the bf16 wire slices), a clip value that bites on some tensors and not on others, one tensor with grad None."""
    from wsovod_amd.engine.trainer import HipSGD

    torch.manual_seed(3)
    shapes = [(300, 70), (4097,), (64, 64), (5,)]
    ps = [torch.nn.Parameter(torch.randn(s, device=gpu)) for s in shapes]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    value = {"full_model": 3.0, "norm": 20.0, "value": 0.05}[kind]
    hip = HipSGD([{"params": [p], "lr": 0.1, "weight_decay": 1e-3} for p in ps], 0.1, momentum=0.9, clip=(kind, value))
    hip.grad_scale = 0.5
    ref = torch.optim.SGD([{"params": [q], "lr": 0.1, "weight_decay": 1e-3} for q in qs], 0.1, momentum=0.9)
    for step in range(3):
        grads = [torch.randn(s, device=gpu) * (0.02 if i == 2 else 0.3) for i, s in enumerate(shapes)]
        if wire:
            grads = [g.to(torch.bfloat16).float() for g in grads]
        for i, (p, q, g) in enumerate(zip(ps, qs, grads)):
            if i == 3 and step == 1:  # no gradient this step: skipped by both, and not part of the norm
                p.grad = q.grad = None
                p._wire_grad = None
                continue
            q.grad = g * 0.5
            if wire:
                p.grad, p._wire_grad = None, g.to(torch.bfloat16).reshape(-1)
            else:
                p.grad, p._wire_grad = g.clone(), None
        live = [q for q in qs if q.grad is not None]
        if kind == "full_model":
            torch.nn.utils.clip_grad_norm_(live, value)
        elif kind == "norm":
            for q in live:
                torch.nn.utils.clip_grad_norm_(q, value)
        else:
            for q in live:
                torch.nn.utils.clip_grad_value_(q, value)
        ref.step()
        hip.step()
        for p, q in zip(ps, qs):
            torch.testing.assert_close(p.detach(), q.detach(), rtol=2e-6, atol=2e-6)
    if kind != "value":
        c = hip.last_clip_coef.cpu()
        assert bool((c <= 1.0).all()) and bool((c < 1.0).any())
        if kind == "norm":
            assert float(c[2]) == 1.0  # the small tensor's norm is under the bound: left alone


def test_build_optimizer_reads_clip_gradients(gpu):
    from wsovod_amd.engine import build_optimizer
    from wsovod_amd.testing import build_hot_path_model

    cfg, model = build_hot_path_model(device="cpu")
    assert build_optimizer(cfg, model).clip is None
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "full_model"
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = 1.5
    assert build_optimizer(cfg, model).clip == ("full_model", 1.5)
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "norm"
    cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE = 1.0
    with pytest.raises(NotImplementedError):
        build_optimizer(cfg, model)
