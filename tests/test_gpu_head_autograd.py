"""-m gpu: the head-side autograd fronts of wsovod_amd/layers/functions.py -- `cosine_logits`, `data_aware_features`,
`global_avgpool_nhwc`, `add_group_rows` -- and `scale_losses`, called as the model calls them, against fp64 autograd
(tests/functions_ref.py).  Tolerances |err| <= c u B, each c derived beside its use; the observed ratios go to
profiles/functions_autograd_bounds.json (WSOVOD_FUNCTIONS_AUTOGRAD_BOUNDS=<file>)."""
import pytest
import torch

from tests import functions_ref as FR
from tests.util import same_bits

pytestmark = pytest.mark.gpu

U32, UBF, UX2 = FR.U32, FR.UBF, FR.UX2


@pytest.fixture(scope="module", autouse=True)
def _record_ratios():
    yield
    FR.write_ratios()


def _fn():
    from wsovod_amd.layers import functions as Fn
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.layers import precision
    return Fn, H, precision


def _within(key, got, ref, B, c, u, bf16_out=False):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    bound = c * u * B
    if bf16_out:
        err = (err - FR.bf16_ulp(ref) - 2.0 ** -8 * bound).clamp_min(0)
    worst = FR.record(key, err, u * B)
    print(f"{key}: max err / (u B) = {worst:.3f}, c = {c:.2f}, u = 2^{torch.log2(torch.tensor(u)).item():.0f}")
    assert bool((err <= bound).all()), (key, worst, c)


# ---- cosine_logits ----------------------------------------------------------------------------------------------------
# mode -> (scope name or None, z / class-matrix dtype, u forward, u backward, operand roundings forward, backward)
#   fp32          every operand as read, every product and sum in fp32: no operand rounding.
#   bf16          z and the class matrix ARE bf16 (as read: the reference holds the same numbers), products exact in the fp32
#                 accumulator.  Backward: the logits' gradient is rounded to bf16 (1 rounding = 2 u at u = 2^-9,
#                 conv_backward_ref.ROUND) and dz is cast to bf16 at the end (handled as a bf16 output) -> 2.
#   parity        forward: z and the class matrix are encoded as (hi, lo) bf16 pairs, each within 2^-18 = u / 2 of the value, and
#                 the lo * lo product (<= 2^-18 of the term) is dropped: 1.5 u, counted 2.  Backward (forward-only split): the
#                 gradient AND the fp32 class matrix are rounded to bf16: 2 roundings = 4 u at u = 2^-9.
#   parity_train  ("dx" split, the default of WSOVOD_PT_SPLIT): the backward contraction keeps the split on fp32 operands:
#                 as the parity forward, 2 at u = 2^-17.
MODES = {"fp32": (None, torch.float32, U32, U32, 0.0, 0.0), "bf16": (None, torch.bfloat16, UBF, UBF, 0.0, 2.0),
         "parity": ("parity", torch.float32, UX2, UBF, 2.0, 4.0), "parity_train": ("parity_train", torch.float32, UX2, UX2, 2.0, 2.0)}


def _class_matrix(H, rows, dtype):
    """OpenVocabularyClassifier._class_matrix with a given classifier, norm_weight and append_background."""
    Cn, D = rows.shape
    K1 = Cn + 1
    wn = torch.zeros((K1, D), dtype=dtype, device=rows.device)
    H.scale_rows(rows, H.row_l2norm_scale(rows, 1.0), wn)
    return wn, H.transpose_cast(wn, dtype, ld_dst=(K1 + 7) // 8 * 8)


@pytest.mark.parametrize("K1", [2, 21, 81])
@pytest.mark.parametrize("D", [64, 520])
@pytest.mark.parametrize("M", [1, 37, 300])
@pytest.mark.parametrize("mode", list(MODES))
def test_cosine_logits_autograd(gpu, monkeypatch, mode, M, D, K1):
    """z >= 0 as behind the ReLU (half its entries exactly 0: the backward must NOT mask them again, `relu_mask=False`), row 0
    all zero, row 1 of norm < eps (M = 1: each in turn).  Both take F.normalize's clamped branch: logits T z / eps and
    dz = T v / eps with no projection term -- the kernel's `clamped` branch is the same expression, and the reference model
    (open_vocabulary_classifier.py:94: F.normalize(x, p=2, dim=1)) is what fp64 autograd differentiates here."""
    Fn, H, precision = _fn()
    monkeypatch.delenv("WSOVOD_PT_SPLIT", raising=False)
    scope_name, dtype, u_f, u_b, r_f, r_b = MODES[mode]
    if scope_name and D % 32:
        # bf16x2 rows are whole 32-value groups: the "parity" modes refuse D = 520, they do not fall back (the model's D is
        # 512).  The modes' odd contraction length is D = 544 = 17 * 32 instead: no multiple of the 64-column K-step either.
        with precision.scope(precision.TABLE[scope_name]), pytest.raises(RuntimeError, match="multiple of 32"):
            Fn.cosine_logits(torch.zeros(M, D, device=gpu), torch.zeros(K1, D, device=gpu),
                             torch.zeros(D, (K1 + 7) // 8 * 8, device=gpu), 50.0, True, None)
        D = 544
    T = 50.0
    g = torch.Generator().manual_seed(M * 1000 + D + K1)
    rows = torch.randn(K1 - 1, D, generator=g).to(gpu)
    wn, wnT = _class_matrix(H, rows, dtype)
    assert wnT.shape == (D, (K1 + 7) // 8 * 8) and bool((wn[-1] == 0).all()) and bool((wnT[:, K1 - 1:] == 0).all())
    base = torch.relu(torch.randn(M, D, generator=g))
    dl = torch.randn(M, K1, generator=g)
    bias0 = torch.randn(K1, generator=g)
    variants = ["zero+tiny"] if M > 1 else ["zero", "tiny"]
    K1p = wnT.size(1)
    for variant in variants:
        z0 = base.clone()
        if variant == "zero+tiny":
            z0[1] = 1e-14 * (z0[2] + 0.5)
            z0[0] = 0
        elif variant == "zero":
            z0[0] = 0
        else:
            z0[0] = 1e-14 * (z0[0] + 0.5)
        z0 = z0.to(dtype)
        for normalize in (True, False):
            for with_bias in (True, False):
                z = z0.to(gpu).requires_grad_()
                bias = bias0.to(gpu).requires_grad_() if with_bias else None
                scope = precision.scope(precision.TABLE[scope_name]) if scope_name else precision.x3_mode(False)
                with scope:
                    y = Fn.cosine_logits(z, wn, wnT, T, normalize, bias)
                    y.backward(dl.to(gpu))
                ref = FR.cosine_reference(z0, wn, T, normalize, None if bias is None else bias0, dl)
                key = f"cosine-{mode}-M{M}-D{D}-K{K1}"
                if normalize:
                    assert float(z0.float().norm(dim=1).min()) < 1e-12  # the clamped branch is exercised
                assert y.dtype == torch.float32 and z.grad.dtype == dtype
                # forward: functions_ref.c_cosine_forward (normalize off: its norm terms are simply not spent)
                _within(key + "-logits", y, ref["logits"], ref["B_logits"], FR.c_cosine_forward(D, u_f, r_f), u_f)
                # backward: functions_ref.c_cosine_backward
                _within(key + "-dz", z.grad, ref["dz"], ref["B_dz"], FR.c_cosine_backward(D, K1p, u_b, r_b), u_b,
                        bf16_out=dtype == torch.bfloat16)
                if with_bias:
                    # segment_colsum over one segment of M rows: M terms, fixed order, + the final store
                    _within(key + "-db", bias.grad, ref["db"], ref["B_db"], M + 1, U32)


# ---- data_aware_features ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 512, 32, 5, 512), (2, 48, 3, 7, 33)])
def test_data_aware_features_autograd(gpu, dims):
    """All five gradients through `_DataAware.backward`'s return order against fp64 autograd, with the bound of
    test_gpu_elementwise.py::test_data_aware_backward ((terms + 8) 2^-24 on the magnitudes that carry tanh's slope).  W1
    (Hd, C), W2 (P, Hd), E (P, F) and the two biases all differ in shape or in value, so no two returns can change places."""
    Fn, H, _ = _fn()
    N, C, Hd, P, Fd = dims
    case = FR.data_aware_case(N, C, Hd, P, Fd, torch.Generator().manual_seed(sum(dims)))
    gap, ddaf = case[0], case[6]
    daf_ref, grads, mags = FR.data_aware_reference(*case)
    dev = [t.to(gpu).requires_grad_() for t in case[1:6]]
    daf = Fn.data_aware_features(gap.to(gpu), *dev)
    daf.backward(ddaf.to(gpu))
    terms = FR.data_aware_terms(N, C, Hd, P, Fd)
    _within(f"data_aware-{dims}-daf", daf, daf_ref, mags["daf"], C + Hd + P + 8, U32)
    for name, t in zip(("dW1", "db1", "dW2", "db2", "dE"), dev):
        assert float(mags[name].max()) > 0
        _within(f"data_aware-{dims}-{name}", t.grad, grads[name], mags[name], terms[name], U32)


# ---- the global average pool ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [64, 100])
def test_global_avgpool_autograd(gpu, C, dtype):
    """Forward: a sum of H W = 35 values as read and one scaling: (35 + 1) 2^-24 of mean |x|.  Backward: g / (H W) broadcast --
    one fp32 division (1 u of |g| / 35; a product with the rounded reciprocal would spend two), for a bf16 map one rounding
    to bf16 on top."""
    Fn, _, _ = _fn()
    g = torch.Generator().manual_seed(C)
    x0 = torch.randn(2, 5, 7, C, generator=g).to(dtype)
    dy = torch.randn(2, C, generator=g)
    x = x0.to(gpu).requires_grad_()
    y = Fn.global_avgpool_nhwc(x)
    y.backward(dy.to(gpu))
    assert y.dtype == torch.float32 and x.grad.dtype == dtype and x.grad.shape == x.shape
    _within(f"gap-{C}-{dtype}-fwd", y, FR.gap(x0.double()), FR.gap(x0.double().abs()), 36, U32)
    ref = (dy.double() / 35).view(2, 1, 1, C).expand(2, 5, 7, C)
    _within(f"gap-{C}-{dtype}-bwd", x.grad, ref, ref.abs(), 1, U32, bf16_out=dtype == torch.bfloat16)


# ---- add_group_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,counts,N", [("plain", [3, 0, 4, 1], 20), ("plain", [3, 0, 4, 1], 64), ("x2", [3, 0, 4, 1], 64),
                                           ("x2", [3, 0, 4, 2], 64)])
def test_add_group_rows_autograd(gpu, mode, counts, N):
    """Segments with an empty one; the x2 mode on a bf16x2 carrier (the (9, 64) carrier: counts [3, 0, 4, 2]).  dy passes to x
    bit for bit; dadd is the segment's column sum: len terms + the store, (len + 1) 2^-24 sum |dy|; the empty segment's row
    is exactly 0.  Forward, plain: one fp32 add, same bits as torch's; x2: tests/test_gpu_elementwise.py's bound."""
    Fn, H, precision = _fn()
    M, G = sum(counts), len(counts)
    g = torch.Generator().manual_seed(M + N)
    x0, add0, dy = torch.randn(M, N, generator=g), torch.randn(G, N, generator=g), torch.randn(M, N, generator=g)
    rg = torch.repeat_interleave(torch.arange(G, dtype=torch.int32), torch.tensor(counts))
    seg = torch.tensor([sum(counts[:i]) for i in range(G + 1)], dtype=torch.int32)
    add = add0.to(gpu).requires_grad_()
    if mode == "x2":
        x = H.x2_encode(x0.to(gpu))
        stored = H.x2_decode(x).cpu()
        x.requires_grad_()
        with precision.scope(precision.TABLE["parity"]):
            y = Fn.add_group_rows(x, add, rg.to(gpu), seg.to(gpu))
        want = FR.add_group_rows(stored.double(), add0.double(), rg)
        bound = 2.0 ** -15 * torch.maximum(stored.abs(), add0[rg.long()].abs()).double()
        assert bool(((H.x2_decode(y.detach()).cpu().double() - want).abs() <= bound).all())
    else:
        x = x0.to(gpu).requires_grad_()
        y = Fn.add_group_rows(x, add, rg.to(gpu), seg.to(gpu))
        assert same_bits(y.detach().cpu(), FR.add_group_rows(x0, add0, rg))
    y.backward(dy.to(gpu))
    assert same_bits(x.grad.cpu(), dy)
    got = add.grad.cpu()
    assert got.shape == (G, N) and bool((got[1] == 0).all())
    for i, n in enumerate(counts):
        rows = dy[seg[i]:seg[i + 1]].double()
        _within(f"add_group_rows-{mode}-{counts}-{N}-seg{i}", got[i], rows.sum(0), rows.abs().sum(0), n + 1, U32)
        if n == 0:
            assert bool((got[i] == 0).all())


# ---- scale_losses -----------------------------------------------------------------------------------------------------------
def test_scale_losses(gpu):
    """A float weight scales every loss; a dict scales the named ones and leaves the others (weight 1: the SAME tensor, no
    kernel); the gradient of loss * w is w."""
    Fn, _, _ = _fn()
    a = torch.tensor(1.5, device=gpu, requires_grad=True)
    b = torch.tensor(-0.25, device=gpu, requires_grad=True)
    losses = {"loss_a": a * 2.0, "loss_b": b * 4.0}
    out = Fn.scale_losses(losses, 0.5)
    assert set(out) == set(losses) and float(out["loss_a"]) == 1.5 and float(out["loss_b"]) == -0.5
    same = Fn.scale_losses(losses, 1.0)
    assert same["loss_a"] is losses["loss_a"] and same["loss_b"] is losses["loss_b"]
    byname = Fn.scale_losses(losses, {"loss_b": 3.0, "loss_c": 7.0})
    assert byname["loss_a"] is losses["loss_a"] and float(byname["loss_b"]) == -3.0 and set(byname) == set(losses)
    (out["loss_a"] + byname["loss_b"]).backward()
    assert float(a.grad) == 1.0 and float(b.grad) == 12.0
