"""-m gpu: the two index kernels of the MRRP RPN's proposal stage (wsovod_rpn_group_topk, wsovod_nms_merge_groups)
against their torch comparators, bit for bit, and the whole selection against the CPU restatement."""
import itertools

import pytest
import torch

from tests import mrrp_rpn_util as U
from tests.conftest import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

HWS, AS, PRES, BS = (1, 63, 64, 65, 300, 2049, 5000), (1, 6, 18), (1, 7, 64, 2048), (1, 6)


def make_logits(pattern, B, HW, A, gen):
    x = torch.randn((B, HW, A), generator=gen)
    if pattern == "quantised":  # 5 levels: many ties straddle the k-th value
        x = torch.round(x.clamp(-2, 2))
    elif pattern == "equal":
        x = torch.full((B, HW, A), 0.375)
    elif pattern in ("special", "nan_payloads"):  # +-0, +-inf and NaN among few distinct values
        x = torch.round(x.clamp(-1, 1))
        pick = torch.randint(0, 8, (B, HW, A), generator=gen)
        for code, v in ((0, 0.0), (1, -0.0), (2, float("inf")), (3, float("-inf")), (4, float("nan"))):
            x = torch.where(pick == code, torch.full_like(x, v), x)
        if pattern == "nan_payloads":  # a second payload and the negative sign
            for code, word in ((5, 0x7FC00001), (6, -0x400000)):
                v = torch.tensor([word], dtype=torch.int32).view(torch.float32)
                x = torch.where(pick == code, v.expand_as(x), x)
    return x


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("pattern", ["random", "quantised", "equal", "special"])
def test_group_topk_equals_the_stable_torch_sort(gpu, pattern):
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.modeling.proposal_generator import _group_topk_torch

    gen = torch.Generator().manual_seed(11)
    for HW, A, pre, B in itertools.product(HWS, AS, PRES, BS):
        x = make_logits(pattern, B, HW, A, gen).cuda()
        sc, idx = H.rpn_group_topk(x, pre)
        k = min(HW, pre)
        ref_sc, ref_pos = torch.sort(x.permute(0, 2, 1), dim=-1, descending=True, stable=True)
        ref_idx = ref_pos[..., :k] * A + torch.arange(A, device="cuda").view(1, A, 1)
        assert sc.shape == (B, A, k) and idx.dtype == torch.int64
        assert torch.equal(idx, ref_idx), (pattern, HW, A, pre, B)
        assert torch.equal(bits(sc), bits(ref_sc[..., :k])), (pattern, HW, A, pre, B)
        t_sc, t_idx = _group_topk_torch(x, k)  # the route past the kernel's limit gives the same bits
        assert torch.equal(t_idx, idx) and torch.equal(bits(t_sc), bits(sc))


def test_group_topk_holds_every_nan_equal(gpu):
    """NaNs of other payloads or sign are one value to the kernel, as to torch's comparison-based sort.  The device sort
    that torch picks for these shapes orders such NaNs by their bits (0x7fc00001 ahead of 0x7fc00000), so the comparator
    here is the stable sort on the CPU; the rows of the test above hold the canonical NaN only."""
    from wsovod_amd.layers import hip_ops as H

    gen = torch.Generator().manual_seed(13)
    for HW, A, pre in ((65, 6, 7), (300, 1, 64), (2049, 6, 2048)):
        x = make_logits("nan_payloads", 2, HW, A, gen)
        sc, idx = H.rpn_group_topk(x.cuda(), pre)
        k = min(HW, pre)
        ref_sc, ref_pos = torch.sort(x.permute(0, 2, 1), dim=-1, descending=True, stable=True)
        assert torch.equal(idx.cpu(), ref_pos[..., :k] * A + torch.arange(A).view(1, A, 1)), (HW, A, pre)
        assert torch.equal(bits(sc.cpu()), bits(ref_sc[..., :k])), (HW, A, pre)


def test_group_topk_refuses_more_than_2048(gpu):
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.modeling.proposal_generator import rpn_group_topk

    x = torch.randn((1, 4096, 2), device="cuda")
    with pytest.raises(RuntimeError, match="2048"):
        H.rpn_group_topk(x, 2049)
    sc, idx = rpn_group_topk(x, 3000)  # the wrapper takes the torch route
    ref = torch.sort(x.permute(0, 2, 1), dim=-1, descending=True, stable=True)
    assert torch.equal(sc, ref.values[..., :3000]) and torch.equal(idx // 2, ref.indices[..., :3000])


def segments(N, G, k, counts, gen, dup):
    """Descending-score segments with keep lists as nms_segments writes them (ascending relative positions)."""
    sc = torch.randn((N * G, k), generator=gen)
    if dup:  # scores duplicated across (and inside) groups
        sc = torch.round(sc * 2) / 2
    sc = torch.sort(sc, dim=1, descending=True).values
    boxes = torch.rand((N * G * k, 4), generator=gen) * 100
    keep_idx = torch.full((N * G * k,), -7, dtype=torch.int32)
    for s, c in enumerate(counts):
        keep_idx[s * k:s * k + c] = torch.sort(torch.randperm(k, generator=gen)[:c]).values.to(torch.int32)
    return boxes, sc.reshape(-1), keep_idx, torch.tensor(counts, dtype=torch.int32)


@pytest.mark.parametrize("G,A", [(1, 1), (3, 1), (18, 6)])
@pytest.mark.parametrize("post", [1, 100, 1024])
def test_merge_groups_equals_gather_and_stable_sort(gpu, G, A, post):
    from wsovod_amd.layers import hip_ops as H

    gen = torch.Generator().manual_seed(5 + G + post)
    N = 3
    for k, mode, dup in itertools.product((1, 64, 300), ("zeros", "full", "short", "mixed"), (False, True)):
        cap = min(k, post)  # nms_segments stops at max_keep = post
        if mode == "zeros":
            counts = [0] * (N * G)
        elif mode == "full":  # every list as long as it can be (longer than post where k allows)
            counts = [cap] * (N * G)
        elif mode == "short":  # total below post where possible
            counts = [min(cap, max(0, (post - 1) // max(G, 1) - (s % 2))) for s in range(N * G)]
        else:
            counts = torch.randint(0, cap + 1, (N * G,), generator=gen).tolist()
        boxes, sc, keep_idx, keep_count = segments(N, G, k, counts, gen, dup)
        ob, osc, oid, oc = H.nms_merge_groups(boxes.cuda(), sc.cuda(), keep_idx.cuda(), keep_count.cuda(), N, G, A, k, post)
        ref = U.merge_lists(boxes, sc, keep_idx, keep_count, N, G, A, k, post)
        for n, (rb, rs, rt) in enumerate(ref):
            c = int(oc[n])
            assert c == len(rs) == min(post, sum(counts[n * G:(n + 1) * G])), (k, mode, dup, n)
            assert torch.equal(ob[n, :c].cpu(), rb) and torch.equal(osc[n, :c].cpu(), rs), (k, mode, dup, n)
            assert torch.equal(oid[n, :c].cpu(), rt), (k, mode, dup, n)


def test_whole_selection_equals_the_restatement(gpu):
    """N = 2, L = 3, A = 6, a 12 x 16 map, pre 64, post 100: the same scores and already-decoded boxes through
    group top-k -> nms_segments -> merge, against the CPU restatement; exact."""
    from wsovod_amd.layers import hip_ops as H

    gen = torch.Generator().manual_seed(3)
    N, L, A, HW, pre, post, thr = 2, 3, 6, 12 * 16, 64, 100, 0.7
    logits = torch.round(torch.randn((L * N, HW, A), generator=gen) * 8) / 8  # ties inside and across groups
    ctr = torch.rand((L * N, HW * A, 2), generator=gen) * 200
    half = torch.rand((L * N, HW * A, 2), generator=gen) * 60 + 1
    boxes = torch.cat([ctr - half, ctr + half], dim=-1).clamp(0, 256)
    valid = torch.rand((L * N, HW * A), generator=gen) > 0.1
    ref = U.select_from_decoded(logits, boxes, valid, N, L, pre, post, thr)
    k = min(HW, pre)
    G = L * A
    sc, idx = H.rpn_group_topk(logits.cuda(), pre)  # (L*N, A, k)
    flat = idx.view(L * N, A * k)
    b = boxes.cuda().gather(1, flat[..., None].expand(-1, -1, 4)).view(L, N, A * k, 4).permute(1, 0, 2, 3).reshape(-1, 4)
    v = valid.cuda().gather(1, flat).view(L, N, A * k).permute(1, 0, 2).reshape(-1)
    s = sc.view(L, N, A * k).permute(1, 0, 2).reshape(-1)
    seg = torch.arange(N * G + 1, dtype=torch.int32, device="cuda") * k
    keep, count = H.nms_segments(b.contiguous(), seg, k, thr, post, valid=v & torch.isfinite(s))
    ob, osc, oid, oc = H.nms_merge_groups(b.contiguous(), s.contiguous(), keep, count, N, G, A, k, post)
    for n, (rb, rs, rt) in enumerate(ref):
        c = int(oc[n])
        assert c == len(rs) and c > 20
        assert torch.equal(ob[n, :c].cpu(), rb) and torch.equal(osc[n, :c].cpu(), rs) and torch.equal(oid[n, :c].cpu(), rt)
