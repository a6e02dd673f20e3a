"""The carrier tag of a float32-typed activation (wsovod_amd/layers/carrier.py) on CPU tensors: what `tag` records, which
torch operations keep the tag and which drop it, how `like` restores it, and what `refuse` raises for."""
import pytest
import torch

from wsovod_amd.layers import carrier as Cr


def _hi(t):
    return t.to(torch.bfloat16)


def test_tag_records_format_and_hi_and_returns_the_tensor():
    t = torch.randn(8, 32)
    assert Cr.fmt_of(t) is None and Cr.hi_of(t) is None and Cr.fmt_of(None) is None
    hi = _hi(t)
    assert Cr.tag(t, Cr.MX, hi) is t
    assert Cr.fmt_of(t) == Cr.MX and Cr.hi_of(t) is hi
    u = Cr.tag(torch.randn(8, 32), Cr.X2)
    assert Cr.fmt_of(u) == Cr.X2 and Cr.hi_of(u) is None
    assert len({Cr.X2, Cr.X2P, Cr.MX}) == 3


def test_a_second_tag_replaces_the_first():
    t = torch.randn(8, 32)
    Cr.tag(t, Cr.MX, _hi(t))
    Cr.tag(t, Cr.X2)
    assert Cr.fmt_of(t) == Cr.X2 and Cr.hi_of(t) is None  # (the hi of the first tag is gone with it)
    assert [k for k in vars(t) if "carrier" in k] == [Cr._ATTR]  # one attribute, whatever was tagged before


@pytest.mark.parametrize("fmt", [Cr.X2, Cr.X2P, Cr.MX])
def test_whole_views_carry_format_and_hi(fmt):
    t = torch.randn(4, 2, 4, 4)
    hi = _hi(t)
    Cr.tag(t, fmt, hi)
    for v in (t.view(4, 32), torch.flatten(t, start_dim=1), t.reshape(-1, 16), t.view(4, 32).view(8, 16)):
        assert v._base is t and Cr.fmt_of(v) == fmt and Cr.hi_of(v) is hi


def test_slices_cat_clone_and_detach_drop_the_tag():
    t = Cr.tag(torch.randn(8, 32), Cr.MX, _hi(torch.randn(8, 32)))
    for u in (t[2:6], t[:4], t[4:], torch.cat([t, t]), torch.cat([t[:4], t[4:]]), t.clone(), t.detach()):
        assert Cr.fmt_of(u) is None and Cr.hi_of(u) is None
    assert Cr.fmt_of(t[0:8]) == Cr.MX  # (all rows: a whole view after all)


def test_a_view_with_another_numel_or_pointer_is_not_the_carrier():
    t = Cr.tag(torch.randn(8, 32), Cr.X2P)
    head, tail = t.view(-1)[:128], t.view(-1)[128:]
    assert head._base is t and head.data_ptr() == t.data_ptr() and Cr.fmt_of(head) is None  # same pointer, fewer values
    assert tail.data_ptr() != t.data_ptr() and Cr.fmt_of(tail.view(4, 32)) is None
    assert Cr.fmt_of(t.t()) == Cr.X2P  # the rule is pointer + numel (the fronts refuse what is not contiguous themselves)


def test_a_bfloat16_view_of_a_carrier_is_not_a_carrier():
    t = torch.randn(8, 32)
    plane = t.view(-1).view(torch.bfloat16)[:t.numel()].view(t.shape)  # the hi plane of a planar carrier, as the poolers attach it
    Cr.tag(t, Cr.X2P, plane)
    assert Cr.hi_of(t) is plane and Cr.fmt_of(plane) is None and Cr.hi_of(plane) is None
    whole = t.view(torch.bfloat16)  # same pointer, all of t's bytes: still a plain bf16 matrix
    assert whole.data_ptr() == t.data_ptr() and Cr.fmt_of(whole) is None
    assert Cr.fmt_of(Cr.tag(torch.zeros(4, dtype=torch.bfloat16), Cr.MX)) is None  # not float32-typed: never a carrier


def test_a_function_output_tagged_in_forward_is_tagged_at_the_caller():
    class Lin(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w):
            y = x @ w.t()
            ctx.save_for_backward(x, w)
            return Cr.tag(y, Cr.MX, _hi(y))

        @staticmethod
        def backward(ctx, dy):
            x, w = ctx.saved_tensors
            return dy @ w, dy.t() @ x

    x, w = torch.randn(4, 32), torch.randn(16, 32, requires_grad=True)
    y = Lin.apply(x, w)
    assert y.requires_grad and Cr.fmt_of(y) == Cr.MX and Cr.hi_of(y).dtype == torch.bfloat16
    assert Cr.fmt_of(torch.flatten(y, start_dim=1)) == Cr.MX
    y.sum().backward()
    assert w.grad.shape == w.shape


@pytest.mark.parametrize("fmt", [Cr.X2, Cr.MX])
def test_like_restores_the_format_not_the_hi(fmt):
    t = Cr.tag(torch.randn(8, 32), fmt, _hi(torch.randn(8, 32)))
    parts = [Cr.like(t, t[i:i + 4]) for i in (0, 4)]
    assert all(Cr.fmt_of(p) == fmt and Cr.hi_of(p) is None for p in parts)
    whole = torch.cat(parts)
    assert Cr.like(parts[0], whole) is whole and Cr.fmt_of(whole) == fmt
    assert Cr.fmt_of(Cr.like(t.view(4, 64), t.detach())) == fmt  # (the source may be a whole view)
    plain = torch.randn(8, 32)
    assert Cr.like(plain, plain[:4]).shape == (4, 32) and Cr.fmt_of(Cr.like(plain, plain[:4])) is None
    with pytest.raises(AssertionError, match="whole"):
        Cr.like(Cr.tag(torch.randn(8, 32), Cr.X2P), t[:4])


def test_refuse_names_the_format_and_passes_what_is_declared():
    x2, plain = Cr.tag(torch.randn(8, 32), Cr.X2), torch.randn(8, 32)
    mx, planar = Cr.tag(torch.randn(8, 32), Cr.MX), Cr.tag(torch.randn(8, 32), Cr.X2P)
    Cr.refuse("gemm_nt", (x2, plain, None, mx.to(torch.bfloat16)))  # an X2 tag, no tag, no tensor, another dtype: read
    with pytest.raises(RuntimeError, match="gemm_nt: got an f16mx carrier"):
        Cr.refuse("gemm_nt", (x2, None, mx))
    with pytest.raises(RuntimeError, match="f16mx"):
        Cr.refuse("gemm_nt", (mx.view(4, 64),), reads=(Cr.X2P,))
    with pytest.raises(RuntimeError, match="x2_decode: got a PLANAR bf16x2 carrier"):
        Cr.refuse("x2_decode", (torch.flatten(planar),), reads=(Cr.MX,))
    Cr.refuse("gemm_nt", (planar,), reads=(Cr.X2P,))  # the declared planar operand (a_planar=True)
    Cr.refuse("x2_decode", (mx,), reads=(Cr.MX,))
    Cr.refuse("gemm_nt", (planar[:4], mx.clone()))  # what lost its tag cannot be refused: the producers' and `like`'s job


def test_the_public_names_of_hip_ops_answer_from_the_tag():
    from wsovod_amd.layers import hip_ops as H

    assert (H.X2, H.MX) == (Cr.X2, Cr.MX)
    t = torch.randn(4, 2, 4, 4)
    hi = _hi(t)
    Cr.tag(t, Cr.MX, hi)
    flat = torch.flatten(t, start_dim=1)
    assert H.mx_of(flat) and not H.x2_planar_of(flat) and H.x2_hi_of(flat) is hi and H.x2_hi_pop(flat) is hi
    Cr.tag(t, Cr.X2P, hi[:2])
    assert H.x2_planar_of(flat) and not H.mx_of(flat) and H.x2_hi_pop(flat) is None  # (a hi of another size is not popped)
    assert not H.mx_of(None) and not H.x2_planar_of(None) and not H.mx_of(torch.randn(4))
