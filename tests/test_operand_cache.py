"""The operand cache of a weight (wsovod_amd/layers/operand_cache.py) on CPU tensors with stand-in encoders that count their
calls: when a lookup encodes, which operand the update kernels are handed, and what is current after a kernel or a graph
replay wrote the parameter behind Python's back."""
import pytest
import torch

from wsovod_amd.layers import operand_cache as OC


class Enc:
    """Stand-in encoder: a tagged copy of what it is handed; counts its calls."""

    def __init__(self, dtype=torch.float32):
        self.calls, self.dtype = 0, dtype

    def __call__(self, src):
        self.calls += 1
        return src.to(self.dtype).clone()


def _param(*shape):
    return torch.nn.Parameter(torch.randn(*shape))


def _seed_mx(p, one_scale=True, byte=True):
    """An f16mx entry as hip_ops.mx_cached leaves it: (carrier, scales), the scale byte kept on the tensor."""
    if byte:
        OC.scale_byte(p, torch.tensor([130], dtype=torch.uint8))
    return OC.lookup(p, "mx", lambda src: (src.clone(), torch.zeros(src.shape[0], 1, dtype=torch.uint8)), one_scale=one_scale)


def _written(p):
    """What an update kernel does to the parameter: new values through `.data`, the version counter untouched."""
    v = p._version
    p.data.mul_(0.5)
    assert p._version == v


@pytest.mark.parametrize("fmt,variant", [("x2", None), ("mx", None), ("x3", 1), ("bf16", torch.bfloat16)])
def test_lookup_encodes_once_per_version_and_view(fmt, variant):
    p, enc = _param(8, 32), Enc()
    a = OC.lookup(p, fmt, enc, variant=variant)
    assert enc.calls == 1 and OC.lookup(p, fmt, enc, variant=variant) is a and enc.calls == 1  # nothing changed: a hit
    assert OC.current(p, fmt, variant=variant) is a
    with torch.no_grad():
        p.add_(1.0)  # an in-place change: the version moves
    assert OC.current(p, fmt, variant=variant) is None
    b = OC.lookup(p, fmt, enc, variant=variant)
    assert enc.calls == 2 and torch.equal(b, p.detach())
    c = OC.lookup(p, fmt, enc, (4, 64), variant=variant)  # another view: another operand
    assert enc.calls == 3 and tuple(c.shape) == (4, 64)
    assert OC.lookup(p, fmt, enc, (4, 64), variant=variant) is c and enc.calls == 3
    OC.lookup(p, fmt, enc, variant=variant)  # (one entry per format: the view displaced the plain one)
    assert enc.calls == 4


def test_x3_sides_and_shadow_dtypes_are_distinct_keys():
    p, enc = _param(8, 32), Enc()
    OC.lookup(p, "x3", enc, variant=1)
    OC.lookup(p, "x3", enc, variant=0)
    assert enc.calls == 2
    half, bf = Enc(torch.float16), Enc(torch.bfloat16)
    assert OC.lookup(p, "bf16", half, variant=torch.float16).dtype == torch.float16
    assert OC.lookup(p, "bf16", bf, variant=torch.bfloat16).dtype == torch.bfloat16  # not the fp16 copy
    assert (half.calls, bf.calls) == (1, 1)


def test_a_swapped_storage_misses():
    p, enc = _param(8, 32), Enc(torch.bfloat16)
    OC.lookup(p, "bf16", enc, variant=torch.bfloat16)
    v = p._version
    p.data = p.data.clone()  # same version, other memory
    assert p._version == v and OC.current(p, "bf16", variant=torch.bfloat16) is None
    OC.lookup(p, "bf16", enc, variant=torch.bfloat16)
    assert enc.calls == 2


def test_storing_is_skipped_on_request_and_for_a_non_leaf_shadow(monkeypatch):
    from wsovod_amd.layers import functions as Fn

    casts = []
    monkeypatch.setattr(Fn.H, "cast", lambda t, cd: casts.append(cd) or t.to(cd))
    p = _param(8, 32)
    assert Fn.weight_shadow(p, torch.float32) is p and not casts  # fp32 compute: the weight itself
    sh = Fn.weight_shadow(p, torch.bfloat16)
    assert sh.dtype == torch.bfloat16 and Fn.weight_shadow(p, torch.bfloat16) is sh and len(casts) == 1
    assert OC.refreshable(p) == ("bf16", sh)
    w = p * 2.0  # a non-leaf: cast at every use, nothing kept on it
    Fn.weight_shadow(w, torch.bfloat16)
    Fn.weight_shadow(w, torch.bfloat16)
    assert len(casts) == 3 and OC.current(w, "bf16", variant=torch.bfloat16) is None
    enc = Enc()
    OC.lookup(p, "x2", enc, store=False)
    OC.lookup(p, "x2", enc, store=False)
    assert enc.calls == 2


def test_refreshable_priority_mx_over_x2_over_bf16():
    p = _param(8, 32)
    assert OC.refreshable(p) == (None, None)
    bf = OC.lookup(p, "bf16", Enc(torch.bfloat16), variant=torch.bfloat16)
    assert OC.refreshable(p) == ("bf16", bf)
    x2 = OC.lookup(p, "x2", Enc())
    fmt, sh = OC.refreshable(p)
    assert fmt == "x2" and sh is x2
    car, _ = _seed_mx(p)
    fmt, sh = OC.refreshable(p)
    assert fmt == "mx" and sh[0] is car and sh[1] is OC.scale_byte(p)  # (carrier, scale byte)
    OC.lookup(p, "x3", Enc(), variant=1)  # never refreshable: changes nothing
    assert OC.refreshable(p)[0] == "mx"


def test_what_disqualifies_an_entry_from_refresh():
    p = _param(3, 11)  # no whole 32-element blocks: neither bf16x2 nor f16mx
    OC.lookup(p, "x2", Enc())
    _seed_mx(p)
    assert OC.refreshable(p) == (None, None)
    bf = OC.lookup(p, "bf16", Enc(torch.bfloat16), variant=torch.bfloat16)
    assert OC.refreshable(p) == ("bf16", bf)  # the bf16 copy has no such condition

    p = _param(8, 32)
    _seed_mx(p, one_scale=False)  # per-row scales (a frozen weight, a fallback encode)
    assert OC.refreshable(p) == (None, None)
    p = _param(8, 32)
    _seed_mx(p, byte=False)  # no scale byte kept
    assert OC.refreshable(p) == (None, None)
    p = _param(8, 32)
    OC.lookup(p, "bf16", Enc(torch.float16), variant=torch.float16)  # an fp16 copy is cached, never handed to a kernel
    assert OC.current(p, "bf16", variant=torch.float16) is not None and OC.refreshable(p) == (None, None)

    p = _param(8, 32)  # entries with a view
    OC.scale_byte(p, torch.tensor([130], dtype=torch.uint8))
    for fmt, variant in (("mx", None), ("x2", None), ("bf16", torch.bfloat16)):
        OC.lookup(p, fmt, Enc(torch.bfloat16), (4, 64), variant=variant, **({"one_scale": True} if fmt == "mx" else {}))
    assert OC.refreshable(p) == (None, None)
    OC.replayed(p)
    assert all(OC.current(p, f, (4, 64), variant=v) is None for f, v in (("mx", None), ("x2", None), ("bf16", torch.bfloat16)))

    p = _param(8, 32)  # a stale entry
    OC.lookup(p, "x2", Enc())
    with torch.no_grad():
        p.add_(1.0)
    assert OC.refreshable(p) == (None, None)


def test_after_a_kernel_wrote_only_the_refreshed_entry_is_current():
    p = _param(8, 32)
    bf_enc, x2_enc = Enc(torch.bfloat16), Enc()
    OC.lookup(p, "bf16", bf_enc, variant=torch.bfloat16)
    x2 = OC.lookup(p, "x2", x2_enc)
    fmt, sh = OC.refreshable(p)
    assert fmt == "x2"
    _written(p)
    v = p._version
    OC.wrote(p, fmt)
    assert p._version == v + 1
    assert OC.lookup(p, "x2", x2_enc) is x2 and x2_enc.calls == 1  # re-stamped: the buffer the kernel refreshed
    OC.lookup(p, "bf16", bf_enc, variant=torch.bfloat16)  # the second format went stale
    assert bf_enc.calls == 2

    q = _param(8, 32)  # no operand handed over: only the version advances
    enc = Enc()
    OC.lookup(q, "x3", enc, variant=1)
    assert OC.refreshable(q) == (None, None)
    v = q._version
    OC.wrote(q, None)
    assert q._version == v + 1
    OC.lookup(q, "x3", enc, variant=1)
    assert enc.calls == 2
    r = _param(4)  # never cached
    OC.wrote(r, None)
    OC.replayed(r)
    assert r._version == 2


def test_wrote_restamps_the_one_scale_mx_entry_and_keeps_its_tensors():
    p = _param(8, 32)
    car, scales = _seed_mx(p)
    byte = OC.scale_byte(p)
    fmt, sh = OC.refreshable(p)
    _written(p)
    OC.wrote(p, fmt)
    assert OC.current(p, "mx") == (car, scales) and OC.current(p, "mx")[0] is car
    assert OC.refreshable(p)[0] == "mx" and OC.one_scale_mx(p)[0] is car
    with torch.no_grad():
        p.mul_(2.0)  # stale now: the carrier stays reachable for the in-place re-encode, the byte is overwritten in place
    assert OC.current(p, "mx") is None and OC.one_scale_mx(p)[0] is car
    assert OC.scale_byte(p, torch.tensor([133], dtype=torch.uint8)) is byte and int(byte) == 133
    _seed_mx(p, one_scale=False, byte=False)
    assert OC.one_scale_mx(p) is None and OC.scale_byte(p) is byte


def test_after_a_replay_every_current_refreshable_entry_hits_and_a_stale_one_stays_stale():
    p = _param(8, 32)
    bf_enc, x2_enc, x3_enc = Enc(torch.bfloat16), Enc(), Enc()
    OC.lookup(p, "x2", x2_enc)
    with torch.no_grad():
        p.add_(1.0)  # x2 is stale from here on
    bf = OC.lookup(p, "bf16", bf_enc, variant=torch.bfloat16)
    car, _ = _seed_mx(p)
    OC.lookup(p, "x3", x3_enc, variant=1)
    v = p._version
    _written(p)
    OC.replayed(p)
    assert p._version == v + 1
    assert OC.lookup(p, "bf16", bf_enc, variant=torch.bfloat16) is bf and bf_enc.calls == 1
    assert OC.current(p, "mx")[0] is car and OC.refreshable(p)[0] == "mx"
    assert OC.current(p, "x2") is None
    OC.lookup(p, "x2", x2_enc)
    OC.lookup(p, "x3", x3_enc, variant=1)  # (no kernel refreshes a split: re-split)
    assert (x2_enc.calls, x3_enc.calls) == (2, 2)


def test_a_tensor_scale_request_falls_back_to_row_scales(monkeypatch):
    """hip_ops.mx_cached: a view, or a tensor that is not 2-D contiguous with whole blocks per row, gets the per-row
    encode; that entry is cached and not refreshable."""
    from wsovod_amd.layers import hip_ops as H

    rows = []
    monkeypatch.setattr(H, "mx_encode", lambda src: rows.append(tuple(src.shape)) or (src.clone(), torch.zeros(1)))
    for p, view in ((_param(8, 32), (4, 64)), (_param(8, 40), None), (_param(2, 4, 32), None)):
        out = H.mx_cached(p, view, tensor_scale=True)
        assert H.mx_cached(p, view, tensor_scale=True) is out
        assert OC.refreshable(p) == (None, None) and OC.scale_byte(p) is None and OC.one_scale_mx(p) is None
    assert rows == [(4, 64), (8, 40), (2, 4, 32)]
