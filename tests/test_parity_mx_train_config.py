"""MODEL.HIP.PRECISION = "parity_mx_train" on the host: what the name maps to in every module that reads it, and the
operand-cache format of the mode's transposed weight operand (pure torch: no GPU, no HIP library)."""
import pytest
import torch


@pytest.mark.parametrize("name,want", [
    ("parity", ("parity", False, False)), ("parity_mx", ("parity", True, False)), ("parity_train", ("parity", False, True)),
    ("parity_mx_train", ("parity", True, True)), ("bf16", ("bf16", False, False))])
def test_precision_name_maps_to_forward_precision_and_flags(name, want):
    """Every module sees the forward precision; the meta-arch holds the two flags: "parity_mx_train" = ("parity", the f16mx
    kernels, the backward split)."""
    from wsovod_amd.modeling.backbone import forward_precision
    from wsovod_amd.testing import build_hot_path_model

    cfg, model = build_hot_path_model(seed=0, precision=name, device="cpu")
    assert cfg.MODEL.HIP.PRECISION == name and forward_precision(name) == want[0]
    assert (model.backbone.precision, model.mx, model.backward_split) == want
    assert model.roi_heads.precision == want[0]
    assert model.x3 == ("x2" if want[0] == "parity" else False)


def test_unknown_precision_name_is_not_mapped():
    """A name the project does not know is handed through unchanged, as before: no composite mapping, neither flag."""
    from wsovod_amd.modeling.backbone import forward_precision
    from wsovod_amd.testing import build_hot_path_model

    assert forward_precision("parity_mx_trainx") == "parity_mx_trainx"
    cfg, model = build_hot_path_model(seed=0, precision="parity_mx_trainx", device="cpu")
    assert (model.backbone.precision, model.roi_heads.precision) == ("parity_mx_trainx",) * 2
    assert not model.mx and not model.backward_split and model.x3 is False


def test_backward_split_route_switches(monkeypatch):
    from wsovod_amd.layers import functions as Fn

    monkeypatch.delenv("WSOVOD_PT_DX", raising=False)
    monkeypatch.delenv("WSOVOD_PT_SPLIT", raising=False)
    assert Fn._pt_dx() == "x2" and Fn._bwd_split() == frozenset()
    with Fn.backward_split(True):
        assert Fn._bwd_split() == frozenset({"dx"})
        monkeypatch.setenv("WSOVOD_PT_SPLIT", "dw,dx")
        assert Fn._bwd_split() == frozenset({"dw", "dx"})
    monkeypatch.setenv("WSOVOD_PT_DX", "x3")
    assert Fn._pt_dx() == "x3"


def test_transposed_operand_is_cached_by_version_and_never_restamped():
    """The "x2t" entry of layers/operand_cache.py: hit while the tensor stands, miss after an in-place change; the update
    kernels do not refresh it, so `wrote` and `replayed` drop it while they re-stamp the operand the kernel did refresh."""
    from wsovod_amd.layers import operand_cache as oc

    w = torch.nn.Parameter(torch.randn(8, 32))
    n = [0]

    def enc(src):
        n[0] += 1
        return src.t().contiguous()

    a = oc.lookup(w, "x2t", enc)
    assert oc.lookup(w, "x2t", enc) is a and n[0] == 1 and oc.current(w, "x2t") is a
    x2 = oc.lookup(w, "x2", lambda src: src.clone())
    with torch.no_grad():
        w.add_(1.0)
    assert oc.current(w, "x2t") is None and oc.current(w, "x2") is None
    b = oc.lookup(w, "x2t", enc)
    x2 = oc.lookup(w, "x2", lambda src: src.clone())
    assert n[0] == 2 and torch.equal(b, w.detach().t())
    oc.wrote(w, "x2")  # (an eager update kernel refreshed the bf16x2 operand in its pass)
    assert oc.current(w, "x2") is x2 and oc.current(w, "x2t") is None
    c = oc.lookup(w, "x2t", enc)
    oc.replayed(w)  # (a replayed step graph did the same)
    assert oc.current(w, "x2") is x2 and oc.current(w, "x2t") is None and c is not None
