"""layers/precision.py on the host: the table of MODEL.HIP.PRECISION names, the state every model entry point enters for each
of them, and the scopes of the per-thread state (pure torch: no GPU, no HIP library)."""
import ast
import threading

import pytest

# name -> (forward, x3, x3_float_entry, mx, bwd_split)
ROWS = {
    "bf16": ("bf16", False, False, False, False),
    "fp32": ("fp32", False, False, False, False),
    "bf16x3": ("bf16x3", "full", "full", False, False),
    "bf16x3f": ("bf16x3f", "fwd", "fwd", False, False),
    "parity": ("parity", "x2", "fwd", False, False),
    "parity_train": ("parity", "x2", "fwd", False, True),
    "parity_mx": ("parity", "x2", "fwd", True, False),
    "parity_mx_train": ("parity", "x2", "fwd", True, True),
    "no_such_precision": ("no_such_precision", False, False, False, False),
}
DEFAULTS = (False, False, False)


def _state():
    from wsovod_amd.layers import precision as P

    return P.x3_active(), P.mx_active(), bool(P._bwd_split())


def test_module_imports_torch_only():
    from wsovod_amd.layers import precision as P

    tree = ast.parse(open(P.__file__).read())
    mods = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    mods |= {("." * n.level) + (n.module or "") for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert mods == {"os", "threading", "dataclasses", "torch"}


@pytest.mark.parametrize("name", list(ROWS))
def test_table_rows(name):
    import dataclasses

    import torch

    from wsovod_amd.layers import precision as P
    from wsovod_amd.modeling.backbone import forward_precision

    p = P.of(name)
    assert (p.name, p.forward, p.x3, p.x3_float_entry, p.mx, p.bwd_split) == (name,) + ROWS[name]
    assert p.compute_dtype == (torch.bfloat16 if name == "bf16" else torch.float32)
    assert forward_precision(name) == ROWS[name][0]
    assert (name in P.TABLE) == (name != "no_such_precision") and (name not in P.TABLE or P.TABLE[name] is p)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.mx = True


def test_the_one_table_feeds_the_guard_and_the_old_names():
    from wsovod_amd.layers import functions as Fn
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.layers import mx_guard
    from wsovod_amd.layers import precision as P

    assert list(P.TABLE) == list(ROWS)[:-1]
    assert mx_guard.MX_PRECISIONS == ("parity_mx", "parity_mx_train")
    assert (H.x3_mode, H.mx_mode, H.x3_active, H.mx_active, H.x2_active) == (P.x3_mode, P.mx_mode, P.x3_active, P.mx_active, P.x2_active)
    assert (Fn.backward_split, Fn._bwd_split, Fn._pt_dx, Fn._no_split) == (P.backward_split, P._bwd_split, P._pt_dx, P._no_split)


def _recorded(model):
    """The three entry points of `model` with their bodies replaced by recorders -> {entry point: state seen inside}."""
    seen = {}
    for entry in ("forward_frozen", "forward_trainable", "inference"):
        setattr(model, "_" + entry, lambda *a, _e=entry, **k: seen.__setitem__(_e, _state()))
    model.forward_frozen([])
    model.forward_trainable({})
    model.eval().inference([])
    assert _state() == DEFAULTS
    return seen


@pytest.mark.parametrize("name", list(ROWS))
def test_entry_points_enter_the_records_state(name, monkeypatch):
    from wsovod_amd.testing import build_hot_path_model

    monkeypatch.delenv("WSOVOD_PT_SPLIT", raising=False)
    _, x3, _, mx, split = ROWS[name]
    _, model = build_hot_path_model(seed=0, precision=name, device="cpu")
    assert (model.x3, model.mx, model.backward_split, model.mx_on) == (x3, mx, split, mx)
    assert _recorded(model) == {"forward_frozen": (x3, mx, False), "forward_trainable": (x3, mx, split), "inference": (x3, mx, False)}


@pytest.mark.parametrize("name", ["parity_mx", "parity_mx_train"])
def test_a_guard_that_fell_back_switches_the_f16mx_kernels_off_everywhere(name, monkeypatch):
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    monkeypatch.delenv("WSOVOD_PT_SPLIT", raising=False)
    cfg = hot_path_cfg(precision=name, device="cpu")
    cfg.MODEL.HIP.MX_RANGE_GUARD = "fallback"
    model = build_model(cfg)
    split = ROWS[name][4]
    # the guard stands: every entry point selects the f16mx kernels (inference through its audited branch)
    assert _recorded(model) == {"forward_frozen": ("x2", True, False), "forward_trainable": ("x2", True, split),
                                "inference": ("x2", True, False)}
    model.mx_guard.fallen_back = True
    assert model.mx and not model.mx_on
    assert _recorded(model) == {"forward_frozen": ("x2", False, False), "forward_trainable": ("x2", False, split),
                                "inference": ("x2", False, False)}


def test_model_without_a_cfg_takes_the_backbones_precision():
    from wsovod_amd.modeling.meta_arch import GeneralizedRCNN_WSOVOD
    from wsovod_amd.testing import build_hot_path_model

    _, built = build_hot_path_model(seed=0, precision="parity_mx", device="cpu")
    model = GeneralizedRCNN_WSOVOD(backbone=built.backbone, proposal_generator=None, roi_heads=built.roi_heads,
                                   pixel_mean=(0.0, 0.0, 0.0), pixel_std=(1.0, 1.0, 1.0))
    assert built.backbone.precision == "parity" and (model.x3, model.mx, model.backward_split) == ("x2", False, False)


def test_scopes_nest_and_override(monkeypatch):
    from wsovod_amd.layers import precision as P

    monkeypatch.delenv("WSOVOD_PT_SPLIT", raising=False)
    assert _state() == DEFAULTS
    with P.scope(P.of("parity_mx_train")):
        assert _state() == ("x2", True, True) and P.x2_active()
        with P.scope(P.of("parity_mx_train"), mx=False, bwd_split=False):
            assert _state() == ("x2", False, False)
            with P.mx_mode(True), P.backward_split():
                assert _state() == ("x2", True, True)
            assert _state() == ("x2", False, False)
        with P.x3_mode("fwd"):  # the f16mx kernels are selected in the "x2" mode only
            assert _state() == ("fwd", False, True) and not P.x2_active()
            with P.scope(P.of("bf16"), mx=True):
                assert _state() == DEFAULTS
            assert _state() == ("fwd", False, True)
        with P.x3_mode():
            assert P.x3_active() == "full"
        with P.x3_mode(0):
            assert P.x3_active() is False
        assert _state() == ("x2", True, True)
    assert _state() == DEFAULTS


def test_scopes_restore_after_an_exception():
    from wsovod_amd.layers import precision as P

    for make in (lambda: P.scope(P.of("parity_mx_train")), lambda: P.x3_mode("x2"), P.mx_mode, P.backward_split):
        with pytest.raises(ZeroDivisionError):
            with P.scope(P.of("bf16x3")), make():
                1 / 0
        assert _state() == DEFAULTS


def test_a_second_thread_sees_the_defaults():
    from wsovod_amd.layers import precision as P

    seen = []

    def other():
        seen.append(_state())
        with P.scope(P.of("bf16x3")):  # ... and what it enters stays its own
            seen.append(_state())

    with P.scope(P.of("parity_mx_train")):
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert _state() == ("x2", True, True)
    assert seen == [DEFAULTS, ("full", False, False)]
