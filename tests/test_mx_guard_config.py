"""MODEL.HIP.MX_RANGE_GUARD on the host: the configuration keys, which precisions take a guard, the report and trip logic of
layers/mx_guard.py on a hand-filled table, the arming schedule, and the audit entry point's declaration (no GPU)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f16_bits(v):
    return int(np.array([v], dtype=np.float16).view(np.uint16)[0])


def test_config_keys_and_defaults():
    from wsovod_amd.config import get_cfg
    from wsovod_amd.testing import build_hot_path_model

    cfg = get_cfg()
    assert cfg.MODEL.HIP.MX_RANGE_GUARD == "off" and cfg.MODEL.HIP.MX_RANGE_GUARD_PERIOD == 100
    for precision in ("bf16", "parity", "parity_mx", "parity_mx_train"):
        _, model = build_hot_path_model(seed=0, precision=precision, device="cpu")
        assert model.mx_guard is None and model.mx_on == (precision in ("parity_mx", "parity_mx_train"))


def _model_with_guard(precision, mode, period=None):
    from wsovod_amd.modeling import build_model
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(precision=precision, device="cpu")
    cfg.MODEL.HIP.MX_RANGE_GUARD = mode
    if period is not None:
        cfg.MODEL.HIP.MX_RANGE_GUARD_PERIOD = period
    return build_model(cfg)


@pytest.mark.parametrize("mode", ["warn", "raise", "fallback"])
def test_guard_is_built_for_the_mx_precisions_and_refused_for_the_others(mode):
    from wsovod_amd.layers.mx_guard import MxRangeGuard

    for precision in ("parity_mx", "parity_mx_train"):
        model = _model_with_guard(precision, mode, period=7)
        g = model.mx_guard
        assert isinstance(g, MxRangeGuard) and (g.mode, g.period) == (mode, 7) and not g.armed() and not g.fallen_back
        # the modules whose outputs are audited are known by their qualified names
        assert g.names[id(model.roi_heads.box_head.fc1)] == "roi_heads.box_head.fc1"
    for precision in ("bf16", "fp32", "bf16x3", "parity", "parity_train"):
        with pytest.raises(ValueError, match="MX_RANGE_GUARD"):
            _model_with_guard(precision, mode)


def test_unknown_mode_and_bad_period_are_refused():
    with pytest.raises(ValueError, match="MX_RANGE_GUARD"):
        _model_with_guard("parity_mx", "maybe")
    with pytest.raises(ValueError, match="PERIOD"):
        _model_with_guard("parity_mx", "warn", period=0)


def test_report_and_trip_logic_on_a_hand_filled_table():
    from wsovod_amd.layers import mx_guard as G

    names = ["backbone.mx_from_x2", "backbone.res4.1.conv2", "roi_heads.pooled", "weight:fc1"]
    table = np.array([[1024, 0, 0, _f16_bits(41.5)],
                      [2048, 0, 3, _f16_bits(500.0)],
                      [4096, 2, 5, _f16_bits(65504.0)],
                      [0, 0, 0, 0]], dtype=np.int64)
    rep = G.build_report(names, table)
    assert list(rep) == names
    assert rep[names[0]] == G.SiteReport(1024, 0, 0, 41.5)
    assert rep[names[1]] == G.SiteReport(2048, 0, 3, 500.0)
    assert rep[names[2]] == G.SiteReport(4096, 2, 5, 65504.0)
    assert rep[names[3]] == G.SiteReport(0, 0, 0, 0.0)
    assert G.tripping(rep) == names[1:3]
    err = G.MxRangeError(rep)
    assert isinstance(err, RuntimeError) and err.site == names[1] and err.report is rep and names[1] in str(err)
    clean = G.build_report(names[:1], table[:1])
    assert G.tripping(clean) == [] and G.MxRangeError(clean).site is None


def test_settle_acts_by_the_mode():
    from wsovod_amd.layers import mx_guard as G

    sat = G.build_report(["a", "b"], [[10, 0, 0, 0], [10, 0, 1, _f16_bits(448.0)]])
    inf = G.build_report(["a"], [[10, 1, 0, 0]])
    ok = G.build_report(["a"], [[10, 0, 0, _f16_bits(3.0)]])
    for mode in ("warn", "raise", "fallback"):
        assert G.MxRangeGuard(mode).settle(ok) == "ok" and G.MxRangeGuard(mode).settle(ok, updated=True) == "ok"
    g = G.MxRangeGuard("warn")
    assert g.settle(sat) == "warn" and g.settle(inf) == "warn" and not g.fallen_back and g._warned == {"a", "b"}
    with pytest.raises(G.MxRangeError) as e:
        G.MxRangeGuard("raise").settle(sat)
    assert e.value.site == "b"
    g = G.MxRangeGuard("fallback")
    assert g.settle(sat) == "fallback" and g.fallen_back and not g.arm()  # (sticky: never armed again)
    g = G.MxRangeGuard("fallback")
    assert g.settle(sat, updated=True) == "fallback" and g.fallen_back
    # a non-finite value that went into an applied update raises in every mode
    for mode in ("warn", "raise", "fallback"):
        with pytest.raises(G.MxRangeError, match="non-finite"):
            G.MxRangeGuard(mode).settle(inf, updated=True)
    # ... but an armed step that only accumulated gradients (no update yet) follows the mode
    assert G.MxRangeGuard("warn").settle(inf, updated=False, training=True) == "warn"
    assert G.MxRangeGuard("fallback").settle(inf, updated=False, training=True) == "fallback"
    with pytest.raises(G.MxRangeError) as e:
        G.MxRangeGuard("raise").settle(inf, updated=False, training=True)
    assert "already applied" not in str(e.value)
    with pytest.raises(ValueError):
        G.MxRangeGuard("off")


def test_training_steps_are_armed_first_and_every_period():
    from wsovod_amd.layers import mx_guard as G

    g = G.MxRangeGuard("warn", period=3)
    armed = []
    for _ in range(7):
        armed.append(g.begin_step())
        g.arm(False)
    assert armed == [True, False, False, True, False, False, True]
    g.begin_step()   # (step 7: not due)
    assert not g.armed()
    g.rearm()        # a state dict was loaded
    assert g.begin_step() and not g.arm(False)
    assert [g.begin_step() for _ in range(3)] == [False, False, True]


def test_state_dict_load_rearms_the_models_guard():
    model = _model_with_guard("parity_mx", "warn", period=50)
    g = model.mx_guard
    assert g.begin_step()
    g.arm(False)
    assert not g.begin_step()
    model.load_state_dict(model.state_dict())
    assert g.begin_step()


def test_audit_without_an_armed_active_guard_launches_nothing(monkeypatch):
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd.layers import mx_guard as G

    calls = []
    monkeypatch.setattr(H, "mx_range", lambda *a, **k: calls.append(a))
    x = torch.zeros(4, 32)
    G.audit("site", x)  # no active guard
    g = G.MxRangeGuard("warn")
    with G.active(g):
        assert not G.launching()
        G.audit("site", x)  # active, not armed
        g.arm()
        assert G.launching()
        G.audit("site", x)
        G.audit("site", x)
        G.audit("other", x)
    assert not G.launching()
    G.audit("site", x)  # armed, no longer active
    assert len(calls) == 3 and list(g.sites) == ["site", "other"]
    assert g.table.shape == (G.MAX_SITES, 4) and g.table.dtype == torch.int64
    assert calls[0][1].data_ptr() == calls[1][1].data_ptr() == g.table[0].data_ptr() and calls[2][1].data_ptr() == g.table[1].data_ptr()
    g.table[0] = torch.tensor([64, 0, 0, _f16_bits(2.5)])
    rep = g.poll()
    assert rep["site"] == G.SiteReport(64, 0, 0, 2.5) and rep["other"].audited == 0 and g.totals["site"] == 64 and g.polls == 1
    g.reset()
    assert g.poll()["site"].audited == 0 and g.totals["site"] == 64


def test_audit_entry_point_is_declared_and_exported():
    from wsovod_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "wsovod_hip.h")).read()
    m = re.search(r"\bint\s+wsovod_f16mx_range\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m is not None and m.group(1).count(",") + 1 == len(_lib.SIGNATURES["wsovod_f16mx_range"]) == 6
    assert "box_head.py:60-75" in hdr[max(0, m.start() - 1200):m.start()] and "resnet_wsl.py:94-110" in hdr[max(0, m.start() - 1200):m.start()]
    assert hasattr(_lib.lib(), "wsovod_f16mx_range")
    assert _lib.ABI_VERSION == 9


def test_audit_arguments_are_checked_before_any_launch():
    import ctypes as C

    from wsovod_amd import _lib

    L = _lib.lib()
    buf = (C.c_char * 256)()
    cnt = (C.c_longlong * 4)()
    src, ctr = C.addressof(buf), C.addressof(cnt)
    src += (-src) % 16
    assert L.wsovod_f16mx_range(src, 32, 0, 32, ctr, None) == 0       # rows == 0: a no-op
    assert L.wsovod_f16mx_range(None, 32, 0, 64, None, None) == 0
    assert L.wsovod_f16mx_range(src, 32, 1, 48, ctr, None) != 0       # cols not a multiple of 32
    assert L.wsovod_f16mx_range(src, 16, 1, 32, ctr, None) != 0       # ld < cols
    assert L.wsovod_f16mx_range(src, 34, 1, 32, ctr, None) != 0       # rows not 16-byte aligned
    assert L.wsovod_f16mx_range(None, 32, 1, 32, ctr, None) != 0
    assert L.wsovod_f16mx_range(src, 32, 1, 32, None, None) != 0
    assert L.wsovod_f16mx_range(src + 4, 32, 1, 32, ctr, None) != 0   # misaligned source
    assert L.wsovod_f16mx_range(src, 32, -1, 32, ctr, None) != 0
    assert list(cnt) == [0, 0, 0, 0]
