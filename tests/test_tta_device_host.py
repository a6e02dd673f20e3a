"""CPU: the host side of device test-time augmentation (MODEL.HIP.TTA_DEVICE).  The numpy restatements the device route is
built from -- Pillow's fixed-point bilinear resample (the tables wsovod_resample_u8 reads) and the float32 back-mapping of a
view's boxes -- are held against the code they restate, PIL.Image.resize and _InvertibleList.inverse().apply_box, bit for bit;
the three entries are declared and bound; the config key is off by default and leaves the host mapper as it was."""
import os
import re

import numpy as np
import pytest
import torch

from tests.tta_cases import SOURCES, VIEW_LISTS, boxes_f32, pil_resize, source_image, targets
from wsovod_amd.data.proposals import HFlipTransform, ResizeTransform
from wsovod_amd.layers.pil_resample import resample_table, resample_u8_host
from wsovod_amd.modeling.test_time_augmentation import _InvertibleList, _shortest_edge_size
from wsovod_amd.modeling.tta_device import DatasetMapperTTAAVG, back_map_host, back_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hw", SOURCES, ids=lambda s: "%dx%d" % s)
def test_resample_restatement_equals_pillow(hw):
    img = source_image(*hw)
    for nh, nw in targets(*hw):
        got = resample_u8_host(img, nh, nw)
        assert got.shape == (nh, nw, 3) and np.array_equal(got, pil_resize(img, nh, nw)), (hw, nh, nw)
    chw = np.ascontiguousarray(img.transpose(2, 0, 1))  # the plane-major form the kernel reads
    assert np.array_equal(resample_u8_host(chw, 192, 264, channels_first=True).transpose(1, 2, 0), pil_resize(img, 192, 264))


def test_resample_table_shape_and_bounds():
    for n_in, n_out in [(500, 100), (333, 111), (352, 264), (7, 22), (1, 5), (9, 1)]:
        kk, bounds, ksize = resample_table(n_in, n_out)
        assert ksize == int(np.ceil(max(n_in / n_out, 1.0))) * 2 + 1
        assert kk.shape == (n_out, ksize) and kk.dtype == np.int32 and bounds.shape == (n_out, 2) and bounds.dtype == np.int32
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ksize).all()
        assert (bounds.sum(axis=1) <= n_in).all()
        live = np.arange(ksize)[None] < bounds[:, 1:2]
        assert not kk[~live].any() and (np.abs(kk.sum(axis=1) - (1 << 22)) <= ksize).all()
    assert resample_table(500, 100)[2] == 11 and resample_table(333, 111)[2] == 7
    assert resample_table(500, 100) is resample_table(500, 100)  # cached per (in, out) pair


@pytest.mark.parametrize("name", sorted(VIEW_LISTS))
def test_back_mapping_restatement_equals_apply_box(name):
    tfm = _InvertibleList(VIEW_LISTS[name]())
    last = tfm.transforms[-1]
    w, h = (last.width, 1152) if isinstance(last, HFlipTransform) else (last.new_w, last.new_h)
    boxes = boxes_f32(257, w, h, seed=len(name))
    want = tfm.inverse().apply_box(boxes)
    got = back_map_host(boxes, back_params(tfm))
    assert want.dtype == got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_back_params_refuses_other_lists():
    assert back_params(_InvertibleList([HFlipTransform(10)])) is None
    assert back_params(_InvertibleList([HFlipTransform(10), ResizeTransform(4, 4, 8, 8)])) is None
    assert back_params(_InvertibleList([])) is None


def test_tta_entries_declared_and_bound():
    from wsovod_amd import _lib

    header = open(os.path.join(ROOT, "include", "wsovod_hip.h")).read()
    for name, nargs in (("wsovod_resample_u8", 15), ("wsovod_tta_map_boxes", 5), ("wsovod_tta_avg", 7)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 9 == _lib.lib().wsovod_abi_version()
    assert re.search(r"#define WSOVOD_TTA_MAX_VIEWS 32\b", header) and _lib.TTA_MAX_VIEWS == 32
    import ctypes as C

    assert C.sizeof(_lib.TtaXform) == 28 and C.sizeof(_lib.TtaView) == 48 and C.sizeof(_lib.TtaViews) == 8 + 32 * 48


def test_fronts_refuse_host_tensors():
    from wsovod_amd.layers import hip_ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.resample_u8(torch.zeros((3, 4, 4), dtype=torch.uint8), 2, 2, True)
    xf = hip_ops.tta_xform(True, 264, 352 / 264, 256 / 192)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.tta_map_boxes(torch.zeros((3, 4)), xf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.tta_avg([torch.zeros((3, 4))], [torch.zeros((3, 2))], [xf])
    with pytest.raises(hip_ops.Unsupported):
        hip_ops.tta_avg([torch.zeros((3, 4))] * 33, [torch.zeros((3, 2))] * 33, [xf] * 33)


def test_config_key_defaults_off_and_host_mapper_is_unchanged():
    from wsovod_amd.config import get_cfg

    cfg = get_cfg()
    assert cfg.MODEL.HIP.TTA_DEVICE is False
    cfg.TEST.AUG.MIN_SIZES, cfg.TEST.AUG.MAX_SIZE, cfg.TEST.AUG.FLIP = (192, 300), 4000, True
    mapper = DatasetMapperTTAAVG(cfg)
    assert mapper.device_views is False
    img = source_image(256, 352)
    inp = {"image": torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))), "height": 256, "width": 352}
    views = mapper(inp)
    assert len(views) == 4
    for i, v in enumerate(views):
        nh, nw = _shortest_edge_size(256, 352, (192, 300)[i // 2], 4000)
        want = pil_resize(img, nh, nw)
        want = want[:, ::-1] if i % 2 else want
        assert v["image"].device.type == "cpu" and v["image"].dtype == torch.uint8
        assert np.array_equal(v["image"].numpy(), want.transpose(2, 0, 1))
        assert [type(t) for t in v["transforms"].transforms] == [ResizeTransform] + ([HFlipTransform] if i % 2 else [])
    assert torch.equal(inp["image"], torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))))
