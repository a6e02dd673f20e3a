"""GPU: test-time augmentation on the device (MODEL.HIP.TTA_DEVICE).  wsovod_resample_u8 against PIL.Image.resize byte for
byte; wsovod_tta_map_boxes against _InvertibleList.inverse().apply_box and wsovod_tta_avg against its fp64 restatement bit
for bit; the device mapper against the reference's own views (golden G15); the AVG and UNION wrappers' device route against
their host route on the same seeded model."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import wsovod_ref as R
from tests.golden import gen
from tests.helpers import build_seeded_hip_model, load_golden, to_inputs
from tests.tta_cases import SOURCES, VIEW_LISTS, boxes_f32, pil_resize, source_image, targets
from wsovod_amd.data.proposals import HFlipTransform, ResizeTransform
from wsovod_amd.modeling.test_time_augmentation import _InvertibleList
from wsovod_amd.modeling.tta_device import DatasetMapperTTAAVG, DatasetMapperTTAUNION, back_map_host, back_params

pytestmark = pytest.mark.gpu

EXTRA = {(333, 500): [(480, 721), (111, 100)], (12, 17): [(7, 5)]}  # odd width; ksize 7 and 11; small odd sizes


def _resample_cases():
    for hw in SOURCES + [(12, 17)]:
        tg = [t for t in (targets(*hw) if hw in SOURCES else []) if (hw, t) != ((480, 640), (3 * 480 + 2, 3 * 640 + 1))]
        yield hw, tg + EXTRA.get(hw, [])


@pytest.mark.parametrize("hw,tg", list(_resample_cases()), ids=["%dx%d" % hw for hw, _ in _resample_cases()])
def test_resample_u8_equals_pillow(gpu, hw, tg):
    from wsovod_amd.layers import hip_ops

    img = source_image(*hw)
    dev = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).to(gpu)
    for i, (nh, nw) in enumerate(tg):
        ref = pil_resize(img, nh, nw)
        out = hip_ops.resample_u8(dev, nh, nw, True)
        assert out.shape == (2, 3, nh, nw) and out.dtype == torch.uint8 and out.is_contiguous()
        got = out.cpu().numpy().transpose(0, 2, 3, 1)
        assert np.array_equal(got[0], ref), (hw, nh, nw)
        assert np.array_equal(got[1], ref[:, ::-1]), (hw, nh, nw)
        if i % 3 == 0:  # the one-slice form
            one = hip_ops.resample_u8(dev, nh, nw, False)
            assert one.shape == (1, 3, nh, nw) and np.array_equal(one[0].cpu().numpy().transpose(1, 2, 0), ref)


def _view_lists(V):
    """V view transform lists over a 256 x 352 image: mixed sizes (non-square scales), every other one flipped."""
    sizes = [(192, 264), (1152, 1584), (300, 413), (480, 721)]
    out = []
    for v in range(V):
        nh, nw = sizes[v % len(sizes)]
        nh += v // len(sizes)
        out.append(_InvertibleList([ResizeTransform(256, 352, nh, nw)] + ([HFlipTransform(nw)] if v % 2 else [])))
    return out


def avg_restatement(view_boxes, view_scores, params):
    """wsovod_tta_avg on the host: back-map in float32, add the views in order in fp64, divide in fp64, round once."""
    R_, bc = view_boxes[0].shape
    acc_b, acc_s = np.zeros((R_, bc), np.float64), np.zeros(view_scores[0].shape, np.float64)
    for b, s, p in zip(view_boxes, view_scores, params):
        acc_b += back_map_host(b.reshape(-1, 4), p).reshape(R_, bc).astype(np.float64)
        acc_s += s.astype(np.float64)
    n = np.float64(len(view_boxes))
    return (acc_b / n).astype(np.float32), (acc_s / n).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("V", [1, 4, 16])
def test_tta_avg_equals_fp64_restatement(gpu, V):
    from wsovod_amd.layers import hip_ops

    tfms = _view_lists(V)
    params = [back_params(t) for t in tfms]
    xforms = [hip_ops.tta_xform(*p) for p in params]
    for R_ in (1, 63, 1000):
        for bc in (4, 80):
            g = torch.Generator().manual_seed(100 * V + R_ + bc)
            vb = [(boxes_f32(R_ * bc // 4, t.transforms[0].new_w, t.transforms[0].new_h, seed=7 * v + R_)).reshape(R_, bc)
                  for v, t in enumerate(tfms)]
            # scores over many magnitudes: the fp64 sum is then order-dependent, and the order is the views'
            vs = [(torch.rand((R_, 21), generator=g) * 10.0 ** torch.randint(-12, 1, (R_, 21), generator=g).float()).numpy()
                  for _ in range(V)]
            mb, ms = hip_ops.tta_avg([torch.from_numpy(b).to(gpu) for b in vb], [torch.from_numpy(s).to(gpu) for s in vs], xforms)
            wb, ws = avg_restatement(vb, vs, params)
            assert mb.shape == (R_, bc) and ms.shape == (R_, 21)
            assert np.array_equal(_bits(mb.cpu().numpy()), _bits(wb)), (V, R_, bc)
            assert np.array_equal(_bits(ms.cpu().numpy()), _bits(ws)), (V, R_, bc)


def test_tta_avg_refuses_33_views(gpu):
    from wsovod_amd import _lib
    from wsovod_amd.layers import hip_ops

    xf = hip_ops.tta_xform(False, 0, 1.5, 1.25)
    b, s = torch.zeros((8, 4), device=gpu), torch.zeros((8, 21), device=gpu)
    with pytest.raises(hip_ops.Unsupported):
        hip_ops.tta_avg([b] * 33, [s] * 33, [xf] * 33)
    table = _lib.TtaViews()  # the entry itself: a count beyond the table is refused before anything is read or launched
    table.n_views = 33
    out_b, out_s = torch.zeros_like(b), torch.zeros_like(s)
    rc = _lib.lib().wsovod_tta_avg(C.byref(table), 8, 4, 21, _lib.ptr(out_b), _lib.ptr(out_s), _lib.stream())
    assert rc == 3 and b"33 views" in _lib.lib().wsovod_last_error()
    mb, ms = hip_ops.tta_avg([b] * 32, [s] * 32, [xf] * 32)  # 32 is served
    assert not bool(mb.any()) and not bool(ms.any())


@pytest.mark.parametrize("name", sorted(VIEW_LISTS))
def test_tta_map_boxes_equals_apply_box(gpu, name):
    from wsovod_amd.layers import hip_ops

    tfm = _InvertibleList(VIEW_LISTS[name]())
    xf = hip_ops.tta_xform(*back_params(tfm))
    for M in (0, 1, 65, 1000):
        boxes = boxes_f32(M, 1584, 1152, seed=M + 1)
        got = hip_ops.tta_map_boxes(torch.from_numpy(boxes).to(gpu), xf)
        want = tfm.inverse().apply_box(boxes)
        assert got.shape == (M, 4) and np.array_equal(_bits(got.cpu().numpy()), _bits(want.astype(np.float32))), (name, M)


@pytest.fixture(scope="module")
def seeded_model(gpu):
    cfg, model, sd = build_seeded_hip_model("fp32")
    model.eval()
    return cfg, model


def _g15_setup(seeded_model, gpu):
    g = load_golden("g15_tta_avg")
    cfg, model = seeded_model
    cfg = cfg.clone()
    model.classifier = g["classifier"].to(gpu)
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST, cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST = 1e-5, 0.3
    cfg.TEST.DETECTIONS_PER_IMAGE = 100
    return g, cfg, model, to_inputs(gen.seeded_batch(1, 60, 20, 256, 352, seed=21))[0]


def test_device_mapper_matches_reference_views_golden(gpu):
    """G15: the views of the reference's own DatasetMapperTTAAVG, built on the device."""
    from wsovod_amd.modeling.meta_arch import GeneralizedRCNN_WSOVOD

    g = load_golden("g15_tta_avg")
    inp = to_inputs(gen.seeded_batch(1, 60, 20, 256, 352, seed=21))[0]
    views = DatasetMapperTTAAVG([192, 256], 4000, True, 0, device_views=gpu)(inp)
    assert len(views) == 4
    for i, v in enumerate(views):
        assert v["image"].device == gpu and v["image"].dtype == torch.uint8 and v["image"].is_contiguous()
        assert float(v["image"].double().sum()) == float(g[f"view{i}/image_checksum"])
        assert torch.equal(v["proposals"].proposal_boxes.tensor.cpu(), g[f"view{i}/proposal_boxes"])
    for a, b in ((0, 1), (2, 3)):  # a size's view and its mirror: one batch of 2 without a copy
        pair = GeneralizedRCNN_WSOVOD._adjacent([views[a]["image"], views[b]["image"]])
        assert pair is not None and pair.data_ptr() == views[a]["image"].data_ptr()
        assert torch.equal(views[b]["image"], views[a]["image"].flip(-1))


def test_tta_avg_device_route_matches_reference_golden(gpu, seeded_model):
    """G15 through the device route (views as batches of 2), at the bars of test_tta_avg_matches_reference_golden."""
    from wsovod_amd.modeling import GeneralizedRCNNWithTTAAVG

    g, cfg, model, inp = _g15_setup(seeded_model, gpu)
    tta = GeneralizedRCNNWithTTAAVG(cfg, model, DatasetMapperTTAAVG([192, 256], 4000, True, 0, device_views=gpu),
                                    batch_size=2, device_views=True)
    captured = {}
    orig = tta._average
    tta._average = lambda *a: captured.setdefault("avg", orig(*a))
    out = tta([inp])[0]["instances"]
    assert (captured["avg"][1].cpu() - g["avg_scores"]).abs().max() < 1e-4
    assert (captured["avg"][0].cpu() - g["avg_boxes"]).abs().max() < 2e-2
    assert len(out) == len(g["scores"])
    torch.testing.assert_close(out.scores.cpu(), g["scores"], rtol=1e-3, atol=1e-4)


def _wrapper_setup(seeded_model, gpu):
    cfg, model = seeded_model
    cfg = cfg.clone()
    model.classifier = torch.randn(20, 512, generator=torch.Generator().manual_seed(5)).to(gpu)
    pred = model.roi_heads.box_refinery[-1]
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST, cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST = pred.test_score_thresh, pred.test_nms_thresh
    cfg.TEST.DETECTIONS_PER_IMAGE = pred.test_topk_per_image
    return cfg, model, pred, to_inputs(gen.seeded_batch(1, 60, 20, 256, 352, seed=21))


def test_tta_avg_wrapper_device_route_equals_host_route(gpu, seeded_model, monkeypatch):
    from wsovod_amd.modeling import GeneralizedRCNNWithTTAAVG

    cfg, model, pred, batch = _wrapper_setup(seeded_model, gpu)
    runs = {}
    for route in ("host", "device"):
        dv = route == "device"
        tta = GeneralizedRCNNWithTTAAVG(cfg, model, DatasetMapperTTAAVG([192, 256], 4000, True, 0, device_views=gpu if dv else False),
                                        device_views=dv)
        assert tta.device_views is dv
        cap = runs[route] = {}
        run_model, get_boxes = tta._run_model, tta._get_augmented_boxes

        def run(views, run_model=run_model, cap=cap):  # the per-view tensors, whichever route merges them
            out, sc, bx = run_model(views)
            cap["boxes"], cap["scores"] = [b.clone() for b in bx], [s.clone() for s in sc]
            return out, sc, bx

        def get(views, tfms, get_boxes=get_boxes, cap=cap):
            cap["tfms"] = tfms
            cap["avg"] = get_boxes(views, tfms)[:2]
            return (*cap["avg"], None)

        tta._run_model, tta._get_augmented_boxes = run, get
        if dv:  # the merge stage of the device route reads nothing back
            average = tta._average

            def guarded(*a, average=average):
                with monkeypatch.context() as m:
                    def refuse(*a, **k):
                        raise AssertionError("device route copied to the host")
                    for name in ("cpu", "numpy", "tolist", "item"):
                        m.setattr(torch.Tensor, name, refuse)
                    cap["merged_on_device"] = True
                    return average(*a)

            tta._average = guarded
        cap["out"] = tta(batch)[0]["instances"]
    host, dev = runs["host"], runs["device"]
    assert len(dev["boxes"]) == 4 and dev["merged_on_device"] and "merged_on_device" not in host
    for a, b in zip(host["boxes"] + host["scores"], dev["boxes"] + dev["scores"]):  # same bytes in, same kernels
        assert torch.equal(a, b)
    params = [back_params(t) for t in dev["tfms"]]
    wb, ws = avg_restatement([b[0].cpu().numpy() for b in dev["boxes"]], [s[0].cpu().numpy() for s in dev["scores"]], params)
    assert np.array_equal(_bits(dev["avg"][0].cpu().numpy()), _bits(wb))
    assert np.array_equal(_bits(dev["avg"][1].cpu().numpy()), _bits(ws))
    # the merged detections against the oracle tail on the hand-averaged (float32 mean) host-mapped tensors
    hb = torch.stack([torch.from_numpy(t.inverse().apply_box(b[0].cpu().numpy())).float() for b, t in zip(dev["boxes"], dev["tfms"])])
    hs = torch.stack([s[0].cpu() for s in dev["scores"]])
    rb, rs, rc, _ = R.fast_rcnn_inference_single_image(hb.mean(0), hs.mean(0), (256, 352), pred.test_score_thresh,
                                                       pred.test_nms_thresh, pred.test_topk_per_image)
    out = dev["out"]
    assert torch.equal(out.pred_classes.cpu(), rc)
    torch.testing.assert_close(out.pred_boxes.tensor.cpu(), rb, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(out.scores.cpu(), rs, rtol=1e-5, atol=1e-7)


def test_tta_union_wrapper_device_route_equals_host_route(gpu, seeded_model):
    from wsovod_amd.modeling import GeneralizedRCNNWithTTAUNION

    cfg, model, pred, batch = _wrapper_setup(seeded_model, gpu)
    outs = []
    for dv in (False, True):
        mapper = DatasetMapperTTAUNION([192, 256], 4000, True, 4000, device_views=gpu if dv else False)
        outs.append(GeneralizedRCNNWithTTAUNION(cfg, model, mapper, device_views=dv)(batch)[0]["instances"])
    host, dev = outs
    assert len(host) > 0
    assert torch.equal(dev.pred_boxes.tensor, host.pred_boxes.tensor) and torch.equal(dev.scores, host.scores)
    assert torch.equal(dev.pred_classes, host.pred_classes)
