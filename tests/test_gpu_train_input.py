"""GPU: the training input stage on the device (MODEL.HIP.INPUT_DEVICE).  wsovod_resample_u8_batch against PIL.Image.resize byte
for byte (both source layouts, an odd canvas width, the padding zeroed) and against wsovod_resample_u8 image by image;
wsovod_transform_proposals against data/proposals.py:transform_proposals bit for bit; DeviceTrainInput against HostTrainInput on
the same records and draws, through `_canvas` (no copy) and one training step.  Everything is integer or single-operation
float32 arithmetic: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import build_seeded_hip_model
from tests.train_input_cases import collision_boxes, input_cfg, logits_for, raw_record, segment, special_boxes
from tests.tta_cases import pil_resize, source_image
from wsovod_amd.data.proposals import HFlipTransform, ResizeTransform, TransformList, transform_proposals
from wsovod_amd.data.train_input import DeviceTrainInput, HostTrainInput

pytestmark = pytest.mark.gpu

# (source h, w) -> (nh, nw), flip: up from one pixel; both axes kept (the copy path); the 0 / 255 pattern one axis up and one
# down, mirrored; both axes down; a wide ksize (200 -> 13: 33 taps) with the height kept.  Wp = 31 is odd.
RESAMPLE = [((1, 1), (3, 2), False), ((5, 7), (5, 7), False), ((37, 53), (61, 29), True), ((48, 64), (24, 31), False),
            ((9, 200), (9, 13), True)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _dev_images(gpu, layout):
    out = []
    for g, ((h, w), _, _) in enumerate(RESAMPLE):
        img = source_image(h, w)
        inter = layout == "interleaved" or (layout == "mixed" and g % 2 == 0)
        out.append((torch.from_numpy(img if inter else np.ascontiguousarray(img.transpose(2, 0, 1))).to(gpu), inter))
    return out


@pytest.mark.parametrize("layout", ["interleaved", "planar", "mixed"])
def test_resample_batch_equals_pillow_and_the_single_image_entry(gpu, layout):
    from wsovod_amd.layers import hip_ops

    imgs = _dev_images(gpu, layout)
    Hp, Wp = max(t[0] for _, t, _ in RESAMPLE), max(t[1] for _, t, _ in RESAMPLE)
    assert (Hp, Wp) == (61, 31) and Wp % 2 == 1
    canvas = torch.full((len(RESAMPLE), 3, Hp, Wp), 0xAB, dtype=torch.uint8, device=gpu)
    got = hip_ops.resample_u8_batch([t for t, _ in imgs], [t for _, t, _ in RESAMPLE], [f for _, _, f in RESAMPLE],
                                    interleaved=[i for _, i in imgs], out=canvas)
    assert got.data_ptr() == canvas.data_ptr()
    host = canvas.cpu().numpy()
    for g, ((h, w), (nh, nw), flip) in enumerate(RESAMPLE):
        ref = pil_resize(source_image(h, w), nh, nw)
        ref = ref[:, ::-1] if flip else ref
        assert np.array_equal(host[g, :, :nh, :nw], ref.transpose(2, 0, 1)), (g, layout)
        pad = host[g].copy()
        pad[:, :nh, :nw] = 0
        assert not pad.any(), (g, layout)  # every byte outside nh x nw is 0, none left at 0xAB
        chw = torch.from_numpy(np.ascontiguousarray(source_image(h, w).transpose(2, 0, 1))).to(gpu)
        one = hip_ops.resample_u8(chw, nh, nw, True)[1 if flip else 0]
        assert torch.equal(canvas[g, :, :nh, :nw], one), (g, layout)


def test_resample_batch_limit(gpu):
    """33 images are refused by the entry; the front serves them as 32 + 1 (the canvas is 4-byte aligned again there)."""
    from wsovod_amd import _lib
    from wsovod_amd.layers import hip_ops

    table = _lib.ResampleBatch()
    table.n = 33
    out = torch.zeros((64,), dtype=torch.uint8, device=gpu)
    rc = _lib.lib().wsovod_resample_u8_batch(C.byref(table), None, 0, None, 0, _lib.ptr(out), 4, 4, _lib.stream())
    assert rc == 3 and b"33 images" in _lib.lib().wsovod_last_error()
    img = source_image(5, 7)
    dev = torch.from_numpy(img).to(gpu)
    sizes = [(3 + g % 3, 5 + g % 2) for g in range(33)]
    canvas = hip_ops.resample_u8_batch([dev] * 33, sizes, [g % 2 == 1 for g in range(33)], interleaved=True).cpu().numpy()
    assert canvas.shape == (33, 3, 5, 6)
    for g in (0, 1, 31, 32):
        nh, nw = sizes[g]
        ref = pil_resize(img, nh, nw)
        ref = ref[:, ::-1] if g % 2 else ref
        assert np.array_equal(canvas[g, :, :nh, :nw], ref.transpose(2, 0, 1)), g
        assert not canvas[g, :, nh:].any() and not canvas[g, :, :, nw:].any()


def _proposal_segments():
    """(raw boxes, h, w, nh, nw) per image: lengths 1, 63, 64, 65 and 4100, the hash collision in a frame wider than 1000, and
    an image all of whose boxes die."""
    segs = []
    for n, (h, w, nh, nw) in zip((1, 63, 64, 65), ((37, 53, 61, 29), (48, 64, 24, 31), (37, 53, 74, 106), (50, 80, 50, 80))):
        segs.append((segment(n, w, h, seed=n, sx=nw / w, sy=nh / h), h, w, nh, nw))
    segs.append((segment(4100, 640, 480, seed=4100, sx=800 / 640, sy=600 / 480), 480, 640, 600, 800))
    segs.append((collision_boxes(), 50, 1200, 50, 1200))
    segs.append((special_boxes(53, 37)[8:13], 37, 53, 37, 53))  # wholly outside or zero-sized: count 0
    return segs


def _host_proposals(raw, logits, h, w, nh, nw, flip, topk):
    d = {"proposal_boxes": raw.copy(), "proposal_objectness_logits": logits.copy(), "proposal_bbox_mode": 0}
    tf = TransformList([ResizeTransform(h, w, nh, nw)] + ([HFlipTransform(nw)] if flip else []))
    transform_proposals(d, (nh, nw), tf, proposal_topk=topk)
    return d["proposals"].proposal_boxes.tensor.numpy(), d["proposals"].objectness_logits.numpy()


@pytest.mark.parametrize("topk", [4000, 50])
@pytest.mark.parametrize("flip", [False, True])
def test_transform_proposals_equals_the_host(gpu, flip, topk):
    from wsovod_amd.layers import hip_ops

    segs = _proposal_segments()
    logits = [logits_for(len(s[0]), seed=i) for i, s in enumerate(segs)]
    boxes_d = torch.from_numpy(np.concatenate([s[0] for s in segs])).to(gpu)
    logits_d = torch.from_numpy(np.concatenate(logits)).to(gpu)
    table, r0 = [], 0
    for raw, h, w, nh, nw in segs:
        table.append((r0, len(raw), h, w, nh, nw, flip))
        r0 += len(raw)
    runs = [tuple(t.cpu().numpy() for t in hip_ops.transform_proposals(boxes_d, logits_d, table, topk)) for _ in range(2)]
    for a, b in zip(*runs):  # the same bytes from either call, the rows behind the counts included
        assert a.tobytes() == b.tobytes()
    out_boxes, out_logits, counts = runs[0]
    assert out_boxes.shape == (len(segs), topk, 4) and counts.dtype == np.int32
    lengths = []
    for g, ((raw, h, w, nh, nw), lg) in enumerate(zip(segs, logits)):
        want_b, want_l = _host_proposals(raw, lg, h, w, nh, nw, flip, topk)
        n = int(counts[g])
        assert n == len(want_b), (g, n, len(want_b))
        assert np.array_equal(_bits(out_boxes[g, :n]), _bits(want_b)), g
        assert np.array_equal(_bits(out_logits[g, :n]), _bits(want_l)), g
        assert not out_boxes[g, n:].any() and not out_logits[g, n:].any()
        lengths.append(n)
    assert lengths[-1] == 0 and lengths[0] == 1  # an image all of whose boxes die
    assert lengths[-2] == (5 if flip else 4)  # of the six collision rows (tests/train_input_cases.py)
    assert lengths[4] == topk  # 4072 rows survive the dedupe: the cut comes behind it
    assert lengths[1] == 46  # duplicates and empties were dropped from the 63


@pytest.fixture(scope="module")
def mapped(gpu):
    """Three records of different sizes through both routes on the same draws."""
    cfg = input_cfg(min_sizes=(96, 112, 128, 144), max_size=200, topk=120)
    records = [raw_record(75, 100, 300, seed=1), raw_record(96, 128, 90, seed=2, classes=(5,)), raw_record(122, 80, 41, seed=3)]
    host, dev = HostTrainInput(cfg), DeviceTrainInput(cfg, gpu)
    return cfg, records, host, dev, host(records, np.random.RandomState(11)), dev(records, np.random.RandomState(11))


def _assert_same_batch(want, got, gpu, on_device=True):
    assert len(want) == len(got)
    for a, b in zip(want, got):
        assert b["image"].is_cuda == on_device and tuple(b["image"].shape) == tuple(a["image"].shape)
        assert torch.equal(b["image"].cpu(), a["image"])
        assert (b["height"], b["width"], b["file_name"]) == (a["height"], a["width"], a["file_name"])
        pa, pb = a["proposals"], b["proposals"]
        assert pb.image_size == pa.image_size and len(pb) == len(pa)
        assert pb.proposal_boxes.tensor.is_cuda == on_device
        assert np.array_equal(_bits(pb.proposal_boxes.tensor.cpu().numpy()), _bits(pa.proposal_boxes.tensor.numpy()))
        assert np.array_equal(_bits(pb.objectness_logits.cpu().numpy()), _bits(pa.objectness_logits.numpy()))
        assert not b["instances"].gt_classes.is_cuda and torch.equal(b["instances"].gt_classes, a["instances"].gt_classes)
        assert b["instances"].image_size == a["instances"].image_size
        assert not any(k in b for k in ("annotations", "proposal_boxes", "proposal_objectness_logits"))


def test_device_mapper_equals_host_mapper(gpu, mapped):
    cfg, records, host, dev, want, got = mapped
    assert dev.last_route == "device"
    _assert_same_batch(want, got, gpu)
    sizes = {tuple(o["image"].shape[1:]) for o in got}
    assert len(sizes) == 3 and len({len(o["proposals"]) for o in got}) > 1 and max(len(o["proposals"]) for o in got) == 120
    assert tuple(dev.canvas.shape) == (3, 3, max(s[0] for s in sizes), max(s[1] for s in sizes))


def test_canvas_is_handed_on_without_a_copy(gpu, mapped):
    from wsovod_amd.modeling.meta_arch import GeneralizedRCNN_WSOVOD as M

    cfg, records, host, dev, want, got = mapped
    images = [o["image"] for o in got]
    sizes = [tuple(im.shape[1:]) for im in images]
    Hp, Wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
    canvas = M._padded_views(images, sizes, Hp, Wp, gpu)
    assert canvas is not None and canvas.data_ptr() == dev.canvas.data_ptr() and tuple(canvas.shape) == (3, 3, Hp, Wp)
    # what exists today takes the path it takes today: host images, device copies, another order, an unmarked canvas
    assert M._padded_views([o["image"] for o in want], sizes, Hp, Wp, gpu) is None
    assert M._padded_views([im.clone() for im in images], sizes, Hp, Wp, gpu) is None
    assert M._padded_views(images[::-1], sizes[::-1], Hp, Wp, gpu) is None
    plain = dev.canvas.clone()
    assert M._padded_views([plain[g, :, :h, :w] for g, (h, w) in enumerate(sizes)], sizes, Hp, Wp, gpu) is None


def test_float64_boxes_fall_back_to_the_host_route(gpu, mapped):
    cfg, records, host, dev, _, _ = mapped
    odd = [dict(r) for r in records]
    odd[1]["proposal_boxes"] = odd[1]["proposal_boxes"].astype(np.float64)
    other = DeviceTrainInput(cfg, gpu)
    got = other(odd, np.random.RandomState(11))
    assert other.last_route == "host" and other.canvas is None
    _assert_same_batch(host(odd, np.random.RandomState(11)), got, gpu, on_device=False)


def test_training_step_losses_equal_from_either_route(gpu, mapped):
    """One R18 training step at plumbing size: the device route's batch goes through `_canvas` without a copy and gives the
    losses of the host route's batch bit for bit."""
    cfg, records, host, dev, want, got = mapped
    _, model, _ = build_seeded_hip_model("fp32")
    seen = []
    canvas_of = model._canvas
    model._canvas = lambda batch: seen.append(canvas_of(batch)) or seen[-1]
    losses = []
    for batch in (want, got):
        model.roi_heads.iter = 0
        out = model(batch)
        losses.append({k: float(v.detach()) for k, v in out.items()})
    assert seen[1][0].data_ptr() == dev.canvas.data_ptr() and seen[0][0].data_ptr() != dev.canvas.data_ptr()
    assert torch.equal(seen[0][0], seen[1][0]) and seen[0][2] == seen[1][2]
    assert losses[0].keys() == losses[1].keys() and len(losses[0]) > 0
    for k in losses[0]:
        assert np.isfinite(losses[0][k]) and losses[0][k] == losses[1][k], (k, losses[0][k], losses[1][k])
