"""GPU: the random crop of the training input stage on the device (MODEL.HIP.INPUT_CROP).  wsovod_resample_u8_batch_win against
PIL.Image.resize of the numpy slice byte for byte (unaligned window starts, an odd pitch, the corner window, both layouts, the
paths that read the source directly, an odd canvas width, the padding zeroed); wsovod_transform_proposals_win against
data/proposals.py:transform_proposals under TransformList([Crop, Resize, HFlip]) bit for bit; DeviceTrainInput against
HostTrainInput under crop, through `_canvas` (no copy) and one training step.  Integer or single-operation float32 arithmetic:
every comparison is exact."""
import numpy as np
import pytest
import torch

from tests.helpers import build_seeded_hip_model
from tests.train_input_cases import logits_for, special_boxes
from tests.train_input_crop_cases import (ANNOTATION_FATE, annotated_record, crop_cfg, crop_list, cropped_segment, raw_record,
                                          shifted_collision)
from tests.tta_cases import pil_resize, source_image
from wsovod_amd.data.proposals import transform_proposals
from wsovod_amd.data.train_input import DeviceTrainInput, HostTrainInput

pytestmark = pytest.mark.gpu

# source (h, w), planar, window (y0, x0, ch, cw) or None, (nh, nw), flip.  Wp = 31 is odd.
WINDOWS = [
    ((37, 53), False, (2, 1, 30, 47), (45, 31), False),   # x0 = 1 of a 53-wide interleaved source: odd pitch, unaligned start
    ((48, 64), False, (20, 40, 28, 24), (14, 12), True),  # the bottom-right corner: src_bytes exact to the byte; mirrored
    ((5, 7), False, (3, 4, 1, 1), (3, 2), False),         # a 1 x 1 window up to 3 x 2
    ((48, 64), False, (4, 3, 20, 25), (33, 25), True),    # keeps its width: the vertical pass reads the source; mirrored
    ((48, 64), False, (5, 6, 17, 19), (17, 19), False),   # keeps both sizes: a windowed copy
    ((37, 53), True, (3, 5, 20, 31), (25, 18), True),     # a plane-major source; mirrored
    ((9, 200), True, (1, 7, 8, 190), (8, 13), False),     # plane-major, the height kept, a wide ksize
    ((48, 64), False, None, (24, 31), False),             # the whole image as a window
]
OUTSIDE = 0x5A


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _windowed_source(h, w, win):
    """The seeded image inside the window, another pattern everywhere outside it."""
    img = source_image(h, w)
    if win is None:
        return img
    y0, x0, ch, cw = win
    out = np.full_like(img, OUTSIDE)
    out[::2, 1::2] = 255 - OUTSIDE
    out[y0:y0 + ch, x0:x0 + cw] = img[y0:y0 + ch, x0:x0 + cw]
    return out


def test_windowed_resize_equals_pillow_of_the_slice(gpu):
    from wsovod_amd.layers import hip_ops

    srcs = [_windowed_source(h, w, win) for (h, w), _, win, _, _ in WINDOWS]
    dev = [torch.from_numpy(np.ascontiguousarray(s.transpose(2, 0, 1)) if planar else s).to(gpu)
           for s, (_, planar, _, _, _) in zip(srcs, WINDOWS)]
    Hp, Wp = max(t[3][0] for t in WINDOWS), max(t[3][1] for t in WINDOWS)
    assert (Hp, Wp) == (45, 31)
    assert (3 * (2 * 53 + 1)) % 4 != 0 and (3 * 53) % 2 == 1  # the first window's start and pitch
    canvas = torch.full((len(WINDOWS), 3, Hp, Wp), 0xAB, dtype=torch.uint8, device=gpu)
    kw = dict(interleaved=[not t[1] for t in WINDOWS], windows=[t[2] for t in WINDOWS])
    got = hip_ops.resample_u8_batch(dev, [t[3] for t in WINDOWS], [t[4] for t in WINDOWS], out=canvas, **kw)
    assert got.data_ptr() == canvas.data_ptr()
    host = canvas.cpu().numpy()
    for g, (src, (_, planar, win, (nh, nw), flip)) in enumerate(zip(srcs, WINDOWS)):
        y0, x0, ch, cw = win if win is not None else (0, 0) + src.shape[:2]
        ref = pil_resize(np.ascontiguousarray(src[y0:y0 + ch, x0:x0 + cw]), nh, nw)
        ref = ref[:, ::-1] if flip else ref
        assert np.array_equal(host[g, :, :nh, :nw], ref.transpose(2, 0, 1)), g
        pad = host[g].copy()
        pad[:, :nh, :nw] = 0
        assert not pad.any(), g  # every byte outside nh x nw is 0, none left at 0xAB
    # the whole image as a window gives the bytes of the entry without windows
    g = len(WINDOWS) - 1
    plain = hip_ops.resample_u8_batch(dev[g:], [WINDOWS[g][3]], [WINDOWS[g][4]], interleaved=True)
    assert torch.equal(plain[0], canvas[g, :, :WINDOWS[g][3][0], :WINDOWS[g][3][1]])
    # the same bytes from a second call
    again = hip_ops.resample_u8_batch(dev, [t[3] for t in WINDOWS], [t[4] for t in WINDOWS], **kw)
    assert torch.equal(again, canvas)


def _proposal_segments():
    """(raw boxes, crop (x0, y0, cw, ch), nh, nw) per image: lengths 1, 63, 64, 65 and 4100 around small windows of larger
    sources, the hash collision shifted into a window wider than 1000, and a window that no box touches."""
    segs = []
    for n, (sh, sw), crop, (nh, nw) in ((1, (200, 300), (41, 27, 53, 37), (61, 29)), (63, (200, 300), (7, 150, 64, 48), (24, 31)),
                                         (64, (150, 220), (100, 3, 53, 37), (74, 106)), (65, (300, 200), (0, 111, 80, 50), (50, 80)),
                                         (4100, (900, 1200), (333, 250, 640, 480), (600, 800))):
        segs.append((cropped_segment(n, sw, sh, crop, nh, nw, seed=n), crop, nh, nw))
    wide = (37, 5, 1200, 50)
    segs.append((shifted_collision(wide), wide, 50, 1200))
    segs.append((special_boxes(53, 37)[:8], (400, 300, 53, 37), 37, 53))  # every box lies left of and above the window
    return segs


def _host_proposals(raw, logits, crop, nh, nw, flip, topk):
    d = {"proposal_boxes": raw.copy(), "proposal_objectness_logits": logits.copy(), "proposal_bbox_mode": 0}
    transform_proposals(d, (nh, nw), crop_list(crop, nh, nw, flip), proposal_topk=topk)
    return d["proposals"].proposal_boxes.tensor.numpy(), d["proposals"].objectness_logits.numpy()


@pytest.mark.parametrize("topk", [4000, 50])
@pytest.mark.parametrize("flip", [False, True])
def test_cropped_proposals_equal_the_host(gpu, flip, topk):
    from wsovod_amd.layers import hip_ops

    segs = _proposal_segments()
    logits = [logits_for(len(s[0]), seed=i) for i, s in enumerate(segs)]
    boxes_d = torch.from_numpy(np.concatenate([s[0] for s in segs])).to(gpu)
    logits_d = torch.from_numpy(np.concatenate(logits)).to(gpu)
    table, crops, r0 = [], [], 0
    for raw, (x0, y0, cw, ch), nh, nw in segs:
        table.append((r0, len(raw), ch, cw, nh, nw, flip))
        crops.append((x0, y0))
        r0 += len(raw)
    runs = [tuple(t.cpu().numpy() for t in hip_ops.transform_proposals(boxes_d, logits_d, table, topk, crops=crops))
            for _ in range(2)]
    for a, b in zip(*runs):  # the same bytes from either call, the rows behind the counts included
        assert a.tobytes() == b.tobytes()
    out_boxes, out_logits, counts = runs[0]
    assert out_boxes.shape == (len(segs), topk, 4) and counts.dtype == np.int32
    lengths = []
    for g, ((raw, crop, nh, nw), lg) in enumerate(zip(segs, logits)):
        want_b, want_l = _host_proposals(raw, lg, crop, nh, nw, flip, topk)
        n = int(counts[g])
        assert n == len(want_b), (g, n, len(want_b))
        assert np.array_equal(_bits(out_boxes[g, :n]), _bits(want_b)), g
        assert np.array_equal(_bits(out_logits[g, :n]), _bits(want_l)), g
        assert not out_boxes[g, n:].any() and not out_logits[g, n:].any()
        lengths.append(n)
    assert lengths[-1] == 0  # the window no box touches: count 0, the slot zeroed
    assert lengths[-2] == (5 if flip else 4)  # of the six collision rows (tests/train_input_cases.py)
    assert lengths[0] == 1 and lengths[1] < 63 and 50 <= lengths[4] <= topk and (topk != 50 or lengths[4] == 50)
    # zero offsets and no crop at all: the bytes of the entry without crops
    zero = [tuple(t.cpu().numpy() for t in hip_ops.transform_proposals(boxes_d, logits_d, table, topk, crops=c))
            for c in ([(0, 0)] * len(segs), [None] * len(segs), None)]
    for a, b, c in zip(*zero):
        assert a.tobytes() == c.tobytes() and b.tobytes() == c.tobytes()
    assert zero[0][2].tolist() != counts.tolist()


def _records():
    return [raw_record(75, 100, 300, seed=1), raw_record(96, 128, 90, seed=2, classes=(5,)), raw_record(122, 80, 41, seed=3)]


def _run(gpu, kind, size, records, seed=12):
    cfg = crop_cfg(kind, size, min_sizes=(96, 112, 128, 144), max_size=200, topk=120)
    host, dev = HostTrainInput(cfg), DeviceTrainInput(cfg, gpu)
    return cfg, host, dev, host(records, np.random.RandomState(seed)), dev(records, np.random.RandomState(seed))


@pytest.fixture(scope="module")
def mapped(gpu):
    """Three records of different sizes through both routes on the same draws, under relative_range."""
    records = _records()
    return (records,) + _run(gpu, "relative_range", (0.9, 0.9), records)


def _assert_same_batch(want, got, on_device=True):
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


def test_device_mapper_equals_host_mapper_relative_range(gpu, mapped):
    records, cfg, host, dev, want, got = mapped
    assert dev.last_route == "device"
    _assert_same_batch(want, got)
    plans = host.plan(records, np.random.RandomState(12))
    assert any(p[3][0] > 0 for p in plans) and any(p[3][1] > 0 for p in plans) and len({p[2] for p in plans}) == 2
    sizes = {tuple(o["image"].shape[1:]) for o in got}
    assert len(sizes) == 3 and tuple(dev.canvas.shape) == (3, 3, max(s[0] for s in sizes), max(s[1] for s in sizes))
    assert [(o["height"], o["width"]) for o in got] == [(75, 100), (96, 128), (122, 80)]


def test_device_mapper_equals_host_mapper_absolute_and_planar(gpu):
    """`absolute` (one crop larger than its image on an axis), a plane-major source (three row slices staged back to back) and
    annotations that carry boxes (the filter runs on the host in both routes)."""
    records = _records()
    records[1]["image"] = torch.from_numpy(np.ascontiguousarray(records[1]["image"].transpose(2, 0, 1)))
    plan0 = HostTrainInput(crop_cfg("absolute", (90, 70), min_sizes=(96, 112, 128, 144), max_size=200)).plan(
        records, np.random.RandomState(7))
    x0, y0, cw, ch = plan0[2][3]
    assert x0 >= 1 and (cw, ch) == (70, 90) and plan0[0][3][3] == 75  # 90 rows asked of a 75-row image
    records[2] = dict(annotated_record(122, 80, plan0[2][3]), file_name=records[2]["file_name"])
    cfg, host, dev, want, got = _run(gpu, "absolute", (90, 70), records, seed=7)
    assert dev.last_route == "device"
    _assert_same_batch(want, got)
    assert got[2]["instances"].gt_classes.tolist() == [c for c, keep in ANNOTATION_FATE.items() if keep]


def test_canvas_is_handed_on_without_a_copy(gpu, mapped):
    from wsovod_amd.modeling.meta_arch import GeneralizedRCNN_WSOVOD as M

    records, cfg, host, dev, want, got = mapped
    images = [o["image"] for o in got]
    sizes = [tuple(im.shape[1:]) for im in images]
    Hp, Wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
    canvas = M._padded_views(images, sizes, Hp, Wp, gpu)
    assert canvas is not None and canvas.data_ptr() == dev.canvas.data_ptr() and tuple(canvas.shape) == (3, 3, Hp, Wp)
    assert M._padded_views([o["image"] for o in want], sizes, Hp, Wp, gpu) is None


def test_float64_boxes_fall_back_to_the_host_route(gpu, mapped):
    records, cfg, host, dev, _, _ = mapped
    odd = [dict(r) for r in records]
    odd[1]["proposal_boxes"] = odd[1]["proposal_boxes"].astype(np.float64)
    other = DeviceTrainInput(cfg, gpu)
    got = other(odd, np.random.RandomState(12))
    assert other.last_route == "host" and other.canvas is None
    _assert_same_batch(host(odd, np.random.RandomState(12)), got, on_device=False)


def test_training_step_losses_equal_from_either_route(gpu, mapped):
    """One R18 training step at plumbing size: the device route's cropped batch goes through `_canvas` without a copy and
    gives the losses of the host route's batch bit for bit."""
    records, cfg, host, dev, want, got = mapped
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
