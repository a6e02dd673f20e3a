"""CPU: the random crop of the training input stage (MODEL.HIP.INPUT_CROP).  The keys and their defaults; T.RandomCrop's four
types redrawn by hand from the same RandomState, and the draw order; HostTrainInput under crop against its pieces composed by
hand, bit for bit; the annotation filter; the two windowed entries declared, bound and validated by status without a GPU; the
kernel's step 1 and int64-key dedupe restated in numpy against TransformList.apply_box and unique_boxes on cropped segments."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.train_input_cases import input_cfg, int64_key_dedupe
from tests.train_input_crop_cases import (ANNOTATION_FATE, PLAN_SEED, annotated_record, by_hand, crop_cfg, crop_list, crop_records,
                                          cropped_segment, hand_plan, kernel_step1, shifted_collision)
from wsovod_amd.config import get_cfg
from wsovod_amd.data.proposals import unique_boxes
from wsovod_amd.data.train_input import DeviceTrainInput, HostTrainInput, build_train_input
from wsovod_amd.modeling.test_time_augmentation import _shortest_edge_size
from wsovod_amd.structures import Boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keys_and_defaults():
    cfg = get_cfg()
    assert cfg.MODEL.HIP.INPUT_CROP is False and cfg.INPUT.CROP.ENABLED is False
    assert cfg.INPUT.CROP.TYPE == "relative_range" and list(cfg.INPUT.CROP.SIZE) == [0.9, 0.9]  # detectron2's defaults
    off = input_cfg()
    off.INPUT.CROP.ENABLED = True
    with pytest.raises(NotImplementedError, match="crop stays with detectron2's DatasetMapper"):  # the key is the switch
        HostTrainInput(off)
    on = crop_cfg()
    assert HostTrainInput(on).crop == ("relative_range", (0.9, 0.9)) and DeviceTrainInput(on, "cpu").crop is not None
    assert HostTrainInput(input_cfg()).crop is None
    from wsovod_amd.testing import _CONFIG_DIR

    cfg.merge_from_file(os.path.join(_CONFIG_DIR, "hot_path_r18_input_device_crop.yaml"))
    assert cfg.MODEL.HIP.INPUT_CROP is True and cfg.MODEL.HIP.INPUT_DEVICE is True and cfg.INPUT.CROP.ENABLED is True
    assert cfg.INPUT.CROP.TYPE == "relative_range" and len(cfg.INPUT.MIN_SIZE_TRAIN) == 24 and cfg.INPUT.MAX_SIZE_TRAIN == 2000
    mapper = build_train_input(cfg, "cpu")
    assert isinstance(mapper, DeviceTrainInput) and mapper.crop == ("relative_range", (0.9, 0.9)) and mapper.proposal_topk == 4000
    with pytest.raises(ValueError, match="CROP"):
        HostTrainInput(crop_cfg("diagonal"))
    with pytest.raises(ValueError, match="absolute_range"):
        HostTrainInput(crop_cfg("absolute_range", (30, 20)))


@pytest.mark.parametrize("kind,size", [("relative_range", (0.9, 0.9)), ("relative", (0.5, 0.75)), ("absolute", (1000, 30)),
                                       ("absolute_range", (20, 45))])
def test_crop_types_redrawn_by_hand(kind, size):
    mapper = HostTrainInput(crop_cfg(kind, size))
    records = crop_records()
    plans = mapper.plan(records, np.random.RandomState(PLAN_SEED))
    assert plans == hand_plan(mapper, kind, size, records, np.random.RandomState(PLAN_SEED))
    for r, (nh, nw, flip, (x0, y0, cw, ch)) in zip(records, plans):
        h, w = r["image"].shape[:2]
        assert 0 <= x0 and x0 + cw <= w and 0 <= y0 and y0 + ch <= h and cw > 0 and ch > 0
        assert min(nh, nw) in mapper.min_sizes or max(nh, nw) == mapper.max_size  # the size of the CROPPED shape
    if kind == "absolute":  # a crop larger than the image takes the image's size on that axis
        assert [p[3][2:] for p in plans] == [(30, 37), (30, 48), (30, 61)]
    if kind == "relative":
        assert [p[3][2:] for p in plans] == [(40, 19), (48, 24), (30, 31)]
    if kind == "relative_range":
        assert len({p[2] for p in plans}) == 2, "the seed must draw a flipped and an unflipped image"
        assert any(3 * p[3][0] % 4 != 0 for p in plans), "the seed must draw a window that does not start on a 4-byte boundary"
        assert any(p[3][2:] != r["image"].shape[1::-1] for p, r in zip(plans, records))
        # another order of the same draws -- all sizes first, then the crops and flips -- gives another plan
        rng = np.random.RandomState(PLAN_SEED)
        sizes = [int(rng.choice(mapper.min_sizes)) for _ in records]
        other = []
        for r, s in zip(records, sizes):
            crop = mapper.draw_crop(rng, *r["image"].shape[:2])
            other.append(_shortest_edge_size(crop[3], crop[2], s, mapper.max_size) + (bool(rng.uniform(0.0, 1.0) < 0.5), crop))
        assert other != plans


def test_empty_crop_raises():
    with pytest.raises(ValueError, match="crop of a"):
        HostTrainInput(crop_cfg("relative", (0.0, 0.5))).plan(crop_records(), np.random.RandomState(0))
    with pytest.raises(ValueError, match="crop of a"):
        HostTrainInput(crop_cfg("absolute", (0, 10))).plan(crop_records(), np.random.RandomState(0))


@pytest.mark.parametrize("kind,size", [("relative_range", (0.9, 0.9)), ("absolute", (30, 41))])
def test_host_route_equals_its_pieces(kind, size):
    mapper = HostTrainInput(crop_cfg(kind, size, topk=120))
    records = crop_records()
    before = copy.deepcopy(records)
    outs = mapper(records, np.random.RandomState(PLAN_SEED))
    again = mapper(records, np.random.RandomState(PLAN_SEED))
    plans = hand_plan(mapper, kind, size, records, np.random.RandomState(PLAN_SEED))
    for r, o, o2, (nh, nw, flip, crop) in zip(records, outs, again, plans):
        image, props, _ = by_hand(r, nh, nw, flip, crop, 120)
        assert o["image"].dtype == torch.uint8 and tuple(o["image"].shape) == (3, nh, nw)
        assert np.array_equal(o["image"].numpy(), image)
        assert o["proposals"].image_size == (nh, nw) and len(o["proposals"]) == len(props) <= 120
        assert o["proposals"].proposal_boxes.tensor.numpy().tobytes() == props.proposal_boxes.tensor.numpy().tobytes()
        assert o["proposals"].objectness_logits.numpy().tobytes() == props.objectness_logits.numpy().tobytes()
        assert (o["height"], o["width"]) == r["image"].shape[:2]  # the source's, not the crop's
        assert o["instances"].image_size == (nh, nw)
        # these annotations carry no bbox: every non-crowd class is kept
        assert o["instances"].gt_classes.tolist() == [a["category_id"] for a in r["annotations"] if not a["iscrowd"]]
        assert o["image"].numpy().tobytes() == o2["image"].numpy().tobytes()
        assert o["proposals"].proposal_boxes.tensor.numpy().tobytes() == o2["proposals"].proposal_boxes.tensor.numpy().tobytes()
    for r, b in zip(records, before):  # the records are left as they were
        assert r.keys() == b.keys() and np.array_equal(r["image"], b["image"]) and r["annotations"] == b["annotations"]
        assert np.array_equal(r["proposal_boxes"], b["proposal_boxes"])
    assert len({len(o["proposals"]) for o in outs}) > 1


def test_annotation_filter():
    kind, size, h, w = "absolute", (20, 30), 40, 60
    mapper = HostTrainInput(crop_cfg(kind, size, topk=50))
    seed = 1
    (nh, nw, flip, crop), = mapper.plan([annotated_record(h, w, (1, 0, 30, 20))], np.random.RandomState(seed))
    record = annotated_record(h, w, crop)
    before = copy.deepcopy(record["annotations"])
    out, = mapper([record], np.random.RandomState(seed))
    assert nw * 2e-6 / crop[2] < 1e-5 < nw * 1.0 / crop[2]  # the sliver is narrower than the threshold, the pixel is not
    kept = out["instances"].gt_classes.tolist()
    assert kept == [c for c, keep in ANNOTATION_FATE.items() if keep] and 7 not in kept
    assert record["annotations"] == before
    dropped = [c for c, keep in ANNOTATION_FATE.items() if not keep]
    assert len(dropped) >= 1 and len(kept) >= 1  # the seed's window drops a class and keeps one
    # the same record without the crop keeps every non-crowd class
    plain, = HostTrainInput(input_cfg(topk=50))([record], np.random.RandomState(seed))
    assert plain["instances"].gt_classes.tolist() == [1, 2, 3, 4, 5, 6, 8]


def test_entries_declared_and_bound():
    from wsovod_amd import _lib

    header = open(os.path.join(ROOT, "include", "wsovod_hip.h")).read()
    for name, nargs in (("wsovod_resample_u8_batch_win", 9), ("wsovod_transform_proposals_win", 11)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 9 == _lib.lib().wsovod_abi_version()  # additive entries: the version stays
    assert C.sizeof(_lib.ResampleWindow) == 88 and C.sizeof(_lib.ResampleWindowBatch) == 8 + 32 * 88
    assert C.sizeof(_lib.ProposalWindow) == 48 and C.sizeof(_lib.ProposalWindowBatch) == 4 + 32 * 48
    assert C.sizeof(_lib.ResampleImage) == 64 and C.sizeof(_lib.ProposalImage) == 32  # the earlier entries' tables are as they were
    for name, cites in (("wsovod_resample_u8_batch_win", ("dataset_mapper.py:88-89", "T.RandomCrop", "CropTransform")),
                        ("wsovod_transform_proposals_win", ("detection_utils.py:206-265", "CropTransform"))):
        at = header.index("int " + name + "(")
        assert all(c in header[max(0, at - 5000):at] for c in cites), name


def _window(d, src_bytes, H=4, W=5, strides=(1, 15, 3)):
    d.src, d.src_bytes, d.H, d.W, d.nh, d.nw = 16, src_bytes, H, W, H, W
    d.stride_c, d.stride_y, d.stride_x = strides


def test_entries_validate_before_any_launch():
    """No GPU: the tables are checked on the host, and what is refused is refused by status before anything is launched."""
    from wsovod_amd import _lib

    L = _lib.lib()
    rb = _lib.ResampleWindowBatch()
    rb.n = 33
    call = lambda: L.wsovod_resample_u8_batch_win(C.byref(rb), None, 0, None, 0, C.c_void_p(16), 8, 8, None)  # noqa: E731
    assert call() == 3 and b"33 images" in L.wsovod_last_error()
    rb.n = 1
    # a 4 x 5 interleaved window: its last sample is byte 2 + 3 * 15 + 4 * 3 = 59, so 60 bytes must be readable
    _window(rb.img[0], 59)
    assert call() == 1 and b"last sample lies at byte 59 of the 59" in L.wsovod_last_error()
    _window(rb.img[0], 60, strides=(1, 0, 3))
    assert call() == 1 and b"strides" in L.wsovod_last_error()
    _window(rb.img[0], 60, strides=(0, 15, 3))
    assert call() == 1 and b"strides" in L.wsovod_last_error()
    _window(rb.img[0], 60, strides=(1, 15, 2))
    assert call() == 1 and b"strides" in L.wsovod_last_error()
    _window(rb.img[0], 60, strides=(1, -15, 3))
    assert call() == 1 and b"strides" in L.wsovod_last_error()
    _window(rb.img[0], 60)
    rb.img[0].nh = 9  # what the entry without a window validates is still validated
    assert call() == 1 and b"does not fit" in L.wsovod_last_error()
    pb = _lib.ProposalWindowBatch()
    pb.n = 33
    args = (C.c_void_p(16), C.c_void_p(16), 8, 4, C.c_void_p(16), 1 << 20, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None)
    assert L.wsovod_transform_proposals_win(C.byref(pb), *args) == 3 and b"33 images" in L.wsovod_last_error()
    pb.n = 1
    p = pb.img[0]
    p.start, p.count, p.sx, p.sy, p.clip_w, p.clip_h, p.has_crop = 0, 8, 1.0, 1.0, 10.0, 10.0, 1
    for cx, cy in ((1.5, 0.0), (0.0, 2.25), (-1.0, 0.0), (0.0, -3.0), (4.0e6 + 1, 0.0)):
        p.crop_x, p.crop_y = cx, cy
        assert L.wsovod_transform_proposals_win(C.byref(pb), *args) == 3 and b"crop offset" in L.wsovod_last_error(), (cx, cy)
    p.crop_x, p.crop_y, p.count = 3.0, 4.0, 9
    assert L.wsovod_transform_proposals_win(C.byref(pb), *args) == 1 and b"lie outside the 8 rows" in L.wsovod_last_error()


# (n, source (h, w), crop (x0, y0, cw, ch), (nh, nw)): the window is a small part of the source
CROPPED = [(1, (200, 300), (41, 27, 53, 37), (61, 29)), (63, (200, 300), (7, 150, 64, 48), (24, 31)),
           (64, (150, 220), (100, 3, 53, 37), (74, 106)), (65, (300, 200), (0, 111, 80, 50), (50, 80)),
           (4100, (900, 1200), (333, 250, 640, 480), (600, 800))]


@pytest.mark.parametrize("flip", [False, True])
def test_kernel_arithmetic_restated_equals_the_host(flip):
    """Without a GPU: step 1 with the crop in single float32 operations gives TransformList.apply_box's bits, and the
    int64-key dedupe selects unique_boxes' rows, on cropped segments where most boxes clip onto the window's border."""
    cases = [(cropped_segment(n, sw, sh, crop, nh, nw, seed=n), crop, nh, nw) for n, (sh, sw), crop, (nh, nw) in CROPPED]
    wide = (37, 5, 1200, 50)
    cases.append((shifted_collision(wide), wide, 50, 1200))
    for raw, crop, nh, nw in cases:
        want = crop_list(crop, nh, nw, flip).apply_box(raw)
        got = kernel_step1(raw, crop, nh, nw, flip)
        assert want.dtype == np.float32 and got.tobytes() == want.tobytes(), (len(raw), flip)
        boxes = Boxes(want)
        boxes.clip((nh, nw))
        t = boxes.tensor.numpy()
        if len(raw) >= 63:
            on_border = ((t[:, 0] == 0) | (t[:, 1] == 0) | (t[:, 2] == nw) | (t[:, 3] == nh)).mean()
            assert on_border > 0.5, on_border
            assert (want.min(axis=0)[:2] < 0).all()  # the crop sends boxes negative
        keep = unique_boxes(boxes)
        assert np.array_equal(int64_key_dedupe(t), keep), (len(raw), flip)
        if len(raw) >= 63:
            assert len(keep) < len(raw)
        if crop is wide:
            assert keep.tolist() == ([0, 1, 2, 3, 4] if flip else [0, 2, 4, 5])  # the hash, not the box
