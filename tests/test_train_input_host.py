"""CPU: the host side of the training input stage (MODEL.HIP.INPUT_DEVICE).  The config keys and their defaults; the two entries
declared and bound; HostTrainInput against its pieces composed by hand on seeded records (same seed twice, and the draw order);
the int64-key restatement of unique_boxes the kernel computes against unique_boxes itself; crop refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.train_input_cases import collision_boxes, input_cfg, int64_key_dedupe, raw_record, segment
from tests.tta_cases import pil_resize
from wsovod_amd.config import get_cfg
from wsovod_amd.data.proposals import HFlipTransform, ResizeTransform, TransformList, transform_proposals, unique_boxes
from wsovod_amd.data.train_input import DeviceTrainInput, HostTrainInput, build_train_input
from wsovod_amd.modeling.test_time_augmentation import _shortest_edge_size
from wsovod_amd.structures import Boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_keys_and_defaults():
    cfg = get_cfg()
    assert cfg.MODEL.HIP.INPUT_DEVICE is False
    assert cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING == "choice" and cfg.INPUT.RANDOM_FLIP == "horizontal"  # detectron2's defaults
    assert type(build_train_input(input_cfg())) is HostTrainInput
    from wsovod_amd.testing import _CONFIG_DIR

    cfg.merge_from_file(os.path.join(_CONFIG_DIR, "hot_path_r18_input_device.yaml"))
    assert cfg.MODEL.HIP.INPUT_DEVICE is True and cfg.INPUT.CROP.ENABLED is False
    assert len(cfg.INPUT.MIN_SIZE_TRAIN) == 24 and cfg.INPUT.MAX_SIZE_TRAIN == 2000
    assert cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN == 4000
    assert isinstance(build_train_input(cfg, "cpu"), DeviceTrainInput)  # (built without a device; a call needs one)


def test_entries_declared_and_bound():
    from wsovod_amd import _lib

    header = open(os.path.join(ROOT, "include", "wsovod_hip.h")).read()
    for name, nargs in (("wsovod_resample_u8_batch", 9), ("wsovod_transform_proposals", 11),
                        ("wsovod_transform_proposals_workspace_bytes", 1)):
        decl = re.search(r"\b(?:int|long long) " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 9 == _lib.lib().wsovod_abi_version()
    assert re.search(r"#define WSOVOD_INPUT_MAX_IMAGES 32\b", header) and _lib.INPUT_MAX_IMAGES == 32
    assert C.sizeof(_lib.ResampleImage) == 64 and C.sizeof(_lib.ResampleBatch) == 8 + 32 * 64
    assert C.sizeof(_lib.ProposalImage) == 32 and C.sizeof(_lib.ProposalBatch) == 4 + 32 * 32
    # the comment of each entry cites the reference code it replaces
    for name, cites in (("wsovod_resample_u8_batch", ("dataset_mapper.py:144-191", "ResizeShortestEdge")),
                        ("wsovod_transform_proposals", ("detection_utils.py:206-265", "unique_boxes"))):
        at = header.index("int " + name + "(")
        assert all(c in header[max(0, at - 6000):at] for c in cites), name


def test_entries_validate_before_any_launch():
    """No GPU: the batch tables are checked on the host, and what is refused is refused by status."""
    from wsovod_amd import _lib

    L = _lib.lib()
    rb = _lib.ResampleBatch()
    rb.n = 33
    assert L.wsovod_resample_u8_batch(C.byref(rb), None, 0, None, 0, C.c_void_p(16), 4, 4, None) == 3
    assert b"33 images" in L.wsovod_last_error()
    rb.n = 1
    d = rb.img[0]
    d.src, d.H, d.W, d.nh, d.nw = 16, 4, 4, 8, 4
    assert L.wsovod_resample_u8_batch(C.byref(rb), None, 0, None, 0, C.c_void_p(16), 4, 4, None) == 1
    assert b"does not fit" in L.wsovod_last_error()
    assert L.wsovod_resample_u8_batch(C.byref(rb), None, 0, None, 0, C.c_void_p(16), 8, 4, None) == 1
    assert b"exactly when its size changes" in L.wsovod_last_error()
    d.kk_v, d.bounds_v, d.ksize_v = 0, 24, 3
    assert L.wsovod_resample_u8_batch(C.byref(rb), C.c_void_p(16), 39, None, 0, C.c_void_p(16), 8, 4, None) == 1
    assert b"vertical table lies outside" in L.wsovod_last_error()
    pb = _lib.ProposalBatch()
    pb.n = 33
    args = (C.c_void_p(16), C.c_void_p(16), 8, 4, C.c_void_p(16), 1 << 20, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None)
    assert L.wsovod_transform_proposals(C.byref(pb), *args) == 3 and b"33 images" in L.wsovod_last_error()
    pb.n = 1
    p = pb.img[0]
    p.start, p.count, p.sx, p.sy, p.clip_w, p.clip_h = 0, 9, 1.0, 1.0, 10.0, 10.0
    assert L.wsovod_transform_proposals(C.byref(pb), *args) == 1 and b"lie outside the 8 rows" in L.wsovod_last_error()
    p.count, p.clip_w = 8, 5.0e6
    assert L.wsovod_transform_proposals(C.byref(pb), *args) == 3 and b"4e6" in L.wsovod_last_error()
    p.clip_w = 10.5
    assert L.wsovod_transform_proposals(C.byref(pb), *args) == 3
    assert L.wsovod_transform_proposals_workspace_bytes(4100) == 16384 * 12 + 4100 * 20 + 16


def _by_hand(mapper, record, nh, nw, flip):
    """One image through the pieces, composed here: PIL resize, mirror, the transform list, transform_proposals."""
    img = record["image"]
    h, w = img.shape[:2]
    image = pil_resize(img, nh, nw)
    tf = [ResizeTransform(h, w, nh, nw)]
    if flip:
        image, tf = image[:, ::-1], tf + [HFlipTransform(nw)]
    d = {k: record[k] for k in ("proposal_boxes", "proposal_objectness_logits", "proposal_bbox_mode")}
    transform_proposals(d, (nh, nw), TransformList(tf), proposal_topk=mapper.proposal_topk)
    return np.ascontiguousarray(image.transpose(2, 0, 1)), d["proposals"]


def _records():
    return [raw_record(37, 53, 300, seed=1), raw_record(48, 64, 90, seed=2, classes=(5,)), raw_record(61, 40, 41, seed=3)]


def test_host_route_equals_its_pieces_and_the_draw_order():
    mapper = HostTrainInput(input_cfg(topk=120))
    records = _records()
    outs = mapper(records, np.random.RandomState(5))
    again = mapper(records, np.random.RandomState(5))
    rng = np.random.RandomState(5)  # the draws by hand: per image the size first, then the flip
    plans = []
    for r in records:
        size = int(rng.choice(mapper.min_sizes))
        flip = bool(rng.uniform(0.0, 1.0) < 0.5)
        plans.append(_shortest_edge_size(*r["image"].shape[:2], size, mapper.max_size) + (flip,))
    assert len({p[2] for p in plans}) == 2, "the seed must draw a flipped and an unflipped image"
    for r, o, o2, (nh, nw, flip) in zip(records, outs, again, plans):
        image, props = _by_hand(mapper, r, nh, nw, flip)
        assert o["image"].dtype == torch.uint8 and np.array_equal(o["image"].numpy(), image)
        assert o["proposals"].image_size == (nh, nw) and len(o["proposals"]) == len(props) <= 120
        assert torch.equal(o["proposals"].proposal_boxes.tensor, props.proposal_boxes.tensor)
        assert torch.equal(o["proposals"].objectness_logits, props.objectness_logits)
        assert (o["height"], o["width"]) == r["image"].shape[:2] and o["file_name"] == r["file_name"]
        assert o["instances"].gt_classes.tolist() == [a["category_id"] for a in r["annotations"] if not a["iscrowd"]]
        assert not o["instances"].gt_classes.is_cuda and o["instances"].image_size == (nh, nw)
        assert not any(k in o for k in ("annotations", "proposal_boxes", "proposal_objectness_logits", "proposal_bbox_mode"))
        assert torch.equal(o["image"], o2["image"]) and torch.equal(o["proposals"].proposal_boxes.tensor, o2["proposals"].proposal_boxes.tensor)
    assert "proposal_boxes" in records[0] and records[0]["image"].shape == (37, 53, 3)  # the records are left as they were
    # another order of the same draws -- all sizes first, then all flips -- gives another batch
    rng = np.random.RandomState(5)
    sizes = [int(rng.choice(mapper.min_sizes)) for _ in records]
    flips = [bool(rng.uniform(0.0, 1.0) < 0.5) for _ in records]
    other = [_shortest_edge_size(*r["image"].shape[:2], s, mapper.max_size) + (f,) for r, s, f in zip(records, sizes, flips)]
    assert other != plans
    assert mapper.plan(records, np.random.RandomState(5)) == plans


def test_sampling_range_flip_none_and_no_proposals():
    m = HostTrainInput(input_cfg(min_sizes=(40, 80), sampling="range", flip="none", topk=50))
    rng = np.random.RandomState(0)
    plans = m.plan(_records() * 4, rng)
    want = np.random.RandomState(0)
    for r, (nh, nw, flip) in zip(_records() * 4, plans):  # one randint per image and no flip draw
        assert (nh, nw) == _shortest_edge_size(*r["image"].shape[:2], int(want.randint(40, 81)), 100) and flip is False
    assert len({p[:2] for p in plans}) > 3
    cfg = input_cfg()
    cfg.MODEL.LOAD_PROPOSALS = False
    out = HostTrainInput(cfg)(_records()[:1], np.random.RandomState(0))[0]
    assert "proposals" not in out and "instances" in out
    chw = dict(_records()[0], image=torch.from_numpy(np.ascontiguousarray(_records()[0]["image"].transpose(2, 0, 1))))
    a = HostTrainInput(input_cfg())([chw], np.random.RandomState(3))[0]
    b = HostTrainInput(input_cfg())(_records()[:1], np.random.RandomState(3))[0]
    assert torch.equal(a["image"], b["image"]) and (a["height"], a["width"]) == (37, 53)


def test_crop_and_unknown_keys_raise():
    cfg = input_cfg()
    cfg.INPUT.CROP.ENABLED = True
    with pytest.raises(NotImplementedError, match="CROP"):
        HostTrainInput(cfg)
    with pytest.raises(NotImplementedError, match="CROP"):
        DeviceTrainInput(cfg, "cpu")
    cfg = input_cfg(flip="vertical")
    with pytest.raises(NotImplementedError, match="RANDOM_FLIP"):
        HostTrainInput(cfg)
    with pytest.raises(ValueError, match="range"):
        HostTrainInput(input_cfg(sampling="range"))


@pytest.mark.parametrize("flip", [False, True])
def test_int64_key_dedupe_equals_unique_boxes(flip):
    """The key claim without a GPU: int64 keys from float32 rint select the rows unique_boxes selects (fp64 hash)."""
    cases = [(n, 53, 37, 61 / 37, 29 / 53) for n in (1, 63, 64, 65, 4100)] + [(6, 1200, 50, 1.0, 1.0)]
    for n, w, h, sy, sx in cases:
        nh, nw = int(round(h * sy)), int(round(w * sx))
        raw = collision_boxes() if w == 1200 else segment(n, w, h, seed=n, sx=nw / w, sy=nh / h)
        tf = TransformList([ResizeTransform(h, w, nh, nw)] + ([HFlipTransform(nw)] if flip else []))
        boxes = Boxes(tf.apply_box(raw))
        boxes.clip((nh, nw))
        want = unique_boxes(boxes)
        got = int64_key_dedupe(boxes.tensor.numpy())
        assert np.array_equal(got, want), (n, flip)
        if w == 1200:
            assert want.tolist() == ([0, 1, 2, 3, 4] if flip else [0, 2, 4, 5])  # the hash, not the box
        if n >= 63:
            assert len(want) < n  # duplicates exist
