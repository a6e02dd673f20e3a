"""Shared cases of the random-crop tests of the training input stage (test_train_input_crop_host.py,
test_gpu_train_input_crop.py): configs with MODEL.HIP.INPUT_CROP on, T.RandomCrop's draws restated by hand, one image through
the pieces composed by hand, records whose annotations carry boxes, cropped proposal segments and a numpy restatement of the
kernel's step 1."""
import numpy as np

from tests.train_input_cases import collision_boxes, input_cfg, random_boxes, raw_record, segment
from tests.tta_cases import pil_resize
from wsovod_amd.data.proposals import CropTransform, HFlipTransform, ResizeTransform, TransformList, transform_proposals
from wsovod_amd.modeling.test_time_augmentation import _shortest_edge_size

PLAN_SEED = 2  # relative_range on crop_records(): a flipped and an unflipped image, and windows with 3 * x0 % 4 != 0


def crop_cfg(kind="relative_range", size=(0.9, 0.9), **kw):
    cfg = input_cfg(**kw)
    cfg.MODEL.HIP.INPUT_CROP = True
    cfg.INPUT.CROP.ENABLED, cfg.INPUT.CROP.TYPE, cfg.INPUT.CROP.SIZE = True, kind, list(size)
    return cfg


def crop_records():
    return [raw_record(37, 53, 300, seed=1), raw_record(48, 64, 90, seed=2, classes=(5,)), raw_record(61, 40, 41, seed=3)]


def hand_crop(kind, size, rng, h, w):
    """T.RandomCrop.get_transform by hand: (x0, y0, cw, ch)."""
    if kind == "relative":
        ch, cw = int(h * size[0] + 0.5), int(w * size[1] + 0.5)
    elif kind == "relative_range":
        c = np.asarray(size, dtype=np.float32)
        ch_f, cw_f = c + rng.rand(2) * (1 - c)
        assert (1 - c).dtype == np.float32 and ch_f.dtype == np.float64
        ch, cw = int(h * ch_f + 0.5), int(w * cw_f + 0.5)
    elif kind == "absolute":
        ch, cw = min(size[0], h), min(size[1], w)
    else:
        assert kind == "absolute_range" and size[0] <= size[1]
        ch = rng.randint(min(h, size[0]), min(h, size[1]) + 1)
        cw = rng.randint(min(w, size[0]), min(w, size[1]) + 1)
    y0 = rng.randint(h - ch + 1)
    x0 = rng.randint(w - cw + 1)
    return int(x0), int(y0), int(cw), int(ch)


def hand_plan(mapper, kind, size, records, rng):
    """Per image, in batch order: the crop draws, then the size (of the cropped shape), then the flip."""
    plans = []
    for r in records:
        crop = hand_crop(kind, size, rng, *r["image"].shape[:2])
        s = int(rng.choice(mapper.min_sizes))
        flip = bool(rng.uniform(0.0, 1.0) < 0.5)
        plans.append(_shortest_edge_size(crop[3], crop[2], s, mapper.max_size) + (flip, crop))
    return plans


def by_hand(record, nh, nw, flip, crop, topk):
    """One image through the pieces composed here: numpy slice, PIL resize, mirror, TransformList([Crop, Resize, HFlip]),
    transform_proposals.  Returns (image (3, nh, nw), proposals, the transform list)."""
    x0, y0, cw, ch = crop
    image = pil_resize(np.ascontiguousarray(record["image"][y0:y0 + ch, x0:x0 + cw]), nh, nw)
    tf = [CropTransform(x0, y0, cw, ch), ResizeTransform(ch, cw, nh, nw)]
    if flip:
        image, tf = image[:, ::-1], tf + [HFlipTransform(nw)]
    d = {"proposal_boxes": record["proposal_boxes"].copy(), "proposal_bbox_mode": record["proposal_bbox_mode"],
         "proposal_objectness_logits": record["proposal_objectness_logits"].copy()}
    transform_proposals(d, (nh, nw), TransformList(tf), proposal_topk=topk)
    return np.ascontiguousarray(image.transpose(2, 0, 1)), d["proposals"], TransformList(tf)


# what becomes of each annotation of annotated_record under its crop: category id -> kept
ANNOTATION_FATE = {1: True, 2: False, 3: False, 4: True, 5: True, 6: False, 8: True}


def annotated_record(h, w, crop, seed=4):
    """A record whose annotations are placed against the window `crop` = (x0, y0, cw, ch) of its (h, w) image: inside (1),
    wholly outside (2), overlapping by a sliver of 2e-6 source pixels at the window's left edge (3: narrower than 1e-5 after
    a scale below 5), overlapping by one pixel there (4), XYWH_ABS inside (5), XYWH_ABS wholly outside (6: read as XYXY it
    would lie inside), a crowd box inside (7: ignored), no bbox (8: kept)."""
    x0, y0, cw, ch = crop
    assert x0 >= 1 and cw >= 12 and ch >= 12, crop
    r = raw_record(h, w, 60, seed=seed)
    xyxy, xywh = 0, 1
    r["annotations"] = [
        {"category_id": 1, "iscrowd": 0, "bbox": [x0 + 2.0, y0 + 3.0, x0 + 9.0, y0 + 8.0], "bbox_mode": xyxy},
        {"category_id": 2, "iscrowd": 0, "bbox": [x0 + cw + 1.0, y0 + 1.0, x0 + cw + 7.0, y0 + 6.0], "bbox_mode": xyxy},
        {"category_id": 3, "iscrowd": 0, "bbox": [x0 - 5.0, y0 + 2.0, x0 + 2e-6, y0 + 10.0], "bbox_mode": xyxy},
        {"category_id": 4, "iscrowd": 0, "bbox": [x0 - 5.0, y0 + 2.0, x0 + 1.0, y0 + 10.0], "bbox_mode": xyxy},
        {"category_id": 5, "iscrowd": 0, "bbox": [x0 + 2.0, y0 + 2.0, 5.0, 5.0], "bbox_mode": xywh},
        {"category_id": 6, "iscrowd": 0, "bbox": [x0 + cw + 2.0, y0 + ch + 2.0, 3.0, 3.0], "bbox_mode": xywh},
        {"category_id": 7, "iscrowd": 1, "bbox": [x0 + 2.0, y0 + 3.0, x0 + 9.0, y0 + 8.0], "bbox_mode": xyxy},
        {"category_id": 8, "iscrowd": 0},
    ]
    return r


def cropped_segment(n, src_w, src_h, crop, nh, nw, seed):
    """n source-frame boxes for the window `crop` of a (src_h, src_w) image resized to (nh, nw): the special cases of
    train_input_cases.segment shifted into the window, then seeded boxes over the WHOLE source -- the window is a small part
    of it, so most of them clip onto the window's border (and many go negative under the crop)."""
    x0, y0, cw, ch = crop
    inside = segment(min(n, 15), cw, ch, seed, sx=nw / cw, sy=nh / ch) + np.array([x0, y0, x0, y0], dtype=np.float32)
    return np.concatenate([inside, random_boxes(n - len(inside), src_w, src_h, seed + 1)], axis=0).astype(np.float32)


def shifted_collision(crop):
    x0, y0 = crop[:2]
    return collision_boxes() + np.array([x0, y0, x0, y0], dtype=np.float32)


def crop_list(crop, nh, nw, flip):
    x0, y0, cw, ch = crop
    return TransformList([CropTransform(x0, y0, cw, ch), ResizeTransform(ch, cw, nh, nw)] + ([HFlipTransform(nw)] if flip else []))


def kernel_step1(boxes, crop, nh, nw, flip):
    """The kernel's step 1 in numpy float32, operation by operation: the crop's differences, the two products with the
    host-rounded float32 factors, the flip's difference, min / max over the corners."""
    x0, y0, cw, ch = crop
    b = boxes.astype(np.float32)
    sx, sy = np.float32(nw * 1.0 / cw), np.float32(nh * 1.0 / ch)
    xa, xb = (b[:, 0] - np.float32(x0)) * sx, (b[:, 2] - np.float32(x0)) * sx
    ya, yb = (b[:, 1] - np.float32(y0)) * sy, (b[:, 3] - np.float32(y0)) * sy
    if flip:
        xa, xb = np.float32(nw) - xa, np.float32(nw) - xb
    out = np.stack([np.minimum(xa, xb), np.minimum(ya, yb), np.maximum(xa, xb), np.maximum(ya, yb)], axis=1)
    assert out.dtype == np.float32
    return out
