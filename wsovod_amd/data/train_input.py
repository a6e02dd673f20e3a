"""The training input stage: raw dataset records -> the model's `batched_inputs` (MODEL.HIP.INPUT_DEVICE, default off).

What the reference's DatasetMapper does per image before every step (wsovod/data/dataset_mapper.py:144-191 with detectron2's
ResizeShortestEdge and RandomFlip, un-vendored): draw a short-edge size from INPUT.MIN_SIZE_TRAIN, resize (Pillow
bilinear for uint8 images), draw a flip, move the ~4000 loaded proposals with the image (`transform_proposals`: apply_box, clip,
unique_boxes, nonempty, top-k), read the image-level classes off the annotations; the batch is zero-padded to its largest image.

A raw record is a dict with `image` (uint8, (H, W, 3) as read_image returns it, or a (3, H, W) tensor), optionally
`proposal_boxes` / `proposal_objectness_logits` / `proposal_bbox_mode` (what load_proposals_into_dataset attaches) and
`annotations` (dicts with `category_id`, optionally `iscrowd`, `bbox` / `bbox_mode`).  Decoding and colour augmentations are
not done here.

* `HostTrainInput`  the reference route restated from the repository's pieces: `_shortest_edge_size` / `_resize_image`
  (modeling/test_time_augmentation.py) and the transforms / `transform_proposals` of data/proposals.py.
* `DeviceTrainInput`  the same draws and the same outputs with the work on the device: one pinned staging buffer and ONE
  asynchronous upload of the raw images, boxes and logits; `hip_ops.resample_u8_batch` (two launches) writes the batch canvas;
  `hip_ops.transform_proposals` (a memset and two launches) the proposals; the only host read is the per-image proposal
  counts.  The `image` of each output is the view canvas[g, :, :nh, :nw], which `GeneralizedRCNN_WSOVOD._canvas` hands on
  without a copy.  A batch with a record the kernels do not take (boxes that are not float32 XYXY_ABS or not finite, an image
  that is not uint8) goes through the host route, unchanged.

Both take an explicit numpy RandomState and draw, per image in batch order, the size first and the flip second -- the order
of detectron2's augmentation list, one `uniform()` per flip.

Random crop (INPUT.CROP.ENABLED with MODEL.HIP.INPUT_CROP; without that key INPUT.CROP.ENABLED raises): dataset_mapper.py:88-89
puts detectron2's T.RandomCrop(INPUT.CROP.TYPE, INPUT.CROP.SIZE) at position 0 of the list, so per image the crop is drawn first
(`draw_crop`: the size by TYPE, then y0, then x0), ResizeShortestEdge sees the cropped shape, and the transform list is
[CropTransform, ResizeTransform, HFlipTransform?].  `height` / `width` stay the source's.  A plan entry is then
(new_h, new_w, flip, (x0, y0, cw, ch)).  Under crop the annotations are filtered as the reference does
(detection_utils.py:268-299 transform_instance_annotations, :472-499 filter_empty_instances): the bbox of a non-crowd annotation,
as XYXY in float64, goes through the transform list, is clipped to the output frame, becomes float32 (the Boxes of
annotations_to_instances) and keeps its class only if its width and height are both > 1e-5.  An annotation without a `bbox`
(image-level labels only) cannot be placed and is kept.  The host route slices the image with numpy; the device route stages
only rows [y0, y0 + ch) of each source and cuts the columns in the kernel (window origin and pitch).
"""
import numpy as np
import torch

from ..modeling.test_time_augmentation import _resize_image, _shortest_edge_size
from ..structures import Boxes, Instances
from .proposals import XYWH_ABS, XYXY_ABS, CropTransform, HFlipTransform, ResizeTransform, TransformList, transform_proposals

__all__ = ["HostTrainInput", "DeviceTrainInput", "build_train_input"]

_RAW_KEYS = ("image", "annotations", "proposal_boxes", "proposal_objectness_logits", "proposal_bbox_mode")


def _image_hw(image):
    """(H, W, plane_major) of a raw record's image."""
    if isinstance(image, torch.Tensor):  # the DatasetMapper's own output format: (3, H, W)
        return int(image.shape[1]), int(image.shape[2]), True
    return int(image.shape[0]), int(image.shape[1]), False


def _box_survives(anno, transforms, image_shape):
    """transform_instance_annotations + filter_empty_instances on one annotation's box, in numpy float64 up to the Boxes."""
    box = np.asarray(anno["bbox"], dtype=np.float64).reshape(1, 4)
    mode = int(getattr(anno["bbox_mode"], "value", anno["bbox_mode"]))
    if mode == XYWH_ABS:
        box = np.concatenate([box[:, :2], box[:, :2] + box[:, 2:]], axis=1)
    elif mode != XYXY_ABS:
        raise NotImplementedError(f"annotation bbox_mode {mode}: XYXY_ABS / XYWH_ABS only")
    box = transforms.apply_box(box)[0].clip(min=0)
    box = np.minimum(box, [image_shape[1], image_shape[0], image_shape[1], image_shape[0]]).astype(np.float32)
    return bool(box[2] - box[0] > 1e-5 and box[3] - box[1] > 1e-5)


class HostTrainInput:
    """`mapper(records, rng)` -> list of dicts with `image` (uint8 (3, nh, nw)), `height` / `width` (the record's own, else
    the source image's), `proposals` (Instances; when the record carries proposal_boxes and proposals are loaded) and
    `instances` (Instances with the host `gt_classes`; when the record carries annotations)."""

    def __init__(self, cfg):
        self.crop = None  # (TYPE, SIZE) of T.RandomCrop
        if cfg.INPUT.CROP.ENABLED:
            if not cfg.MODEL.HIP.INPUT_CROP:
                raise NotImplementedError("INPUT.CROP.ENABLED: the training input stage builds ResizeShortestEdge and RandomFlip "
                                          "only; crop stays with detectron2's DatasetMapper")
            kind, size = cfg.INPUT.CROP.TYPE, tuple(cfg.INPUT.CROP.SIZE)
            if kind not in ("relative_range", "relative", "absolute", "absolute_range") or len(size) != 2:
                raise ValueError(f"INPUT.CROP.TYPE {kind!r} / SIZE {size}: 'relative_range', 'relative', 'absolute' or "
                                 "'absolute_range' and two numbers")
            if kind == "absolute_range" and not size[0] <= size[1]:
                raise ValueError(f"INPUT.CROP.SIZE {size}: (min, max) with 'absolute_range'")
            self.crop = (kind, size)
        self.min_sizes = tuple(int(s) for s in cfg.INPUT.MIN_SIZE_TRAIN)
        self.max_size = int(cfg.INPUT.MAX_SIZE_TRAIN)
        self.sampling = cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING
        if self.sampling not in ("choice", "range"):
            raise ValueError(f"INPUT.MIN_SIZE_TRAIN_SAMPLING {self.sampling!r}: 'choice' or 'range'")
        if self.sampling == "range" and len(self.min_sizes) != 2:
            raise ValueError(f"INPUT.MIN_SIZE_TRAIN must hold (min, max) with 'range' sampling, got {self.min_sizes}")
        if cfg.INPUT.RANDOM_FLIP not in ("horizontal", "none"):
            raise NotImplementedError(f"INPUT.RANDOM_FLIP {cfg.INPUT.RANDOM_FLIP!r}: 'horizontal' or 'none'")
        self.flip = cfg.INPUT.RANDOM_FLIP == "horizontal"
        self.proposal_topk = int(cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN) if cfg.MODEL.LOAD_PROPOSALS else 0

    # ---- the random part, shared by both routes ----
    def draw_crop(self, rng, h, w):
        """(x0, y0, cw, ch) of one (h, w) image: T.RandomCrop.get_transform -- the size by TYPE (get_crop_size), then y0, x0."""
        kind, size = self.crop
        if kind == "relative":
            ch, cw = int(h * size[0] + 0.5), int(w * size[1] + 0.5)
        elif kind == "relative_range":
            c = np.asarray(size, dtype=np.float32)
            ch_f, cw_f = c + rng.rand(2) * (1 - c)  # (1 - c is float32, the sum float64: detectron2's expression)
            ch, cw = int(h * ch_f + 0.5), int(w * cw_f + 0.5)
        elif kind == "absolute":
            ch, cw = min(size[0], h), min(size[1], w)
        else:
            ch = rng.randint(min(h, size[0]), min(h, size[1]) + 1)
            cw = rng.randint(min(w, size[0]), min(w, size[1]) + 1)
        ch, cw = int(ch), int(cw)
        if not (0 < ch <= h and 0 < cw <= w):
            raise ValueError(f"INPUT.CROP {kind} {size}: a {ch} x {cw} crop of a {h} x {w} image")
        y0 = int(rng.randint(h - ch + 1))
        x0 = int(rng.randint(w - cw + 1))
        return x0, y0, cw, ch

    def draw(self, rng, h, w):
        """(new_h, new_w, flip) of one image: ResizeShortestEdge.get_transform's draw, then RandomFlip's.  Under crop the
        crop's draws come first, the size is that of the cropped shape and the crop (x0, y0, cw, ch) is a fourth entry."""
        if self.crop is not None:
            crop = self.draw_crop(rng, h, w)
            h, w = crop[3], crop[2]
        if self.sampling == "range":
            size = int(rng.randint(self.min_sizes[0], self.min_sizes[1] + 1))
        else:
            size = int(rng.choice(self.min_sizes))
        nh, nw = _shortest_edge_size(h, w, size, self.max_size)
        flip = bool(rng.uniform(0.0, 1.0) < 0.5) if self.flip else False
        return (nh, nw, flip) if self.crop is None else (nh, nw, flip, crop)

    def plan(self, records, rng):
        return [self.draw(rng, *_image_hw(r["image"])[:2]) for r in records]

    # ---- the parts that stay on the host in both routes ----
    @staticmethod
    def _carry(record, h, w):
        out = {k: v for k, v in record.items() if k not in _RAW_KEYS}
        out.setdefault("height", h)
        out.setdefault("width", w)
        return out

    @staticmethod
    def _instances(record, image_shape, transforms=None):
        """Image-level supervision: the classes of the non-crowd annotations (get_image_level_gt reads nothing else).  With
        `transforms` (under crop) an annotation that carries a `bbox` keeps its class only if the box is non-empty in the
        output frame (module docstring); one without a `bbox` is kept."""
        annos = [a for a in record["annotations"] if a.get("iscrowd", 0) == 0]
        if transforms is not None:
            annos = [a for a in annos if "bbox" not in a or _box_survives(a, transforms, image_shape)]
        classes = [int(a["category_id"]) for a in annos]
        return Instances(image_shape, gt_classes=torch.tensor(classes, dtype=torch.int64))

    @staticmethod
    def _transforms(h, w, nh, nw, flip, crop):
        """(TransformList, the resize input's (h, w)) of one image."""
        tf = []
        if crop is not None:
            tf.append(CropTransform(*crop))
            h, w = crop[3], crop[2]
        tf.append(ResizeTransform(h, w, nh, nw))
        if flip:
            tf.append(HFlipTransform(nw))
        return TransformList(tf), (h, w)

    def _wants_proposals(self, record):
        return self.proposal_topk > 0 and "proposal_boxes" in record

    # ---- the host route ----
    def map_one(self, record, nh, nw, flip, crop=None):
        image = record["image"]
        h, w, planar = _image_hw(image)
        hwc = image.permute(1, 2, 0).numpy() if planar else np.asarray(image)
        if crop is not None:
            hwc = np.ascontiguousarray(CropTransform(*crop).apply_image(hwc))
        resized = _resize_image(hwc, nh, nw)
        if flip:
            resized = resized[:, ::-1]
        out = self._carry(record, h, w)
        out["image"] = torch.from_numpy(np.ascontiguousarray(resized.transpose(2, 0, 1)))
        tf, _ = self._transforms(h, w, nh, nw, flip, crop)
        if self._wants_proposals(record):
            d = {"proposal_boxes": record["proposal_boxes"], "proposal_bbox_mode": record.get("proposal_bbox_mode", XYXY_ABS),
                 "proposal_objectness_logits": record["proposal_objectness_logits"]}
            transform_proposals(d, (nh, nw), tf, proposal_topk=self.proposal_topk)
            out["proposals"] = d["proposals"]
        if "annotations" in record:
            out["instances"] = self._instances(record, (nh, nw), tf if crop is not None else None)
        return out

    def map_planned(self, records, plans):
        return [self.map_one(r, *p) for r, p in zip(records, plans)]

    def __call__(self, records, rng):
        return self.map_planned(records, self.plan(records, rng))


class DeviceTrainInput(HostTrainInput):
    """The same interface, draws and outputs with images and proposals built on `device` (see the module docstring).
    `last_route` names the route the last batch took ("device" / "host"); `canvas` is the last device batch's canvas."""

    def __init__(self, cfg, device):
        super().__init__(cfg)
        self.device = torch.device(device)
        self._pinned = None
        self.last_route, self.canvas = None, None

    def _takes(self, record):
        image = record["image"]
        if isinstance(image, torch.Tensor):
            ok = image.dtype == torch.uint8 and image.dim() == 3 and image.shape[0] == 3 and not image.is_cuda
        else:
            ok = isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
        if not ok or image.shape[0] == 0 or image.shape[1] == 0 or image.shape[2] == 0:
            return False
        if not self._wants_proposals(record):
            return True
        boxes, logits = record["proposal_boxes"], record["proposal_objectness_logits"]
        mode = record.get("proposal_bbox_mode", XYXY_ABS)
        return (isinstance(boxes, np.ndarray) and boxes.dtype == np.float32 and boxes.ndim == 2 and boxes.shape[1] == 4
                and int(getattr(mode, "value", mode)) == XYXY_ABS and isinstance(logits, np.ndarray)
                and logits.shape == (boxes.shape[0],) and bool(np.isfinite(boxes).all()))

    def _stage(self, nbytes):
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty((max(nbytes, 1 << 20) * 5 // 4,), dtype=torch.uint8).pin_memory()
        return self._pinned

    def map_planned(self, records, plans):
        from ..layers import hip_ops as H

        with_props = [self._wants_proposals(r) for r in records]
        if not all(self._takes(r) for r in records) or len(set(with_props)) != 1:
            self.last_route, self.canvas = "host", None
            return super().map_planned(records, plans)
        props = with_props[0]
        crops = [p[3] if len(p) > 3 else None for p in plans]  # (x0, y0, cw, ch) under crop
        # layout of the staging buffer: the raw images (each at a multiple of 16), then all boxes, then all logits.  Under crop
        # only rows [y0, y0 + ch) of a source are staged -- one slice of an interleaved source, three row slices back to back
        # of a plane-major one -- and (rows, w) below is the staged block's size
        geo, at = [], 0
        for r, crop in zip(records, crops):
            h, w, planar = _image_hw(r["image"])
            y0, rows_staged = (0, h) if crop is None else (crop[1], crop[3])
            geo.append((at, h, w, planar, y0, rows_staged))
            at += (3 * rows_staged * w + 15) // 16 * 16
        rows = [int(r["proposal_boxes"].shape[0]) for r in records] if props else []
        n_rows = sum(rows)
        box_at, logit_at = at, at + 16 * n_rows
        nbytes = logit_at + 4 * n_rows
        pinned = self._stage(nbytes)
        host = pinned.numpy()
        for r, (off, h, w, planar, y0, ch) in zip(records, geo):
            src = r["image"].numpy()[:, y0:y0 + ch] if planar else r["image"][y0:y0 + ch]
            host[off:off + 3 * ch * w] = np.ascontiguousarray(src).reshape(-1)
        if props:
            hb = host[box_at:logit_at].view(np.float32).reshape(n_rows, 4)
            hl = host[logit_at:nbytes].view(np.float32)
            r0 = 0
            for r, n in zip(records, rows):
                hb[r0:r0 + n] = r["proposal_boxes"]
                hl[r0:r0 + n] = r["proposal_objectness_logits"].astype("float32")
                r0 += n
        dev = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        # the one upload; the read of the counts below waits for it, so the staging buffer is free again when this returns
        dev.copy_(pinned[:nbytes], non_blocking=True)
        images = [dev[off:off + 3 * ch * w].view((3, ch, w) if planar else (ch, w, 3)) for off, _, w, planar, _, ch in geo]
        # the columns of a crop are cut by the kernel: a window (0, x0, ch, cw) of the staged rows
        windows = [(0, c[0], c[3], c[2]) for c in crops] if self.crop is not None else None
        try:
            canvas = H.resample_u8_batch(images, [(p[0], p[1]) for p in plans], [p[2] for p in plans],
                                         interleaved=[not g[3] for g in geo], windows=windows)
            if props:
                segs, r0 = [], 0
                for (_, h, w, _, _, _), n, p, crop in zip(geo, rows, plans, crops):
                    if crop is not None:
                        h, w = crop[3], crop[2]
                    segs.append((r0, n, h, w, p[0], p[1], p[2]))
                    r0 += n
                out_boxes, out_logits, counts = H.transform_proposals(
                    dev[box_at:logit_at].view(torch.float32).view(n_rows, 4), dev[logit_at:nbytes].view(torch.float32), segs,
                    self.proposal_topk, crops=[(c[0], c[1]) for c in crops] if self.crop is not None else None)
                counts = counts.cpu().tolist()  # the stage's one host read
            else:
                torch.cuda.current_stream(self.device).synchronize()
        except H.Unsupported:  # a size the kernels refuse is never approximated: this batch takes the host route
            torch.cuda.current_stream(self.device).synchronize()
            self.last_route, self.canvas = "host", None
            return super().map_planned(records, plans)
        canvas.zero_padded = True  # (what _canvas's no-copy branch asks of the views' base: the kernel wrote every byte)
        outs = []
        for g, (r, (_, h, w, _, _, _), p, crop) in enumerate(zip(records, geo, plans, crops)):
            nh, nw, flip = p[:3]
            out = self._carry(r, h, w)
            out["image"] = canvas[g, :, :nh, :nw]
            if props:
                out["proposals"] = Instances((nh, nw), proposal_boxes=Boxes(out_boxes[g, :counts[g]]),
                                             objectness_logits=out_logits[g, :counts[g]])
            if "annotations" in r:
                out["instances"] = self._instances(r, (nh, nw), self._transforms(h, w, nh, nw, flip, crop)[0] if crop else None)
            outs.append(out)
        self.last_route, self.canvas = "device", canvas
        return outs


def build_train_input(cfg, device=None):
    """MODEL.HIP.INPUT_DEVICE: the device stage on `device` (default MODEL.DEVICE); else the host stage."""
    if cfg.MODEL.HIP.INPUT_DEVICE:
        return DeviceTrainInput(cfg, device if device is not None else cfg.MODEL.DEVICE)
    return HostTrainInput(cfg)
