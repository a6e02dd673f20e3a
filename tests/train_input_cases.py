"""Shared cases of the training input stage tests (test_train_input_host.py, test_gpu_train_input.py): seeded raw records, the
proposal segments with every duplicate kind of the issue, and a numpy restatement of the kernel's int64-key dedupe."""
import numpy as np

from tests.tta_cases import source_image
from wsovod_amd.config import get_cfg


def input_cfg(min_sizes=(48, 56, 64, 72), max_size=100, topk=4000, flip="horizontal", sampling="choice"):
    cfg = get_cfg()
    cfg.MODEL.LOAD_PROPOSALS = True
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = tuple(min_sizes), max_size
    cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING, cfg.INPUT.RANDOM_FLIP = sampling, flip
    cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN = topk
    return cfg


def special_boxes(w, h, sx=1.0, sy=1.0):
    """Boxes in the SOURCE frame of a (h, w) image that is scaled by (sx, sy) -- whole numbers, so the products stay exact --
    whose images in the target frame are: exact duplicates; duplicates only after rounding; duplicates only after clipping;
    boxes wholly outside (empty after the clip); a zero-width and a zero-height box.  (The hash collision: collision_boxes.)"""
    W, Hh = w * sx, h * sy  # the target frame
    t = np.array([
        [10, 12, 40, 44], [10, 12, 40, 44],                      # exact duplicates
        [20.2, 8.4, 50.3, 30.1], [19.8, 8.0, 49.9, 29.6],        # equal after rounding only
        [30, 6, W + 7, Hh + 3], [30, 6, W + 90, Hh + 50],        # equal after clipping only
        [-9, -4, 25, 18], [-2, -1, 25, 18],                      # ... and at the low edge
        [W + 5, 3, W + 30, 20], [4, Hh + 2, 20, Hh + 9],         # wholly outside: empty after the clip
        [-30, -30, -2, -5],                                      # ... on the low side
        [33, 10, 33, 29], [12, 17, 31, 17],                      # zero width / zero height
        [0.4, 0.3, 41, 37], [0.4, 0.3, 41, 37.4],                # a pair that differs below the rounding
    ], dtype=np.float64)
    t[:, [0, 2]] /= sx
    t[:, [1, 3]] /= sy
    return t.astype(np.float32)


def collision_boxes():
    """(1000, 0, x2, y2) and (0, 1, x2, y2): different boxes, equal hashes (1000 * 1 == 1 * 1000) -- the host drops the second.
    They need a frame wider than 1000, so they get a segment of their own with unit scale and width 1200.  The last two rows
    are the same collision for the mirrored frame: (100, 0, 200, 40) and (100, 1, 1200, 40) become (1000, 0, 1100, 40) and
    (0, 1, 1100, 40) under x -> 1200 - x.  Survivors: rows 0, 2, 4, 5 unflipped; rows 0 - 4 flipped."""
    return np.array([[1000, 0, 1100, 40], [0, 1, 1100, 40], [0, 1, 1100, 41], [1000, 0, 1100, 41],
                     [100, 0, 200, 40], [100, 1, 1200, 40]], dtype=np.float32)


def random_boxes(n, w, h, seed):
    rng = np.random.RandomState(seed)
    x0, y0 = rng.uniform(-6, w, n), rng.uniform(-6, h, n)
    b = np.stack([x0, y0, x0 + rng.uniform(0, 0.6 * w, n), y0 + rng.uniform(0, 0.6 * h, n)], axis=1)
    b[::5] = np.round(b[::5] / 4) * 4  # a coarse grid: plenty of duplicates at a distance
    b[::11, [0, 2]] = b[::11, [2, 0]]  # x0 > x1: min / max over the corners matters
    return b.astype(np.float32)


def logits_for(n, seed):
    return np.sort(np.random.RandomState(seed + 77).uniform(0, 1, n))[::-1].astype(np.float32)


def segment(n, w, h, seed, sx=1.0, sy=1.0):
    """n boxes for a (h, w) source: the special cases first (as many as fit), seeded boxes behind them."""
    sp = special_boxes(w, h, sx, sy)[:n]
    return np.concatenate([sp, random_boxes(n - len(sp), w, h, seed)], axis=0)


def raw_record(h, w, n_boxes, seed, dtype=np.float32, classes=(3, 7, 3)):
    """A raw dataset record: interleaved uint8 image, proposals sorted by descending logit, annotations (one crowd)."""
    ann = [{"category_id": c, "iscrowd": 0} for c in classes] + [{"category_id": 19, "iscrowd": 1}]
    return {"file_name": f"img_{h}x{w}_{seed}.jpg", "image_id": seed, "image": source_image(h, w),
            "proposal_boxes": segment(n_boxes, w, h, seed).astype(dtype), "proposal_objectness_logits": logits_for(n_boxes, seed),
            "proposal_bbox_mode": 0, "annotations": ann}


def int64_key_dedupe(boxes_f32):
    """The kernel's unique_boxes on the host: int64 keys from the float32 rint of each coordinate, the first row of every
    distinct key, ascending."""
    r = np.rint(boxes_f32.astype(np.float32)).astype(np.int64)
    key = r[:, 0] + 1000 * r[:, 1] + 1000000 * r[:, 2] + 1000000000 * r[:, 3]
    first = {}
    for i, k in enumerate(key.tolist()):
        first.setdefault(k, i)
    return np.array(sorted(first.values()), dtype=np.int64)
