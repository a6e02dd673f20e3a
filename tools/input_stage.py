"""The training input stage per batch, host route next to device route (MODEL.HIP.INPUT_DEVICE), measured in ONE process:

    python tools/input_stage.py [--steps 15] [--warmup 2] [--crop]      (one MI355X)

Raw records -- interleaved uint8 images of 500 x 375 and 800 x 600 (alternating), 4000 float32 proposals each -- through
`HostTrainInput` and `DeviceTrainInput` under configs/hot_path_r18_input_device.yaml (the shipped 24-entry MIN_SIZE_TRAIN list,
MAX_SIZE_TRAIN 2000, flip, top-k 4000), at 1, 8 and 32 images.  The two routes take turns call by call on the SAME records and
the same draws (one RandomState seed per round), so that clock and temperature drift lands on both alike.  A round times, per
route, (a) the whole mapper call, then (b) its two stages on their own -- the resize stage (resize + mirror + padding; the
device figure includes nothing of the upload) and the proposal stage (the device figure includes the read of the counts) --
and (c) for the host route what the model's `_canvas` / `_proposals` add before the first kernel can run: the zeroed canvas,
one copy per image, the proposals' upload.  The device route's whole call contains its upload.  Host clock around work that
ends in a synchronise; a figure is the MEDIAN of its timed calls with min / max beside it.  Before timing, the two routes'
outputs are compared once, byte for byte.  One process and one host thread: a multi-worker host loader is not measured.
Writes profiles/input_device.json and prints it.

--crop: the same protocol under configs/hot_path_r18_input_device_crop.yaml (T.RandomCrop relative_range [0.9, 0.9] in front of
the list, MODEL.HIP.INPUT_CROP): the host stages slice with numpy, the device stages read windows of the resident images and
subtract the crop offsets.  Writes profiles/input_device_crop.json.  --compare PARENT TREE PARENT adds the device route's
whole-call figures of three crop-OFF runs of this tool (their JSON files: the parent commit, this tree, the parent commit again,
taken in that order on one box) under "crop_off_device_call" with the verdict whether the tree's median lies inside the spread
of the two parent runs: the crop shares the kernels of the crop-off route.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wsovod_amd.config import get_cfg
from wsovod_amd.data.proposals import transform_proposals
from wsovod_amd.data.train_input import DeviceTrainInput, HostTrainInput
from wsovod_amd.layers import hip_ops as H
from wsovod_amd.modeling.test_time_augmentation import _resize_image
from wsovod_amd.testing import _CONFIG_DIR

SOURCES = ((375, 500), (600, 800))
BATCHES = (1, 8, 32)


def _stat(ms):
    return {"ms": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def make_records(n, proposals, seed=123):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        h, w = SOURCES[i % len(SOURCES)]
        x0, y0 = rng.uniform(0, w - 17, proposals), rng.uniform(0, h - 17, proposals)
        bw = 16 + rng.uniform(0, 1, proposals) * (np.minimum(w - x0, 400.0) - 16)
        bh = 16 + rng.uniform(0, 1, proposals) * (np.minimum(h - y0, 300.0) - 16)
        boxes = np.stack([x0, y0, x0 + bw, y0 + bh], axis=1).astype(np.float32)
        logits = np.sort(1.0 - rng.uniform(0, 1, proposals))[::-1].astype(np.float32)
        out.append({"image": rng.randint(0, 256, (h, w, 3), dtype=np.uint8), "proposal_boxes": boxes,
                    "proposal_objectness_logits": logits, "proposal_bbox_mode": 0,
                    "annotations": [{"category_id": int(c), "iscrowd": 0} for c in rng.permutation(20)[:2]]})
    return out


def host_resize_stage(records, plans):
    out = []
    for r, (nh, nw, flip, *crop) in zip(records, plans):
        img = r["image"]
        if crop:
            x0, y0, cw, ch = crop[0]
            img = np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw])
        a = _resize_image(img, nh, nw)
        out.append(np.ascontiguousarray((a[:, ::-1] if flip else a).transpose(2, 0, 1)))
    return out


def host_proposal_stage(records, plans, topk):
    out = []
    for r, (nh, nw, flip, *crop) in zip(records, plans):
        h, w = r["image"].shape[:2]
        d = {k: r[k] for k in ("proposal_boxes", "proposal_objectness_logits", "proposal_bbox_mode")}
        tf, _ = HostTrainInput._transforms(h, w, nh, nw, flip, crop[0] if crop else None)
        transform_proposals(d, (nh, nw), tf, proposal_topk=topk)
        out.append(d["proposals"])
    return out


def host_hand_over(outs, device):
    """What GeneralizedRCNN_WSOVOD._canvas / _proposals do with the host route's batch."""
    sizes = [tuple(o["image"].shape[1:]) for o in outs]
    canvas = torch.zeros((len(outs), 3, max(s[0] for s in sizes), max(s[1] for s in sizes)), dtype=torch.uint8, device=device)
    for i, (o, (h, w)) in enumerate(zip(outs, sizes)):
        canvas[i, :, :h, :w].copy_(o["image"], non_blocking=True)
    return canvas, [o["proposals"].to(device) for o in outs]


def compare_crop_off(paths):
    """The device route's whole-call figures of three crop-off runs (parent, tree, parent again) and, per batch size, whether
    the tree's median lies inside the spread (lowest min .. highest max) of the two parent runs."""
    runs = []
    for path in paths:
        with open(path) as f:
            runs.append({n: b["device"]["call"] for n, b in json.load(f)["batches"].items()})
    res = {"order": "parent, tree, parent again; one box, one after the other", "batches": {}}
    for n in runs[0]:
        lo = min(runs[0][n]["ms_min"], runs[2][n]["ms_min"])
        hi = max(runs[0][n]["ms_max"], runs[2][n]["ms_max"])
        res["batches"][n] = {"parent": runs[0][n], "tree": runs[1][n], "parent_again": runs[2][n],
                             "tree_median_inside_parent_spread": bool(lo <= runs[1][n]["ms"] <= hi)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proposals", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--crop", action="store_true")
    ap.add_argument("--compare", nargs=3, metavar=("PARENT", "TREE", "PARENT"), default=None)
    args = ap.parse_args()
    name = "hot_path_r18_input_device_crop" if args.crop else "hot_path_r18_input_device"
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "input_device_crop.json" if args.crop else "input_device.json")
    gpu = torch.device("cuda", 0)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(_CONFIG_DIR, name + ".yaml"))
    host, dev = HostTrainInput(cfg), DeviceTrainInput(cfg, gpu)
    topk = host.proposal_topk
    crop_text = f"random crop {host.crop[0]} {list(host.crop[1])}, " if args.crop else ""
    out = {"workload": f"training input stage under {name}.yaml ({crop_text}{len(host.min_sizes)} short-edge sizes "
                       f"{host.min_sizes[0]} .. {host.min_sizes[-1]}, max {host.max_size}, flip, top-k {topk}); sources 500 x 375 and "
                       f"800 x 600 alternating, {args.proposals} proposals each; one process, one host thread, routes interleaved "
                       f"call by call on the same records and draws; {args.warmup} warm-up + {args.steps} timed rounds, medians "
                       "(host clock, synchronised)",
           "device": torch.cuda.get_device_name(0), "not_measured": "a multi-worker host loader; image decoding" + ("" if args.crop else "; crop"),
           "batches": {}}
    for n in BATCHES:
        records = make_records(n, args.proposals)
        a, b = host(records, np.random.RandomState(0)), dev(records, np.random.RandomState(0))
        assert dev.last_route == "device"
        equal = all(torch.equal(x["image"], y["image"].cpu())
                    and torch.equal(x["proposals"].proposal_boxes.tensor, y["proposals"].proposal_boxes.tensor.cpu())
                    and torch.equal(x["proposals"].objectness_logits, y["proposals"].objectness_logits.cpu()) for x, y in zip(a, b))
        # the device stages' inputs, resident: the stage figures hold no upload
        d_images = [torch.from_numpy(r["image"]).to(gpu) for r in records]
        d_boxes = torch.from_numpy(np.concatenate([r["proposal_boxes"] for r in records])).to(gpu)
        d_logits = torch.from_numpy(np.concatenate([r["proposal_objectness_logits"] for r in records])).to(gpu)
        ms = {r: {"call": [], "resize": [], "proposals": []} for r in ("host", "device")}
        ms["host"]["hand_over"] = []
        for rnd in range(args.warmup + args.steps):
            order = ("host", "device") if rnd % 2 == 0 else ("device", "host")
            plans = host.plan(records, np.random.RandomState(1000 + rnd))
            segs, r0 = [], 0
            for r, (nh, nw, flip, *crop) in zip(records, plans):
                h, w = (crop[0][3], crop[0][2]) if crop else r["image"].shape[:2]
                segs.append((r0, args.proposals, h, w, nh, nw, flip))
                r0 += args.proposals
            # (x0, y0, cw, ch) of the plan -> the fronts' window (y0, x0, ch, cw) of the resident image and offset (x0, y0)
            windows = [(p[3][1], p[3][0], p[3][3], p[3][2]) for p in plans] if args.crop else None
            crops = [p[3][:2] for p in plans] if args.crop else None
            t = {}
            for route in order:
                mapper = host if route == "host" else dev
                t[route, "call"], res = _clock(lambda: mapper(records, np.random.RandomState(1000 + rnd)))
                if route == "host":
                    t[route, "hand_over"], _ = _clock(lambda: host_hand_over(res, gpu))
            for route in order:
                if route == "host":
                    t[route, "resize"], _ = _clock(lambda: host_resize_stage(records, plans))
                    t[route, "proposals"], _ = _clock(lambda: host_proposal_stage(records, plans, topk))
                else:
                    more = {"windows": windows} if args.crop else {}
                    t[route, "resize"], _ = _clock(lambda: H.resample_u8_batch(
                        d_images, [p[:2] for p in plans], [p[2] for p in plans], interleaved=True, **more))
                    more = {"crops": crops} if args.crop else {}
                    t[route, "proposals"], _ = _clock(
                        lambda: H.transform_proposals(d_boxes, d_logits, segs, topk, **more)[2].cpu())
            if rnd >= args.warmup:
                for (route, name), v in t.items():
                    ms[route][name].append(v)
        out["batches"][str(n)] = {"outputs_equal_byte_for_byte": bool(equal),
                                  **{r: {k + ("_stage" if k in ("resize", "proposals") else ""): _stat(v) for k, v in d.items()}
                                     for r, d in ms.items()}}
    if args.compare:
        out["crop_off_device_call"] = compare_crop_off(args.compare)
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
