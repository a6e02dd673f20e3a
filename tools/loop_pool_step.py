"""POOLER_TYPE ROILoopPool (the three-output pool + the contextlocnet mining head of the WSOVOD_MRRP_WSR_* configs), measured:
the training step per precision and the pooling stage alone, in ONE process:

    python tools/loop_pool_step.py [--steps 15] [--warmup 3] [--images 8 32]      (one MI355X)

The benchmark's synthetic image size (800 x 600) and 512 proposals, K = 20, dropout on, HotPathTrainer + HipSGD as bench.py
drives them.  One hot-path model per precision ("bf16x3f" -- the only route this pooler had before the fused entry --,
"parity", "parity_mx"), all resident; at every batch size the precisions take turns step by step (the order rotated every
round), so that clock and temperature drift lands on all alike.  Every step is bracketed by device events and followed by a
synchronize; a figure is the MEDIAN of its timed steps (min / max beside it).

Then the pooling stage alone, on one res5-shaped fp32 map (512 channels, 75 x 100 cells per image) and the batch's own boxes
and objectness, the forms interleaved launch by launch:

    unfused      wsovod_roi_loop_pool_forward (fp32 values + int32 argmax for 3R rows), `out * roi_scale.repeat(3)` in torch,
                 the cast to the compute dtype -- the sequence the ROI heads ran before
    fused fp32   wsovod_roi_loop_pool_forward_ex, fp32 out, no argmax: the same bits in one launch (checked here)
    fused x2p    the same entry writing planar bf16x2 ("parity", training)
    fused mx+hi  the same entry writing unit-scale f16mx + its bf16 copy ("parity_mx", training)

Writes profiles/loop_pool_step.json and prints it.  Two requirements are recorded as booleans next to the figures: no fused
form is slower than the unfused sequence, and "parity" is not slower than "bf16x3f".
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from wsovod_amd.data import make_batch
from wsovod_amd.engine import HotPathTrainer, build_optimizer
from wsovod_amd.layers import hip_ops as H
from wsovod_amd.modeling.fast_rcnn_open_vocabulary import segment_offsets
from wsovod_amd.testing import build_hot_path_model

PRECISIONS = ("bf16x3f", "parity", "parity_mx")


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _stat(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def pooling_stage(batch, reps):
    """The four forms of the pooling stage on the same map, boxes and scale, interleaved."""
    dev = batch[0]["image"].device
    n = len(batch)
    g = torch.Generator(device=dev).manual_seed(7)
    feat = torch.relu(torch.randn(n, 75, 100, 512, device=dev, generator=g)).permute(0, 3, 1, 2)  # NHWC storage
    boxes = H.cat_rows([x["proposals"].proposal_boxes.tensor for x in batch])
    nums = [len(x["proposals"]) for x in batch]
    rois, scale = H.format_rois(boxes, segment_offsets(nums, dev), H.cat_rows([x["proposals"].objectness_logits for x in batch]))
    size = (7, 7)

    def unfused():
        out = H.roi_loop_pool_forward(feat, rois, 0.125, size)[0]
        return (out * scale.repeat(3).view(-1, 1, 1, 1)).to(torch.float32)

    runs = {
        "unfused (fp32 kernel + argmax, multiply, cast)": unfused,
        "fused fp32": lambda: H.roi_loop_pool_forward_fused(feat, rois, 0.125, size, roi_scale=scale, out_dtype=torch.float32,
                                                           need_argmax=False)[0],
        "fused planar bf16x2": lambda: H.roi_loop_pool_forward_fused(feat, rois, 0.125, size, roi_scale=scale, out_dtype=H.X2,
                                                                    need_argmax=False, want_hi=True)[0],
        "fused f16mx + bf16 copy": lambda: H.roi_loop_pool_forward_fused(feat, rois, 0.125, size, roi_scale=scale,
                                                                        out_dtype=H.MX, need_argmax=False, want_hi=True)[0],
    }
    same = bool(torch.equal(runs["fused fp32"](), unfused()))
    ms = {k: [] for k in runs}
    names = list(runs)
    for rep in range(reps + 2):
        for k in names[rep % len(names):] + names[:rep % len(names)]:
            t, out = _timed(runs[k])
            del out
            if rep >= 2:
                ms[k].append(t)
    res = {k: _stat(v) for k, v in ms.items()}
    base = res[names[0]]["ms"]
    return {"rows": 3 * int(rois.shape[0]), "fused_fp32_equals_unfused_bit_for_bit": same, **res,
            "fused_not_slower_than_unfused": all(res[k]["ms"] <= base for k in names[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--proposals", type=int, default=512)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "loop_pool_step.json"))
    args = ap.parse_args()
    assert args.steps >= 15, "a median over fewer than 15 timed steps is not reported"
    gpu = torch.device("cuda", 0)
    runs = []
    for precision in PRECISIONS:
        cfg, model = build_hot_path_model(seed=0, precision=precision, pooler="ROILoopPool", device="cuda:0")
        cfg.SOLVER.BASE_LR = 1e-4
        model.train()
        runs.append({"precision": precision, "model": model, "trainer": HotPathTrainer(model, build_optimizer(cfg, model))})
    out = {"workload": f"hot-path R18 model, POOLER_TYPE ROILoopPool, 800x600 x {args.proposals} proposals, K = 20, dropout on, "
                       f"one process, precisions interleaved step by step; {args.warmup} warm-up + {args.steps} timed steps "
                       "each, medians",
           "device": torch.cuda.get_device_name(0), "steps": {}, "pooling_stage": {}}
    for n in args.images:
        host = make_batch(n, args.proposals, 20, seed=123)
        batch = [{"image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu), "instances": x["instances"],
                  "height": x["height"], "width": x["width"]} for x in host]
        ms = {r["precision"]: [] for r in runs}

        def one_step(r):
            losses = r["trainer"].run_step(batch)
            r["trainer"].flush()
            return losses

        for rnd in range(args.warmup + args.steps):
            for r in runs[rnd % len(runs):] + runs[:rnd % len(runs)]:
                t, losses = _timed(lambda: one_step(r))
                assert all(bool(torch.isfinite(v)) for v in losses.values()), (r["precision"], losses)
                if rnd >= args.warmup:
                    ms[r["precision"]].append(t)
        res = {p: {**_stat(v), "images_per_s": round(n / statistics.median(v) * 1e3, 2)} for p, v in ms.items()}
        res["parity_not_slower_than_bf16x3f"] = res["parity"]["ms"] <= res["bf16x3f"]["ms"]
        out["steps"][f"{n} images"] = res
        out["pooling_stage"][f"{n} images"] = pooling_stage(batch, args.steps)
    for r in runs:
        r["trainer"].close()
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
