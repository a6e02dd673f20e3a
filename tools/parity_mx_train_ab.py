"""A/B of the training precisions that meet (or are measured against) the five-step trajectory gate, in ONE process:

    python tools/parity_mx_train_ab.py [--images 32] [--steps 15] [--warmup 4]      (one MI355X)

  parity_mx                          f16mx forward, plain bf16 backward
  parity_train                       bf16x2 forward, split input gradients on the generic x3 route
  parity_mx_train                    f16mx forward, split input gradients as ONE bf16x2 contraction (the default route)
  parity_mx_train, WSOVOD_PT_DX=x3   the same mode on the generic x3 route

Config-2 shapes (WSR_18, 800x600, 512 proposals, K = 20), dropout on, HotPathTrainer + HipSGD as bench.py drives them.  One
model per variant, all resident; the variants take turns step by step (one step of each per round, the order rotated every
round), so that clock and temperature drift lands on all of them alike.  Every step is bracketed by device events on the
stream and followed by a synchronize; the figure of a variant is the MEDIAN of its timed steps (min / max kept beside it).
Writes profiles/parity_mx_train_ab.json and prints it.
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
from wsovod_amd.testing import build_hot_path_model

VARIANTS = [  # (label, MODEL.HIP.PRECISION, WSOVOD_PT_DX)
    ("parity_mx", "parity_mx", None),
    ("parity_train", "parity_train", None),
    ("parity_mx_train", "parity_mx_train", None),
    ("parity_mx_train, WSOVOD_PT_DX=x3", "parity_mx_train", "x3"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--proposals", type=int, default=512)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "parity_mx_train_ab.json"))
    args = ap.parse_args()
    gpu = torch.device("cuda", 0)
    os.environ.pop("WSOVOD_PT_SPLIT", None)
    host = make_batch(args.images, args.proposals, 20, seed=123)
    batch = [{"image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu), "instances": x["instances"],
              "height": x["height"], "width": x["width"]} for x in host]
    runs = []
    for label, precision, route in VARIANTS:
        cfg, model = build_hot_path_model(seed=0, precision=precision, device="cuda:0")
        cfg.SOLVER.BASE_LR = 1e-4
        model.train()
        runs.append({"label": label, "route": route, "trainer": HotPathTrainer(model, build_optimizer(cfg, model)), "ms": []})

    def one_step(r):
        if r["route"] is None:
            os.environ.pop("WSOVOD_PT_DX", None)
        else:
            os.environ["WSOVOD_PT_DX"] = r["route"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        losses = r["trainer"].run_step(batch)
        r["trainer"].flush()
        e1.record()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v)) for v in losses.values()), (r["label"], losses)
        return e0.elapsed_time(e1)

    for rnd in range(args.warmup + args.steps):
        order = runs[rnd % len(runs):] + runs[:rnd % len(runs)]
        for r in order:
            ms = one_step(r)
            if rnd >= args.warmup:
                r["ms"].append(ms)
    os.environ.pop("WSOVOD_PT_DX", None)
    out = {"workload": f"{args.images} images x 800x600 x {args.proposals} proposals, WSR_18, K = 20, dropout on, one process, "
                       f"variants interleaved step by step; {args.warmup} warm-up + {args.steps} timed steps each, medians",
           "device": torch.cuda.get_device_name(0), "variants": {}}
    for r in runs:
        med = statistics.median(r["ms"])
        out["variants"][r["label"]] = {"ms_per_step": round(med, 3), "images_per_s": round(args.images / med * 1e3, 1),
                                       "ms_min": round(min(r["ms"]), 3), "ms_max": round(max(r["ms"]), 3),
                                       "whole_step_graph": bool(r["trainer"]._graphs)}
        r["trainer"].close()
    v = out["variants"]
    ips = lambda k: v[k]["images_per_s"]
    out["parity_mx_train / parity_train"] = round(ips("parity_mx_train") / ips("parity_train"), 4)
    out["parity_mx_train / parity_mx"] = round(ips("parity_mx_train") / ips("parity_mx"), 4)
    out["bf16x2 dX route / x3 dX route"] = round(ips("parity_mx_train") / ips("parity_mx_train, WSOVOD_PT_DX=x3"), 4)
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
