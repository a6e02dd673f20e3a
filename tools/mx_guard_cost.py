"""What the f16mx range guard (MODEL.HIP.MX_RANGE_GUARD) costs, in ONE process:

    python tools/mx_guard_cost.py [--images 32] [--steps 15] [--warmup 4]      (one MI355X)

  off     "parity_mx", guard off: no audit is ever launched (the default)
  armed   "parity_mx", guard "warn" with MX_RANGE_GUARD_PERIOD = 1: EVERY step audits every f16mx carrier and the trained
          weights' operands, applies its update before the step returns and ends with the guard's one host read

Config-2 shapes (WSR_18, 800x600, 512 proposals, K = 20), dropout on, HotPathTrainer + HipSGD as bench.py drives them.  Both
models resident; they take turns step by step (the order swapped every round).  Every step is bracketed by device events and
followed by a synchronize; the figure of a variant is the MEDIAN of its timed steps.  The amortised cost at a period P is
(armed - off) / P per step.  The audit kernel alone is timed on one large carrier (achieved GB/s over the bytes it reads: three
of a value's four).  Writes profiles/mx_range_guard_cost.json and prints it.
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
from wsovod_amd.modeling import build_model
from wsovod_amd.testing import hot_path_cfg


def build(guard):
    cfg = hot_path_cfg(precision="parity_mx", device="cuda:0")
    cfg.MODEL.HIP.MX_RANGE_GUARD = guard
    cfg.MODEL.HIP.MX_RANGE_GUARD_PERIOD = 1
    cfg.SOLVER.BASE_LR = 1e-4
    torch.manual_seed(0)
    model = build_model(cfg)
    with torch.no_grad():
        model.backbone.stem.conv1.norm.weight.fill_(1.0 / 64.0)  # (testing.build_hot_path_model's calibration)
    model.train()
    return model, HotPathTrainer(model, build_optimizer(cfg, model))


def kernel_rate(gpu, rows=16384, cols=4096, reps=20):
    car, _ = H.mx_encode(torch.randn(rows, cols, device=gpu), unit=True)
    c = torch.zeros(4, dtype=torch.int64, device=gpu)
    for _ in range(3):
        H.mx_range(car, c)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        H.mx_range(car, c)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    assert int(c[0]) == (reps + 3) * rows * cols
    return {"carrier": f"{rows} x {cols} values ({rows * cols * 4 / 1e6:.0f} MB)", "ms": round(ms, 4),
            "GB_per_s_read": round(rows * cols * 3 / ms / 1e6, 1), "GB_per_s_of_the_carrier": round(rows * cols * 4 / ms / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--proposals", type=int, default=512)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mx_range_guard_cost.json"))
    args = ap.parse_args()
    gpu = torch.device("cuda", 0)
    host = make_batch(args.images, args.proposals, 20, seed=123)
    batch = [{"image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu), "instances": x["instances"],
              "height": x["height"], "width": x["width"]} for x in host]
    runs = [{"label": label, "ms": []} for label in ("off", "armed")]
    for r in runs:
        r["model"], r["trainer"] = build("off" if r["label"] == "off" else "warn")

    def one_step(r):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        losses = r["trainer"].run_step(batch)
        r["trainer"].flush()
        e1.record()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v)) for v in losses.values()), (r["label"], losses)
        return e0.elapsed_time(e1)

    for rnd in range(args.warmup + args.steps):
        for r in (runs if rnd % 2 == 0 else runs[::-1]):
            ms = one_step(r)
            if rnd >= args.warmup:
                r["ms"].append(ms)
    guard = runs[1]["model"].mx_guard
    assert guard.polls == args.warmup + args.steps and not any(v.nonfinite or v.top_code for v in guard.last.values())
    audited = sum(v.audited for v in guard.last.values())
    out = {"workload": f"{args.images} images x 800x600 x {args.proposals} proposals, WSR_18, K = 20, parity_mx, dropout on, one "
                       f"process, variants interleaved step by step; {args.warmup} warm-up + {args.steps} timed steps each, medians",
           "device": torch.cuda.get_device_name(0), "variants": {}}
    for r in runs:
        med = statistics.median(r["ms"])
        out["variants"][r["label"]] = {"ms_per_step": round(med, 3), "images_per_s": round(args.images / med * 1e3, 1),
                                       "ms_min": round(min(r["ms"]), 3), "ms_max": round(max(r["ms"]), 3)}
        r["trainer"].close()
    off, armed = (out["variants"][k]["ms_per_step"] for k in ("off", "armed"))
    out["audited_per_armed_step"] = {"sites": len(guard.last), "values": audited, "carrier_GB": round(audited * 4 / 1e9, 3),
                                     "largest_finite_hi": max(v.max_abs for v in guard.last.values())}
    out["armed_minus_off_ms"] = round(armed - off, 3)
    out["amortised_at_period_100"] = f"{(armed - off) / 100 / off * 100:.4f} % of a step"
    out["audit_kernel"] = kernel_rate(gpu)
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
