"""The VGG16 DC5 model's training step, measured: images/s per precision and batch size, the library's per-kernel table, and
the new stride-1 first-conv kernels next to the stride-2 ones, in ONE process:

    python tools/vgg16_step.py [--steps 10] [--warmup 3] [--images 32 8 1]      (one MI355X)

The benchmark's own synthetic image size (800 x 600) and 512 proposals, K = 20, dropout on, HotPathTrainer + HipSGD as
bench.py drives them.  One model per precision ("parity_mx", "parity", "bf16"), all resident; at every batch size the
precisions take turns step by step (the order rotated every round), so that clock and temperature drift lands on all alike.
Every step is bracketed by device events and followed by a synchronize; a figure is the MEDIAN of its timed steps (min / max
beside it).  Then, per-launch event brackets on (captured graphs are bypassed), two "parity_mx" steps at the largest batch give
the per-kernel table; the dominant conv's algorithmic FLOP/s is set against the 2.5 PFLOP/s nameplate.  Last, the four
first-conv kernels run interleaved on the same canvas: achieved OUTPUT bytes/s of stride 1 next to stride 2, same run.
Writes profiles/vgg16_step.json and prints it.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from wsovod_amd import _lib
from wsovod_amd.data import make_batch
from wsovod_amd.engine import HotPathTrainer, build_optimizer
from wsovod_amd.layers import hip_ops as H
from wsovod_amd.testing import build_hot_path_model

PRECISIONS = ("parity_mx", "parity", "bf16")
NAMEPLATE = 2.5e15


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _stat(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def stem_kernels(canvas, sizes_t, mean, std, reps):
    """The four fused first-conv kernels on one canvas, interleaved: time per launch and output bytes/s."""
    dev = canvas.device
    w = torch.randn(64, 32, device=dev) * 0.05
    w[:, 27:] = 0
    b = torch.zeros(64, device=dev)
    wb, wx = w.to(torch.bfloat16), H.x2_encode(w)
    N, _, Hp, Wp = canvas.shape
    s2 = ((Hp - 1) // 2 + 1) * ((Wp - 1) // 2 + 1)
    runs = {  # name -> (launch, output bytes)
        "stem_conv1 (stride 2, bf16)": (lambda: H.stem_conv1(canvas, sizes_t, mean, std, wb, b), N * s2 * 128),
        "stem_conv1_s1 (stride 1, bf16)": (lambda: H.stem_conv1_s1(canvas, sizes_t, mean, std, wb, b), N * Hp * Wp * 128),
        "stem_conv1_x2 (stride 2, bf16x2)": (lambda: H.stem_conv1_x2(canvas, sizes_t, mean, std, wx, b), N * s2 * 256),
        "stem_conv1_s1_x2 (stride 1, bf16x2)": (lambda: H.stem_conv1_s1_x2(canvas, sizes_t, mean, std, wx, b), N * Hp * Wp * 256),
    }
    ms = {k: [] for k in runs}
    for rep in range(reps + 2):
        for k, (fn, _) in runs.items():
            t, out = _timed(fn)
            del out
            if rep >= 2:
                ms[k].append(t)
    out = {}
    for k, (_, nbytes) in runs.items():
        st = _stat(ms[k])
        out[k] = {**st, "output_MB": round(nbytes / 1e6, 1), "output_GB_per_s": round(nbytes / st["ms"] / 1e6, 1),
                  "ns_per_output_KB": round(st["ms"] * 1e6 / (nbytes / 1e3), 3),
                  "ns_per_output_KB_min_max": [round(min(ms[k]) * 1e6 / (nbytes / 1e3), 3), round(max(ms[k]) * 1e6 / (nbytes / 1e3), 3)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[32, 8, 1])
    ap.add_argument("--proposals", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "vgg16_step.json"))
    args = ap.parse_args()
    gpu = torch.device("cuda", 0)
    runs = []
    for precision in PRECISIONS:
        cfg, model = build_hot_path_model(seed=0, backbone="vgg16", precision=precision, device="cuda:0")
        cfg.SOLVER.BASE_LR = 1e-4
        model.train()
        runs.append({"precision": precision, "model": model, "trainer": HotPathTrainer(model, build_optimizer(cfg, model))})
    out = {"workload": f"VGG16 DC5 (CONV5_DILATION 2, FREEZE_AT 5), 800x600 x {args.proposals} proposals, K = 20, dropout on, one "
                       f"process, precisions interleaved step by step; {args.warmup} warm-up + {args.steps} timed steps each, medians",
           "device": torch.cuda.get_device_name(0), "steps": {}}
    batches = {}
    for n in args.images:
        host = make_batch(n, args.proposals, 20, seed=123)
        batch = batches[n] = [{"image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu), "instances": x["instances"],
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
        out["steps"][f"{n} images"] = {p: {**_stat(v), "images_per_s": round(n / statistics.median(v) * 1e3, 2)}
                                       for p, v in ms.items()}
    # ---- the per-kernel table of "parity_mx" at the largest batch ----
    n = max(args.images)
    r = runs[0]
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        for _ in range(2):
            r["trainer"].run_step(batches[n])
            r["trainer"].flush()
        torch.cuda.synchronize()
        table = sorted((e for e in _lib.profile_collect() if e["launches"] > 0), key=lambda e: -e["ms"])
    finally:
        _lib.profile_enable(False)
    total = sum(e["ms"] for e in table)
    out["kernels"] = {"of": f"parity_mx, {n} images, 2 steps (per-launch event brackets: graphs bypassed)", "total_ms": round(total, 3),
                      "table": [{"name": e["name"], "launches": e["launches"], "ms": round(e["ms"], 3),
                                 "share": round(e["ms"] / total, 4),
                                 "TFLOP_per_s": round(e["flops"] / e["ms"] / 1e9, 1) if e["flops"] else None,
                                 "GB_per_s": round(e["bytes"] / e["ms"] / 1e6, 1) if e["bytes"] else None} for e in table[:24]]}
    convs = [e for e in table if e["name"].startswith("conv_") and e["flops"]]
    if convs:
        top = convs[0]
        out["dominant_conv"] = {"name": top["name"], "ms": round(top["ms"], 3),
                                "algorithmic_fraction_of_2.5_PFLOP_per_s": round(top["flops"] / (top["ms"] * 1e-3) / NAMEPLATE, 4)}
    canvas, sizes_t, _ = r["model"]._canvas(batches[n])
    out["first_conv_kernels"] = {"of": f"{n} images, one canvas, kernels interleaved, 7 timed launches each, medians",
                                 **stem_kernels(canvas, sizes_t, r["model"]._mean, r["model"]._std, 7)}
    for r in runs:
        r["trainer"].close()
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
