"""MIST pseudo-GT mining, measured, in ONE process:

    python tools/mist_step.py [--images 1 8 32]      (one MI355X)

Part (a): the mining + labelling stage (get_pgt_mist + the matching of label_and_sample_proposals_wsl) at 800 x 600,
4000 + 1024 = 5024 boxes per image, K = 20, 3 image-level classes per image, on the SAME inputs
  hip    hip_ops.mist_mine_and_label (select, merge, NMS mask + scan, label: five launches, no host read)
  torch  the reference's formulation in torch ops on the device: tests/mist_util.py moved to the GPU (per image and per
         class list comprehensions, a host loop inside the NMS)
the two taking turns run by run, 3 warm-up + 15 timed rounds, medians with min / max (the spread).
Part (b): the eager "parity_mx" training step of hot_path_r18_mist.yaml next to hot_path_wsr18.yaml (top-1 mining),
interleaved step by step; the synthetic batch carries 2 image-level classes per image (wsovod_amd.data.make_batch).
Writes profiles/mist_step.json and prints it.  A difference below the larger of the two spreads is reported as such."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tests import mist_util as U
from wsovod_amd.data import make_batch
from wsovod_amd.engine import build_optimizer, run_step
from wsovod_amd.layers import hip_ops as H
from wsovod_amd.testing import build_hot_path_model

R, K, C, HH, WW = 5024, 20, 3, 600, 800


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _stat(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def _ab(forms, rounds, warmup):
    ms = {k: [] for k in forms}
    names = list(forms)
    for rnd in range(warmup + rounds):
        for name in (names if rnd % 2 == 0 else names[::-1]):
            t, _ = _timed(forms[name])
            if rnd >= warmup:
                ms[name].append(t)
    out = {k: _stat(v) for k, v in ms.items()}
    a, b = (out[n] for n in names)
    out["spread_ms"] = round(max(a["ms_max"] - a["ms_min"], b["ms_max"] - b["ms_min"]), 4)
    out["difference_exceeds_spread"] = bool(abs(a["ms"] - b["ms"]) > out["spread_ms"])
    return out


def stage(n_img, dev, rounds, warmup):
    gen = torch.Generator().manual_seed(n_img)
    batch = make_batch(n_img, R, K, H=HH, W=WW, seed=7)
    boxes = [b["proposals"].proposal_boxes.tensor.to(dev) for b in batch]
    scores = [torch.softmax(torch.randn(R, K + 1, generator=gen) * 3, dim=1).to(dev) for _ in range(n_img)]
    classes = [torch.randperm(K, generator=gen)[:C].sort()[0].to(dev) for _ in range(n_img)]
    seg = torch.arange(0, (n_img + 1) * R, R, dtype=torch.int32, device=dev)
    gt_off = torch.arange(0, (n_img + 1) * C, C, dtype=torch.int32, device=dev)
    boxes_cat, scores_cat, gt_cat = torch.cat(boxes), torch.cat(scores), torch.cat(classes)
    forms = {
        "hip": lambda: H.mist_mine_and_label(scores_cat, boxes_cat, seg, gt_cat, gt_off, K, 0.5, max_rows=R, max_classes=C),
        "torch": lambda: U.mine_and_label(boxes, scores, classes, K, 0.5),
    }
    out = _ab(forms, rounds, warmup)
    o = forms["hip"]()
    out["targets_per_image"] = o["pgt_count"].cpu().tolist()[:4]
    return out


def step(n_img, dev, rounds, warmup):
    models = {}
    for name, mist in (("mist", True), ("top1", False)):
        cfg, model = build_hot_path_model(seed=0, precision="parity_mx", device=dev, mist=mist)
        model.train()
        models[name] = (model, build_optimizer(cfg, model))
    batch = make_batch(n_img, R, K, H=HH, W=WW, seed=11)
    forms = {name: (lambda m=m, o=o: run_step(m, o, batch)) for name, (m, o) in models.items()}
    return _ab(forms, rounds, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-images", type=int, nargs="*", default=None, help="image counts of part (b); default: --images")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mist_step.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "boxes_per_image": R, "K": K, "classes_per_image": C,
           "image": [HH, WW], "rounds": a.rounds, "warmup": a.warmup, "stage": {}, "step_parity_mx": {}}
    for n in a.images:
        res["stage"][str(n)] = stage(n, dev, a.rounds, a.warmup)
        if n in (a.images if a.step_images is None else a.step_images):
            res["step_parity_mx"][str(n)] = step(n, dev, a.rounds, a.warmup)
            torch.cuda.empty_cache()
        print(n, json.dumps({k: res[k][str(n)] for k in ("stage", "step_parity_mx") if str(n) in res[k]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
