"""Test-time augmentation (TTA-AVG) per image, host route next to device route (MODEL.HIP.TTA_DEVICE), measured in ONE process:

    python tools/tta_step.py [--steps 15] [--warmup 2]      (one MI355X)

R18 under "parity_mx" in eval mode, 4000 loaded proposals, the shipped TEST.AUG.MIN_SIZES (480 ... 1152) plus flip = 16 views,
on one 500 x 375 image (the VOC size) and one 800 x 600 image.  The two routes take turns call by call, so that clock and
temperature drift lands on both alike.  A round times, per route, (a) the whole wrapper call and then (b) a second call whose
two stages are bracketed on their own -- building the views (the mapper) and the merge input (back-mapping + mean over the
views: the wrapper's prediction stage less the forwards inside it) -- each between device synchronisations, which is why
(b) is not added into (a).  Host clock around work that ends in a synchronise; a figure is the MEDIAN of its timed calls with min / max beside it.  Before timing, the two routes' averaged
tensors are compared once (they differ by the rounding of the mean only).  Writes profiles/tta_device.json and prints it.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from wsovod_amd.data import make_batch
from wsovod_amd.modeling import GeneralizedRCNNWithTTAAVG
from wsovod_amd.modeling.tta_device import DatasetMapperTTAAVG
from wsovod_amd.testing import build_hot_path_model

MIN_SIZES = (480, 576, 672, 768, 864, 960, 1056, 1152)  # the shipped TEST.AUG.MIN_SIZES; TEST.AUG.MAX_SIZE 4000, FLIP on
IMAGES = ((375, 500), (600, 800))


def _stat(ms):
    return {"ms": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class Staged:
    """A wrapper whose stages are clocked on their own while `on`: the mapper, and the merge input = `_get_augmented_boxes`
    less the `_run_model` inside it (each clocked between synchronisations)."""

    def __init__(self, tta):
        self.tta, self.on, self.ms, self.avg = tta, False, {"views": 0.0, "forwards": 0.0, "merge": 0.0}, None
        mapper, run_model, get_boxes = tta.tta_mapper, tta._run_model, tta._get_augmented_boxes

        def timed(name, fn):
            def call(*a):
                if not self.on:
                    return fn(*a)
                self.ms[name], out = _clock(lambda: fn(*a))
                return out
            return call

        def merge(*a):
            if not self.on:
                self.avg = get_boxes(*a)[:2]
                return (*self.avg, None)
            t, out = _clock(lambda: get_boxes(*a))
            self.ms["merge"] = t - self.ms["forwards"]
            return out

        tta.tta_mapper, tta._run_model, tta._get_augmented_boxes = timed("views", mapper), timed("forwards", run_model), merge


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proposals", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "tta_device.json"))
    args = ap.parse_args()
    gpu = torch.device("cuda", 0)
    cfg, model = build_hot_path_model(seed=0, precision="parity_mx", device="cuda:0")
    model.eval()
    routes = {}
    for name, dv in (("host", False), ("device", True)):
        mapper = DatasetMapperTTAAVG(list(MIN_SIZES), 4000, True, 0, device_views=gpu if dv else False)
        routes[name] = Staged(GeneralizedRCNNWithTTAAVG(cfg, model, mapper, device_views=dv))
    out = {"workload": f"R18 parity_mx, eval, TTA-AVG, {args.proposals} loaded proposals, MIN_SIZES {list(MIN_SIZES)} x flip = "
                       f"{2 * len(MIN_SIZES)} views, batch_size 1; one process, routes interleaved call by call; {args.warmup} warm-up + "
                       f"{args.steps} timed rounds, medians (host clock, synchronised)",
           "device": torch.cuda.get_device_name(0), "images": {}}
    for h, w in IMAGES:
        inp = make_batch(1, args.proposals, 20, H=h, W=w, seed=123)[0]
        inp = {k: inp[k] for k in ("image", "proposals", "height", "width")}
        ms = {r: {"call": [], "views": [], "merge": []} for r in routes}
        for rnd in range(args.warmup + args.steps):
            order = list(routes) if rnd % 2 == 0 else list(routes)[::-1]
            for r in order:
                t, res = _clock(lambda: routes[r].tta([inp]))
                assert bool(torch.isfinite(res[0]["instances"].scores).all())
                if rnd >= args.warmup:
                    ms[r]["call"].append(t)
            for r in order:
                routes[r].on = True
                routes[r].tta([inp])
                routes[r].on = False
                if rnd >= args.warmup:
                    ms[r]["views"].append(routes[r].ms["views"])
                    ms[r]["merge"].append(routes[r].ms["merge"])
        hb, hs = routes["host"].avg
        db, ds = routes["device"].avg
        out["images"][f"{w} x {h}"] = {
            "avg_max_abs_diff_device_vs_host": {"boxes": float((hb - db).abs().max()), "scores": float((hs - ds).abs().max())},
            **{r: {"whole_call": _stat(v["call"]), "views_stage": _stat(v["views"]), "merge_stage": _stat(v["merge"])}
               for r, v in ms.items()}}
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
