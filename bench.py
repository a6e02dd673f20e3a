#!/usr/bin/env python3
"""Benchmark of the WSOVOD hot path on MI355X (contract: see the task statement / DESIGN.md).

One "step" = one full training iteration of WSOVOD_WSR_18_DC5 in proposals-only mode on a batch of
synthetic 800x600 images with 512 proposals each: uint8 image -> fused normalise+stem -> frozen
backbone -> RoIPool(+objectness) -> neck -> object mining (MIL) -> pseudo-GT mining/labelling ->
instance refinement (cosine-similarity head) -> losses -> backward -> fused SGD step
(reference: wsovod/engine/trainer.py:37-84).  Inputs are resident in HBM before the timed region.

  python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run)
  python bench.py --gpus 1 --steps K --warmup W --full   (+ roofline pass, oracle comparisons, side lines, CPU baseline)
  python bench.py ... --dump-outputs DIR                  (+ the last timed step's outputs as DIR/<name>.npy)

Prints ONE JSON line on rank 0.  `value` = images/sec over all N GPUs (weak scaling: per-GPU batch fixed).
A plain run (no --full) does only what that headline needs: set-up, warm-up, the K timed steps, the line.
The default precision is "parity_mx" (round 6) -- the "parity" mode, which meets the north star's bound (MIL-head logits
within 1e-3 of the reference path, proposal indexing bit-exact), with its big forward contractions (res4 / res5 convs, fc1 /
fc2) on the block-scaled f16mx kernels: at N = 1 --full the line carries that comparison, made with the oracle on the timed batch
itself (the oracle is the checker here, never the thing measured), `roofline.frac` counts ALGORITHMIC flops (the executed
matrix-pipe work travels as `executed_frac`), and "parity" (bf16x2 everywhere) and plain bf16 are `side` lines.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# the arithmetic type the path computes in (bench contract: not a precision claim -- that is the `parity` object)
DTYPE = {"parity": "bf16 (bf16x2 hi/lo activations, three MFMA products per value pair forward; plain bf16 backward; fp32 "
                   "accumulation, master weights, losses and optimizer)",
         "bf16": "bf16", "fp32": "f32", "bf16x3": "bf16 (hi/lo split operands, forward and backward)",
         "bf16x3f": "bf16 (hi/lo split operands forward, plain bf16 backward)",
         "parity_mx": "bf16 / fp16 + MX fp8 (the parity forward with the res4 / res5 convs and fc1 / fc2 on fp16 hi*hi + block-scaled "
                      "e4m3 cross terms -- two v_mfma_f32_32x32x16_f16 + one v_mfma_scale_f32_32x32x64_f8f6f4 per 32x32x32 tile --, "
                      "bf16x2 three-product forward elsewhere; plain bf16 backward; fp32 accumulation, master weights, losses "
                      "and optimizer)",
         "parity_train": "bf16 (the parity forward; the input-gradient contractions of the backward keep the hi/lo split: "
                         "three bf16 MFMA products on fp32 gradients and fp32 master weights)"}
PEAK = {"bf16": 2500.0, "fp32": 157.3, "bf16x3": 2500.0, "bf16x3f": 2500.0, "parity": 2500.0, "parity_train": 2500.0,
        "parity_mx": 2500.0}  # dense MFMA TFLOP/s (MI355X_MICROARCH.md); x3 runs bf16 MFMAs
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU per step")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for debugging)")
    ap.add_argument("--share-device", action="store_true",
                    help="debug: every rank uses cuda:0 (lets the N>1 code path run on a 1-GPU box with --backend gloo)")
    ap.add_argument("--precision", default="parity_mx", choices=["parity", "parity_mx", "parity_train", "bf16", "fp32", "bf16x3", "bf16x3f"],
                    help="parity_mx (default, the headline since round 6) = parity with the res4 / res5 convs and fc1 / fc2 on the "
                         "block-scaled f16mx kernels (fp16 hi*hi + MX-e4m3 cross terms: two thirds of the matrix-pipe cycles); "
                         "parity = the mode that MEETS the north star's 1e-3 logit bound with exact "
                         "proposal indexing: bf16 MFMA arithmetic on bf16x2 (hi, lo) activations, three products per value "
                         "pair in the forward pass, plain bf16 backward; bf16 = plain bf16 MFMA (BASELINE config 2's dtype, "
                         "misses the bound: a side line); fp32 = exact-fp32 MFMA; bf16x3 / bf16x3f = round 2's split forms")
    ap.add_argument("--depth", type=int, default=18)
    ap.add_argument("--proposals", type=int, default=512)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--embed-dim", type=int, default=512)
    ap.add_argument("--pooler", default="ROIPool")
    ap.add_argument("--rpn", action="store_true",
                    help="the shipped form of the config: RPN branch on next to the loaded proposals (SURVEY 8f n1); "
                         "not the north-star workload, so no CPU baseline is taken")
    ap.add_argument("--grad-wire", default="auto", choices=["auto", "fp32", "bf16"],
                    help="gradient all-reduce format at N>1: auto = the compute precision (bf16 run -> bf16 wire, the "
                         "counterpart of the reference's fp16 compression hook; master weights/momentum stay fp32)")
    ap.add_argument("--exchange", default="auto", choices=["auto", "ring", "direct"],
                    help="bf16 wire at N>1: ring = RCCL all-reduce (running sum rounded to bf16 at every hop); direct = "
                         "all-to-all of shards over the xGMI mesh + fp32 sum with one rounding + all-gather; "
                         "auto = direct from 3 ranks up")
    ap.add_argument("--one-rank-group", action="store_true",
                    help="debug/measurement: at N=1 still create a 1-rank RCCL group, so that the whole exchange path "
                         "(gradient pack, split weight-gradient launch, collectives, SGD on the wire slices) runs and "
                         "its cost without any wire time can be read off one GPU")
    ap.add_argument("--eval", action="store_true",
                    help="side measurement, not the headline metric: images/s of model.inference() (eval mode: frozen "
                         "backbone, RoI pooling, heads, score threshold + per-class NMS tail) on the same synthetic batch")
    ap.add_argument("--launch-check", action="store_true",
                    help="launcher self-test (no GPU work): every rank joins the group, all-reduces its rank and rank 0 "
                         "prints {n_gpus, ranks_seen}; with --backend gloo it runs on a CPU-only host (tests/test_bench_launcher.py)")
    ap.add_argument("--h2d", action="store_true",
                    help="stage the uint8 images of every step from pinned host memory (asynchronous copy on a side "
                         "stream, double buffered) instead of keeping the batch resident in HBM")
    ap.add_argument("--no-side", action="store_true", help="skip the short side measurements (N=1 only)")
    ap.add_argument("--side-steps", type=int, default=10)
    ap.add_argument("--no-parity", action="store_true", help="skip the per-precision deviation from the ORACLE at full size")
    ap.add_argument("--parity-images", type=int, default=2, help="images of the per-precision comparison with the oracle")
    ap.add_argument("--no-parity-at-batch", action="store_true",
                    help="skip the comparison of the HEADLINE precision with the oracle at the timed batch size itself "
                         "(~1 min of host CPU for the oracle's step at 32 images)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the roofline pass (hipEvent kernel table), the per-precision and "
                         "at-batch comparisons with the oracle, the side lines and the CPU baseline (each still switched "
                         "off by its --no-* flag).  Without it a run sets up, warms up, times --steps steps and prints the "
                         "headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step handed its caller to DIR/<name>.npy "
                         "(float32): the step's losses and, after the deferred update, a fixed seeded sample of every "
                         "trained tensor (--eval: the detections of the last timed call)")
    args = ap.parse_args()
    if not args.full:
        args.no_side = args.no_parity = args.no_cpu_baseline = args.no_roofline = True
    return args


def pmc_traffic(kernel_name, args):
    """HBM/fabric bytes per launch of `kernel_name` from the committed rocprofv3 PMC passes (FETCH_SIZE and
    WRITE_SIZE cannot be collected from inside this process).  Only returned when the run matches the
    profiled workload; otherwise null."""
    import re

    path = None
    prec = args.precision
    for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):  # newest committed PMC pass of this workload (written by tools/collect_profiles.sh)
        cand = os.path.join(ROOT, "profiles", f"{rnd}_pmc_traffic_b{args.batch}_{prec}.json")
        if os.path.exists(cand):
            path = cand
            break
    if not (path and prec in ("bf16", "parity", "parity_mx") and args.depth == 18 and args.proposals == 512):
        return None, None
    if getattr(args, "rpn", False) or args.pooler != "ROIPool" or args.h2d:
        return None, None
    m = re.match(r"(gemm_nt|conv_igemm)_(bf16x2|bf16|f32|f16mx)_(\d+)x(\d+)(_dma|_8ph)?$", kernel_name)
    if not m:
        return None, None
    conv, x3 = m.group(1) == "conv_igemm", m.group(2) == "bf16x2"
    if m.group(2) == "f16mx":  # csrc/gemm8mx.hip: gemm256_mx_kernel<CONV, EPI> -- one instantiation per epilogue form
        tags = ("gemm256_mx_kernel<%s," % ("true" if conv else "false"), "gemm256_mx_kernel<%s>" % ("true" if conv else "false"))
    elif m.group(5) == "_8ph":  # rocprofv3 prints this one demangled: gemm256_8ph_kernel<CONV, X3, PH, LEAN>
        c, x = ("true" if conv else "false"), ("true" if x3 else "false")
        tags = (f"gemm256_8ph_kernel<{c}, {x},", f"gemm256_8ph_kernel<{c}>") if not x3 else (f"gemm256_8ph_kernel<{c}, {x},",)
    else:
        tags = ("gemm_nt_kernelI%sLi%sELi%sELb%dELi4ELi4ELb1ELi2ELb%dE" % ("f" if m.group(2) == "f32" else "DF16b", m.group(3),
                                                                          m.group(4), conv, x3),
                "gemm_nt_kernelI%sLi%sELi%sELb%dELi4ELi4ELb1ELi2EEE" % ("f" if m.group(2) == "f32" else "DF16b", m.group(3),
                                                                       m.group(4), conv))
    with open(path) as f:
        table = json.load(f)["kernels"]
    hits = [v for k, v in table.items() if any(t in k for t in tags)]
    if not hits or (len(hits) != 1 and m.group(2) != "f16mx"):
        return None, None
    # (f16mx: the kernel's instantiations -- epilogue forms, the split-K last rounds -- as one family: launch-weighted mean)
    n = sum(max(1, int(v.get("launches_sampled", 1))) for v in hits)
    traffic = sum(v["traffic_bytes_per_launch"] * max(1, int(v.get("launches_sampled", 1))) for v in hits) / n
    return traffic, (f"profiles/{os.path.basename(path)}: builder-run rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this "
                     f"command, NOT measured in this run" + ("; launch-weighted mean over the kernel's instantiations"
                                                              if len(hits) > 1 else ""))


def to_device_batch(batch, dev):
    """The resident form of one batch: the images as per-image views of ONE collated device tensor (what a collate
    function that batches before the copy hands over), the reference's list-of-dicts format otherwise unchanged."""
    import torch
    out = []
    shapes = {tuple(x["image"].shape) for x in batch}
    images = torch.stack([x["image"] for x in batch]).to(dev) if len(shapes) == 1 else None
    for i, x in enumerate(batch):
        out.append({"image": images[i] if images is not None else x["image"].to(dev), "proposals": x["proposals"].to(dev),
                    "instances": x["instances"],  # image-level labels stay on the host (no sync to read them)
                    "height": x["height"], "width": x["width"]})
        if "dataset_id" in x:
            out[-1]["dataset_id"] = x["dataset_id"]
    return out


DUMP_SAMPLE = 1 << 16  # --dump-outputs: elements kept of each trained tensor
DUMP_LIMIT = 64 << 20  # --dump-outputs: bytes written at most


def step_outputs(model, losses):
    """--dump-outputs of a training step: its losses and the trained tensors after its update, each tensor larger than
    DUMP_SAMPLE elements as a sample at fixed indices (seeded by the tensor's name: the same elements in every run)."""
    import zlib

    out = {k: torch.tensor([float(v)], dtype=torch.float32) for k, v in sorted(losses.items())}  # (keys: loss_*)
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        flat = p.detach().reshape(-1)
        if flat.numel() > DUMP_SAMPLE:
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            idx = torch.randint(flat.numel(), (DUMP_SAMPLE,), generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        out[f"param.{name}"] = flat.float().cpu()
    return out


def detection_outputs(results):
    """--dump-outputs of an inference call (--eval): the detections of every image, concatenated in image order."""
    inst = [r["instances"] for r in results]
    return {"det_boxes": torch.cat([x.pred_boxes.tensor.float().cpu() for x in inst]),
            "det_scores": torch.cat([x.scores.float().cpu() for x in inst]),
            "det_classes": torch.cat([x.pred_classes.float().cpu() for x in inst]),
            "det_image": torch.cat([torch.full((len(x),), float(i)) for i, x in enumerate(inst)])}


def write_outputs(dirname, arrays):
    import numpy as np

    total = sum(a.numel() * 4 for a in arrays.values())
    if total > DUMP_LIMIT:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT}-byte limit")
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a.numpy().astype(np.float32))


def cpu_baseline(model, sd, batch, args):
    """The oracle (CPU restatement of the reference path) timed on the host cores: baseline only."""
    from oracle import wsovod_ref as R

    host_cores = os.cpu_count() or 1
    train_keys = [k for k, p in model.named_parameters() if p.requires_grad]
    for k in train_keys:
        sd[k].requires_grad_(True)
    sample = R.batch_from_inputs(batch[:1])
    bufs = {}

    def step():
        losses, _ = R.train_forward(sd, sample, depth=args.depth, num_classes=args.classes, pooler_type=args.pooler)
        total = sum(losses.values())
        grads = torch.autograd.grad(total, [sd[k] for k in train_keys], allow_unused=True)
        with torch.no_grad():
            for k, g in zip(train_keys, grads):
                if g is None:
                    continue
                g = g + 5e-4 * sd[k]
                bufs[k] = g if k not in bufs else bufs[k].mul_(0.9).add_(g)
                sd[k].sub_(0.01 * bufs[k])

    # pick the thread count the host runs this path fastest at (all cores oversubscribe the small ops)
    best = None
    for nt in sorted({host_cores, min(host_cores, 64), min(host_cores, 32), min(host_cores, 16)}, reverse=True):
        torch.set_num_threads(nt)
        if best is None:
            step()  # warm-up (also builds/loads the C oracle)
        t0 = time.time()
        step()
        dt = time.time() - t0
        if best is None or dt < best[1]:
            best = (nt, dt)
    ncores = best[0]
    torch.set_num_threads(ncores)
    n, t0, per_step = 0, time.time(), []
    while True:  # at least 3 repeats (the pool's hosts differ by 2x from run to run: the MEDIAN step is reported)
        t1 = time.time()
        step()
        per_step.append(time.time() - t1)
        n += 1
        if (time.time() - t0 > args.cpu_seconds and n >= 3) or n >= 8:
            break
    dt = sorted(per_step)[len(per_step) // 2] * n  # n x the median step
    # share of the single-thread C RoIPool inside one step (so that nobody reads the GPU/CPU ratio as kernel credit)
    from oracle import roi_ops
    feat = torch.randn(1, 512 if args.depth == 18 else 2048, 75, 100)
    rois = torch.cat([torch.zeros(len(sample[0]["boxes"]), 1), sample[0]["boxes"]], dim=1)
    t1 = time.time()
    roi_ops.roi_pool_forward(feat, rois, 0.125, (7, 7))
    pool_s = time.time() - t1
    return {"value": n / dt, "unit": "images/sec", "cores": ncores, "kind": "port",
            "statistic": f"median of {n} steps", "step_seconds": [round(v, 3) for v in per_step],
            "value_min_max": [1.0 / max(per_step), 1.0 / min(per_step)],
            "roi_pool_share_of_step": round(pool_s / (dt / n), 3),
            "sample": f"{n} full fp32 training steps of 1 image x {args.proposals} proposals (oracle/wsovod_ref.py, "
                      f"torch {torch.__version__} CPU, {ncores} of {host_cores} host threads = fastest of 16/32/64/all); "
                      f"the RoIPool leg is the SINGLE-THREAD C oracle = {pool_s:.2f} s of the {dt / n:.2f} s step "
                      f"({100 * pool_s / (dt / n):.0f} %): a baseline, not a tuned CPU implementation"}


def eval_bench(args, cfg, model, dev, result_fd):
    """Inference throughput (1 GPU): model.inference(batch) with the class text embeddings given per call."""
    from wsovod_amd.data import make_batch

    model.eval()
    batch = to_device_batch(make_batch(args.batch, args.proposals, args.classes, seed=1234), dev)
    g = torch.Generator().manual_seed(7)
    classifier = torch.randn(args.classes, args.embed_dim, generator=g).to(dev)
    for _ in range(args.warmup):
        out = model.inference(batch, classifier=classifier)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = model.inference(batch, classifier=classifier)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        write_outputs(args.dump_outputs, detection_outputs(out))
    elapsed_np = None
    if args.full:  # side figure: the same calls without the detector post-processing
        t1 = time.perf_counter()
        for _ in range(args.steps):
            model.inference(batch, classifier=classifier, do_postprocess=False)
        torch.cuda.synchronize()
        elapsed_np = time.perf_counter() - t1
    res = {"metric": "inference images/sec (side measurement)", "value": args.batch * args.steps / elapsed,
           "unit": "images/sec", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "dtype": args.precision,
           "data": "synthetic",
           "config": {"workload": f"WSR_{args.depth}_DC5 inference, {args.proposals} proposals/img, {args.classes} classes, "
                                  f"{args.pooler}, score threshold + per-class NMS + top-100 tail", "images_per_step": args.batch,
                      "ms_per_step_without_detector_postprocess": elapsed_np / args.steps * 1e3 if elapsed_np else None,
                      "detections_first_image": int(len(out[0]["instances"]))}}
    os.write(result_fd, (json.dumps(res) + "\n").encode())
    return 0


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks here, one process per GPU, as
    the reference's `launch(main, num_gpus)` does (/root/reference/tools/train_net.py:80-90).  The parent never
    touches the GPU (no HIP call, no exec after one): it only spawns children, relays rank 0's JSON line and
    returns non-zero if any rank fails.  Every child gets its share of the host threads (OMP_NUM_THREADS = cores // N);
    rank 0's stdout is drained by a reader thread (a line longer than the pipe buffer must not block it); a launch that
    dies within its first seconds (the rendezvous port was taken between probing and binding) is retried on a new port."""
    import threading

    cores = os.cpu_count() or 1
    for attempt in range(3):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        procs = []
        t_start = time.time()
        for r in range(args.gpus):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WSOVOD_BENCH_CHILD="1")
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this driver
            env.setdefault("OMP_NUM_THREADS", str(max(1, cores // args.gpus)))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=subprocess.PIPE if r == 0 else sys.stderr))
        chunks = []
        reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
        reader.start()
        rc = 0
        try:
            pending = set(range(args.gpus))
            while pending:
                for r in sorted(pending):
                    code = procs[r].poll()
                    if code is None:
                        continue
                    pending.discard(r)
                    if code != 0:
                        rc = rc or code
                        print(f"bench.py: rank {r} exited with code {code}", file=sys.stderr)
                if rc:  # a dead rank leaves the others waiting in a collective: stop exactly the children started here
                    for r in pending:
                        procs[r].terminate()
                    for r in pending:
                        try:
                            procs[r].wait(timeout=20)
                        except subprocess.TimeoutExpired:
                            procs[r].kill()
                    break
                time.sleep(0.05)
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        reader.join(timeout=30)
        line = b"".join(chunks)
        if rc and time.time() - t_start < 15 and attempt < 2 and not os.environ.get("WSOVOD_BENCH_FAIL_RANK"):
            print(f"bench.py: launch attempt {attempt + 1} died within {time.time() - t_start:.0f} s: retrying on a new port",
                  file=sys.stderr)
            continue
        break
    lines = [x for x in line.decode().splitlines() if x.strip()]
    if rc == 0 and (len(lines) != 1 or json.loads(lines[0]).get("n_gpus") != args.gpus):
        print(f"bench.py: expected one JSON line with n_gpus={args.gpus} from rank 0, got {lines!r}", file=sys.stderr)
        rc = 1
    if rc == 0:
        sys.stdout.write(lines[0] + "\n")
        sys.stdout.flush()
    return rc


def launch_check(args, world, rank, result_fd):
    """The launcher path without GPU work: group creation, one all-reduce, one JSON line."""
    if os.environ.get("WSOVOD_BENCH_FAIL_RANK") == str(rank):  # tests: a rank that dies before joining the group
        raise SystemExit(3)
    dist.init_process_group(args.backend)
    t = torch.tensor([1 << rank], dtype=torch.int64)
    if args.backend == "nccl":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        t = t.cuda()
    dist.all_reduce(t)
    if rank == 0:
        os.write(result_fd, (json.dumps({"metric": "launch-check", "n_gpus": dist.get_world_size(),
                                         "ranks_seen": int(t.item()), "backend": args.backend}) + "\n").encode())
    dist.barrier()
    dist.destroy_process_group()
    return 0


def pct(xs, q):
    xs = sorted(xs)
    if not xs:
        return None
    k = (len(xs) - 1) * q
    lo, hi = int(k), min(int(k) + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (k - lo)


class H2DStager:
    """The a1 input copy inside the timed region: the uint8 images (46 MB per 32 x 800x600 step) and the proposal
    boxes of every step travel from pinned host memory on a side stream, double buffered, while the previous step
    computes; the step's stream waits on the copy event (reference: rcnn_wsovod.py:321-328 `x["image"].to(device)`).
    Round 6: the host side is what a pinning collate function hands over -- ONE pinned uint8 batch tensor, one pinned box /
    objectness tensor -- so a step is three asynchronous copies into preallocated device slots (96 small ones before), and
    the per-image dicts are adjacent views of the device canvas (the model takes them as they are: no gather pass)."""

    def __init__(self, host_batch, dev):
        from wsovod_amd.structures import Boxes, Instances

        self.dev = dev
        self.stream = torch.cuda.Stream(device=dev)
        shapes = {tuple(x["image"].shape) for x in host_batch}
        assert len(shapes) == 1, "the bench batch has one image size"
        self.h_img = torch.stack([x["image"] for x in host_batch]).pin_memory()
        self.h_box = torch.cat([x["proposals"].proposal_boxes.tensor for x in host_batch]).pin_memory()
        self.h_obj = torch.cat([x["proposals"].objectness_logits for x in host_batch]).pin_memory()
        nums = [len(x["proposals"]) for x in host_batch]
        self.slots, self.events = [], [None, None]
        for _ in range(2):
            canvas = torch.empty(self.h_img.shape, dtype=torch.uint8, device=dev)
            box = torch.empty(self.h_box.shape, dtype=self.h_box.dtype, device=dev)
            obj = torch.empty(self.h_obj.shape, dtype=self.h_obj.dtype, device=dev)
            batch, r = [], 0
            for i, (x, m) in enumerate(zip(host_batch, nums)):
                props = Instances(x["proposals"].image_size, proposal_boxes=Boxes(box[r:r + m]), objectness_logits=obj[r:r + m])
                batch.append({"image": canvas[i], "proposals": props, "instances": x["instances"], "height": x["height"],
                              "width": x["width"]})
                r += m
            self.slots.append((canvas, box, obj, batch))
        self.i = 0
        self._issue(0)

    def _issue(self, k):
        canvas, box, obj, _ = self.slots[k]
        # the slot's previous consumer (two steps ago) has been enqueued on the compute stream: order the copy behind it
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.stream):
            canvas.copy_(self.h_img, non_blocking=True)
            box.copy_(self.h_box, non_blocking=True)
            obj.copy_(self.h_obj, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.events[k] = ev

    def next(self):
        k = self.i & 1
        torch.cuda.current_stream().wait_event(self.events[k])
        batch = self.slots[k][3]
        self.i += 1
        self._issue(self.i & 1)
        return batch


def _agree(flag, dev, op):
    """All ranks learn the MIN / MAX of a per-rank number (one tiny all-reduce on the bench's own process group)."""
    t = torch.tensor([float(flag)], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=op)
    return float(t.item())


def pick_exchange(trainer, step, sync, dev, algos=("ring", "direct"), warm=2, steps=4):
    """N > 1, bf16 wire: time BOTH gradient exchanges in this run, in this process (`trainer.set_exchange`), a few steps
    each after a short warm-up, and leave the trainer on the faster one.  An algorithm that raises or produces a
    non-finite loss on ANY rank is dropped on EVERY rank (the ranks agree through an all-reduce of an ok flag) and its
    half-finished exchange is aborted -- never a re-exec, never a second process on a GPU that was touched.  Returns
    {"ms": {algo: ms_per_step | None}, "errors": {algo: text}, "chosen": algo}."""
    ms, errors = {}, {}
    for algo in algos:
        ok, err = 1.0, None
        try:
            trainer.set_exchange(algo)
            for _ in range(warm):
                last = step()
            trainer.flush()
            if not all(bool(torch.isfinite(v.detach()).all()) for v in last.values()):
                ok, err = 0.0, "non-finite loss during warm-up"
        except Exception as e:  # noqa: BLE001 -- whatever the collective raised: fall back, in process
            ok, err = 0.0, f"{type(e).__name__}: {e}"[:300]
        if _agree(ok, dev, dist.ReduceOp.MIN) < 1.0:
            errors[algo] = err or "failed on another rank"
            ms[algo] = None
            trainer.abort_pending()
            continue
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        trainer.flush()
        sync()
        ms[algo] = _agree((time.perf_counter() - t0) / steps * 1e3, dev, dist.ReduceOp.MAX)  # the slowest rank's time
    good = [a for a in algos if ms.get(a) is not None]
    if not good:
        raise RuntimeError(f"no gradient exchange worked: {errors}")
    chosen = min(good, key=lambda a: ms[a])
    trainer.set_exchange(chosen)
    return {"ms": ms, "errors": errors, "chosen": chosen}


def run_config(args, dev, rank, world, *, precision, batch_size, pooler, steps, warmup, h2d=False, rpn=False,
               want_roofline=False, keep=False, depth=None, proposals=None, classes=None, embed_dim=None, mixed=False,
               dump=False):
    """Build the model, run `warmup` + `steps` training steps, return the timing record (and the live objects if keep).
    mixed: the mixed-dataset model (BASELINE config 5), every step drawn from its largest-vocabulary source.
    dump: the record carries `outputs`, what the last timed step handed its caller (step_outputs)."""
    from wsovod_amd import _lib
    from wsovod_amd.data import make_batch
    from wsovod_amd.engine import HotPathTrainer, build_optimizer
    from wsovod_amd.testing import build_hot_path_model, build_mixed_model

    depth, proposals = depth or args.depth, proposals or args.proposals
    classes, embed_dim = classes or args.classes, embed_dim or args.embed_dim
    if mixed:
        cfg, model = build_mixed_model(seed=0, names=("voc_2007_train", "coco_2017_train", "lvis_v1_train"),
                                       Ks=(20, 80, classes), D=embed_dim, depth=depth, precision=precision, pooler=pooler,
                                       device=str(dev))
    else:
        cfg, model = build_hot_path_model(seed=0, depth=depth, K=classes, D=embed_dim, precision=precision,
                                          pooler=pooler, device=str(dev), rpn=rpn)
    if rpn:
        model.roi_heads.iter = cfg.SOLVER.MAX_ITER // 2  # mid-training objectness ramp (rcnn_wsovod.py:181-184)
    model.train()
    # the config's BASE_LR 0.01 is reached through detectron2's warm-up in the reference; on the random-init synthetic
    # model it oscillates from the first step, so the benchmark trains at the warm-up-phase rate (throughput is unaffected,
    # the reported final losses stay meaningful: tests/test_gpu_model_parity.py::test_training_on_a_fixed_batch_...)
    cfg.SOLVER.BASE_LR = 1e-3
    optimizer = build_optimizer(cfg, model)
    wire = ("bf16" if precision in ("bf16", "parity", "parity_mx", "parity_train", "bf16x3f") else "fp32") if args.grad_wire == "auto" else args.grad_wire
    # asynchronous gradient exchange behind the next step's frozen forward.  At N > 1 with --exchange auto both forms are
    # timed below and the faster one carries the headline: the trainer starts on the ring (RCCL's own all-reduce)
    ab = world > 1 and wire == "bf16" and args.exchange == "auto"
    trainer = HotPathTrainer(model, optimizer, grad_wire=wire, reduce_unused=mixed,
                             exchange=("ring" if ab else args.exchange) if wire == "bf16" else "ring")
    trainer.broadcast_parameters()
    cpu_state = None
    if keep and rank == 0 and world == 1 and not args.no_cpu_baseline:  # untrained weights for the CPU leg
        cpu_state = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    host_batch = make_batch(batch_size, proposals, classes, seed=1234 + rank)
    if mixed:
        for x in host_batch:
            x["dataset_id"] = 2
    stager = H2DStager(host_batch, dev) if h2d else None
    resident = None if h2d else to_device_batch(host_batch, dev)

    def step():
        return trainer.run_step(stager.next() if h2d else resident)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    sync()
    exchange_ab = None
    if ab:
        exchange_ab = pick_exchange(trainer, step, sync, dev, steps=max(3, min(6, steps)))
        for _ in range(2):  # settle on the chosen form before the timed region
            step()
        sync()
    events = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    trainer.stats_enable(world > 1 or dist.is_initialized())  # two event records per step: where the exchange went
    t0 = time.perf_counter()
    events[0].record()
    for i in range(steps):
        last = step()
        events[i + 1].record()
    sync()
    elapsed = time.perf_counter() - t0
    comm = trainer.stats()
    trainer.stats_enable(False)
    per_step = [events[i].elapsed_time(events[i + 1]) for i in range(steps)]
    # the last timed step's losses (read before anything else runs: a replayed step graph reuses its output tensors)
    final_losses = {k: float(v.detach()) for k, v in last.items()}
    if not all(v == v and abs(v) != float("inf") for v in final_losses.values()):
        raise RuntimeError(f"training diverged during the benchmark: {final_losses}")
    rec = {"elapsed": elapsed, "per_step_ms": per_step, "final_losses": final_losses, "wire": wire,
           "exchange": trainer.exchange_algo, "exchange_ab": exchange_ab, "comm": comm}
    if dump:
        trainer.flush()  # the deferred update of the last timed step: what a caller reads from the parameters after it
        rec["outputs"] = step_outputs(model, last)

    if want_roofline:
        # second pass over the same K steps with every launch bracketed by hipEvents on its stream
        _lib.profile_reset()
        _lib.profile_enable(True)
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        table = _lib.profile_collect()
        _lib.profile_enable(False)
        rec["kernel_table"] = sorted([e for e in table if e["launches"] > 0], key=lambda e: -e["ms"])
    trainer.flush()
    if keep:
        rec.update(model=model, cpu_state=cpu_state, host_batch=host_batch)
    else:
        del trainer, optimizer, model, resident, stager
        torch.cuda.empty_cache()
    return rec


def measured_parity(args, dev, cfgv, images=1):
    """The deviation of ONE side configuration from the ORACLE, measured in this run (never asserted from the precision's
    name): one training step of the configuration's own model (depth, pooler, proposals, classes, embedding width, mixed
    or not) on `images` full-size images, dropout off, through the HIP path in the configuration's precision, against
    oracle/wsovod_ref.py on the same weights and inputs (1.5 - 6 s of host CPU per line).  The batch size of a line does
    not enter: rows of different images never meet before the per-image softmaxes, which the 32-image check of the
    headline (`parity.at_timed_batch`) and tests/test_gpu_full_size.py cover."""
    from oracle import compare as OC
    from wsovod_amd.data import make_batch
    from wsovod_amd.testing import build_hot_path_model, build_mixed_model, capture_full_step

    depth, proposals = cfgv.get("depth") or args.depth, cfgv.get("proposals") or args.proposals
    classes, embed_dim = cfgv.get("classes") or args.classes, cfgv.get("embed_dim") or args.embed_dim
    precision, pooler, mixed = cfgv["precision"], cfgv["pooler"], bool(cfgv.get("mixed"))
    host = make_batch(images, proposals, classes, seed=2468)
    extra, source_id = {}, 2
    if mixed:
        cfg, model = build_mixed_model(seed=0, names=("voc_2007_train", "coco_2017_train", "lvis_v1_train"),
                                       Ks=(20, 80, classes), D=embed_dim, depth=depth, precision=precision, pooler=pooler,
                                       device=str(dev))
        for x in host:
            x["dataset_id"] = source_id
        model.roi_heads.select_source(source_id)
        prefix = f"roi_heads.object_miners.{source_id}."
        extra = dict(classifier=model.classifier_train[source_id].detach().float().cpu(), miner_prefix=prefix)
        train_keys = [k for k, p in model.named_parameters()
                      if p.requires_grad and (not k.startswith("roi_heads.object_miners.") or k.startswith(prefix))]
    else:
        cfg, model = build_hot_path_model(seed=0, depth=depth, K=classes, D=embed_dim, precision=precision, pooler=pooler,
                                          device=str(dev))
        train_keys = [k for k, p in model.named_parameters() if p.requires_grad]
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    state = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
    got = capture_full_step(model, to_device_batch(host, dev))
    del model
    torch.cuda.empty_cache()
    t0 = time.time()
    want = OC.oracle_step(state, host, train_keys, depth=depth, num_classes=classes, pooler_type=pooler, **extra)
    rep = OC.compare(got, want)
    keys = ("max_abs_logit_err", "max_abs_score_err", "max_abs_delta_err", "max_rel_loss_err", "labels_exact",
            "label_boxes_exact", "pgt_exact", "max_rel_gradnorm_err", "meets_1e-3_logit_bound")
    return dict({k: rep[k] for k in keys}, images=images, oracle_seconds=round(time.time() - t0, 1),
                vs="oracle/wsovod_ref.py on the same weights and inputs, measured in this run")


def side_measurements(args, dev):
    """Short runs in the SAME process as the headline line (N = 1): the reference's own per-GPU batch (1), 8 images,
    the north star's pooler, the two parity-grade precisions, and the variant with the input copy inside the step."""
    out, parity_cache = [], {}
    variants = [
        # (small batches: >= 40 timed steps -- the first replay behind the warm-up's synchronisation runs ~1 ms long (an
        # 80-step run at 8 images: 8.78, then 7.78 - 7.99 ms), which a 10-step line reported as "one slow step in ten")
        ("b1 (the reference's images per GPU)", dict(batch_size=1, steps=max(40, args.side_steps))),
        ("b8", dict(batch_size=8, steps=max(40, args.side_steps))),
        ("48 images/step", dict(batch_size=48)),
        ("plain bf16 (BASELINE config 2's dtype; does NOT meet the 1e-3 logit bound: see parity.modes.bf16)",
         dict(precision="bf16")),
        ("plain bf16, b1", dict(precision="bf16", batch_size=1, steps=max(40, args.side_steps))),
        ("ROIAlignV2 pooler (north-star wording)", dict(pooler="ROIAlignV2")),
        ("parity_train (the parity forward + a backward that keeps the hi/lo split: the mode whose five-step trajectory "
         "stays within 1e-3 of the oracle's, tests/test_gpu_full_size.py)", dict(precision="parity_train",
                                                                                steps=max(5, args.side_steps // 2))),
        ("fp32 (exact-fp32 MFMA)", dict(precision="fp32", steps=max(3, args.side_steps // 3), warmup=2)),
        ("H2D-inclusive (uint8 images + boxes copied from pinned host memory every step)", dict(h2d=True)),
        ("BASELINE config 2 shapes: K = 80 classes, D = 768 (CLIP ViT-L/14)", dict(classes=80, embed_dim=768)),
        ("BASELINE config 3 shapes: WSR_50, 1024 proposals, K = 80, 8 images/step", dict(depth=50, proposals=1024, classes=80,
                                                                                   batch_size=8, steps=max(3, args.side_steps // 2))),
        ("BASELINE config 5 shapes: mixed-dataset model, WSR_50, 1024 proposals, K = 1203 per-call text embeddings, "
         "8 images/step", dict(depth=50, proposals=1024, classes=1203, batch_size=8, mixed=True,
                               steps=max(3, args.side_steps // 2))),
        ("BASELINE config 5 at the reference's own 1 image per GPU (mixed-dataset model, WSR_50, 1024 proposals, K = 1203): "
         "whole-step HIP graph keyed on (source, layout)", dict(depth=50, proposals=1024, classes=1203, batch_size=1,
                                                                mixed=True, steps=max(20, args.side_steps))),
    ]
    if args.precision != "parity":  # (the headline was moved off the default: keep the tolerance-meeting mode in the line)
        variants.insert(0, ("parity: the tolerance-meeting mode", dict(precision="parity")))
    for name, kw in variants:
        cfgv = dict(precision=args.precision, batch_size=args.batch, pooler=args.pooler, steps=args.side_steps,
                    warmup=5, h2d=False)
        cfgv.update(kw)
        if cfgv["batch_size"] <= 8 and "warmup" not in kw:
            # whole-step HIP graphs: captured on the layout's fourth step, and the first few replays run 5 - 10 % slow
            # (measured at 8 images: 8.7 / 8.1 / 8.9 / 9.0 ms, then 7.95 +- 0.03) -- the timed region starts behind them
            cfgv["warmup"] = 12
        try:
            r = run_config(args, dev, 0, 1, **cfgv)
        except Exception as e:  # a side line must never take the headline down
            out.append({"name": name, "error": f"{type(e).__name__}: {e}"[:300]})
            continue
        ms = r["per_step_ms"]
        # parity of the line: MEASURED against the oracle for this configuration (one comparison per distinct model /
        # precision / pooler / shape; lines that differ only in images per step or in where the inputs live share it)
        # (round 6: on the line's OWN images per step up to 8 -- the tile / split-K rules of a small batch are the ones the
        # comparison runs; larger steps share a 2-image comparison, the headline's 32 are compared in `parity.at_timed_batch`)
        b_ = int(cfgv["batch_size"])
        pimg = (b_ if b_ <= 8 else 2) if not cfgv.get("depth") == 50 else min(b_, 2)
        pkey = (cfgv["precision"], cfgv["pooler"], cfgv.get("depth"), cfgv.get("proposals"), cfgv.get("classes"),
                cfgv.get("embed_dim"), bool(cfgv.get("mixed")), pimg)
        if args.no_parity:
            par = {"skipped": "--no-parity"}
        else:
            if pkey not in parity_cache:
                try:
                    parity_cache[pkey] = measured_parity(args, dev, cfgv, images=pimg)
                except Exception as e:  # noqa: BLE001 -- reported in the line, never silently replaced by a claim
                    parity_cache[pkey] = {"error": f"{type(e).__name__}: {e}"[:300]}
            par = parity_cache[pkey]
        out.append({"name": name, "precision": cfgv["precision"], "images_per_step": cfgv["batch_size"],
                    "warmup": cfgv["warmup"],
                    "meets_1e-3_logit_bound": par.get("meets_1e-3_logit_bound"), "parity": par,
                    "pooler": cfgv["pooler"], "steps": cfgv["steps"], "depth": cfgv.get("depth") or args.depth,
                    "proposals": cfgv.get("proposals") or args.proposals,
                    "images_per_sec": cfgv["batch_size"] * cfgv["steps"] / r["elapsed"],
                    "ms_per_step": r["elapsed"] / cfgv["steps"] * 1e3, "median_ms": pct(ms, 0.5), "p10_ms": pct(ms, 0.1),
                    "p90_ms": pct(ms, 0.9)})
    return out


def parity_block(args, dev):
    """What error each precision has AGAINST THE ORACLE at the configuration's own size: ONE training step on the same
    `--parity-images` full-size images (800x600, `--proposals` boxes each), same weights, dropout off, through the HIP
    path in every mode, compared with oracle/wsovod_ref.py (the CPU restatement of the reference, pinned to the
    reference's golden vectors by tests/test_oracle_golden.py) run on the same inputs -- the oracle is the checker
    here, never the thing measured.  `vs_fp32_hip` keeps the HIP-vs-HIP cross-check of earlier rounds as a second field."""
    from oracle import compare as OC
    from wsovod_amd.data import make_batch
    from wsovod_amd.testing import build_hot_path_model, capture_full_step

    batch = make_batch(args.parity_images, args.proposals, args.classes, seed=4321)
    modes = ["fp32", "bf16", "bf16x3", "parity"]
    if args.precision not in modes:
        modes.append(args.precision)
    res, state, train_keys = {}, None, None
    for prec in modes:
        cfg, model = build_hot_path_model(seed=0, depth=args.depth, K=args.classes, D=args.embed_dim, precision=prec,
                                          pooler=args.pooler, device=str(dev))
        if state is None:
            state = {k: v.detach().clone() for k, v in model.state_dict().items()}
            train_keys = [k for k, p in model.named_parameters() if p.requires_grad]
        else:
            model.load_state_dict(state)
        model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.eval()
        res[prec] = capture_full_step(model, to_device_batch(batch, dev))
        del model
        torch.cuda.empty_cache()
    t0 = time.time()
    want = OC.oracle_step({k: v.float().cpu() for k, v in state.items()}, batch, train_keys, depth=args.depth,
                          num_classes=args.classes, pooler_type=args.pooler)
    oracle_s = time.time() - t0
    out = {"vs": "oracle/wsovod_ref.py (CPU fp32 restatement of the reference path, pinned to the reference's golden "
                 "vectors) on the same images and weights",
           "workload": f"{args.parity_images} x 800x600 images x {args.proposals} proposals, one training step, dropout off, "
                       f"identical weights", "oracle_seconds": round(oracle_s, 2), "north_star_bound": 1e-3, "modes": {}}
    keys = ("max_abs_logit_err", "max_abs_score_err", "max_abs_delta_err", "max_rel_loss_err", "labels_exact",
            "label_boxes_exact", "pgt_exact", "max_rel_gradnorm_err", "meets_1e-3_logit_bound")
    for prec in modes:
        rep = OC.compare(res[prec], want)
        out["modes"][prec] = {k: rep[k] for k in keys}
    ref = res["fp32"]
    out["vs_fp32_hip"] = {prec: {"max_abs_logit_err": float((res[prec]["refine_logits"] - ref["refine_logits"]).abs().max()),
                                 "max_abs_score_err": float((res[prec]["mining_scores"] - ref["mining_scores"]).abs().max())}
                          for prec in modes if prec != "fp32"}
    out["mode"] = args.precision
    out["max_abs_logit_err"] = out["modes"][args.precision]["max_abs_logit_err"]
    out["max_abs_score_err"] = out["modes"][args.precision]["max_abs_score_err"]
    if not args.no_parity_at_batch and args.batch > args.parity_images:
        # the HEADLINE precision at the timed batch itself (M = batch x proposals rows through fc1, the dW reductions at
        # that length): one more oracle step on the timed batch's own images
        del res, want
        big = make_batch(args.batch, args.proposals, args.classes, seed=1234)
        cfg, model = build_hot_path_model(seed=0, depth=args.depth, K=args.classes, D=args.embed_dim,
                                          precision=args.precision, pooler=args.pooler, device=str(dev))
        model.load_state_dict(state)
        model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.eval()
        got = capture_full_step(model, to_device_batch(big, dev), keep_grads_below=2_000_000)
        del model
        torch.cuda.empty_cache()
        t0 = time.time()
        want = OC.oracle_step({k: v.float().cpu() for k, v in state.items()}, big, train_keys, depth=args.depth,
                              num_classes=args.classes, pooler_type=args.pooler)
        rep = OC.compare(got, want)
        out["at_timed_batch"] = dict({k: rep[k] for k in keys + ("max_rel_grad_elem_err", "max_abs_img_score_err")},
                                     images=args.batch, precision=args.precision, oracle_seconds=round(time.time() - t0, 1))
    return out


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            return launch_ranks(args)
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}: the launcher and "
                         f"the flag must agree (the reported n_gpus is the size of the process group)")
    # stdout carries exactly ONE line, the JSON result: libraries that print to fd 1 (RCCL's version banner at
    # communicator creation does) are sent to stderr for the duration of the run.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and "OMP_NUM_THREADS" not in os.environ:  # (an external launcher: N ranks share the host's cores)
        torch.set_num_threads(max(1, (os.cpu_count() or 1) // world))
    if args.launch_check:
        return launch_check(args, world, rank, result_fd)
    if not torch.cuda.is_available():
        raise RuntimeError("bench.py needs an MI355X (no CPU fallback on the product path)")
    if args.share_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} ranks")
    if world > 1 or args.one_rank_group:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)
        if dist.get_world_size() != world:
            raise RuntimeError(f"process group has {dist.get_world_size()} ranks, expected {world}")

    if args.rpn:
        args.no_cpu_baseline = True
    if args.eval:
        from wsovod_amd.testing import build_hot_path_model

        cfg, model = build_hot_path_model(seed=0, depth=args.depth, K=args.classes, D=args.embed_dim,
                                          precision=args.precision, pooler=args.pooler, device=f"cuda:{local_rank}",
                                          rpn=args.rpn)
        return eval_bench(args, cfg, model, dev, result_fd)

    rec = run_config(args, dev, rank, world, precision=args.precision, batch_size=args.batch, pooler=args.pooler,
                     steps=args.steps, warmup=args.warmup, h2d=args.h2d, rpn=args.rpn,
                     want_roofline=not args.no_roofline, keep=True, dump=bool(args.dump_outputs) and rank == 0)
    if "outputs" in rec:
        write_outputs(args.dump_outputs, rec.pop("outputs"))
    elapsed, my_ms = rec["elapsed"], rec["elapsed"] / args.steps * 1e3
    rank_ms = [my_ms]
    comm_ranks = None
    if world > 1:
        c = rec.get("comm") or {}
        t = torch.tensor([elapsed, c.get("exchange_wait_ms", 0.0), c.get("overlap_window_ms", 0.0)], device=dev,
                         dtype=torch.float64)
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        rank_ms = [float(x[0].item()) / args.steps * 1e3 for x in allt]
        elapsed = max(float(x[0].item()) for x in allt)  # the job is as slow as its slowest rank
        # the line explains itself: per rank, how long the compute stream stood still for the exchange of the previous
        # step (EXPOSED communication) next to the frozen forward it is scheduled behind
        comm_ranks = {"exchange_wait_ms": [round(float(x[1].item()), 4) for x in allt],
                      "overlap_window_ms": [round(float(x[2].item()), 4) for x in allt],
                      "wire_bytes_per_step": c.get("wire_bytes_per_step"),
                      "bytes_sent_per_rank_per_step": c.get("bytes_sent_per_rank_per_step"),
                      "exchange": c.get("exchange"), "wire": c.get("wire"),
                      "note": "exchange_wait_ms = hipEvent time on the compute stream across the waits for the previous "
                              "step's collectives (0 = fully hidden behind the frozen forward of overlap_window_ms)"}
    elif rec.get("comm"):
        c = rec["comm"]
        comm_ranks = {"exchange_wait_ms": [round(c["exchange_wait_ms"], 4)], "overlap_window_ms": [round(c["overlap_window_ms"], 4)],
                      "wire_bytes_per_step": c["wire_bytes_per_step"], "exchange": c["exchange"], "wire": c["wire"]}
    device_identity_warning = None
    if world > 1 and args.backend == "nccl" and not args.share_device:
        # one process per GPU means one GPU per process: a launcher that put two ranks on one device fails the run
        # (identity = the device's UUID / PCI address, not its index: a launcher may show every rank one device as index 0)
        props = torch.cuda.get_device_properties(dev)
        ident = [getattr(props, a, None) for a in ("uuid", "pci_domain_id", "pci_bus_id", "pci_device_id")]
        if any(v is not None for v in ident):
            import zlib

            me = torch.tensor([zlib.crc32(str(ident[0]).encode()) & 0x7FFFFFFF] + [int(v) if isinstance(v, int) else -1
                                                                                   for v in ident[1:]]
                              + [torch.cuda.current_device(), torch.cuda.device_count()], device=dev, dtype=torch.int64)
            ids = [torch.zeros_like(me) for _ in range(world)]
            dist.all_gather(ids, me)
            seen = [tuple(int(v) for v in x.tolist()) for x in ids]
            if len(set(t[:4] for t in seen)) != world:
                # the same identity twice: fatal when the ranks also name the same device index (or see one device only);
                # with DIFFERENT indices of a multi-device process the identity fields are not trustworthy on this host
                # (virtualised PCI addresses / no UUID): reported in the line, not fatal
                if len(set(t[4] for t in seen)) != world or any(t[5] < world for t in seen):
                    raise RuntimeError(f"bench.py --gpus {world}: the ranks sit on devices {seen}, not on {world} different GPUs")
                device_identity_warning = f"device identities (uuid crc, pci domain / bus / device) repeat across ranks: {seen}"

    roofline = None
    table = rec.get("kernel_table")
    if rank == 0 and table:
        # A kernel on bf16x2 operands issues three MFMA products per value pair; the profiler's table counts those
        # EXECUTED flops.  The roofline is quoted on ALGORITHMIC work (2 M N K per contraction) -- `frac` --
        # and the executed rate travels next to it as `executed_*`.
        def algo(e):
            return e["flops"] / 3.0 if "bf16x2" in e["name"] else e["flops"]

        top = table[0]
        mfma = top["flops"] > 0 and ("gemm" in top["name"] or "conv" in top["name"])
        avg_ms = top["ms"] / top["launches"]
        peak = PEAK[args.precision] if mfma else HBM_PEAK_GBS
        work = algo(top) if mfma else top["bytes"]
        ach = (work / top["launches"] / (avg_ms * 1e-3)) / (1e12 if mfma else 1e9)
        traffic, source = pmc_traffic(top["name"], args)
        step_ms = rec["elapsed"] / args.steps * 1e3
        roofline = {"bound": "mfma" if mfma else "hbm", "achieved": ach, "peak": peak,
                    "unit": "TFLOP/s" if mfma else "GB/s", "frac": ach / peak, "traffic": traffic,
                    "traffic_source": source,
                    "algorithmic_per_launch": work / top["launches"],
                    "kernel": top["name"], "launches_per_step": top["launches"] / args.steps, "avg_launch_ms": avg_ms,
                    "share_of_kernel_time": top["ms"] / sum(e["ms"] for e in table),
                    "kernels": [{"name": e["name"], "ms_per_step": e["ms"] / args.steps,
                                 "launches_per_step": e["launches"] / args.steps,
                                 "tflops": (algo(e) / (e["ms"] * 1e-3) / 1e12) if e["flops"] and e["ms"] else None,
                                 "executed_tflops": (e["flops"] / (e["ms"] * 1e-3) / 1e12) if e["flops"] and e["ms"] else None,
                                 "gbs": (e["bytes"] / (e["ms"] * 1e-3) / 1e9) if e["bytes"] and e["ms"] else None}
                                for e in table[:16]]}
        if mfma:
            # (f16mx operands: per 32x32x32 block two fp16 MFMAs + one block-scaled fp8 MFMA of the same pipe time = the cycles
            # of FOUR bf16-rate MFMA units of 32x32x16, i.e. twice the cycles of a plain 16-bit contraction)
            exf = 2.0 if "f16mx" in top["name"] else 1.0
            ex = exf * top["flops"] / top["launches"] / (avg_ms * 1e-3) / 1e12
            roofline["executed_achieved"], roofline["executed_frac"] = ex, ex / peak
            roofline["executed_note"] = ("bf16x2 operands: three bf16 MFMA products per value pair (hi*hi + hi*lo + lo*hi), the "
                                         "price of the 1e-3 logit bound on a 16-bit matrix pipe; `frac` counts the "
                                         "algorithmic 2*M*N*K only") if "bf16x2" in top["name"] else (
                "f16mx operands: hi*hi as two fp16 MFMAs + both cross terms as ONE block-scaled e4m3 MFMA per 32x32x32 block "
                "= the matrix-pipe cycles of two 16-bit products per value pair (three with bf16x2); `executed` prices those "
                "cycles at the 16-bit rate, `frac` counts the algorithmic 2*M*N*K only") if "f16mx" in top["name"] else None
        # end to end: SURVEY 8d's algorithmic FLOP per image x images per step / step time, against the same MFMA peak
        gf_img = {(18, 512): 469.2, (50, 1024): 2199.4}.get((args.depth, args.proposals))
        if gf_img is not None and not args.rpn:
            e2e = gf_img * args.batch / step_ms  # GFLOP / ms = TFLOP/s
            roofline["end_to_end"] = {"algorithmic_gflop_per_image": gf_img, "achieved": e2e, "unit": "TFLOP/s",
                                      "frac": e2e / PEAK[args.precision]}

    if rank == 0:
        images = world * args.batch * args.steps
        ms = rec["per_step_ms"]
        rccl = None
        if dist.is_initialized() and args.backend == "nccl":
            try:
                rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                rccl = None
        out = {
            "metric": "images/sec (512 proposals/img) WSR_18_DC5 fwd+bwd at 1/2/4/8 MI355X",
            "value": images / elapsed, "unit": "images/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "median_ms": pct(ms, 0.5),
            "p10_ms": pct(ms, 0.1), "p90_ms": pct(ms, 0.9), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": DTYPE[args.precision], "precision": args.precision,
            "data": "synthetic",
            "config": {"workload": f"VOC07 WSOVOD_WSR_{args.depth}_DC5_1x, {args.proposals} proposals/img, "
                                   f"{args.classes}-class embeddings (D={args.embed_dim}), 800x600 images, "
                                   f"{'RPN + loaded proposals' if args.rpn else 'proposals-only mode'}, {args.pooler}, "
                                   f"full training step (fwd+bwd+SGD)",
                       "images_per_gpu_per_step": args.batch, "global_batch": world * args.batch,
                       "parallelism": f"dp{world}",
                       "grad_allreduce": (f"{rec['wire']} over {'RCCL ' + str(rccl) if rccl else args.backend}, "
                                          + ("all-to-all + fp32 shard sum (one rounding) + all-gather"
                                             if rec["exchange"] == "direct" else "all-reduce"))
                       if dist.is_initialized() else "none (1 GPU)",
                       "inputs": "uint8 images + boxes copied from pinned host memory inside every step (async, double "
                                 "buffered)" if args.h2d else "resident in HBM before the timed region, handed over in the "
                                 "reference's list-of-dicts format as per-image views of ONE collated uint8 batch tensor (the "
                                 "model takes adjacent views as they are: no per-step gather pass; `side` has the H2D form)",
                       "per_step_percentiles": "hipEvent time between consecutive steps on rank 0's stream",
                       "rank_ms_per_step": {"max": max(rank_ms), "min": min(rank_ms), "all": rank_ms},
                       "process_group_ranks": dist.get_world_size() if dist.is_initialized() else 1,
                       "process_group": {"backend": dist.get_backend(), "ranks": dist.get_world_size(), "rccl": rccl,
                                         "ranks_equal_gpus_flag": dist.get_world_size() == args.gpus,
                                         "device_identity_warning": device_identity_warning}
                       if dist.is_initialized() else None,
                       "exchange_ab": rec.get("exchange_ab"),
                       "communication": comm_ranks,
                       "final_losses": rec["final_losses"]},
        }
        if args.full:  # (a plain line stays short whatever --steps is: the percentiles above summarise the list)
            out["config"]["per_step_ms"] = [round(v, 3) for v in ms]
        if roofline is not None:
            out["roofline"] = roofline
        model, cpu_state, host_batch = rec.pop("model"), rec.pop("cpu_state"), rec.pop("host_batch")
        del rec
        torch.cuda.empty_cache()
        if world == 1 and not args.rpn:
            if not args.no_parity:
                out["parity"] = parity_block(args, dev)
                # what the headline precision is worth against the oracle, in the line itself: at the timed batch when it
                # was compared there, else on the small comparison
                pm = out["parity"].get("at_timed_batch") or out["parity"]["modes"].get(args.precision, {})
                for k in ("max_abs_logit_err", "max_abs_score_err", "labels_exact", "pgt_exact", "meets_1e-3_logit_bound",
                          "max_rel_gradnorm_err", "max_rel_grad_elem_err"):
                    if k in pm:
                        out[k] = pm[k]
                out["parity_checked_on_images"] = pm.get("images", args.parity_images)
                out["gradient_grade"] = ("forward quantities of fp32 grade (the bound above); the backward pass runs in plain "
                                         "bf16 on the hi halves: gradient norms / elements carry bf16's grade (fields above)"
                                         if args.precision in ("parity", "parity_mx", "bf16x3f") else None)
            if not args.no_side:
                out["side"] = side_measurements(args, dev)
                # the reference's own operating points (1 and 8 images per GPU) as top-level keys
                for key, name in (("b1_images_per_sec", "b1 (the reference's images per GPU)"), ("b8_images_per_sec", "b8")):
                    line = next((x for x in out["side"] if x.get("name") == name and "images_per_sec" in x), None)
                    if line is not None:
                        out[key] = line["images_per_sec"]
                        out[key.replace("images_per_sec", "ms_per_step")] = line["ms_per_step"]
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(model, cpu_state, host_batch, args)
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
