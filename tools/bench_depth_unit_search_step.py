#!/usr/bin/env python3
"""The depth tree's unit-search training step on the MI355X (Appr.search_epoch of rag_depth/src/approaches/rag.py:371-438, run for
every task t > 0 with run_rag_depth.sh's o_batch 12): ms / step issued eagerly (rag_amd.depth_search_step) and as a captured graph
(DepthGraphedSearchStep, one capture per epoch since the path is fixed within an epoch), with the capture's node census, every number
measured with HIP events in this process.

Model: the shipped task-3 weights (tests/golden/g14) expanded for task 4 with a seeded, freshly initialised candidate of the g25
fixture's genotype, after freeze_model + modify_param(new_models) and net.search_mode(); B=12, 384x768; FlatSGD(lr 1e-3, momentum 0.9,
weight decay 3e-4), clip_grad_norm_(5), a DepthEpochMeter fed by every step.  Paths: `new` (every candidate unit), `reused` (the last
trained unit of every layer: only task 4's heads train and the trunk runs without an autograd graph) and `A` (the mixed path of the
g25 fixture).

`--path loss` instead times the loss alone at B=8, 384x768: `silog_metrics_loss` forward (two launches: loss, metrics, saved scalars,
meter) against `silog_loss` + `depth_metrics` (four launches) on the same tensors.

One case per process (`--path`), so that a driver can give every case its own time limit; each run merges its result into
profiles/depth_unit_search_step_bench.json (`--out`).  There is no baseline to compare the step with: before rag_amd.depth_search the
expanded depth network could not take this step at all.

Usage:  python tools/bench_depth_unit_search_step.py --path A [--iters N] [--out PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rag_amd  # noqa: E402
from rag_amd.depth import DepthEpochMeter, _geno, depth_metrics, load_depth_checkpoint, silog_loss, silog_metrics_loss  # noqa: E402
from rag_amd.train import FlatSGD, GradBucket  # noqa: E402

DEV = "cuda:0"
T = 4
GOLDEN = os.path.join(ROOT, "tests", "golden")


def timed_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def build():
    with np.load(os.path.join(GOLDEN, "g14_depth_ckpt_task3.npz")) as z:
        sd = {k: torch.from_numpy(z[k]) for k in z.files}
    with np.load(os.path.join(GOLDEN, "g25_depth_unit_search.npz")) as z:
        mixed, sel_a = z["mixed"], [int(v) for v in z["sel_A"]]
    net = load_depth_checkpoint({"model": sd}, "cpu", "from_keys")[0]
    torch.manual_seed(5)
    net.expand(T, _geno(mixed), "cpu")
    net = net.to(DEV)
    for p in net.parameters():                     # utils.freeze_model + modify_param(new_models, True)
        p.requires_grad = False
    net.modify_param(net.new_models, True)
    net.search_mode()
    counts = [len(net._units(n)) for n in net._p_layers()]
    paths = {"new": [c - 1 for c in counts], "reused": [c - 2 for c in counts], "A": sel_a}
    g = torch.Generator().manual_seed(6)
    B, H, W = 12, 384, 768
    left = (torch.rand((B, 3, H, W), generator=g) * 2 - 1).to(DEV)
    gt = torch.rand((B, H, W), generator=g) * 70 + 2
    gt[torch.rand((B, H, W), generator=g) < 0.3] = 0
    bucket = GradBucket(net.parameters())
    return net, bucket, FlatSGD(bucket, lr=1e-3, momentum=0.9, weight_decay=3e-4), left, gt.to(DEV), (B, H, W), paths


def run(path, iters):
    net, bucket, opt, left, gt, (B, H, W), paths = build()
    sel = paths[path]
    meter = DepthEpochMeter(DEV)
    for _ in range(2):
        rag_amd.depth_search_step(net, opt, bucket, left, gt, T, sel, meter=meter)
    torch.cuda.synchronize()
    eager = timed_ms(lambda: rag_amd.depth_search_step(net, opt, bucket, left, gt, T, sel, meter=meter), iters)
    st = rag_amd.DepthGraphedSearchStep(net, opt, bucket, left, gt, T, sel, meter=meter, warmup=1)
    st()
    torch.cuda.synchronize()
    graphed = timed_ms(st, iters)
    batches = 2 + iters + 2 + iters
    mean = meter.mean()
    assert float(meter.sums[10]) == batches, (float(meter.sums[10]), batches)
    return {"B": B, "image": [H, W], "path": path, "t": T, "selected_ops": sel,
            "active_tensors": len(net.active_parameters(T, sel)), "tensors": len(bucket.params), "values": int(bucket.flat.numel()),
            "eager_ms_per_step": round(eager, 3), "graphed_ms_per_step": round(graphed, 3),
            "graphed_samples_per_s": round(B * 1e3 / graphed, 1), "loss_after_steps": round(float(st.loss), 4),
            "meter_batches": batches, "meter_mean_loss": round(mean["silog_loss"], 4), "meter_mean_abs_rel": round(mean["abs_rel"], 4),
            "graph_kernel_nodes": st.node_census["kernel"], "graph_memcpy_nodes": st.node_census["memcpy"],
            "graph_memset_nodes": st.node_census["memset"], "iters": iters}


def run_loss(iters):
    g = torch.Generator().manual_seed(6)
    B, H, W = 8, 384, 768
    est = (torch.rand((B, H, W), generator=g) * 70 + 1).to(DEV)
    gt = est.cpu() * torch.exp(torch.randn((B, H, W), generator=g) * 0.2)
    gt[torch.rand((B, H, W), generator=g) < 0.3] = 0
    gt = gt.to(DEV)
    meter = DepthEpochMeter(DEV)
    est.requires_grad_(True)                       # the training forward: both losses save their backward's scalars

    def fused():
        silog_metrics_loss(est, gt, meter)

    def split():
        silog_loss(est, gt)
        depth_metrics(est, gt)

    for fn in (fused, split):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    reps = max(iters, 50)
    a, b = timed_ms(fused, reps), timed_ms(split, reps)
    a2, b2 = timed_ms(fused, reps), timed_ms(split, reps)
    return {"B": B, "image": [H, W], "iters": reps, "silog_metrics_loss_fwd_us": [round(a * 1e3, 1), round(a2 * 1e3, 1)],
            "silog_loss_plus_depth_metrics_us": [round(b * 1e3, 1), round(b2 * 1e3, 1)],
            "note": "eager issue, HIP events around `iters` calls, two rounds each; includes the host's launch cost"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=("A", "loss", "new", "reused"), required=True)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_unit_search_step_bench.json"))
    args = ap.parse_args()
    res = run_loss(args.iters) if args.path == "loss" else run(args.path, args.iters)
    data = {"metric": "depth_unit_search_step"}
    if os.path.exists(args.out):
        with open(args.out) as f:
            data = json.load(f)
    data[args.path] = res
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({args.path: res}))


if __name__ == "__main__":
    main()
