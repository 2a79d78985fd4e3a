#!/usr/bin/env python3
"""The cell search's training step on the MI355X (automl/mdenas_search.py of both trees; run_rag.sh / run_rag_depth.sh: c_batch 8
stereo, 16 depth): ms / step issued eagerly (rag_amd.train.train_step) and as a captured graph (GraphedTrainStep, one capture per
epoch since the ops are fixed within an epoch), with the capture's node census, every number measured with HIP events in this
process.

Cases: the stereo supernet at B=8, 192x384, D=192 and the depth supernet at B=16, 384x768; each for draw A
(fea_ops=[1,0,1,1,0,1,0,1,1], mat_ops=[0,1,1,0,1,1,1,0,1]) and for all-conv ops.  Freshly initialised (seeded) supernets in train
mode, FlatSGD with the run scripts' hyper-parameters, clip_grad_norm_(5).

One case per process (`--case`), so that a driver can give every case its own time limit; each run merges its result into
profiles/search_step_bench.json (`--out`).  There is no baseline to compare with: before `sampled_ops` no supernet could take a
step through rag_amd.train at all.

Usage:  python tools/bench_search_step.py --case depth_A [--iters N] [--out PATH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rag_amd  # noqa: E402
from rag_amd.train import FlatSGD, GradBucket, GraphedTrainStep, train_step  # noqa: E402

DEV = "cuda:0"
DRAWS = {"A": ([1, 0, 1, 1, 0, 1, 0, 1, 1], [0, 1, 1, 0, 1, 1, 1, 0, 1]), "conv": ([1] * 9, [1] * 9)}
CASES = {f"{net}_{draw}": (net, draw) for net in ("stereo", "depth") for draw in DRAWS}


def timed_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def build(kind):
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(6)
    if kind == "stereo":
        B, H, W = 8, 192, 384
        net = rag_amd.BasicNetwork(device=DEV, maxdisp=192)
        right = torch.randn((B, 3, H, W), generator=g).to(DEV)
        gt = (torch.rand((B, H, W), generator=g) * 200).to(DEV)
        hyper = dict(lr=1e-3, momentum=0.9, weight_decay=3e-3)
    else:
        B, H, W = 16, 384, 768
        net = rag_amd.DepthBasicNetwork(device=DEV)
        right = None
        gt = torch.rand((B, H, W), generator=g) * 79 + 1
        gt[torch.rand((B, H, W), generator=g) < 0.5] = 0
        gt = gt.to(DEV)
        hyper = dict(lr=0.002, momentum=0.9, weight_decay=3e-4)
    left = torch.randn((B, 3, H, W), generator=g).to(DEV)
    net = net.to(DEV).train()
    bucket = GradBucket(net.parameters())
    return net, bucket, FlatSGD(bucket, **hyper), left, right, gt, (B, H, W)


def run(case, iters):
    kind, draw_name = CASES[case]
    draw = DRAWS[draw_name]
    net, bucket, opt, left, right, gt, (B, H, W) = build(kind)
    for _ in range(2):
        train_step(net, opt, bucket, left, right, gt, sampled_ops=draw)
    torch.cuda.synchronize()
    eager = timed_ms(lambda: train_step(net, opt, bucket, left, right, gt, sampled_ops=draw), iters)
    st = GraphedTrainStep(net, opt, bucket, left, right, gt, sampled_ops=draw, warmup=1)
    st()
    torch.cuda.synchronize()
    graphed = timed_ms(st, iters)
    loss = float(st.loss)
    return {"B": B, "image": [H, W], "maxdisp": net.maxdisp if kind == "stereo" else None, "draw": draw_name,
            "active_tensors": len(net.active_parameters(*draw)), "tensors": len(bucket.params), "values": int(bucket.flat.numel()),
            "eager_ms_per_step": round(eager, 3), "graphed_ms_per_step": round(graphed, 3),
            "graphed_samples_per_s": round(B * 1e3 / graphed, 1), "loss_after_steps": round(loss, 4),
            "graph_kernel_nodes": st.node_census["kernel"], "graph_memcpy_nodes": st.node_census["memcpy"],
            "graph_memset_nodes": st.node_census["memset"], "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_step_bench.json"))
    args = ap.parse_args()
    res = run(args.case, args.iters)
    data = {"metric": "search_step"}
    if os.path.exists(args.out):
        with open(args.out) as f:
            data = json.load(f)
    data[args.case] = res
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({args.case: res}))


if __name__ == "__main__":
    main()
