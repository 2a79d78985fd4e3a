#!/usr/bin/env python3
"""The unit search's training step on the MI355X (Appr.search_epoch of approaches/rag.py:344-406, run for every task t > 0 with
run.py's o_batch 6): ms / step issued eagerly (rag_amd.train.train_step(selected_ops=, t=, meter=)) and as a captured graph
(GraphedTrainStep, one capture per epoch since the path is fixed within an epoch), with the capture's node census, every number
measured with HIP events in this process.

Model: the grown all-conv Network expanded for task 1 with an all-conv candidate (seeded, freshly initialised), after
freeze_model + modify_param(new_models) and net.search_mode(); B=6, 192x384, D=192; FlatSGD(lr 1e-3, momentum 0.9, weight decay
3e-4), clip_grad_norm_(5), an EpochMeter fed by every step.  Paths: `new` (every candidate unit), `reused` (every unit of task 0:
only task 1's head trains and the trunk runs on the inference executor) and `A` (the mixed path of the g10 / g24 fixtures).

One path per process (`--path`), so that a driver can give every case its own time limit; each run merges its result into
profiles/unit_search_step_bench.json (`--out`).  There is no baseline to compare with: before `selected_ops` the expanded network
could not take this step through rag_amd.train at all.

Usage:  python tools/bench_unit_search_step.py --path A [--iters N] [--out PATH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rag_amd  # noqa: E402
from rag_amd.metrics import EpochMeter  # noqa: E402
from rag_amd.train import FlatSGD, GradBucket, GraphedTrainStep, train_step  # noqa: E402

DEV = "cuda:0"
T = 1
PATHS = {"new": [1] * 18, "reused": [0] * 18, "A": [0, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1]}


def timed_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def build():
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(6)
    B, H, W = 6, 192, 384
    net = rag_amd.Network(rag_amd.ALL_CONV_GENOTYPE, DEV, maxdisp=192)
    net.expand(T, rag_amd.ALL_CONV_GENOTYPE, "cpu")
    net = net.to(DEV)
    for p in net.parameters():                     # utils.freeze_model + modify_param(new_models, True), rag.py:89-90
        p.requires_grad = False
    net.modify_param(net.new_models, True)
    net.search_mode()
    left = torch.randn((B, 3, H, W), generator=g).to(DEV)
    right = torch.randn((B, 3, H, W), generator=g).to(DEV)
    gt = (torch.rand((B, H, W), generator=g) * 200).to(DEV)
    bucket = GradBucket(net.parameters())
    return net, bucket, FlatSGD(bucket, lr=1e-3, momentum=0.9, weight_decay=3e-4), left, right, gt, (B, H, W)


def run(path, iters):
    sel = PATHS[path]
    net, bucket, opt, left, right, gt, (B, H, W) = build()
    meter = EpochMeter(DEV)
    kw = dict(selected_ops=sel, t=T, meter=meter)
    for _ in range(2):
        train_step(net, opt, bucket, left, right, gt, **kw)
    torch.cuda.synchronize()
    eager = timed_ms(lambda: train_step(net, opt, bucket, left, right, gt, **kw), iters)
    st = GraphedTrainStep(net, opt, bucket, left, right, gt, warmup=1, **kw)
    st()
    torch.cuda.synchronize()
    graphed = timed_ms(st, iters)
    batches = 2 + iters + 2 + iters
    mean = meter.mean()
    assert float(meter.sums[6]) == batches, (float(meter.sums[6]), batches)
    return {"B": B, "image": [H, W], "maxdisp": net.maxdisp, "path": path, "t": T,
            "active_tensors": len(net.active_parameters(T, sel)), "tensors": len(bucket.params), "values": int(bucket.flat.numel()),
            "eager_ms_per_step": round(eager, 3), "graphed_ms_per_step": round(graphed, 3),
            "graphed_samples_per_s": round(B * 1e3 / graphed, 1), "loss_after_steps": round(float(st.loss), 4),
            "meter_batches": batches, "meter_mean_loss": round(mean["loss"], 4),
            "graph_kernel_nodes": st.node_census["kernel"], "graph_memcpy_nodes": st.node_census["memcpy"],
            "graph_memset_nodes": st.node_census["memset"], "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=sorted(PATHS), required=True)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unit_search_step_bench.json"))
    args = ap.parse_args()
    res = run(args.path, args.iters)
    data = {"metric": "unit_search_step"}
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
