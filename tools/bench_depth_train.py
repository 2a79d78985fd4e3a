#!/usr/bin/env python3
"""Monocular-depth training on the MI355X: one JSON line, every number measured in this one process.

  * the depth training step at upstream's configuration (run_rag_depth.sh: B=8, 384x768 crops; g14's trained task-3 weights, the
    last unit of every layer trained, silog -> backward -> clip_grad_norm_(5) -> SGD(1e-3, 0.9, 3e-3)): forward + loss + backward
    replayed as ONE hipGraph (rag_amd.train.GraphedTrainStep) plus the eager FlatSGD step, timed with HIP events -> ms / step and
    image pairs / s, with the capture's node census;
  * the fused head + silog forward and backward (DepthHeadFn + SilogLossFn) against the same sequence in ATen autograd
    (depth_head_torch + the reference's silog expression), alternated in one loop, HIP events;
  * the head backward's algorithmic bytes: d_out + y + dy (the weights are noise).

Per-kernel times come from a separate rocprofv3 --kernel-trace --stats run of `--head-only`.

Usage:  python tools/bench_depth_train.py [--iters N] [--head-only]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rag_amd.depth import DepthHeadFn, SilogLossFn, depth_head_torch, load_depth_checkpoint, silog_loss_torch  # noqa: E402
from rag_amd.train import GradBucket, GraphedTrainStep, make_optimizer  # noqa: E402

DEV = "cuda:0"
B, H_IMG, W_IMG = 8, 384, 768


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3        # us per call


def step(iters):
    path = os.path.join(ROOT, "tests", "golden", "g14_depth_ckpt_task3.npz")
    with np.load(path) as z:
        sd = {k: torch.as_tensor(z[k]) for k in z.files}
    net, _ = load_depth_checkpoint({"model": sd}, DEV, "from_keys")
    layers = net._p_layers() + ["last_3_3d", "last_6_3d", "last_12_3d"]
    archi = {name: [len(net._units(name)) - 1] for name in layers}
    net.train()
    for name in layers:                                  # reused units in eval() and frozen (approaches/rag.py:185-228)
        for i, unit in enumerate(net._units(name)):
            if i != archi[name][0]:
                unit.eval()
    for p in net.parameters():
        p.requires_grad_(False)
    net.modify_param(archi, True)
    g = torch.Generator().manual_seed(3)
    left = (torch.rand((B, 3, H_IMG, W_IMG), generator=g) * 2 - 1).to(DEV)
    gt = torch.rand((B, H_IMG, W_IMG), generator=g) * 70 + 1
    gt[torch.rand((B, H_IMG, W_IMG), generator=g) < 0.5] = 0
    gt = gt.to(DEV)
    bucket = GradBucket(net.parameters())
    opt = make_optimizer(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=3e-3, bucket=bucket)
    st = GraphedTrainStep(net, opt, bucket, left, None, gt, task_arch=archi, warmup=2)
    for _ in range(3):
        st()
    torch.cuda.synchronize()
    loss = float(st.loss)
    us = timed(st, iters)
    return {"B": B, "image": [H_IMG, W_IMG], "ms_per_step": round(us / 1e3, 3), "pairs_per_s": round(B * 1e6 / us, 1),
            "loss_after_warmup": round(loss, 4), "trained_values": int(bucket.flat.numel()), "graph_kernel_nodes": st.node_census["kernel"],
            "graph_memcpy_nodes": st.node_census["memcpy"], "graph_memset_nodes": st.node_census["memset"]}


def head_loss(iters):
    h, w = H_IMG // 3, W_IMG // 3
    g = torch.Generator().manual_seed(7)
    y = torch.randn((B, 12, h // 2, w // 2), generator=g).to(DEV)
    w3 = (torch.randn((1, 12, 3, 3), generator=g) * 0.1).to(DEV)
    w1 = (torch.randn((1, 1, 3, 3), generator=g) * 0.3).to(DEV)
    b1 = torch.randn((1,), generator=g).to(DEV)
    gt = torch.rand((B, H_IMG, W_IMG), generator=g) * 70 + 1
    gt[torch.rand((B, H_IMG, W_IMG), generator=g) < 0.5] = 0
    gt = gt.to(DEV)
    ins = [t.clone().requires_grad_(True) for t in (y, w3, w1, b1)]

    def fused():
        for t in ins:
            t.grad = None
        loss = SilogLossFn.apply(DepthHeadFn.apply(*ins, (h, w), 3, 80.0), gt, 0.85)
        loss.backward()
        return loss

    def aten():
        for t in ins:
            t.grad = None
        loss = silog_loss_torch(depth_head_torch(*ins, (h, w), 3, 80.0), gt)
        loss.backward()
        return loss

    lf = fused()
    gf = [t.grad.clone() for t in ins]
    la = aten()
    diff = max(float((a - t.grad).abs().max() / t.grad.abs().max().clamp_min(1e-30)) for a, t in zip(gf, ins))
    loss_diff = abs(float(lf.detach()) - float(la.detach())) / abs(float(la.detach()))
    for _ in range(5):
        fused(), aten()
    tf, ta = [], []
    for _ in range(5):                                   # alternated: both see the same clocks
        tf.append(timed(fused, iters))
        ta.append(timed(aten, iters))
    nbytes = 4 * B * (9 * h * w + 2 * 12 * (h // 2) * (w // 2))
    return {"B": B, "fused_us": round(float(np.median(tf)), 2), "aten_us": round(float(np.median(ta)), 2),
            "speedup": round(float(np.median(ta) / np.median(tf)), 2), "loss_rel_diff": loss_diff, "grad_rel_max_diff": diff,
            "head_bwd_bytes": nbytes, "head_bwd_bytes_us_at_8TBps": round(nbytes / 8e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--head-only", action="store_true", help="only the fused head + loss loop (for a rocprofv3 run)")
    args = ap.parse_args()
    res = {"metric": "depth_train"}
    if not args.head_only:
        res["step"] = step(args.iters)
    res["head_loss_fwd_bwd"] = head_loss(5 * args.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
