#!/usr/bin/env python3
"""Monocular-depth inference on the MI355X: one JSON line, every number measured in this one process.

  * images -> depth maps per second at 384x1248 (features 128x416), B=1 and B=8: the forward captured as ONE hipGraph, replays
    timed with HIP events after a warm-up (the model: g14's trained task-3 weights, the last unit of every layer);
  * the fused head kernel (ops.depth_head) against the same head as the eager ATen sequence (F.interpolate, conv2d, conv2d,
    sigmoid, F.interpolate, mul), alternated in one loop, HIP events;
  * the head's algorithmic bytes: 12 (h/2)(w/2) x 4 in + 3h 3w x 4 out, 2.56 MB at B=1 (launch-bound, not HBM-bound);
  * the kernel-node count of the captured forward and its memcpy / memset nodes;
  * aten_kernels: GPU kernels of one eager forward whose name is not a ragmi:: kernel (torch.profiler).

Usage:  python tools/bench_depth.py [--iters N]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rag_amd import ops  # noqa: E402
from rag_amd.depth import depth_head_torch, load_depth_checkpoint  # noqa: E402
from rag_amd.train import graph_census  # noqa: E402

DEV = "cuda:0"
H_IMG, W_IMG = 384, 1248


def model():
    path = os.path.join(ROOT, "tests", "golden", "g14_depth_ckpt_task3.npz")
    with np.load(path) as z:
        sd = {k: torch.as_tensor(z[k]) for k in z.files}
    net, _ = load_depth_checkpoint({"model": sd}, DEV, "from_keys")
    archi = {name: [len(net._units(name)) - 1] for name in net._p_layers() + ["last_3_3d", "last_6_3d", "last_12_3d"]}
    return net, archi


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3        # us per call


def graphed(net, archi, B, iters):
    g = torch.Generator().manual_seed(B)
    left = (torch.rand((B, 3, H_IMG, W_IMG), generator=g) * 2 - 1).to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                net(left, None, 3, archi)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            out = net(left, None, 3, archi)
        census = graph_census(graph)
        graph.instantiate()
        eager = net(left, None, 3, archi)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), "graph replay differs from the eager forward"
        us = timed(graph.replay, iters)
    return us, census


def aten_kernels(net, archi):
    from torch.profiler import ProfilerActivity, profile
    left = torch.rand((1, 3, H_IMG, W_IMG)).to(DEV)
    with torch.no_grad():
        net(left, None, 3, archi)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            net(left, None, 3, archi)
            torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "ragmi" not in e.name
             and not e.name.startswith(("Memcpy", "Memset", "hip"))]
    return len(names), sorted(set(names))[:8]


def head(B, iters):
    h, w = H_IMG // 3, W_IMG // 3
    g = torch.Generator().manual_seed(7)
    y = torch.randn((B, 12, h // 2, w // 2), generator=g).to(DEV)
    w3 = (torch.randn((1, 12, 3, 3), generator=g) * 0.1).to(DEV)
    w1 = (torch.randn((1, 1, 3, 3), generator=g) * 0.3).to(DEV)
    b1 = torch.randn((1,), generator=g).to(DEV)
    fused = lambda: ops.depth_head(y, w3, w1, b1, (h, w), 3, 80.0)  # noqa: E731
    aten = lambda: depth_head_torch(y, w3, w1, b1, (h, w), 3, 80.0)  # noqa: E731
    with torch.no_grad():
        err = float((fused() - aten()).abs().max())
        for _ in range(5):
            fused(), aten()
        tf, ta = [], []
        for _ in range(5):                     # alternated: both see the same clocks
            tf.append(timed(fused, iters))
            ta.append(timed(aten, iters))
    nbytes = 4 * (12 * (h // 2) * (w // 2) + 9 * h * w) * B
    return {"B": B, "fused_us": round(float(np.median(tf)), 2), "aten_us": round(float(np.median(ta)), 2),
            "speedup": round(float(np.median(ta) / np.median(tf)), 2), "max_abs_diff_m": err, "bytes": nbytes,
            "achieved_GBps": round(nbytes / (float(np.median(tf)) * 1e3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    net, archi = model()
    res = {"metric": "depth_inference", "image": [H_IMG, W_IMG], "precision": ops.get_conv_precision()}
    for B in (1, 8):
        us, census = graphed(net, archi, B, args.iters)
        res[f"B{B}"] = {"forward_us": round(us, 1), "maps_per_s": round(B * 1e6 / us, 1), "graph_kernel_nodes": census["kernel"],
                        "graph_memcpy_nodes": census["memcpy"], "graph_memset_nodes": census["memset"]}
    res["head"] = [head(1, 200), head(8, 100)]
    res["head_note"] = "launch-bound: 2.56 MB at B=1 is ~0.3 us of HBM time"
    n, names = aten_kernels(net, archi)
    res["aten_kernels"] = n
    res["aten_kernel_names"] = names
    print(json.dumps(res))


if __name__ == "__main__":
    main()
