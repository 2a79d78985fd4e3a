"""The self-supervised loss (re_and_sm_loss, src_self/models/loss.py:112-141) at the continual-adaptation training shape (B = 3,
192x384, run_rag_self.sh; D = 192), one JSON line on stdout:
  * loss forward + backward: the fused HIP kernels (rag_amd.metrics.re_and_sm_loss) against the plain-torch restatement
    (rag_amd.metrics.re_and_sm_loss_torch, ATen kernels) on the same GPU: us per call from device events around back-to-back calls,
    and launches per call counted by torch.profiler;
  * the graphed training step (rag_amd.train.GraphedTrainStep) with supervise=True against supervise=False, timed alternately in
    one process (ms per step, device events).
    python tools/bench_selfsup.py [--loss-only] [--iters N] [--steps K] [--rounds R]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rag_amd as ra  # noqa: E402

B, C, H, W, MAXDISP = 3, 3, 192, 384, 192
DEV = "cuda:0"


def inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    left = torch.randn((B, C, H, W), generator=g).to(DEV)
    right = torch.randn((B, C, H, W), generator=g).to(DEV)
    disp = (torch.rand((B, H, W), generator=g) * MAXDISP).to(DEV)
    return disp, left, right


def loss_call(fn, d, left, right):
    d.grad = None                                     # every call allocates its gradient (no accumulation kernel)
    fn(d, left, right).backward()


def time_loss(fn, d, left, right, iters):
    for _ in range(20):
        loss_call(fn, d, left, right)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        loss_call(fn, d, left, right)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def count_launches(fn, d, left, right):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    loss_call(fn, d, left, right)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loss_call(fn, d, left, right)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    return len(names), sorted(set(names))


def graphed_steps(steps, rounds):
    from rag_amd.train import GradBucket, GraphedTrainStep, make_optimizer
    g = torch.Generator().manual_seed(1234)
    left = torch.randn((B, 3, H, W), generator=g).to(DEV)
    right = torch.randn((B, 3, H, W), generator=g).to(DEV)
    gt = (torch.rand((B, H, W), generator=g) * 200).to(DEV)
    runs = {}
    for supervise in (True, False):
        torch.manual_seed(0)
        net = ra.Network(ra.ALL_CONV_GENOTYPE, DEV, maxdisp=MAXDISP).to(DEV).train()
        bucket = GradBucket(net.parameters())
        opt = make_optimizer(net.parameters(), bucket=bucket)
        step = GraphedTrainStep(net, opt, bucket, left, right, gt if supervise else None, clip=5.0, supervise=supervise)
        runs["supervised" if supervise else "self_supervised"] = (step, step.node_census)
    times = {k: [] for k in runs}
    for k, (step, _) in runs.items():                # warm-up replays
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    for _ in range(rounds):                          # alternate the two modes: shared-host noise hits both
        for k, (step, _) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return {"ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
            "ms_per_step_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
            "ratio_self_over_supervised": round(med["self_supervised"] / med["supervised"], 4),
            "graph_nodes": {k: c for k, (_, c) in runs.items()}, "steps_per_round": steps, "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss-only", action="store_true", help="skip the graphed training steps (profiling runs)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_selfsup needs the MI355X"
    d0, left, right = inputs()
    d = d0.clone().requires_grad_(True)
    hip = lambda a, b_, c: ra.metrics.re_and_sm_loss(a, b_, c)            # noqa: E731
    aten = lambda a, b_, c: ra.metrics.re_and_sm_loss_torch(a, b_, c)[0]  # noqa: E731
    with torch.no_grad():
        l_hip = float(ra.metrics.self_supervised_terms(d0, left, right)[0])
        l_aten = float(aten(d0, left, right))
    us_hip = time_loss(hip, d, left, right, args.iters)
    us_aten = time_loss(aten, d, left, right, args.iters)
    n_hip, k_hip = count_launches(hip, d, left, right)
    n_aten, _ = count_launches(aten, d, left, right)
    nbytes = B * H * W * (8 * C + 8)                   # left + right read (8C), disp read + unit gradient written (8)
    out = {"metric": f"self-supervised loss fwd+bwd at B={B}, {H}x{W}, C={C}", "unit": "us",
           "loss_fwd_bwd_us": {"hip": round(us_hip, 2), "aten": round(us_aten, 2)},
           "launches_per_fwd_bwd": {"hip": n_hip, "aten": n_aten}, "hip_kernels": k_hip,
           "timing": f"device events around {args.iters} back-to-back eager forward+backward calls (after 20 warm-up calls)",
           "loss_value": {"hip": l_hip, "aten_fp32": l_aten},
           "algorithmic_bytes": nbytes, "hbm_floor_us_at_8TBps": round(nbytes / 8e12 * 1e6, 2)}
    if not args.loss_only:
        out["graphed_step"] = graphed_steps(args.steps, args.rounds)
        out["graphed_step"]["config"] = f"GraphedTrainStep, all-conv Network, B={B}, {H}x{W}, D={MAXDISP}, fp32, FlatSGD"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
