"""The adjoint of the statistics head against the plain head's adjoint, and the uncertainty-aware training step against the plain one
(rag_amd/csrc/disp_stats_train.hip).  One process; writes one JSON file (default
profiles/disp_stats_train_bench.json) and prints it.
  * adjoint: ops.disp_softargmin_bwd (disp_softargmin_bwd_kernel, one cotangent) and ops.disp_softargmin_stats_bwd
    (disp_softargmin_stats_bwd_kernel, all four cotangents) on the same cost, at the cost shapes [B,1,64,64,128] (the 192 x 384
    training crop; B = 1 and the reference's training batch of 8) and [1,1,64,128,416] (the headline head shape).  Each call zeroes
    its dcost first (a fill kernel, the same in both).  Device events around replays of a captured graph that holds INNER calls,
    the two graphs replayed ALTERNATELY over ROUNDS rounds, median of the rounds (min and max are reported);
  * step: rag_amd.train.GraphedTrainStep with and without uncertainty=True on two identical all-conv Networks at 192 x 384,
    D = 192, B = 2 (the smallest batch the census accepts), replayed alternately, device events around each step (forward +
    backward as one graph, clip and SGD eager), median of the rounds.
No time is gated.
    python tools/bench_disp_stats_train.py [--out FILE] [--rounds R] [--replays N] [--inner N] [--no-step]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rag_amd  # noqa: E402
from rag_amd import ops  # noqa: E402
from bench_disp_stats import events_us, graphed  # noqa: E402

DEV = "cuda:0"
MAXDISP = 192
SHAPES = ((1, 64, 64, 128), (8, 64, 64, 128), (1, 64, 128, 416))


def cost_volume(B, D, H, W):
    """A cost with a mode per coarse pixel plus noise (what a trained network hands the head), seeded."""
    g = torch.Generator().manual_seed(10 + B + H)
    t = torch.rand((B, 1, H, W), generator=g) * (D - 1)
    z = torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)
    return (0.5 * (z - t) ** 2 + 0.05 * torch.randn((B, D, H, W), generator=g)).to(DEV)


def med(v):
    return {"us": round(statistics.median(v), 2), "min_max": [round(min(v), 2), round(max(v), 2)]}


def adjoint_case(B, D, H, W, args):
    cost = cost_volume(B, D, H, W)
    g = torch.Generator().manual_seed(20 + B + H)
    dout = torch.randn((B, 3 * H, 3 * W), generator=g).to(DEV)
    dstats = torch.randn((B, 3, 3 * H, 3 * W), generator=g).to(DEV)
    gp = graphed(lambda: ops.disp_softargmin_bwd(cost, dout, MAXDISP), args.inner)
    gs = graphed(lambda: ops.disp_softargmin_stats_bwd(cost, dout, dstats, MAXDISP), args.inner)
    gz = graphed(lambda: torch.zeros_like(cost), args.inner)
    for gr in (gp, gs, gz):
        gr.replay()
    torch.cuda.synchronize()
    tp, ts, tz = [], [], []
    for _ in range(args.rounds):
        tp.append(events_us(gp.replay, args.replays) / args.inner)
        ts.append(events_us(gs.replay, args.replays) / args.inner)
        tz.append(events_us(gz.replay, args.replays) / args.inner)
    p, s, z = med(tp), med(ts), med(tz)
    return {"plain_bwd": p, "stats_bwd": s, "dcost_fill": z, "stats_over_plain": round(s["us"] / p["us"], 3),
            "stats_over_plain_without_fill": round((s["us"] - z["us"]) / (p["us"] - z["us"]), 3),
            "fine_samples": B * MAXDISP * 9 * H * W, "bytes_read_cost": B * D * H * W * 4, "bytes_read_cotangents": 4 * B * 9 * H * W * 4}


def step_case(args):
    from rag_amd.train import GradBucket, GraphedTrainStep, make_optimizer
    B, H, W = 2, 192, 384
    g = torch.Generator().manual_seed(1234)
    left, right = torch.randn((B, 3, H, W), generator=g).to(DEV), torch.randn((B, 3, H, W), generator=g).to(DEV)
    gt = (torch.rand((B, H, W), generator=g) * 200).to(DEV)
    steps = {}
    for name, unc in (("plain", False), ("uncertainty", True)):
        torch.manual_seed(0)
        net = rag_amd.Network(rag_amd.ALL_CONV_GENOTYPE, DEV, maxdisp=MAXDISP).to(DEV).train()
        bucket = GradBucket(net.parameters())
        opt = make_optimizer(net.parameters(), bucket=bucket)
        steps[name] = GraphedTrainStep(net, opt, bucket, left, right, gt, clip=5.0, uncertainty=unc)
    times = {k: [] for k in steps}
    for _ in range(args.rounds):
        for name, st in steps.items():
            times[name].append(events_us(st, 3) / 1e3)
    out = {name: {"ms": round(statistics.median(v), 3), "min_max": [round(min(v), 3), round(max(v), 3)],
                  "kernel_nodes": steps[name].node_census["kernel"], "loss": round(float(steps[name].loss), 5)} for name, v in times.items()}
    out["uncertainty_over_plain"] = round(out["uncertainty"]["ms"] / out["plain"]["ms"], 4)
    out["workload"] = f"all-conv Network, {B} pairs at {H}x{W}, D={MAXDISP}, fp32, forward+backward as one graph, clip 5 + FlatSGD eager"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "disp_stats_train_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step comparison")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_disp_stats_train needs the MI355X"
    out = {"metric": "adjoint of the disparity head: plain (disparity) vs statistics (disparity, variance, peak, entropy)",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "timing": f"device events around {args.replays} replays of a captured graph of {args.inner} calls; the graphs alternate over "
                     f"{args.rounds} rounds; median, with min and max; every call includes the fill of its dcost (timed alone as dcost_fill)",
           "adjoint": {}}
    for (B, D, H, W) in SHAPES:
        out["adjoint"][f"B{B}_{D}x{H}x{W}"] = adjoint_case(B, D, H, W, args)
    if not args.no_step:
        out["step"] = step_case(args)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
