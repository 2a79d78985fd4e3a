"""The disparity head with and without the per-pixel statistics of its distribution (rag_amd/csrc/disp.hip) at the headline head shape,
cost [B, 1, 64, 128, 416] -> 384 x 1248, B = 1 and 8, fp32 cost.  One process; writes one JSON file (default
profiles/disp_stats_bench.json) and prints it.  Per batch size:
  * plain_us      ops.disp_softargmin       (disp_softargmin_x3_kernel<float, false, false>, the register form);
  * stats_us      ops.disp_softargmin_stats (disp_softargmin_x3_kernel<float, true, false>), caller-owned outputs;
                  both: device events around replays of a captured graph that holds INNER launches, the two graphs replayed
                  ALTERNATELY over ROUNDS rounds, median of the rounds (the spread is reported);
  * aten_us       the twin rag_amd.metrics.disp_stats_torch on the same GPU (F.interpolate -> softmin -> moments), device events
                  around eager calls: the route a user had before;
  * the equality of the two launches' disparity, the statistics' distance from the ATen twin, and the algorithmic bytes.
No time is gated.
    python tools/bench_disp_stats.py [--out FILE] [--rounds R] [--replays N] [--inner N]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_amd import ops  # noqa: E402
from rag_amd.metrics import disp_stats_torch  # noqa: E402

DEV = "cuda:0"
D, H, W, MAXDISP = 64, 128, 416, 192


def events_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def graphed(fn, inner):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    return graph


def cost_volume(B):
    """A cost with a mode per coarse pixel plus noise (what a trained network hands the head), seeded."""
    g = torch.Generator().manual_seed(10 + B)
    t = torch.rand((B, 1, H, W), generator=g) * (D - 1)
    z = torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)
    return (0.5 * (z - t) ** 2 + 0.05 * torch.randn((B, D, H, W), generator=g))[:, None].to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "disp_stats_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_disp_stats needs the MI355X"
    out = {"metric": f"disparity head, cost [B,1,{D},{H},{W}] fp32 -> {3 * H}x{3 * W}, plain vs statistics launch", "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "hip": torch.version.hip,
           "timing": {"plain_us / stats_us": f"device events around {args.replays} replays of a captured graph of {args.inner} launches; the two graphs "
                                             f"alternate over {args.rounds} rounds; median, with min and max",
                      "aten_us": "device events around 5 eager calls of disp_stats_torch on cuda (after 2 warm-up calls)"},
           "cases": {}}
    with torch.no_grad():
        for B in (1, 8):
            cost = cost_volume(B)
            disp = torch.empty((B, 3 * H, 3 * W), device=DEV)
            stats = torch.empty((B, 3, 3 * H, 3 * W), device=DEV)
            plain_out = ops.disp_softargmin(cost, MAXDISP)
            ops.disp_softargmin_stats(cost, MAXDISP, disp, stats)
            twin_disp, twin_stats = disp_stats_torch(cost, MAXDISP)
            torch.cuda.synchronize()
            same = bool(torch.equal(plain_out, disp))
            dist = {name: float((stats[:, p] - twin_stats[:, p]).abs().max()) for p, name in enumerate(("variance", "peak", "entropy"))}
            del twin_disp, twin_stats
            gp = graphed(lambda: ops.disp_softargmin(cost, MAXDISP), args.inner)
            gs = graphed(lambda: ops.disp_softargmin_stats(cost, MAXDISP, disp, stats), args.inner)
            for g in (gp, gs):
                g.replay()
            torch.cuda.synchronize()
            tp, ts = [], []
            for _ in range(args.rounds):
                tp.append(events_us(gp.replay, args.replays) / args.inner)
                ts.append(events_us(gs.replay, args.replays) / args.inner)
            for _ in range(2):
                disp_stats_torch(cost, MAXDISP)
            aten_us = events_us(lambda: disp_stats_torch(cost, MAXDISP), 5)
            plain_us, stats_us = statistics.median(tp), statistics.median(ts)
            read, px = B * D * H * W * 4, B * 9 * H * W * 4
            out["cases"][f"B{B}"] = {
                "plain_us": round(plain_us, 2), "plain_us_min_max": [round(min(tp), 2), round(max(tp), 2)],
                "stats_us": round(stats_us, 2), "stats_us_min_max": [round(min(ts), 2), round(max(ts), 2)],
                "stats_over_plain": round(stats_us / plain_us, 3), "aten_us": round(aten_us, 1), "aten_over_stats": round(aten_us / stats_us, 1),
                "disparity_bitwise_equal": same, "stats_max_abs_diff_vs_aten_fp32_twin": dist,
                "bytes_read": read, "bytes_written_plain": px, "bytes_written_stats": 4 * px,
                "stats_GBps": round((read + 4 * px) / stats_us * 1e-3, 1), "aten_upsampled_tensor_bytes": B * MAXDISP * 9 * H * W * 4}
            del gp, gs
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
