"""The disparity head's plain, statistics and mode launches (rag_amd/csrc/disp.hip) at the headline head shape, cost [1, 1, 64, 128, 416]
-> 384 x 1248, fp32 cost.  One process; writes one JSON file (default profiles/disp_mode_bench.json) and prints it.
  * plain_us      ops.disp_softargmin       (disp_softargmin_x3_kernel<float, false, false>, the register form);
  * stats_us      ops.disp_softargmin_stats (disp_softargmin_x3_kernel<float, true, false>), caller-owned outputs;
  * mode_us       ops.disp_softargmin_mode  (disp_softargmin_x3_kernel<float, true, true>) at radius MODE_RADIUS, caller-owned outputs, and
                  mode_full_us at radius maxdisp (the radius is a kernel argument: the same code object);
                  all: device events around replays of a captured graph that holds INNER launches, the graphs replayed ALTERNATELY over
                  ROUNDS rounds, median of the rounds (the spread is reported);
  * aten_us       the twin rag_amd.metrics.disp_mode_torch on the same GPU (F.interpolate -> softmin -> moments -> arg-min -> window
                  sums), device events around eager calls: the route a user had before;
  * the equality of the three launches' disparity and of the two launches' statistics, the mode planes' distance from the ATen twin
    evaluated about the kernel's own index, and the share of pixels on which the two arg-mins differ.
No time is gated.
    python tools/bench_disp_mode.py [--out FILE] [--rounds R] [--replays N] [--inner N]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_amd import ops  # noqa: E402
from rag_amd.metrics import MODE_RADIUS, disp_mode_torch  # noqa: E402

DEV = "cuda:0"
B, D, H, W, MAXDISP = 1, 64, 128, 416, 192


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


def cost_volume():
    """A cost with a mode per coarse pixel plus noise (what a trained network hands the head), seeded."""
    g = torch.Generator().manual_seed(10 + B)
    t = torch.rand((B, 1, H, W), generator=g) * (D - 1)
    z = torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)
    return (0.5 * (z - t) ** 2 + 0.05 * torch.randn((B, D, H, W), generator=g))[:, None].to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "disp_mode_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_disp_mode needs the MI355X"
    with torch.no_grad():
        cost = cost_volume()
        shape = (B, 3 * H, 3 * W)
        disp_s, disp_m = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
        stats_s, stats_m, mode = (torch.empty((B, 3, 3 * H, 3 * W), device=DEV) for _ in range(3))
        plain_out = ops.disp_softargmin(cost, MAXDISP)
        ops.disp_softargmin_stats(cost, MAXDISP, disp_s, stats_s)
        ops.disp_softargmin_mode(cost, MAXDISP, MODE_RADIUS, disp_m, stats_m, mode)
        torch.cuda.synchronize()
        same = bool(torch.equal(plain_out, disp_m)) and bool(torch.equal(disp_s, disp_m)) and bool(torch.equal(stats_s, stats_m))
        _d, _s, own = disp_mode_torch(cost, MAXDISP, MODE_RADIUS)
        differ = float((own[:, 0] != mode[:, 0]).float().mean())
        del _d, _s, own
        _d, _s, twin = disp_mode_torch(cost, MAXDISP, MODE_RADIUS, index=mode[:, 0])
        dist = {name: float((mode[:, p] - twin[:, p]).abs().max()) for p, name in enumerate(("index", "disp", "mass"))}
        flying = float(((mode[:, 1] - disp_m).abs() > 1.0).float().mean())
        del _d, _s, twin
        graphs = {"plain": graphed(lambda: ops.disp_softargmin(cost, MAXDISP), args.inner),
                  "stats": graphed(lambda: ops.disp_softargmin_stats(cost, MAXDISP, disp_s, stats_s), args.inner),
                  "mode": graphed(lambda: ops.disp_softargmin_mode(cost, MAXDISP, MODE_RADIUS, disp_m, stats_m, mode), args.inner),
                  "mode_full": graphed(lambda: ops.disp_softargmin_mode(cost, MAXDISP, MAXDISP, disp_m, stats_m, mode), args.inner)}
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
        times = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                times[k].append(events_us(g.replay, args.replays) / args.inner)
        for _ in range(2):
            disp_mode_torch(cost, MAXDISP, MODE_RADIUS)
        aten_us = events_us(lambda: disp_mode_torch(cost, MAXDISP, MODE_RADIUS), 5)
    med = {k: statistics.median(v) for k, v in times.items()}
    read, px = B * D * H * W * 4, B * 9 * H * W * 4
    out = {"metric": f"disparity head, cost [{B},1,{D},{H},{W}] fp32 -> {3 * H}x{3 * W}: plain, statistics and mode launch (radius {MODE_RADIUS})",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "timing": {"plain_us / stats_us / mode_us / mode_full_us": f"device events around {args.replays} replays of a captured graph of {args.inner} "
                                                                      f"launches; the four graphs alternate over {args.rounds} rounds; median, with min and max",
                      "aten_us": "device events around 5 eager calls of disp_mode_torch on cuda (after 2 warm-up calls)"},
           "radius": MODE_RADIUS}
    for k in graphs:
        out[f"{k}_us"] = round(med[k], 2)
        out[f"{k}_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    out.update({"stats_over_plain": round(med["stats"] / med["plain"], 3), "mode_over_stats": round(med["mode"] / med["stats"], 3),
                "mode_over_plain": round(med["mode"] / med["plain"], 3), "mode_full_over_mode": round(med["mode_full"] / med["mode"], 3),
                "aten_us": round(aten_us, 1), "aten_over_mode": round(aten_us / med["mode"], 1),
                "disparity_and_stats_bitwise_equal": same, "mode_max_abs_diff_vs_aten_fp32_twin_about_kernel_index": dist,
                "argmin_differs_from_aten_fp32_twin_share": differ, "pixels_with_mode_disp_over_1px_from_disp_share": flying,
                "bytes_read": read, "bytes_written_plain": px, "bytes_written_stats": 4 * px, "bytes_written_mode": 7 * px,
                "mode_GBps": round((read + 7 * px) / med["mode"] * 1e-3, 1), "aten_upsampled_tensor_bytes": B * MAXDISP * 9 * H * W * 4})
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
