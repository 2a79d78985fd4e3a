"""Sparsification curves + AUSE / AURG (rag_amd/csrc/sparsify.hip) against the ATen route at 384 x 1248, B = 1 and 8, K = 20 fractions.
One process; writes one JSON file (default profiles/sparsification_bench.json) and prints it.  Per batch size:
  * fused_us        rag_amd.sparsification with a CalibrationMeter (the call allocates its workspace from torch's cache): device
                    events around replays of a captured graph that holds INNER calls, median over ROUNDS rounds (spread reported);
  * fused_ties_*    the same with unc quantised to 4 values (every cut inside a large tie group) and with one constant unc: the
                    inputs that put most pixels into a few histogram bins;
  * aten_us         the route a user had before, per image: boolean-mask gather (a host synchronisation), torch.sort of unc and of the
                    error, cumsum, a gather at the K cuts; device events around eager calls.  It breaks ties arbitrarily and cannot be
                    captured;
  * the distance of the fused result from the float64 twin on the CPU, in fp32 ulps.
No time is gated.
    python tools/bench_sparsification.py [--out FILE] [--rounds R] [--replays N] [--inner N]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rag_amd  # noqa: E402
from rag_amd.metrics import sparsification_torch  # noqa: E402

DEV = "cuda:0"
H, W, MAXDISP, K = 384, 1248, 192, 20


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


def inputs(B):
    """gt with a fifth of the pixels outside the mask, disp = gt + noise with a heavy tail, unc correlated with the error; seeded."""
    g = torch.Generator().manual_seed(20 + B)
    gt = 1.0 + (MAXDISP - 2.0) * torch.rand((B, H, W), generator=g)
    gt = torch.where(torch.rand((B, H, W), generator=g) < 0.2, torch.zeros_like(gt), gt)
    noise = torch.randn((B, H, W), generator=g) * torch.where(torch.rand((B, H, W), generator=g) < 0.1, 8.0, 0.6)
    unc = noise.abs() * (1 + 0.5 * torch.randn((B, H, W), generator=g)).abs() + 0.05
    return gt + noise, unc, gt


def aten_route(disp, unc, gt):
    """Per image: gather the masked pixels, sort by unc and by error, cumulative sums, read the K cuts (ties in arbitrary order)."""
    out = []
    for b in range(disp.shape[0]):
        mask = (gt[b] > 0) & (gt[b] < MAXDISP) & torch.isfinite(disp[b]) & torch.isfinite(unc[b])
        err = (disp[b][mask] - gt[b][mask]).abs().double()               # the gather synchronises
        n = err.numel()
        keep = n - (torch.arange(K, device=err.device) * n) // K
        by_unc = err[torch.sort(unc[b][mask]).indices].cumsum(0)[keep - 1] / keep
        by_err = torch.sort(err).values.cumsum(0)[keep - 1] / keep
        out.append(torch.stack((by_unc, by_err, (by_unc - by_err).mean().expand(K))))
    return torch.stack(out)


def max_ulp(a, b):
    def ordered(x):
        i = x.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))
    a, b = a.cpu().float().reshape(-1), b.cpu().float().reshape(-1)
    keep = ~(torch.isnan(a) | torch.isnan(b))
    return int((ordered(a[keep]) - ordered(b[keep])).abs().max())


def timed(graph, rounds, replays, inner):
    graph.replay()
    torch.cuda.synchronize()
    t = [events_us(graph.replay, replays) / inner for _ in range(rounds)]
    return round(statistics.median(t), 2), [round(min(t), 2), round(max(t), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sparsification_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sparsification needs the MI355X"
    lib = rag_amd.load_library()
    out = {"metric": f"sparsification curves + AUSE / AURG, [B,{H},{W}] fp32, K = {K}: fused HIP call vs the ATen route",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "timing": {"fused_us": f"device events around {args.replays} replays of a captured graph of {args.inner} calls (11 launches each); "
                                  f"median of {args.rounds} rounds, with min and max",
                      "aten_us": "device events around 3 eager calls of the gather / sort / cumsum route (after 1 warm-up call)"},
           "cases": {}}
    with torch.no_grad():
        for B in (1, 8):
            disp_c, unc_c, gt_c = inputs(B)
            disp, unc, gt = disp_c.to(DEV), unc_c.to(DEV), gt_c.to(DEV)
            quant = (unc * 4).floor().clamp(max=3.0)
            const = torch.full_like(unc, 0.5)
            meter = rag_amd.CalibrationMeter(DEV, K)
            got = rag_amd.sparsification(disp, unc, gt, MAXDISP, K)
            twin = sparsification_torch(disp_c, unc_c, gt_c, MAXDISP, K)
            ulp = max(max_ulp(got.tensor, twin.tensor), max_ulp(got.scalars, twin.scalars))
            got_q = rag_amd.sparsification(disp, quant, gt, MAXDISP, K)
            ulp_q = max_ulp(got_q.tensor, sparsification_torch(disp_c, quant.cpu(), gt_c, MAXDISP, K).tensor)
            case = {"max_ulp_vs_float64_twin": ulp, "max_ulp_vs_float64_twin_ties": ulp_q,
                    "workspace_bytes": 16 * int(lib.ragmi_sparsification_workspace_elems(B, H, W, K)), "bytes_read_per_pass": 3 * B * H * W * 4}
            for name, u in (("fused_us", unc), ("fused_ties_quant4_us", quant), ("fused_ties_constant_us", const)):
                graph = graphed(lambda u=u: rag_amd.sparsification(disp, u, gt, MAXDISP, K, meter=meter), args.inner)
                case[name], case[name + "_min_max"] = timed(graph, args.rounds, args.replays, args.inner)
                del graph
            aten_route(disp, unc, gt)
            case["aten_us"] = round(events_us(lambda: aten_route(disp, unc, gt), 3), 1)
            case["aten_over_fused"] = round(case["aten_us"] / case["fused_us"], 1)
            out["cases"][f"B{B}"] = case
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
