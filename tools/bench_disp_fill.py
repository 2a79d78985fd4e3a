"""The dense-disparity fill, one JSON line on stdout (also written to --out):
  * at one 384x1248 pair (stacked 2) and at eight pairs (stacked 16), on the same build: rag_amd.metrics.fill_disparity alone and with
    the 3x3 / 5x5 median, for the fp32 weight of the left-right check and for a bool mask, each against its ATen twin
    (fill_disparity_torch on the same GPU): us per call from device events around back-to-back calls, the variants taken in turn in
    every round, and launches per call counted by torch.profiler; the byte floor of the fill and what it gives at 8 TB/s;
  * Network.forward_dense against Network.forward_lr (the code of the parent commit, unchanged) on one 384x1248 pair, alternately in
    one process (ms per call, device events);
  * --kernels-only runs nothing but the HIP calls, for a `rocprofv3 --kernel-trace --stats` run of its own:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_disp_fill.py --kernels-only
    python tools/bench_disp_fill.py [--pieces-only] [--kernels-only] [--iters N] [--calls K] [--rounds R] [--out PATH]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rag_amd as ra  # noqa: E402

SHAPES = {"pair_B1_384x1248": (1, 384, 1248), "pairs_B8_384x1248": (8, 384, 1248)}
NET_H, NET_W, MAXDISP = 384, 1248, 192
DEV = "cuda:0"


def timed(variants, iters, rounds, warmup=20):
    """{name: (median per call, [per call of each round])} in us: device events around `iters` back-to-back calls, the variants taken
    in turn in each of `rounds` rounds (shared-host noise hits all of them), after `warmup` calls of each."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: (sorted(v)[len(v) // 2], [round(x, 2) for x in v]) for k, v in times.items()}


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if e.device_type == DeviceType.CUDA])


def inputs(name):
    """Stacked disparities as in tools/bench_lr_check.py (one level per pair plus noise of the size of the tolerance) and their own
    left-right check: consistent pixels, mismatches and the out-of-view band at the rows' ends."""
    B, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(0)
    level = (torch.rand((B, 1, 1), generator=g) * 40 + 8).repeat(2, 1, 1)
    disp = (level + torch.rand((2 * B, H, W), generator=g) * 1.5).to(DEV)
    chk = ra.lr_consistency(disp, disp, mirrored=True, partner_shift=B, want_error=False)
    return disp, chk


def calls(disp, chk):
    mask = chk.mask
    out = {}
    for form, keep in (("weight_fp32", chk.weight), ("mask_bool", mask)):
        for median in (0, 3, 5):
            out[f"fill_median{median}_{form}"] = dict(hip=lambda k=keep, m=median: ra.fill_disparity(disp, k, median=m),
                                                      aten=lambda k=keep, m=median: ra.fill_disparity_torch(disp, k, median=m))
    return out


def pieces(name, iters, rounds):
    B, H, W = SHAPES[name]
    disp, chk = inputs(name)
    out = {"shape": {"pairs": B, "stacked": 2 * B, "H": H, "W": W}, "kept_share": round(float(chk.valid.mean()), 4)}
    for key, variants in calls(disp, chk).items():
        t = timed(variants, iters, rounds)
        got, want = variants["hip"](), variants["aten"]()
        out[key] = {"us_median": {k: round(v[0], 2) for k, v in t.items()}, "us_all": {k: v[1] for k, v in t.items()},
                    "aten_over_hip": round(t["aten"][0] / t["hip"][0], 2), "launches": {k: launches(fn) for k, fn in variants.items()},
                    "equal_to_twin": bool(torch.equal(got.disp, want.disp) and torch.equal(got.code, want.code)
                                          and torch.equal(got.counts, want.counts))}
    npx = 2 * B * H * W
    # the fill reads disp and keep (8 B with the fp32 weight, 5 B with a byte mask), writes out and code (5 B) and reads its own
    # out and code back once in the second sweep (5 B); the median reads and writes the map once more
    out["algorithmic_bytes"] = {"fill_weight_fp32": 18 * npx, "fill_mask_bool": 15 * npx, "median": 8 * npx}
    out["hbm_floor_us_at_8TBps"] = {k: round(v / 8e12 * 1e6, 2) for k, v in out["algorithmic_bytes"].items()}
    out["codes"] = ra.fill_disparity(disp, chk).counts.sum(0).tolist()
    return out


def dense_against_lr(n_calls, rounds):
    g = torch.Generator().manual_seed(1234)
    left = torch.randn((1, 3, NET_H, NET_W), generator=g).to(DEV)
    right = torch.randn((1, 3, NET_H, NET_W), generator=g).to(DEV)
    torch.manual_seed(0)
    net = ra.Network(ra.ALL_CONV_GENOTYPE, DEV, maxdisp=MAXDISP).to(DEV).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    variants = {"forward_lr": lambda: net.forward_lr(left, right, 0, net.arch_init, want_error=False),
                "forward_dense": lambda: net.forward_dense(left, right, 0, net.arch_init, want_error=False),
                "forward_dense_median3": lambda: net.forward_dense(left, right, 0, net.arch_init, median=3, want_error=False)}
    t = timed(variants, n_calls, rounds, warmup=2)
    med = {k: v[0] / 1e3 for k, v in t.items()}
    return {"config": f"all-conv Network, eval, one {NET_H}x{NET_W} pair (forward of the stacked 2), D={MAXDISP}, fp32, eager",
            "ms_per_call_median": {k: round(v, 4) for k, v in med.items()},
            "ms_per_call_all": {k: [round(x / 1e3, 4) for x in v[1]] for k, v in t.items()},
            "ratio_dense_over_lr": round(med["forward_dense"] / med["forward_lr"], 4),
            "ratio_dense_median3_over_lr": round(med["forward_dense_median3"] / med["forward_lr"], 4),
            "calls_per_round": n_calls, "rounds": rounds}


def kernels_only(iters):
    for name in SHAPES:
        disp, chk = inputs(name)
        for variants in calls(disp, chk).values():
            for _ in range(iters):
                variants["hip"]()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces-only", action="store_true", help="skip forward_dense against forward_lr")
    ap.add_argument("--kernels-only", action="store_true", help="only the HIP calls, for a kernel-trace run; prints nothing")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_disp_fill needs the MI355X"
    if args.kernels_only:
        kernels_only(args.iters)
        return
    out = {"metric": "dense-disparity fill (row scan, column pass, count finalize) and its 3x3 / 5x5 median; forward_dense", "unit": "us / ms",
           "timing": f"pieces: device events around {args.iters} back-to-back eager calls, variants in turn in each of {args.rounds} rounds, "
                     "median (after 20 warm-up calls each); an eager call includes the host's launch cost and its five allocations "
                     "when the device work is shorter than them",
           "pieces": {name: pieces(name, args.iters, args.rounds) for name in SHAPES}}
    if not args.pieces_only:
        out["forward_dense"] = dense_against_lr(args.calls, args.rounds)
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
