"""The speckle filter, one JSON line on stdout (also written to --out):
  * at one 384x1248 pair (stacked 2) and at eight pairs (stacked 16), with the stacked disparities and checks of
    tools/bench_disp_fill.py: rag_amd.metrics.filter_speckles for the fp32 weight of the left-right check, a bool mask and no keep, against
    its ATen twin (filter_speckles_torch on the same GPU; a few calls only, it synchronises once per round): us per call from device
    events around back-to-back calls, the variants taken in turn in every round; launches per call and the mean device time of each
    kernel from torch.profiler; the bytes each launch moves and what they give at 8 TB/s;
  * Network.forward_dense with and without speckle=(100, 1.0) on one 384x1248 pair, alternately in one process (ms per call);
  * --kernels-only runs nothing but the HIP calls, for a `rocprofv3 --kernel-trace --stats` run of its own:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_speckle.py --kernels-only
    python tools/bench_speckle.py [--pieces-only] [--kernels-only] [--iters N] [--calls K] [--rounds R] [--out PATH]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rag_amd as ra  # noqa: E402
from bench_disp_fill import DEV, MAXDISP, NET_H, NET_W, SHAPES, inputs, launches, timed  # noqa: E402

MAX_SIZE, MAX_DIFF = 100, 1.0
TWIN_CALLS = 2


def kernel_times(fn, calls=20):
    """{kernel name: mean device us per launch} over `calls` calls, from torch.profiler."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    total, count = {}, {}
    for e in prof.events():
        if e.device_type == DeviceType.CUDA:
            name = e.name.split("(")[0].split("<")[0].split("::")[-1]
            total[name] = total.get(name, 0.0) + (e.device_time if hasattr(e, "device_time") else e.cuda_time)
            count[name] = count.get(name, 0) + 1
    return {k: round(total[k] / count[k], 2) for k in total}


def calls(disp, chk):
    return {"weight_fp32": chk.weight, "mask_bool": chk.mask, "none": None}


def pieces(name, iters, rounds):
    B, H, W = SHAPES[name]
    disp, chk = inputs(name)
    out = {"shape": {"pairs": B, "stacked": 2 * B, "H": H, "W": W}, "kept_share": round(float(chk.valid.mean()), 4),
           "max_size": MAX_SIZE, "max_diff": MAX_DIFF}
    for key, keep in calls(disp, chk).items():
        hip = lambda k=keep: ra.filter_speckles(disp, k, MAX_SIZE, MAX_DIFF)                 # noqa: E731
        aten = lambda k=keep: ra.filter_speckles_torch(disp, k, MAX_SIZE, MAX_DIFF)          # noqa: E731
        t = timed({"hip": hip}, iters, rounds)
        t.update(timed({"aten": aten}, TWIN_CALLS, 2, warmup=1))
        got, want = hip(), aten()
        out[key] = {"us_median": {k: round(v[0], 2) for k, v in t.items()}, "us_all": {k: v[1] for k, v in t.items()},
                    "aten_over_hip": round(t["aten"][0] / t["hip"][0], 1), "launches": {"hip": launches(hip), "aten": launches(aten)},
                    "kernel_us": kernel_times(hip),
                    "equal_to_twin": bool(torch.equal(got.keep, want.keep) and torch.equal(got.label, want.label)
                                          and torch.equal(got.size, want.size) and torch.equal(got.counts, want.counts)
                                          and torch.equal(got.density, want.density))}
    npx = 2 * B * H * W
    tr, tc = ra.metrics.SPECKLE_TILE
    tiles_y, tiles_x = (H + tr - 1) // tr, (W + tc - 1) // tc
    tiles = 2 * B * tiles_y * tiles_x
    # tile: reads disp and keep (8 B with the fp32 weight, 5 B with a byte mask, 4 B without), writes parent, lcount and total (12 B);
    # seam: per seam pixel two parent words, two disparities and the roots it touches (>= 24 B); flatten: reads parent and lcount,
    # walks to the root (>= one more word), writes label (>= 16 B); apply: reads label and total[label], writes size and keep_out (13 B)
    seam_px = 2 * B * ((tiles_x - 1) * H + (tiles_y - 1) * W)
    out["algorithmic_bytes"] = {"tile_weight_fp32": 20 * npx, "tile_mask_bool": 17 * npx, "tile_none": 16 * npx, "seam": 24 * seam_px,
                                "flatten": 16 * npx, "apply": 13 * npx}
    out["hbm_floor_us_at_8TBps"] = {k: round(v / 8e12 * 1e6, 2) for k, v in out["algorithmic_bytes"].items()}
    out["tiles"], out["seam_pixels"] = tiles, seam_px
    out["counts"] = dict(zip(ra.metrics.SPECKLE_COUNTS, ra.filter_speckles(disp, chk, MAX_SIZE, MAX_DIFF).counts.sum(0).tolist()))
    return out


def dense_with_and_without(n_calls, rounds):
    g = torch.Generator().manual_seed(1234)
    left = torch.randn((1, 3, NET_H, NET_W), generator=g).to(DEV)
    right = torch.randn((1, 3, NET_H, NET_W), generator=g).to(DEV)
    torch.manual_seed(0)
    net = ra.Network(ra.ALL_CONV_GENOTYPE, DEV, maxdisp=MAXDISP).to(DEV).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    variants = {"forward_dense": lambda: net.forward_dense(left, right, 0, net.arch_init, want_error=False),
                "forward_dense_speckle": lambda: net.forward_dense(left, right, 0, net.arch_init, speckle=(MAX_SIZE, MAX_DIFF),
                                                                   want_error=False)}
    t = timed(variants, n_calls, rounds, warmup=2)
    med = {k: v[0] / 1e3 for k, v in t.items()}
    return {"config": f"all-conv Network, eval, one {NET_H}x{NET_W} pair (forward of the stacked 2), D={MAXDISP}, fp32, eager",
            "ms_per_call_median": {k: round(v, 4) for k, v in med.items()},
            "ms_per_call_all": {k: [round(x / 1e3, 4) for x in v[1]] for k, v in t.items()},
            "ratio_speckle_over_plain": round(med["forward_dense_speckle"] / med["forward_dense"], 4),
            "calls_per_round": n_calls, "rounds": rounds}


def kernels_only(iters):
    for name in SHAPES:
        disp, chk = inputs(name)
        for keep in calls(disp, chk).values():
            for _ in range(iters):
                ra.filter_speckles(disp, keep, MAX_SIZE, MAX_DIFF)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces-only", action="store_true", help="skip forward_dense with and without speckle")
    ap.add_argument("--kernels-only", action="store_true", help="only the HIP calls, for a kernel-trace run; prints nothing")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_speckle needs the MI355X"
    if args.kernels_only:
        kernels_only(args.iters)
        return
    out = {"metric": "speckle filter (tile labelling, seam union, flatten, apply, count finalize); forward_dense(speckle=...)", "unit": "us / ms",
           "timing": f"pieces: device events around {args.iters} back-to-back eager calls in each of {args.rounds} rounds, median (after 20 "
                     f"warm-up calls); the ATen twin: {TWIN_CALLS} calls in each of 2 rounds; an eager call includes the host's launch cost "
                     "and its six allocations when the device work is shorter than them; kernel_us: torch.profiler, mean of 20 calls",
           "pieces": {name: pieces(name, args.iters, args.rounds) for name in SHAPES}}
    if not args.pieces_only:
        out["forward_dense"] = dense_with_and_without(args.calls, args.rounds)
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
