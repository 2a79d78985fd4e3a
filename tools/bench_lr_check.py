"""The occlusion-aware self-supervised step's pieces, one JSON line on stdout (also written to --out):
  * at the training crop (B = 4, 192x384, stacked 8) and at one 384x1248 pair (stacked 2), on the same build: the left-right check
    launch (rag_amd.metrics.lr_consistency on the stacked disparities), the stack-and-mirror launch (lr_stack) and the weighted loss
    forward + backward (re_and_sm_loss(..., weight=)), each against its ATen twin (lr_consistency_torch, torch.cat / flip,
    re_and_sm_loss_torch(..., weight=)) and the weighted loss against the UNWEIGHTED kernel: us per call from device events around
    back-to-back calls, and launches per call counted by torch.profiler;
  * the whole graphed step: occlusion=True at B against the plain supervise=False step at the same 2B batch and at B, timed
    alternately in one process (ms per step, device events).
    python tools/bench_lr_check.py [--pieces-only] [--iters N] [--steps K] [--rounds R] [--out PATH]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rag_amd as ra  # noqa: E402

SHAPES = {"crop_B4_192x384": (4, 3, 192, 384), "pair_B1_384x1248": (1, 3, 384, 1248)}
STEP_B, STEP_H, STEP_W, MAXDISP = 4, 192, 384, 192
DEV = "cuda:0"


def timed(variants, iters, rounds):
    """{name: (median us per call, [us per call of each round])}: device events around `iters` back-to-back calls, the variants taken
    in turn in each of `rounds` rounds (shared-host noise hits all of them), after 20 warm-up calls of each."""
    for fn in variants.values():
        for _ in range(20):
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


def pieces(name, iters, rounds):
    B, C, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(0)
    left = torch.randn((B, C, H, W), generator=g).to(DEV)
    right = torch.randn((B, C, H, W), generator=g).to(DEV)
    # stacked disparities: one level per pair (the same in both of its views) plus noise of the size of the tolerance, so that all of
    # the check's branches are taken: consistent, inconsistent, and out of view at the rows' ends
    level = (torch.rand((B, 1, 1), generator=g) * 40 + 8).repeat(2, 1, 1)
    disp = (level + torch.rand((2 * B, H, W), generator=g) * 1.5).to(DEV)
    left2, right2 = ra.lr_stack(left, right)
    chk = ra.lr_consistency(disp, disp, mirrored=True, partner_shift=B)
    weight = chk.weight
    d = disp.clone().requires_grad_(True)

    def loss_call(fn):
        def run():
            d.grad = None
            fn().backward()
        return run
    calls = {
        "check": dict(hip=lambda: ra.lr_consistency(disp, disp, mirrored=True, partner_shift=B),
                      aten=lambda: ra.lr_consistency_torch(disp, disp, mirrored=True, partner_shift=B)),
        "check_no_error": dict(hip=lambda: ra.lr_consistency(disp, disp, mirrored=True, partner_shift=B, want_error=False),
                               aten=lambda: ra.lr_consistency_torch(disp, disp, mirrored=True, partner_shift=B, want_error=False)),
        "stack": dict(hip=lambda: ra.lr_stack(left, right),
                      aten=lambda: (torch.cat((left, right.flip(-1))), torch.cat((right, left.flip(-1))))),
        "weighted_loss_fwd_bwd": dict(hip=loss_call(lambda: ra.re_and_sm_loss(d, left2, right2, weight)),
                                      aten=loss_call(lambda: ra.re_and_sm_loss_torch(d, left2, right2, weight)[0]),
                                      unweighted_hip=loss_call(lambda: ra.re_and_sm_loss(d, left2, right2))),
    }
    out = {"shape": {"B": B, "stacked": 2 * B, "C": C, "H": H, "W": W}, "valid_share": round(float(chk.valid.mean()), 4)}
    for key, variants in calls.items():
        t = timed(variants, iters, rounds)
        out[key] = {"us_median": {k: round(v[0], 2) for k, v in t.items()}, "us_all": {k: v[1] for k, v in t.items()},
                    "aten_over_hip": round(t["aten"][0] / t["hip"][0], 2), "launches": {k: launches(fn) for k, fn in variants.items()}}
    wl = out["weighted_loss_fwd_bwd"]
    wl["weighted_over_unweighted"] = round(wl["us_median"]["hip"] / wl["us_median"]["unweighted_hip"], 3)
    npx = 2 * B * H * W
    out["algorithmic_bytes"] = {"check": 16 * npx, "stack": 12 * C * npx, "weighted_loss": npx * (8 * C + 12)}
    out["hbm_floor_us_at_8TBps"] = {k: round(v / 8e12 * 1e6, 2) for k, v in out["algorithmic_bytes"].items()}
    with torch.no_grad():
        out["loss_value"] = {"hip": float(ra.metrics.self_supervised_terms(disp, left2, right2, weight)[0]),
                             "aten_fp32": float(ra.re_and_sm_loss_torch(disp, left2, right2, weight)[0])}
    return out


def graphed_steps(steps, rounds):
    from rag_amd.train import GradBucket, GraphedTrainStep, make_optimizer
    g = torch.Generator().manual_seed(1234)
    left = torch.randn((STEP_B, 3, STEP_H, STEP_W), generator=g).to(DEV)
    right = torch.randn((STEP_B, 3, STEP_H, STEP_W), generator=g).to(DEV)
    left2, right2 = ra.lr_stack(left, right)
    configs = {"occlusion_B": (left, right, True), "plain_2B": (left2, right2, False), "plain_B": (left, right, False)}
    runs = {}
    for key, (lt, rt, occlusion) in configs.items():
        torch.manual_seed(0)
        net = ra.Network(ra.ALL_CONV_GENOTYPE, DEV, maxdisp=MAXDISP).to(DEV).train()
        bucket = GradBucket(net.parameters())
        opt = make_optimizer(net.parameters(), bucket=bucket)
        step = GraphedTrainStep(net, opt, bucket, lt, rt, None, clip=5.0, supervise=False, occlusion=occlusion)
        runs[key] = (step, step.node_census)
    times = {k: [] for k in runs}
    for step, _ in runs.values():                    # warm-up replays
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    for _ in range(rounds):                          # alternate the configurations: shared-host noise hits all of them
        for k, (step, _) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return {"config": f"GraphedTrainStep(supervise=False), all-conv Network, B={STEP_B}, {STEP_H}x{STEP_W}, D={MAXDISP}, fp32, FlatSGD",
            "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
            "ms_per_step_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
            "ratio_occlusion_over_plain_2B": round(med["occlusion_B"] / med["plain_2B"], 4),
            "ratio_occlusion_over_plain_B": round(med["occlusion_B"] / med["plain_B"], 4),
            "graph_nodes": {k: c for k, (_, c) in runs.items()}, "steps_per_round": steps, "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces-only", action="store_true", help="skip the graphed training steps")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lr_check needs the MI355X"
    out = {"metric": "left-right check, stack launch and weighted self-supervised loss; occlusion-aware graphed step", "unit": "us / ms",
           "timing": f"pieces: device events around {args.iters} back-to-back eager calls, variants in turn in each of {args.rounds} rounds, "
                     "median (after 20 warm-up calls each); an eager call includes the host's launch cost when the device work is "
                     "shorter than it",
           "pieces": {name: pieces(name, args.iters, args.rounds) for name in SHAPES}}
    if not args.pieces_only:
        out["graphed_step"] = graphed_steps(args.steps, args.rounds)
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
