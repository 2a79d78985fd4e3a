"""Device-side batch preparation (rag_amd.data.prepare_batch, rag_amd/csrc/prep.hip) at rag_depth's sizes: B = 8 decoded 400x881
stereo pairs with a 16-bit ground truth -> the 480x960 evaluation pad and -> 384x768 training crops, with and without the colour
transfer.  One process; writes one JSON file (default profiles/prep_bench.json) and prints it.  Per case:
  * fused_us      the one HIP launch: device events around replays of a captured graph that holds INNER launches (statistics given);
  * aten_us       the same result from ATen ops on the same GPU (prepare_batch_torch on cuda), device events around eager calls;
  * host route    prepare_batch_torch on the CPU (16 threads) + the fp32 upload, against the uint8 / uint16 upload + the launch
                  (for colour: + color_stats on the device, against the float64 statistics and transfer on the host); host clock
                  around work that ends in a device synchronise, pageable host memory on both sides;
  * GB/s          algorithmic bytes (source bytes inside the window + fp32 bytes written) over fused_us.
Also: color_stats (two launches) per image batch, and the equality of the fused and the ATen result at the timed size.
No time is gated.
    python tools/bench_prep.py [--out FILE] [--replays R] [--inner N]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rag_amd as ra  # noqa: E402
from rag_amd.data import color_stats_torch, prepare_batch_torch  # noqa: E402

DEV = "cuda:0"
B, HS, WS = 8, 400, 881
CASES = {"eval_pad_480x960": dict(out_hw=(480, 960), pad=(80, 79)), "train_crop_384x768": dict(out_hw=(384, 768))}


def image(seed, H, W):
    r = np.random.RandomState(seed)
    blocks = np.kron(r.rand(H // 8 + 1, W // 8 + 1, 3), np.ones((8, 8, 1)))[:H, :W]
    ramp = np.linspace(0, 1, W)[None, :, None] * r.rand(3) + np.linspace(0, 1, H)[:, None, None] * r.rand(3)
    return np.clip((0.5 * blocks + 0.4 * ramp + 0.1 * r.rand(H, W, 3)) * 255 * r.uniform(0.6, 1.1), 0, 255).astype(np.uint8)


def events_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def host_ms(fn, n):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


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


def window_bytes(origin, out_hw, views, gt_bytes):
    H, W = out_hw
    px = 0
    for oy, ox in origin.tolist():
        px += max(0, min(H, HS - oy) - max(0, -oy)) * max(0, min(W, WS - ox) - max(0, -ox))
    return px * (3 * views + gt_bytes), B * H * W * 4 * (3 * views + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prep_bench.json"))
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prep needs the MI355X"
    torch.set_num_threads(16)
    r = np.random.RandomState(0)
    left = torch.from_numpy(np.stack([image(2 * b, HS, WS) for b in range(B)]))
    right = torch.from_numpy(np.stack([image(2 * b + 1, HS, WS) for b in range(B)]))
    real = torch.from_numpy(np.stack([image(100 + b, HS, WS) for b in range(B)]))
    gt = torch.from_numpy(r.randint(0, 65536, (B, HS, WS)).astype(np.uint16))
    dl, dr, dg, dreal = (t.to(DEV) for t in (left, right, gt, real))
    stats_dev = tuple(ra.color_stats(t) for t in (dl, dr, dreal))
    stats_host = tuple(color_stats_torch(t) for t in (left, right, real))
    stats_rel = max(float(((a.cpu() - b).abs() / b.abs()).max()) for a, b in zip(stats_dev, stats_host))

    out = {"metric": f"batch preparation, B={B}, {HS}x{WS} uint8 pairs + uint16 gt", "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "hip": torch.version.hip, "host_threads": torch.get_num_threads(),
           "timing": {"fused_us": f"device events around {args.replays} replays of a captured graph of {args.inner} launches",
                      "aten_us": "device events around 20 eager calls of prepare_batch_torch on cuda (after 3 warm-up calls)",
                      "host_route_ms": "median of 7, host clock around work ending in a device synchronise, pageable memory"},
           "color_stats_rel_err_device_vs_float64_twin": stats_rel, "cases": {}}

    cs = graphed(lambda: ra.color_stats(dl), args.inner)
    cs.replay()
    torch.cuda.synchronize()
    out["color_stats_us_per_image_batch"] = round(events_us(cs.replay, args.replays) / args.inner, 2)

    for name, kw in CASES.items():
        H, W = kw["out_hw"]
        if "pad" in kw:
            origin = torch.tensor([[-kw["pad"][0], 0]] * B, dtype=torch.int32)
        else:
            origin = ra.random_crop_origin(B, (HS, WS), (H, W), generator=torch.Generator().manual_seed(1), device="cpu")
        origin_dev = origin.to(DEV)
        bufs = (torch.empty((B, 3, H, W), device=DEV), torch.empty((B, 3, H, W), device=DEV), torch.empty((B, H, W), device=DEV))
        for color in (False, True):
            sd = stats_dev if color else None
            fused = lambda: ra.prepare_batch(dl, dr, dg, out_hw=(H, W), origin=origin_dev, color=sd, out=bufs)  # noqa: E731
            aten = lambda: prepare_batch_torch(dl, dr, dg, out_hw=(H, W), origin=origin, color=sd)  # noqa: E731
            same = all(torch.equal(a, b) for a, b in zip(fused(), aten()))
            g = graphed(fused, args.inner)
            g.replay()
            torch.cuda.synchronize()
            fused_us = events_us(g.replay, args.replays) / args.inner
            for _ in range(3):
                aten()
            aten_us = events_us(aten, 20)

            def host_route():
                sh = (color_stats_torch(left), color_stats_torch(right), color_stats_torch(real)) if color else None
                return [t.to(DEV) for t in prepare_batch_torch(left, right, gt, out_hw=(H, W), origin=origin, color=sh)]

            def device_route():
                l_, r_, g_ = left.to(DEV), right.to(DEV), gt.to(DEV)
                sdv = (ra.color_stats(l_), ra.color_stats(r_), ra.color_stats(real.to(DEV))) if color else None
                return ra.prepare_batch(l_, r_, g_, out_hw=(H, W), origin=origin_dev, color=sdv, out=bufs)

            rd, wr = window_bytes(origin, (H, W), 2, 2)
            out["cases"][name + ("+color" if color else "")] = {
                "fused_us": round(fused_us, 2), "aten_us": round(aten_us, 1), "aten_over_fused": round(aten_us / fused_us, 1),
                "fused_equals_aten": same, "bytes_read": rd, "bytes_written": wr, "fused_GBps": round((rd + wr) / fused_us / 1e3, 1),
                "hbm_floor_us_at_8TBps": round((rd + wr) / 8e12 * 1e6, 2),
                "host_route_ms": {"cpu_twin_plus_fp32_upload": round(host_ms(host_route, 7), 2),
                                  "u8_upload_plus_kernel": round(host_ms(device_route, 7), 3)},
                "upload_bytes": {"fp32": wr, "u8_u16": B * HS * WS * (3 * 2 + 2) + (B * HS * WS * 3 if color else 0)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
