"""The Cityscapes half-resolution branch of batch preparation (rag_amd.data.prepare_batch(**CITYSCAPES_HALF),
rag_amd/csrc/prep_resize.hip) at the reference's sizes: B = 4 and B = 8 decoded 1024x2048 stereo pairs with a 16-bit disparity ->
Lanczos to 512x1024 -> the 192x384 training crop and -> the 576x1248 evaluation pad.  One process; writes one JSON file (default
profiles/prep_resize_bench.json) and prints it.  Per case:
  * fused_us      the one HIP launch: device events around replays of a captured graph that holds INNER launches;
  * aten_us       the same result from ATen ops on the same GPU (prepare_batch_torch on cuda: the whole image is resized, as
                  Pillow does), device events around eager calls;
  * pillow route  where Pillow is importable: Image.resize(..., LANCZOS) of the three images of every sample on the CPU, 16 threads
                  over the samples (Pillow releases the GIL), then the crop / pad / normalise twin on the CPU and the fp32 upload;
                  host clock around work that ends in a device synchronise, against the uint8 / uint16 upload + the launch;
  * GB/s          algorithmic bytes (the source bytes under the filter footprint of the window + fp32 bytes written) over fused_us.
Also the equality of the fused and the ATen result at the timed size.  No time is gated; the yardsticks are the twin and Pillow.
    python tools/bench_prep_resize.py [--out FILE] [--replays R] [--inner N]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rag_amd as ra  # noqa: E402
from rag_amd.data import CITYSCAPES_HALF, lanczos_taps, prepare_batch_torch  # noqa: E402

DEV = "cuda:0"
HS, WS = 1024, 2048
HR, WR = CITYSCAPES_HALF["resize_hw"]
CASES = {"train_crop_192x384": dict(out_hw=(192, 384)), "eval_pad_576x1248": dict(out_hw=(576, 1248), pad=(576 - HR, 1248 - WR))}
THREADS = 16


def image(seed, H, W):
    r = np.random.RandomState(seed)
    blocks = np.kron(r.rand(H // 8 + 1, W // 8 + 1, 3), np.ones((8, 8, 1)))[:H, :W]
    ramp = np.linspace(0, 1, W)[None, :, None] * r.rand(3) + np.linspace(0, 1, H)[:, None, None] * r.rand(3)
    return np.clip((0.5 * blocks + 0.4 * ramp + 0.1 * r.rand(H, W, 3)) * 255 * r.uniform(0.6, 1.1), 0, 255).astype(np.uint8)


def disparity(seed, H, W):
    r = np.random.RandomState(seed)
    blocks = np.kron(r.rand(H // 8 + 1, W // 8 + 1), np.ones((8, 8)))[:H, :W]
    d = 60.0 * blocks + 40.0 * np.linspace(0, 1, W)[None, :]
    d[blocks < 0.15] = 0.0
    return np.round(d * 256).astype(np.uint16)


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


def window_bytes(origin, out_hw, B):
    """(source bytes under the Lanczos footprint of each sample's window: 2 views x 3 bytes + 2 bytes of gt per pixel, fp32 written)."""
    H, W = out_hw
    (yb, _, _), (xb, _, _) = lanczos_taps(HS, HR), lanczos_taps(WS, WR)
    px = 0
    for oy, ox in origin.tolist():
        y0, y1, x0, x1 = max(0, oy), min(HR, oy + H), max(0, ox), min(WR, ox + W)
        if y1 > y0 and x1 > x0:
            px += int(yb[y1 - 1].sum() - yb[y0, 0]) * int(xb[x1 - 1].sum() - xb[x0, 0])
    return px * (3 * 2 + 2), B * H * W * 4 * (3 * 2 + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prep_resize_bench.json"))
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prep_resize needs the MI355X"
    torch.set_num_threads(THREADS)
    try:
        from PIL import Image
        import PIL
        pillow = PIL.__version__
    except ImportError:
        Image, pillow = None, None

    out = {"metric": f"Cityscapes half-resolution batch preparation, {HS}x{WS} uint8 pairs + uint16 gt -> Lanczos {HR}x{WR} -> crop / pad",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip, "pillow": pillow,
           "host_threads": THREADS,
           "timing": {"fused_us": f"device events around {args.replays} replays of a captured graph of {args.inner} launches",
                      "aten_us": "device events around 5 eager calls of prepare_batch_torch on cuda (after 2 warm-up calls)",
                      "host_route_ms": "median of 5, host clock around work ending in a device synchronise, pageable memory"},
           "cases": {}}

    for B in (4, 8):
        left = torch.from_numpy(np.stack([image(2 * b, HS, WS) for b in range(B)]))
        right = torch.from_numpy(np.stack([image(2 * b + 1, HS, WS) for b in range(B)]))
        gt = torch.from_numpy(np.stack([disparity(50 + b, HS, WS) for b in range(B)]))
        dl, dr, dg = (t.to(DEV) for t in (left, right, gt))
        for name, kw in CASES.items():
            H, W = kw["out_hw"]
            if "pad" in kw:
                origin = torch.tensor([[-kw["pad"][0], 0]] * B, dtype=torch.int32)
            else:
                origin = ra.random_crop_origin(B, (HR, WR), (H, W), generator=torch.Generator().manual_seed(1), device="cpu")
            origin_dev = origin.to(DEV)
            bufs = (torch.empty((B, 3, H, W), device=DEV), torch.empty((B, 3, H, W), device=DEV), torch.empty((B, H, W), device=DEV))
            fused = lambda: ra.prepare_batch(dl, dr, dg, out_hw=(H, W), origin=origin_dev, out=bufs, **CITYSCAPES_HALF)  # noqa: E731
            aten = lambda: prepare_batch_torch(dl, dr, dg, out_hw=(H, W), origin=origin, **CITYSCAPES_HALF)  # noqa: E731
            same = all(torch.equal(a, b) for a, b in zip(fused(), aten()))
            g = graphed(fused, args.inner)
            g.replay()
            torch.cuda.synchronize()
            fused_us = events_us(g.replay, args.replays) / args.inner
            aten()
            aten_us = events_us(aten, 5)

            def device_route():
                return ra.prepare_batch(left.to(DEV), right.to(DEV), gt.to(DEV), out_hw=(H, W), origin=origin_dev, out=bufs, **CITYSCAPES_HALF)

            rd, wr = window_bytes(origin, (H, W), B)
            case = {"fused_us": round(fused_us, 2), "aten_us": round(aten_us, 1), "aten_over_fused": round(aten_us / fused_us, 1),
                    "fused_equals_aten": same, "bytes_read": rd, "bytes_written": wr, "fused_GBps": round((rd + wr) / fused_us / 1e3, 1),
                    "hbm_floor_us_at_8TBps": round((rd + wr) / 8e12 * 1e6, 2),
                    "host_route_ms": {"u8_upload_plus_kernel": round(host_ms(device_route, 5), 3)},
                    "upload_bytes": {"fp32": wr, "u8_u16": B * HS * WS * (3 * 2 + 2)}}
            if Image is not None:
                ln, rn, gn = left.numpy(), right.numpy(), gt.numpy()

                def resize_sample(b):
                    return tuple(np.array(Image.fromarray(a[b]).resize((WR, HR), Image.LANCZOS)) for a in (ln, rn, gn))

                def pillow_resize():
                    with ThreadPoolExecutor(THREADS) as ex:
                        parts = list(ex.map(resize_sample, range(B)))
                    return [torch.from_numpy(np.stack([p[k] for p in parts])) for k in range(3)]

                def pillow_route():
                    small = pillow_resize()
                    return [t.to(DEV) for t in prepare_batch_torch(*small, out_hw=(H, W), origin=origin, gt_scale=CITYSCAPES_HALF["gt_scale"])]

                ref = pillow_route()
                case["fused_equals_pillow_route"] = all(torch.equal(a, b) for a, b in zip(fused(), ref))
                t0 = time.perf_counter()
                pillow_resize()
                case["host_route_ms"]["pillow_resize_only"] = round((time.perf_counter() - t0) * 1e3, 2)
                case["host_route_ms"]["pillow_plus_cpu_twin_plus_fp32_upload"] = round(host_ms(pillow_route, 5), 2)
            out["cases"][f"B{B}_{name}"] = case
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
