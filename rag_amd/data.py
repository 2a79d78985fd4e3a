"""Batch preparation on the device: from the decoded bytes of a batch to the network's fp32 inputs in one launch.

The reference prepares every sample on the host (src/dataloaders/data_io.py:6-13, stereo_dataset.py:35-38, 57-121;
src_self/dataloaders/sceneflow_driving_dataset.py:53-70): ``ToTensor`` + ``Normalize``, a random crop (training) or a top / right
zero pad of the NORMALISED image (evaluation), 16-bit disparities ``/ 256``, and in src_self a float64 colour transfer of both views
against a real image; then it uploads fp32.  Here the decoded ``[B,Hs,Ws,3]`` uint8 images (and a uint16 or fp32 ground truth) are
uploaded as they are and `prepare_batch` writes ``[B,3,H,W]`` fp32 (rag_amd/csrc/prep.hip):

  output pixel (y, x) of sample b  =  source pixel (y + origin[b,0], x + origin[b,1]), and 0 where that lies outside the source

so a crop is ``origin = (y1, x1)`` and the evaluation pad is ``origin = (-top_pad, 0)``.  The origins live on the device: a
captured graph replays with new crops.  Image values are bit-identical to the reference's fp32 arithmetic; `*_torch` are the
plain-torch twins (any device): the CPU path and the yardstick of tests/test_prep.py and tools/bench_prep.py.

One loader branch resamples first: src_self/dataloaders/stereo_dataset.py:56-69 halves every Cityscapes sample (2048x1024 ->
1024x512, ``Image.ANTIALIAS`` = Lanczos, views and the 16-bit disparity alike) before the crop or pad, and scales the disparity by
``/ 256 / 2``.  ``prepare_batch(..., **CITYSCAPES_HALF)`` runs that branch in the same single launch
(rag_amd/csrc/prep_resize.hip): Pillow's two-pass arithmetic, bit for bit, on the window of source bytes each output tile needs;
`origin` and `pad` then address the RESIZED image.  `resize_lanczos` is the resize alone, `lanczos_taps` the tables both use.

File decoding (PNG, PFM), list files and DataLoader workers stay with the caller.
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import check, load_library

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
GT_F32, GT_U16 = 0, 1            # RAGMI_GT_* of include/rag_amd.h
# the reference's Cityscapes branch (src_self/dataloaders/stereo_dataset.py:56-69): resize to 1024x512, disparity / 256 / 2
CITYSCAPES_HALF = dict(resize_hw=(512, 1024), gt_scale=1.0 / 512.0)

_NO_CPU = "rag_amd ops run on the MI355X only (got a CPU tensor); there is no CPU fallback"


# --------------------------------------------------------------------------- argument checks shared by the kernel path and the twin
def _check_u8(img, name, like=None):
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
        raise ValueError(f"{name} must be a [B,Hs,Ws,3] uint8 tensor")
    if min(img.shape) < 1:
        raise ValueError(f"{name} is empty")
    if like is not None and img.shape != like.shape:
        raise ValueError(f"{name} must have the shape of left_u8")


def _check_triple(v, name):
    v = tuple(float(x) for x in v)
    if len(v) != 3:
        raise ValueError(f"{name} must hold three floats")
    return v


def _check_hw(hw, name):
    try:
        h, w = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a pair (height, width)") from None
    if h < 1 or w < 1:
        raise ValueError(f"{name} must be positive")
    return h, w


def _resolve(left_u8, right_u8, gt, out_hw, origin, pad, mean, std, color, resize_hw=None, gt_scale_arg=None):
    """Validate everything that does not depend on the device; returns (B, Hs, Ws, H, W, origin, mean, std, gt_scale).  With
    resize_hw, (Hs, Ws) is the RESIZED size: the image that origin and pad address."""
    _check_u8(left_u8, "left_u8")
    if right_u8 is not None:
        _check_u8(right_u8, "right_u8", left_u8)
    B, Hs, Ws, _ = left_u8.shape
    src_hw = (Hs, Ws)
    if resize_hw is not None:
        if color is not None:
            raise ValueError("resize_hw and color= do not combine (no loader of the reference resizes and transfers colour)")
        if gt is not None and isinstance(gt, torch.Tensor) and gt.dtype == torch.float32:
            raise ValueError("resize_hw needs a uint16 gt (the reference resizes 16-bit PNGs only), got float32")
        Hs, Ws = _check_hw(resize_hw, "resize_hw")
    H, W = (int(v) for v in out_hw)
    if H < 1 or W < 1:
        raise ValueError("out_hw must be positive")
    gt_scale = None
    if gt is not None:
        if not isinstance(gt, torch.Tensor) or tuple(gt.shape) != (B, *src_hw):
            raise ValueError("gt must be a [B,Hs,Ws] tensor matching left_u8")
        if gt.dtype == torch.uint16:
            gt_scale = 1.0 / 256.0          # stereo_dataset.py:35-38
        elif gt.dtype == torch.float32:
            gt_scale = 1.0
        else:
            raise ValueError(f"gt must be uint16 (16-bit PNG, scaled by 1/256) or float32 (PFM), got {gt.dtype}")
        if gt_scale_arg is not None:
            gt_scale = float(gt_scale_arg)
    if (origin is None) == (pad is None):
        raise ValueError("give exactly one of origin= and pad=")
    if pad is not None:
        top, right = (int(v) for v in pad)
        if top < 0 or right < 0 or (H, W) != (Hs + top, Ws + right):
            raise ValueError(f"pad={tuple(pad)} on a {Hs}x{Ws} source gives {Hs + top}x{Ws + right}, not out_hw={H}x{W}")
        origin = (-top, 0)
    if isinstance(origin, torch.Tensor):
        if origin.dtype not in (torch.int32, torch.int64) or tuple(origin.shape) != (B, 2):
            raise ValueError("origin must be an int32 / int64 tensor [B,2] of (y, x), or a pair")
    else:
        oy, ox = (int(v) for v in origin)
        origin = torch.tensor([[oy, ox]] * B, dtype=torch.int32)
    if color is not None:
        if len(color) != 3:
            raise ValueError("color must be (stats_left, stats_right, stats_source)")
        for k, s in enumerate(color):
            if s is None and k == 1 and right_u8 is None:
                continue
            if not isinstance(s, torch.Tensor) or s.dtype != torch.float64 or tuple(s.shape) != (B, 3, 2):
                raise ValueError("color statistics must be float64 [B,3,2] tensors (color_stats)")
    return B, Hs, Ws, H, W, origin, _check_triple(mean, "mean"), _check_triple(std, "std"), gt_scale


# --------------------------------------------------------------------------- Lanczos tables (Pillow's precompute_coeffs)
def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


@functools.lru_cache(maxsize=64)
def _lanczos_taps_cached(n: int, m: int):
    if n == m:                          # Pillow skips an axis whose size does not change: the identity, exactly, in both arithmetics
        bounds = torch.stack((torch.arange(m, dtype=torch.int32), torch.ones(m, dtype=torch.int32)), dim=1)
        return bounds, torch.full((m, 1), 1 << 22, dtype=torch.int32), torch.ones((m, 1), dtype=torch.float64)
    scale = n / m
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ss = 1.0 / fs                       # Pillow multiplies by the reciprocal; for a power-of-two scale that is the division
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, kd, ki = [], [], []
    for i in range(m):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        ln = min(n, int(center + support + 0.5)) - xmin
        k = [_lanczos((j + xmin - center + 0.5) * ss) for j in range(ln)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        bounds.append((xmin, ln))
        kd.append(k + [0.0] * (ksize - ln))
        ki.append([int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in k] + [0] * (ksize - ln))
    return (torch.tensor(bounds, dtype=torch.int32), torch.tensor(ki, dtype=torch.int32), torch.tensor(kd, dtype=torch.float64))


def lanczos_taps(n: int, m: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Pillow's Lanczos (``Image.LANCZOS``, once ``ANTIALIAS``) coefficients for resampling an axis of `n` samples to `m`, as CPU
    tensors: bounds int32 ``[m,2]`` = (first source index, tap count) per output index, the 8-bit path's fixed-point taps int32
    ``[m,ksize]`` (``k * 2**22`` rounded half away from zero) and the float64 taps ``[m,ksize]`` of the 16-bit path, both zero past
    the tap count.  Float64 host arithmetic in Pillow's order (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc).
    n == m gives the identity (one tap of 1): Pillow does not filter such an axis.  The tensors are cached: do not modify them."""
    n, m = int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError("lanczos_taps: sizes must be positive")
    return _lanczos_taps_cached(n, m)


_DEVICE_TAPS = {}


def _device_taps(n: int, m: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """lanczos_taps on `device`, uploaded once per (n, m, device): three small copies, outside any graph capture when warmed up."""
    key = (int(n), int(m), str(device))
    t = _DEVICE_TAPS.get(key)
    if t is None:
        t = _DEVICE_TAPS[key] = tuple(x.to(device).contiguous() for x in lanczos_taps(n, m))
    return t


def _check_resize_input(x, name):
    if not isinstance(x, torch.Tensor) or not ((x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3)
                                               or (x.dtype == torch.uint16 and x.dim() == 3)):
        raise ValueError(f"{name} must be a [B,H,W,3] uint8 or a [B,H,W] uint16 tensor")
    if min(x.shape) < 1:
        raise ValueError(f"{name} is empty")


# --------------------------------------------------------------------------- HIP path
def random_crop_origin(B: int, src_hw: Sequence[int], crop_hw: Sequence[int], generator: Optional[torch.Generator] = None,
                       device="cuda") -> torch.Tensor:
    """The reference's crop position (stereo_dataset.py:61-62): x1 uniform in [0, w - crop_w], y1 uniform in [0, h - crop_h], one
    pair per sample, as an int32 ``[B,2]`` tensor of (y1, x1) on `device`.  Drawn on the generator's device (the CPU by default)."""
    (h, w), (ch, cw) = (int(v) for v in src_hw), (int(v) for v in crop_hw)
    if ch > h or cw > w or ch < 1 or cw < 1:
        raise ValueError(f"crop {ch}x{cw} does not fit the {h}x{w} source")
    gdev = generator.device if generator is not None else "cpu"
    x1 = torch.randint(0, w - cw + 1, (B,), generator=generator, device=gdev)
    y1 = torch.randint(0, h - ch + 1, (B,), generator=generator, device=gdev)
    return torch.stack((y1, x1), dim=1).to(device=device, dtype=torch.int32)


def color_stats(img_u8: torch.Tensor) -> torch.Tensor:
    """transfer_color's statistics of ``[B,Hs,Ws,3]`` uint8 images (sceneflow_driving_dataset.py:57-61), float64 ``[B,3,2]``: per
    channel the mean of u/255 and the population std over columns of the per-column population stds (``x.std(0).std(0)``: not
    the image's std).  Two launches, bitwise reproducible, graph-capturable."""
    _check_u8(img_u8, "img_u8")
    if not img_u8.is_cuda:
        raise RuntimeError(_NO_CPU)
    img = img_u8.contiguous()
    B, Hs, Ws, _ = img.shape
    lib = load_library()
    ws = torch.empty((max(1, lib.ragmi_color_stats_workspace_elems(B, Hs, Ws)),), device=img.device, dtype=torch.int64)
    stats = torch.empty((B, 3, 2), device=img.device, dtype=torch.float64)
    check(lib.ragmi_color_stats(img.data_ptr(), B, Hs, Ws, ws.data_ptr(), stats.data_ptr(), ops._stream()), "color_stats")
    return stats


def transfer_color(target_u8: torch.Tensor, source_u8: torch.Tensor) -> torch.Tensor:
    """The reference's ``transfer_color(target, source)`` (sceneflow_driving_dataset.py:53-70) for batches: ``[B,H,W,3]`` uint8
    target against ``[B,Hs,Ws,3]`` uint8 source, sample by sample; returns the uint8 image.  `prepare_batch(color=...)` is the
    fused form that never writes it.  A constant target channel (std 0) divides by zero in the reference and its uint8 cast of
    NaN is undefined: the result for such a channel is unspecified here too (it does not fault)."""
    _check_u8(target_u8, "target_u8")
    _check_u8(source_u8, "source_u8")
    if target_u8.shape[0] != source_u8.shape[0]:
        raise ValueError("target_u8 and source_u8 must hold the same number of samples")
    if not (target_u8.is_cuda and source_u8.is_cuda):
        raise RuntimeError(_NO_CPU)
    st, ss = color_stats(target_u8), color_stats(source_u8)
    tgt = target_u8.contiguous()
    out = torch.empty_like(tgt)
    B, H, W, _ = tgt.shape
    check(load_library().ragmi_color_transfer(tgt.data_ptr(), st.data_ptr(), ss.data_ptr(), out.data_ptr(), B, H, W, ops._stream()),
          "color_transfer")
    return out


def resize_lanczos(x: torch.Tensor, out_hw: Sequence[int]) -> torch.Tensor:
    """``PIL.Image.resize((Wr, Hr), Image.LANCZOS)`` of every image of a batch, bit for bit: ``[B,H,W,3]`` uint8 (mode RGB) or
    ``[B,H,W]`` uint16 (mode I;16) -> the same layout at ``out_hw = (Hr, Wr)``.  One launch; `prepare_batch(resize_hw=...)` is the
    fused form that never writes the resized image.  A size pair whose tile window does not fit the LDS (an extreme
    downscale) raises."""
    _check_resize_input(x, "x")
    Hr, Wr = _check_hw(out_hw, "out_hw")
    if not x.is_cuda:
        raise RuntimeError(_NO_CPU)
    src = x.contiguous()
    B, Hs, Ws = src.shape[:3]
    yb, yki, ykd = _device_taps(Hs, Hr, src.device)
    xb, xki, xkd = _device_taps(Ws, Wr, src.device)
    out = torch.empty((B, Hr, Wr) + tuple(src.shape[3:]), device=src.device, dtype=src.dtype)
    lib = load_library()
    if src.dtype == torch.uint8:
        check(lib.ragmi_resize_lanczos_u8(src.data_ptr(), out.data_ptr(), B, Hs, Ws, Hr, Wr, yb.data_ptr(), yki.data_ptr(), yki.shape[1],
                                          xb.data_ptr(), xki.data_ptr(), xki.shape[1], ops._stream()), "resize_lanczos_u8")
    else:
        check(lib.ragmi_resize_lanczos_u16(src.data_ptr(), out.data_ptr(), B, Hs, Ws, Hr, Wr, yb.data_ptr(), ykd.data_ptr(), ykd.shape[1],
                                           xb.data_ptr(), xkd.data_ptr(), xkd.shape[1], ops._stream()), "resize_lanczos_u16")
    return out


def prepare_batch(left_u8: torch.Tensor, right_u8: Optional[torch.Tensor] = None, gt: Optional[torch.Tensor] = None, *,
                  out_hw: Sequence[int], origin=None, pad: Optional[Sequence[int]] = None, mean: Sequence[float] = IMAGENET_MEAN,
                  std: Sequence[float] = IMAGENET_STD, color=None, out=None, resize_hw: Optional[Sequence[int]] = None,
                  gt_scale: Optional[float] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """``(left, right, gt)`` as the reference's loaders produce them, from decoded bytes, in ONE launch.

    left_u8, right_u8: ``[B,Hs,Ws,3]`` uint8 (HWC); right_u8=None is the depth network's case.  gt: ``[B,Hs,Ws]`` uint16 (a 16-bit
    disparity PNG: scaled by 1/256, exact) or float32 (PFM: copied).  Returns ``[B,3,H,W]`` fp32 images normalised as ToTensor +
    Normalize(mean, std) in fp32, bit for bit, and gt ``[B,H,W]`` fp32; None where not given.

    origin: int tensor ``[B,2]`` of (y, x) per sample (on the device: no copy, and a captured graph replays with new values) or a
    pair for the whole batch.  Output pixel (y, x) reads source pixel (y + origin_y, x + origin_x); outside the source it is 0 in
    images (0 AFTER normalisation, as the reference pads) and gt.  Training crop: ``origin = (y1, x1)`` (`random_crop_origin`).
    pad=(top_pad, right_pad): the evaluation pad, ``origin = (-top_pad, 0)``; out_hw must equal the source size plus the pad.

    color=(stats_left, stats_right, stats_source): `color_stats` of the two views and of the real image, float64 ``[B,3,2]``
    (stats_right=None without a right view): every byte first goes through transfer_color's float64 sequence and its uint8
    truncation; the transferred image is never written.  A constant target channel (std 0) gives an unspecified result, as in the
    reference (division by zero, then an undefined cast), without faulting.

    out=(left, right, gt): write into existing contiguous fp32 tensors (the static inputs of a GraphedTrainStep, the buffers of a
    serving loop); None entries where the input is None.

    resize_hw=(Hr, Wr): first resize views and gt as ``PIL.Image.resize((Wr, Hr), Image.ANTIALIAS)`` does (Lanczos; 8-bit RGB and
    16-bit I;16 arithmetic, bit for bit), still in the one launch: origin, pad and out_hw then address the resized image, which is
    never written.  Needs a uint16 gt and no color=.  ``**CITYSCAPES_HALF`` is the reference's Cityscapes branch
    (src_self/dataloaders/stereo_dataset.py:56-69).  gt_scale: the factor on gt (default 1/256 for uint16, 1 for float32)."""
    src_hw = tuple(left_u8.shape[1:3]) if isinstance(left_u8, torch.Tensor) and left_u8.dim() == 4 else None
    B, Hs, Ws, H, W, origin, mean, std, gt_scale = _resolve(left_u8, right_u8, gt, out_hw, origin, pad, mean, std, color, resize_hw,
                                                            gt_scale)
    dev = left_u8.device
    for t in (left_u8, right_u8, gt) + (tuple(color) if color is not None else ()) + (tuple(out) if out is not None else ()):
        if t is not None and (not t.is_cuda or t.device != dev):
            raise RuntimeError(_NO_CPU if not t.is_cuda else "prepare_batch: tensors on different devices")
    if origin.device != dev or origin.dtype != torch.int32:
        origin = origin.to(device=dev, dtype=torch.int32)        # a pair, or a host tensor: one small copy (not under capture)
    origin = origin.contiguous()
    if out is None:
        out = (torch.empty((B, 3, H, W), device=dev, dtype=torch.float32),
               torch.empty((B, 3, H, W), device=dev, dtype=torch.float32) if right_u8 is not None else None,
               torch.empty((B, H, W), device=dev, dtype=torch.float32) if gt is not None else None)
    else:
        if len(out) != 3:
            raise ValueError("out must be (left, right, gt)")
        for t, src, shape, name in ((out[0], left_u8, (B, 3, H, W), "left"), (out[1], right_u8, (B, 3, H, W), "right"),
                                    (out[2], gt, (B, H, W), "gt")):
            if (t is None) != (src is None):
                raise ValueError(f"out: the {name} entry must be given exactly when its input is")
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f"out: the {name} entry must be a contiguous float32 tensor of shape {shape}")
    lt = left_u8.contiguous()
    rt = right_u8.contiguous() if right_u8 is not None else None
    g = gt.contiguous() if gt is not None else None
    stats = [s.contiguous() if s is not None else None for s in color] if color is not None else [None, None, None]
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    gt_dtype, gt_scale = GT_U16 if (g is not None and g.dtype == torch.uint16) else GT_F32, gt_scale if gt_scale is not None else 1.0
    if resize_hw is not None:
        yb, yki, ykd = _device_taps(src_hw[0], Hs, dev)
        xb, xki, xkd = _device_taps(src_hw[1], Ws, dev)
        check(load_library().ragmi_prep_batch_resized(
            ptr(lt), ptr(rt), ptr(g), gt_dtype, gt_scale, ptr(origin), ptr(out[0]), ptr(out[1]), ptr(out[2]), B, src_hw[0], src_hw[1],
            Hs, Ws, H, W, *mean, *std, ptr(yb), ptr(yki), ptr(ykd), yki.shape[1], ptr(xb), ptr(xki), ptr(xkd), xki.shape[1],
            ops._stream()), "prep_batch_resized")
        return out[0], out[1], out[2]
    check(load_library().ragmi_prep_batch(
        ptr(lt), ptr(rt), ptr(g), gt_dtype, gt_scale, ptr(origin),
        ptr(out[0]), ptr(out[1]), ptr(out[2]), B, Hs, Ws, H, W, *mean, *std, ptr(stats[0]), ptr(stats[1]), ptr(stats[2]),
        ops._stream()), "prep_batch")
    return out[0], out[1], out[2]


# --------------------------------------------------------------------------- plain-torch twins (any device)
def _div(x: torch.Tensor, d) -> torch.Tensor:
    """x / d with d as a 1-element tensor on x's device: a true division on every backend (a Python-scalar divisor is turned into a
    multiplication by its reciprocal on the GPU, which is not the reference's arithmetic)."""
    return x / torch.tensor([d], dtype=x.dtype, device=x.device)


def color_stats_torch(img_u8: torch.Tensor) -> torch.Tensor:
    """Plain-torch restatement of `color_stats` in float64, in numpy's two-pass form (mean, then the mean squared deviation)."""
    _check_u8(img_u8, "img_u8")
    x = _div(img_u8.to(torch.float64), 255.0)                       # [B,H,W,3]

    def pstd(v):                                                    # population std over dim 1
        m = v.mean(dim=1, keepdim=True)
        return ((v - m) ** 2).mean(dim=1).sqrt()

    return torch.stack((x.mean(dim=1).mean(dim=1), pstd(pstd(x))), dim=-1)


def _transfer_with_stats(target_u8, st, ss):
    t = _div(target_u8.to(torch.float64), 255.0)
    tm, ts, sm, sd = (s.view(-1, 1, 1, 3) for s in (st[..., 0], st[..., 1], ss[..., 0], ss[..., 1]))
    t = t - tm
    t = t / (ts / sd)
    t = t + sm
    t = t.clamp(0.0, 1.0)
    return (t * 255.0).to(torch.uint8)                              # truncates, as numpy's astype


def transfer_color_torch(target_u8: torch.Tensor, source_u8: torch.Tensor) -> torch.Tensor:
    """Plain-torch restatement of `transfer_color` (float64, the reference's order of operations)."""
    _check_u8(target_u8, "target_u8")
    _check_u8(source_u8, "source_u8")
    return _transfer_with_stats(target_u8, color_stats_torch(target_u8), color_stats_torch(source_u8))


def _u16_to_f32(gt: torch.Tensor) -> torch.Tensor:
    return (gt.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32)      # uint16 has few kernels of its own


def _resample_axis_torch(v: torch.Tensor, dim: int, m: int, sixteen: bool) -> torch.Tensor:
    """One Pillow resampling pass along `dim`: v holds pixel values as int32 (8-bit) or float64 (16-bit); returns the same."""
    n = v.shape[dim]
    if n == m:
        return v                                                    # Pillow skips the pass
    bounds, ki, kd = (t.to(v.device) for t in lanczos_taps(n, m))
    xmin = bounds[:, 0].to(torch.int64)
    shape = [1] * v.dim()
    shape[dim] = m
    if sixteen:
        acc = torch.zeros(v.shape[:dim] + (m,) + v.shape[dim + 1:], dtype=torch.float64, device=v.device)
        for j in range(kd.shape[1]):                                # ascending j; product and sum rounded separately; px * 0.0 past the count
            acc = acc + v.index_select(dim, (xmin + j).clamp(max=n - 1)) * kd[:, j].view(shape)
        r = torch.where(acc < 0, acc - 0.5, acc + 0.5).to(torch.int64)      # the cast truncates toward zero
        lo, hi = torch.fmod(r, 256).clamp(0, 255), (r >> 8).clamp(0, 255)   # the two bytes are clipped separately (C remainder sign)
        return (hi * 256 + lo).to(torch.float64)
    acc = torch.full(v.shape[:dim] + (m,) + v.shape[dim + 1:], 1 << 21, dtype=torch.int32, device=v.device)
    for j in range(ki.shape[1]):
        acc = acc + v.index_select(dim, (xmin + j).clamp(max=n - 1)) * ki[:, j].view(shape)
    return (acc >> 22).clamp(0, 255)                                # arithmetic shift


def resize_lanczos_torch(x: torch.Tensor, out_hw: Sequence[int]) -> torch.Tensor:
    """Plain-torch restatement of `resize_lanczos` on the device of `x`: Pillow's arithmetic in integer / float64 tensor
    operations, the horizontal pass first and stored (uint8 / uint16) before the vertical one.  Written to be that arithmetic,
    not to be fast."""
    _check_resize_input(x, "x")
    Hr, Wr = _check_hw(out_hw, "out_hw")
    if x.dtype == torch.uint8:
        return _resample_axis_torch(_resample_axis_torch(x.to(torch.int32), 2, Wr, False), 1, Hr, False).to(torch.uint8)
    v = (x.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float64)
    v = _resample_axis_torch(_resample_axis_torch(v, 2, Wr, True), 1, Hr, True)
    return v.to(torch.int32).to(torch.int16).view(torch.uint16)     # 0..65535 -> the same 16 bits


def prepare_batch_torch(left_u8, right_u8=None, gt=None, *, out_hw, origin=None, pad=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                        color=None, resize_hw=None, gt_scale=None):
    """Plain-torch restatement of `prepare_batch` on the device of its inputs: (with resize_hw, `resize_lanczos_torch` first, then)
    normalise the whole source as the reference does (``.to(float32).div(255)``, ``sub(mean).div(std)``), then copy the window
    that `origin` selects into zeros."""
    B, Hs, Ws, H, W, origin, mean, std, gt_scale = _resolve(left_u8, right_u8, gt, out_hw, origin, pad, mean, std, color, resize_hw,
                                                            gt_scale)
    if resize_hw is not None:
        left_u8, right_u8, gt = (resize_lanczos_torch(t, (Hs, Ws)) if t is not None else None for t in (left_u8, right_u8, gt))
    dev = left_u8.device
    org = origin.tolist()
    m = torch.tensor(mean, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=dev).view(1, 3, 1, 1)

    def place(src, shape):                                          # src [B,...,Hs,Ws] -> zeros [B,...,H,W] with the window copied
        dst = torch.zeros(shape, dtype=torch.float32, device=dev)
        for b, (oy, ox) in enumerate(org):
            y0, y1 = max(0, -oy), min(H, Hs - oy)
            x0, x1 = max(0, -ox), min(W, Ws - ox)
            if y1 > y0 and x1 > x0:
                dst[b, ..., y0:y1, x0:x1] = src[b, ..., y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        return dst

    def image(u8, k):
        if u8 is None:
            return None
        if color is not None:
            u8 = _transfer_with_stats(u8, color[k], color[2])
        v = _div(u8.permute(0, 3, 1, 2).to(torch.float32), 255.0)   # ToTensor
        return place((v - m) / s, (B, 3, H, W))                     # Normalize, then crop / pad

    g = None
    if gt is not None:
        g = place((_u16_to_f32(gt) if gt.dtype == torch.uint16 else gt) * gt_scale, (B, H, W))
    return image(left_u8, 0), image(right_u8, 1), g
