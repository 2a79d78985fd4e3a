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

File decoding (PNG, PFM), list files and DataLoader workers stay with the caller.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import check, load_library

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
GT_F32, GT_U16 = 0, 1            # RAGMI_GT_* of include/rag_amd.h

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


def _resolve(left_u8, right_u8, gt, out_hw, origin, pad, mean, std, color):
    """Validate everything that does not depend on the device; returns (B, Hs, Ws, H, W, origin, mean, std, gt_scale)."""
    _check_u8(left_u8, "left_u8")
    if right_u8 is not None:
        _check_u8(right_u8, "right_u8", left_u8)
    B, Hs, Ws, _ = left_u8.shape
    H, W = (int(v) for v in out_hw)
    if H < 1 or W < 1:
        raise ValueError("out_hw must be positive")
    gt_scale = None
    if gt is not None:
        if not isinstance(gt, torch.Tensor) or tuple(gt.shape) != (B, Hs, Ws):
            raise ValueError("gt must be a [B,Hs,Ws] tensor matching left_u8")
        if gt.dtype == torch.uint16:
            gt_scale = 1.0 / 256.0          # stereo_dataset.py:35-38
        elif gt.dtype == torch.float32:
            gt_scale = 1.0
        else:
            raise ValueError(f"gt must be uint16 (16-bit PNG, scaled by 1/256) or float32 (PFM), got {gt.dtype}")
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


def prepare_batch(left_u8: torch.Tensor, right_u8: Optional[torch.Tensor] = None, gt: Optional[torch.Tensor] = None, *,
                  out_hw: Sequence[int], origin=None, pad: Optional[Sequence[int]] = None, mean: Sequence[float] = IMAGENET_MEAN,
                  std: Sequence[float] = IMAGENET_STD, color=None, out=None) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
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
    serving loop); None entries where the input is None."""
    B, Hs, Ws, H, W, origin, mean, std, gt_scale = _resolve(left_u8, right_u8, gt, out_hw, origin, pad, mean, std, color)
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
    check(load_library().ragmi_prep_batch(
        ptr(lt), ptr(rt), ptr(g), GT_U16 if (g is not None and g.dtype == torch.uint16) else GT_F32, gt_scale or 1.0, ptr(origin),
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


def prepare_batch_torch(left_u8, right_u8=None, gt=None, *, out_hw, origin=None, pad=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                        color=None):
    """Plain-torch restatement of `prepare_batch` on the device of its inputs: normalise the whole source as the reference does
    (``.to(float32).div(255)``, ``sub(mean).div(std)``), then copy the window that `origin` selects into zeros."""
    B, Hs, Ws, H, W, origin, mean, std, gt_scale = _resolve(left_u8, right_u8, gt, out_hw, origin, pad, mean, std, color)
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
