"""Loss and evaluation metrics of the stereo loops, fused on the device.

The reference computes, per batch, a masked smooth-L1 loss and five metrics with six boolean gathers and six
`.item()` synchronisations (approaches/rag.py:418-430, utilstool/metrics.py:21-65).  Here one kernel pass accumulates
everything per image, a second tiny kernel applies the reference's per-image rules, and the eight results stay in
one device tensor: a caller that wants Python floats pays ONE device-to-host copy (`StereoMetrics.floats()`), and the
training loss never leaves the device.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from ._lib import check, load_library

NAMES = ("loss", "EPE", "D1", "Thres1", "Thres2", "Thres3")


class EpochMeter:
    """The `AverageMeterDict` of one epoch (utilstool/experiment.py:126-151) on the device.  The reference feeds it with six
    `.item()` synchronisations per batch (rag.py:386-396, 457-466); here the finalize kernel of the loss / metrics launch adds the
    batch's floats to `sums` (ragmi_stereo_metrics_meter_fwd: no extra launch, nothing leaves the device) and `mean()` is the
    epoch's one device-to-host copy.

    `sums`: float64 [8] - running sums of loss, EPE, D1, Thres1, Thres2, Thres3 (each batch's float added in double, as the
    reference adds Python floats), the number of batches, the images kept.  `last`: the most recent batch's 8-float vector (the
    kernel's `out` itself, not a copy; None before the first batch)."""

    def __init__(self, device):
        self.sums = torch.zeros((8,), device=device, dtype=torch.float64)
        self.last = None

    def reset(self) -> None:
        self.sums.zero_()
        self.last = None

    def mean(self) -> Dict[str, float]:
        """AverageMeterDict.mean(): NAMES -> sums[k] / sums[6] as Python floats (nan before the first batch)."""
        vals = self.sums.tolist()          # the only synchronisation
        n = vals[6]
        return {k: (v / n if n else float("nan")) for k, v in zip(NAMES, vals[:6])}


def _raw(disp_est: torch.Tensor, disp_gt: torch.Tensor, maxdisp: float, meter: Optional[EpochMeter] = None) -> torch.Tensor:
    ops._need_gpu(disp_est, disp_gt)
    if disp_est.shape != disp_gt.shape or disp_est.dim() != 3:
        raise ValueError("stereo metrics: disp_est and disp_gt must both be [B, H, W]")   # metrics.py:14-18
    est, gt = disp_est.contiguous(), disp_gt.contiguous()
    B, H, W = est.shape
    buf = torch.empty((B + 1, 8), device=est.device, dtype=torch.float32)
    out = buf[B]
    if meter is None:
        check(load_library().ragmi_stereo_metrics_fwd(est.data_ptr(), gt.data_ptr(), B, H, W, float(maxdisp), buf.data_ptr(),
                                                      out.data_ptr(), ops._stream()), "stereo_metrics")
        return out
    if not isinstance(meter, EpochMeter) or meter.sums.device != est.device:
        raise ValueError("stereo metrics: meter must be a rag_amd.metrics.EpochMeter on the device of disp_est")
    check(load_library().ragmi_stereo_metrics_meter_fwd(est.data_ptr(), gt.data_ptr(), B, H, W, float(maxdisp), buf.data_ptr(),
                                                        out.data_ptr(), meter.sums.data_ptr(), ops._stream()), "stereo_metrics_meter")
    meter.last = out
    return out


class StereoMetrics:
    """Result of `stereo_metrics`: `.tensor` is the 8-float device vector (loss, EPE, D1, Thres1, Thres2, Thres3,
    masked pixel count, images kept); `[name]` gives a 0-d device tensor; `floats()` copies once to the host."""

    def __init__(self, tensor: torch.Tensor):
        self.tensor = tensor

    def __getitem__(self, name: str) -> torch.Tensor:
        return self.tensor[NAMES.index(name)]

    def floats(self) -> Dict[str, float]:
        vals = self.tensor.tolist()        # the only synchronisation
        return dict(zip(NAMES, vals[:6]))


def stereo_metrics(disp_est: torch.Tensor, disp_gt: torch.Tensor, maxdisp: float = 192, meter: Optional[EpochMeter] = None) -> StereoMetrics:
    """loss, EPE, D1, Thres1/2/3 of Appr.eval (rag.py:418-430) for disp_est, disp_gt [B,H,W]; no gradient.  `meter`: the same launch
    also adds the batch to that EpochMeter."""
    with torch.no_grad():
        return StereoMetrics(_raw(disp_est.detach(), disp_gt, maxdisp, meter))


# --------------------------------------------------------------------------- per-pixel statistics of the disparity distribution
STAT_NAMES = ("variance", "peak", "entropy")


class DispStats:
    """Result of a `forward_stats` call: `.disp` [B,H,W] is the disparity (the bits of the plain forward), `.tensor` [B,3,H,W] the
    statistics of the softmin distribution it is the mean of; `.variance` (px^2), `.peak` (max_k p_k) and `.entropy` (nats) are
    views of its planes.  Everything stays on the device."""

    def __init__(self, disp: torch.Tensor, tensor: torch.Tensor):
        self.disp = disp
        self.tensor = tensor

    def __getitem__(self, name: str) -> torch.Tensor:
        return self.tensor[:, STAT_NAMES.index(name)]

    @property
    def variance(self) -> torch.Tensor:
        return self.tensor[:, 0]

    @property
    def peak(self) -> torch.Tensor:
        return self.tensor[:, 1]

    @property
    def entropy(self) -> torch.Tensor:
        return self.tensor[:, 2]

    def _uncertainty(self, which: str) -> torch.Tensor:
        if which == "variance":
            return self.variance
        if which == "entropy":
            return self.entropy
        if which == "one_minus_peak":
            return 1.0 - self.peak
        if which == "one_minus_mode_mass":
            raise ValueError("sparsification: which='one_minus_mode_mass' needs a DispMode (a forward_mode result); this is a DispStats")
        raise ValueError(f"sparsification: which must be one of {SPARSIFY_WHICH}, got {which!r}")

    def sparsification(self, gt: torch.Tensor, which: str = "variance", meter: Optional["CalibrationMeter"] = None,
                       maxdisp: float = 192, fractions: int = 20) -> "Sparsification":
        """Sparsification curves of `.disp` against gt [B,H,W] with one of the head's own statistics as the uncertainty: `which` in
        "variance", "entropy", "one_minus_peak", and on a DispMode "one_minus_mode_mass".  See `sparsification`."""
        return sparsification(self.disp, self._uncertainty(which), gt, maxdisp, fractions, meter)


def refuse_autograd(what: str, *ts) -> None:
    """The statistics launches have no backward: refuse an input that autograd would track."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(f"rag_amd {what}: inference only (the statistics have no backward and the call would drop the input's "
                           "autograd graph); call it under torch.no_grad() or on detached inputs")


def prob_stats_torch(prob: torch.Tensor):
    """(disp [B,H,W], stats [B,3,H,W]) of a distribution prob[B,D,H,W] over the disparity axis, taken as given, in prob's dtype and
    on its device: disp = sum p k, variance = sum p (k - disp)^2 (the centred second moment), peak = max p, entropy = -sum p ln p
    with terms of p <= 0 contributing 0."""
    k = torch.arange(prob.shape[1], dtype=prob.dtype, device=prob.device).view(1, -1, 1, 1)
    disp = (prob * k).sum(1)
    var = (prob * (k - disp[:, None]) ** 2).sum(1)
    pos = prob > 0
    ent = -(torch.where(pos, prob, torch.ones_like(prob)).log() * prob * pos).sum(1)
    return disp, torch.stack((var, prob.max(1).values, ent), dim=1)


def disp_stats_torch(cost: torch.Tensor, maxdisp: int, size=None):
    """Plain-torch twin of ops.disp_softargmin_stats in cost's dtype and on its device (the CPU path, and the float64 / ATen yardstick
    of the tests and tools/bench_disp_stats.py): cost [B,1,d,h,w] or [B,d,h,w] -> F.interpolate to (maxdisp, *size) (trilinear,
    align_corners=False; size defaults to (3h, 3w)) -> softmin over the disparity axis -> prob_stats_torch.  Returns (disp, stats)."""
    import torch.nn.functional as F
    if cost.dim() == 4:
        cost = cost[:, None]
    Ho, Wo = (3 * cost.shape[3], 3 * cost.shape[4]) if size is None else size
    v = F.interpolate(cost, (int(maxdisp), int(Ho), int(Wo)), mode="trilinear", align_corners=False)[:, 0]
    return prob_stats_torch(F.softmin(v, dim=1))


# --------------------------------------------------------------------------- mode-local disparity and the mass of its window
MODE_NAMES = ("index", "disp", "mass")
# The default window radius of forward_mode, in fine-disparity pixels: one coarse plane of the x3 head (3 fine px) plus one, so the window
# always holds the mode's own coarse cell and a sample beyond it on each side.  A parameter like VAR_FLOOR, not a measurement.
MODE_RADIUS = 4


class DispMode(DispStats):
    """Result of a `forward_mode` call: a DispStats (`.disp`, `.tensor` and its views: the bits of `forward_stats`) plus `.mode_tensor`
    [B,3,H,W] with the views `.mode_index` (k*, the fine index of the smallest upsampled cost, integer-valued fp32), `.mode_disp` (the
    disparity regressed over |k - k*| <= `.radius` about k*: it stays on one surface where `.disp` averages two) and `.mode_mass` (the
    probability that window holds).  Everything stays on the device."""

    def __init__(self, disp: torch.Tensor, tensor: torch.Tensor, mode_tensor: torch.Tensor, radius: int):
        super().__init__(disp, tensor)
        self.mode_tensor = mode_tensor
        self.radius = int(radius)

    def __getitem__(self, name: str) -> torch.Tensor:
        if name in MODE_NAMES:
            return self.mode_tensor[:, MODE_NAMES.index(name)]
        return super().__getitem__(name)

    @property
    def mode_index(self) -> torch.Tensor:
        return self.mode_tensor[:, 0]

    @property
    def mode_disp(self) -> torch.Tensor:
        return self.mode_tensor[:, 1]

    @property
    def mode_mass(self) -> torch.Tensor:
        return self.mode_tensor[:, 2]

    def _uncertainty(self, which: str) -> torch.Tensor:
        if which == "one_minus_mode_mass":
            return 1.0 - self.mode_mass
        return super()._uncertainty(which)


def _window_torch(p: torch.Tensor, radius: int, index: torch.Tensor) -> torch.Tensor:
    """mode [B,3,H,W] = (k*, k* + sum_W p (k - k*) / sum_W p, sum_W p) of p[B,D,H,W] over W = {k : |k - k*| <= radius} about index = k*
    [B,H,W]; the window is clipped at both ends and a window without mass gives k*."""
    if int(radius) != radius or not 0 <= int(radius) <= p.shape[1]:
        raise ValueError(f"rag_amd mode twin: radius must be an integer in [0, {p.shape[1]}], got {radius!r}")
    ks = index.to(device=p.device, dtype=p.dtype)[:, None]
    t = torch.arange(p.shape[1], dtype=p.dtype, device=p.device).view(1, -1, 1, 1) - ks
    pw = p * (t.abs() <= int(radius))
    mass = pw.sum(1)
    m1 = (pw * t).sum(1)
    safe = torch.where(mass != 0, mass, torch.ones_like(mass))
    return torch.stack((ks[:, 0], ks[:, 0] + torch.where(mass != 0, m1 / safe, torch.zeros_like(m1)), mass), dim=1)


def _first_index(x: torch.Tensor, extreme: torch.Tensor) -> torch.Tensor:
    """The lowest index along dim 1 at which x equals its extreme [B,1,H,W], formed explicitly (argmax's tie order is not a contract)."""
    idx = torch.arange(x.shape[1], device=x.device).view(1, -1, 1, 1)
    return torch.where(x == extreme, idx, torch.full_like(idx, x.shape[1])).amin(1)


def prob_mode_torch(prob: torch.Tensor, radius: int, index=None):
    """(disp, stats, mode) of a distribution prob[B,D,H,W] taken as given, in prob's dtype and on its device: prob_stats_torch plus
    mode [B,3,H,W] = (k*, mode_disp, mode_mass) with k* the FIRST arg-max of prob, or `index` [B,H,W] where it is given (the window
    about a k* found elsewhere)."""
    disp, stats = prob_stats_torch(prob)
    if index is None:
        index = _first_index(prob, prob.amax(1, keepdim=True))
    return disp, stats, _window_torch(prob, radius, index)


def disp_mode_torch(cost: torch.Tensor, maxdisp: int, radius: int, size=None, index=None):
    """Plain-torch twin of ops.disp_softargmin_mode in cost's dtype and on its device: the upsampled cost v and p = softmin(v) of
    disp_stats_torch, k* = the first arg-min of v (or `index`), then the window sums of p about k*.  Returns (disp, stats, mode)."""
    import torch.nn.functional as F
    if cost.dim() == 4:
        cost = cost[:, None]
    Ho, Wo = (3 * cost.shape[3], 3 * cost.shape[4]) if size is None else size
    v = F.interpolate(cost, (int(maxdisp), int(Ho), int(Wo)), mode="trilinear", align_corners=False)[:, 0]
    p = F.softmin(v, dim=1)
    disp, stats = prob_stats_torch(p)
    if index is None:
        index = _first_index(v, v.amin(1, keepdim=True))
    return disp, stats, _window_torch(p, radius, index)


class MaskedSmoothL1Fn(torch.autograd.Function):
    """F.smooth_l1_loss(disp_est[mask], disp_gt[mask]) with mask = 0 < gt < maxdisp (rag.py:210-211), forward and
    backward in one kernel each, without the boolean gather (no stream synchronisation)."""

    @staticmethod
    def forward(ctx, disp_est, disp_gt, maxdisp, meter=None):
        est = disp_est.contiguous()
        out = _raw(est, disp_gt, maxdisp, meter)
        ctx.save_for_backward(est, disp_gt.contiguous(), out)
        ctx.maxdisp = float(maxdisp)
        return out[0] * 1.0          # a kernel, not a memcpy (see ragmi_stereo_metrics_fwd on hipGraph memcpy nodes)

    @staticmethod
    def backward(ctx, gout):
        est, gt, out = ctx.saved_tensors
        B, H, W = est.shape
        gout = gout.reshape(1).contiguous().float()
        d = torch.empty_like(est)
        check(load_library().ragmi_masked_smooth_l1_bwd(est.data_ptr(), gt.data_ptr(), out.data_ptr(), gout.data_ptr(), d.data_ptr(),
                                                        B, H, W, ctx.maxdisp, ops._stream()), "masked_smooth_l1_bwd")
        return d, None, None, None


def masked_smooth_l1(disp_est: torch.Tensor, disp_gt: torch.Tensor, maxdisp: float = 192, meter: Optional[EpochMeter] = None) -> torch.Tensor:
    """`meter`: the loss launch is also the epoch meter's update for this batch (the reference scores the disp_est it trained on,
    rag.py:386-396)."""
    return MaskedSmoothL1Fn.apply(disp_est, disp_gt, maxdisp, meter)


# --------------------------------------------------------------------------- training the head's uncertainty
VAR_FLOOR = 1.0 / 12.0       # px^2: the variance of a uniform distribution over one disparity bin; a parameter, not a measurement


def disp_stats_bwd_torch(cost: torch.Tensor, maxdisp: int, dout: Optional[torch.Tensor], dstats: Optional[torch.Tensor]) -> torch.Tensor:
    """Plain-torch twin of ops.disp_softargmin_stats_bwd in cost's dtype and on its device: the closed form
        dL/dv_k = -p_k [ gmu (k - mu) + gV ((k - mu)^2 - var) - gH (ln p_k + H) - gP peak ] - [k = k*] gP peak
    on the upsampled cost v (p = softmin(v), k* = the first arg-max), then the adjoint of the trilinear x3 upsample (linear: ATen's
    own).  cost [B,1,d,h,w] or [B,d,h,w]; dout [B,3h,3w] or None; dstats [B,3,3h,3w] (variance, peak, entropy) or None."""
    import torch.nn.functional as F
    shape = cost.shape
    c = (cost if cost.dim() == 5 else cost[:, None]).detach().clone().requires_grad_(True)
    Ho, Wo = 3 * c.shape[3], 3 * c.shape[4]
    with torch.enable_grad():
        v = F.interpolate(c, (int(maxdisp), Ho, Wo), mode="trilinear", align_corners=False)
    with torch.no_grad():
        logp = F.log_softmax(-v[:, 0], dim=1)
        p = logp.exp()
        zero = torch.zeros((), dtype=c.dtype, device=c.device)
        gmu = dout[:, None].to(c.dtype) if dout is not None else zero
        gV, gP, gH = (dstats[:, i:i + 1].to(c.dtype) for i in range(3)) if dstats is not None else (zero, zero, zero)
        k = torch.arange(int(maxdisp), dtype=c.dtype, device=c.device).view(1, -1, 1, 1)
        u = k - (p * k).sum(1, keepdim=True)
        var = (p * u * u).sum(1, keepdim=True)
        ent = -(p * logp).sum(1, keepdim=True)
        peak, kstar = p.max(1, keepdim=True)
        gv = -p * (gmu * u + gV * (u * u - var) - gH * (logp + ent) - gP * peak)
        gv = gv - torch.zeros_like(p).scatter_(1, kstar, 1.0) * (gP * peak)
    (g,) = torch.autograd.grad(v, c, gv[:, None])
    return g.reshape(shape)


def uncertainty_loss_torch(disp: torch.Tensor, stats: torch.Tensor, gt: torch.Tensor, maxdisp: float, var_floor: float = VAR_FLOOR) -> torch.Tensor:
    """Plain-torch twin of uncertainty_loss in disp's dtype and on its device (differentiable in disp and stats): the mean over
    mask = 0 < gt < maxdisp of smooth_l1(disp - gt) * rsqrt(s) + 0.5 ln s with s = stats[:, 0] + var_floor; nan on an empty mask."""
    import torch.nn.functional as F
    mask = (gt > 0) & (gt < maxdisp)
    s = stats[:, 0] + var_floor
    per = F.smooth_l1_loss(disp, gt.to(disp.dtype), reduction="none") * torch.rsqrt(s) + 0.5 * torch.log(s)
    return torch.where(mask, per, torch.zeros_like(per)).sum() / mask.sum()


class UncertaintyLossFn(torch.autograd.Function):
    """The uncertainty-aware loss of the head's own variance: one fused forward (two launches, no atomics) and a one-launch backward
    that writes d loss / d disp and all three planes of d loss / d stats."""

    @staticmethod
    def forward(ctx, disp_est, stats, disp_gt, maxdisp, var_floor):
        est, st, gt = disp_est.contiguous(), stats.contiguous(), disp_gt.contiguous()
        out = ops.uncertainty_loss_fwd(est, st, gt, maxdisp, var_floor)
        ctx.save_for_backward(est, st, gt, out)
        ctx.maxdisp, ctx.var_floor = float(maxdisp), float(var_floor)
        return out[0] * 1.0          # a kernel, not a memcpy node (as MaskedSmoothL1Fn)

    @staticmethod
    def backward(ctx, gout):
        est, st, gt, out = ctx.saved_tensors
        gout = gout.reshape(1).contiguous().float()
        ddisp, dstats = ops.uncertainty_loss_bwd(est, st, gt, out, gout, ctx.maxdisp, ctx.var_floor)
        return ddisp, dstats, None, None, None


def uncertainty_loss(disp: torch.Tensor, stats: torch.Tensor, gt: torch.Tensor, maxdisp: float = 192, var_floor: float = VAR_FLOOR) -> torch.Tensor:
    """Uncertainty-aware regression loss (Kendall & Gal's form) over the head's own variance: disp [B,H,W] and stats [B,3,H,W] of a
    forward_train_stats call (DispStats.disp / .tensor), gt [B,H,W].  Per pixel of mask = 0 < gt < maxdisp, with
    s = stats[:, 0] + var_floor:  smooth_l1(disp - gt) * rsqrt(s) + 0.5 ln s, averaged over the mask.  A residual the network marks
    as uncertain costs less, and marking it costs ln sigma.  Differentiable in disp and stats (HIP, fp32); on CPU tensors the
    plain-torch twin runs.  ops.uncertainty_loss_fwd gives the logging vector (loss, smooth-L1 mean, mean sigma, N)."""
    if not disp.is_cuda:
        return uncertainty_loss_torch(disp, stats, gt, maxdisp, var_floor)
    return UncertaintyLossFn.apply(disp, stats, gt, maxdisp, var_floor)


# --------------------------------------------------------------------------- scoring the uncertainty: sparsification curves, AUSE, AURG
SPARSIFY_WHICH = ("variance", "entropy", "one_minus_peak", "one_minus_mode_mass")
CURVE_NAMES = ("S_epe", "O_epe", "S_d1", "O_d1")
SCALAR_NAMES = ("AUSE_epe", "AURG_epe", "AUSE_d1", "AURG_d1", "N", "Nbad")
MAX_FRACTIONS = 32
_EQ_MAX = 4294967295.0     # e_q saturates at 2^32 - 1 (4096 px): it is the 32-bit radix key of the error-ranked curve O


def _fractions(fractions) -> int:
    if int(fractions) != fractions or not 1 <= int(fractions) <= MAX_FRACTIONS:
        raise ValueError(f"sparsification: fractions must be an integer in 1..{MAX_FRACTIONS}, got {fractions!r}")
    return int(fractions)


class CalibrationMeter:
    """Running float64 sums of the per-image sparsification rows of an epoch, on the device: `sums` [4K + 7] = the four curves, the
    six scalars, the number of images counted (those with a non-empty mask).  `sparsification(..., meter=m)` adds a batch in its
    finalize kernel (no extra launch, nothing leaves the device); `mean()` is the epoch's one device-to-host copy."""

    def __init__(self, device, fractions: int = 20):
        self.fractions = _fractions(fractions)
        self.sums = torch.zeros((4 * self.fractions + 7,), device=device, dtype=torch.float64)

    def reset(self) -> None:
        self.sums.zero_()

    def mean(self) -> Dict[str, object]:
        """CURVE_NAMES -> list of K floats, SCALAR_NAMES -> float (each the mean over the counted images; nan before the first one),
        "images" -> the number counted."""
        vals = self.sums.tolist()          # the only synchronisation
        K, n = self.fractions, vals[-1]
        avg = [v / n if n else float("nan") for v in vals[:-1]]
        out: Dict[str, object] = {name: avg[c * K:(c + 1) * K] for c, name in enumerate(CURVE_NAMES)}
        out.update(zip(SCALAR_NAMES, avg[4 * K:]))
        out["images"] = n
        return out


class Sparsification:
    """Result of `sparsification`: `.tensor` [B,4,K] fp32 holds S_epe, O_epe, S_d1, O_d1 per image (the error of the pixels kept when
    the (j N) / K most uncertain, for S, or most wrong, for O, are removed), `.scalars` [B,6] AUSE_epe, AURG_epe, AUSE_d1, AURG_d1, N,
    Nbad.  `[name]` and the attributes of the same names give views ([B,K] / [B]); `floats()` copies once to the host."""

    def __init__(self, flat: torch.Tensor, B: int, K: int):
        self._flat = flat                                  # one buffer behind both views: floats() is one copy
        self.tensor = flat[:B * 4 * K].view(B, 4, K)
        self.scalars = flat[B * 4 * K:].view(B, 6)

    def __getitem__(self, name: str) -> torch.Tensor:
        if name in CURVE_NAMES:
            return self.tensor[:, CURVE_NAMES.index(name)]
        return self.scalars[:, SCALAR_NAMES.index(name)]

    def __getattr__(self, name: str) -> torch.Tensor:
        if name in CURVE_NAMES or name in SCALAR_NAMES:
            return self[name]
        raise AttributeError(name)

    def floats(self) -> Dict[str, list]:
        """CURVE_NAMES -> B lists of K floats, SCALAR_NAMES -> B floats."""
        B, _, K = self.tensor.shape
        vals = self._flat.tolist()         # the only synchronisation
        out: Dict[str, list] = {name: [vals[(b * 4 + c) * K:(b * 4 + c + 1) * K] for b in range(B)] for c, name in enumerate(CURVE_NAMES)}
        s0 = B * 4 * K
        out.update({name: [vals[s0 + b * 6 + c] for b in range(B)] for c, name in enumerate(SCALAR_NAMES)})
        return out


def _sparsify_inputs(disp: torch.Tensor, unc: torch.Tensor, gt: torch.Tensor):
    if disp.dim() != 3 or unc.shape != disp.shape or gt.shape != disp.shape:
        raise ValueError("sparsification: disp, unc and gt must all be [B, H, W]")
    if disp.shape[1] * disp.shape[2] >= 2 ** 31:
        raise ValueError("sparsification: H * W must stay below 2^31")


def _kept_curve(key: torch.Tensor, e: torch.Tensor, bad: torch.Tensor, n: torch.Tensor):
    """(sum of e, number of bad) over the n[j] pixels of smallest key, in float64; the group of equal keys a cut falls into gives
    double(group sum) * double(kept of it) / double(its size), so the order inside a group never enters."""
    ks, idx = torch.sort(key)
    counts = torch.unique_consecutive(ks, return_counts=True)[1]
    ends = counts.cumsum(0)
    zero = ends.new_zeros(1)
    out = []
    gi = torch.searchsorted(ends, n)                       # the group that holds the n-th smallest key
    m, c = (n - (ends[gi] - counts[gi])).double(), counts[gi].double()
    for v in (e, bad):
        incl = v[idx].cumsum(0)[ends - 1]                  # int64: exact
        below = torch.cat((zero, incl[:-1]))
        out.append(below[gi].double() + (incl[gi] - below[gi]).double() * m / c)
    return out


def _sparsify_image(d: torch.Tensor, u: torch.Tensor, g: torch.Tensor, maxdisp: float, K: int):
    """(curves [4,K], scalars [6]) fp32 of one image: the definition of DESIGN.md 4.8.3 in int64 and float64."""
    d, u, g = d.reshape(-1), u.reshape(-1), g.reshape(-1)
    mask = (g > 0) & (g < torch.tensor(float(maxdisp), dtype=torch.float32, device=g.device)) & torch.isfinite(d) & torch.isfinite(u)
    d, u, g = d[mask], u[mask], g[mask]
    N = int(d.numel())
    nan = float("nan")
    if N == 0:
        return torch.full((4, K), nan, device=d.device), torch.tensor([nan] * 4 + [0.0, 0.0], device=d.device)
    e = torch.clamp(torch.round((d.double() - g.double()).abs() * 2.0 ** 20), max=_EQ_MAX).to(torch.int64)   # round: half to even
    E = (g - d).abs()
    bad = ((E > 3) & (E / g.abs() > torch.tensor(0.05, dtype=torch.float32, device=g.device))).to(torch.int64)   # D1's flag, in fp32
    bits = u.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    bits = torch.where((bits & 0x7FFFFFFF) == 0, torch.zeros_like(bits), bits)                                  # -0 == +0
    key = torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)                                   # fp32's total order
    j = torch.arange(K, dtype=torch.int64, device=d.device)
    r = (j * N) // K
    n = N - r
    nd = n.double()
    Nbad = int(bad.sum())
    s_e, s_b = _kept_curve(key, e, bad, n)
    o_e, _ = _kept_curve(e, e, bad, n)
    curves = torch.stack((s_e * 2.0 ** -20 / nd, o_e * 2.0 ** -20 / nd, s_b / nd, torch.clamp(Nbad - r, min=0).double() / nd)).float()
    rows = curves.double().tolist()

    def mean(terms):                                       # float64, j ascending
        a = 0.0
        for t in terms:
            a += t
        return a / K
    scal = [mean(s - o for s, o in zip(rows[0], rows[1])), mean(rows[0][0] - s for s in rows[0]),
            mean(s - o for s, o in zip(rows[2], rows[3])), mean(rows[2][0] - s for s in rows[2]), float(N), float(Nbad)]
    return curves, torch.tensor(scal, dtype=torch.float64, device=d.device).float()


def _meter_of(meter, device, K: int) -> None:
    if not isinstance(meter, CalibrationMeter) or meter.sums.device != device or meter.fractions != K:
        raise ValueError("sparsification: meter must be a rag_amd.CalibrationMeter on the inputs' device with the same fractions")


def sparsification_torch(disp: torch.Tensor, unc: torch.Tensor, gt: torch.Tensor, maxdisp: float = 192, fractions: int = 20,
                         meter: Optional[CalibrationMeter] = None) -> Sparsification:
    """Plain-torch twin of `sparsification` on the inputs' device: the same definition with torch.sort, unique_consecutive and int64 /
    float64 sums (the CPU path, and the yardstick of the tests and tools/bench_sparsification.py)."""
    K = _fractions(fractions)
    _sparsify_inputs(disp, unc, gt)
    if not maxdisp > 0:
        raise ValueError("sparsification: maxdisp must be positive")
    if meter is not None:
        _meter_of(meter, disp.device, K)
    with torch.no_grad():
        d, u, g = (t.detach().float() for t in (disp, unc, gt))
        rows = [_sparsify_image(d[b], u[b], g[b], maxdisp, K) for b in range(d.shape[0])]
        curves, scalars = torch.stack([c for c, _ in rows]), torch.stack([s for _, s in rows])
        if meter is not None:
            counted = (scalars[:, 4] > 0).double()[:, None]
            both = torch.cat((curves.reshape(len(rows), -1), scalars), dim=1).double()
            meter.sums[:-1] += torch.where(counted > 0, both, torch.zeros_like(both)).sum(0)
            meter.sums[-1] += counted.sum()
        return Sparsification(torch.cat((curves.reshape(-1), scalars.reshape(-1))), len(rows), K)


def sparsification(disp: torch.Tensor, unc: torch.Tensor, gt: torch.Tensor, maxdisp: float = 192, fractions: int = 20,
                   meter: Optional[CalibrationMeter] = None) -> Sparsification:
    """Does `unc` rank the errors of `disp`?  Per image of disp, unc, gt [B,H,W] (larger unc = less certain), over the pixels with
    0 < gt < maxdisp and finite disp and unc: S_epe[j] / S_d1[j] are the EPE / D1 of the pixels kept after removing the (j N) / K most
    uncertain (j < K = fractions), O_epe / O_d1 the same when the most wrong are removed instead; AUSE = mean_j(S - O) (0 for a perfect
    ranking), AURG = mean_j(S[0] - S[j]) (the gain over random removal).  Equal uncertainties share their group's error in
    proportion, so no tie order enters; errors are summed as integers of 2^-20 px, so the result is bitwise reproducible.  One fused
    device pass without a sort: no synchronisation, no gather, capturable in a graph.  `meter`: the same launches
    also add the images with a non-empty mask to that CalibrationMeter.  An image with an empty mask gives NaN curves and areas.  No
    gradient; on CPU tensors the plain-torch twin runs."""
    refuse_autograd("sparsification", disp, unc, gt)
    if not disp.is_cuda:
        return sparsification_torch(disp, unc, gt, maxdisp, fractions, meter)
    K = _fractions(fractions)
    ops._need_gpu(disp, unc, gt)
    _sparsify_inputs(disp, unc, gt)
    if meter is not None:
        _meter_of(meter, disp.device, K)
    with torch.no_grad():
        d, u, g = disp.detach().contiguous(), unc.detach().contiguous(), gt.detach().contiguous()
        B, H, W = d.shape
        lib = load_library()
        ws = torch.empty((max(1, lib.ragmi_sparsification_workspace_elems(B, H, W, K)), 2), device=d.device, dtype=torch.int64)
        flat = torch.empty((B * (4 * K + 6),), device=d.device, dtype=torch.float32)
        check(lib.ragmi_sparsification_fwd(d.data_ptr(), u.data_ptr(), g.data_ptr(), B, H, W, float(maxdisp), K, ws.data_ptr(),
                                           flat.data_ptr(), flat.data_ptr() + 4 * B * 4 * K,
                                           meter.sums.data_ptr() if meter is not None else None, ops._stream()), "sparsification")
        return Sparsification(flat, B, K)


# --------------------------------------------------------------------------- self-supervised loss (src_self, supervise=False)
SELFSUP_NAMES = ("loss", "ssim", "l1", "smooth")


def _selfsup_raw(disp_est: torch.Tensor, left: torch.Tensor, right: torch.Tensor, want_grad: bool, weight: Optional[torch.Tensor] = None):
    """(out[4], unit gradient or None) of ragmi_selfsup_loss_fwd, or of ragmi_selfsup_loss_weighted_fwd with `weight` [B, H, W];
    nothing leaves the device."""
    for t in (disp_est, left, right, weight):
        if t is not None and not t.is_cuda:
            raise RuntimeError("rag_amd ops run on the MI355X only (got a CPU tensor); there is no CPU fallback")
    if disp_est.dim() != 3 or left.dim() != 4 or right.shape != left.shape or left.shape[0] != disp_est.shape[0] \
            or tuple(left.shape[2:]) != tuple(disp_est.shape[1:]):
        raise ValueError("re_and_sm_loss: disp_est must be [B, H, W] and left, right [B, C, H, W]")
    if weight is not None and weight.shape != disp_est.shape:
        raise ValueError("re_and_sm_loss: weight must be [B, H, W] like disp_est")
    dtypes = {disp_est.dtype, left.dtype, right.dtype} | ({weight.dtype} if weight is not None else set())
    dt = ops._DT.get(disp_est.dtype, -1) if len(dtypes) == 1 else -1     # the library refuses what it was not built for
    B, C, H, W = left.shape
    d, lt, rt = disp_est.contiguous(), left.contiguous(), right.contiguous()
    lib = load_library()
    out = torch.empty((4,), device=d.device, dtype=torch.float32)
    ug = torch.empty((B, H, W), device=d.device, dtype=torch.float32) if want_grad else None
    name = "selfsup_loss" if weight is None else "selfsup_loss_weighted"
    w = () if weight is None else (weight.contiguous(),)
    ws = torch.empty((max(1, getattr(lib, f"ragmi_{name}_workspace_elems")(B, H, W)),), device=d.device, dtype=torch.float32)
    check(getattr(lib, f"ragmi_{name}_fwd")(*(t.data_ptr() for t in (lt, rt, d) + w), B, C, H, W, dt, ws.data_ptr(), out.data_ptr(),
                                            ug.data_ptr() if ug is not None else None, ops._stream()), f"{name}_fwd")
    return out, ug


class SelfSupervisedLossFn(torch.autograd.Function):
    """re_and_sm_loss (src_self/models/loss.py:112-141) of disp_est [B,H,W] against the images it was computed from: one fused
    forward that also writes d loss / d disp_est at unit scale, and a backward that scales it by the incoming gradient.  Images get
    no gradient (the reference's step never asks for one), and neither does `weight` (a constant of the weighted form)."""

    @staticmethod
    def forward(ctx, disp_est, left, right, weight=None):
        out, ug = _selfsup_raw(disp_est.detach(), left.detach(), right.detach(), ctx.needs_input_grad[0],
                               weight.detach() if weight is not None else None)
        if ug is not None:
            ctx.save_for_backward(ug)
        ctx.weighted = weight is not None
        return out[0] * 1.0          # a kernel, not a memcpy node (as MaskedSmoothL1Fn)

    @staticmethod
    def backward(ctx, gout):
        (ug,) = ctx.saved_tensors
        gout = gout.reshape(1).contiguous().float()
        g = torch.empty_like(ug)
        lib = load_library()
        bwd = lib.ragmi_selfsup_loss_weighted_bwd if ctx.weighted else lib.ragmi_selfsup_loss_bwd
        check(bwd(ug.data_ptr(), gout.data_ptr(), g.data_ptr(), ug.numel(), ops._stream()), "selfsup_loss_bwd")
        return g, None, None, None


def re_and_sm_loss(disp_est: torch.Tensor, left: torch.Tensor, right: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The self-supervised training loss of src_self (models/loss.py:112-141) under the reference's name: 0.85 SSIM + 0.15 L1
    of `right` warped to `left` by disp_est, + 0.1 edge-aware smoothness; differentiable in disp_est (HIP, fp32).  `weight` [B,H,W]
    (finite, non-negative, e.g. LRCheck.weight; a constant: no gradient flows to it): L1 = sum w |left - left_est| / (C sum w),
    SSIM = sum wb term / (C sum wb) with wb = avg_pool2d(w, 3), smoothness unweighted; a term whose weights sum to 0 is 0.  None
    takes the unweighted kernel."""
    if weight is None:
        return SelfSupervisedLossFn.apply(disp_est, left, right)
    return SelfSupervisedLossFn.apply(disp_est, left, right, weight)


def self_supervised_terms(disp_est: torch.Tensor, left: torch.Tensor, right: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 4-float device vector (loss, SSIM_mean, L1_mean, smoothness) of re_and_sm_loss for logging: no gradient, no sync."""
    with torch.no_grad():
        return _selfsup_raw(disp_est.detach(), left.detach(), right.detach(), False, weight.detach() if weight is not None else None)[0]


def re_and_sm_loss_torch(disp_est: torch.Tensor, left: torch.Tensor, right: torch.Tensor, weight: Optional[torch.Tensor] = None):
    """Plain-torch restatement of re_and_sm_loss in the dtype and on the device of its inputs (host twin of the CPU step, and the
    fp64 / ATen yardstick of the tests and tools/bench_selfsup.py).  Returns (loss, (ssim_mean, l1_mean, smooth_mean)).  `weight`
    [B,H,W]: the weighted form of re_and_sm_loss (a constant; a term whose weights sum to 0 is 0)."""
    import torch.nn.functional as F
    B, C, H, W = left.shape
    dt, dev = disp_est.dtype, disp_est.device
    xs = torch.arange(W, device=dev, dtype=dt).view(1, 1, W) - disp_est
    ys = torch.arange(H, device=dev, dtype=dt).view(1, H, 1).expand(B, H, W)
    grid = torch.stack((2 * xs / (W - 1) - 1, 2 * ys / (H - 1) - 1), dim=-1)      # align_corners=True normalisation ...
    sample = F.grid_sample(right, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # ... sampled without it
    with torch.no_grad():
        cover = F.grid_sample(torch.ones_like(right[:, :1]), grid.detach(), mode="bilinear", padding_mode="zeros", align_corners=False)
        keep = (cover >= 0.9999).to(dt)
    est = sample * keep
    mu_x, mu_y = F.avg_pool2d(left, 3), F.avg_pool2d(est, 3)                    # stride 3: non-overlapping blocks
    var_x = F.avg_pool2d(left * left, 3) - mu_x * mu_x
    var_y = F.avg_pool2d(est * est, 3) - mu_y * mu_y
    cov = F.avg_pool2d(left * est, 3) - mu_x * mu_y
    c1, c2 = 1e-4, 9e-4
    s = (2 * mu_x * mu_y + c1) * (2 * cov + c2) / ((mu_x * mu_x + mu_y * mu_y + c1) * (var_x + var_y + c2))
    term = torch.clamp((1 - s) / 2, 0, 1)
    if weight is None:
        l1 = (left - est).abs().mean()
        ssim = term.mean()
    else:
        w = weight.detach().to(dt)[:, None]
        wb = F.avg_pool2d(w, 3)

        def wmean(num, den):                                                    # 0 where the weights sum to 0 (never 0 / 0)
            return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(num))
        l1 = wmean((w * (left - est).abs()).sum(), C * w.sum())
        ssim = wmean((wb * term).sum(), C * wb.sum())
    wx = torch.exp(-(left[..., :, :-1] - left[..., :, 1:]).mean(1).abs())
    wy = torch.exp(-(left[..., :-1, :] - left[..., 1:, :]).mean(1).abs())
    smooth = (((disp_est[..., :, :-1] - disp_est[..., :, 1:]).abs() * wx).sum()
              + ((disp_est[..., :-1, :] - disp_est[..., 1:, :]).abs() * wy).sum()) / (B * H * W)
    return 0.85 * ssim + 0.15 * l1 + 0.1 * smooth, (ssim, l1, smooth)


# --------------------------------------------------------------------------- left-right consistency (occlusion-aware adaptation step)
class LRCheck:
    """Result of `lr_consistency`: `.weight` [B,H,W] is 1 where the pixel's disparity agrees with the other view's and
    `occluded_weight` elsewhere (the `weight=` of re_and_sm_loss), `.error` [B,H,W] the disagreement |d - d'| in px (+inf where the
    pixel's match lies outside the other image or a value is not finite; None with want_error=False), `.valid` [B] the consistent
    share of each image, `.mask` the boolean `weight == 1`.  Everything stays on the device."""

    def __init__(self, weight: torch.Tensor, error: Optional[torch.Tensor], valid: torch.Tensor):
        self.weight, self.error, self.valid = weight, error, valid

    @property
    def mask(self) -> torch.Tensor:
        return self.weight == 1


def _lr_args(disp: torch.Tensor, partner: torch.Tensor, abs_tol, rel_tol, occluded_weight, partner_shift) -> None:
    import math
    if disp.dim() != 3 or partner.shape != disp.shape:
        raise ValueError("lr_consistency: disp_left and disp_right must both be [B, H, W]")
    if disp.shape[0] < 1 or disp.shape[1] < 1 or disp.shape[2] < 2:
        raise ValueError("lr_consistency: needs B, H >= 1 and W >= 2")
    for name, v in (("abs_tol", abs_tol), ("rel_tol", rel_tol)):
        if not (math.isfinite(v) and v >= 0):
            raise ValueError(f"lr_consistency: {name} must be finite and non-negative, got {v!r}")
    if not (math.isfinite(occluded_weight) and 0 <= occluded_weight <= 1):
        raise ValueError(f"lr_consistency: occluded_weight must lie in [0, 1], got {occluded_weight!r}")
    if int(partner_shift) != partner_shift or not 0 <= int(partner_shift) < disp.shape[0]:
        raise ValueError(f"lr_consistency: partner_shift must be an integer in [0, {disp.shape[0]}), got {partner_shift!r}")


def lr_consistency_torch(disp_left: torch.Tensor, disp_right: torch.Tensor, abs_tol: float = 1.0, rel_tol: float = 0.0,
                         occluded_weight: float = 0.0, mirrored: bool = False, partner_shift: int = 0, want_error: bool = True) -> LRCheck:
    """Plain-torch twin of `lr_consistency` in the dtype and on the device of its inputs (the CPU path, and the float64 / ATen
    yardstick of the tests and tools/bench_lr_check.py).  The three parameters are rounded to float32 first, as the C ABI takes them."""
    _lr_args(disp_left, disp_right, abs_tol, rel_tol, occluded_weight, partner_shift)
    with torch.no_grad():
        d = disp_left.detach()
        dt, dev = d.dtype, d.device
        B, H, W = d.shape
        a_tol, r_tol, occ = (torch.tensor(float(v), dtype=torch.float32, device=dev).to(dt) for v in (abs_tol, rel_tol, occluded_weight))
        p = disp_right.detach().to(dt)
        if int(partner_shift):
            p = torch.roll(p, -int(partner_shift), 0)                          # p[b] = partner[(b + shift) mod B]
        if mirrored:
            p = p.flip(-1)
        xr = torch.arange(W, device=dev, dtype=dt).view(1, 1, W) - d
        in_view = torch.isfinite(d) & (xr >= 0) & (xr <= W - 1)
        xs = torch.where(in_view, xr, torch.zeros_like(xr))                    # a value out of view is never an index
        x0f = torch.floor(xs)
        x0 = x0f.long()
        x1 = torch.clamp(x0 + 1, max=W - 1)
        f = xs - x0f
        e = (d - ((1 - f) * torch.gather(p, 2, x0) + f * torch.gather(p, 2, x1))).abs()
        seen = in_view & torch.isfinite(e)
        inf = torch.full_like(e, float("inf"))
        ok = seen & (torch.where(seen, e, inf) <= torch.maximum(a_tol, r_tol * d.abs()))
        weight = torch.where(ok, torch.ones_like(e), occ.expand_as(e))
        valid = (ok.sum((1, 2)).double() / float(H * W)).float()
        return LRCheck(weight, torch.where(seen, e, inf) if want_error else None, valid)


def lr_consistency(disp_left: torch.Tensor, disp_right: torch.Tensor, abs_tol: float = 1.0, rel_tol: float = 0.0,
                   occluded_weight: float = 0.0, mirrored: bool = False, partner_shift: int = 0, want_error: bool = True) -> LRCheck:
    """Left-right consistency check of disp_left [B,H,W] against the other view's disparity disp_right [B,H,W] (both positive for a
    point in front of the cameras, each in its view's coordinates such that pixel x of the first matches x - d of the second).  Per
    pixel d = disp_left[b,y,x] is looked up at x - d in the partner map (linear along the row) and the pixel is consistent when its
    match lies inside the image and |d - d'| <= max(abs_tol, rel_tol |d|); occluded pixels and mismatches are not.  -> LRCheck
    (.weight: 1 / occluded_weight, .error, .valid, .mask).  `partner_shift`: image b is checked against
    disp_right[(b + partner_shift) mod B]; `mirrored`: the partner row is read mirrored along x.  With both, the [2B,H,W] output D
    of a forward on the `lr_stack` batch checks itself: lr_consistency(D, D, mirrored=True, partner_shift=B).  One fused HIP pass
    (two launches, no synchronisation, bitwise reproducible); no gradient; on CPU tensors the plain-torch twin runs."""
    refuse_autograd("lr_consistency", disp_left, disp_right)
    if not disp_left.is_cuda:
        return lr_consistency_torch(disp_left, disp_right, abs_tol, rel_tol, occluded_weight, mirrored, partner_shift, want_error)
    ops._need_gpu(disp_left, disp_right)
    _lr_args(disp_left, disp_right, abs_tol, rel_tol, occluded_weight, partner_shift)
    if disp_left.dtype != torch.float32 or disp_right.dtype != torch.float32:
        raise RuntimeError(f"lr_consistency: float32 only (got {disp_left.dtype}, {disp_right.dtype})")
    with torch.no_grad():
        d, p = disp_left.detach().contiguous(), disp_right.detach().contiguous()
        B, H, W = d.shape
        lib = load_library()
        ws = torch.empty((max(1, lib.ragmi_lr_check_workspace_elems(B, H, W)),), device=d.device, dtype=torch.int32)
        weight = torch.empty_like(d)
        err = torch.empty_like(d) if want_error else None
        valid = torch.empty((B,), device=d.device, dtype=torch.float32)
        check(lib.ragmi_lr_check_fwd(d.data_ptr(), p.data_ptr(), B, H, W, int(partner_shift), int(bool(mirrored)), float(abs_tol),
                                     float(rel_tol), float(occluded_weight), ws.data_ptr(), weight.data_ptr(),
                                     err.data_ptr() if err is not None else None, valid.data_ptr(), ops._stream()), "lr_check_fwd")
        return LRCheck(weight, err, valid)


def lr_stack(left: torch.Tensor, right: torch.Tensor, out=None):
    """The two-view batch of the left-right check: (left2, right2) = ([left ; mirror_x(right)], [right ; mirror_x(left)]), both
    [2B,C,H,W].  Sample i is the ordinary pair, sample i + B the pair seen from the right camera; mirrored along x it is again a
    left / right pair, so one forward of the 2B batch gives both views' disparities (the right view's mirrored).  One HIP launch
    (fp32; a kernel, so a captured step holds no memcpy node); torch.cat / flip on CPU tensors.  `out`: a pair of [2B,C,H,W]
    buffers to write into.  No gradient."""
    if left.dim() != 4 or right.shape != left.shape:
        raise ValueError("lr_stack: left and right must both be [B, C, H, W]")
    B, C, H, W = left.shape
    if out is not None and (len(out) != 2 or any(tuple(o.shape) != (2 * B, C, H, W) or o.dtype != left.dtype or o.device != left.device
                                                 or not o.is_contiguous() for o in out)):
        raise ValueError("lr_stack: out must be a pair of contiguous [2B, C, H, W] tensors of left's dtype on its device")
    with torch.no_grad():
        lt, rt = left.detach(), right.detach()
        if not lt.is_cuda:
            l2, r2 = torch.cat((lt, rt.flip(-1))), torch.cat((rt, lt.flip(-1)))
            if out is None:
                return l2, r2
            out[0].copy_(l2)
            out[1].copy_(r2)
            return out[0], out[1]
        ops._need_gpu(lt, rt)
        if lt.dtype != torch.float32 or rt.dtype != torch.float32:
            raise RuntimeError(f"lr_stack: float32 only (got {lt.dtype}, {rt.dtype})")
        lt, rt = lt.contiguous(), rt.contiguous()
        l2, r2 = out if out is not None else (torch.empty((2 * B, C, H, W), device=lt.device, dtype=lt.dtype) for _ in range(2))
        check(load_library().ragmi_lr_stack_fwd(lt.data_ptr(), rt.data_ptr(), l2.data_ptr(), r2.data_ptr(), B, C, H, W, ops._stream()),
              "lr_stack_fwd")
        return l2, r2


# --------------------------------------------------------------------------- dense disparity: fill what the keep map rejects
FILL_CODES = ("kept", "row_min", "row_one_side", "column_min", "column_one_side", "fill_value")


class FilledDisp:
    """Result of `fill_disparity`: `.disp` [B,H,W] the dense map (with median=0 a kept pixel keeps its bits), `.code` [B,H,W] uint8
    where each value came from (0 kept, 1 the smaller of the row's two neighbours, 2 its only neighbour, 3 / 4 the same along the
    column for a row without a reliable pixel, 5 fill_value: FILL_CODES), `.counts` [B,6] int32 the pixels per code, `.density` [B]
    the share of code 0, `.filled` the boolean `code != 0`.  Codes and counts describe the fill, not the median.  `.speckles`: the
    `Speckles` whose keep map was filled (Network.forward_dense(speckle=...)), else None.  Everything stays on the device."""

    def __init__(self, disp: torch.Tensor, code: torch.Tensor, counts: torch.Tensor, density: torch.Tensor, speckles=None):
        self.disp, self.code, self.counts, self.density, self.speckles = disp, code, counts, density, speckles

    @property
    def filled(self) -> torch.Tensor:
        return self.code != 0


def _fill_args(disp: torch.Tensor, keep, median, fill_value) -> torch.Tensor:
    """The checks shared by the launch and its twin -> the keep tensor (an LRCheck gives its weight, a Speckles its keep)."""
    import math
    if isinstance(keep, LRCheck):
        keep = keep.weight
    elif isinstance(keep, Speckles):
        keep = keep.keep
    if not isinstance(disp, torch.Tensor) or not isinstance(keep, torch.Tensor):
        raise TypeError("fill_disparity: disp must be a tensor and keep an LRCheck, a Speckles or a tensor")
    if disp.dim() != 3 or keep.shape != disp.shape or min(disp.shape) < 1:
        raise ValueError("fill_disparity: disp and keep must both be [B, H, W] with B, H, W >= 1")
    if not disp.dtype.is_floating_point:
        raise TypeError(f"fill_disparity: disp must be a floating-point map, got {disp.dtype}")
    if keep.dtype not in (torch.bool, torch.uint8) and not keep.dtype.is_floating_point:
        raise TypeError(f"fill_disparity: keep must be bool, uint8 (non-zero keeps) or a floating-point weight (== 1 keeps), got {keep.dtype}")
    if keep.device != disp.device:
        raise RuntimeError(f"fill_disparity: disp is on {disp.device} and keep on {keep.device} (a CPU and a GPU tensor do not mix)")
    if isinstance(median, bool) or median not in (0, 3, 5):
        raise ValueError(f"fill_disparity: median must be 0, 3 or 5, got {median!r}")
    if isinstance(fill_value, bool) or not isinstance(fill_value, (int, float)) or not math.isfinite(fill_value):
        raise ValueError(f"fill_disparity: fill_value must be a finite number, got {fill_value!r}")
    return keep


def _farther(later: torch.Tensor, first: torch.Tensor) -> torch.Tensor:
    return torch.where(later < first, later, first)                             # (later < first) ? later : first, never fmin


def _nearest(ok: torch.Tensor, dim: int):
    """Along `dim`: the index of the nearest True at or before each position (-1: none) and at or after it (size: none)."""
    n = ok.shape[dim]
    shape = [1] * ok.dim()
    shape[dim] = n
    idx = torch.arange(n, device=ok.device).view(shape).expand_as(ok)
    before = torch.where(ok, idx, torch.full_like(idx, -1)).cummax(dim).values
    after = torch.where(ok, idx, torch.full_like(idx, n)).flip(dim).cummin(dim).values.flip(dim)
    return before, after


def median_disparity_torch(disp: torch.Tensor, m: int) -> torch.Tensor:
    """The m x m median (m = 3, 5) of a finite map [B,H,W] over replicate-padded windows: the (m*m+1)/2-th smallest."""
    if m not in (3, 5):
        raise ValueError(f"median_disparity_torch: m must be 3 or 5, got {m!r}")
    B, H, W = disp.shape
    r = m // 2
    ys = torch.arange(-r, H + r, device=disp.device).clamp(0, H - 1)
    xs = torch.arange(-r, W + r, device=disp.device).clamp(0, W - 1)
    padded = disp[:, ys][:, :, xs]
    win = padded.unfold(1, m, 1).unfold(2, m, 1).reshape(B, H, W, m * m)
    return win.sort(-1).values[..., (m * m) // 2].contiguous()


def fill_disparity_torch(disp: torch.Tensor, keep, median: int = 0, fill_value: float = 0.0) -> FilledDisp:
    """Plain-torch twin of `fill_disparity` in the dtype and on the device of its inputs (the CPU path, and the ATen yardstick of the
    tests and tools/bench_disp_fill.py): cummax / cummin give the nearest reliable neighbour on each side, gather fetches it."""
    keep = _fill_args(disp, keep, median, fill_value)
    with torch.no_grad():
        d = disp.detach()
        k = keep.detach()
        B, H, W = d.shape
        reliable = ((k == 1) if k.dtype.is_floating_point else (k != 0)) & torch.isfinite(d)
        v = torch.where(reliable, d, torch.zeros_like(d))                      # a value that is not reliable is never read
        li, ri = _nearest(reliable, 2)
        has_l, has_r = li >= 0, ri < W
        v_l, v_r = torch.gather(v, 2, li.clamp(min=0)), torch.gather(v, 2, ri.clamp(max=W - 1))
        both = has_l & has_r
        row = torch.where(both, _farther(v_r, v_l), torch.where(has_l, v_l, v_r))
        code = torch.where(reliable, torch.zeros_like(li), torch.where(both, torch.ones_like(li), torch.full_like(li, 2)))
        row_ok = reliable.any(2)                                                # [B,H]: rows the row pass completes
        ui, di = _nearest(row_ok, 1)
        has_u, has_d = (ui >= 0)[..., None], (di < H)[..., None]
        r_u = torch.gather(row, 1, ui.clamp(min=0)[..., None].expand(B, H, W))
        r_d = torch.gather(row, 1, di.clamp(max=H - 1)[..., None].expand(B, H, W))
        fill = torch.full_like(d, float(fill_value))
        col = torch.where(has_u & has_d, _farther(r_d, r_u), torch.where(has_u, r_u, torch.where(has_d, r_d, fill)))
        col_code = torch.where(has_u & has_d, 3, torch.where(has_u | has_d, 4, 5)).expand(B, H, W)
        out = torch.where(row_ok[..., None], row, col)
        code = torch.where(row_ok[..., None], code, col_code).to(torch.uint8)
        counts = torch.stack([(code == c).sum((1, 2)) for c in range(6)], 1).to(torch.int32)
        density = (counts[:, 0].double() / float(H * W)).float()
        if median:
            out = median_disparity_torch(out, median)
        return FilledDisp(out, code, counts, density)


def fill_disparity(disp: torch.Tensor, keep, median: int = 0, fill_value: float = 0.0) -> FilledDisp:
    """Dense disparity from disp [B,H,W] and a keep map: an `LRCheck` (its .weight), a bool / uint8 tensor (non-zero keeps) or an
    fp32 weight (== 1 keeps), by background interpolation.  A pixel is reliable iff it is kept and finite; an unreliable one takes
    the SMALLER of the nearest reliable disparities to its left and right on its row ((v[R] < v[L]) ? v[R] : v[L]: the farther
    surface, which is what lies behind an occluder), or the only one; a row without a reliable pixel takes the same rule along the
    columns from the nearest rows that have one; an image without one becomes `fill_value`.  `median` = 3 or 5 then takes the
    m x m median of the filled map (clamped at the border).  Every output value is a copy of a reliable input (or fill_value), so
    the result is exact.  -> FilledDisp (.disp, .code, .counts, .density, .filled).  Three HIP launches (row scan, column pass, count
    finalize) and one for the median: no atomics, no synchronisation, bitwise reproducible; fp32; no gradient; on CPU tensors the
    plain-torch twin runs."""
    keep = _fill_args(disp, keep, median, fill_value)
    refuse_autograd("fill_disparity", disp, keep if keep.dtype.is_floating_point else None)
    if not disp.is_cuda:
        return fill_disparity_torch(disp, keep, median, fill_value)
    if disp.dtype != torch.float32 or (keep.dtype.is_floating_point and keep.dtype != torch.float32):
        raise RuntimeError(f"fill_disparity: float32 only (got {disp.dtype}, keep {keep.dtype})")
    with torch.no_grad():
        d, k = disp.detach().contiguous(), keep.detach().contiguous()
        is_u8 = k.dtype != torch.float32
        if k.dtype == torch.bool:
            k = k.view(torch.uint8)                                             # the same bytes: no launch
        B, H, W = d.shape
        lib = load_library()
        ws = torch.empty((lib.ragmi_disp_fill_workspace_elems(B, H, W),), device=d.device, dtype=torch.int32)
        out = torch.empty_like(d)
        code = torch.empty((B, H, W), device=d.device, dtype=torch.uint8)
        counts = torch.empty((B, 6), device=d.device, dtype=torch.int32)
        density = torch.empty((B,), device=d.device, dtype=torch.float32)
        check(lib.ragmi_disp_fill_fwd(d.data_ptr(), k.data_ptr(), int(is_u8), B, H, W, float(fill_value), ws.data_ptr(), out.data_ptr(),
                                      code.data_ptr(), counts.data_ptr(), density.data_ptr(), ops._stream()), "disp_fill_fwd")
        if median:
            smooth = torch.empty_like(out)
            check(lib.ragmi_disp_median_fwd(out.data_ptr(), smooth.data_ptr(), B, H, W, int(median), ops._stream()), "disp_median_fwd")
            out = smooth
        return FilledDisp(out, code, counts, density)


# --------------------------------------------------------------------------- speckle filter: drop small disparity segments before the fill
SPECKLE_COUNTS = ("reliable", "segments", "removed_pixels", "removed_segments", "largest")
SPECKLE_TILE = (16, 64)                         # RAGMI_SPECKLE_TILE_ROWS / _COLS of include/rag_amd.h: the tile of the first launch


class Speckles:
    """Result of `filter_speckles`: `.keep` [B,H,W] bool, True iff the pixel is reliable and its segment has more than max_size
    pixels (a `keep` for fill_disparity), `.label` [B,H,W] int32 the smallest y*W + x of the pixel's segment (-1: unreliable), `.size`
    [B,H,W] int32 the segment's pixel count (0: unreliable), `.counts` [B,5] int32 (SPECKLE_COUNTS: reliable pixels, segments, removed
    pixels, removed segments, the largest segment's size), `.density` [B] the share of kept pixels, `.removed` the boolean
    `(label >= 0) & ~keep`.  Everything stays on the device."""

    def __init__(self, keep: torch.Tensor, label: torch.Tensor, size: torch.Tensor, counts: torch.Tensor, density: torch.Tensor):
        self.keep, self.label, self.size, self.counts, self.density = keep, label, size, counts, density

    @property
    def removed(self) -> torch.Tensor:
        return (self.label >= 0) & ~self.keep


def _speckle_args(disp: torch.Tensor, keep, max_size, max_diff) -> Optional[torch.Tensor]:
    """The checks shared by the launch and its twin -> the keep tensor (an LRCheck gives its weight) or None."""
    import ctypes
    import math
    import numbers
    if isinstance(keep, LRCheck):
        keep = keep.weight
    if not isinstance(disp, torch.Tensor) or not (keep is None or isinstance(keep, torch.Tensor)):
        raise TypeError("filter_speckles: disp must be a tensor and keep an LRCheck, a tensor or None")
    if disp.dim() != 3 or min(disp.shape) < 1 or (keep is not None and keep.shape != disp.shape):
        raise ValueError("filter_speckles: disp and keep must both be [B, H, W] with B, H, W >= 1")
    if not disp.dtype.is_floating_point:
        raise TypeError(f"filter_speckles: disp must be a floating-point map, got {disp.dtype}")
    if keep is not None:
        if keep.dtype not in (torch.bool, torch.uint8) and not keep.dtype.is_floating_point:
            raise TypeError("filter_speckles: keep must be bool, uint8 (non-zero keeps) or a floating-point weight (== 1 keeps), "
                            f"got {keep.dtype}")
        if keep.device != disp.device:
            raise RuntimeError(f"filter_speckles: disp is on {disp.device} and keep on {keep.device} (a CPU and a GPU tensor do not mix)")
    if isinstance(max_size, bool) or not isinstance(max_size, numbers.Integral) or not 0 <= max_size <= 0x7fffffff:
        raise ValueError(f"filter_speckles: max_size must be an integer >= 0, got {max_size!r}")
    if (isinstance(max_diff, bool) or not isinstance(max_diff, numbers.Real) or not math.isfinite(max_diff) or max_diff < 0
            or not math.isfinite(ctypes.c_float(max_diff).value)):
        raise ValueError(f"filter_speckles: max_diff must be a finite number >= 0 (in float32), got {max_diff!r}")
    return keep


def filter_speckles_torch(disp: torch.Tensor, keep=None, max_size: int = 100, max_diff: float = 1.0) -> Speckles:
    """Plain-torch twin of `filter_speckles` in the dtype and on the device of its inputs (the CPU path, and the ATen yardstick of the
    tests and tools/bench_speckle.py).  Every pixel holds the index of a pixel of its own segment that is not larger than its own; a
    round takes the minimum over the joined neighbours' and then jumps to that pixel's own pointer, until a round changes nothing
    (one host synchronisation per round); scatter_add counts the sizes.  max_diff is rounded to float32 first, as the C ABI takes it."""
    keep = _speckle_args(disp, keep, max_size, max_diff)
    with torch.no_grad():
        d = disp.detach()
        B, H, W = d.shape
        n, dev = H * W, d.device
        reliable = torch.isfinite(d)
        if keep is not None:
            k = keep.detach()
            reliable = reliable & ((k == 1) if k.dtype.is_floating_point else (k != 0))
        md = torch.tensor(float(max_diff), dtype=torch.float32, device=dev).to(d.dtype)
        v = torch.where(reliable, d, torch.zeros_like(d))                      # a value that is not reliable is never read
        right = reliable[..., :-1] & reliable[..., 1:] & ((v[..., :-1] - v[..., 1:]).abs() <= md)      # [B,H,W-1]: x joined to x + 1
        down = reliable[:, :-1] & reliable[:, 1:] & ((v[:, :-1] - v[:, 1:]).abs() <= md)               # [B,H-1,W]: y joined to y + 1
        idx = torch.arange(n, device=dev).view(1, H, W).expand(B, H, W)
        none = torch.full((B, H, W), n, device=dev, dtype=idx.dtype)           # slot n: the unreliable pixels', it points at itself
        lab = torch.where(reliable, idx, none)
        while True:
            new = lab.clone()
            new[..., 1:] = torch.minimum(new[..., 1:], torch.where(right, lab[..., :-1], none[..., 1:]))
            new[..., :-1] = torch.minimum(new[..., :-1], torch.where(right, lab[..., 1:], none[..., 1:]))
            new[:, 1:] = torch.minimum(new[:, 1:], torch.where(down, lab[:, :-1], none[:, 1:]))
            new[:, :-1] = torch.minimum(new[:, :-1], torch.where(down, lab[:, 1:], none[:, 1:]))
            flat = torch.cat((new.reshape(B, n), none.reshape(B, n)[:, :1]), 1)
            for _ in range(2):                                                  # pointer jumping
                flat = flat.gather(1, flat)
            new = flat[:, :n].reshape(B, H, W)
            if torch.equal(new, lab):
                break
            lab = new
        flat = lab.reshape(B, n)
        total = torch.zeros((B, n + 1), device=dev, dtype=flat.dtype).scatter_add_(1, flat, torch.ones_like(flat))
        size = torch.where(reliable, total.gather(1, flat).reshape(B, H, W), torch.zeros_like(lab))
        kept = reliable & (size > int(max_size))
        root = reliable & (lab == idx)
        gone = reliable & ~kept
        counts = torch.stack((reliable.sum((1, 2)), root.sum((1, 2)), gone.sum((1, 2)), (root & gone).sum((1, 2)),
                              size.amax((1, 2))), 1).to(torch.int32)
        density = ((counts[:, 0] - counts[:, 2]).double() / float(n)).float()
        label = torch.where(reliable, lab, torch.full_like(lab, -1)).to(torch.int32)
        return Speckles(kept, label, size.to(torch.int32), counts, density)


def filter_speckles(disp: torch.Tensor, keep=None, max_size: int = 100, max_diff: float = 1.0) -> Speckles:
    """Speckle filter of a disparity map disp [B,H,W] (OpenCV's filterSpeckles, on the device): `keep` is an `LRCheck` (its .weight), a
    bool / uint8 tensor (non-zero keeps), an fp32 weight (== 1 keeps) or None (keep everything).  A pixel is reliable iff it is kept
    and finite; two 4-neighbours are joined iff both are reliable and |d_p - d_q| <= max_diff (fp32: one subtraction, one comparison;
    per edge, so a ramp of small steps is one segment; diagonals never join); a segment is a connected component and one of at most
    `max_size` pixels is a speckle: its pixels leave the keep map.  max_size=0 removes nothing (a pure labelling).  The defaults
    (100 px, 1 px) sit in the range OpenCV's SGBM documentation recommends (window 50-200, range 1-2): a convention, not something
    tuned here.  -> Speckles (.keep, .label, .size, .counts, .density, .removed); pass it to fill_disparity as its keep.  Five HIP
    launches (tile labelling in LDS, union at the tile seams, flatten, apply, count finalize): integer atomics only, no
    synchronisation, bitwise reproducible, graph-capturable; fp32; no gradient; on CPU tensors the plain-torch twin runs."""
    keep = _speckle_args(disp, keep, max_size, max_diff)
    refuse_autograd("filter_speckles", disp, keep if keep is not None and keep.dtype.is_floating_point else None)
    if not disp.is_cuda:
        return filter_speckles_torch(disp, keep, max_size, max_diff)
    if disp.dtype != torch.float32 or (keep is not None and keep.dtype.is_floating_point and keep.dtype != torch.float32):
        raise RuntimeError(f"filter_speckles: float32 only (got {disp.dtype}, keep {keep.dtype if keep is not None else None})")
    with torch.no_grad():
        d = disp.detach().contiguous()
        kind, k = 2, None
        if keep is not None:
            k = keep.detach().contiguous()
            kind = 0 if k.dtype == torch.float32 else 1
            if k.dtype == torch.bool:
                k = k.view(torch.uint8)                                         # the same bytes: no launch
        B, H, W = d.shape
        lib = load_library()
        ws = torch.empty((lib.ragmi_speckle_workspace_elems(B, H, W),), device=d.device, dtype=torch.int32)
        label = torch.empty((B, H, W), device=d.device, dtype=torch.int32)
        size = torch.empty_like(label)
        kept = torch.empty((B, H, W), device=d.device, dtype=torch.uint8)
        counts = torch.empty((B, len(SPECKLE_COUNTS)), device=d.device, dtype=torch.int32)
        density = torch.empty((B,), device=d.device, dtype=torch.float32)
        check(lib.ragmi_speckle_fwd(d.data_ptr(), k.data_ptr() if k is not None else None, kind, B, H, W, int(max_size), float(max_diff),
                                    ws.data_ptr(), label.data_ptr(), size.data_ptr(), kept.data_ptr(), counts.data_ptr(),
                                    density.data_ptr(), ops._stream()), "speckle_fwd")
        return Speckles(kept.view(torch.bool), label, size, counts, density)                # 0 / 1 bytes: no launch
