"""`Network` — the reference's grown monocular-depth model (rag_depth/src/models/rag_model.py:201-800) on the HIP kernels of
``rag_amd``, for inference and training.

The depth network is the stereo `rag_amd.network.Network` without the cost volume and the right image: the Matching-Net
layers keep their names (``stem3d0``, ``cells_3d``, ``last_*_3d``, hence the checkpoint's state_dict keys) but are the 2-D
modules (`ConvBR_2d`, `Cell_2d` built from ``genotype.normal``) over the left image's features, and `DispHead` + x3 bilinear +
x ``max_depth`` replaces `Disp`.  The unit bookkeeping and the growth API (``expand`` / ``select`` / ``get_new_model`` /
``get_param`` / ``modify_param``) are the stereo network's; only `_new_unit` differs.

``forward(left, right, t, task_arch, path)`` runs the Feature Net and the 2-D matching chain on the existing kernels, the
``last_12_3d`` -> ``upsample_12`` -> ``last_6_3d`` chain on the 1x1 kernels, and ``upsample_6`` -> ``last_3_3d`` -> DispHead ->
x3 upsample -> x max_depth as ONE launch (``ops.depth_head``).  It is inference only: a call that would need autograd or batch
statistics raises and names the training entry point.

``forward_train(left, t, task_arch, path)`` is the training forward of Appr.train_epoch (approaches/rag.py:182-246): the trunk on
the `rag_amd.autograd` Functions (train-mode BatchNorm where a unit is in train()), the head through `DepthHeadFn` (the same fused
forward launch; its backward is ``ops.depth_head_bwd``).  `silog_loss` is the loss of that step (utilstool/experiment.py:154-161)
with its fused HIP gradient; ``rag_amd.train`` drives both.  `search_forward` and a standalone `DispHead` stay inference only.

``search_forward_train(left, t, selected_ops)`` is the training forward of Appr.search_epoch (approaches/rag.py:371-427): one unit per
layer of `p` and the heads of task t.  `silog_metrics_loss` is that loop's loss, error metrics and epoch meter (`DepthEpochMeter`) as
the ONE pass of `depth_metrics`; ``rag_amd.depth_search`` drives the step.

`load_depth_checkpoint` rebuilds a grown model from the reference's ``checkpoint_task{t}.ckpt`` (``train()`` it to fine-tune or grow
a task); `depth_metrics` is the eval loop's silog_loss + compute_errors (approaches/rag.py:440-489) in one fused pass.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .checkpoint import _HEADS, _check_cell_pattern, _genotype, _unit_counts
from .modules import _CELL3D_ARCH, _ConvBR, ALL_CONV_ROWS, Cell_2d, ConvBR_2d, Genotype, _head_quarter, _plan_head
from .network import Network as _StereoNetwork

MAX_DEPTH = 80          # rag_model.py:298
FP32_ONLY = "rag_amd.depth.Network: fp32 only (bf16 activation storage is not built for the depth network)"
DEPTH_NAMES = ("silog_loss", "silog", "abs_rel", "log10", "rms", "sq_rel", "log_rms", "d1", "d2", "d3")


class DispHead(nn.Module):
    """rag_model.py:51-64: sigmoid(conv1(x)) then x `scale` bilinear (align_corners=False).  `conv1` is Conv2d(input_dim, 1, 3,
    padding=1) WITH bias.  Inside `Network.forward` the head is fused with upsample_6 and last_3_3d (ops.depth_head); called on its
    own (input_dim 1) it is the same kernel with an identity 3x3 in place of last_3_3d."""

    def __init__(self, input_dim=100):
        super().__init__()
        self.conv1 = nn.Conv2d(input_dim, 1, 3, padding=1)
        self.sigmoid = nn.Sigmoid()              # kept for attribute parity; the sigmoid runs in the kernel

    def forward(self, x, scale):
        if x.dim() != 4 or x.shape[1] != 1 or self.conv1.in_channels != 1:
            raise NotImplementedError("rag_amd DispHead: built for the one-channel head the depth network uses")
        _refuse_autograd(x, self.conv1.weight, self.conv1.bias)
        eye = _identity3x3(x.device)
        return ops.depth_head(x, eye, self.conv1.weight.detach(), self.conv1.bias.detach(), x.shape[2:], int(scale), 1.0)[:, None]


_EYE: Dict[str, torch.Tensor] = {}


def _identity3x3(device) -> torch.Tensor:
    key = str(device)
    if key not in _EYE:
        eye = torch.zeros((1, 1, 3, 3), dtype=torch.float32)
        eye[0, 0, 1, 1] = 1.0
        _EYE[key] = eye.to(device)
    return _EYE[key]


def _refuse_autograd(*ts) -> None:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError("rag_amd.depth: inference only (a standalone DispHead has no backward; the depth network trains through "
                           "Network.forward_train); call it under torch.no_grad() with the model in eval()")


class DepthHeadFn(torch.autograd.Function):
    """upsample_6 -> last_3_3d -> DispHead(., scale) -> x max_depth (rag_model.py:51-64, 357-416): the fused forward launch, and
    ops.depth_head_bwd (two launches, u / m / s recomputed from y) as its backward.  Weight gradients go straight into bucket-backed
    .grad views (rag_amd.autograd._direct) when there are some."""

    @staticmethod
    def forward(ctx, y, w3, w1, b1, size, scale, max_depth):
        size = tuple(int(v) for v in size)
        ctx.size, ctx.scale, ctx.max_depth = size, int(scale), float(max_depth)
        ctx.params = (w3, w1, b1)
        ctx.save_for_backward(y, w3, w1, b1)
        return ops.depth_head(y.detach(), w3.detach(), w1.detach(), b1.detach(), size, ctx.scale, ctx.max_depth)

    @staticmethod
    def backward(ctx, d_out):
        from .autograd import _direct
        y, w3, w1, b1 = ctx.saved_tensors
        need = ctx.needs_input_grad[1:4]
        direct = [_direct(p) if n else None for p, n in zip(ctx.params, need)]
        dy, dw3, dw1, db1 = ops.depth_head_bwd(y, w3.detach(), w1.detach(), b1.detach(), d_out, ctx.size, ctx.scale, ctx.max_depth,
                                               *direct)
        grads = [None if (not n or t is not None) else g for g, n, t in zip((dw3, dw1, db1), need, direct)]
        return (dy if ctx.needs_input_grad[0] else None, *grads, None, None, None)


class SilogLossFn(torch.autograd.Function):
    """silog_loss (utilstool/experiment.py:154-161) over gt > 0: two launches forward, one backward (ops.silog_loss / _bwd)."""

    @staticmethod
    def forward(ctx, est, gt, variance_focus):
        out, saved = ops.silog_loss(est.detach(), gt.detach(), variance_focus)
        ctx.vf = float(variance_focus)
        ctx.save_for_backward(est, gt, saved)
        return out.view(())

    @staticmethod
    def backward(ctx, grad):
        est, gt, saved = ctx.saved_tensors
        return ops.silog_loss_bwd(est.detach(), gt, saved, grad, ctx.vf), None, None


def silog_loss(est: torch.Tensor, gt: torch.Tensor, variance_focus: float = 0.85) -> torch.Tensor:
    """The depth training loss (utilstool/experiment.py:154-161, mask gt > 0): 10 sqrt(mean d^2 - variance_focus mean(d)^2),
    d = log est - log gt, as a 0-d tensor with a gradient w.r.t. `est`.  On the GPU the fused HIP loss (no boolean gather, no
    synchronisation); on the CPU `silog_loss_torch`.  No pixel with gt > 0: NaN loss (as the reference) and an all-zero gradient."""
    if est.is_cuda:
        return SilogLossFn.apply(est, gt, float(variance_focus))
    return silog_loss_torch(est, gt, variance_focus)


def silog_loss_torch(est: torch.Tensor, gt: torch.Tensor, variance_focus: float = 0.85) -> torch.Tensor:
    """Plain-torch restatement of the reference's silog_loss (CPU twin of `silog_loss`; the boolean gather synchronises)."""
    mask = gt > 0
    d = torch.log(est[mask]) - torch.log(gt[mask])
    return torch.sqrt((d ** 2).mean() - variance_focus * (d.mean() ** 2)) * 10.0


class DepthEpochMeter:
    """The epoch's running sums of Appr.search_epoch / search_eval / eval (approaches/rag.py:397-436, 441-490, 493-529) on the device.
    The reference copies the full depth_est and depth_gt maps to the host after every batch, gathers the masked pixels in numpy, runs
    compute_errors there and adds one `.item()` for the loss; here the finalize kernel of the loss / metrics launch adds the batch's ten
    floats to `sums` (ragmi_depth_metrics_meter_fwd: no extra launch, nothing leaves the device) and `mean()` is the epoch's one
    device-to-host copy.

    `sums`: float64 [12] - running sums of the ten DEPTH_NAMES (each batch's float added in double), the number of batches, the
    masked pixels.  The reference accumulates abs_rel and rmse in numpy float32 (compute_errors returns float32 for its entries 0-5
    and `0 + np.float32` stays float32) and d1-d3 and the loss in double; the meter accumulates all ten in double, so its means
    differ from the reference's float32 ones by at most (batches) x 2^-24 relative.  A batch without a valid pixel adds NaN, as
    numpy's mean of an empty selection does there.  `last`: the most recent batch's 10-float vector (the kernel's `out` itself,
    not a copy; None before the first batch)."""

    def __init__(self, device):
        self.sums = torch.zeros((12,), device=device, dtype=torch.float64)
        self.last = None

    def reset(self) -> None:
        self.sums.zero_()
        self.last = None

    def mean(self) -> Dict[str, float]:
        """DEPTH_NAMES -> sums[k] / sums[10] as Python floats (nan before the first batch)."""
        vals = self.sums.tolist()          # the only synchronisation
        n = vals[10]
        return {k: (v / n if n else float("nan")) for k, v in zip(DEPTH_NAMES, vals[:10])}


METER_NEEDS_GPU = "a DepthEpochMeter is updated by the HIP metrics launch: it needs the MI355X (there is no CPU meter)"


def _check_meter(meter, device) -> None:
    if meter is not None and (not isinstance(meter, DepthEpochMeter) or meter.sums.device != device):
        raise ValueError("meter must be a rag_amd.depth.DepthEpochMeter on the device of the depth maps")


class SilogMetricsLossFn(torch.autograd.Function):
    """silog_loss as out[0] of the depth-metrics pass (two launches: the loss, the nine compute_errors entries, the saved scalars of
    the backward and, with a meter, its update); the backward is ops.silog_loss_bwd (one launch)."""

    @staticmethod
    def forward(ctx, est, gt, variance_focus, meter):
        saved = torch.empty((3,), device=est.device, dtype=torch.float64)
        out = ops.depth_metrics(est.detach(), gt.detach(), variance_focus, saved=saved, meter=meter.sums if meter is not None else None)
        if meter is not None:
            meter.last = out
        ctx.vf = float(variance_focus)
        ctx.save_for_backward(est, gt, saved)
        return out[0] * 1.0          # a kernel, not a memcpy node (as MaskedSmoothL1Fn)

    @staticmethod
    def backward(ctx, grad):
        est, gt, saved = ctx.saved_tensors
        return ops.silog_loss_bwd(est.detach(), gt, saved, grad, ctx.vf), None, None, None


def silog_metrics_loss(est: torch.Tensor, gt: torch.Tensor, meter: Optional[DepthEpochMeter] = None,
                       variance_focus: float = 0.85) -> torch.Tensor:
    """`silog_loss` of one batch of the unit search (approaches/rag.py:407-427) as a 0-d tensor with a gradient w.r.t. `est`, computed
    by the depth-metrics pass: the same two launches also give compute_errors' nine entries of the batch (`meter.last`) and add all
    ten to `meter` (DepthEpochMeter), where the reference copies both maps to the host.  Bit for bit the loss and the gradient of
    `silog_loss`.  On the CPU `silog_loss_torch`; a meter there raises (there is no CPU meter)."""
    if est.is_cuda:
        _check_meter(meter, est.device)
        return SilogMetricsLossFn.apply(est, gt, float(variance_focus), meter)
    if meter is not None:
        raise RuntimeError(METER_NEEDS_GPU)
    return silog_loss_torch(est, gt, variance_focus)


class Network(_StereoNetwork):
    """rag_depth/src/models/rag_model.py:201-800.  Same constructor, attributes, ModuleList names and state_dict keys as the
    reference; `depth_head` (never grown) and `max_depth = 80` in place of the stereo head."""

    def __init__(self, genotype, device):
        super().__init__(genotype, device, maxdisp=192)
        self.depth_head = DispHead(input_dim=1)
        self.max_depth = MAX_DEPTH

    def _init_matching(self, genotype, maxdisp):
        # rag_model.py:250-298: the stereo Matching-Net layers with their 2-D twins (same attribute names)
        self._step = 3
        self._block_multiplier = 3
        self._filter_multiplier = 4
        self._num_layers_3d = 8
        for name in ("stem_3d0", "stem_3d1", "last_3_3d", "last_6_3d", "last_12_3d"):
            self.length[name] = 1
            self.arch_init[name] = [0]
        self.cells_3d = nn.ModuleList()
        self.stem3d0 = nn.ModuleList([self._new_unit("stem_3d0", genotype)])
        self.stem3d1 = nn.ModuleList([self._new_unit("stem_3d1", genotype)])
        for i in range(self._num_layers_3d):
            self.cells_3d.append(nn.ModuleList([self._new_unit(f"cell_3d{i}", genotype)]))
            self.arch_init[f"cell_3d{i}"] = [0]
            self.length[f"cell_3d{i}"] = 1
        self.last_3_3d = nn.ModuleList([self._new_unit("last_3_3d", genotype)])
        self.last_6_3d = nn.ModuleList([self._new_unit("last_6_3d", genotype)])
        self.last_12_3d = nn.ModuleList([self._new_unit("last_12_3d", genotype)])
        self.maxdisp = maxdisp
        from .modules import Disp
        self.disp = Disp(self.maxdisp)          # the reference builds it too (unused, no parameters)

    def _new_unit(self, name: str, genotype) -> nn.Module:
        fm = 12
        if name in ("stem_3d0", "stem_3d1"):
            return ConvBR_2d(fm, fm, 3, stride=1, padding=1)
        if name.startswith("cell_3d"):
            pp, p, f, du = _CELL3D_ARCH[int(name[7:])]
            return Cell_2d(3, 3, pp, p, genotype, f, du)
        if name == "last_3_3d":
            return ConvBR_2d(fm, 1, 3, 1, 1, bn=False, relu=False)
        if name == "last_6_3d":
            return ConvBR_2d(fm * 2, fm, 1, 1, 0)
        if name == "last_12_3d":
            return ConvBR_2d(fm * 4, fm * 2, 1, 1, 0)
        return super()._new_unit(name, genotype)

    # ------------------------------------------------------------------ inference paths
    def _check_inference(self, x) -> None:
        if self._training_graph(x):
            raise RuntimeError("rag_amd.depth.Network: forward is inference only; call it under torch.no_grad() with the model in "
                               "eval(), or train through Network.forward_train (rag_amd.train.train_step drives it)")
        if self.act_dtype != torch.float32 or x.dtype != torch.float32:
            raise RuntimeError(FP32_ONLY)

    def _trunk(self, x, stem0, stem1, cells, m6, m12, train: bool = False) -> torch.Tensor:
        """stem3d0 -> stem3d1 -> cells (rag_model.py:363-373), then the head's 1x1 part: the input of upsample_6, at (h/2, w/2) or
        already at (h, w) (rag_model.py:378-385).  `train`: the unfused m6(m12(.), resample_to=half) chain, whose units have
        autograd forms (the one-launch 1x1 chain is inference only)."""
        return self._trunk_head(self._trunk_cells(x, stem0, stem1, cells), x.shape[2], x.shape[3], m6, m12, train)

    @staticmethod
    def _trunk_cells(x, stem0, stem1, cells) -> torch.Tensor:
        out = (stem0(x),)
        out = (out[0], stem1(out[0]))
        for c in cells:
            out = c(out[0], out[1])
        return out[-1]

    def _trunk_head(self, last, h: int, w: int, m6, m12, train: bool = False) -> torch.Tensor:
        if last.shape[2] == h:
            return last
        if last.shape[2] == h // 2:
            return m6(last)
        if last.shape[2] != h // 4:
            raise ValueError("rag_amd.depth.Network: feature height must be a multiple of 4 (input H a multiple of 12)")
        half = (1, h // 2, w // 2)
        if train:
            return m6(m12(last), resample_to=half)
        # the stereo head's 1/4-level step on a depth-1 volume (one launch for last_12_3d and last_6_3d's channel mix where it is built)
        last5 = last.unsqueeze(2)
        plan = _plan_head((1, h, w), last5.shape[2:], last.dtype, None, m6, m12, False)
        return _head_quarter(last5, m12, m6, half, plan)[:, :, 0]

    def _head(self, y6, size, m3) -> torch.Tensor:
        if m3.use_bn or m3.relu or m3._geometry() != 3 or m3.conv.out_channels != 1:
            raise NotImplementedError("rag_amd.depth.Network: last_3_3d must be the reference's 3x3 conv without BN / ReLU")
        dh = self.depth_head.conv1
        return ops.depth_head(y6, m3.conv.weight.detach(), dh.weight.detach(), dh.bias.detach(), size, 3, float(self.max_depth))

    def _matching_units(self, task_arch, path):
        def unit(name):
            return task_arch[name][0] if task_arch is not None else None

        cells = []
        for i, cell in enumerate(self.cells_3d):
            arch_cell = None
            if task_arch is not None:
                arch_cell = task_arch[f"cell_3d{i}"][0]
            elif path is not None:
                arch_cell = path[i + 1]
            cells.append(cell[arch_cell])
        return (self.stem3d0[unit("stem_3d0")], self.stem3d1[unit("stem_3d1")], cells, self.last_3_3d[unit("last_3_3d")],
                self.last_6_3d[unit("last_6_3d")], self.last_12_3d[unit("last_12_3d")])

    def matching(self, x, task_arch, path=None):                # rag_model.py:347-389 -> mat [B, 1, h, w]
        self._check_inference(x)
        stem0, stem1, cells, m3, m6, m12 = self._matching_units(task_arch, path)
        y6 = self._trunk(x, stem0, stem1, cells, m6, m12)
        h, w = x.shape[2], x.shape[3]
        u = ops.trilinear3d(y6.unsqueeze(2), (1, h, w), True)
        # last_3_3d on the VALU 3x3x3 form: the 2-D weight is the dz = 1 plane of a 3x3x3 over a depth-1 volume
        key = (m3.stamp(),)
        hit = getattr(m3, "_w5_cache", None)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                wt = m3.conv.weight.detach()
                w5 = torch.zeros(wt.shape[:2] + (3, 3, 3), device=wt.device, dtype=wt.dtype)
                w5[:, :, 1] = wt
            hit = (key, w5)
            m3._w5_cache = hit
        mat = torch.empty((x.shape[0], 1, 1, h, w), device=x.device, dtype=torch.float32)
        ops.conv3d_k3_small(u, hit[1], None, None, False, mat, 0)
        return mat[:, :, 0]

    def forward(self, left, right=None, t=None, task_arch=None, path=None):   # rag_model.py:391-416 (`right` is ignored)
        self._check_inference(left)
        x = self.feature(left, task_arch, path)
        stem0, stem1, cells, m3, m6, m12 = self._matching_units(task_arch, path)
        return self._head(self._trunk(x, stem0, stem1, cells, m6, m12), x.shape[2:], m3)

    def forward_train(self, left, t=None, task_arch=None, path=None):   # rag_model.py:391-416 under autograd (approaches/rag.py:234)
        """The training forward: -> depth [B, 3h, 3w] with an autograd graph through the HIP Functions of rag_amd.autograd and
        `DepthHeadFn`.  BatchNorm uses batch statistics in the units that are in train() and running statistics in the others, as
        the reference's train_epoch (reused units in eval()).  fp32 only."""
        if self.act_dtype != torch.float32 or left.dtype != torch.float32:
            raise RuntimeError("rag_amd.depth.Network: training is fp32 only")
        x = self.feature(left, task_arch, path)
        stem0, stem1, cells, m3, m6, m12 = self._matching_units(task_arch, path)
        y6 = self._trunk(x, stem0, stem1, cells, m6, m12, train=True)
        if m3.use_bn or m3.relu or m3._geometry() != 3 or m3.conv.out_channels != 1:
            raise NotImplementedError("rag_amd.depth.Network: last_3_3d must be the reference's 3x3 conv without BN / ReLU")
        dh = self.depth_head.conv1
        return DepthHeadFn.apply(y6, m3.conv.weight, dh.weight, dh.bias, x.shape[2:], 3, float(self.max_depth))

    def search_forward(self, left, right, t, selected_ops):        # rag_model.py:716-740
        self._check_inference(left)
        x = self.search_feature(left, selected_ops)
        cells = [cell[selected_ops[i + 10]] for i, cell in enumerate(self.cells_3d)]
        y6 = self._trunk(x, self.stem3d0[selected_ops[8]], self.stem3d1[selected_ops[9]], cells, self.last_6_3d[t], self.last_12_3d[t])
        return self._head(y6, x.shape[2:], self.last_3_3d[t])

    def forward_stats(self, *args, **kwargs):
        """The stereo head's statistics do not exist here: the depth head is a sigmoid of one value per pixel, not a distribution."""
        raise NotImplementedError("rag_amd.depth.Network: forward_stats belongs to the stereo head (a softmin over disparities); "
                                  "the depth head has no distribution")

    search_forward_stats = forward_stats

    def forward_mode(self, *args, **kwargs):
        """The stereo head's mode-local disparity does not exist here, for the reason forward_stats gives."""
        raise NotImplementedError("rag_amd.depth.Network: forward_mode belongs to the stereo head (a softmin over disparities); "
                                  "the depth head has no distribution")

    search_forward_mode = forward_mode
    forward_train_stats = forward_stats

    def forward_lr(self, *args, **kwargs):
        """The left-right check needs a second view: the depth network sees the left image only."""
        raise NotImplementedError("rag_amd.depth.Network: forward_lr belongs to the stereo network (a left-right consistency check); "
                                  "the depth network has no second view")

    def forward_dense(self, *args, **kwargs):
        """The dense fill repairs what the left-right check rejects: the depth network has no such check."""
        raise NotImplementedError("rag_amd.depth.Network: forward_dense belongs to the stereo network (it fills what the left-right "
                                  "check rejects); the depth network has no second view")

    def search_forward_train(self, left, t, selected_ops):         # rag_model.py:716-740 under autograd (approaches/rag.py:405)
        """The training forward of a sampled path: `search_forward` on the composition of `forward_train`, -> depth [B, 3h, 3w] with
        an autograd graph.  The module modes are the caller's (`search_mode()`: the trunk's BatchNorms on running statistics, the
        heads of task t on batch statistics).  When no selected trunk unit has a parameter that requires grad (a path that reuses
        every unit) the trunk runs without a graph, on the inference forms up to the last cell's output, and only the head's tensors
        train.  fp32 only."""
        if self.act_dtype != torch.float32 or left.dtype != torch.float32:
            raise RuntimeError("rag_amd.depth.Network: training is fp32 only")
        sel = self.check_selected(t, selected_ops)
        trunk = [self._units(name)[idx] for name, idx in zip(self._p_layers(), sel)]
        graph = torch.is_grad_enabled() and (left.requires_grad or any(p.requires_grad for u in trunk for p in u.forward_parameters()))
        with torch.set_grad_enabled(graph):
            x = self.search_feature(left, sel)
            last = self._trunk_cells(x, trunk[8], trunk[9], trunk[10:])
        m3, m6, m12 = self.last_3_3d[int(t)], self.last_6_3d[int(t)], self.last_12_3d[int(t)]
        y6 = self._trunk_head(last, x.shape[2], x.shape[3], m6, m12, train=True)
        if m3.use_bn or m3.relu or m3._geometry() != 3 or m3.conv.out_channels != 1:
            raise NotImplementedError("rag_amd.depth.Network: last_3_3d must be the reference's 3x3 conv without BN / ReLU")
        dh = self.depth_head.conv1
        return DepthHeadFn.apply(y6, m3.conv.weight, dh.weight, dh.bias, x.shape[2:], 3, float(self.max_depth))

    def active_parameters(self, t, selected_ops) -> list:
        """The stereo network's set (the selected units and the heads of task t, those that require grad), and the depth head's
        conv1 weight and bias when they require grad (after freeze_model + modify_param(new_models) they do not: `depth_head` is in
        no model list, rag_model.py:553-638)."""
        dh = self.depth_head.conv1
        return super().active_parameters(t, selected_ops) + [p for p in (dh.weight, dh.bias) if p.requires_grad]


DepthNetwork = Network


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def rows_from_keys(keys, prefix: str) -> np.ndarray:
    """STAND-IN genotype rows of one cell unit from its state_dict keys: [[0,p0],[1,p1],[2,p2],[3,p3],[5,p4],[6,p5]] with pj = 1 when
    positional op j has a convolution.  The reference never recorded the searched branches (upstream writes them to tensorboard
    text only), so these rows reproduce the checkpoint's op TYPES, not necessarily its branch wiring."""
    keys = set(keys)
    branches = ALL_CONV_ROWS[:, 0]
    return np.array([[int(br), int(f"{prefix}_ops.{j}.conv.weight" in keys)] for j, br in enumerate(branches)])


def genotypes_from_keys(keys) -> Dict[str, List[np.ndarray]]:
    """{layer: [stand-in rows per unit]} for every cell layer of a depth state_dict (see `rows_from_keys`)."""
    counts = _unit_counts(keys)
    out = {}
    for name, n in counts.items():
        if name.startswith("cell_"):
            attr = "cells_2d" if name.startswith("cell_2d") else "cells_3d"
            out[name] = [rows_from_keys(keys, f"{attr}.{name[7:]}.{idx}.") for idx in range(n)]
    return out


def _geno(g) -> Genotype:
    if isinstance(g, (np.ndarray, list, tuple)) and not hasattr(g, "normal"):
        rows = np.asarray(g)
        return Genotype(normal=rows, normal_concat=None, reduce=rows, reduce_concat=None)
    return _genotype(g)


def load_depth_checkpoint(src: Union[str, dict], device="cuda", genotypes: Union[None, str, dict] = None,
                          archis: Optional[Sequence[dict]] = None):
    """-> (depth Network in eval mode on `device`, archis) from the reference's ``{'task', 'model', 'optimizer'}`` file
    (rag_depth/src/run.py) or a dict holding ``model``.  The file is read with ``weights_only=True`` and the state_dict loaded strictly.

    The reference checkpoint records no genotypes.  `genotypes`: ``{layer: [rows or Genotype per unit]}`` for every cell layer, or
    ``"from_keys"`` for the stand-in rows of `rows_from_keys` (they reproduce each unit's conv / identity op types from the key
    names, NOT necessarily the searched branch wiring, which upstream never saved).  Every cell is checked against its keys (ValueError
    on a mismatch).  `archis`: per-task architecture dicts; None gives ``[net.arch_init]``."""
    data = torch.load(src, map_location="cpu", weights_only=True) if not isinstance(src, dict) else src
    sd = data["model"] if "model" in data else data
    keys = set(sd.keys())
    counts = _unit_counts(keys)
    if genotypes is None:
        raise ValueError("load_depth_checkpoint: the reference checkpoint records no genotypes; pass genotypes= (rows per unit, or "
                         "'from_keys')")
    if isinstance(genotypes, str):
        if genotypes != "from_keys":
            raise ValueError(f"load_depth_checkpoint: genotypes must be a dict or 'from_keys', got {genotypes!r}")
        genotypes = genotypes_from_keys(keys)

    def geno(name: str, idx: int) -> Genotype:
        return _geno(genotypes[name][idx]) if isinstance(genotypes, dict) else _geno(genotypes)

    first = geno("cell_3d0", 0)
    net = Network(first, "cpu")
    for name in net._p_layers() + list(_HEADS):
        units = net._units(name)
        want = counts.get(name, 1)
        if name.startswith("cell_"):
            units[0] = net._new_unit(name, geno(name, 0))
        for idx in range(1, want):
            units.append(net._new_unit(name, geno(name, idx) if name.startswith("cell_") else first))
        if name not in _HEADS:
            net.length[name] = want
    for name in net._p_layers():
        if name.startswith("cell_"):
            attr = "cells_2d" if name.startswith("cell_2d") else "cells_3d"
            for idx, unit in enumerate(net._units(name)):
                _check_cell_pattern(unit, f"{attr}.{name[7:]}.{idx}.", keys, name, idx)
    net.load_state_dict(sd, strict=True)
    out_archis = list(archis) if archis is not None else [net.arch_init]
    for t, a in enumerate(out_archis):
        for name, (k, *_rest) in a.items():
            if int(k) >= len(net._units(name)):
                raise ValueError(f"load_depth_checkpoint: archis[{t}][{name!r}] = {k} but the checkpoint has "
                                 f"{len(net._units(name))} unit(s)")
    return net.to(device).eval(), [dict(a) for a in out_archis]


# ---------------------------------------------------------------------------------------------------------------- metrics
class DepthMetrics:
    """Result of `depth_metrics`: `.tensor` is the 10-float device vector (DEPTH_NAMES order); `[name]` gives a 0-d device tensor;
    `floats()` copies once to the host."""

    def __init__(self, tensor: torch.Tensor):
        self.tensor = tensor

    def __getitem__(self, name: str) -> torch.Tensor:
        return self.tensor[DEPTH_NAMES.index(name)]

    def floats(self) -> Dict[str, float]:
        return dict(zip(DEPTH_NAMES, self.tensor.tolist()))      # the only synchronisation


def depth_metrics(depth_est: torch.Tensor, depth_gt: torch.Tensor, variance_focus: float = 0.85,
                  meter: Optional[DepthEpochMeter] = None) -> DepthMetrics:
    """silog_loss + compute_errors of the depth eval loop (approaches/rag.py:440-489) over the pixels with gt > 0 of the whole batch,
    on the device, without the boolean gather or the per-batch D2H copy; no gradient.  `meter` (DepthEpochMeter): the same launch
    also adds the batch to it."""
    if isinstance(meter, DepthEpochMeter) and not depth_est.is_cuda:
        raise RuntimeError(METER_NEEDS_GPU)
    _check_meter(meter, depth_est.device)
    with torch.no_grad():
        out = ops.depth_metrics(depth_est.detach(), depth_gt.detach(), variance_focus, meter=meter.sums if meter is not None else None)
    if meter is not None:
        meter.last = out
    return DepthMetrics(out)


# ---------------------------------------------------------------------------------------------------------------- plain-torch twins
def depth_head_torch(y, w3, w1, b1, size: Sequence[int], scale: int = 3, max_depth: float = 80.0) -> torch.Tensor:
    """Plain-torch restatement of ops.depth_head in the dtype and on the device of its inputs (CPU twin and ATen yardstick)."""
    import torch.nn.functional as F
    u = F.interpolate(y, size=tuple(int(v) for v in size), mode="bilinear", align_corners=True)
    m = F.conv2d(u, w3, padding=1)
    s = torch.sigmoid(F.conv2d(m, w1, b1, padding=1))
    if scale > 1:
        s = F.interpolate(s, scale_factor=scale, mode="bilinear", align_corners=False)
    return s[:, 0] * max_depth


def depth_metrics_torch(est: torch.Tensor, gt: torch.Tensor, variance_focus: float = 0.85) -> torch.Tensor:
    """Plain-torch restatement of ops.depth_metrics: per-pixel terms in the inputs' dtype, means in float64."""
    mask = gt > 0
    e, g = est[mask], gt[mask]
    d = torch.log(e) - torch.log(g)
    diff = g - e
    th = torch.maximum(g / e, e / g)
    mean = lambda t: t.double().mean()  # noqa: E731
    md, md2 = mean(d), mean(d * d)
    out = [torch.sqrt(md2 - variance_focus * md * md) * 10.0, torch.sqrt(md2 - md * md) * 100.0, mean(diff.abs() / g),
           mean((torch.log10(e) - torch.log10(g)).abs()), torch.sqrt(mean(diff * diff)), mean(diff * diff / g), torch.sqrt(md2),
           mean((th < 1.25).to(e.dtype)), mean((th < 1.25 ** 2).to(e.dtype)), mean((th < 1.25 ** 3).to(e.dtype))]
    return torch.stack(out)
