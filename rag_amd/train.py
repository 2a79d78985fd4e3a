"""Host side of the training step (BASELINE config 5; reference: approaches/rag.py:155-219, Appr.train_epoch).

One step = forward (HIP) -> masked smooth-L1 -> backward (HIP, rag_amd.autograd) -> gradient all-reduce ->
clip_grad_norm_ -> SGD.  Data-parallel replicas (one process per GPU) exchange gradients as ONE flat fp32
bucket: the `.grad` of every trainable parameter is a view into `GradBucket.flat`, so autograd accumulates
straight into the buffer RCCL reduces — no pack/unpack copies and a single collective per step (the message is
< 1 MB, i.e. latency-bound on xGMI: one call is what matters).  Train-mode BatchNorm keeps
per-replica statistics, like the single-GPU reference per replica.

The cell search's step (automl/mdenas_search.py:161-173 of both trees) is the same sequence on a supernet with one sampled
operation per edge: `sampled_ops=(fea_ops, mat_ops)`.  Only the sampled operations receive gradients and torch.optim.SGD skips a
parameter whose .grad is None, so that step updates `net.active_parameters(fea_ops, mat_ops)` alone (FlatSGD.set_active).

The unit search's step (Appr.search_epoch / search_eval of approaches/rag.py:344-406, 443-470, run for every task t > 0) is the same
sequence again on the expanded `Network` with one sampled unit per layer: `selected_ops=[unit per layer of p], t=<task>`.  The forward
is `net.search_forward`, the update reaches `net.active_parameters(t, selected_ops)` alone, and `meter=` (rag_amd.metrics.EpochMeter)
makes the loss launch the epoch meter's update.  The module modes are the caller's (`net.search_mode()`), and so are the sampling
from `p`, h_e / h_a and the probability update.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence

import torch
import torch.nn.functional as F


class GradBucket:
    """All trainable parameters' gradients as views of one flat buffer (`requires_grad` is read at construction:
    build it after `freeze_model` / `modify_param`, rag.py:101-102)."""

    def __init__(self, params: Iterable[torch.nn.Parameter]):
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("GradBucket: no trainable parameters")
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(n, device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            p._ragmi_direct = True          # rag_amd.autograd accumulates into these views in place (no AccumulateGrad adds)
            off += p.numel()

    def zero(self) -> None:
        """optimizer.zero_grad() that keeps the views (rag.py:213)."""
        self.flat.zero_()
        for p, g in zip(self.params, self._views()):
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g

    def _views(self):
        off = 0
        for p in self.params:
            yield self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()

    def all_reduce_mean(self, dist=None) -> None:
        """Sum over replicas in one collective, then divide by the world size.  A one-rank group still issues the collective
        (the identity): a single-GPU run of a distributed job exercises the same RCCL path as the 8-GPU one."""
        if dist is not None and dist.is_initialized():
            dist.all_reduce(self.flat)
            if dist.get_world_size() > 1:
                self.flat.div_(dist.get_world_size())

    def clip_(self, max_norm: float) -> torch.Tensor:
        """torch.nn.utils.clip_grad_norm_ over the bucket (rag.py:215); returns the total norm."""
        total = torch.linalg.vector_norm(self.flat)
        self.flat.mul_(torch.clamp(max_norm / (total + 1e-6), max=1.0))
        return total


def masked_smooth_l1(disp: torch.Tensor, gt: torch.Tensor, maxdisp: int, meter=None) -> torch.Tensor:
    """F.smooth_l1_loss(disp[mask], gt[mask]) with mask = 0 < gt < maxdisp (rag.py:210-211) without the boolean gather
    (no stream synchronisation): the fused HIP loss of rag_amd.metrics on the GPU.  `meter` (rag_amd.metrics.EpochMeter, GPU only):
    the same launch adds the batch's loss and metrics to it."""
    if disp.is_cuda:
        from .metrics import masked_smooth_l1 as fused
        return fused(disp, gt, maxdisp, meter)
    if meter is not None:
        raise RuntimeError("an EpochMeter is updated by the HIP loss launch: it needs the MI355X (there is no CPU meter)")
    mask = ((gt < maxdisp) & (gt > 0)).to(disp.dtype)          # host-side twin (CPU tests of the step logic)
    per = F.smooth_l1_loss(disp, gt, reduction="none")
    return (per * mask).sum() / mask.sum()


def self_supervised_loss(disp: torch.Tensor, left: torch.Tensor, right: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """re_and_sm_loss(disp, left, right) of src_self/models/loss.py:112-141, the loss of the supervise=False step
    (src_self/approaches/rag.py:270-278): the fused HIP loss of rag_amd.metrics on the GPU.  `weight` [B,H,W]: its weighted form
    (rag_amd.metrics.re_and_sm_loss), the loss of the occlusion=True step."""
    if disp.is_cuda:
        from .metrics import re_and_sm_loss as fused
        return fused(disp, left, right, weight)
    from .metrics import re_and_sm_loss_torch           # host-side twin (CPU tests of the step logic)
    return re_and_sm_loss_torch(disp, left, right, weight)[0]


def uncertainty_loss(disp: torch.Tensor, stats: torch.Tensor, gt: torch.Tensor, maxdisp: int, var_floor: float = 1.0 / 12.0) -> torch.Tensor:
    """The uncertainty-aware loss of rag_amd.metrics over the head's own variance (disp, stats of a forward_train_stats call): the
    fused HIP loss on the GPU, its plain-torch twin on CPU tensors."""
    from .metrics import uncertainty_loss as fused
    return fused(disp, stats, gt, maxdisp, var_floor)


def _check_uncertainty(uncertainty: bool, net, supervise: bool, sampled_ops, selected_ops, meter) -> None:
    """Argument checks of uncertainty=True, before any launch."""
    if not uncertainty:
        return
    if not supervise:
        raise ValueError("uncertainty=True trains on the ground truth: supervise=False is refused")
    if sampled_ops is not None:
        raise ValueError("uncertainty=True is built for the grown stereo Network and a MatchingNet on features: sampled_ops (the cell "
                         "search's supernet) is refused")
    if selected_ops is not None:
        raise ValueError("uncertainty=True is built for the grown stereo Network and a MatchingNet on features: selected_ops (the unit "
                         "search) is refused")
    if _is_depth(net) or _supernet_kind(net) is not None:
        raise ValueError("uncertainty=True needs the stereo head's distribution: a depth network or a supernet is refused")
    if meter is not None:
        raise ValueError("uncertainty=True: an EpochMeter is fed by the masked smooth-L1 launch, which this step does not run: meter is "
                         "refused")


def _check_occlusion(occlusion: bool, net, supervise: bool, features: bool, sampled_ops, selected_ops, uncertainty: bool, meter,
                     lr_tol, occluded_weight) -> None:
    """Argument checks of occlusion=True, before any launch."""
    if not occlusion:
        return
    if supervise:
        raise ValueError("occlusion=True weights the self-supervised loss: supervise=True is refused")
    if features:
        raise ValueError("occlusion=True needs the images (it stacks and mirrors them): features=True is refused")
    if sampled_ops is not None:
        raise ValueError("occlusion=True is built for the grown stereo Network: sampled_ops (the cell search's supernet) is refused")
    if selected_ops is not None:
        raise ValueError("occlusion=True is built for the grown stereo Network: selected_ops (the unit search) is refused")
    if uncertainty:
        raise ValueError("occlusion=True and uncertainty=True are two different losses: their combination is refused")
    if meter is not None:
        raise ValueError("occlusion=True: an EpochMeter is fed by the masked smooth-L1 launch, which this step does not run: meter is "
                         "refused")
    if _is_depth(net) or _supernet_kind(net) is not None:
        raise ValueError("occlusion=True needs a second view: a depth network or a supernet is refused")
    import math
    if len(lr_tol) != 2 or not all(math.isfinite(v) and v >= 0 for v in lr_tol):
        raise ValueError(f"occlusion=True: lr_tol must be (abs_tol, rel_tol), finite and non-negative, got {lr_tol!r}")
    if not (math.isfinite(occluded_weight) and 0 <= occluded_weight <= 1):
        raise ValueError(f"occlusion=True: occluded_weight must lie in [0, 1], got {occluded_weight!r}")


def _is_depth(net) -> bool:
    from .depth import Network as DepthNetwork
    return isinstance(net, DepthNetwork)


def _supernet_kind(net) -> Optional[str]:
    from .supernet import BasicNetwork, DepthBasicNetwork
    return "depth" if isinstance(net, DepthBasicNetwork) else "stereo" if isinstance(net, BasicNetwork) else None


def _check_sampled(net, sampled_ops, gt, task_arch, features: bool, supervise: bool) -> Optional[str]:
    """Argument checks of the sampled-op step, before any launch.  -> "stereo" / "depth" when `sampled_ops` is given, else None."""
    kind = _supernet_kind(net)
    if sampled_ops is None:
        if kind is not None:
            raise ValueError("a supernet runs one sampled operation per edge: pass sampled_ops=(fea_ops, mat_ops)")
        return None
    if kind is None:
        raise ValueError("sampled_ops is the cell search's step: net must be rag_amd.BasicNetwork or rag_amd.DepthBasicNetwork")
    if len(sampled_ops) != 2:
        raise ValueError("sampled_ops must be the pair (fea_ops, mat_ops)")
    if task_arch is not None or features or not supervise:
        raise ValueError("sampled_ops: a supernet has no units to choose (task_arch), takes images (features=True is refused) and "
                         "trains supervised (supervise=False is refused)")
    if gt is None:
        raise ValueError("sampled_ops: the search step needs the ground truth gt (disparity, or depth in metres with 0 = invalid)")
    return kind


def _check_selected(net, selected_ops, t, gt, sampled_ops=None, task_arch=None, features: bool = False,
                    supervise: bool = True) -> Optional[List[int]]:
    """Argument checks of the unit-search step, before any launch.  -> selected_ops as a list of ints, or None without it."""
    if selected_ops is None:
        if t is not None:
            raise ValueError("t is the head index of the unit search's step: it goes with selected_ops")
        return None
    if sampled_ops is not None or task_arch is not None or features or not supervise:
        raise ValueError("selected_ops: the unit search runs search_forward on the images and trains supervised: sampled_ops, "
                         "task_arch, features=True and supervise=False are refused")
    if _is_depth(net):
        raise ValueError("selected_ops: the depth network's unit search is not built into this entry point: use "
                         "rag_amd.depth_search_step / depth_search_eval_step / DepthGraphedSearchStep")
    from .network import Network
    if not isinstance(net, Network):
        raise ValueError("selected_ops is the unit search's step: net must be the stereo rag_amd.Network (after expand)")
    if t is None:
        raise ValueError("selected_ops: the step needs the task index t (the head it trains)")
    if gt is None:
        raise ValueError("selected_ops: the step needs the ground-truth disparity gt")
    return net.check_selected(t, selected_ops)


def _check_meter(meter, net, supervise: bool) -> None:
    if meter is not None and (not supervise or _is_depth(net) or _supernet_kind(net) == "depth"):
        raise ValueError("meter: an EpochMeter is fed by the masked smooth-L1 launch of the supervised stereo steps only")


def _check_supervision(gt, features: bool, supervise: bool, depth: bool = False) -> None:
    if depth:
        if not supervise or features:
            raise ValueError("a depth network trains on silog_loss(depth, gt) from the left image only: supervise=False and "
                             "features=True are refused")
        if gt is None:
            raise ValueError("the depth training step needs the ground-truth depth gt (metres, 0 = invalid)")
        return
    if not supervise and features:
        raise ValueError("supervise=False needs the images (the loss warps the right image onto the left): features=True is refused")
    if supervise and gt is None:
        raise ValueError("supervise=True needs the ground-truth disparity gt")


TRAIN_PRECISION = "fp32"     # the reference's training step is fp32 (rag.py:204-216); "f16x3" is opt-in (~6 % of the step)


def forward_backward(net, bucket: GradBucket, left, right, gt, *, task_arch=None, features: bool = False,
                     precision: Optional[str] = None, supervise: bool = True, sampled_ops: Optional[Sequence] = None,
                     selected_ops: Optional[Sequence] = None, t: Optional[int] = None, meter=None, uncertainty: bool = False,
                     var_floor: float = 1.0 / 12.0, occlusion: bool = False, lr_tol: Sequence[float] = (1.0, 0.0),
                     occluded_weight: float = 0.0):
    """forward -> masked smooth-L1 -> zero the bucket -> backward (rag.py:208-214).  A depth network (rag_amd.depth.Network):
    Network.forward_train(left) -> silog_loss(depth, gt) with gt the ground-truth depth in metres (0 = invalid) as in
    rag_depth/src/approaches/rag.py:232-242; `right` may be None.  `supervise=False`: the self-supervised loss
    re_and_sm_loss(disp, left, right) of src_self (approaches/rag.py:270-278) instead, `gt` may be None, and left/right must be
    the images (features=True raises ValueError).  `features=True`: `net` is a
    MatchingNet and left/right are Feature-Net outputs.  `precision`: arithmetic of the 3x3x3 convolutions of the step (forward and
    data gradient): "fp32" (default, TRAIN_PRECISION: every contraction on the fp32-input MFMA forms, the reference's arithmetic
    class) or "f16x3" (opt-in; bound in include/rag_amd.h).  `sampled_ops=(fea_ops, mat_ops)`: `net` is a supernet
    (rag_amd.BasicNetwork / DepthBasicNetwork) and the step is the cell search's (automl/mdenas_search.py:161-173): forward
    net(left, right, fea_ops, mat_ops), masked smooth-L1 against net.maxdisp for the stereo supernet, silog_loss (gt > 0) for the
    depth one; task_arch, features=True and supervise=False are refused, and so is a supernet without sampled_ops.
    `selected_ops=[unit per layer of p], t=<task>`: `net` is the expanded stereo Network and the step is the unit search's
    (rag.py:371-382): forward net.search_forward(left, right, t, selected_ops), masked smooth-L1 against net.maxdisp; the module
    modes are the caller's (net.search_mode()); sampled_ops, task_arch, features=True, supervise=False, another kind of net, a
    missing t or gt, a wrong length and an index outside its list are refused.  `meter` (rag_amd.metrics.EpochMeter): the masked
    smooth-L1 launch also adds this batch to the epoch's meter (rag.py:386-396 scores the disp_est it trained on).
    `uncertainty=True` (the grown stereo Network, or a MatchingNet with features=True; supervised): forward_train_stats in place of
    forward and rag_amd.metrics.uncertainty_loss(disp, stats, gt, net.maxdisp, var_floor) in place of the masked smooth-L1, so the
    variance the head reports is trained; supervise=False, sampled_ops, selected_ops, a depth network and a meter are refused.
    `occlusion=True` (with supervise=False, the grown stereo Network on images): the occlusion-aware form of the self-supervised
    step.  The batch is stacked with its mirrored right-camera view (rag_amd.metrics.lr_stack), ONE forward runs on the 2B pairs
    (train-mode BatchNorm statistics are those of the 2B batch), the detached disparities are checked against each other
    (lr_consistency(D, D, *lr_tol, occluded_weight, mirrored=True, partner_shift=B)) and the loss is
    re_and_sm_loss(D, left2, right2, weight=check.weight) over all 2B pairs: both views train, and a pixel that is occluded in the
    other view or whose disparity disagrees with it counts `occluded_weight` in the photometric terms (the smoothness term fills
    it).  supervise=True, features=True, sampled_ops, selected_ops, uncertainty, a meter and a depth network are refused.
    Returns the (detached) loss."""
    _check_occlusion(occlusion, net, supervise, features, sampled_ops, selected_ops, uncertainty, meter, lr_tol, occluded_weight)
    _check_uncertainty(uncertainty, net, supervise, sampled_ops, selected_ops, meter)
    sel = _check_selected(net, selected_ops, t, gt, sampled_ops, task_arch, features, supervise)
    kind = _check_sampled(net, sampled_ops, gt, task_arch, features, supervise)
    depth = _is_depth(net)
    if kind is None and sel is None:
        _check_supervision(gt, features, supervise, depth)
    _check_meter(meter, net, supervise)
    from . import ops
    with ops.conv_precision(precision or TRAIN_PRECISION):
        if sel is not None:
            loss = masked_smooth_l1(net.search_forward(left, right, int(t), sel), gt, net.maxdisp, meter)
        elif kind is not None:
            out = net(left, right, sampled_ops[0], sampled_ops[1])
            if kind == "depth":
                from .depth import silog_loss
                loss = silog_loss(out, gt)
            else:
                loss = masked_smooth_l1(out, gt, net.maxdisp, meter)
        elif depth:
            from .depth import silog_loss
            loss = silog_loss(net.forward_train(left, 0, task_arch if task_arch is not None else net.arch_init), gt)
        elif uncertainty:
            res = net.forward_train_stats(left, right, task_arch) if features else \
                net.forward_train_stats(left, right, 0, task_arch if task_arch is not None else net.arch_init)
            loss = uncertainty_loss(res.disp, res.tensor, gt, net.maxdisp, var_floor)
        elif occlusion:
            from .metrics import lr_consistency, lr_stack
            left2, right2 = lr_stack(left, right)
            disp = net(left2, right2, 0, task_arch if task_arch is not None else net.arch_init)
            seen = disp.detach()
            chk = lr_consistency(seen, seen, float(lr_tol[0]), float(lr_tol[1]), float(occluded_weight), mirrored=True,
                                 partner_shift=left.shape[0], want_error=False)
            loss = self_supervised_loss(disp, left2, right2, chk.weight)
        else:
            disp = net(left, right, task_arch) if features else net(left, right, 0, task_arch if task_arch is not None else net.arch_init)
            loss = masked_smooth_l1(disp, gt, net.maxdisp, meter) if supervise else self_supervised_loss(disp, left, right)
        bucket.zero()
        loss.backward()
    return loss.detach()


class FlatSGD:
    """torch.optim.SGD(lr, momentum, weight_decay) of rag.py:64-70 over a GradBucket, with the parameters themselves moved
    into one flat buffer next to the flat gradient: clip_grad_norm_ + step is then ONE pair of HIP launches
    (ragmi_sgd_clip_step) instead of torch's multi-tensor launches over ~500 small tensors.  GPU only (no CPU fallback: on
    the CPU use torch.optim.SGD via make_optimizer).  `param_groups[0]["lr"]` may be changed between steps like torch's.

    `set_active(params)`: the following steps update those parameters only (ragmi_sgd_clip_step_masked), as torch.optim.SGD does
    when the .grad of every other parameter is None - no weight decay and no momentum on them, the norm over the active gradients,
    and an unsampled parameter's momentum starts at its own first update (the momentum buffer starts at zero, which gives exactly
    torch's lazily created buffer).  The choice holds until the next call; `set_active(None)` goes back to the whole buffer."""

    def __init__(self, bucket: GradBucket, lr: float = 1e-3, momentum: float = 0.9, weight_decay: float = 3e-3):
        if not bucket.flat.is_cuda:
            raise RuntimeError("FlatSGD runs on the MI355X only; use make_optimizer (torch.optim.SGD) for CPU tensors")
        self.bucket = bucket
        self.param_groups = [dict(params=bucket.params, lr=lr, momentum=momentum, weight_decay=weight_decay)]
        self.flat = torch.empty_like(bucket.flat)
        off = 0
        for p in bucket.params:                       # parameters become views of one buffer (values kept)
            v = self.flat[off:off + p.numel()].view_as(p)
            v.copy_(p.detach())
            p.data = v
            off += p.numel()
        self.momentum_buffer = torch.zeros_like(self.flat)
        self.steps = 0
        from . import ops
        self._ops = ops
        self._ws = torch.empty((ops.load_library().ragmi_sgd_workspace_bytes() // 4,), device=self.flat.device, dtype=torch.float32)
        self.total_norm = torch.zeros((1,), device=self.flat.device, dtype=torch.float32)
        self._offsets = {}
        off = 0
        for p in bucket.params:
            self._offsets[id(p)] = (off, p.numel())
            off += p.numel()
        self._active_key, self._active_mask = None, None

    def set_active(self, params: Optional[Iterable[torch.nn.Parameter]]) -> None:
        """Restrict the following steps to `params` (each must be in the bucket); None: every parameter again.  The byte mask is
        built on the host and copied to the device once per call (a repeated call with the same parameters keeps the mask)."""
        if params is None:
            self._active_key, self._active_mask = None, None
            return
        key = tuple(sorted(id(p) for p in params))
        if key == self._active_key:
            return
        import numpy as np
        mask = np.zeros((self.flat.numel(),), dtype=np.uint8)
        for i in key:
            if i not in self._offsets:
                raise ValueError("FlatSGD.set_active: a parameter that is not in the optimizer's GradBucket")
            off, n = self._offsets[i]
            mask[off:off + n] = 1
        self._active_key, self._active_mask = key, torch.from_numpy(mask).to(self.flat.device)

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.bucket.zero()

    def step(self, clip: float = 0.0) -> torch.Tensor:
        """clip_grad_norm_(clip) (clip <= 0: none) + SGD step; returns the pre-clip total gradient norm (device tensor)."""
        g = self.param_groups[0]
        if self._active_mask is not None:
            self._ops.sgd_clip_step_masked(self.flat, self.bucket.flat, self.momentum_buffer, self._active_mask, g["lr"], g["momentum"],
                                           g["weight_decay"], clip, self._ws, self.total_norm)
        else:
            self._ops.sgd_clip_step(self.flat, self.bucket.flat, self.momentum_buffer, g["lr"], g["momentum"], g["weight_decay"], clip,
                                    self.steps == 0 or g["momentum"] == 0.0, self._ws, self.total_norm)
        self.steps += 1
        torch.autograd.graph.increment_version(self.bucket.params)       # packed-weight caches key on ._version
        return self.total_norm

    def state_dict(self):
        return {"momentum_buffer": self.momentum_buffer.clone(), "steps": self.steps,
                "param_groups": [{k: v for k, v in self.param_groups[0].items() if k != "params"}]}

    def load_state_dict(self, sd) -> None:
        self.momentum_buffer.copy_(sd["momentum_buffer"])
        self.steps = int(sd["steps"])
        self.param_groups[0].update(sd["param_groups"][0])


def exchange_and_update(optimizer, bucket: GradBucket, *, clip: float = 5.0, dist=None,
                        active: Optional[Sequence[torch.nn.Parameter]] = None) -> None:
    """gradient all-reduce (mean over replicas) -> clip_grad_norm_ -> optimizer step (rag.py:215-216).  `active` (the sampled-op
    step): only these parameters are updated; the others and their momentum state stay bit for bit.  FlatSGD masks its fused
    launch; for a torch optimizer the inactive parameters' .grad is None during optimizer.step() (their bucket slices are all
    zero after the backward, so the clipping norm is already the active one) and the bucket's views are put back after it."""
    bucket.all_reduce_mean(dist)
    if isinstance(optimizer, FlatSGD):
        if active is not None:
            optimizer.set_active(active)
        optimizer.step(clip)
        return
    bucket.clip_(clip)
    if active is None:
        optimizer.step()
        return
    keep = {id(p) for p in active}
    idle = [(p, p.grad) for p in bucket.params if id(p) not in keep]
    for p, _g in idle:
        p.grad = None
    optimizer.step()
    for p, g in idle:
        p.grad = g


def _active_of(net, sampled_ops, selected_ops, t) -> Optional[list]:
    """The parameters the step updates: the sampled operations' / the sampled path's, or None (all of the bucket)."""
    if selected_ops is not None:
        return net.active_parameters(t, selected_ops)
    return net.active_parameters(*sampled_ops) if sampled_ops is not None else None


def search_eval_step(net, left, right, gt, t, selected_ops, meter=None):
    """One batch of Appr.search_eval (rag.py:448-466): stereo_metrics(net.search_forward(left, right, t, selected_ops), gt,
    net.maxdisp) under no_grad, with `net` in eval() (the caller's, as in rag.py:445; a net in training mode is refused); `meter`
    (rag_amd.metrics.EpochMeter) takes the batch in the same launch.  The argument checks of the training step's selected_ops."""
    sel = _check_selected(net, selected_ops, t, gt)
    if net.training:
        raise ValueError("search_eval_step: net must be in eval() (Appr.search_eval, rag.py:445)")
    from .metrics import stereo_metrics
    with torch.no_grad():
        return stereo_metrics(net.search_forward(left, right, int(t), sel), gt, net.maxdisp, meter=meter)


def train_step(net, optimizer, bucket: GradBucket, left, right, gt, *, task_arch=None, clip: float = 5.0, dist=None,
               features: bool = False, precision: Optional[str] = None, supervise: bool = True,
               sampled_ops: Optional[Sequence] = None, selected_ops: Optional[Sequence] = None, t: Optional[int] = None, meter=None,
               uncertainty: bool = False, var_floor: float = 1.0 / 12.0, occlusion: bool = False, lr_tol: Sequence[float] = (1.0, 0.0),
               occluded_weight: float = 0.0):
    """One optimisation step as in Appr.train_epoch (rag.py:204-216); `precision`, `supervise`, `sampled_ops`, `selected_ops` / `t`,
    `meter`, `uncertainty` / `var_floor` and `occlusion` / `lr_tol` / `occluded_weight` as in forward_backward (defaults: fp32, supervised, a grown network).  With `sampled_ops`
    the optimizer updates net.active_parameters(*sampled_ops) only (exchange_and_update), with `selected_ops` (one batch of
    Appr.search_epoch, rag.py:371-396) net.active_parameters(t, selected_ops).  Returns the (detached) loss."""
    loss = forward_backward(net, bucket, left, right, gt, task_arch=task_arch, features=features, precision=precision,
                            supervise=supervise, sampled_ops=sampled_ops, selected_ops=selected_ops, t=t, meter=meter,
                            uncertainty=uncertainty, var_floor=var_floor, occlusion=occlusion, lr_tol=lr_tol,
                            occluded_weight=occluded_weight)
    active = _active_of(net, sampled_ops, selected_ops, t)
    exchange_and_update(optimizer, bucket, clip=clip, dist=dist, active=active)
    return loss


def graph_census(graph: "torch.cuda.CUDAGraph") -> dict:
    """Node counts {kernel, memcpy, memset, other} of a captured hipGraph (ragmi_graph_node_census: hipGraphGetNodes /
    hipGraphNodeGetType).  `graph` must have been created with keep_graph=True and not yet released.  A graph that holds memcpy
    or memset nodes is not replay-safe on this runtime when null-stream copies run between replays."""
    import ctypes
    from ._lib import check, load_library
    n = [ctypes.c_int32() for _ in range(4)]
    check(load_library().ragmi_graph_node_census(graph.raw_cuda_graph(), *[ctypes.byref(v) for v in n]), "graph_node_census")
    return dict(zip(("kernel", "memcpy", "memset", "other"), (v.value for v in n)))


class _GraphedStep:
    """What GraphedTrainStep and rag_amd.depth_search.DepthGraphedSearchStep share: warm-up steps on a side stream, the capture of
    forward + loss + backward, the node census that refuses memcpy / memset nodes, and the replay followed by the eager update.  A
    subclass sets net, opt, bucket, clip, dist and _active, then calls `_capture(run, warmup)` with `run()` = its forward_backward
    on its static input buffers."""

    def _capture(self, run, warmup: int) -> None:
        net, name = self.net, type(self).__name__
        self.first_loss = None                         # loss of the first warm-up step (a real step on the given batch)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                  # warm-up on a side stream: lazy state (allocator pools, occupancy
            for _ in range(max(warmup, 1)):            # queries, momentum buffers) exists before capture
                loss = run()
                exchange_and_update(self.opt, self.bucket, clip=self.clip, dist=self.dist, active=self._active)
                if self.first_loss is None:
                    self.first_loss = loss
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph(keep_graph=True)     # keep the hipGraph_t: its nodes are inspected below
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):   # RCCL's watchdog thread must not trip it
            self.loss = run()
        self.node_census = self._census()
        if self.node_census["memcpy"] or self.node_census["memset"]:
            raise RuntimeError(
                f"{name}: the captured step holds {self.node_census['memcpy']} memcpy and {self.node_census['memset']} "
                "memset node(s); such nodes are not replay-safe on this runtime (DESIGN.md 4.4).  tools/find_memcpy_ops.py lists "
                "the ATen calls behind them; run the step eagerly (rag_amd.train.train_step) until they are kernels.")
        self.graph.instantiate()
        # train-mode BatchNorm buffers change at every replay through raw pointers: their version counters are bumped by hand
        # (the eval-mode caches of rag_amd.modules key on them)
        self._bn_buffers = [t for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training
                            and m.track_running_stats for t in (m.running_mean, m.running_var, m.num_batches_tracked) if t is not None]

    def _census(self) -> dict:
        return graph_census(self.graph)

    def _replay(self, pairs):
        """Copy the new inputs `(static buffer, tensor or None)` in, replay the graph, update eagerly.  -> the static loss."""
        for dst, src in pairs:
            if src is not None and dst is not None and src.data_ptr() != dst.data_ptr():
                dst.copy_(src)
        self.graph.replay()
        if self._bn_buffers:
            torch.autograd.graph.increment_version(self._bn_buffers)
        exchange_and_update(self.opt, self.bucket, clip=self.clip, dist=self.dist, active=self._active)
        return self.loss


class GraphedTrainStep(_GraphedStep):
    """The same step with forward + loss + backward replayed as ONE captured hipGraph (the ~2500 kernel launches of a
    step cost more host time than GPU time when issued one by one); the gradient exchange, clipping and the optimizer
    step stay eager (a handful of launches, and the collective stays outside the graph).  Inputs are copied into static
    buffers; shapes, the architecture and which parameters train must not change after capture.

    Nothing on the captured path may be a memset or memcpy NODE (hipMemsetAsync, a contiguous same-dtype copy_/clone):
    on this runtime (ROCm 7.2) a memcpy issued on the null stream between two replays (a `.item()`, a `.clone()`) left the next
    replay computing garbage whenever the instantiated graph held such a node — measured: 6-7 of 8 runs with one 160-byte memset
    and one 4-byte clone in the graph, 0 of 80 once both were kernels, with the same null-stream copies between replays
    (DESIGN.md 4.4 lists what was ruled out; tests/test_hip_train.py drives exactly that pattern).  The cause inside the runtime
    is not established, so the invariant is ENFORCED rather than assumed: the captured graph's nodes are counted at capture time
    (ragmi_graph_node_census) and a capture holding any memcpy / memset node is refused — an ATen op that starts lowering to
    copy_ or memset after a torch upgrade fails loudly here instead of corrupting a replay.  The graph replays on the caller's
    current stream; no private stream is involved.  `supervise=False`: the self-supervised step of src_self (gt may be None).
    A depth network: the silog step of forward_backward (right may be None).

    `sampled_ops=(fea_ops, mat_ops)`: the cell search's step on a supernet (forward_backward).  The search keeps its ops for an
    epoch, so it builds one object per epoch over the same bucket and optimizer (momentum carries over); the warm-up steps are real
    steps on the given batch, so with warmup=1 the constructor IS the epoch's first step, `first_loss` is its loss, and later calls
    replay.  Batch size 1 stays refused by the census as for the grown network (torch.cat of 5-D tensors is a copy there).

    `selected_ops=, t=, meter=`: the unit search's step (forward_backward), one object per epoch in the same way (a path holds for an
    epoch, rag.py:275-290).  The meter's update is part of the captured loss launch: every replay adds its batch to `meter.sums`, and
    `meter.last` stays the static vector the replays rewrite.

    `uncertainty=True, var_floor=`: the uncertainty-aware step of forward_backward; the statistics launch, the loss and both adjoints are
    kernels, so the census holds as for the plain step.

    `occlusion=True, lr_tol=, occluded_weight=` (with supervise=False): the occlusion-aware step of forward_backward.  The static
    inputs stay [B, ...]; the stacked 2B batch, the check and its weight are buffers inside the captured graph, and the stack, the
    check and the weighted loss are kernels, so the census holds."""

    def __init__(self, net, optimizer, bucket: GradBucket, left, right, gt, *, task_arch=None, clip: float = 5.0, dist=None,
                 features: bool = False, warmup: int = 2, precision: Optional[str] = None, supervise: bool = True,
                 sampled_ops: Optional[Sequence] = None, selected_ops: Optional[Sequence] = None, t: Optional[int] = None, meter=None,
                 uncertainty: bool = False, var_floor: float = 1.0 / 12.0, occlusion: bool = False,
                 lr_tol: Sequence[float] = (1.0, 0.0), occluded_weight: float = 0.0):
        _check_occlusion(occlusion, net, supervise, features, sampled_ops, selected_ops, uncertainty, meter, lr_tol, occluded_weight)
        _check_uncertainty(uncertainty, net, supervise, sampled_ops, selected_ops, meter)
        sel = _check_selected(net, selected_ops, t, gt, sampled_ops, task_arch, features, supervise)
        if _check_sampled(net, sampled_ops, gt, task_arch, features, supervise) is None and sel is None:
            _check_supervision(gt, features, supervise, _is_depth(net))
        _check_meter(meter, net, supervise)
        self._active = _active_of(net, sampled_ops, sel, t)
        self.net, self.opt, self.bucket, self.clip, self.dist = net, optimizer, bucket, clip, dist
        self.left = left.clone()
        self.right = right.clone() if right is not None else None
        self.gt = gt.clone() if gt is not None else None
        self.precision = precision or TRAIN_PRECISION
        kw = dict(task_arch=task_arch, features=features, precision=self.precision, supervise=supervise, sampled_ops=sampled_ops,
                  selected_ops=sel, t=t, meter=meter, uncertainty=uncertainty, var_floor=var_floor, occlusion=occlusion,
                  lr_tol=tuple(lr_tol), occluded_weight=occluded_weight)
        self._capture(lambda: forward_backward(net, bucket, self.left, self.right, self.gt, **kw), warmup)

    def __call__(self, left=None, right=None, gt=None):
        return self._replay(((self.left, left), (self.right, right), (self.gt, gt)))


def make_optimizer(params, lr: float = 1e-3, momentum: float = 0.9, weight_decay: float = 3e-3, bucket: Optional[GradBucket] = None):
    """rag.py:64-70: SGD over the parameters that require grad.  With `bucket` (on the GPU): the fused flat-buffer FlatSGD."""
    if bucket is not None and bucket.flat.is_cuda:
        return FlatSGD(bucket, lr=lr, momentum=momentum, weight_decay=weight_decay)
    return torch.optim.SGD([p for p in params if p.requires_grad], lr=lr, momentum=momentum, weight_decay=weight_decay)
