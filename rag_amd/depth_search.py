"""The depth tree's unit search on the device: one batch of `Appr.search_epoch` and of `Appr.search_eval`
(rag_depth/src/approaches/rag.py:371-438, 492-535), which `Appr.search_t` runs 100 epochs of for every task t > 0 on the expanded
`rag_amd.depth.Network`.

The step is forward (`Network.search_forward_train`: one unit per layer of `p`, the heads of task t) -> silog loss -> backward ->
clip_grad_norm_ -> SGD over `net.active_parameters(t, selected_ops)` alone, as torch.optim.SGD leaves a parameter whose .grad is None.
The loss is `silog_metrics_loss`: the pass that gives the loss also gives compute_errors' nine entries and adds all ten to the
epoch's `DepthEpochMeter`, where the reference copies depth_est and depth_gt to the host after every batch, gathers in numpy and
calls `.item()`.  Nothing leaves the device until `meter.mean()` at the end of the epoch.

The drivers stay with the caller as for the stereo tree: sampling from `p`, h_e / h_a, the probability update, `select`, and the
module modes (`net.search_mode()` for the training batches, `net.eval()` for the eval batches).  The generic
`rag_amd.train.forward_backward(.., selected_ops=)` and `search_eval_step` keep refusing a depth network and name these entry points.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .train import TRAIN_PRECISION, GradBucket, _GraphedStep, exchange_and_update


def _check(net, gt, t, selected_ops, meter, left=None) -> List[int]:
    """Argument checks of the three entry points, before any launch.  -> selected_ops as a list of ints."""
    from .depth import DepthEpochMeter, Network
    if not isinstance(net, Network):
        raise ValueError("depth unit search: net must be rag_amd.depth.Network (after expand)")
    if t is None:
        raise ValueError("depth unit search: the step needs the task index t (the heads it trains)")
    if gt is None:
        raise ValueError("depth unit search: the step needs the ground-truth depth gt (metres, 0 = invalid)")
    sel = net.check_selected(t, selected_ops)
    if meter is not None:
        dev = left.device if left is not None else gt.device
        if not isinstance(meter, DepthEpochMeter) or not meter.sums.is_cuda or meter.sums.device != dev:
            raise ValueError("depth unit search: meter must be a rag_amd.depth.DepthEpochMeter on the device of the batch")
    return sel


def _forward_backward(net, bucket: GradBucket, left, gt, t: int, sel: List[int], meter, precision: Optional[str]) -> torch.Tensor:
    from . import ops
    from .depth import silog_metrics_loss
    with ops.conv_precision(precision or TRAIN_PRECISION):
        loss = silog_metrics_loss(net.search_forward_train(left, t, sel), gt, meter)
        bucket.zero()
        loss.backward()
    return loss.detach()


def depth_search_step(net, optimizer, bucket: GradBucket, left, gt, t, selected_ops: Sequence[int], *, meter=None, clip: float = 5.0,
                      dist=None, precision: Optional[str] = None) -> torch.Tensor:
    """One batch of Appr.search_epoch (rag.py:401-427): net.search_forward_train(left, t, selected_ops) -> silog_metrics_loss(est, gt,
    meter) -> backward -> gradient all-reduce -> clip_grad_norm_(clip) -> SGD over net.active_parameters(t, selected_ops) only
    (FlatSGD.set_active; a torch optimizer sees .grad None on the others), so reused units, unsampled candidates and their momentum
    stay bit for bit.  The module modes are the caller's (`net.search_mode()`).  `meter` (rag_amd.depth.DepthEpochMeter): the loss
    launch adds this batch's loss and compute_errors entries to it, and `meter.last[0]` is the returned loss.  A net that is not
    rag_amd.depth.Network, a missing t or gt, a length other than the layers of p, a unit index outside its list, t outside the head
    lists and a meter that is not a DepthEpochMeter on the device raise ValueError before any launch.  Returns the detached loss."""
    sel = _check(net, gt, t, selected_ops, meter, left)
    loss = _forward_backward(net, bucket, left, gt, int(t), sel, meter, precision)
    exchange_and_update(optimizer, bucket, clip=clip, dist=dist, active=net.active_parameters(int(t), sel))
    return loss


def depth_search_eval_step(net, left, gt, t, selected_ops: Sequence[int], meter=None):
    """One batch of Appr.search_eval (rag.py:501-522): depth_metrics(net.search_forward(left, None, t, selected_ops), gt, meter=meter)
    under no_grad, with `net` in eval() (the caller's, as in rag.py:498; a net in training mode is refused).  -> DepthMetrics.  The
    argument checks of `depth_search_step`."""
    sel = _check(net, gt, t, selected_ops, meter, left)
    if net.training:
        raise ValueError("depth_search_eval_step: net must be in eval() (Appr.search_eval, rag.py:498)")
    from .depth import depth_metrics
    with torch.no_grad():
        return depth_metrics(net.search_forward(left, None, int(t), sel), gt, meter=meter)


class DepthGraphedSearchStep(_GraphedStep):
    """`depth_search_step` with forward + loss + backward replayed as ONE captured hipGraph (rag_amd.train.GraphedTrainStep's
    machinery and its rule: kernel nodes only).  A path holds for an epoch (rag.py:275-290), so the search builds one object per
    epoch over the same bucket and optimizer (momentum carries over): the warm-up steps are real steps on the given batch, so with
    warmup=1 the constructor IS the epoch's first step, `first_loss` is its loss, and later calls replay.  The meter's update is part
    of the captured loss launch: every replay adds its batch to `meter.sums`, and `meter.last` stays the static vector the replays
    rewrite."""

    def __init__(self, net, optimizer, bucket: GradBucket, left, gt, t, selected_ops: Sequence[int], *, meter=None, clip: float = 5.0,
                 warmup: int = 1, dist=None, precision: Optional[str] = None):
        sel = _check(net, gt, t, selected_ops, meter, left)
        self.net, self.opt, self.bucket, self.clip, self.dist = net, optimizer, bucket, clip, dist
        self._active = net.active_parameters(int(t), sel)
        self.left, self.gt = left.clone(), gt.clone()
        self.precision = precision or TRAIN_PRECISION
        self._capture(lambda: _forward_backward(net, bucket, self.left, self.gt, int(t), sel, meter, self.precision), warmup)

    def __call__(self, left=None, gt=None):
        return self._replay(((self.left, left), (self.gt, gt)))
