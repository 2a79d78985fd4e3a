#!/usr/bin/env python3
"""Generate the depth-training fixtures by running the REFERENCE itself (build container only), like make_golden_depth.py (whose
reference import, grown-model builder and writer this script reuses).  On a machine without the reference it exits with a message
and changes nothing.  Inputs of g14 (trained weights) and g16 (head cases) are read from their files, not copied.

Fixtures:
  g19_depth_head_bwd.npz   (a) the head backward on g16's four cases: ``case{k}_dout`` (random, stored as float16, exact in fp32) ->
                           torch autograd through upsample_6 -> last_3_3d -> DispHead(., 3) -> x 80 in fp32 (``case{k}_{dy,dw3,dw1,db1}``)
                           and in fp64 (``..._64``, stored rounded to fp32).
                           (b) silog_loss (utilstool/experiment.py:154-161) on three B=3 cases (some gt == 0; case 2 with large |d|):
                           ``silog{k}_{est,gt,loss,grad}`` (loss and d loss / d est from the reference module, fp32).
  g20_depth_train_step.npz one step of Appr.train_epoch (approaches/rag.py:182-246) for task 3 on g14's weights (stand-in genotypes,
                           archi = the last unit of every layer), B=2 48x96: ``model.train()``, the units outside the scripted
                           ``model_to_train`` (JSON) in eval() and frozen, silog -> backward -> clip_grad_norm_(5) ->
                           SGD(lr=1e-3, momentum=0.9, weight_decay=3e-3) (run_rag_depth.sh).  ``left``, ``gt``, ``archi`` (JSON),
                           ``depth_est``, ``loss``, ``grad::depth_est``, ``grad::<param>`` (before clipping), ``total_norm``,
                           ``after::<param>`` (trained parameters after the step), ``after::<buffer>`` (BN running statistics of the
                           trained units after the step).  The same step in fp64: ``grad64::<param>`` (from the stored
                           ``grad::depth_est``), ``delta64::<param>`` (after - before) and ``after64::<buffer>``, stored as fp32 (the
                           yardstick of the fp32 numbers, whose own spread from fp64 reaches a few percent on some tensors).

Usage:  python tests/golden/make_golden_depth_train.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_depth import HEADS, LAYERS, OUT, _import_reference, build_grown, save, units  # noqa: E402

# trained layers of the scripted task-3 step (their archi unit); every other unit is reused: eval() and frozen
TRAINED = ["stem_2d1", "cell_2d1", "cell_2d3", "last_3_2d", "stem_3d1", "cell_3d2", "cell_3d5", "cell_3d7"] + list(HEADS)


def head_bwd(rm, g16, k, dout, dtype):
    y = torch.as_tensor(g16[f"case{k}_y"]).to(dtype).requires_grad_(True)
    h, w = (int(v) for v in g16[f"case{k}_hw"])
    last3 = rm.ConvBR_2d(12, 1, 3, 1, 1, bn=False, relu=False).to(dtype)
    head = rm.DispHead(1).to(dtype)
    with torch.no_grad():
        last3.conv.weight.copy_(torch.as_tensor(g16[f"case{k}_w3"]))
        head.conv1.weight.copy_(torch.as_tensor(g16[f"case{k}_w1"]))
        head.conv1.bias.copy_(torch.as_tensor(g16[f"case{k}_b1"]))
    up6 = nn.Upsample(size=(h, w), mode="bilinear", align_corners=True)
    out = torch.squeeze(head(last3(up6(y)), 3), 1) * 80
    out.backward(dout.to(dtype))
    return [t.detach().float().numpy() for t in (y.grad, last3.conv.weight.grad, head.conv1.weight.grad, head.conv1.bias.grad)]


def main():
    rm, Genotype, ex, appr = _import_reference()
    torch.set_num_threads(1)
    g14 = dict(np.load(os.path.join(OUT, "g14_depth_ckpt_task3.npz")))
    g16 = dict(np.load(os.path.join(OUT, "g16_depth_head.npz")))

    # ---- G19 (a): the head's backward on g16's cases
    gen = torch.Generator().manual_seed(191)
    arrays = {}
    for k in range(4):
        h, w = (int(v) for v in g16[f"case{k}_hw"])
        dout = torch.randn((2, 3 * h, 3 * w), generator=gen).half()
        arrays[f"case{k}_dout"] = dout.numpy()
        r32 = head_bwd(rm, g16, k, dout.float(), torch.float32)
        r64 = head_bwd(rm, g16, k, dout.double(), torch.float64)
        for name, a32, a64 in zip(("dy", "dw3", "dw1", "db1"), r32, r64):
            arrays[f"case{k}_{name}"] = a32
            arrays[f"case{k}_{name}_64"] = a64
        print(f"g19 case {k}: |dy| {np.abs(r64[0]).max():.3e}  |dw3| {np.abs(r64[1]).max():.3e}  |dw1| {np.abs(r64[2]).max():.3e}  "
              f"db1 {float(r64[3][0]):.3e};  fp32 vs fp64 dy {np.abs(r32[0] - r64[0]).max():.2e}")

    # ---- G19 (b): silog_loss and its gradient
    crit = ex.silog_loss()
    for k in range(3):
        est = torch.rand((3, 32, 48), generator=gen) * 70 + 1
        spread = 0.2 if k < 2 else 2.5                       # case 2: |d| up to ~10
        gt = est * torch.exp(torch.randn((3, 32, 48), generator=gen) * spread)
        gt[torch.rand((3, 32, 48), generator=gen) < (0.3 if k != 1 else 0.9)] = 0
        e = est.clone().requires_grad_(True)
        loss = crit(e, gt, gt > 0)
        loss.backward()
        arrays.update({f"silog{k}_est": est.numpy(), f"silog{k}_gt": gt.numpy(), f"silog{k}_loss": np.float32(loss.item()),
                       f"silog{k}_grad": e.grad.numpy()})
        print(f"g19 silog {k}: loss {loss.item():.6f}  n {int((gt > 0).sum())}")
    save("g19_depth_head_bwd", **arrays)

    # ---- G20: one training step of task 3, in fp32 (the stored step) and in fp64 (the yardstick of the fp32 numbers)
    sd = {k: torch.as_tensor(v) for k, v in g14.items()}
    gen = torch.Generator().manual_seed(201)
    left = torch.rand((2, 3, 48, 96), generator=gen) * 2 - 1
    gt = torch.rand((2, 48, 96), generator=gen) * 60 + 2
    gt[torch.rand((2, 48, 96), generator=gen) < 0.3] = 0

    def step_net(dtype):
        net, _rows, counts = build_grown(rm, Genotype, sd)
        net = net.to(dtype)
        archi = {name: [counts[name] - 1] for name in LAYERS + list(HEADS)}
        model_to_train = {name: (archi[name] if name in TRAINED else []) for name in LAYERS + list(HEADS)}
        net.train()
        for name in LAYERS + list(HEADS):                # approaches/rag.py:185-228: reused units in eval()
            for i, unit in enumerate(units(net, name)):
                if i not in model_to_train[name]:
                    unit.eval()
        for p in net.parameters():                       # utils.freeze_model + modify_param(model_to_train) (rag.py:125-127)
            p.requires_grad = False
        net.modify_param(model_to_train, True)
        return net, archi, model_to_train

    def train_step(net, archi, dtype):
        opt = torch.optim.SGD(filter(lambda p: p.requires_grad, net.parameters()), lr=1e-3, weight_decay=3e-3, momentum=0.9)
        est = net(left.to(dtype), left.to(dtype), 3, archi)
        est.retain_grad()
        loss = ex.silog_loss()(est, gt.to(dtype), gt > 0)
        opt.zero_grad()
        loss.backward()
        grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.requires_grad and p.grad is not None}
        total = torch.nn.utils.clip_grad_norm_(net.parameters(), 5.0)
        opt.step()
        return est, loss, grads, total

    def bn_after(net, trained):
        prefixes = {k.rsplit(".conv.", 1)[0].rsplit(".bn.", 1)[0] for k in trained}
        return {k: v for k, v in net.state_dict().items()
                if (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))
                and k.rsplit(".bn.", 1)[0] in prefixes}

    net, archi, model_to_train = step_net(torch.float32)
    est, loss, grads, total = train_step(net, archi, torch.float32)
    named = dict(net.named_parameters())
    # trained tensors that take part in the forward (bn=False units construct a BatchNorm they never use: no gradient, no update)
    trained = list(grads)
    arrays = {"left": left.numpy(), "gt": gt.numpy(), "archi": np.frombuffer(json.dumps(archi).encode(), dtype=np.uint8),
              "model_to_train": np.frombuffer(json.dumps(model_to_train).encode(), dtype=np.uint8),
              "depth_est": est.detach().numpy(), "loss": np.float32(loss.item()), "grad::depth_est": est.grad.numpy()}
    for k in trained:
        arrays[f"grad::{k}"] = grads[k].numpy()
    arrays["total_norm"] = np.float32(float(total))
    for k in trained:
        arrays[f"after::{k}"] = named[k].detach().numpy().copy()
    for k, v in bn_after(net, trained).items():
        arrays[f"after::{k}"] = v.numpy().copy()

    # fp64: the parameter gradients of the stored d loss / d depth (the fixture's own fp32 run differs from them by up to a few
    # percent on some tensors: train-mode BatchNorm over B=2 on trained weights amplifies fp32 rounding), the step's update and the
    # running statistics
    net64, _a, _m = step_net(torch.float64)
    est64 = net64(left.double(), left.double(), 3, archi)
    est64.backward(est.grad.double())
    for k, p in net64.named_parameters():
        if k in grads:
            arrays[f"grad64::{k}"] = p.grad.float().numpy()
    before = {k: v.detach().double().clone() for k, v in sd.items()}
    net64, _a, _m = step_net(torch.float64)
    train_step(net64, archi, torch.float64)
    for k, p in net64.named_parameters():
        if k in grads:
            arrays[f"delta64::{k}"] = (p.detach() - before[k]).float().numpy()
    for k, v in bn_after(net64, trained).items():
        arrays[f"after64::{k}"] = v.float().numpy() if v.is_floating_point() else v.numpy()
    spread = max(float((grads[k].double() - torch.as_tensor(arrays[f"grad64::{k}"]).double()).abs().max()
                       / torch.as_tensor(arrays[f"grad64::{k}"]).double().abs().max()) for k in trained)
    print(f"g20: loss {loss.item():.6f}, total norm {float(total):.4f}, {len(trained)} trained tensors, "
          f"{sum(named[k].numel() for k in trained)} trained values; fp32 vs fp64 gradients up to {spread:.2e} (relative to max)")
    save("g20_depth_train_step", **arrays)


if __name__ == "__main__":
    main()
