#!/usr/bin/env python3
"""Generate the depth-supernet fixture by running the REFERENCE itself (build container only), like make_golden_depth.py (whose
reference import and writer this script reuses).  On a machine without the reference it exits with a message and changes nothing.

Fixtures (three files, each under the 1 MiB limit of a committed file; tests read them through one merged dict):
  g23_depth_supernet.npz   the MdeNAS supernet of the depth tree (rag_depth/src/automl/mdenas_basicmodel.py BasicNetwork =
                           AutoFeature -> 2-D AutoMatching -> DispHead x 80 m), seeded, with its BatchNorm statistics calibrated so
                           that eval mode does not saturate the sigmoid: every BN momentum set to 1.0, one train-mode forward of a
                           [4,3,48,96] normal batch with draw A and one with all-conv ops, momentum back to 0.1.
                           ``sd::<key>``: the state dict after the calibration.
                           Eval forwards: ``img0`` (B=2 48x96), ``img1`` (B=1 60x84: level sizes 20x28, 10x14, 5x7, and the up-path
                           resizes 5x7 to 9x13) -> ``eval{i}_A`` / ``eval{i}_conv``.
  g23_depth_supernet_step_a.npz
                           One search training step (mdenas_search.py:186-203) at B=2 48x96 with draw A: silog_loss ->
                           clip_grad_norm_(5) -> SGD(lr=0.002, momentum=0.9, weight_decay=3e-4) (run_rag_depth.sh): ``left``, ``gt``
                           (uniform in (0, 80), ~10 % zeros), ``depth_train``, ``loss``, ``total_norm``, ``active_keys`` (JSON: the
                           names whose .grad is not None), ``unmoved`` (JSON: parameters bit-equal before and after), and for the
                           stems, ``last_*``, ``depth_head``, ``feature.cells.0`` and ``matching.cells.{0,4,7}``: ``grad::<param>``,
                           ``after::<param>``, ``after::<BN buffer>``.  The same step in fp64, stored as fp32: ``grad64::<param>``,
                           ``delta64::<param>`` (after - before), ``after64::<BN buffer>``.
  g23_depth_supernet_step_b.npz
                           A second step with draw B on the same optimizer: ``active_keys_B``, ``after2::<param>`` and its fp64 twin
                           ``delta2_64::<param>`` (after2 - after) for the same selection.
                           Back in g23_depth_supernet.npz: ``p_normal`` / ``p_reduce``: a random probability table, ``geno_normal`` /
                           ``geno_reduce``: the rows the reference's genotype() returns for it.

Usage:  python tests/golden/make_golden_depth_supernet.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_depth import _import_reference, save  # noqa: E402

DRAW_A = ([1, 0, 1, 1, 0, 1, 0, 1, 1], [0, 1, 1, 0, 1, 1, 1, 0, 1])
DRAW_B = ([0, 1, 1, 1, 0, 0, 1, 1, 0], [1, 1, 0, 1, 0, 1, 0, 1, 1])
ALL_CONV = ([1] * 9, [1] * 9)
STORED = (".stem", ".last_", "depth_head.", "feature.cells.0.", "matching.cells.0.", "matching.cells.4.", "matching.cells.7.")
BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def _blob(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def stored(name):
    return any(s in "." + name for s in STORED)


def main():
    _rm, _Genotype, ex, _appr = _import_reference()
    import automl.mdenas_basicmodel as mb
    torch.set_num_threads(1)
    # The all-conv pass overwrites the statistics draw A left in the units both draws share, so draw A's eval forward is the one
    # that can saturate: of seeds 1, 2, 3, 23, 91, 231, 2300 the reference keeps >= 0.9 of its pixels in (1, 79) m in all four eval
    # cases for seed 1 only (0.99 each); the assertion below holds the recipe to that.
    torch.manual_seed(1)
    sup = mb.BasicNetwork(device="cpu")

    # ---- BatchNorm calibration: running statistics = the batch statistics of a normal batch
    bns = [m for m in sup.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    gen = torch.Generator().manual_seed(2)
    for m in bns:
        m.momentum = 1.0
    sup.train()
    with torch.no_grad():
        for draw in (DRAW_A, ALL_CONV):
            x = torch.randn((4, 3, 48, 96), generator=gen)
            sup(x, x, *draw)
    for m in bns:
        m.momentum = 0.1
    sd = {k: v.detach().clone() for k, v in sup.state_dict().items()}
    arrays = {"sd::" + k: v.numpy() for k, v in sd.items()}

    # ---- eval forwards
    imgs = [torch.randn((2, 3, 48, 96), generator=gen), torch.randn((1, 3, 60, 84), generator=gen)]
    sup.eval()
    with torch.no_grad():
        for i, img in enumerate(imgs):
            arrays[f"img{i}"] = img.numpy()
            for tag, draw in (("A", DRAW_A), ("conv", ALL_CONV)):
                out = sup(img, img, *draw)
                inside = float(((out > 1) & (out < 79)).float().mean())
                print(f"g23 eval{i}_{tag} {tuple(out.shape)}: {float(out.min()):.2f} .. {float(out.max()):.2f} m, {inside:.2f} in (1, 79)")
                assert inside >= 0.9, "the sigmoid saturates: the calibration failed"
                arrays[f"eval{i}_{tag}"] = out.numpy()

    # ---- the search's training step: draw A, then draw B on the same optimizer; fp32 (stored) and fp64 (its yardstick)
    left = torch.randn((2, 3, 48, 96), generator=gen)
    gt = torch.rand((2, 48, 96), generator=gen) * 80
    gt[torch.rand((2, 48, 96), generator=gen) < 0.1] = 0
    step_a, step_b = dict(left=left.numpy(), gt=gt.numpy()), {}

    def two_steps(dtype):
        net = mb.BasicNetwork(device="cpu")
        net.load_state_dict(sd, strict=True)
        net = net.to(dtype).train()
        opt = torch.optim.SGD(net.parameters(), lr=0.002, momentum=0.9, weight_decay=3e-4)
        crit = ex.silog_loss()
        rec = []
        for draw in (DRAW_A, DRAW_B):
            before = {k: p.detach().clone() for k, p in net.named_parameters()}
            opt.zero_grad()
            est = net(left.to(dtype), None, *draw)
            loss = crit(est, gt.to(dtype), gt > 0)
            loss.backward()
            grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
            total = torch.nn.utils.clip_grad_norm_(net.parameters(), 5.0)
            opt.step()
            after = {k: p.detach().clone() for k, p in net.named_parameters()}
            bufs = {k: v.detach().clone() for k, v in net.state_dict().items() if k.rsplit(".", 1)[-1] in BN_BUFFERS}
            rec.append(dict(est=est.detach(), loss=loss.item(), grads=grads, total=float(total), before=before, after=after, bufs=bufs))
        return rec

    (a32, b32), (a64, b64) = two_steps(torch.float32), two_steps(torch.float64)
    active = sorted(a32["grads"])
    assert active == sorted(a64["grads"])
    moved = [k for k in a32["after"] if not torch.equal(a32["after"][k], a32["before"][k])]
    assert sorted(moved) == active, "exactly the parameters with a gradient move"
    step_a.update(depth_train=a32["est"].numpy(), loss=np.float64(a32["loss"]), total_norm=np.float64(a32["total"]),
                  loss64=np.float64(a64["loss"]), total_norm64=np.float64(a64["total"]), active_keys=_blob(active),
                  unmoved=_blob(sorted(k for k in a32["after"] if k not in moved)))
    step_b.update(active_keys_B=_blob(sorted(b32["grads"])), loss_B=np.float64(b32["loss"]))
    for k in active:
        if stored(k):
            step_a["grad::" + k] = a32["grads"][k].numpy()
            step_a["grad64::" + k] = a64["grads"][k].float().numpy()
            step_a["after::" + k] = a32["after"][k].numpy()
            step_a["delta64::" + k] = (a64["after"][k] - a64["before"][k]).float().numpy()
    for k in a32["after"]:
        if stored(k) and (k in a32["grads"] or k in b32["grads"]):       # active in A only: the second step must not move it
            step_b["after2::" + k] = b32["after"][k].numpy()
            step_b["delta2_64::" + k] = (b64["after"][k] - b64["before"][k]).float().numpy()
    changed = 0
    for k, v in a32["bufs"].items():
        if stored(k) and not torch.equal(v, sd[k]):
            step_a["after::" + k] = v.numpy()
            step_a["after64::" + k] = a64["bufs"][k].float().numpy() if v.is_floating_point() else a64["bufs"][k].numpy()
            changed += 1
    spread = max(float((a32["grads"][k].double() - a64["grads"][k]).abs().max() / a64["grads"][k].abs().max()) for k in active)
    print(f"g23 step A: loss {a32['loss']:.6f} (fp64 {a64['loss']:.6f}), total norm {a32['total']:.4f}, {len(active)} of "
          f"{len(a32['after'])} tensors active, {changed} stored BN buffers changed; fp32 vs fp64 gradients up to {spread:.2e} "
          f"(relative to max); step B: loss {b32['loss']:.6f}, {len(b32['grads'])} active")

    # ---- genotype() of a random probability table
    sup.p = {"normal": torch.rand((9, 2), generator=gen), "reduce": torch.rand((9, 2), generator=gen)}
    geno = sup.genotype()
    arrays.update(p_normal=sup.p["normal"].numpy(), p_reduce=sup.p["reduce"].numpy(),
                  geno_normal=np.asarray(geno.normal, dtype=np.int64), geno_reduce=np.asarray(geno.reduce, dtype=np.int64))
    arrays["n_params"] = np.int64(len(a32["after"]))
    save("g23_depth_supernet", **arrays)
    save("g23_depth_supernet_step_a", **step_a)
    save("g23_depth_supernet_step_b", **step_b)


if __name__ == "__main__":
    main()
