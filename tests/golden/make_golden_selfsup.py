#!/usr/bin/env python3
"""Generate the self-supervised loss fixtures by running the REFERENCE itself (build container only).

Imports chzhang18/RAG's continual-adaptation tree from /root/reference/src_self (read-only), runs its own
``re_and_sm_loss`` (models/loss.py:112-141) and its own Network training step on CPU on seeded inputs, and writes
inputs + outputs as small ``.npz`` fixtures next to this script.  On a machine without the reference this script
exits with a message and changes nothing.

Harness-side shims (the same class as make_golden.py's):
  * ``torch.Tensor.cuda`` -> identity: ``warp()`` (loss.py:6-37) moves the tensors it builds with ``.cuda()``;
  * ``torch.cuda.current_device`` -> CPU: DisparityRegression (models/rag_model.py:26);
  * ``torch.set_default_dtype(torch.float64)`` for the fp64 outputs: ``warp()`` builds its mask with the default dtype.

Fixtures:
  g12_selfsup_loss.npz        cases (B, H, W) of the loss alone: inputs, loss, the three terms and d loss / d disp, in fp32
                              and fp64.  Disparities are redrawn until every sample abscissa xs lies >= 1e-3 from an integer
                              (no pixel on a bilinear kink or in the 0.9999 mask band); asserted.
  g13_selfsup_train_step.npz  g6's training step (all-conv, 36x48, D = 24, train mode, stem3d0[0] in eval, the SAME weights:
                              seed 61, asserted equal to g6's ``sd::`` entries, which the tests load from g6) with re_and_sm_loss
                              instead of smooth-L1, on smooth images (noise upsampled x4, bilinear).  Keys as g6 (without the
                              ``sd::`` copy) plus ``grad::disp``.

Usage:  python tests/golden/make_golden_selfsup.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference/src_self"
OUT = os.path.dirname(os.path.abspath(__file__))
EPS_XS = 1e-3


def _import_reference():
    if not os.path.isdir(REF):
        print("reference not present; golden fixtures are used as committed")
        sys.exit(0)
    sys.path.insert(0, REF)
    torch.Tensor.cuda = lambda self, *a, **k: self                    # loss.py:21,33 shim
    torch.cuda.current_device = lambda: torch.device("cpu")          # rag_model.py:26 shim
    import models.loss as loss_mod  # noqa
    import models.rag_model as rm  # noqa
    from automl.genotypes_2d import Genotype  # noqa
    return loss_mod, rm, Genotype


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"{name}.npz  {size / 1024:.1f} KiB")
    assert size < 1024 * 1024, "fixture over the 1 MiB limit"


def xs_of(disp64, W):
    """The sample abscissa of every pixel (fp64): ((2 (x - d)/(W-1) - 1 + 1) W - 1)/2."""
    x = np.arange(W, dtype=np.float64)
    return (2.0 * (x - disp64) / (W - 1) - 1.0 + 1.0) * W / 2.0 - 0.5


def xs32_of(disp32, W):
    """The same abscissa in fp32, in the order of the reference's arithmetic (normalise, then grid_sample's unnormalise)."""
    x = np.arange(W, dtype=np.float32)
    g = np.float32(2.0) * (x - disp32) / np.float32(W - 1) - np.float32(1.0)
    return ((g + np.float32(1.0)) * np.float32(W) - np.float32(1.0)) / np.float32(2.0)


def near_kink(disp32, W):
    a = xs_of(disp32.astype(np.float64), W)
    b = xs32_of(disp32, W).astype(np.float64)
    return (np.abs(a - np.round(a)) < EPS_XS) | (np.abs(b - np.round(b)) < EPS_XS)


def draw_disp(gen, B, H, W, dmax, tile=None):
    """U(0, dmax) disparities (constant on tile x tile squares if `tile`), redrawn until no xs is within EPS_XS of an integer."""
    if tile is None:
        d = (torch.rand((B, H, W), generator=gen) * dmax).numpy()
        for _ in range(100):
            bad = near_kink(d, W)
            if not bad.any():
                break
            d[bad] = (torch.rand((int(bad.sum()),), generator=gen) * dmax).numpy()
    else:
        th, tw = -(-H // tile), -(-W // tile)
        t = (torch.rand((B, th, tw), generator=gen) * dmax).numpy()
        for _ in range(100):
            d = np.repeat(np.repeat(t, tile, axis=1), tile, axis=2)[:, :H, :W].copy()
            bad = near_kink(d, W)
            if not bad.any():
                break
            bt = np.zeros(t.shape, dtype=bool)
            for b, y, x in zip(*np.nonzero(bad)):
                bt[b, y // tile, x // tile] = True
            t[bt] = (torch.rand((int(bt.sum()),), generator=gen) * dmax).numpy()
    assert not near_kink(d, W).any(), "could not keep every xs away from the bilinear kinks"
    return d.astype(np.float32)


def run_loss(loss_mod, disp, left, right, dtype):
    """The reference's loss and its terms, and d loss / d disp, with `dtype` as the default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        d = torch.from_numpy(disp).to(dtype).requires_grad_(True)
        lt, rt = torch.from_numpy(left).to(dtype), torch.from_numpy(right).to(dtype)
        loss = loss_mod.re_and_sm_loss(d, lt, rt)
        loss.backward()
        with torch.no_grad():                    # the three terms, from the reference's own pieces
            de = d.detach().unsqueeze(1)
            est = loss_mod.warp(rt, de)
            ssim = loss_mod.mean_SSIM(lt, est)
            l1 = loss_mod.mean_l1(lt, est)
            total = loss.detach()
            smooth = (total - (0.85 * ssim + 0.15 * l1)) / 0.1
            assert float(est[:, :, 0].abs().max()) == 0.0 and float(est[:, :, -1].abs().max()) == 0.0   # rows 0, H-1 masked
        return (np.float64(total.item()), np.array([ssim.item(), l1.item(), smooth.item()], dtype=np.float64),
                d.grad.numpy().astype(np.float64 if dtype == torch.float64 else np.float32))
    finally:
        torch.set_default_dtype(old)


def smooth_images(gen, B, H, W):
    lo = torch.randn((B, 3, H // 4, W // 4), generator=gen)
    return F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).contiguous()


def main():
    loss_mod, rm, Genotype = _import_reference()
    torch.set_num_threads(8)

    # ---- G12: the loss alone
    arrays = {}
    cases = {"a": (2, 12, 20, 12.0, None), "odd": (1, 13, 22, 14.0, None), "b": (2, 36, 48, 30.0, None),
             "outview": (2, 12, 20, 30.0, None), "ties": (2, 24, 36, 20.0, 4)}
    for i, (tag, (B, H, W, dmax, tile)) in enumerate(cases.items()):
        gen = torch.Generator().manual_seed(120 + i)
        left = torch.randn((B, 3, H, W), generator=gen).numpy()
        right = torch.randn((B, 3, H, W), generator=gen).numpy()
        disp = draw_disp(gen, B, H, W, dmax, tile)
        l32, t32, g32 = run_loss(loss_mod, disp, left, right, torch.float32)
        l64, t64, g64 = run_loss(loss_mod, disp, left, right, torch.float64)
        if tag == "ties":
            assert (disp[:, :, :-1] == disp[:, :, 1:]).mean() > 0.5
        arrays.update({f"{tag}::left": left, f"{tag}::right": right, f"{tag}::disp": disp,
                       f"{tag}::loss32": l32, f"{tag}::terms32": t32, f"{tag}::grad32": g32,
                       f"{tag}::loss64": l64, f"{tag}::terms64": t64, f"{tag}::grad64": g64})
        print(f"  {tag}: loss {l64:.6f} terms {t64} |fp32-fp64| grad {np.abs(g32 - g64).max():.2e}")
    arrays["cases"] = np.array(list(cases))
    save("g12_selfsup_loss", **arrays)

    # ---- G13: g6's training step with the self-supervised loss
    rows = np.array([[0, 1], [1, 1], [2, 1], [3, 1], [5, 1], [6, 1]])
    torch.manual_seed(61)
    net = rm.Network(Genotype(normal=rows, normal_concat=None, reduce=rows, reduce_concat=None), "cpu")
    gen_bn = torch.Generator().manual_seed(61 + 1000)
    for m in net.modules():                       # make_golden.randomize_bn, same draws
        if isinstance(m, (torch.nn.BatchNorm3d, torch.nn.BatchNorm2d)):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen_bn) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen_bn) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen_bn) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen_bn) + 0.5)
    net.maxdisp = 24
    net.disp = rm.Disp(24)
    with np.load(os.path.join(OUT, "g6_train_step.npz")) as g6:
        sd6 = {k[4:]: g6[k] for k in g6.files if k.startswith("sd::")}
    sd = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    assert sd.keys() == sd6.keys() and all(np.array_equal(sd[k], sd6[k]) for k in sd), "weights differ from g6's"
    net.train()
    net.stem3d0[0].eval()
    gen = torch.Generator().manual_seed(130)
    left = smooth_images(gen, 2, 36, 48)
    right = smooth_images(gen, 2, 36, 48)
    gt = torch.rand((2, 36, 48), generator=gen) * 30
    feas = []

    def _keep(_m, _inp, o):
        o.retain_grad()
        feas.append(o)

    hk = net.last_3_2d[0].register_forward_hook(_keep)
    out = net.forward(left, right, 0, net.arch_init)
    hk.remove()
    out.retain_grad()
    loss = loss_mod.re_and_sm_loss(out, left, right)
    loss.backward()
    arrays = {"left": left.numpy(), "right": right.numpy(), "gt": gt.numpy(), "disp": out.detach().numpy(),
              "loss": np.float64(loss.item()), "rows": rows, "maxdisp": np.int64(24),
              "left_fea": feas[0].detach().numpy(), "right_fea": feas[1].detach().numpy(),
              "grad::left_fea": feas[0].grad.numpy(), "grad::right_fea": feas[1].grad.numpy(), "grad::disp": out.grad.numpy()}
    arrays.update({"after::" + k: v.detach().numpy().copy() for k, v in net.state_dict().items()
                   if ("running_" in k or "num_batches" in k) and ("3d" in k)})
    for k, p in net.named_parameters():
        if p.grad is not None and (k.startswith("stem3d") or k.startswith("last_") or k.startswith("cells_3d.0.")
                                   or k.startswith("cells_3d.7.")):
            arrays["grad::" + k] = p.grad.numpy()
    xs = xs_of(out.detach().double().numpy(), 48)
    print(f"  g13: loss {loss.item():.6f}; pixels with xs within 1e-4 of an integer: "
          f"{int((np.abs(xs - np.round(xs)) < 1e-4).sum())} of {xs.size}")
    save("g13_selfsup_train_step", **arrays)


if __name__ == "__main__":
    main()
