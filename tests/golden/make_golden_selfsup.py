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
  g14_selfsup_edges.npz       the edge table G14_ROWS (B, C, H, W, d_lo, d_hi) of the loss alone, keys as g12: every channel count,
                              every (H % 3, W % 3), one block per row / column, 63 / 64 / 65 threads, a workgroup boundary inside
                              a later batch item, disparities of both signs, and three rows again with the disparity constant on
                              4 x 4 tiles.  Disparities are redrawn until ``ill_conditioned`` marks no pixel (asserted); ``probes``
                              holds the pixels tests/test_selfsup_sweep.py moves on PROBE_ROW.

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


def draw_disp_rounds(gen, B, H, W, dmax, tile=None, dmin=0.0, bad_of=None, rounds=100):
    """U(dmin, dmax) disparities (constant on tile x tile squares if `tile`), redrawn where `bad_of(d)` (default: near_kink) marks a
    pixel, for at most `rounds` rounds.  Returns (disparities, redraw rounds used)."""
    if bad_of is None:
        bad_of = lambda d: near_kink(d, W)  # noqa: E731

    def uniform(shape):
        return (torch.rand(shape, generator=gen) * (dmax - dmin) + dmin).numpy()

    used = 0
    if tile is None:
        d = uniform((B, H, W))
        for used in range(rounds + 1):
            bad = bad_of(d)
            if not bad.any() or used == rounds:
                break
            d[bad] = uniform((int(bad.sum()),))
    else:
        th, tw = -(-H // tile), -(-W // tile)
        t = uniform((B, th, tw))
        for used in range(rounds + 1):
            d = np.repeat(np.repeat(t, tile, axis=1), tile, axis=2)[:, :H, :W].copy()
            bad = bad_of(d)
            if not bad.any() or used == rounds:
                break
            bt = np.zeros(t.shape, dtype=bool)
            for b, y, x in zip(*np.nonzero(bad)):
                bt[b, y // tile, x // tile] = True
            t[bt] = uniform((int(bt.sum()),))
    assert not bad_of(d).any(), "could not draw disparities that meet the conditioning rules"
    return d.astype(np.float32), used


def draw_disp(gen, B, H, W, dmax, tile=None):
    """U(0, dmax) disparities (constant on tile x tile squares if `tile`), redrawn until no xs is within EPS_XS of an integer."""
    return draw_disp_rounds(gen, B, H, W, dmax, tile)[0]


# ---- G14: the edge table of tests/test_selfsup_sweep.py.  (B, C, H, W, d_lo, d_hi); seed 700 + position (tiled rows follow the table)
G14_ROWS = (
    (1, 3, 3, 3, -0.5, 1.5),                                                   # one thread, Hb = Wb = 1, no remainder
    (1, 1, 4, 5, -1.0, 3.0),                                                   # C = 1, Hb = Wb = 1, remainder 1 row / 2 columns
    (2, 2, 5, 4, -1.0, 3.0),                                                   # C = 2, Hb = Wb = 1, remainder 2 rows / 1 column, B = 2
    (1, 4, 6, 9, -2.0, 6.0),                                                   # C = 4, no remainder
    (1, 1, 3, 7, -2.0, 5.0),                                                   # Hb = 1, Wb = 2
    (1, 2, 8, 3, -1.0, 2.0),                                                   # Wb = 1, Hb = 2
) + tuple((1, 3, H, W, -3.0, 9.0) for H in (6, 7, 8) for W in (9, 10, 11)) + (  # all nine (H % 3, W % 3) with Hb, Wb >= 2
    (1, 3, 21, 27, -6.0, 20.0),                                                # 63 threads
    (1, 3, 24, 24, -6.0, 20.0),                                                # 64 threads
    (1, 1, 17, 41, -8.0, 30.0),                                                # 65 threads: a second workgroup with one live lane
    (3, 3, 16, 17, -4.0, 24.0),                                                # 75 threads: the workgroup boundary inside batch item 2
    (2, 4, 13, 22, -20.0, 44.0),                                               # C = 4, most disparities out of view on both sides
    (1, 3, 23, 29, -4.0, 12.0),                                                # 63 threads with remainder 2 / 2
)
G14_TILED = ((1, 3, 7, 10, -3.0, 9.0), (3, 3, 16, 17, -4.0, 24.0), (2, 4, 13, 22, -20.0, 44.0))   # disparity constant on 4 x 4 tiles
G14_TILE = 4
PROBE_ROW = (1, 3, 8, 11, -3.0, 9.0)
PROBES = ((4, 5), (6, 4), (3, 9))          # (y, x) on PROBE_ROW: inside a 3x3 block, in the remainder rows, in the remainder columns
PROBE_SHIFT = 0.37
EPS_COND = 1e-3
MIN_SHARE = 0.25


def g14_cases():
    """[(tag, row, tile or None)] in fixture order."""
    tag = "B{}C{}_{}x{}".format
    return [(tag(*r[:4]), r, None) for r in G14_ROWS] + [(tag(*r[:4]) + "_tiled", r, G14_TILE) for r in G14_TILED]


def selfsup_parts64(left, right, disp):
    """The loss's intermediate values in fp64, from arrays: (left_est [B,C,H,W], kept-by-the-mask [B,H,W], (1 - SSIM)/2 per 3x3 block
    and channel before the clamp [B,C,Hb,Wb]).  Plain torch, so that the rules below can be checked without the reference."""
    lt, rt = torch.from_numpy(np.asarray(left)).double(), torch.from_numpy(np.asarray(right)).double()
    d = torch.from_numpy(np.asarray(disp)).double()
    B, _, H, W = lt.shape
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W) - d
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1).expand(B, H, W)
    grid = torch.stack((2 * xs / (W - 1) - 1, 2 * ys / (H - 1) - 1), dim=-1)
    kept = F.grid_sample(torch.ones_like(rt[:, :1]), grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0] >= 0.9999
    est = F.grid_sample(rt, grid, mode="bilinear", padding_mode="zeros", align_corners=False) * kept[:, None]
    mu_x, mu_y = F.avg_pool2d(lt, 3), F.avg_pool2d(est, 3)
    var_x, var_y = F.avg_pool2d(lt * lt, 3) - mu_x * mu_x, F.avg_pool2d(est * est, 3) - mu_y * mu_y
    cov = F.avg_pool2d(lt * est, 3) - mu_x * mu_y
    ssim = (2 * mu_x * mu_y + 1e-4) * (2 * cov + 9e-4) / ((mu_x * mu_x + mu_y * mu_y + 1e-4) * (var_x + var_y + 9e-4))
    return est, kept, (1 - ssim) / 2


def ill_conditioned(left, right, disp):
    """Pixels [B,H,W] on or next to one of the loss's kinks, where an fp32 and an fp64 evaluation may legitimately take different
    sides: (1) sample abscissa within EPS_XS of an integer (near_kink); (2) kept by the mask and |left - left_est| < EPS_COND in some
    channel; (3) in a 3x3 block whose (1 - SSIM)/2 lies within EPS_COND of 0 or 1 in some channel (the clamp); (4) a neighbour's
    disparity differs by less than EPS_COND without being equal (the smoothness term's |.|).  And (5), so that no row degenerates
    into smoothness only: at H >= 6, W >= 9 the mask keeps at least MIN_SHARE of the pixels, else the out-of-view ones are marked."""
    disp = np.asarray(disp, dtype=np.float32)
    lt = torch.from_numpy(np.asarray(left)).double()
    H, W = disp.shape[1:]
    bad = near_kink(disp, W)
    est, kept, half = selfsup_parts64(left, right, disp)
    bad |= (kept & ((lt - est).abs() < EPS_COND).any(1)).numpy()
    blocks = ((half.abs() < EPS_COND) | ((half - 1).abs() < EPS_COND)).any(1).numpy()
    bad[:, :3 * (H // 3), :3 * (W // 3)] |= np.repeat(np.repeat(blocks, 3, axis=1), 3, axis=2)
    d64 = disp.astype(np.float64)
    for a, b in ((np.s_[:, :, :-1], np.s_[:, :, 1:]), (np.s_[:, :-1, :], np.s_[:, 1:, :])):
        gap = np.abs(d64[a] - d64[b])
        close = (gap < EPS_COND) & (gap != 0)
        bad[a] |= close
        bad[b] |= close
    if H >= 6 and W >= 9 and float(kept.double().mean()) < MIN_SHARE:      # (5): out-of-view pixels off the always-masked rows 0, H-1
        bad[:, 1:H - 1] |= ~kept.numpy()[:, 1:H - 1]
    return bad


def unmasked_share(left, right, disp):
    return float(selfsup_parts64(left, right, disp)[1].double().mean())


def probe_disp(disp, probe):
    """PROBE_ROW's disparities with the one at `probe` moved by PROBE_SHIFT."""
    moved = np.array(disp, dtype=np.float32, copy=True)
    moved[0, probe[0], probe[1]] += np.float32(PROBE_SHIFT)
    return moved


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

    # ---- G14: the loss alone on the edge table
    arrays, redrawn = {}, []
    for i, (tag, (B, C, H, W, lo, hi), tile) in enumerate(g14_cases()):
        gen = torch.Generator().manual_seed(700 + i)
        left = torch.randn((B, C, H, W), generator=gen).numpy()
        right = torch.randn((B, C, H, W), generator=gen).numpy()
        disp, rounds = draw_disp_rounds(gen, B, H, W, hi, tile, dmin=lo, bad_of=lambda d: ill_conditioned(left, right, d), rounds=200)
        if rounds:
            redrawn.append((tag, rounds))
        assert not ill_conditioned(left, right, disp).any() and float(disp.min()) >= lo and float(disp.max()) <= hi
        share = unmasked_share(left, right, disp)
        assert share > 0 and (share >= MIN_SHARE or H < 6 or W < 9), (tag, share)
        if tile:
            assert (disp[:, :, :-1] == disp[:, :, 1:]).mean() > 0.5
        if (B, C, H, W, lo, hi) == PROBE_ROW:
            for probe in PROBES:               # the locality test's shifted inputs stay clear of every kink too
                assert not ill_conditioned(left, right, probe_disp(disp, probe)).any(), probe
        torch.set_default_dtype(torch.float64)                 # the rules were checked on the reference's own left_est
        try:
            with torch.no_grad():
                est_ref = loss_mod.warp(torch.from_numpy(right).double(), torch.from_numpy(disp).double().unsqueeze(1))
        finally:
            torch.set_default_dtype(torch.float32)
        assert float((est_ref - selfsup_parts64(left, right, disp)[0]).abs().max()) <= 1e-12
        l32, t32, g32 = run_loss(loss_mod, disp, left, right, torch.float32)
        l64, t64, g64 = run_loss(loss_mod, disp, left, right, torch.float64)
        yard = np.abs(g32 - g64).max() / np.abs(g64).max()
        assert yard <= 2.5e-4, (tag, yard)     # the reference's own fp32 run is a usable yardstick: else redraw the row
        arrays.update({f"{tag}::left": left, f"{tag}::right": right, f"{tag}::disp": disp,
                       f"{tag}::loss32": l32, f"{tag}::terms32": t32, f"{tag}::grad32": g32,
                       f"{tag}::loss64": l64, f"{tag}::terms64": t64, f"{tag}::grad64": g64})
        print(f"  {tag}: loss {l64:.6f} unmasked {share:.2f} redraw rounds {rounds} |fp32-fp64| grad / max|g| {yard:.2e}")
    arrays["cases"] = np.array([tag for tag, _row, _tile in g14_cases()])
    arrays["probes"] = np.array(PROBES, dtype=np.int64)
    print(f"  g14 rows redrawn: {redrawn}")
    save("g14_selfsup_edges", **arrays)

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
