#!/usr/bin/env python3
"""Generate golden vectors by running the REFERENCE itself (build container only).

Imports chzhang18/RAG from /root/reference/src (read-only), runs its own
modules on seeded inputs on CPU, and writes inputs + state_dicts + outputs as
small ``.npz`` fixtures next to this script.  The reference never travels to
the GPU box; only these data files do.  On a machine without /root/reference
this script exits with a message and changes nothing.

Harness-side shims: ``torch.cuda.current_device`` -> CPU, required by
DisparityRegression (src/models/rag_model.py:26) to run without a GPU; and, for
G11 only, an empty placeholder module named ``torchvision`` so that
``utilstool/experiment.py:7``'s import statement succeeds (the metric functions
under test never touch it).

Usage:  python tests/golden/make_golden.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))


def _import_reference():
    if not os.path.isdir(REF):
        print("reference not present; golden fixtures are used as committed")
        sys.exit(0)
    sys.path.insert(0, REF)
    torch.cuda.current_device = lambda: torch.device("cpu")  # rag_model.py:26 shim
    import models.rag_model as rm  # noqa
    from automl.genotypes_2d import Genotype  # noqa
    return rm, Genotype


def randomize_bn(module, gen):
    """Give every BatchNorm non-trivial affine + running stats so folding is exercised."""
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm3d, torch.nn.BatchNorm2d)):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) + 0.5)


def sd_np(module, prefix="sd::"):
    # copies: .numpy() aliases the live buffers, which train-mode BatchNorm updates in place
    return {prefix + k: v.detach().cpu().numpy().copy() for k, v in module.state_dict().items()}


ONLY = [a for a in sys.argv[1:] if not a.startswith("-")]   # e.g. `make_golden.py g8` regenerates one fixture family


def forward_f64(net, feas, fn):
    """fn(copy of `net` in float64) under no_grad, with the Feature Net's outputs (last_3_2d) replaced by `feas` (stored float32
    features, cast to double, in call order): the Matching-Net half alone, as the oracle tests feed it."""
    import copy
    net64 = copy.deepcopy(net).double()
    queue = [torch.from_numpy(f).double() for f in feas]
    hk = [m.register_forward_hook(lambda _m, _i, _o: queue.pop(0)) for m in net64.last_3_2d]
    with torch.no_grad():
        out = fn(net64).numpy()
    for h_ in hk:
        h_.remove()
    assert not queue
    return out


def save(name, **arrays):
    if ONLY and not any(name.startswith(o) for o in ONLY):
        return
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


ALL_CONV = np.array([[0, 1], [1, 1], [2, 1], [3, 1], [5, 1], [6, 1]])
ALL_SKIP = np.array([[0, 0], [1, 0], [2, 0], [3, 0], [5, 0], [6, 0]])
MIXED_UNSORTED = np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]])   # SURVEY §8 A6 probe
MIXED_DEEP = np.array([[1, 1], [0, 0], [4, 1], [2, 0], [7, 1], [8, 1]])       # uses s2 and s3 as inputs


def main():
    rm, Genotype = _import_reference()
    torch.set_num_threads(8)

    def genotype(rows):
        return Genotype(normal=rows, normal_concat=None, reduce=rows, reduce_concat=None)

    def network(rows, maxdisp, seed):
        torch.manual_seed(seed)
        net = rm.Network(genotype(rows), "cpu")
        randomize_bn(net, torch.Generator().manual_seed(seed + 1000))
        net.maxdisp = maxdisp             # reference hard-codes 192 (rag_model.py:274)
        net.disp = rm.Disp(maxdisp)
        net.eval()
        return net

    # ---- G1: cost volume, produced by the reference's inline loop (rag_model.py:375-383).
    # Features are fed straight in by bypassing feature(); the loop's output is captured
    # at the entrance of stem3d0.
    for tag, (B, C, h, w, d) in {"a": (2, 12, 6, 20, 8), "b": (1, 12, 4, 5, 8)}.items():
        net = network(ALL_SKIP, 3 * d, seed=1)
        g = torch.Generator().manual_seed(11)
        L = torch.randn((B, C, h, w), generator=g)
        R = torch.randn((B, C, h, w), generator=g)
        captured = {}
        net.feature = lambda x, ta, p: x
        hook = net.stem3d0[0].register_forward_pre_hook(lambda m, inp: captured.__setitem__("cost", inp[0].clone()))
        try:
            with torch.no_grad():
                net.forward(L, R, 0, net.arch_init)
        except Exception:
            pass  # shapes this small may fail later in matching(); only the captured cost matters
        hook.remove()
        save(f"g1_costvol_{tag}", left_fea=L.numpy(), right_fea=R.numpy(), maxdisp=np.int64(3 * d),
             cost=captured["cost"].numpy())

    # ---- G2: Disp / DisparityRegression (rag_model.py:18-44)
    g = torch.Generator().manual_seed(21)
    x = torch.randn((2, 1, 8, 4, 8), generator=g) * 3
    with torch.no_grad():
        out = rm.Disp(24)(x)
        prob = torch.softmax(torch.randn((2, 24, 5, 7), generator=g), dim=1).contiguous()
        reg = rm.DisparityRegression(24)(prob)
        x2 = torch.randn((1, 1, 5, 3, 4), generator=g) * 2          # maxdisp not 3*d: generic D scale
        out2 = rm.Disp(13)(x2)
    save("g2_disp", x=x.numpy(), maxdisp=np.int64(24), out=out.numpy(), prob=prob.numpy(), reg=reg.numpy(),
         x2=x2.numpy(), maxdisp2=np.int64(13), out2=out2.numpy())

    # ---- G3: ConvBR_3d eval + train mode (operations_3d.py:31-47)
    arrays = {}
    cases = {"k3": (4, 4, 3, 1, True, True), "k3_wide": (24, 12, 3, 1, True, True),
             "k1": (12, 4, 1, 0, True, True), "k3_nobn": (12, 1, 3, 1, False, False)}
    for name, (cin, cout, k, pad, bn, relu) in cases.items():
        torch.manual_seed(31)
        m = rm.ConvBR_3d(cin, cout, k, 1, pad, bn=bn, relu=relu)
        randomize_bn(m, torch.Generator().manual_seed(32))
        g = torch.Generator().manual_seed(33)
        x = torch.randn((2, cin, 5, 6, 9), generator=g)
        m.eval()
        with torch.no_grad():
            y_eval = m(x.clone())
        m.train()
        with torch.no_grad():
            y_train = m(x.clone())
        arrays.update({f"{name}::x": x.numpy(), f"{name}::y_eval": y_eval.numpy(), f"{name}::y_train": y_train.numpy(),
                       f"{name}::cfg": np.array([cin, cout, k, pad, int(bn), int(relu)])})
        # state_dict BEFORE the train-mode call mutated running stats is what eval used; re-create it
        torch.manual_seed(31)
        m0 = rm.ConvBR_3d(cin, cout, k, 1, pad, bn=bn, relu=relu)
        randomize_bn(m0, torch.Generator().manual_seed(32))
        arrays.update({f"{name}::" + k_: v for k_, v in sd_np(m0).items()})
    save("g3_convbr", **arrays)

    # ---- G4: Cell_3d for each downup, even and odd dims, sorted + unsorted genotypes
    arrays = {}
    cell_cases = {
        "same_conv": (4, 4, 4, 0, ALL_CONV, (6, 8, 10), (6, 8, 10)),
        "same_unsorted": (4, 4, 4, 0, MIXED_UNSORTED, (5, 6, 7), (5, 6, 7)),
        "same_deep": (4, 4, 4, 0, MIXED_DEEP, (4, 6, 9), (4, 6, 9)),
        "down_even": (4, 4, 8, -1, ALL_CONV, (8, 12, 16), (8, 12, 16)),
        "down_odd": (4, 8, 16, -1, MIXED_UNSORTED, (8, 12, 20), (7, 9, 13)),
        "up": (8, 16, 8, 1, MIXED_DEEP, (6, 8, 10), (3, 4, 5)),
        "skip": (8, 16, 16, 0, ALL_SKIP, (4, 6, 8), (4, 6, 8)),
    }
    for name, (pp, p, fm, du, rows, size0, size1) in cell_cases.items():
        torch.manual_seed(41)
        cell = rm.Cell_3d(3, 3, pp, p, genotype(rows), fm, du)
        randomize_bn(cell, torch.Generator().manual_seed(42))
        cell.eval()
        g = torch.Generator().manual_seed(43)
        s0 = torch.randn((2, 3 * pp) + size0, generator=g)
        s1 = torch.randn((2, 3 * p) + size1, generator=g)
        with torch.no_grad():
            prev, cat = cell(s0, s1)
        assert prev is s1
        arrays.update({f"{name}::s0": s0.numpy(), f"{name}::s1": s1.numpy(), f"{name}::out": cat.numpy(),
                       f"{name}::rows": rows, f"{name}::cfg": np.array([pp, p, fm, du])})
        arrays.update({f"{name}::" + k_: v for k_, v in sd_np(cell).items()})
    save("g4_cell3d", **arrays)

    # ---- G5: full matching() and forward() (rag_model.py:325-387); B=2
    for name, (rows, H, W, D, seed) in {"conv_48x96_d48": (ALL_CONV, 48, 96, 48, 51),
                                        "unsorted_36x60_d24": (MIXED_UNSORTED, 36, 60, 24, 52),
                                        "skip_48x72_d24": (ALL_SKIP, 48, 72, 24, 53)}.items():
        net = network(rows, D, seed)
        g = torch.Generator().manual_seed(seed + 1)
        left = torch.randn((2, 3, H, W), generator=g)
        right = torch.randn((2, 3, H, W), generator=g)
        cap = {}
        h1 = net.stem3d0[0].register_forward_pre_hook(lambda m, inp: cap.__setitem__("cost", inp[0].clone()))
        h2 = net.disp.register_forward_pre_hook(lambda m, inp: cap.__setitem__("mat", inp[0].clone()))
        with torch.no_grad():
            lf = net.feature(left, net.arch_init, None)
            rf = net.feature(right, net.arch_init, None)
            disp = net.forward(left, right, 0, net.arch_init)
        h1.remove(); h2.remove()
        arrays = {"left": left.numpy(), "right": right.numpy(), "left_fea": lf.numpy(), "right_fea": rf.numpy(),
                  "mat": cap["mat"].numpy(), "disp": disp.numpy(), "rows": rows, "maxdisp": np.int64(D)}
        arrays.update(sd_np(net))
        save("g5_forward_" + name, **arrays)
        # mat and disp in float64 from the same stored features and weights (see G10's float64 outputs below for why)
        cap64 = {}

        def run64(n_):
            n_.disp.register_forward_pre_hook(lambda m, inp: cap64.__setitem__("mat", inp[0].clone()))
            return n_.forward(left.double(), right.double(), 0, n_.arch_init)

        disp64 = forward_f64(net, (arrays["left_fea"], arrays["right_fea"]), run64)
        save("g5_forward_" + name + "_f64", mat=cap64["mat"].numpy(), disp=disp64)

    # ---- G6: one fwd+bwd training step as in approaches/rag.py:155-219 (smooth-L1 on 0<gt<192 mask)
    net = network(ALL_CONV, 24, 61)
    net.train()
    net.stem3d0[0].eval()         # a "reused" unit keeps BN in eval (rag.py:159-200)
    g = torch.Generator().manual_seed(62)
    left = torch.randn((2, 3, 36, 48), generator=g)
    right = torch.randn((2, 3, 36, 48), generator=g)
    gt = torch.rand((2, 36, 48), generator=g) * 30
    sd_before = sd_np(net)
    feas = []                      # Feature-Net outputs (left, then right) as the Matching Net sees them in train mode
    def _keep(_m, _inp, o):
        o.retain_grad()
        feas.append(o)

    hk = net.last_3_2d[0].register_forward_hook(_keep)
    out = net.forward(left, right, 0, net.arch_init)
    hk.remove()
    mask = (gt < 24) & (gt > 0)
    loss = torch.nn.functional.smooth_l1_loss(out[mask], gt[mask], reduction="mean")
    loss.backward()
    arrays = {"left": left.numpy(), "right": right.numpy(), "gt": gt.numpy(), "disp": out.detach().numpy(),
              "loss": np.float64(loss.item()), "rows": ALL_CONV, "maxdisp": np.int64(24),
              "left_fea": feas[0].detach().numpy(), "right_fea": feas[1].detach().numpy(),
              "grad::left_fea": feas[0].grad.numpy(), "grad::right_fea": feas[1].grad.numpy()}
    arrays.update(sd_before)
    arrays.update({"after::" + k_[4:]: v for k_, v in sd_np(net).items()     # running statistics after the step's forward
                   if ("running_" in k_ or "num_batches" in k_) and ("3d" in k_)})
    for k_, p_ in net.named_parameters():
        if p_.grad is not None and (k_.startswith("stem3d") or k_.startswith("last_") or k_.startswith("cells_3d.0.")
                                    or k_.startswith("cells_3d.7.")):
            arrays["grad::" + k_] = p_.grad.numpy()
    save("g6_train_step", **arrays)

    # ---- G7: plumbing config (BASELINE configs[0]): 256x512 padded to 264x516, D=48, B=1.
    # Full output is too big to commit: keep a 64x64 centre crop + checksums.
    net = network(ALL_CONV, 48, 71)
    g = torch.Generator().manual_seed(72)
    left = torch.randn((1, 3, 264, 516), generator=g)
    right = torch.randn((1, 3, 264, 516), generator=g)
    with torch.no_grad():
        lf = net.feature(left, net.arch_init, None)
        rf = net.feature(right, net.arch_init, None)
        disp = net.forward(left, right, 0, net.arch_init)
    crop = disp[:, 100:164, 226:290].contiguous()
    arrays = {"left_fea": lf.numpy().astype(np.float32), "right_fea": rf.numpy().astype(np.float32),
              "disp_crop": crop.numpy(), "crop_box": np.array([100, 164, 226, 290]),
              "disp_mean": np.float64(disp.double().mean().item()),
              "disp_abs_sum": np.float64(disp.double().abs().sum().item()),
              "disp_row_means": disp.double().mean(dim=2).numpy()[0],
              "rows": ALL_CONV, "maxdisp": np.int64(48)}
    arrays.update({k_: v for k_, v in sd_np(net).items()
                   if any(s in k_ for s in ("stem3d", "cells_3d", "last_3_3d", "last_6_3d", "last_12_3d"))})
    save("g7_plumbing_264x516_d48", **arrays)


    # ---- G8: growth-API bookkeeping of Network.expand / get_new_model / select (rag_model.py:391-551, 709-845)
    import json
    torch.manual_seed(81)
    net = rm.Network(genotype(ALL_CONV), "cpu")
    keys0 = sorted(net.state_dict().keys())
    net.expand(1, genotype(MIXED_UNSORTED), "cpu")
    keys1 = sorted(net.state_dict().keys())
    p_expand = [p_.numpy().tolist() for p_ in net.p]
    new_models = {k_: [int(v) for v in vs] for k_, vs in net.new_models.items()}
    winners = (1, 5, 9, 12)                 # p-indices where the candidate unit wins
    for k_, p_ in enumerate(net.p):
        if k_ in winners:
            p_[-1] = 0.9
    best = net.select(1)
    to_int = lambda d: {k_: [int(v) for v in vs] for k_, vs in d.items()}  # noqa: E731
    blob = {"keys_initial": keys0, "keys_expanded": keys1, "keys_selected": sorted(net.state_dict().keys()),
            "p_after_expand": p_expand, "new_models": new_models, "winners": list(winners),
            "best_archi": to_int(best), "model_to_train": to_int(net.model_to_train),
            "length": {k_: int(v) for k_, v in net.length.items()}, "arch_init": to_int(net.arch_init)}
    # second growth round on top, everything reused
    net.expand(2, genotype(ALL_SKIP), "cpu")
    best2 = net.select(2)
    blob["best_archi_round2"] = to_int(best2)
    blob["length_round2"] = {k_: int(v) for k_, v in net.length.items()}
    blob["keys_round2"] = sorted(net.state_dict().keys())
    save("g8_growth_api", blob=np.frombuffer(json.dumps(blob).encode(), dtype=np.uint8))

    # ---- G9: the MdeNAS supernet (automl/mdenas_basicmodel.py BasicNetwork = AutoFeature + AutoMatching with one sampled
    # op per edge, automl/build_model_{2d,3d}.py): eval forward and one training step (mdenas_search.py:164-173)
    import automl.mdenas_basicmodel as mb
    torch.manual_seed(91)
    sup = mb.BasicNetwork(device="cpu")
    randomize_bn(sup, torch.Generator().manual_seed(1091))
    sup.maxdisp = 48
    sup.disp = mb.Disp(48)
    g = torch.Generator().manual_seed(92)
    left = torch.randn((1, 3, 48, 96), generator=g)
    right = torch.randn((1, 3, 48, 96), generator=g)
    gt = torch.rand((1, 48, 96), generator=g) * 60
    fea_ops = np.array([1, 0, 1, 1, 0, 1, 0, 1, 1])
    mat_ops = np.array([0, 1, 1, 0, 1, 1, 1, 0, 1])
    sd0 = sd_np(sup)
    sup.eval()
    with torch.no_grad():
        disp_eval = sup(left, right, fea_ops, mat_ops)
        disp_eval_conv = sup(left, right, np.ones(9, dtype=np.int64), np.ones(9, dtype=np.int64))
    sup.train()
    out = sup(left, right, fea_ops, mat_ops)
    mask = (gt < 48) & (gt > 0)
    loss = torch.nn.functional.smooth_l1_loss(out[mask], gt[mask], reduction="mean")
    loss.backward()
    arrays = {"left": left.numpy(), "right": right.numpy(), "gt": gt.numpy(), "fea_ops": fea_ops, "mat_ops": mat_ops,
              "disp_eval": disp_eval.numpy(), "disp_eval_all_conv": disp_eval_conv.numpy(), "disp_train": out.detach().numpy(),
              "loss": np.float64(loss.item()), "maxdisp": np.int64(48)}
    arrays.update(sd0)
    n = 0
    for k_, p_ in sup.named_parameters():
        if p_.grad is not None and (".stem" in k_ or ".last_" in k_ or ".cells.0." in k_ or "matching.cells.4." in k_ or "matching.cells.7." in k_):
            arrays["grad::" + k_] = p_.grad.numpy()
            n += 1
    arrays["n_params_with_grad"] = np.int64(sum(1 for p_ in sup.parameters() if p_.grad is not None))
    arrays["n_params"] = np.int64(sum(1 for _ in sup.parameters()))
    save("g9_supernet", **arrays)

    # ---- G10: a GROWN model (rag_model.py:391-522 expand, :709-845 select): numerical outputs with unit index != 0 and t != 0.
    # search_forward on the expanded supermodel with mixed unit choices (rag_model.py:663-706), then forced winners ->
    # select(1) -> eval forward of task 0 (arch_init) and task 1 (best_archi) on the selected model (what run.py:194-196 saves).
    torch.manual_seed(101)
    net = rm.Network(genotype(ALL_CONV), "cpu")
    net.maxdisp = 48
    net.disp = rm.Disp(48)
    arch0 = {k_: [int(v) for v in vs] for k_, vs in net.arch_init.items()}
    net.expand(1, genotype(MIXED_UNSORTED), "cpu")
    randomize_bn(net, torch.Generator().manual_seed(1101))          # after expand: the candidate units get statistics too
    net.eval()
    g = torch.Generator().manual_seed(102)
    left = torch.randn((1, 3, 48, 96), generator=g)
    right = torch.randn((1, 3, 48, 96), generator=g)
    feas = []
    hk = [m.register_forward_hook(lambda _m, _i, o: feas.append(o.detach().clone())) for m in net.last_3_2d]
    sel_a = [0, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1]       # unit per layer: p-order (8 = stem3d0, 9 = stem3d1, 10.. = cells)
    sel_b = [1] * 18                                                     # every candidate unit
    arrays = {"left": left.numpy(), "right": right.numpy(), "maxdisp": np.int64(48), "rows_unit0": ALL_CONV, "rows_unit1": MIXED_UNSORTED,
              "sel_a": np.array(sel_a), "sel_b": np.array(sel_b)}
    arrays.update(sd_np(net, "search::"))
    with torch.no_grad():
        for tag, sel, t in (("a", sel_a, 1), ("b", sel_b, 1), ("c", sel_a, 0)):
            del feas[:]
            arrays[f"search_disp_{tag}"] = net.search_forward(left, right, t, sel).numpy()
            arrays[f"search_left_fea_{tag}"], arrays[f"search_right_fea_{tag}"] = feas[0].numpy(), feas[1].numpy()
    # the same outputs in float64 from the same stored features and weights (g10_grown_model_f64; g5 likewise): at random weights the
    # float32 forward is ill-conditioned (|cost| ~1e4, softmin nearly an argmin), so its last bits — the summation order of the
    # host's BLAS, which differs between CPU models — move single pixels by up to ~0.05 px; in float64 they do not
    f64 = {}
    for tag, sel, t in (("a", sel_a, 1), ("b", sel_b, 1), ("c", sel_a, 0)):
        f64[f"search_disp_{tag}"] = forward_f64(net, (arrays[f"search_left_fea_{tag}"], arrays[f"search_right_fea_{tag}"]),
                                                lambda n_, sel=sel, t=t: n_.search_forward(left.double(), right.double(), t, sel))
    winners = (1, 3, 5, 7, 9, 11, 12, 15, 17)           # p-indices where the candidate wins (2-D and 3-D layers, both stems kinds)
    for k_, p_ in enumerate(net.p):
        if k_ in winners:
            p_[-1] = 0.9
    best = net.select(1)
    best = {k_: [int(v) for v in vs] for k_, vs in best.items()}
    arrays.update(sd_np(net, "selected::"))
    with torch.no_grad():
        for t, arch in ((0, arch0), (1, best)):
            del feas[:]
            arrays[f"disp_t{t}"] = net.forward(left, right, t, arch).numpy()
            arrays[f"left_fea_t{t}"], arrays[f"right_fea_t{t}"] = feas[0].numpy(), feas[1].numpy()
    for t, arch in ((0, arch0), (1, best)):
        f64[f"disp_t{t}"] = forward_f64(net, (arrays[f"left_fea_t{t}"], arrays[f"right_fea_t{t}"]),
                                        lambda n_, t=t, arch=arch: n_.forward(left.double(), right.double(), t, arch))
    save("g10_grown_model_f64", **f64)
    for h_ in hk:
        h_.remove()
    blob = {"arch_t0": arch0, "arch_t1": best, "winners": list(winners), "length": {k_: int(v) for k_, v in net.length.items()}}
    arrays["blob"] = np.frombuffer(json.dumps(blob).encode(), dtype=np.uint8)
    save("g10_grown_model", **arrays)

    # ------------------------------------------------------------------ G11: eval-loop loss + metrics
    # utilstool/metrics.py:21-65 with the mask and loss of approaches/rag.py:418-430.  metrics.py imports `make_nograd_func`
    # from utilstool/experiment.py, whose module-level `import torchvision.utils as vutils` (experiment.py:7) serves an image
    # logger (experiment.py:87) that the metric functions never reach; torchvision is not installed here.  Harness-side shim of
    # the same class as `current_device` above: an EMPTY placeholder module under that name, so the import statement succeeds —
    # no function of it is ever called, and none is defined.
    import types
    if "torchvision" not in sys.modules:
        tv = types.ModuleType("torchvision")
        tv.utils = types.ModuleType("torchvision.utils")
        sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tv.utils
    import warnings
    import torch.nn.functional as F
    from utilstool.metrics import D1_metric, EPE_metric, Thres_metric
    max_disp = 192                                         # rag.py:60
    gen = torch.Generator().manual_seed(1111)
    arrays = {}

    def metric_case(tag, est, gt):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                # size_average= is deprecated spelling of reduction="mean"
            mask = (gt < max_disp) & (gt > 0)                                               # rag.py:418
            loss = F.smooth_l1_loss(est[mask], gt[mask], size_average=True)                 # rag.py:419
            vals = [loss, EPE_metric(est, gt, mask), D1_metric(est, gt, mask), Thres_metric(est, gt, mask, 1.0),
                    Thres_metric(est, gt, mask, 2.0), Thres_metric(est, gt, mask, 3.0)]     # rag.py:421-429
        arrays[f"{tag}::est"], arrays[f"{tag}::gt"] = est.numpy(), gt.numpy()
        arrays[f"{tag}::scalars"] = np.array([float(v) for v in vals], dtype=np.float64)     # loss, EPE, D1, Thres1, Thres2, Thres3

    # a: three ordinary images: gt ~ U(-10, 210) (zeros / negatives and >= 192 fall outside the mask), est = gt + noise of mixed sizes
    gt = torch.rand((3, 24, 40), generator=gen) * 220 - 10
    est = gt + torch.randn(gt.shape, generator=gen) * torch.tensor([0.5, 2.0, 6.0]).view(3, 1, 1)
    metric_case("a", est.contiguous(), gt)
    # b: image 1 keeps < 10 % of its gt > 0 pixels inside the mask (nearly all >= 192): the per-image wrapper skips it (metrics.py:31-32)
    gt = torch.rand((3, 16, 32), generator=gen) * 180 + 5
    gt[1] = 195 + torch.rand((16, 32), generator=gen) * 20
    gt[1, 0, :24] = 50.0                                   # 24 of 512 pixels = 4.7 % stay
    est = gt + torch.randn(gt.shape, generator=gen) * 3
    metric_case("b", est, gt)
    # c: every image is skipped: the metrics return 0 (metrics.py:36-38); the loss is still the mean over the few masked pixels
    gt = 200 + torch.rand((2, 8, 16), generator=gen) * 10
    gt[:, 0, :4] = 100.0
    est = gt - 1.7
    metric_case("c", est, gt)
    # d: exact thresholds: errors of exactly 1, 2, 3 px and 5 % (strict comparisons, metrics.py:46, 55)
    gt = torch.full((1, 4, 8), 40.0)
    est = gt.clone()
    est[0, 0, :4] += torch.tensor([1.0, 2.0, 3.0, 3.5])
    est[0, 1, :4] -= torch.tensor([1.0, 2.0, 3.0, 3.5])
    gt[0, 2, :] = 100.0
    est[0, 2, :4] = 100.0 + torch.tensor([3.0, 4.0, 5.0, 5.5])   # 5.5 / 100 > 0.05 and > 3
    metric_case("d", est, gt)
    save("g11_metrics", **arrays)


if __name__ == "__main__":
    main()
