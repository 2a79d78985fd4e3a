#!/usr/bin/env python3
"""Generate the monocular-depth fixtures by running the REFERENCE itself (build container only).

Imports chzhang18/RAG's monocular-depth tree from /root/reference/rag_depth/src (read-only), runs its own Network, DispHead,
silog_loss and compute_errors on CPU, and writes inputs + outputs as small ``.npz`` fixtures next to this script.  On a machine
without the reference this script exits with a message and changes nothing.

Harness-side shims (the same class as make_golden.py's):
  * ``torch.cuda.current_device`` -> CPU: DisparityRegression (models/rag_model.py) builds on it;
  * empty placeholder modules for ``torchvision`` (+ ``.utils``, ``.transforms``) and ``torch.utils.tensorboard``, which
    utilstool/experiment.py and approaches/rag.py import but the two metric functions never use.

Fixtures:
  g14_depth_ckpt_task3.npz   the ``model`` state_dict of the shipped logs/checkpoint_task3.ckpt (trained weights), one array per key.
  g15_depth_forward.npz      the reference forward on g14's weights: ``rows`` (JSON: the stand-in genotype rows of every cell unit,
                             rag_amd.depth.rows_from_keys's rule), images ``img{i}`` (B=2 48x96, B=1 36x60), archis ``archi{t}`` (JSON,
                             per layer min(t, n_units - 1)), outputs ``out{i}_{t}``; search_forward cases ``sops{k}`` / ``st{k}`` /
                             ``sout{k}_{i}``.
  g16_depth_head.npz         upsample_6 -> last_3_3d -> DispHead(., 3) -> x 80 on random y6 / weights: ``case{k}_{y,w3,w1,b1,hw,out}``;
                             ``case{k}_out64`` is the same reference run in fp64 (stored rounded to fp32); the last case has large |m| so that the sigmoid
                             saturates.
  g17_depth_metrics.npz      B=3 est / gt (some gt == 0) through silog_loss (variance focus 0.85) and compute_errors: ``est``, ``gt``,
                             ``out`` (10 values, float64).
  g18_depth_growth_api.npz   key / shape lists of the reference Network after a scripted expand / select sequence (JSON ``blob``).

Usage:  python tests/golden/make_golden_depth.py
"""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference/rag_depth/src"
CKPT = "/root/reference/rag_depth/logs/checkpoint_task3.ckpt"
OUT = os.path.dirname(os.path.abspath(__file__))
BRANCHES = (0, 1, 2, 3, 5, 6)
ATTR = {"stem_2d0": "stem2d0", "stem_2d1": "stem2d1", "stem_2d2": "stem2d2", "last_3_2d": "last_3_2d", "stem_3d0": "stem3d0",
        "stem_3d1": "stem3d1", "last_3_3d": "last_3_3d", "last_6_3d": "last_6_3d", "last_12_3d": "last_12_3d"}
LAYERS = (["stem_2d0", "stem_2d1", "stem_2d2"] + [f"cell_2d{i}" for i in range(4)] + ["last_3_2d", "stem_3d0", "stem_3d1"]
          + [f"cell_3d{i}" for i in range(8)])
HEADS = ("last_3_3d", "last_6_3d", "last_12_3d")


def _import_reference():
    if not os.path.isdir(REF) or not os.path.exists(CKPT):
        print("reference not present; golden fixtures are used as committed")
        sys.exit(0)
    sys.path.insert(0, REF)
    torch.cuda.current_device = lambda: torch.device("cpu")
    for name in ("torchvision", "torchvision.utils", "torchvision.transforms", "torch.utils.tensorboard"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    import models.rag_model as rm  # noqa
    from automl.genotypes_2d import Genotype  # noqa
    import utilstool.experiment as ex  # noqa
    import approaches.rag as appr  # noqa
    return rm, Genotype, ex, appr


def save(name, **arrays):
    """np.savez_compressed's layout with a fixed member date, so that a rerun rewrites the fixtures bit for bit."""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    print(f"{name}.npz  {size / 1024:.1f} KiB")
    assert size < 1024 * 1024, "fixture over the 1 MiB limit"


def units(net, name):
    if name.startswith("cell_2d"):
        return net.cells_2d[int(name[7:])]
    if name.startswith("cell_3d"):
        return net.cells_3d[int(name[7:])]
    return getattr(net, ATTR[name])


def rows_of(keys, prefix):
    return [[b, int(f"{prefix}_ops.{j}.conv.weight" in keys)] for j, b in enumerate(BRANCHES)]


def counts_of(keys):
    out = {}
    for name in LAYERS + list(HEADS):
        if name.startswith("cell_"):
            pre = ("cells_2d." if name.startswith("cell_2d") else "cells_3d.") + name[7:] + "."
        else:
            pre = ATTR[name] + "."
        idx = {int(k[len(pre):].split(".")[0]) for k in keys if k.startswith(pre)}
        out[name] = max(idx) + 1
    return out


def build_grown(rm, Genotype, sd):
    """The reference Network with one unit per key group, each cell unit built from its stand-in rows."""
    keys = set(sd.keys())
    counts = counts_of(keys)
    rows = {}
    for name in LAYERS:
        if name.startswith("cell_"):
            attr = "cells_2d" if name.startswith("cell_2d") else "cells_3d"
            rows[name] = [rows_of(keys, f"{attr}.{name[7:]}.{k}.") for k in range(counts[name])]
    geno = lambda r: Genotype(normal=np.array(r), normal_concat=None, reduce=np.array(r), reduce_concat=None)  # noqa: E731
    net = rm.Network(geno(rows["cell_3d0"][0]), "cpu")
    for name in LAYERS + list(HEADS):
        lst = units(net, name)
        for k in range(counts[name]):
            if name.startswith("cell_"):
                unit = units(rm.Network(geno(rows[name][k]), "cpu"), name)[0]
            else:
                unit = units(rm.Network(geno(rows["cell_3d0"][0]), "cpu"), name)[0]
            if k == 0:
                lst[0] = unit
            else:
                lst.append(unit)
        if name not in HEADS:
            net.length[name] = counts[name]
    net.load_state_dict(sd, strict=True)
    return net.eval(), rows, counts


def main():
    rm, Genotype, ex, appr = _import_reference()
    torch.set_num_threads(1)

    # ---- G14: the trained task-3 weights
    ck = torch.load(CKPT, map_location="cpu", weights_only=True)
    sd = ck["model"]
    save("g14_depth_ckpt_task3", **{k: v.numpy() for k, v in sd.items()})

    # ---- G15: reference forward on those weights
    net, rows, counts = build_grown(rm, Genotype, sd)
    gen = torch.Generator().manual_seed(151)
    imgs = [torch.rand((2, 3, 48, 96), generator=gen) * 2 - 1, torch.rand((1, 3, 36, 60), generator=gen) * 2 - 1]
    arrays = {"rows": np.frombuffer(json.dumps(rows).encode(), dtype=np.uint8)}
    with torch.no_grad():
        for t in range(4):
            archi = {name: [min(t, counts[name] - 1)] for name in LAYERS + list(HEADS)}
            arrays[f"archi{t}"] = np.frombuffer(json.dumps(archi).encode(), dtype=np.uint8)
            for i, img in enumerate(imgs):
                arrays[f"out{i}_{t}"] = net(img, img, t, archi).numpy()
        sops = [([counts[n] - 1 for n in LAYERS], 3), ([(k * 7 + 1) % counts[n] for k, n in enumerate(LAYERS)], 1)]
        for k, (ops_, t) in enumerate(sops):
            arrays[f"sops{k}"] = np.array(ops_, dtype=np.int64)
            arrays[f"st{k}"] = np.int64(t)
            for i, img in enumerate(imgs):
                arrays[f"sout{k}_{i}"] = net.search_forward(img, img, t, ops_).numpy()
    for i, img in enumerate(imgs):
        arrays[f"img{i}"] = img.numpy()
    lo = min(float(v.min()) for k, v in arrays.items() if k.startswith("out"))
    hi = max(float(v.max()) for k, v in arrays.items() if k.startswith("out"))
    print(f"g15 depth range {lo:.2f} .. {hi:.2f} m")
    save("g15_depth_forward", **arrays)

    # ---- G16: the head alone (fp32, and the same modules in fp64: the kernel is checked against the fp64 output)
    torch.manual_seed(161)
    arrays = {}
    cases = [(16, 32), (12, 20), (40, 132), (12, 20)]
    for k, (h, w) in enumerate(cases):
        last3 = rm.ConvBR_2d(12, 1, 3, 1, 1, bn=False, relu=False)
        head = rm.DispHead(1)
        y = torch.randn((2, 12, h // 2, w // 2))
        if k < 3:
            with torch.no_grad():
                last3.conv.weight.mul_(0.1)           # |m| ~ 1, depths spread over the range as a trained head's are
        else:
            # large |m| of one sign per half image: the sigmoid saturates at 0 and at 1 (without cancellation in m)
            y[..., : w // 4] += 1.5
            y[..., w // 4:] -= 1.5
            with torch.no_grad():
                last3.conv.weight.copy_(torch.rand(last3.conv.weight.shape) * 3)
                head.conv1.weight.copy_(torch.rand(head.conv1.weight.shape) * 0.2 + 0.05)
        up6 = nn.Upsample(size=(h, w), mode="bilinear", align_corners=True)
        with torch.no_grad():
            out = torch.squeeze(head(last3(up6(y)), 3), 1) * 80
            out64 = torch.squeeze(head.double()(last3.double()(up6(y.double())), 3), 1) * 80
        arrays.update({f"case{k}_y": y.numpy(), f"case{k}_w3": last3.conv.weight.detach().float().numpy(),
                       f"case{k}_w1": head.conv1.weight.detach().float().numpy(), f"case{k}_b1": head.conv1.bias.detach().float().numpy(),
                       f"case{k}_hw": np.array([h, w], dtype=np.int64), f"case{k}_out": out.numpy(), f"case{k}_out64": out64.float().numpy()})
        sat = float(((out < 0.01) | (out > 79.99)).float().mean())
        print(f"g16 case {k} {h}x{w}: out {float(out.min()):.3f} .. {float(out.max()):.3f}, saturated {sat:.2f}, "
              f"fp32 vs fp64 {float((out.double() - out64).abs().max()):.2e}")
    save("g16_depth_head", **arrays)

    # ---- G17: silog_loss + compute_errors on a batch with holes in the ground truth
    gen = torch.Generator().manual_seed(171)
    est = torch.rand((3, 48, 96), generator=gen) * 70 + 1
    gt = est * torch.exp(torch.randn((3, 48, 96), generator=gen) * 0.2)
    gt[torch.rand((3, 48, 96), generator=gen) < 0.3] = 0
    loss = ex.silog_loss()(est, gt, gt > 0)
    errs = appr.compute_errors(gt.numpy()[gt.numpy() > 0], est.numpy()[gt.numpy() > 0])
    save("g17_depth_metrics", est=est.numpy(), gt=gt.numpy(), out=np.array([float(loss)] + [float(e) for e in errs], dtype=np.float64))

    # ---- G18: growth-API bookkeeping (rag_model.py:420-800)
    torch.manual_seed(181)
    all_conv = [[0, 1], [1, 1], [2, 1], [3, 1], [5, 1], [6, 1]]
    mixed = [[0, 1], [1, 0], [2, 1], [3, 1], [5, 0], [6, 1]]
    geno = lambda r: Genotype(normal=np.array(r), normal_concat=None, reduce=np.array(r), reduce_concat=None)  # noqa: E731
    shapes = lambda m: [[k, list(v.shape)] for k, v in sorted(m.state_dict().items())]  # noqa: E731
    to_int = lambda d: {k: [int(v) for v in vs] for k, vs in d.items()}  # noqa: E731
    g = rm.Network(geno(all_conv), "cpu")
    blob = {"shapes_initial": shapes(g), "arch_init": to_int(g.arch_init)}
    g.expand(1, geno(mixed), "cpu")
    blob["shapes_expanded"] = shapes(g)
    blob["p_after_expand"] = [p.numpy().tolist() for p in g.p]
    blob["new_models"] = to_int(g.new_models)
    winners = (0, 4, 9, 13)
    for k, p in enumerate(g.p):
        if k in winners:
            p[-1] = 0.9
    blob["winners"] = list(winners)
    blob["best_archi"] = to_int(g.select(1))
    blob["model_to_train"] = to_int(g.model_to_train)
    blob["length"] = {k: int(v) for k, v in g.length.items()}
    blob["shapes_selected"] = shapes(g)
    save("g18_depth_growth_api", blob=np.frombuffer(json.dumps(blob).encode(), dtype=np.uint8))


if __name__ == "__main__":
    main()
