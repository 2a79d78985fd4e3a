#!/usr/bin/env python3
"""Generate the unit-search fixture by running the REFERENCE itself (build container only), like make_golden.py (whose reference
import, `current_device` shim and writer this script reuses; the empty `torchvision` placeholder of G11 is restated below for
utilstool.metrics).  On a machine without the reference it exits with a message and changes nothing.

The step is the one `Appr.search_epoch` runs per batch for a task t > 0 (approaches/rag.py:344-406): `approaches/rag.py` itself
cannot be imported here (its imports reach the data loaders), so its preamble is restated: `utils.freeze_model` +
`modify_param(new_models, True)` (rag.py:89-90), the optimizer over `get_param(new_models)` (rag.py:72-82; lr 1e-3, weight decay
3e-4 for the fixture), `model.train()` followed by `.eval()` on every unit of the stems, `last_3_2d` and the cells (rag.py:345-368).

The model is g10's: base ALL_CONV, candidate MIXED_UNSORTED, maxdisp 48, the weights of g10_grown_model.npz (`search::`) loaded with
strict=True, so no weight is stored again.  t = 1, B = 2, 48x96; left, right = randn and gt = rand * 60 from Generator(7).

Paths: A = g10's sel_a, then C = [0]*17 + [1] on the same model and optimizer; D = [0]*18 on a fresh model.  Each sequence runs in
fp32 and on a .double() copy; the fp64 step is the yardstick and is stored rounded to float32, with, per tensor, the scalar
rel_max(fp32 step, fp64 step) = max |a32 - a64| / max |a64| that the tolerance rule of tests/test_search_step.py needs.

Files (each under the 1 MiB limit of a committed file; tests read them through one merged dict):
  g24_unit_search.npz          left, right, gt, sel_A/C/D, ``train_bn`` (JSON: BatchNorms in training mode), ``n_tensors``,
                               ``trainable`` (JSON: parameters in the optimizer), ``keys_A/C/D`` (JSON: .grad is not None),
                               ``moved_A/C`` (JSON: state-dict entries that changed), and per step S in A, C, D: ``disp_S`` (the
                               train-mode disparity, fp32), ``loss_S``, ``loss64_S``, ``norm_S``, ``norm64_S`` (pre-clip),
                               ``scalars_S`` (loss, EPE, D1, Thres1, Thres2, Thres3 of rag.py:386-394 on disp_S, as .item() floats);
                               steps C and D in full: ``grad64_S::<param>``, ``gdist_S::<param>``, ``delta64_S::<param>`` (after -
                               before), ``ddist_S::<param>``, ``stat64_S::<buffer>``, ``sdist_S::<buffer>`` (num_batches_tracked: int).
  g24_unit_search_a_grad.npz   ``grad64_A::``, ``gdist_A::``, ``stat64_A::``, ``sdist_A::``
  g24_unit_search_a_delta.npz  ``delta64_A::``, ``ddist_A::``

Usage:  python tests/golden/make_golden_unit_search.py
"""
import copy
import json
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import ALL_CONV, MIXED_UNSORTED, OUT, _import_reference, save  # noqa: E402

T = 1
SEL_C = [0] * 17 + [1]
SEL_D = [0] * 18
HYPER = dict(lr=1e-3, momentum=0.9, weight_decay=3e-4)
CLIP = 5.0


def _blob(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def rel_max(a32, a64):
    return float((a32.double() - a64.double()).abs().max()) / max(float(a64.double().abs().max()), 1e-30)


def search_mode(model):
    """rag.py:345-368"""
    model.train()
    for name in ("stem2d0", "stem2d1", "stem2d2", "last_3_2d", "stem3d0", "stem3d1"):
        for unit in getattr(model, name):
            unit.eval()
    for cells in (model.cells_2d, model.cells_3d):
        for units in cells:
            for unit in units:
                unit.eval()


def main():
    rm, Genotype = _import_reference()
    if "torchvision" not in sys.modules:                    # G11's placeholder: utilstool/experiment.py:7 imports it, nothing calls it
        tv = types.ModuleType("torchvision")
        tv.utils = types.ModuleType("torchvision.utils")
        sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tv.utils
    import utils
    from utilstool.metrics import D1_metric, EPE_metric, Thres_metric
    torch.set_num_threads(8)
    g10 = np.load(os.path.join(OUT, "g10_grown_model.npz"))
    sd = {k[len("search::"):]: torch.from_numpy(g10[k]) for k in g10.files if k.startswith("search::")}
    sel_a = [int(v) for v in g10["sel_a"]]
    maxdisp = int(g10["maxdisp"])

    def genotype(rows):
        return Genotype(normal=rows, normal_concat=None, reduce=rows, reduce_concat=None)

    def model(dtype):
        net = rm.Network(genotype(ALL_CONV), "cpu")
        net.maxdisp = maxdisp
        net.disp = rm.Disp(maxdisp)
        net.expand(T, genotype(MIXED_UNSORTED), "cpu")
        net.load_state_dict(sd, strict=True)
        utils.freeze_model(net)                              # rag.py:89-90
        net.modify_param(net.new_models, True)
        net = net.to(dtype)
        search_mode(net)
        opt = torch.optim.SGD(net.get_param(net.new_models), **HYPER)      # rag.py:72-82
        return net, opt

    gen = torch.Generator().manual_seed(7)
    left = torch.randn((2, 3, 48, 96), generator=gen)
    right = torch.randn((2, 3, 48, 96), generator=gen)
    gt = torch.rand((2, 48, 96), generator=gen) * 60

    def step(net, opt, sel, dtype):
        """One batch of search_epoch (rag.py:371-396)."""
        before = {k: v.detach().clone() for k, v in net.state_dict().items()}
        est = net.search_forward(left.to(dtype), right.to(dtype), T, sel)
        gtd = gt.to(dtype)
        mask = (gtd < maxdisp) & (gtd > 0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss = F.smooth_l1_loss(est[mask], gtd[mask], size_average=True)
        opt.zero_grad()
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        total = torch.nn.utils.clip_grad_norm_(net.parameters(), CLIP)
        opt.step()
        with torch.no_grad():
            vals = [loss, EPE_metric(est, gtd, mask), D1_metric(est, gtd, mask), Thres_metric(est, gtd, mask, 1.0),
                    Thres_metric(est, gtd, mask, 2.0), Thres_metric(est, gtd, mask, 3.0)]
        after = {k: v.detach().clone() for k, v in net.state_dict().items()}
        moved = sorted(k for k in after if not torch.equal(after[k], before[k]))
        saturated = float(((est <= 0) | (est >= maxdisp - 1)).float().mean())
        return dict(est=est.detach(), loss=loss.item(), total=float(total), grads=grads, before=before, after=after, moved=moved,
                    scalars=np.array([float(v) for v in vals], dtype=np.float64), saturated=saturated,
                    n_momentum=sum(1 for s in opt.state.values() if "momentum_buffer" in s))

    def run(dtype):
        net, opt = model(dtype)
        a = step(net, opt, sel_a, dtype)
        c = step(net, opt, SEL_C, dtype)
        net_d, opt_d = model(dtype)
        d = step(net_d, opt_d, SEL_D, dtype)
        return net, opt, dict(A=a, C=c, D=d)

    net, opt, r32 = run(torch.float32)
    _net64, _opt64, r64 = run(torch.float64)

    params = dict(net.named_parameters())
    trainable = sorted(k for k, p in params.items() if p.requires_grad)
    in_opt = {id(p) for grp in opt.param_groups for p in grp["params"]}
    assert sorted(k for k, p in params.items() if id(p) in in_opt) == trainable
    train_bn = sorted(k for k, m in net.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training)
    main_f = dict(left=left.numpy(), right=right.numpy(), gt=gt.numpy(), sel_A=np.array(sel_a), sel_C=np.array(SEL_C),
                  sel_D=np.array(SEL_D), t=np.int64(T), maxdisp=np.int64(maxdisp), train_bn=_blob(train_bn),
                  n_tensors=np.int64(len(params)), trainable=_blob(trainable), hyper=_blob(dict(HYPER, clip=CLIP)))
    a_grad, a_delta = {}, {}
    for tag in ("A", "C", "D"):
        s32, s64 = r32[tag], r64[tag]
        keys = sorted(s32["grads"])
        assert keys == sorted(s64["grads"]) and s32["moved"] == s64["moved"]
        assert s32["saturated"] == 0.0, "a disparity saturates: the step would be ill-conditioned"
        moved_params = [k for k in s32["moved"] if k in params]
        assert moved_params == keys, "exactly the parameters with a gradient move"
        main_f.update({f"keys_{tag}": _blob(keys), f"moved_{tag}": _blob(s32["moved"]), f"disp_{tag}": s32["est"].numpy(),
                       f"loss_{tag}": np.float64(s32["loss"]), f"loss64_{tag}": np.float64(s64["loss"]),
                       f"norm_{tag}": np.float64(s32["total"]), f"norm64_{tag}": np.float64(s64["total"]),
                       f"scalars_{tag}": s32["scalars"], f"n_momentum_{tag}": np.int64(s32["n_momentum"])})
        gdst, ddst = (a_grad, a_delta) if tag == "A" else (main_f, main_f)
        worst = 0.0
        for k in keys:
            gdst[f"grad64_{tag}::{k}"] = s64["grads"][k].float().numpy()
            gdst[f"gdist_{tag}::{k}"] = np.float64(rel_max(s32["grads"][k], s64["grads"][k]))
            worst = max(worst, float(gdst[f"gdist_{tag}::{k}"]))
            d32, d64 = s32["after"][k] - s32["before"][k], s64["after"][k] - s64["before"][k]
            ddst[f"delta64_{tag}::{k}"] = d64.float().numpy()
            ddst[f"ddist_{tag}::{k}"] = np.float64(rel_max(d32, d64))
        for k in s32["moved"]:
            if k in params:
                continue
            if s32["after"][k].is_floating_point():
                gdst[f"stat64_{tag}::{k}"] = s64["after"][k].float().numpy()
                gdst[f"sdist_{tag}::{k}"] = np.float64(rel_max(s32["after"][k], s64["after"][k]))
            else:
                gdst[f"stat64_{tag}::{k}"] = s64["after"][k].numpy()
        nbytes = sum(s32["grads"][k].numel() * 4 for k in keys)
        print(f"g24 step {tag}: loss {s32['loss']:.6f} (fp64 {s64['loss']:.6f}), norm {s32['total']:.4f}, {len(keys)} gradients "
              f"({nbytes} B) of {len(trainable)} trainable / {len(params)} tensors, {len(s32['moved'])} moved, "
              f"{s32['n_momentum']} momentum buffers, fp32 vs fp64 gradients up to {worst:.2e}")
    # the tensors A updated and C did not are bit for bit what A left (values; torch creates no new momentum buffer for them)
    a_only = sorted(set(r32["A"]["grads"]) - set(r32["C"]["grads"]))
    assert all(torch.equal(r32["C"]["after"][k], r32["A"]["after"][k]) for k in a_only)
    main_f["a_only"] = _blob(a_only)
    save("g24_unit_search", **main_f)
    save("g24_unit_search_a_grad", **a_grad)
    save("g24_unit_search_a_delta", **a_delta)


if __name__ == "__main__":
    main()
