#!/usr/bin/env python3
"""Generate the depth unit-search fixture by running the REFERENCE itself (build container only), like make_golden_unit_search.py;
the reference import, the grown-model builder and the writer are make_golden_depth.py's.  On a machine without the reference it
exits with a message and changes nothing.

The step is the one `Appr.search_epoch` of rag_depth runs per batch for a task t > 0 (approaches/rag.py:371-427), the eval batch is
`Appr.search_eval`'s (rag.py:492-522).  The preamble is the reference's: `utils.freeze_model` + `modify_param(new_models, True)`,
the optimizer over `get_param(new_models)` (lr 1e-3, momentum 0.9, weight decay 3e-4 for the fixture), clip 5, `model.train()`
followed by `.eval()` on every unit of the stems, `last_3_2d` and the cells (rag.py:372-394).

The model is g14's trained task-3 weights (read from g14_depth_ckpt_task3.npz, not stored again) through `build_grown`, then
`torch.manual_seed(3)` and `expand(4, geno(MIXED), "cpu")`: the candidate's and the new heads' state-dict entries are stored as
``new::<key>``.  t = 4, B = 2, 48x96; left = rand(Generator(7)) * 2 - 1, gt = rand(Generator(GT_SEED)) * 70 + 2 with 0 where
rand(Generator(10)) < 0.3.

Paths, in this order on ONE model and ONE optimizer: A alternates candidates and reused units, C = [0]*17 + [2] trains cell_3d7's
candidate and the heads, D reuses every unit (only the heads train).  Each sequence runs in fp32 and on a .double() copy; the fp64
step is the yardstick and is stored rounded to float32, with, per tensor, rel_max(fp32 step, fp64 step) = max |a32 - a64| /
max |a64|.

Files (each under the 1 MiB limit of a committed file; tests read them through one merged dict):
  g25_depth_unit_search.npz          ``new::<key>``, left, gt, sel_A/C/D, t, ``counts`` (units per layer of p after expand), ``train_bn``
                                     (JSON: BatchNorms in training mode), ``n_tensors``, ``trainable`` (JSON), ``keys_S`` (JSON:
                                     .grad is not None), ``moved_S`` (JSON: state-dict entries that changed), ``a_only`` (JSON), and
                                     per step S in A, C, D: ``est_S`` (the train-mode depth, fp32), ``loss_S``, ``loss64_S``,
                                     ``norm_S``, ``norm64_S`` (pre-clip), ``scalars_S`` (the loss's .item() and compute_errors' nine
                                     entries of rag.py:416-427 on est_S, each as the float the loop holds), ``inside_S``; ``epoch_avg``
                                     (the ten averages as the loop accumulates them: the loss through AverageMeterDict, the others as
                                     ``0 + entry`` sums divided by the count); steps C and D in full: ``grad64_S::<param>``,
                                     ``gdist_S::<param>``, ``delta64_S::<param>``, ``ddist_S::<param>``, ``stat64_S::<buffer>``,
                                     ``sdist_S::<buffer>``; before any step ``eval_est_A/D`` and ``eval_scalars_A/D`` (eval()
                                     search_forward, rag.py:501-522).
  g25_depth_unit_search_a_grad.npz   ``grad64_A::``, ``gdist_A::``, ``stat64_A::``, ``sdist_A::``
  g25_depth_unit_search_a_delta.npz  ``delta64_A::``, ``ddist_A::``

Usage:  python tests/golden/make_golden_depth_unit_search.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_depth import LAYERS, OUT, _import_reference, build_grown, save, units  # noqa: E402

T = 4
MIXED = [[0, 1], [1, 0], [2, 1], [3, 1], [5, 0], [6, 1]]
COUNTS = [4, 4, 4, 4, 4, 5, 3, 4, 3, 4, 3, 5, 4, 4, 4, 4, 4, 3]
SEL_A = [3, 2, 3, 1, 3, 0, 2, 2, 2, 1, 2, 2, 3, 2, 3, 1, 3, 0]
SEL_C = [0] * 17 + [2]
SEL_D = [2, 2, 2, 2, 2, 3, 1, 2, 1, 2, 1, 3, 2, 2, 2, 2, 2, 1]
HYPER = dict(lr=1e-3, momentum=0.9, weight_decay=3e-4)
CLIP = 5.0
GT_SEED = 11          # 9 puts a pixel 8e-6 from 1.25^3 in step A; 11 is the next seed (10 draws the holes) that meets both conditions


def _blob(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def rel_max(a32, a64):
    return float((a32.double() - a64.double()).abs().max()) / max(float(a64.double().abs().max()), 1e-30)


def search_mode(model):
    """rag.py:372-394"""
    model.train()
    for name in LAYERS:
        for unit in units(model, name):
            unit.eval()


def check_thresholds(est, gt, what):
    """No masked pixel's max(gt/est, est/gt) within 1e-5 relative of a d1-d3 threshold: the counts are then the same integers in
    fp32 and fp64, and for an implementation whose depth differs in the last bits."""
    m = gt > 0
    th = torch.maximum(gt[m].double() / est[m].double(), est[m].double() / gt[m].double())
    for k in (1, 2, 3):
        near = float(((th / 1.25 ** k) - 1).abs().min())
        assert near > 1e-5, f"{what}: a pixel sits {near:.1e} from 1.25^{k}: change GT_SEED"


def main():
    rm, Genotype, ex, appr = _import_reference()
    import utils
    torch.set_num_threads(8)
    g14 = dict(np.load(os.path.join(OUT, "g14_depth_ckpt_task3.npz")))
    sd = {k: torch.as_tensor(v) for k, v in g14.items()}
    geno = lambda r: Genotype(normal=np.array(r), normal_concat=None, reduce=np.array(r), reduce_concat=None)  # noqa: E731
    crit = ex.silog_loss()

    net32, _rows, _counts = build_grown(rm, Genotype, sd)
    old_keys = set(net32.state_dict().keys())
    torch.manual_seed(3)
    net32.expand(T, geno(MIXED), "cpu")
    assert [len(units(net32, n)) for n in LAYERS] == COUNTS
    new = {k: v.detach().clone() for k, v in net32.state_dict().items() if k not in old_keys}
    print(f"g25: {len(new)} new state-dict entries, {sum(v.numel() for v in new.values())} values")
    utils.freeze_model(net32)                                # rag.py:89-90 of this tree's train()
    net32.modify_param(net32.new_models, True)
    net64 = copy.deepcopy(net32).double()

    left = torch.rand((2, 3, 48, 96), generator=torch.Generator().manual_seed(7)) * 2 - 1
    gt = torch.rand((2, 48, 96), generator=torch.Generator().manual_seed(GT_SEED)) * 70 + 2
    gt[torch.rand((2, 48, 96), generator=torch.Generator().manual_seed(10)) < 0.3] = 0

    def scalars(loss, est, gtd):
        """rag.py:416-427 / 511-522: the loss's float and compute_errors on the host gather, each as the loop holds it."""
        g, e = gtd.cpu().numpy(), est.detach().cpu().numpy()
        mask = g > 0
        errs = appr.compute_errors(g[mask], e[mask])
        return [ex.tensor2float({"loss": loss})["loss"]] + list(errs)

    # ---- eval() search_forward of A and D before any step (rag.py:492-522)
    main_f = {}
    net32.eval()
    with torch.no_grad():
        for tag, sel in (("A", SEL_A), ("D", SEL_D)):
            est = net32.search_forward(left, left, T, sel)
            loss = crit.forward(est, gt, (gt > 0).to(torch.bool))
            check_thresholds(est, gt, f"eval {tag}")
            main_f[f"eval_est_{tag}"] = est.numpy()
            main_f[f"eval_scalars_{tag}"] = np.array([float(v) for v in scalars(loss, est, gt)], dtype=np.float64)

    def step(net, opt, sel, dtype):
        """One batch of search_epoch (rag.py:401-427)."""
        before = {k: v.detach().clone() for k, v in net.state_dict().items()}
        gtd = gt.to(dtype)
        est = net.search_forward(left.to(dtype), left.to(dtype), T, sel)
        mask = gtd > 0
        loss = crit.forward(est, gtd, mask.to(torch.bool))
        opt.zero_grad()
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        total = torch.nn.utils.clip_grad_norm_(net.parameters(), CLIP)
        opt.step()
        with torch.no_grad():
            vals = scalars(loss, est, gtd)
        after = {k: v.detach().clone() for k, v in net.state_dict().items()}
        moved = sorted(k for k in after if not torch.equal(after[k], before[k]))
        inside = float(((est > 1) & (est < 79)).double().mean())
        return dict(est=est.detach(), loss=loss.item(), total=float(total), grads=grads, before=before, after=after, moved=moved,
                    vals=vals, inside=inside)

    def run(net, dtype):
        search_mode(net)
        opt = torch.optim.SGD(net.get_param(net.new_models), **HYPER)
        return opt, {tag: step(net, opt, sel, dtype) for tag, sel in (("A", SEL_A), ("C", SEL_C), ("D", SEL_D))}

    opt, r32 = run(net32, torch.float32)
    _opt64, r64 = run(net64, torch.float64)

    params = dict(net32.named_parameters())
    trainable = sorted(k for k, p in params.items() if p.requires_grad)
    in_opt = {id(p) for grp in opt.param_groups for p in grp["params"]}
    assert sorted(k for k, p in params.items() if id(p) in in_opt) == trainable
    train_bn = sorted(k for k, m in net32.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training)
    main_f.update({f"new::{k}": v.numpy() for k, v in new.items()})
    main_f.update(left=left.numpy(), gt=gt.numpy(), sel_A=np.array(SEL_A), sel_C=np.array(SEL_C), sel_D=np.array(SEL_D),
                  t=np.int64(T), counts=np.array(COUNTS), mixed=np.array(MIXED), train_bn=_blob(train_bn),
                  n_tensors=np.int64(len(params)), trainable=_blob(trainable), hyper=_blob(dict(HYPER, clip=CLIP)))

    # ---- the epoch averages as the loop accumulates them (rag.py:397-400, 419, 425-427, 432-436)
    meter = ex.AverageMeterDict()
    sums = [0] * 9
    for tag in ("A", "C", "D"):
        vals = r32[tag]["vals"]
        meter.update({"loss": vals[0]})
        for k in range(9):
            sums[k] += vals[1 + k]
    assert sums[1].dtype == np.float32 and sums[3].dtype == np.float32 and sums[6].dtype == np.float64
    main_f["epoch_avg"] = np.array([float(meter.mean()["loss"])] + [float(s / 3) for s in sums], dtype=np.float64)

    a_grad, a_delta = {}, {}
    for tag in ("A", "C", "D"):
        s32, s64 = r32[tag], r64[tag]
        keys = sorted(s32["grads"])
        assert keys == sorted(s64["grads"]) and s32["moved"] == s64["moved"]
        assert s32["inside"] >= 0.9, f"step {tag}: only {s32['inside']:.3f} of the depths inside (1, 79) m: change GT_SEED"
        check_thresholds(s32["est"], gt, f"step {tag}")
        moved_params = [k for k in s32["moved"] if k in params]
        assert moved_params == keys, "exactly the parameters with a gradient move"
        main_f.update({f"keys_{tag}": _blob(keys), f"moved_{tag}": _blob(s32["moved"]), f"est_{tag}": s32["est"].numpy(),
                       f"loss_{tag}": np.float64(s32["loss"]), f"loss64_{tag}": np.float64(s64["loss"]),
                       f"norm_{tag}": np.float64(s32["total"]), f"norm64_{tag}": np.float64(s64["total"]),
                       f"scalars_{tag}": np.array([float(v) for v in s32["vals"]], dtype=np.float64),
                       f"inside_{tag}": np.float64(s32["inside"])})
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
        print(f"g25 step {tag}: loss {s32['loss']:.6f} (fp64 {s64['loss']:.6f}), norm {s32['total']:.4f}, {len(keys)} gradients of "
              f"{len(trainable)} trainable / {len(params)} tensors, {len(s32['moved'])} moved, inside (1, 79) m {s32['inside']:.3f}, "
              f"fp32 vs fp64 gradients up to {worst:.2e}")
    # the tensors A updated and C, D did not are bit for bit what A left
    a_only = sorted(set(r32["A"]["grads"]) - set(r32["C"]["grads"]) - set(r32["D"]["grads"]))
    assert all(torch.equal(r32["D"]["after"][k], r32["A"]["after"][k]) for k in a_only)
    main_f["a_only"] = _blob(a_only)
    save("g25_depth_unit_search", **main_f)
    save("g25_depth_unit_search_a_grad", **a_grad)
    save("g25_depth_unit_search_a_delta", **a_delta)


if __name__ == "__main__":
    main()
