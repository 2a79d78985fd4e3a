"""The unit search's step on the HIP path (Appr.search_epoch / search_eval, approaches/rag.py:344-406, 443-470): Network.search_mode,
Network.active_parameters(t, selected_ops), the `selected_ops=, t=, meter=` step of rag_amd.train, search_eval_step, and the device
epoch meter (rag_amd.metrics.EpochMeter, ragmi_stereo_metrics_meter_fwd), against the REFERENCE's own numbers: g24 (generator
tests/golden/make_golden_unit_search.py, three files read as one dict; the weights are g10's `search::` entries) and g11.

Gates.  Tensors of the training step: against the reference's fp64 step at max(floor, 3 x the reference's own fp32 distance from it,
stored per tensor), floors 5e-4 (gradients), 1e-4 (running statistics), 2e-3 (updates): the rule and the floors of
tests/test_search_step.py.  Loss: 2e-4 relative to the fp64 step.  Metric scalars: g11's 2e-5 * max(1, |v|).  Meter sums: bit for bit
the sequential Python-double sum of the floats the kernel stored.

Unmarked tests run without a GPU; the rest need the MI355X."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, split_sd

DEV = "cuda:0"
FAKE = ctypes.c_void_p(256)      # a non-NULL pointer for argument checks that must refuse before any launch (never dereferenced)
T = 1
FLOOR = {"grad": 5e-4, "stat": 1e-4, "delta": 2e-3}


@functools.lru_cache(maxsize=None)
def g24():
    out = {}
    for name in ("g24_unit_search", "g24_unit_search_a_grad", "g24_unit_search_a_delta"):
        out.update(load_golden(name))
    return out


@functools.lru_cache(maxsize=None)
def g10():
    return load_golden("g10_grown_model")


def _json(a):
    return json.loads(bytes(a).decode())


def _sel(tag):
    return [int(v) for v in g24()["sel_" + tag]]


def gpu(x):
    return torch.as_tensor(np.asarray(x)).to(DEV)


def rel_max(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def close(got, ref, tol, what=""):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float((got - ref).abs().max())
    bound = tol * max(1.0, float(ref.abs().max()))
    assert err <= bound, (what, err, bound)


def _net(device, mode="search"):
    """g10's expanded model (base ALL_CONV, candidate MIXED_UNSORTED, maxdisp 48) after the preamble of rag.py:89-90:
    freeze_model + modify_param(new_models, True)."""
    import rag_amd
    g = g10()
    geno0 = rag_amd.Genotype(g["rows_unit0"], None, g["rows_unit0"], None)
    geno1 = rag_amd.Genotype(g["rows_unit1"], None, g["rows_unit1"], None)
    net = rag_amd.Network(geno0, device, maxdisp=int(g["maxdisp"]))
    net.expand(T, geno1, "cpu")
    net.load_state_dict(split_sd(g, "search::"), strict=True)
    net = net.to(device)
    for p in net.parameters():
        p.requires_grad = False
    net.modify_param(net.new_models, True)
    return net.search_mode() if mode == "search" else net.eval()


def _names(net, params):
    by_id = {id(p): k for k, p in net.named_parameters()}
    return sorted(by_id[id(p)] for p in params)


# --------------------------------------------------------------------------- CPU
def test_search_mode_leaves_the_reference_batchnorms_training():
    net = _net("cpu", mode="eval")
    assert net.search_mode() is net and net.training
    bns = sorted(k for k, m in net.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training)
    assert bns == _json(g24()["train_bn"]) and len(bns) == 6
    assert all(k.startswith("last_") and "_3d." in k for k in bns)


def test_active_parameters_are_the_reference_gradient_sets():
    g = g24()
    net = _net("cpu")
    assert len(list(net.parameters())) == int(g["n_tensors"]) == 522
    assert sorted(k for k, p in net.named_parameters() if p.requires_grad) == _json(g["trainable"])
    for tag, n in (("A", 119), ("C", 22), ("D", 7)):
        a = _names(net, net.active_parameters(T, g["sel_" + tag]))
        assert a == _json(g["keys_" + tag]) and len(a) == len(set(a)) == n, tag
        assert not any(k.startswith(("last_3_2d", "last_3_3d")) and ".bn." in k for k in a)       # bn=False units
    assert len(_json(g["trainable"])) == 207
    assert net.active_parameters(0, _sel("D")) == []          # task 0's head is frozen


def test_unit_search_step_refusals():
    import rag_amd
    from rag_amd.train import GradBucket, GraphedTrainStep, forward_backward, search_eval_step, train_step
    net = _net("cpu")
    bucket = GradBucket(net.parameters())
    left, gt = torch.zeros((1, 3, 48, 96)), torch.ones((1, 48, 96))
    A = _sel("A")
    steps = (lambda **kw: forward_backward(net, bucket, left, left, kw.pop("gt", gt), **kw),
             lambda **kw: train_step(net, None, bucket, left, left, kw.pop("gt", gt), **kw),
             lambda **kw: GraphedTrainStep(net, None, bucket, left, left, kw.pop("gt", gt), **kw))
    bad = (dict(selected_ops=A, t=T, sampled_ops=([1] * 9, [1] * 9)), dict(selected_ops=A, t=T, task_arch=net.arch_init),
           dict(selected_ops=A, t=T, features=True), dict(selected_ops=A, t=T, supervise=False),
           dict(selected_ops=A), dict(selected_ops=A, t=T, gt=None), dict(t=T),
           dict(selected_ops=A[:-1], t=T), dict(selected_ops=A + [0], t=T),
           dict(selected_ops=[2] + A[1:], t=T), dict(selected_ops=A[:-1] + [-1], t=T),
           dict(selected_ops=A, t=2), dict(selected_ops=A, t=-1))
    for kw in bad:
        for step in steps:
            with pytest.raises(ValueError, match="selected_ops"):
                step(**dict(kw))
        if set(kw) <= {"selected_ops", "t", "gt"} and "selected_ops" in kw:
            net.eval()
            with pytest.raises(ValueError, match="selected_ops"):
                search_eval_step(net, left, left, kw.get("gt", gt), kw.get("t"), kw["selected_ops"], None)
            net.search_mode()
    with pytest.raises(ValueError, match="eval"):
        search_eval_step(net, left, left, gt, T, A, None)             # search_eval runs in eval() (rag.py:445)
    assert all(p.grad is not None and not bool(p.grad.any()) for p in bucket.params)         # nothing ran
    # other kinds of net: the depth network (its unit search is not built), a supernet, a bare MatchingNet
    depth = rag_amd.DepthNetwork(rag_amd.ALL_CONV_GENOTYPE, "cpu")
    with pytest.raises(ValueError, match="depth network's unit search is not built"):
        forward_backward(depth, GradBucket(depth.parameters()), left, None, gt, selected_ops=A, t=T)
    with pytest.raises(ValueError, match="depth network's unit search is not built"):
        search_eval_step(depth.eval(), left, None, gt, T, A, None)
    for other in (rag_amd.BasicNetwork(device="cpu", maxdisp=48), rag_amd.MatchingNet(maxdisp=48)):
        with pytest.raises(ValueError, match="selected_ops"):
            forward_backward(other, GradBucket(other.parameters()), left, left, gt, selected_ops=A, t=T)
    with pytest.raises(RuntimeError, match="MI355X"):
        rag_amd.train.masked_smooth_l1(gt, gt, 48, meter=object())


def test_meter_abi_exported_and_validated():
    from rag_amd import _lib
    lib = ctypes.CDLL(_lib.lib_path())
    assert hasattr(lib, "ragmi_stereo_metrics_meter_fwd")
    L = _lib.load_library()
    assert L.ragmi_version() >= 550

    def call(est=FAKE, gt=FAKE, B=2, H=4, W=8, acc=FAKE, out=FAKE, meter=FAKE):
        return L.ragmi_stereo_metrics_meter_fwd(est, gt, B, H, W, 48.0, acc, out, meter, None)

    for kw in (dict(est=None), dict(gt=None), dict(acc=None), dict(out=None), dict(meter=None), dict(B=0), dict(H=0), dict(W=-1),
               dict(B=65536)):
        assert call(**kw) == -1, kw                      # RAGMI_EINVAL, before any launch


def test_public_names():
    import rag_amd
    assert rag_amd.EpochMeter is rag_amd.metrics.EpochMeter and rag_amd.search_eval_step is rag_amd.train.search_eval_step
    m = rag_amd.EpochMeter("cpu")
    assert m.sums.dtype == torch.float64 and tuple(m.sums.shape) == (8,) and m.last is None
    assert set(m.mean()) == set(rag_amd.metrics.NAMES)


# --------------------------------------------------------------------------- GPU: the step against the reference
def _offsets(bucket):
    out, off = {}, 0
    for p in bucket.params:
        out[id(p)] = (off, p.numel())
        off += p.numel()
    return out


def _momentum(opt, bucket, p):
    """The momentum state of one parameter: FlatSGD's slice, torch's lazily created buffer (None while it does not exist)."""
    from rag_amd.train import FlatSGD
    if isinstance(opt, FlatSGD):
        off, n = _offsets(bucket)[id(p)]
        return opt.momentum_buffer[off:off + n].clone()
    buf = opt.state.get(p, {}).get("momentum_buffer")
    return None if buf is None else buf.detach().clone().flatten()


def _hyper():
    h = _json(g24()["hyper"])
    return {k: h[k] for k in ("lr", "momentum", "weight_decay")}, h["clip"]


def _make_opt(net, bucket, flat):
    from rag_amd.train import FlatSGD
    return FlatSGD(bucket, **_hyper()[0]) if flat else torch.optim.SGD(net.get_param(net.new_models), **_hyper()[0])


def _check_step(tag, net, before, clip, check_grads=True):
    """Every gradient (the bucket holds them clipped), moved running statistic and update of step `tag` against the fp64 step."""
    g = g24()
    named, sd = dict(net.named_parameters()), net.state_dict()
    coef = min(1.0, clip / (float(g[f"norm64_{tag}"]) + 1e-6))
    n = {"grad": 0, "delta": 0, "stat": 0}
    worst = {"grad": 0.0, "delta": 0.0, "stat": 0.0}
    fails = []
    for k in g:
        head, _, name = k.partition("::")
        if head == f"grad64_{tag}" and check_grads:
            kind, err, dist = "grad", rel_max(named[name].grad, g[k] * coef), float(g[f"gdist_{tag}::{name}"])
        elif head == f"delta64_{tag}":
            kind, err, dist = "delta", rel_max(named[name].detach() - before[name], g[k]), float(g[f"ddist_{tag}::{name}"])
        elif head == f"stat64_{tag}":
            if "num_batches" in name:
                assert int(sd[name]) == int(g[k]), k
                continue
            kind, err, dist = "stat", rel_max(sd[name], g[k]), float(g[f"sdist_{tag}::{name}"])
        else:
            continue
        tol = max(FLOOR[kind], 3.0 * dist)
        n[kind] += 1
        worst[kind] = max(worst[kind], err / tol)
        if err > tol:
            fails.append((k, err, tol))
    print(f"step {tag}: checked", n, "worst error / gate", worst)
    assert not fails, fails
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("flat", (True, False), ids=("FlatSGD", "torch_SGD"))
def test_unit_search_step_A_then_C_golden(flat):
    """train_step(selected_ops=A, t=1, meter=m) then (selected_ops=C) == the reference's two search batches (g24)."""
    from rag_amd.metrics import EpochMeter
    from rag_amd.train import FlatSGD, GradBucket, train_step
    g = g24()
    left, right, gt = gpu(g["left"]), gpu(g["right"]), gpu(g["gt"])
    A, C = _sel("A"), _sel("C")
    net = _net(DEV)
    bucket = GradBucket(net.parameters())
    assert len(bucket.params) == 207
    opt = _make_opt(net, bucket, flat)
    hyper, clip = _hyper()
    named = dict(net.named_parameters())
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    m = EpochMeter(DEV)
    seen = []
    hook = net.disp.register_forward_hook(lambda _m, _i, out: seen.append(out.detach().clone()))      # the disparity the step scored
    loss = train_step(net, opt, bucket, left, right, gt, selected_ops=A, t=T, meter=m, clip=clip)
    hook.remove()
    disp_err = float((seen[0].cpu().double() - torch.as_tensor(g["disp_A"]).double()).abs().max())
    print(f"train-mode disparity A: max |d| {disp_err:.3e} px")
    print(f"loss {loss.item():.6f} vs fp32 {float(g['loss_A']):.6f} fp64 {float(g['loss64_A']):.6f}")
    assert abs(loss.item() - float(g["loss64_A"])) <= 2e-4 * abs(float(g["loss64_A"]))
    if isinstance(opt, FlatSGD):
        tn, tn32, tn64 = opt.total_norm.item(), float(g["norm_A"]), float(g["norm64_A"])
        print(f"total norm {tn:.5f} vs fp32 {tn32:.5f} fp64 {tn64:.5f}")
        assert tn64 > clip and abs(tn - tn64) <= max(5e-4, 3.0 * abs(tn32 - tn64) / tn64) * tn64
    n = _check_step("A", net, before, clip)
    assert n == {"grad": 119, "delta": 119, "stat": 4}, n
    # the meter: this batch, fed by the loss launch
    last, sums = m.last.cpu(), m.sums.cpu()
    assert float(last[0]) == loss.item() and float(sums[6]) == 1.0 and float(sums[7]) == 2.0
    assert [float(v) for v in sums[:6]] == [float(v) for v in last[:6]]
    epe = float(g["scalars_A"][1])
    print(f"EPE {float(last[1]):.6f} vs {epe:.6f}")
    assert abs(float(last[1]) - epe) <= disp_err + 2e-5 * max(1.0, abs(epe))
    # the 403 other tensors, and the momentum of the 88 trainable ones among them
    a_keys = set(_json(g["keys_A"]))
    others = [k for k in named if k not in a_keys]
    assert len(others) == 403
    idle = 0
    for k in others:
        assert torch.equal(named[k].detach(), before[k]), k
        if named[k].requires_grad:
            idle += 1
            mom = _momentum(opt, bucket, named[k])
            assert mom is None or not bool(mom.any()), k
    assert idle == 88
    moved = sorted(k for k, v in net.state_dict().items() if not torch.equal(v, before[k]))
    assert moved == _json(g["moved_A"]) and len(moved) == 125

    # ---- the second batch, path C, same optimizer
    c_keys = set(_json(g["keys_C"]))
    a_only = sorted(a_keys - c_keys)
    assert len(a_only) == 97 and a_only == _json(g["a_only"])
    after = {k: v.detach().clone() for k, v in net.state_dict().items()}
    mom = {k: _momentum(opt, bucket, named[k]) for k in a_only}
    loss_c = train_step(net, opt, bucket, left, right, gt, selected_ops=C, t=T, meter=m, clip=clip)
    print(f"loss C {loss_c.item():.6f} vs fp64 {float(g['loss64_C']):.6f}")
    assert abs(loss_c.item() - float(g["loss64_C"])) <= 2e-4 * abs(float(g["loss64_C"]))
    moved = sorted(k for k, v in net.state_dict().items() if not torch.equal(v, after[k]))
    assert moved == _json(g["moved_C"]) and len([k for k in moved if k in named]) == 22
    for k in a_only:
        assert torch.equal(named[k].detach(), after[k]), k
        assert mom[k] is not None and bool(mom[k].any()) and torch.equal(_momentum(opt, bucket, named[k]), mom[k]), k
    n = _check_step("C", net, after, clip)
    assert n["grad"] == 22 and n["delta"] == 22, n
    assert float(m.sums[6]) == 2.0 and float(m.sums[0]) == float(loss) + float(loss_c)


@pytest.mark.gpu
def test_unit_search_step_D_runs_the_trunk_on_the_inference_executor():
    """Path D reuses every unit: only task 1's head gets gradients (7 tensors) and no unit of the trunk needs autograd, so the
    Matching-Net trunk runs on the planned inference executor (MatchingNet._run_chain rewrites last_g4_plan)."""
    from rag_amd.train import FlatSGD, GradBucket, train_step
    g = g24()
    net = _net(DEV)
    bucket = GradBucket(net.parameters())
    opt = FlatSGD(bucket, **_hyper()[0])
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.last_g4_plan = None
    loss = train_step(net, opt, bucket, gpu(g["left"]), gpu(g["right"]), gpu(g["gt"]), selected_ops=_sel("D"), t=T, clip=_hyper()[1])
    assert isinstance(net.last_g4_plan, dict) and "pre" in net.last_g4_plan
    print(f"loss D {loss.item():.6f} vs fp64 {float(g['loss64_D']):.6f}")
    assert abs(loss.item() - float(g["loss64_D"])) <= 2e-4 * abs(float(g["loss64_D"]))
    n = _check_step("D", net, before, _hyper()[1])
    assert n == {"grad": 7, "delta": 7, "stat": 4}, n
    moved = sorted(k for k, v in net.state_dict().items() if not torch.equal(v, before[k]))
    assert moved == _json(g["moved_D"])


# --------------------------------------------------------------------------- GPU: the meter
@pytest.mark.gpu
def test_epoch_meter_sums_g11_cases():
    """g11's cases a-d (ordinary images, one skipped image, all skipped, exact thresholds) through stereo_metrics(meter=) into one
    meter.  Every case is one block per image, so a call with and one without the meter add in the same order."""
    from rag_amd.metrics import NAMES, EpochMeter, stereo_metrics
    g = load_golden("g11_metrics")
    m = EpochMeter(DEV)
    assert m.last is None
    py = [0.0] * 8
    for i, tag in enumerate("abcd"):
        est, gt = gpu(g[f"{tag}::est"]), gpu(g[f"{tag}::gt"])
        plain = stereo_metrics(est, gt, 192).tensor
        got = stereo_metrics(est, gt, 192, meter=m)
        assert torch.equal(got.tensor, plain) and m.last is got.tensor, tag
        vals = plain.tolist()
        for k in range(6):
            py[k] += vals[k]                     # AverageMeterDict.update on the .item() floats
        py[6] += 1.0
        py[7] += vals[7]
        assert m.sums.tolist() == py, (tag, m.sums.tolist(), py)
    assert m.sums.dtype == torch.float64 and float(m.sums[6]) == 4.0
    mean = m.mean()
    ref = np.mean([g[f"{tag}::scalars"] for tag in "abcd"], axis=0)
    for k, name in enumerate(NAMES):
        assert abs(mean[name] - ref[k]) <= 2e-5 * max(1.0, abs(ref[k])), (name, mean[name], ref[k])
        assert mean[name] == py[k] / 4.0
    m.reset()
    assert m.last is None and m.sums.tolist() == [0.0] * 8
    # a NaN batch loss (no masked pixel: 0 / 0) propagates into the sum, as it does in the reference's float sum
    gt = torch.full((1, 4, 8), 500.0, device=DEV)
    stereo_metrics(gt, gt, 192, meter=m)
    assert np.isnan(float(m.sums[0])) and float(m.sums[6]) == 1.0


@pytest.mark.gpu
def test_search_eval_step_is_stereo_metrics_of_search_forward():
    """36x48: at most two blocks per image feed the per-image float atomics, and a + b == b + a, so two calls give the same bits
    whatever the order."""
    from rag_amd.metrics import EpochMeter, stereo_metrics
    from rag_amd.train import search_eval_step
    g = g24()
    left, right, gt = (gpu(g[k])[..., :36, :48].contiguous() for k in ("left", "right", "gt"))
    net = _net(DEV, mode="eval")
    m = EpochMeter(DEV)
    got = search_eval_step(net, left, right, gt, T, _sel("A"), m)
    with torch.no_grad():
        ref = stereo_metrics(net.search_forward(left, right, T, _sel("A")), gt, net.maxdisp).tensor
    assert m.last is got.tensor and torch.equal(m.last, ref)
    assert float(m.sums[6]) == 1.0 and np.isfinite(m.last.tolist()).all() and float(ref[6]) > 0
    assert all(p.grad is None for p in net.parameters())
    search_eval_step(net, left, right, gt, T, _sel("C"), m)
    assert float(m.sums[6]) == 2.0 and m.mean()["loss"] == float(m.sums[0]) / 2.0


# --------------------------------------------------------------------------- GPU: the captured step
@pytest.mark.gpu
def test_graphed_unit_search_step_matches_eager():
    """GraphedTrainStep(selected_ops=A, t=1, meter=m, warmup=1) at B = 2, 48x96: kernel nodes only; first_loss + two replays == three
    eager steps on a twin (driven and compared like tests/test_search_step.py::_graphed_vs_eager: a device sync before every replay,
    a clone of the loss between replays, its tolerances); the meter holds the three batches; a second object for path C over the same
    bucket and optimizer continues from A's momentum."""
    from rag_amd.metrics import EpochMeter
    from rag_amd.train import FlatSGD, GradBucket, GraphedTrainStep, train_step
    g = g24()
    left, right, gt = gpu(g["left"]), gpu(g["right"]), gpu(g["gt"])
    A, C = _sel("A"), _sel("C")
    hyper, clip = _hyper()
    finals = []
    for graphed in (False, True):
        net = _net(DEV)
        bucket = GradBucket(net.parameters())
        opt = FlatSGD(bucket, **hyper)
        m = EpochMeter(DEV)
        if graphed:
            step = GraphedTrainStep(net, opt, bucket, left, right, gt, selected_ops=A, t=T, meter=m, warmup=1, clip=clip)
            c = step.node_census
            assert c["memcpy"] == 0 and c["memset"] == 0 and c["other"] == 0 and c["kernel"] > 100, c
            held = [step.first_loss.clone()]
            for _ in range(2):
                torch.cuda.synchronize()
                held.append(step().clone())
            torch.cuda.synchronize()
            losses = [float(x) for x in held]
        else:
            losses = [float(train_step(net, opt, bucket, left, right, gt, selected_ops=A, t=T, meter=m, clip=clip)) for _ in range(3)]
        assert float(m.sums[6]) == 3.0 and float(m.sums[7]) == 6.0
        assert float(m.sums[0]) == (losses[0] + losses[1]) + losses[2], (graphed, float(m.sums[0]), losses)
        assert float(m.last[0]) == losses[2]
        finals.append((losses, {k: v.detach().clone() for k, v in net.state_dict().items()}))
        if graphed:
            named = dict(net.named_parameters())
            a_only = _json(g["a_only"])
            keep = {k: (named[k].detach().clone(), _momentum(opt, bucket, named[k])) for k in a_only}
            shared = "last_12_3d.1.conv.weight"                       # in A and in C: its momentum carries over
            assert shared in _json(g["keys_A"]) and shared in _json(g["keys_C"])
            p0, m0 = named[shared].detach().clone(), _momentum(opt, bucket, named[shared])
            m.reset()
            step_c = GraphedTrainStep(net, opt, bucket, left, right, gt, selected_ops=C, t=T, meter=m, warmup=1, clip=clip)
            c = step_c.node_census
            assert c["memcpy"] == 0 and c["memset"] == 0 and c["other"] == 0 and c["kernel"] > 100, c
            torch.cuda.synchronize()
            # SGD with momentum: buf' = momentum * buf + (g + weight_decay * p), g the clipped gradient the step leaves in the bucket;
            # three fp32 roundings per element, bound 1e-5 of the largest element
            grad = named[shared].grad.detach().flatten()
            want = hyper["momentum"] * m0 + grad + hyper["weight_decay"] * p0.flatten()
            assert bool(m0.any()) and rel_max(_momentum(opt, bucket, named[shared]), want) <= 1e-5
            lc = [float(step_c.first_loss), float(step_c().clone())]
            torch.cuda.synchronize()
            assert all(np.isfinite(lc)) and float(m.sums[6]) == 2.0 and float(m.sums[0]) == lc[0] + lc[1], lc
            for k, (pk, mk) in keep.items():
                assert torch.equal(named[k].detach(), pk), k
                assert bool(mk.any()) and torch.equal(_momentum(opt, bucket, named[k]), mk), k
    (l0, s0), (l1, s1) = finals
    print("eager", l0, "graphed", l1)
    assert l0[0] != l0[1] and l1[0] != l1[1]
    for a, b in zip(l0, l1):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (l0, l1)
    for k in s0:
        close(s1[k].float(), s0[k].float(), 5e-3, k)
