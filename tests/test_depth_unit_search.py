"""The depth tree's unit search on the HIP path (Appr.search_epoch / search_eval of rag_depth, approaches/rag.py:371-438, 492-535):
ragmi_depth_metrics_meter_fwd (loss + compute_errors + saved scalars + epoch meter in the metrics launch), DepthEpochMeter,
silog_metrics_loss, Network.search_forward_train / active_parameters, and the entry points of rag_amd.depth_search, against the
REFERENCE's own numbers: g25 (generator tests/golden/make_golden_depth_unit_search.py, three files read as one dict; the base weights
are g14's, the candidate's and the new heads' are g25's ``new::`` entries).

Gates.  Train-mode and eval depth maps: the depth forward's mean |d| <= 1e-3 m, max |d| <= 2e-2 m.  Loss: 2e-4 relative to the fp64
step.  Tensors of the training step: against the reference's fp64 step at max(floor, 3 x the reference's own fp32 distance from it,
stored per tensor), floors 5e-4 (gradients), 1e-4 (running statistics), 2e-3 (updates): DESIGN.md 4.6.1.  Metric scalars: the
project's metrics floor 1e-5 relative + 1e-6; d1-d3 as integer counts (the stored depth map is the kernel's input bit for bit and the
generator keeps every pixel 1e-5 away from a threshold).  The reference sums abs_rel and rmse over the epoch in float32: three terms
add at most 3 x 2^-24 = 1.8e-7 relative, inside the floor.  Meter sums: bit for bit the sequential Python-double sum of the floats
the kernel stored.  Kernel outputs against the older entry points: bit for bit (a NaN equals a NaN: its payload is not a value).

Unmarked tests run without a GPU; the rest need the MI355X."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

DEV = "cuda:0"
FAKE = ctypes.c_void_p(256)      # a non-NULL, 8-byte aligned pointer for argument checks that must refuse before any launch
ODD = ctypes.c_void_p(260)       # a non-NULL pointer that is not 8-byte aligned (never dereferenced either)
T = 4
FLOOR = {"grad": 5e-4, "stat": 1e-4, "delta": 2e-3}
TAGS = ("A", "C", "D")
N_KEYS = {"A": 124, "C": 25, "D": 7}


@functools.lru_cache(maxsize=None)
def g25():
    out = {}
    for name in ("g25_depth_unit_search", "g25_depth_unit_search_a_grad", "g25_depth_unit_search_a_delta"):
        out.update(load_golden(name))
    return out


def _json(a):
    return json.loads(bytes(a).decode())


def _sel(tag):
    return [int(v) for v in g25()["sel_" + tag]]


def gpu(x):
    return torch.as_tensor(np.asarray(x)).to(DEV)


def rel_max(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def same_bits(a, b) -> bool:
    a, b = np.asarray(a.detach().cpu()), np.asarray(b.detach().cpu())
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _net(device, mode="search"):
    """g14's grown model + g25's candidate and task-4 heads (expand(4, MIXED)) after the preamble of Appr.train for t > 0:
    freeze_model + modify_param(new_models, True)."""
    from rag_amd.depth import _geno, load_depth_checkpoint
    g = g25()
    sd = {k: torch.from_numpy(v) for k, v in load_golden("g14_depth_ckpt_task3").items()}
    net = load_depth_checkpoint({"model": sd}, "cpu", "from_keys")[0]
    net.expand(T, _geno(np.asarray(g["mixed"])), "cpu")
    new = {k[len("new::"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("new::")}
    assert len(new) == 486 and sum(v.numel() for v in new.values()) == 53731
    net.load_state_dict({**sd, **new}, strict=True)
    assert [len(net._units(n)) for n in net._p_layers()] == [int(v) for v in g["counts"]]
    net = net.to(device)
    for p in net.parameters():
        p.requires_grad = False
    net.modify_param(net.new_models, True)
    return net.search_mode() if mode == "search" else net.eval()


def _names(net, params):
    by_id = {id(p): k for k, p in net.named_parameters()}
    return sorted(by_id[id(p)] for p in params)


# --------------------------------------------------------------------------- CPU
def test_search_mode_leaves_the_head_lists_batchnorms_training():
    net = _net("cpu", mode="eval")
    assert net.search_mode() is net and net.training
    bns = sorted(k for k, m in net.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training)
    assert bns == _json(g25()["train_bn"])
    assert bns and all(k.startswith(("last_3_3d.", "last_6_3d.", "last_12_3d.")) for k in bns)


def test_active_parameters_are_the_reference_gradient_sets():
    g = g25()
    net = _net("cpu")
    assert len(list(net.parameters())) == int(g["n_tensors"]) == 1013
    trainable = sorted(k for k, p in net.named_parameters() if p.requires_grad)
    assert trainable == _json(g["trainable"]) and len(trainable) == 243
    for tag in TAGS:
        a = _names(net, net.active_parameters(T, g["sel_" + tag]))
        assert a == _json(g["keys_" + tag]) and len(a) == len(set(a)) == N_KEYS[tag], tag
        assert f"last_3_3d.{T}.conv.weight" in a and not any(k.startswith("depth_head") for k in a)
        assert not any(k.startswith(("last_3_2d", "last_3_3d")) and ".bn." in k for k in a)       # bn=False units
    assert net.active_parameters(0, _sel("D")) == []          # task 0's heads are frozen, and so is the depth head
    for p in net.depth_head.parameters():
        p.requires_grad = True
    a = _names(net, net.active_parameters(T, _sel("D")))
    assert a == sorted(_json(g["keys_D"]) + ["depth_head.conv1.bias", "depth_head.conv1.weight"])


def test_depth_search_refusals():
    import rag_amd
    from rag_amd.depth import DepthEpochMeter
    from rag_amd.train import GradBucket, train_step
    net = _net("cpu")
    bucket = GradBucket(net.parameters())
    left, gt = torch.zeros((1, 3, 48, 96)), torch.ones((1, 48, 96))
    A = _sel("A")
    ok = dict(net=net, gt=gt, t=T, selected_ops=A, meter=None)

    def calls(net, gt, t, selected_ops, meter):
        return (lambda: rag_amd.depth_search_step(net, None, bucket, left, gt, t, selected_ops, meter=meter),
                lambda: rag_amd.depth_search_eval_step(net, left, gt, t, selected_ops, meter),
                lambda: rag_amd.DepthGraphedSearchStep(net, None, bucket, left, gt, t, selected_ops, meter=meter))

    stereo = rag_amd.Network(rag_amd.ALL_CONV_GENOTYPE, "cpu", maxdisp=48)
    bad = (dict(net=stereo), dict(net=rag_amd.DepthBasicNetwork(device="cpu")), dict(t=None), dict(gt=None),
           dict(selected_ops=A[:-1]), dict(selected_ops=A + [0]), dict(selected_ops=None),
           dict(selected_ops=[4] + A[1:]), dict(selected_ops=A[:-1] + [-1]), dict(selected_ops=A[:5] + [5] + A[6:]),
           dict(t=5), dict(t=-1), dict(meter=object()), dict(meter=rag_amd.EpochMeter("cpu")), dict(meter=DepthEpochMeter("cpu")))
    for kw in bad:
        for call in calls(**{**ok, **kw}):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError, match="eval"):
        rag_amd.depth_search_eval_step(net, left, gt, T, A)           # search_eval runs in eval() (rag.py:498)
    assert all(p.grad is not None and not bool(p.grad.any()) for p in bucket.params)         # nothing ran
    # the generic entry points keep refusing a depth network, and name these
    with pytest.raises(ValueError, match="depth network's unit search is not built into this entry point: use rag_amd.depth_search_step"):
        train_step(net, None, bucket, left, None, gt, selected_ops=A, t=T)
    # depth_metrics: a wrong meter type or device
    for meter in (object(), rag_amd.EpochMeter("cpu")):
        with pytest.raises(ValueError, match="DepthEpochMeter"):
            rag_amd.depth_metrics(gt, gt, meter=meter)
    with pytest.raises(RuntimeError, match="MI355X"):
        rag_amd.depth_metrics(gt, gt, meter=DepthEpochMeter("cpu"))
    with pytest.raises(RuntimeError, match="MI355X"):
        rag_amd.silog_metrics_loss(gt, gt, DepthEpochMeter("cpu"))


def test_meter_abi_exported_and_validated():
    from rag_amd import _lib
    lib = ctypes.CDLL(_lib.lib_path())
    assert hasattr(lib, "ragmi_depth_metrics_meter_fwd")
    L = _lib.load_library()
    assert L.ragmi_version() >= 560

    def call(est=FAKE, gt=FAKE, n=100, ws=FAKE, out=FAKE, saved=FAKE, meter=FAKE, dtype=0):
        return L.ragmi_depth_metrics_meter_fwd(est, gt, n, 0.85, ws, out, saved, meter, dtype, None)

    for kw in (dict(est=None), dict(gt=None), dict(ws=None), dict(out=None), dict(n=0), dict(n=-3), dict(ws=ODD), dict(saved=ODD),
               dict(meter=ODD), dict(saved=None, meter=ODD), dict(saved=ODD, meter=None)):
        assert call(**kw) == -1, kw                      # RAGMI_EINVAL, before any launch
    assert call(dtype=1) < 0                             # bf16 is not built


def test_public_names_and_cpu_loss():
    import rag_amd
    from rag_amd.depth import DEPTH_NAMES, silog_loss_torch
    assert rag_amd.DepthEpochMeter is rag_amd.depth.DepthEpochMeter
    assert rag_amd.depth_search_step is rag_amd.depth_search.depth_search_step
    assert rag_amd.depth_search_eval_step is rag_amd.depth_search.depth_search_eval_step
    assert rag_amd.DepthGraphedSearchStep is rag_amd.depth_search.DepthGraphedSearchStep
    assert issubclass(rag_amd.DepthGraphedSearchStep, rag_amd.train._GraphedStep)
    assert issubclass(rag_amd.train.GraphedTrainStep, rag_amd.train._GraphedStep)
    m = rag_amd.DepthEpochMeter("cpu")
    assert m.sums.dtype == torch.float64 and tuple(m.sums.shape) == (12,) and m.last is None
    mean = m.mean()
    assert tuple(mean) == DEPTH_NAMES and all(np.isnan(v) for v in mean.values())
    g = g25()
    est, gt = torch.from_numpy(g["est_A"]).requires_grad_(True), torch.from_numpy(g["gt"])
    loss = rag_amd.silog_metrics_loss(est, gt)
    ref = silog_loss_torch(est, gt)
    assert loss.dim() == 0 and torch.equal(loss, ref)
    assert abs(loss.item() - float(g["loss_A"])) <= 1e-5 * float(g["loss_A"])
    loss.backward()
    assert est.grad is not None and not bool(est.grad[gt <= 0].any())


# --------------------------------------------------------------------------- GPU: the kernel
def _raw_meter(est, gt, saved=None, meter=None, vf=0.85):
    """ragmi_depth_metrics_meter_fwd itself (null pointers included) -> out10"""
    from rag_amd import ops
    from rag_amd._lib import check, load_library
    L = load_library()
    n = est.numel()
    ws = torch.empty((max(2, L.ragmi_depth_metrics_workspace_elems(n)),), device=est.device, dtype=torch.float32)
    out = torch.empty((10,), device=est.device, dtype=torch.float32)
    check(L.ragmi_depth_metrics_meter_fwd(est.data_ptr(), gt.data_ptr(), n, vf, ws.data_ptr(), out.data_ptr(),
                                          saved.data_ptr() if saved is not None else None,
                                          meter.data_ptr() if meter is not None else None, 0, ops._stream()), "depth_metrics_meter")
    return out


def _patterns(n, seed):
    """(name, est, gt, valid pixels) - all valid, 60 % holes, one valid pixel at the very end (the grid-stride tail), none valid."""
    rng = np.random.default_rng(seed)
    est = (rng.random(n, dtype=np.float32) * 70 + 1)
    full = (est * np.exp(rng.standard_normal(n).astype(np.float32) * 0.2)).astype(np.float32)
    holes = full.copy()
    holes[rng.random(n) < 0.6] = 0
    holes[-1] = full[-1]                                  # at least one valid pixel at every n
    tail = np.zeros_like(full)
    tail[-1] = full[-1]
    none = np.zeros_like(full)
    none[::3] = -1.0                                      # gt <= 0 is invalid, negative included
    return [(name, gpu(est), gpu(gt), int((gt > 0).sum())) for name, gt in (("all", full), ("holes", holes), ("tail", tail), ("none", none))]


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 255, 257, 1025, 1048577, 2500001))
def test_meter_kernel_matches_the_older_entry_points_bit_for_bit(n):
    """n = 1 048 577 is one past 1024 x 4 x 256, so the grid-stride loop wraps; 2 500 001 wraps more than twice."""
    from rag_amd import ops
    sums = torch.zeros((12,), device=DEV, dtype=torch.float64)
    py, pixels, batches = [0.0] * 10, 0, 0
    for name, est, gt, valid in _patterns(n, n):
        plain = ops.depth_metrics(est, gt)
        assert same_bits(_raw_meter(est, gt), plain), (n, name)                 # null saved, null meter
        loss, saved_ref = ops.silog_loss(est, gt)
        saved = torch.full((3,), -7.0, device=DEV, dtype=torch.float64)
        out = _raw_meter(est, gt, saved=saved)                                  # saved only
        assert same_bits(out, plain) and same_bits(out[:1], loss) and same_bits(saved, saved_ref), (n, name)
        assert float(saved[0]) == valid
        if name == "none":
            assert np.isnan(float(out[0])) and np.isnan(float(saved[2]))
            continue                                     # a NaN batch is summed in its own test below
        before = sums.clone()
        out = _raw_meter(est, gt, meter=sums)                                   # meter only
        assert same_bits(out, plain), (n, name)
        vals = out.tolist()
        for k in range(10):
            py[k] += vals[k]
        pixels, batches = pixels + valid, batches + 1
        # (one valid pixel: compute_errors' silog is the root of a rounding residue, NaN when that is negative, here as in numpy)
        assert np.array_equal(sums.cpu().numpy(), np.array(py + [float(batches), float(pixels)]), equal_nan=True), (n, name, before.tolist())
    assert batches == 3 and float(sums[10]) == 3.0 and float(sums[11]) == pixels and np.isfinite(float(sums[0]))
    out = _raw_meter(est, gt, saved=saved, meter=sums)                          # the "none" batch, both pointers
    assert np.isnan(float(sums[0])) and float(sums[10]) == 4.0 and float(sums[11]) == pixels and same_bits(out, plain)


@pytest.mark.gpu
def test_silog_metrics_loss_is_silog_loss_with_a_meter():
    from rag_amd.depth import DepthEpochMeter, depth_metrics, silog_loss, silog_metrics_loss
    (_n, est, gt, valid), = [p for p in _patterns(48 * 96 * 2 + 1, 5) if p[0] == "holes"]
    m = DepthEpochMeter(DEV)
    e0, e1 = est.clone().requires_grad_(True), est.clone().requires_grad_(True)
    l0, l1 = silog_loss(e0, gt), silog_metrics_loss(e1, gt, m)
    assert l1.dim() == 0 and same_bits(l0, l1) and float(m.last[0]) == l1.item()
    (l0 * 0.37).backward()
    (l1 * 0.37).backward()
    assert bool(e0.grad.any()) and same_bits(e0.grad, e1.grad)
    got = depth_metrics(est, gt, meter=m)
    assert m.last is got.tensor and same_bits(got.tensor, depth_metrics(est, gt).tensor)
    assert float(m.sums[10]) == 2.0 and float(m.sums[11]) == 2 * valid and float(m.sums[0]) == l1.item() + l1.item()
    assert m.mean()["silog_loss"] == float(m.sums[0]) / 2.0
    # no valid pixel: a NaN loss into the meter (numpy's mean of an empty selection in the reference), an all-zero gradient
    e2 = est.clone().requires_grad_(True)
    l2 = silog_metrics_loss(e2, torch.zeros_like(gt), m)
    l2.backward()
    assert np.isnan(l2.item()) and np.isnan(float(m.sums[0])) and float(m.sums[10]) == 3.0 and not bool(e2.grad.any())
    m.reset()
    assert m.last is None and m.sums.tolist() == [0.0] * 12
    with pytest.raises(ValueError, match="DepthEpochMeter"):
        silog_metrics_loss(est, gt, object())


@pytest.mark.gpu
def test_meter_against_the_reference_loop():
    """The reference's stored train-mode depth maps of A, C, D through the meter: each batch's ten floats and the epoch's averages
    against rag.py:416-436 (compute_errors on the host gather, float32 sums of abs_rel and rmse)."""
    from rag_amd.depth import DEPTH_NAMES, DepthEpochMeter, depth_metrics
    g = g25()
    gt = gpu(g["gt"])
    n = int((g["gt"] > 0).sum())
    m = DepthEpochMeter(DEV)
    for i, tag in enumerate(TAGS):
        got = depth_metrics(gpu(g["est_" + tag]), gt, meter=m).tensor.tolist()
        ref = [float(v) for v in g["scalars_" + tag]]
        print(tag, "worst |got - ref| / gate", max(abs(a - b) / (1e-5 * abs(b) + 1e-6) for a, b in zip(got, ref)))
        for k, name in enumerate(DEPTH_NAMES):
            assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]) + 1e-6, (tag, name, got[k], ref[k])
        for k in (7, 8, 9):
            assert round(got[k] * n) == round(ref[k] * n), (tag, DEPTH_NAMES[k])
        assert float(m.sums[10]) == i + 1 and float(m.sums[11]) == n * (i + 1)
    mean, ref = m.mean(), [float(v) for v in g["epoch_avg"]]
    for k, name in enumerate(DEPTH_NAMES):
        assert abs(mean[name] - ref[k]) <= 1e-5 * abs(ref[k]) + 1e-6, (name, mean[name], ref[k])


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


def _same_momentum(a, b) -> bool:
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def _hyper():
    h = _json(g25()["hyper"])
    return {k: h[k] for k in ("lr", "momentum", "weight_decay")}, h["clip"]


def _check_depth(got, ref, what):
    d = (got.detach().cpu().double() - torch.as_tensor(ref).double()).abs()
    print(f"{what}: mean |d| {float(d.mean()):.3e} m (gate 1e-3), max |d| {float(d.max()):.3e} m (gate 2e-2)")
    assert float(d.mean()) <= 1e-3 and float(d.max()) <= 2e-2, (what, float(d.mean()), float(d.max()))


def _check_step(tag, net, before, clip):
    """Every gradient (the bucket holds them clipped), moved running statistic and update of step `tag` against the fp64 step."""
    g = g25()
    named, sd = dict(net.named_parameters()), net.state_dict()
    coef = min(1.0, clip / (float(g[f"norm64_{tag}"]) + 1e-6))
    n = {"grad": 0, "delta": 0, "stat": 0}
    worst = {"grad": 0.0, "delta": 0.0, "stat": 0.0}
    fails = []
    for k in g:
        head, _, name = k.partition("::")
        if head == f"grad64_{tag}":
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
def test_depth_search_step_A_C_D_golden(flat, monkeypatch):
    """depth_search_step on paths A, C, D, one model, one optimizer, one meter == the reference's three search batches (g25)."""
    import rag_amd
    from rag_amd.train import FlatSGD, GradBucket
    g = g25()
    left, gt = gpu(g["left"]), gpu(g["gt"])
    net = _net(DEV)
    bucket = GradBucket(net.parameters())
    assert len(bucket.params) == 243
    hyper, clip = _hyper()
    opt = FlatSGD(bucket, **hyper) if flat else torch.optim.SGD(net.get_param(net.new_models), **hyper)
    named = dict(net.named_parameters())
    m = rag_amd.DepthEpochMeter(DEV)
    seen = []
    fused = rag_amd.depth.silog_metrics_loss
    monkeypatch.setattr(rag_amd.depth, "silog_metrics_loss", lambda est, *a, **kw: (seen.append(est.detach().clone()), fused(est, *a, **kw))[1])
    a_only, a_state, losses = _json(g["a_only"]), None, []
    assert a_only == sorted(set(_json(g["keys_A"])) - set(_json(g["keys_C"])) - set(_json(g["keys_D"])))
    for i, tag in enumerate(TAGS):
        keys = set(_json(g["keys_" + tag]))
        before = {k: v.detach().clone() for k, v in net.state_dict().items()}
        mom = {k: _momentum(opt, bucket, p) for k, p in named.items() if p.requires_grad and k not in keys}
        loss = rag_amd.depth_search_step(net, opt, bucket, left, gt, T, _sel(tag), meter=m, clip=clip)
        _check_depth(seen[i], g["est_" + tag], f"train-mode depth {tag}")
        l64 = float(g[f"loss64_{tag}"])
        print(f"loss {tag} {loss.item():.6f} vs fp32 {float(g['loss_' + tag]):.6f} fp64 {l64:.6f}: "
              f"{abs(loss.item() - l64) / (2e-4 * l64):.3f} of the gate")
        assert abs(loss.item() - l64) <= 2e-4 * abs(l64)
        assert float(m.last[0]) == loss.item() and float(m.sums[10]) == i + 1
        if isinstance(opt, FlatSGD):
            tn, tn32, tn64 = opt.total_norm.item(), float(g["norm_" + tag]), float(g["norm64_" + tag])
            print(f"total norm {tn:.5f} vs fp32 {tn32:.5f} fp64 {tn64:.5f}")
            assert tn64 > clip and abs(tn - tn64) <= max(5e-4, 3.0 * abs(tn32 - tn64) / tn64) * tn64
        n = _check_step(tag, net, before, clip)
        assert n["grad"] == n["delta"] == N_KEYS[tag] and n["stat"] > 0, n
        moved = sorted(k for k, v in net.state_dict().items() if not torch.equal(v, before[k]))
        assert moved == _json(g["moved_" + tag])
        # every tensor outside the path's set, and its momentum, across the step
        for k, p in named.items():
            if k not in keys:
                assert torch.equal(p.detach(), before[k]), (tag, k)
                if p.requires_grad:
                    assert _same_momentum(_momentum(opt, bucket, p), mom[k]), (tag, k)
        if tag == "A":
            a_state = {k: (named[k].detach().clone(), _momentum(opt, bucket, named[k])) for k in a_only}
            assert all(mk is not None and bool(mk.any()) for _pk, mk in a_state.values())
        losses.append(loss.item())
    for k, (pk, mk) in a_state.items():                  # what only A trained is what A left, after C and D
        assert torch.equal(named[k].detach(), pk) and torch.equal(_momentum(opt, bucket, named[k]), mk), k
    assert float(m.sums[0]) == (losses[0] + losses[1]) + losses[2] and float(m.sums[11]) == 3 * int((g["gt"] > 0).sum())


def _graph_leaves(out):
    """(parameters an autograd graph reaches, its number of nodes)"""
    seen, stack, leaves = set(), [out.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if hasattr(fn, "variable"):
            leaves.append(fn.variable)
        stack += [f for f, _ in fn.next_functions]
    return leaves, len(seen)


@pytest.mark.gpu
def test_all_reused_path_builds_no_trunk_graph():
    """Path D reuses every unit: the graph of search_forward_train holds the head of task 4 only (last_12_3d, last_6_3d with their
    BatchNorms, last_3_3d's weight, the fused depth head), where path A's reaches its 124 tensors through the trunk."""
    g = g25()
    net = _net(DEV)
    left = gpu(g["left"])
    est = net.search_forward_train(left, T, _sel("D"))
    leaves, nodes = _graph_leaves(est)
    assert _names(net, leaves) == _json(g["keys_D"]) and len(leaves) == 7
    est_a = net.search_forward_train(left, T, _sel("A"))
    leaves_a, nodes_a = _graph_leaves(est_a)
    assert _names(net, leaves_a) == _json(g["keys_A"]) and nodes_a > 10 * nodes
    with pytest.raises(RuntimeError, match="inference only"):
        net.search_forward(left, None, T, _sel("D"))     # search_forward itself stays inference only


@pytest.mark.gpu
def test_depth_search_eval_step_golden():
    import rag_amd
    g = g25()
    left, gt = gpu(g["left"]), gpu(g["gt"])
    net = _net(DEV, mode="eval")
    m = rag_amd.DepthEpochMeter(DEV)
    for i, tag in enumerate(("A", "D")):
        got = rag_amd.depth_search_eval_step(net, left, gt, T, _sel(tag), m)
        with torch.no_grad():
            est = net.search_forward(left, None, T, _sel(tag))
        _check_depth(est, g["eval_est_" + tag], f"eval depth {tag}")
        assert m.last is got.tensor and same_bits(got.tensor, rag_amd.depth_metrics(est, gt).tensor) and float(m.sums[10]) == i + 1
    # D's map has no saturated pixel: its scalars are finite and the reference's
    ref = [float(v) for v in g["eval_scalars_D"]]
    assert np.isfinite(ref).all()
    print("eval D", got.tensor.tolist(), "reference", ref)
    assert abs(float(got["abs_rel"]) - ref[2]) <= 2e-2 / 2.0 + 1e-5 * ref[2]          # |d est| <= 2e-2 m over gt >= 2 m
    assert all(p.grad is None for p in net.parameters())


# --------------------------------------------------------------------------- GPU: the captured step
@pytest.mark.gpu
def test_graphed_depth_search_step_matches_eager():
    """DepthGraphedSearchStep(path A, warmup=1) at B = 2, 48x96: kernel nodes only; first_loss + two replays == three eager steps on a
    twin to 1e-6 relative (a device sync before every replay, a clone of the loss between replays); the meter holds the three."""
    import rag_amd
    from rag_amd.train import FlatSGD, GradBucket
    g = g25()
    left, gt = gpu(g["left"]), gpu(g["gt"])
    A = _sel("A")
    hyper, clip = _hyper()
    runs = []
    for graphed in (False, True):
        net = _net(DEV)
        bucket = GradBucket(net.parameters())
        opt = FlatSGD(bucket, **hyper)
        m = rag_amd.DepthEpochMeter(DEV)
        if graphed:
            step = rag_amd.DepthGraphedSearchStep(net, opt, bucket, left, gt, T, A, meter=m, clip=clip, warmup=1)
            c = step.node_census
            assert c["memcpy"] == 0 and c["memset"] == 0 and c["other"] == 0 and c["kernel"] > 100, c
            held = [step.first_loss.clone()]
            for _ in range(2):
                torch.cuda.synchronize()
                held.append(step().clone())
            torch.cuda.synchronize()
            losses = [float(x) for x in held]
        else:
            losses = [float(rag_amd.depth_search_step(net, opt, bucket, left, gt, T, A, meter=m, clip=clip)) for _ in range(3)]
        assert float(m.sums[10]) == 3.0 and float(m.sums[11]) == 3 * int((g["gt"] > 0).sum())
        assert float(m.sums[0]) == (losses[0] + losses[1]) + losses[2], (graphed, float(m.sums[0]), losses)
        assert float(m.last[0]) == losses[2]
        runs.append(losses)
    print("eager", runs[0], "graphed", runs[1])
    assert runs[0][0] != runs[0][1] and abs(runs[0][0] - float(g["loss64_A"])) <= 2e-4 * float(g["loss64_A"])
    for a, b in zip(*runs):
        assert abs(a - b) <= 1e-6 * abs(a), runs
