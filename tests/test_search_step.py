"""The cell search on the HIP path: the depth supernet (rag_amd.DepthBasicNetwork), the sampled-op training step of rag_amd.train
(`sampled_ops=(fea_ops, mat_ops)`) on both supernets, and the masked clip + SGD launch behind it (ragmi_sgd_clip_step_masked),
against the REFERENCE's own numbers: g23 (rag_depth/src/automl/mdenas_basicmodel.py; generator
tests/golden/make_golden_depth_supernet.py, three files read as one dict) and g9 (the stereo supernet).

Gates.  Depth maps: the depth network's own, mean |d| <= 1e-3 m and max |d| <= 2e-2 m.  Tensors of the training step:
against the reference's fp64 step at max(floor, 3 x the reference's own fp32 distance from it), floors 5e-4 (gradients), 1e-4
(running statistics), 2e-3 (updates): the rule and the floors of g20.  The masked launch alone: 1e-6 relative on
active elements (what FlatSGD's launch is held to in test_hip_train.py), bitwise on inactive ones.

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
DRAW_A = ([1, 0, 1, 1, 0, 1, 0, 1, 1], [0, 1, 1, 0, 1, 1, 1, 0, 1])
DRAW_B = ([0, 1, 1, 1, 0, 0, 1, 1, 0], [1, 1, 0, 1, 0, 1, 0, 1, 1])
ALL_CONV = ([1] * 9, [1] * 9)
HYPER = dict(lr=0.002, momentum=0.9, weight_decay=3e-4)          # run_rag_depth.sh


@functools.lru_cache(maxsize=None)
def g23():
    out = {}
    for name in ("g23_depth_supernet", "g23_depth_supernet_step_a", "g23_depth_supernet_step_b"):
        out.update(load_golden(name))
    return out


def _json(a):
    return json.loads(bytes(a).decode())


def gpu(x):
    return torch.as_tensor(np.asarray(x)).to(DEV)


def rel_max(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def fp32_tol(ref32, ref64, floor):
    """`floor`, or 3x the reference's OWN fp32 distance from its fp64 run where that is larger (train-mode BatchNorm over B=2
    amplifies fp32 rounding)."""
    return max(floor, 3.0 * rel_max(ref32, ref64))


def close(got, ref, tol, what=""):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float((got - ref).abs().max())
    bound = tol * max(1.0, float(ref.abs().max()))
    assert err <= bound, (what, err, bound)


def _names(net, params):
    by_id = {id(p): k for k, p in net.named_parameters()}
    return sorted(by_id[id(p)] for p in params)


def _depth_net(device):
    import rag_amd
    net = rag_amd.DepthBasicNetwork(device=device)
    net.load_state_dict(split_sd(g23()), strict=True)
    return net.to(device)


def _stereo_net(device):
    import rag_amd
    g = load_golden("g9_supernet")
    net = rag_amd.BasicNetwork(device=device, maxdisp=int(g["maxdisp"]))
    net.load_state_dict(split_sd(g), strict=True)
    return net.to(device), g


# --------------------------------------------------------------------------- CPU
def test_depth_supernet_keys_shapes_and_strict_load():
    import rag_amd
    assert rag_amd.depth.BasicNetwork is rag_amd.DepthBasicNetwork
    net = rag_amd.DepthBasicNetwork(device="cpu")
    ref = split_sd(g23())
    sd = net.state_dict()
    assert set(sd) == set(ref) and len(ref) == 914
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert len(list(net.parameters())) == int(g23()["n_params"]) == 458
    net.load_state_dict(ref, strict=True)
    assert isinstance(net.matching, rag_amd.DepthAutoMatching) and net.maxdisp == 192 and net.max_depth == 80
    twin = net.new()
    assert type(twin) is type(net) and twin.p is not net.p and torch.equal(twin.p["normal"], net.p["normal"])


def test_depth_supernet_genotype_matches_reference():
    g = g23()
    net = _depth_net("cpu")
    net.p = {"normal": torch.as_tensor(g["p_normal"]), "reduce": torch.as_tensor(g["p_reduce"])}
    geno = net.genotype()
    assert np.array_equal(np.asarray(geno.normal), g["geno_normal"])
    assert np.array_equal(np.asarray(geno.reduce), g["geno_reduce"])


def test_depth_active_parameters_are_the_reference_gradient_sets():
    g = g23()
    net = _depth_net("cpu")
    a = _names(net, net.active_parameters(*DRAW_A))
    assert a == sorted(_json(g["active_keys"])) and len(a) == 289 and len(set(a)) == 289
    assert _names(net, net.active_parameters(*DRAW_B)) == sorted(_json(g["active_keys_B"]))
    assert sorted(set(dict(net.named_parameters())) - set(a)) == sorted(_json(g["unmoved"]))
    assert not any("last_24" in k or k.endswith("last_3.bn.weight") for k in a)


def test_stereo_active_parameters_match_g9():
    net, g = _stereo_net("cpu")
    a = _names(net, net.active_parameters(g["fea_ops"], g["mat_ops"]))
    assert len(a) == len(set(a)) == int(g["n_params_with_grad"])
    for k in g:
        if k.startswith("grad::"):
            assert k[6:] in a, k


def test_masked_sgd_abi_exported_and_validated():
    from rag_amd import _lib
    lib = ctypes.CDLL(_lib.lib_path())
    assert hasattr(lib, "ragmi_sgd_clip_step_masked")
    L = _lib.load_library()
    assert L.ragmi_version() >= 540

    def call(p=FAKE, g=FAKE, b=FAKE, act=FAKE, n=10, lr=0.1, mom=0.9, wd=0.0, ws=FAKE):
        return L.ragmi_sgd_clip_step_masked(p, g, b, act, n, lr, mom, wd, 5.0, ws, None, None)

    for kw in (dict(p=None), dict(g=None), dict(b=None), dict(act=None), dict(ws=None), dict(n=0), dict(lr=-1.0), dict(mom=-0.1),
               dict(wd=-1e-3)):
        assert call(**kw) == -1, kw                      # RAGMI_EINVAL, before any launch


def test_sampled_step_refusals():
    import rag_amd
    from rag_amd.modules import ALL_CONV_GENOTYPE
    from rag_amd.train import GradBucket, GraphedTrainStep, forward_backward, train_step
    left, gt = torch.zeros((1, 3, 48, 96)), torch.ones((1, 48, 96))
    for net in (rag_amd.DepthBasicNetwork(device="cpu"), rag_amd.BasicNetwork(device="cpu", maxdisp=48)):
        bucket = GradBucket(net.parameters())
        with pytest.raises(ValueError, match="sampled_ops"):
            forward_backward(net, bucket, left, left, gt)
        for kw in (dict(task_arch={"x": [0]}), dict(features=True), dict(supervise=False)):
            with pytest.raises(ValueError, match="sampled_ops"):
                forward_backward(net, bucket, left, left, gt, sampled_ops=DRAW_A, **kw)
            with pytest.raises(ValueError, match="sampled_ops"):
                train_step(net, None, bucket, left, left, gt, sampled_ops=DRAW_A, **kw)
            with pytest.raises(ValueError, match="sampled_ops"):
                GraphedTrainStep(net, None, bucket, left, left, gt, sampled_ops=DRAW_A, **kw)
    grown = rag_amd.Network(ALL_CONV_GENOTYPE, "cpu", maxdisp=48)
    with pytest.raises(ValueError, match="supernet|BasicNetwork"):
        forward_backward(grown, GradBucket(grown.parameters()), left, left, gt, sampled_ops=DRAW_A)
    with pytest.raises(RuntimeError, match="fp32 only"):
        rag_amd.DepthBasicNetwork(device="cpu")(left.half(), None, *DRAW_A)


def test_depth_matching_refuses_another_last_level_size(monkeypatch):
    """The last cell is at 1/4 of the feature map; anything else is a ValueError (the check alone: the cells are stubbed)."""
    import rag_amd
    m = rag_amd.DepthAutoMatching()
    monkeypatch.setattr(m, "_cells", lambda x, n_alphas: torch.zeros((1, 48, 1, 5, 8)))
    with pytest.raises(ValueError, match="multiples of 12"):
        m(torch.zeros((1, 12, 24, 32)), ALL_CONV[1])


# --------------------------------------------------------------------------- GPU: eval forward
def _depth_gate(got, ref, what):
    d = (got.detach().cpu().double() - torch.as_tensor(ref).double()).abs()
    mean, mx = float(d.mean()), float(d.max())
    print(f"{what}: mean |d| {mean:.3e} m, max |d| {mx:.3e} m")
    assert got.shape == tuple(ref.shape) and mean <= 1e-3 and mx <= 2e-2, (what, mean, mx)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", (None, "fp32"))
@pytest.mark.parametrize("tag,draw", (("A", DRAW_A), ("conv", ALL_CONV)))
@pytest.mark.parametrize("i", (0, 1))
def test_depth_supernet_eval_forward_golden(i, tag, draw, precision):
    """B=2 48x96 and B=1 60x84 (feature 20x28: the up-path resizes 5x7 to 9x13), draw A and all-conv, under the default conv
    precision and under fp32."""
    from rag_amd import ops
    g = g23()
    net = _depth_net(DEV).eval()
    old = ops.set_conv_precision(precision) if precision else None
    try:
        with torch.no_grad():
            out = net(gpu(g[f"img{i}"]), None, *draw)
    finally:
        if old is not None:
            ops.set_conv_precision(old)
    _depth_gate(out, g[f"eval{i}_{tag}"], f"eval{i}_{tag} {precision}")


# --------------------------------------------------------------------------- GPU: the depth search step
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


def _make_opt(net, bucket, flat):
    from rag_amd.train import FlatSGD
    return FlatSGD(bucket, **HYPER) if flat else torch.optim.SGD(net.parameters(), **HYPER)


@pytest.mark.gpu
@pytest.mark.parametrize("flat", (True, False), ids=("FlatSGD", "torch_SGD"))
def test_depth_search_step_golden(flat):
    """train_step(sampled_ops=A) then (sampled_ops=B) on the depth supernet == the reference's two search steps (g23): the train-mode
    depth map, the loss, and every stored gradient, running statistic and update against the fp64 step; a parameter that was not
    sampled, and its momentum, are bit for bit what they were."""
    from rag_amd import ops
    from rag_amd.train import FlatSGD, GradBucket, train_step
    g = g23()
    left, gt = gpu(g["left"]), gpu(g["gt"])
    twin = _depth_net(DEV).train()
    with torch.no_grad(), ops.conv_precision("fp32"):
        _depth_gate(twin(left, None, *DRAW_A), g["depth_train"], "depth_train")

    net = _depth_net(DEV).train()
    bucket = GradBucket(net.parameters())
    opt = _make_opt(net, bucket, flat)
    named = dict(net.named_parameters())
    sd0 = split_sd(g)
    before = {k: v.detach().clone() for k, v in named.items()}
    loss = train_step(net, opt, bucket, left, None, gt, sampled_ops=DRAW_A)
    print(f"loss {loss.item():.6f} vs {float(g['loss']):.6f}")
    assert abs(loss.item() - float(g["loss"])) <= 2e-4 * abs(float(g["loss"]))
    coef = min(1.0, 5.0 / (float(g["total_norm64"]) + 1e-6))             # the bucket holds the clipped gradients after the step
    if isinstance(opt, FlatSGD):
        tn, tn32, tn64 = opt.total_norm.item(), float(g["total_norm"]), float(g["total_norm64"])
        print(f"total norm {tn:.5f} vs fp32 {tn32:.5f} fp64 {tn64:.5f}")
        assert abs(tn - tn64) <= max(5e-4, 3.0 * abs(tn32 - tn64) / tn64) * tn64
    n = {"grad": 0, "delta": 0, "stat": 0}
    worst = {"grad": 0.0, "delta": 0.0, "stat": 0.0}
    fails = []
    for k in g:
        if k.startswith("grad64::"):
            name, kind = k[8:], "grad"
            err = rel_max(named[name].grad, g[k] * coef)
            tol = fp32_tol(g["grad::" + name], g[k], 5e-4)
        elif k.startswith("delta64::"):
            name, kind = k[9:], "delta"
            err = rel_max(named[name].detach() - before[name], g[k])
            tol = fp32_tol(torch.as_tensor(g["after::" + name]) - sd0[name], g[k], 2e-3)
        elif k.startswith("after64::") and "num_batches" not in k:
            name, kind = k[9:], "stat"
            err = rel_max(net.state_dict()[name], g[k])
            tol = fp32_tol(g["after::" + name], g[k], 1e-4)
        else:
            if k.startswith("after64::"):
                assert int(net.state_dict()[k[9:]]) == int(g[k]), k
            continue
        n[kind] += 1
        worst[kind] = max(worst[kind], err / tol)
        if err > tol:
            fails.append((k, err, tol))
    print("step A: checked", n, "worst error / gate", worst)
    assert not fails, fails
    assert n["grad"] > 80 and n["delta"] > 80 and n["stat"] > 40, n
    unmoved = _json(g["unmoved"])
    assert len(unmoved) == 458 - 289
    for name in unmoved:
        assert torch.equal(named[name].detach(), before[name]), name
        m = _momentum(opt, bucket, named[name])
        assert m is None or not bool(m.any()), name

    # ---- the second step, draw B, same optimizer
    a_keys, b_keys = set(_json(g["active_keys"])), set(_json(g["active_keys_B"]))
    a_only = sorted(a_keys - b_keys)
    assert len(a_only) > 20
    after = {k: v.detach().clone() for k, v in named.items()}
    mom = {k: _momentum(opt, bucket, named[k]) for k in a_only}
    train_step(net, opt, bucket, left, None, gt, sampled_ops=DRAW_B)
    for name in a_only + sorted(set(named) - a_keys - b_keys):
        assert torch.equal(named[name].detach(), after[name]), name
    for name in a_only:
        assert mom[name] is not None and bool(mom[name].any()), name
        assert torch.equal(_momentum(opt, bucket, named[name]), mom[name]), name
    fails, nb, worst_b = [], 0, 0.0
    for k in g:
        if k.startswith("delta2_64::"):
            name = k[11:]
            ref_after = torch.as_tensor(g["after::" + name]) if ("after::" + name) in g else sd0[name]
            err = rel_max(named[name].detach() - after[name], g[k])
            tol = fp32_tol(torch.as_tensor(g["after2::" + name]) - ref_after, g[k], 2e-3)
            nb += 1
            worst_b = max(worst_b, err / tol)
            if err > tol:
                fails.append((k, err, tol))
    print("step B: checked", nb, "worst error / gate", worst_b)
    assert not fails, fails
    assert nb > 80


# --------------------------------------------------------------------------- GPU: the stereo search step
@pytest.mark.gpu
def test_stereo_search_step_golden():
    """train_step(sup, ..., sampled_ops=(fea_ops, mat_ops)) on g9: the bucket's gradients are the reference's (the step leaves them
    clipped: compared after undoing the coefficient), parameters that were not sampled stay bit for bit."""
    from rag_amd.train import FlatSGD, GradBucket, train_step
    net, g = _stereo_net(DEV)
    net.train()
    bucket = GradBucket(net.parameters())
    opt = FlatSGD(bucket, lr=1e-3, momentum=0.9, weight_decay=3e-3)
    named = dict(net.named_parameters())
    before = {k: v.detach().clone() for k, v in named.items()}
    draw = (g["fea_ops"], g["mat_ops"])
    loss = train_step(net, opt, bucket, gpu(g["left"]), gpu(g["right"]), gpu(g["gt"]), sampled_ops=draw)
    assert abs(loss.item() - float(g["loss"])) < 2e-4 * max(1.0, float(g["loss"]))
    coef = min(1.0, 5.0 / (opt.total_norm.item() + 1e-6))
    n = 0
    for k, ref in g.items():
        if k.startswith("grad::"):
            close(named[k[6:]].grad / coef, ref, 1e-3, k)
            n += 1
    assert n > 80
    active = {id(p) for p in net.active_parameters(*draw)}
    idle = [k for k, p in named.items() if id(p) not in active]
    assert len(idle) == int(g["n_params"]) - int(g["n_params_with_grad"])
    for k in idle:
        assert torch.equal(named[k].detach(), before[k]), k
        assert not bool(_momentum(opt, bucket, named[k]).any()), k


# --------------------------------------------------------------------------- GPU: the masked launch alone
def _segments(n, seed):
    r = np.random.RandomState(seed)
    cuts, at = [], 0
    while at < n:
        at = min(n, at + int(r.randint(1, 701)))
        cuts.append(at)
    return list(zip([0] + cuts[:-1], cuts))


@pytest.mark.gpu
@pytest.mark.parametrize("mask_kind", ("runs", "none", "all"))
@pytest.mark.parametrize("n", (1, 255, 257, 100003))
def test_sgd_clip_step_masked_vs_torch(n, mask_kind):
    """Three steps of ragmi_sgd_clip_step_masked over a flat buffer cut into runs of 1-700 elements, each run a parameter of a CPU
    torch.optim.SGD whose .grad is None while the run is inactive (+ clip_grad_norm_).  `runs`: the active runs change every step;
    `none`: nothing may move and the norm is 0; `all`: additionally bitwise equal to ragmi_sgd_clip_step(first_step=0)."""
    from rag_amd import ops
    lr, mom, wd, clip = 1e-2, 0.9, 3e-3, 5.0
    gen = torch.Generator().manual_seed(n)
    segs = _segments(n, n + 1)
    flat0 = torch.randn(n, generator=gen)
    refs = [torch.nn.Parameter(flat0[a:b].clone()) for a, b in segs]
    opt = torch.optim.SGD(refs, lr=lr, momentum=mom, weight_decay=wd)
    p, buf = flat0.to(DEV), torch.zeros(n, device=DEV)
    p_u, buf_u = p.clone(), buf.clone()                                   # the unmasked launch's copies (`all`)
    for step in range(3):
        if mask_kind == "runs":
            on = [(i + step) % 2 == 0 for i in range(len(segs))] if step < 2 else list(np.random.RandomState(n + 7).rand(len(segs)) < 0.5)
        else:
            on = [mask_kind == "all"] * len(segs)
        grad = torch.randn(n, generator=gen) * (0.3 if step != 1 else 1e-3)       # n = 100003: clipped in steps 0 and 2
        mask = torch.zeros(n, dtype=torch.uint8)
        for (a, b), q, o in zip(segs, refs, on):
            q.grad = grad[a:b].clone() if o else None
            mask[a:b] = int(o)
        total_ref = torch.nn.utils.clip_grad_norm_(refs, clip)
        opt.step()
        g_dev, m_dev = grad.to(DEV), mask.to(DEV)
        p0, buf0 = p.clone(), buf.clone()
        total = ops.sgd_clip_step_masked(p, g_dev, buf, m_dev, lr, mom, wd, clip)
        idle = ~mask.bool().to(DEV)
        assert torch.equal(p[idle], p0[idle]) and torch.equal(buf[idle], buf0[idle]) and torch.equal(g_dev[idle], grad.to(DEV)[idle])
        close(total, total_ref.reshape(1), 3e-6, f"norm {step}")           # torch accumulates the norm in fp32
        if not any(on):
            assert total.item() == 0.0
        ref_p = torch.cat([q.detach() for q in refs])
        ref_g = torch.cat([q.grad if q.grad is not None else torch.zeros_like(q) for q in refs])
        ref_b = torch.cat([opt.state[q]["momentum_buffer"] if "momentum_buffer" in opt.state.get(q, {}) else torch.zeros_like(q)
                           for q in refs])
        act = mask.bool()
        if bool(act.any()):
            close(p.cpu()[act], ref_p[act], 1e-6, f"param {step}")
            close(g_dev.cpu()[act], ref_g[act], 1e-6, f"clipped grad {step}")
        close(buf.cpu(), ref_b, 1e-6, f"momentum {step}")
        if mask_kind == "all":
            g_u = grad.to(DEV)
            total_u = ops.sgd_clip_step(p_u, g_u, buf_u, lr, mom, wd, clip, False)
            assert torch.equal(total, total_u) and torch.equal(p, p_u) and torch.equal(buf, buf_u) and torch.equal(g_dev, g_u)


# --------------------------------------------------------------------------- GPU: the captured step
def _graphed_vs_eager(build, left, right, gt, draw_a, draw_b, a_only_of, hyper):
    """first_loss + two replays == three eager train_step calls on a twin network; a second capture with another draw over the same
    optimizer works and leaves the parameters only the first draw sampled bit for bit.  Driven like
    test_hip_train.py::test_graphed_train_step_matches_eager: a device sync before every replay and a clone of the loss between
    replays; its tolerances, for its reason (float atomics in the weight gradients amplified by SGD steps on fresh weights)."""
    from rag_amd.train import FlatSGD, GradBucket, GraphedTrainStep, train_step
    finals = []
    for graphed in (False, True):
        net = build()
        bucket = GradBucket(net.parameters())
        opt = FlatSGD(bucket, **hyper)
        if graphed:
            step = GraphedTrainStep(net, opt, bucket, left, right, gt, sampled_ops=draw_a, warmup=1)
            c = step.node_census
            assert c["memcpy"] == 0 and c["memset"] == 0 and c["kernel"] > 100, c
            held = [step.first_loss.clone()]
            for _ in range(2):
                torch.cuda.synchronize()
                held.append(step().clone())
            torch.cuda.synchronize()
            losses = [float(x) for x in held]
        else:
            losses = [float(train_step(net, opt, bucket, left, right, gt, sampled_ops=draw_a)) for _ in range(3)]
        finals.append((losses, {k: v.detach().clone() for k, v in net.state_dict().items()}))
        if graphed:
            named = dict(net.named_parameters())
            a_only = a_only_of(net)
            assert len(a_only) > 20
            keep = {k: (named[k].detach().clone(), _momentum(opt, bucket, named[k])) for k in a_only}
            step_b = GraphedTrainStep(net, opt, bucket, left, right, gt, sampled_ops=draw_b, warmup=1)
            c = step_b.node_census
            assert c["memcpy"] == 0 and c["memset"] == 0 and c["kernel"] > 100, c
            torch.cuda.synchronize()
            lb = [float(step_b.first_loss), float(step_b().clone())]
            torch.cuda.synchronize()
            assert all(np.isfinite(lb)), lb
            for k, (p0, m0) in keep.items():
                assert torch.equal(named[k].detach(), p0), k
                assert bool(m0.any()) and torch.equal(_momentum(opt, bucket, named[k]), m0), k
    (l0, s0), (l1, s1) = finals
    print("eager", l0, "graphed", l1)
    assert l0[0] != l0[1] and l1[0] != l1[1]
    for a, b in zip(l0, l1):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (l0, l1)
    for k in s0:
        close(s1[k].float(), s0[k].float(), 5e-3, k)


def _a_only(draw_a, draw_b):
    def pick(net):
        by_id = {id(p): k for k, p in net.named_parameters()}
        b = {id(p) for p in net.active_parameters(*draw_b)}
        return sorted(by_id[id(p)] for p in net.active_parameters(*draw_a) if id(p) not in b)
    return pick


@pytest.mark.gpu
def test_graphed_depth_search_step_matches_eager():
    g = g23()
    _graphed_vs_eager(lambda: _depth_net(DEV).train(), gpu(g["left"]), None, gpu(g["gt"]), DRAW_A, DRAW_B, _a_only(DRAW_A, DRAW_B), HYPER)


@pytest.mark.gpu
def test_graphed_stereo_search_step_matches_eager():
    """g9 is B=1 (refused by the census: torch.cat of 5-D tensors is a copy there): its inputs tiled to B=2."""
    g = load_golden("g9_supernet")
    left, right, gt = (gpu(np.concatenate([g[k], g[k]])) for k in ("left", "right", "gt"))
    draw_a = ([int(v) for v in g["fea_ops"]], [int(v) for v in g["mat_ops"]])
    _graphed_vs_eager(lambda: _stereo_net(DEV)[0].train(), left, right, gt, draw_a, DRAW_B, _a_only(draw_a, DRAW_B),
                      dict(lr=1e-3, momentum=0.9, weight_decay=3e-3))
