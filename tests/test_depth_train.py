"""Training the monocular-depth network of rag_depth (approaches/rag.py:182-246): the fused head backward and the silog loss
(rag_amd/csrc/depth_train.hip), `Network.forward_train`, and the depth training step of rag_amd.train, against the REFERENCE's own
numbers (g19, g20; generator tests/golden/make_golden_depth_train.py) and fp64 restatements.

Unmarked tests run without a GPU; the rest need the MI355X."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

DEV = "cuda:0"
HEAD_CASES = (0, 1, 2, 3)
FAKE = ctypes.c_void_p(256)      # a non-NULL pointer for argument checks that must refuse before any launch (never dereferenced)


def _json(a):
    return json.loads(bytes(a).decode())


def fp32_tol(g, name, prefix32, prefix64, floor):
    """Gate of one g20 tensor against the fp64 reference: `floor`, or 3x the reference's OWN fp32 distance from fp64 where that is
    larger (train-mode BatchNorm over B=2 on trained weights amplifies fp32 rounding to a few percent on some tensors)."""
    return max(floor, 3.0 * rel_max(g[prefix32 + name], g[prefix64 + name]))


def rel_max(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def gpu(x):
    return torch.as_tensor(np.asarray(x)).to(DEV)


# --------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("k", (0, 1, 2))
def test_silog_loss_torch_matches_reference(k):
    from rag_amd.depth import silog_loss_torch
    g = load_golden("g19_depth_head_bwd")
    est = torch.as_tensor(g[f"silog{k}_est"]).requires_grad_(True)
    loss = silog_loss_torch(est, torch.as_tensor(g[f"silog{k}_gt"]))
    loss.backward()
    assert abs(loss.item() - float(g[f"silog{k}_loss"])) <= 1e-6 * abs(float(g[f"silog{k}_loss"]))
    assert rel_max(est.grad, g[f"silog{k}_grad"]) <= 1e-6


def test_depth_train_abi_exported_and_validated():
    """New symbols, version, and refusals before any launch: NULL pointers, bf16, Cin > 16."""
    from rag_amd import _lib
    lib = ctypes.CDLL(_lib.lib_path())
    for name in ("ragmi_depth_head_bwd", "ragmi_depth_head_bwd_workspace_elems", "ragmi_silog_loss_fwd", "ragmi_silog_loss_bwd",
                 "ragmi_silog_loss_workspace_elems"):
        assert hasattr(lib, name), name
    L = _lib.load_library()
    assert L.ragmi_version() >= 530
    assert L.ragmi_depth_head_bwd_workspace_elems(2, 12, 16, 32) > 2 * 16 * 32
    assert L.ragmi_silog_loss_workspace_elems(1000) > 0
    head = lambda p, cin, dt: L.ragmi_depth_head_bwd(p, p, p, p, p, p, p, p, p, 0, p, 1, cin, 8, 16, 16, 32, 3, 80.0, dt, None)  # noqa: E731
    assert head(None, 12, 0) == -1                       # RAGMI_EINVAL
    assert head(FAKE, 12, 1) == -2                       # bf16: RAGMI_EUNSUPPORTED
    assert head(FAKE, 17, 0) == -2                       # Cin > 16
    assert L.ragmi_silog_loss_fwd(None, None, 10, 0.85, None, None, None, 0, None) == -1
    assert L.ragmi_silog_loss_fwd(FAKE, FAKE, 10, 0.85, FAKE, FAKE, FAKE, 1, None) == -2
    assert L.ragmi_silog_loss_bwd(None, None, 10, 0.85, None, None, None, 0, None) == -1
    assert L.ragmi_silog_loss_bwd(FAKE, FAKE, 10, 0.85, FAKE, FAKE, FAKE, 1, None) == -2


def test_depth_forward_backward_refuses_self_supervision_and_features():
    from rag_amd.depth import Network
    from rag_amd.modules import ALL_CONV_GENOTYPE
    from rag_amd.train import GradBucket, forward_backward
    net = Network(ALL_CONV_GENOTYPE, "cpu")
    bucket = GradBucket(net.parameters())
    left, gt = torch.zeros((1, 3, 36, 48)), torch.ones((1, 36, 48))
    with pytest.raises(ValueError, match="supervise=False"):
        forward_backward(net, bucket, left, None, gt, supervise=False)
    with pytest.raises(ValueError, match="features=True"):
        forward_backward(net, bucket, left, None, gt, features=True)
    with pytest.raises(ValueError, match="ground-truth depth"):
        forward_backward(net, bucket, left, None, None)


def test_depth_forward_still_inference_only_and_names_forward_train():
    from rag_amd.depth import Network
    from rag_amd.modules import ALL_CONV_GENOTYPE
    net = Network(ALL_CONV_GENOTYPE, "cpu").eval()
    with pytest.raises(RuntimeError, match="inference only") as exc:
        net(torch.zeros((1, 3, 36, 48)), None, 0, net.arch_init)
    assert "forward_train" in str(exc.value)


# --------------------------------------------------------------------------- GPU: head backward
def _head_inputs(k):
    g16, g19 = load_golden("g16_depth_head"), load_golden("g19_depth_head_bwd")
    y, w3, w1, b1 = (gpu(g16[f"case{k}_{n}"]) for n in ("y", "w3", "w1", "b1"))
    hw = tuple(int(v) for v in g16[f"case{k}_hw"])
    return y, w3, w1, b1, hw, gpu(g19[f"case{k}_dout"].astype(np.float32)), g19


@pytest.mark.gpu
@pytest.mark.parametrize("k", HEAD_CASES)
def test_depth_head_bwd_vs_fp64_reference(k):
    """dy, dw3, dw1, db1 of upsample_6 -> last_3_3d -> DispHead -> x80 against the reference's fp64 autograd (g19; case 3 saturates
    the sigmoid); two runs bitwise equal; accumulation into pre-filled buffers adds exactly."""
    from rag_amd import ops
    y, w3, w1, b1, hw, dout, g = _head_inputs(k)
    r1 = ops.depth_head_bwd(y, w3, w1, b1, dout, hw, 3, 80.0)
    r2 = ops.depth_head_bwd(y, w3, w1, b1, dout, hw, 3, 80.0)
    torch.cuda.synchronize()
    for name, got, again in zip(("dy", "dw3", "dw1", "db1"), r1, r2):
        ref = g[f"case{k}_{name}_64"]
        assert rel_max(got.reshape(ref.shape), ref) <= 1e-4, name
        assert torch.equal(got, again), name
    pre = [torch.randn(t.shape, device=DEV) for t in r1[1:]]
    into = [p.clone() for p in pre]
    out = ops.depth_head_bwd(y, w3, w1, b1, dout, hw, 3, 80.0, *into)
    torch.cuda.synchronize()
    for p, fresh, acc, o in zip(pre, r1[1:], into, out[1:]):
        assert o.data_ptr() == acc.data_ptr()
        assert torch.equal(acc, p + fresh)
    assert torch.equal(out[0], r1[0])


@pytest.mark.gpu
def test_depth_head_fn_autograd_matches_torch():
    """DepthHeadFn through torch.autograd == the plain-torch head's fp64 autograd on a random case with an odd, non-doubling size."""
    from rag_amd.depth import DepthHeadFn, depth_head_torch
    g = torch.Generator().manual_seed(7)
    y = torch.randn((2, 12, 7, 11), generator=g, dtype=torch.float64)
    w3 = torch.randn((1, 12, 3, 3), generator=g, dtype=torch.float64) * 0.1
    w1 = torch.randn((1, 1, 3, 3), generator=g, dtype=torch.float64)
    b1 = torch.randn((1,), generator=g, dtype=torch.float64)
    dout = torch.randn((2, 3 * 15, 3 * 25), generator=g, dtype=torch.float64)
    ref = [t.clone().requires_grad_(True) for t in (y, w3, w1, b1)]
    depth_head_torch(*ref, (15, 25), 3, 80.0).backward(dout)
    ins = [t.float().to(DEV).requires_grad_(True) for t in (y, w3, w1, b1)]
    DepthHeadFn.apply(*ins, (15, 25), 3, 80.0).backward(dout.float().to(DEV))
    for a, r in zip(ins, ref):
        assert rel_max(a.grad, r.grad) <= 1e-4


# --------------------------------------------------------------------------- GPU: silog
def _silog64(est, gt, vf=0.85):
    e, t = est.double(), gt.double()
    mask = t > 0
    d = torch.where(mask, torch.log(e) - torch.log(torch.where(mask, t, 1.0)), 0.0)
    n = mask.sum()
    md, md2 = d.sum() / n, (d * d).sum() / n
    sa = torch.sqrt(md2 - vf * md * md)
    grad = torch.where(mask, 10.0 * (d - vf * md) / (n * sa * e), 0.0)
    return 10.0 * sa, grad


@pytest.mark.gpu
@pytest.mark.parametrize("k", (0, 1, 2))
def test_silog_fwd_bwd_vs_reference_and_deterministic(k):
    from rag_amd.depth import silog_loss
    g = load_golden("g19_depth_head_bwd")
    gt = gpu(g[f"silog{k}_gt"])
    grads, losses = [], []
    for _ in range(2):
        est = gpu(g[f"silog{k}_est"]).requires_grad_(True)
        loss = silog_loss(est, gt)
        loss.backward()
        grads.append(est.grad)
        losses.append(loss.detach())
    ref = float(g[f"silog{k}_loss"])
    assert abs(losses[0].item() - ref) <= 1e-5 * abs(ref)
    assert rel_max(grads[0], g[f"silog{k}_grad"]) <= 1e-5
    assert torch.equal(losses[0], losses[1]) and torch.equal(grads[0], grads[1])


@pytest.mark.gpu
def test_silog_at_training_crop_vs_fp64():
    """B=8 384x768 (the reference's training crop): loss and gradient against an fp64 restatement; bitwise deterministic."""
    from rag_amd.depth import silog_loss
    g = torch.Generator().manual_seed(11)
    est = torch.rand((8, 384, 768), generator=g) * 79 + 0.5
    gt = est * torch.exp(torch.randn((8, 384, 768), generator=g) * 0.3)
    gt[torch.rand((8, 384, 768), generator=g) < 0.6] = 0
    ref_loss, ref_grad = _silog64(est, gt)
    out = []
    for _ in range(2):
        e = est.to(DEV).requires_grad_(True)
        loss = silog_loss(e, gt.to(DEV))
        loss.backward()
        out.append((loss.detach(), e.grad))
    assert abs(out[0][0].item() - float(ref_loss)) <= 1e-5 * float(ref_loss)
    assert rel_max(out[0][1], ref_grad) <= 1e-5
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_silog_without_valid_pixels_nan_loss_zero_grad():
    from rag_amd.depth import silog_loss
    est = (torch.rand((2, 24, 40)) * 10 + 1).to(DEV).requires_grad_(True)
    loss = silog_loss(est, torch.zeros((2, 24, 40), device=DEV))
    loss.backward()
    assert torch.isnan(loss).item()
    assert torch.equal(est.grad, torch.zeros_like(est.grad))


# --------------------------------------------------------------------------- GPU: the training step
def _sd():
    return {k: torch.as_tensor(v) for k, v in load_golden("g14_depth_ckpt_task3").items()}


def _step_net(g20):
    """g14's weights, model.train(), the units outside model_to_train in eval() and frozen (approaches/rag.py:125-127, 185-228)."""
    from rag_amd.depth import load_depth_checkpoint
    net = load_depth_checkpoint({"model": _sd()}, DEV, "from_keys")[0]
    mtt = {k: [int(i) for i in v] for k, v in _json(g20["model_to_train"]).items()}
    net.train()
    for name, idxs in mtt.items():
        for i, unit in enumerate(net._units(name)):
            if i not in idxs:
                unit.eval()
    for p in net.parameters():
        p.requires_grad_(False)
    net.modify_param(mtt, True)
    archi = {k: [int(i) for i in v] for k, v in _json(g20["archi"]).items()}
    return net, archi, mtt


@pytest.mark.gpu
def test_depth_train_step_golden():
    """The reference's task-3 step (g20), split so that fp32 differences in depth cannot move pixels across ReLU / bilinear kinks:
    (a) depth_est; (b) the loss gradient on the fixture's depth_est; (c) parameter gradients from the fixture's d loss / d depth;
    (d) the end-to-end loss; then the running statistics after the forward (eval units bit-unchanged).  Gradients and statistics are
    checked against the fp64 reference at fp32_tol: the reference's own fp32 run is up to ~5 % away from fp64 on some tensors."""
    from rag_amd import ops
    from rag_amd.depth import silog_loss
    g = load_golden("g20_depth_train_step")
    net, archi, mtt = _step_net(g)
    left, gt = gpu(g["left"]), gpu(g["gt"])
    with ops.conv_precision("fp32"):                     # the training step's arithmetic (rag_amd.train.TRAIN_PRECISION)
        est = net.forward_train(left, 3, archi)
    ref = g["depth_est"]
    assert float((est.detach().cpu().double() - torch.as_tensor(ref).double()).abs().max()) <= 2e-4 * max(1.0, float(np.abs(ref).max()))  # (a)
    d_fix = gpu(ref).requires_grad_(True)                                                                                     # (b)
    silog_loss(d_fix, gt).backward()
    assert rel_max(d_fix.grad, g["grad::depth_est"]) <= 1e-4
    with ops.conv_precision("fp32"):
        est.backward(gpu(g["grad::depth_est"]))                                                                               # (c)
    named = dict(net.named_parameters())
    n = 0
    for k in g:
        if k.startswith("grad64::"):
            name = k[8:]
            err = rel_max(named[name].grad, g[k])
            assert err <= fp32_tol(g, name, "grad::", "grad64::", 5e-4), (name, err)
            n += 1
    assert n > 40
    sd, ref_sd = net.state_dict(), _sd()                                                                                      # statistics
    for k, r in g.items():
        if k.startswith("after::") and ("running_" in k or "num_batches" in k):
            got = sd[k[7:]].cpu()
            if "num_batches" in k:
                assert int(got) == int(r), k
            else:
                err = rel_max(got, g["after64::" + k[7:]])
                assert err <= fp32_tol(g, k[7:], "after::", "after64::", 1e-4), (k, err)
    frozen = 0
    for name in mtt:
        for i, unit in enumerate(net._units(name)):
            if i in mtt[name]:
                continue
            for m in unit.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    prefix = [k for k, v in net.named_modules() if v is m][0]
                    for b in ("running_mean", "running_var", "num_batches_tracked"):
                        assert torch.equal(sd[f"{prefix}.{b}"].cpu(), ref_sd[f"{prefix}.{b}"]), prefix
                    frozen += 1
    assert frozen > 10
    net2, _, _ = _step_net(g)                                                                                                 # (d)
    loss = silog_loss(net2.forward_train(left, 3, archi), gt)
    assert abs(loss.item() - float(g["loss"])) <= 1e-3 * abs(float(g["loss"])), (loss.item(), float(g["loss"]))


@pytest.mark.gpu
def test_depth_flat_sgd_step_vs_reference():
    """clip_grad_norm_(5) + SGD(1e-3, 0.9, 3e-3) of FlatSGD on the reference's own gradients == the reference's parameters after the
    step (g20), and the total norm."""
    from rag_amd.train import FlatSGD, GradBucket
    g = load_golden("g20_depth_train_step")
    net, _archi, _mtt = _step_net(g)
    bucket = GradBucket(net.parameters())
    opt = FlatSGD(bucket, lr=1e-3, momentum=0.9, weight_decay=3e-3)
    named = dict(net.named_parameters())
    for k, r in g.items():
        if k.startswith("grad::") and k != "grad::depth_est":
            named[k[6:]].grad.copy_(gpu(r))
    total = opt.step(5.0)
    assert abs(total.item() - float(g["total_norm"])) <= 1e-5 * float(g["total_norm"])
    for k, r in g.items():
        if k.startswith("after::") and k[7:] in named:
            assert rel_max(named[k[7:]], r) <= 1e-6, k


@pytest.mark.gpu
def test_depth_train_step_matches_reference_update():
    """train_step(depth_net, opt, bucket, left, None, gt) end to end == the reference's step: the parameter update (after - before)
    of every trained tensor against the fp64 step, at the fp32 reference's own distance from it (fp32_tol)."""
    from rag_amd.train import GradBucket, make_optimizer, train_step
    g = load_golden("g20_depth_train_step")
    net, archi, _mtt = _step_net(g)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    bucket = GradBucket(net.parameters())
    opt = make_optimizer(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=3e-3, bucket=bucket)
    loss = train_step(net, opt, bucket, gpu(g["left"]), None, gpu(g["gt"]), task_arch=archi)
    assert abs(loss.item() - float(g["loss"])) <= 1e-3 * abs(float(g["loss"]))
    named = dict(net.named_parameters())
    n = 0
    for k in list(g):
        if k.startswith("delta64::"):
            name = k[9:]
            delta = named[name].detach() - before[name]
            g["delta32::" + name] = (gpu(g["after::" + name]) - before[name]).cpu()
            err = rel_max(delta, g[k])
            assert err <= fp32_tol(g, name, "delta32::", "delta64::", 2e-3), (name, err)
            n += 1
    assert n > 40


@pytest.mark.gpu
def test_graphed_depth_train_step_matches_eager():
    """GraphedTrainStep on a depth network (right=None): kernel nodes only, and three replays == the eager train_step (the replay
    pattern of test_hip_train.py::test_graphed_train_step_matches_eager)."""
    from rag_amd.train import GradBucket, GraphedTrainStep, make_optimizer, train_step
    g = load_golden("g20_depth_train_step")
    left, gt = gpu(g["left"]), gpu(g["gt"])
    finals = []
    for graphed in (False, True):
        net, archi, _mtt = _step_net(g)
        bucket = GradBucket(net.parameters())
        opt = make_optimizer(net.parameters(), lr=1e-3, bucket=bucket)
        if graphed:
            step = GraphedTrainStep(net, opt, bucket, left, None, gt, task_arch=archi, warmup=2)
            assert step.node_census["memcpy"] == 0 and step.node_census["memset"] == 0 and step.node_census["kernel"] > 50, step.node_census
            held = []
            for _ in range(3):
                torch.cuda.synchronize()
                held.append(step().clone())
            torch.cuda.synchronize()
            losses = [None, None] + [float(x) for x in held]
        else:
            losses = [float(train_step(net, opt, bucket, left, None, gt, task_arch=archi)) for _ in range(5)]
        finals.append((losses, {k: v.detach().clone() for k, v in net.state_dict().items()}))
    (l0, s0), (l1, s1) = finals
    for a, b in zip(l0[2:], l1[2:]):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (l0, l1)
    for k in s0:
        ref = s0[k].float().cpu()
        err = float((s1[k].float().cpu() - ref).abs().max())
        assert err <= 5e-3 * max(1.0, float(ref.abs().max())), k


@pytest.mark.gpu
def test_depth_head_and_silog_run_only_ragmi_kernels():
    """torch.profiler over one eager DepthHeadFn + SilogLossFn forward and backward: every device kernel is one of ours."""
    from rag_amd.depth import DepthHeadFn, SilogLossFn
    try:
        from torch.profiler import ProfilerActivity, profile
    except Exception as exc:  # noqa: BLE001
        pytest.skip(f"torch.profiler unavailable: {exc}")
    y, w3, w1, b1, hw, _dout, _g = _head_inputs(0)
    ins = [t.clone().requires_grad_(True) for t in (y, w3, w1, b1)]
    gt = torch.rand((y.shape[0], 3 * hw[0], 3 * hw[1]), device=DEV) * 70 + 1
    one = torch.ones((), device=DEV)                     # the loss's incoming gradient, made outside the profiled region
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            SilogLossFn.apply(DepthHeadFn.apply(*ins, hw, 3, 80.0), gt, 0.85).backward(one)
            torch.cuda.synchronize()
        kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    except RuntimeError as exc:
        pytest.skip(f"profiler could not trace the device: {exc}")
    assert any("depth_head_bwd" in n for n in kernels) and any("silog" in n for n in kernels), kernels
    bad = sorted({n for n in kernels if "ragmi" not in n})
    assert not bad, bad
