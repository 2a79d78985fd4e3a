"""The self-supervised training loss of the continual-adaptation mode (src_self/models/loss.py:112-141, re_and_sm_loss; the
supervise=False step of src_self/approaches/rag.py:266-278): the fused HIP kernel (rag_amd/csrc/selfsup_loss.hip), its autograd
Function and the training step's switch, against the REFERENCE's own numbers (g12_selfsup_loss, g13_selfsup_train_step; generator
tests/golden/make_golden_selfsup.py) and the plain-torch restatement (rag_amd.metrics.re_and_sm_loss_torch).

Unmarked tests run without a GPU (host twin, step logic, argument validation of the C ABI); the rest need the MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, split_sd

DEV = "cuda:0"
CASES = ("a", "odd", "b", "outview", "ties")


def gpu(x):
    return torch.as_tensor(x).to(DEV)


def rel_max(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def xs_of(disp64, W):
    return (2.0 * (torch.arange(W, dtype=torch.float64, device=disp64.device) - disp64) / (W - 1)) * W / 2.0 - 0.5


# --------------------------------------------------------------------------- CPU: host twin, step logic, ABI validation
@pytest.mark.parametrize("case", CASES)
def test_host_twin_matches_reference_fixture(case):
    """The plain-torch restatement the CPU step uses, against the reference's own runs: in fp64 to 1e-6 relative (loss, terms,
    gradient), and in fp32 against the reference's fp32 gradient."""
    from rag_amd.metrics import re_and_sm_loss_torch
    g = load_golden("g12_selfsup_loss")
    left, right = torch.from_numpy(g[f"{case}::left"]), torch.from_numpy(g[f"{case}::right"])
    d = torch.from_numpy(g[f"{case}::disp"]).double().requires_grad_(True)
    loss, terms = re_and_sm_loss_torch(d, left.double(), right.double())
    loss.backward()
    ref = float(g[f"{case}::loss64"])
    assert abs(loss.item() - ref) <= 1e-6 * abs(ref), (loss.item(), ref)
    for got, want in zip(terms, g[f"{case}::terms64"]):
        assert abs(got.item() - want) <= 1e-6 * abs(want), (got.item(), want)
    assert rel_max(d.grad, g[f"{case}::grad64"]) <= 1e-6
    d32 = torch.from_numpy(g[f"{case}::disp"]).requires_grad_(True)
    loss32, _ = re_and_sm_loss_torch(d32, left, right)
    loss32.backward()
    assert abs(loss32.item() - float(g[f"{case}::loss32"])) <= 1e-6 * abs(ref)
    assert rel_max(d32.grad, g[f"{case}::grad32"]) <= 1e-5


class _TinyNet(torch.nn.Module):
    """A stand-in with the Network call signature: disparity = a + b * mean_c(left - right)."""
    maxdisp = 24
    arch_init = None

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([3.0, 2.0]))

    def forward(self, left, right, task, arch):
        return self.w[0] + self.w[1] * (left - right).mean(1)


def test_forward_backward_self_supervised_on_cpu():
    """supervise=False without ground truth: the loss is re_and_sm_loss(disp, left, right) and its gradient lands in the bucket."""
    from rag_amd.metrics import re_and_sm_loss_torch
    from rag_amd.train import GradBucket, forward_backward
    g = load_golden("g12_selfsup_loss")
    left, right = torch.from_numpy(g["b::left"]), torch.from_numpy(g["b::right"])
    net = _TinyNet()
    bucket = GradBucket(net.parameters())
    bucket.flat.fill_(7.0)                                    # stale gradient: zeroed by the step
    loss = forward_backward(net, bucket, left, right, None, supervise=False)
    ref_net = _TinyNet()
    ref = re_and_sm_loss_torch(ref_net(left, right, 0, None), left, right)[0]
    ref.backward()
    assert torch.allclose(loss, ref.detach(), rtol=1e-6, atol=0)
    assert torch.allclose(bucket.flat, ref_net.w.grad, rtol=1e-5, atol=1e-9)
    assert bucket.flat.abs().max() > 0


def test_self_supervised_step_refuses_features_and_missing_gt():
    from rag_amd.train import GradBucket, forward_backward, train_step
    net = _TinyNet()
    bucket = GradBucket(net.parameters())
    x = torch.zeros(1, 3, 6, 6)
    with pytest.raises(ValueError, match="features"):
        forward_backward(net, bucket, x, x, None, supervise=False, features=True)
    with pytest.raises(ValueError, match="features"):
        train_step(net, torch.optim.SGD(net.parameters(), lr=0.1), bucket, x, x, None, supervise=False, features=True)
    with pytest.raises(ValueError, match="gt"):
        forward_backward(net, bucket, x, x, None)


def test_selfsup_abi_validates_before_launch():
    """Argument checks of ragmi_selfsup_loss_fwd run before any launch (pointers are never dereferenced)."""
    import rag_amd
    lib = rag_amd.load_library()
    fake = ctypes.c_void_p(0x1000)
    assert lib.ragmi_selfsup_loss_workspace_elems(3, 192, 384) == 2 * 3 * ((3 * 64 * 128 + 63) // 64)
    assert lib.ragmi_selfsup_loss_workspace_elems(1, 2, 8) == 0
    assert lib.ragmi_selfsup_loss_fwd(fake, fake, fake, 1, 3, 2, 8, 0, fake, fake, None, None) == -1        # H < 3
    assert b"H, W >= 3" in lib.ragmi_last_error()
    assert lib.ragmi_selfsup_loss_fwd(fake, fake, fake, 1, 5, 6, 8, 0, fake, fake, None, None) == -2        # C = 5
    assert lib.ragmi_selfsup_loss_fwd(fake, fake, fake, 1, 3, 6, 8, 1, fake, fake, None, None) == -2        # bf16
    assert b"float32" in lib.ragmi_last_error()
    assert lib.ragmi_selfsup_loss_fwd(None, fake, fake, 1, 3, 6, 8, 0, fake, fake, None, None) == -1
    assert lib.ragmi_selfsup_loss_bwd(fake, fake, fake, 0, None) == -1


# --------------------------------------------------------------------------- GPU: the fused kernel
@pytest.fixture(scope="module")
def ra():
    import rag_amd
    rag_amd.load_library()
    return rag_amd


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_fused_loss_matches_reference_fixture(ra, case):
    g = load_golden("g12_selfsup_loss")
    d = gpu(g[f"{case}::disp"]).requires_grad_(True)
    left, right = gpu(g[f"{case}::left"]), gpu(g[f"{case}::right"])
    loss = ra.metrics.re_and_sm_loss(d, left, right)
    (loss * 1.5).backward()
    terms = ra.metrics.self_supervised_terms(d, left, right).cpu().double()
    ref = float(g[f"{case}::loss64"])
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref), (loss.item(), ref)
    assert abs(float(terms[0]) - ref) <= 1e-5 * abs(ref)
    for got, want in zip(terms[1:].tolist(), g[f"{case}::terms64"]):
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    assert rel_max(d.grad / 1.5, g[f"{case}::grad64"]) <= 1e-4


def warped64(disp64, right64):
    """left_est of the loss in fp64: bilinear sample of `right` at (x - d, y) (zero padding), masked where the sample of an all-ones
    image is < 0.9999."""
    import torch.nn.functional as F
    B, _, H, W = right64.shape
    xs = torch.arange(W, dtype=torch.float64, device=disp64.device).view(1, 1, W) - disp64
    ys = torch.arange(H, dtype=torch.float64, device=disp64.device).view(1, H, 1).expand(B, H, W)
    grid = torch.stack((2 * xs / (W - 1) - 1, 2 * ys / (H - 1) - 1), dim=-1)
    cover = F.grid_sample(torch.ones_like(right64[:, :1]), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return F.grid_sample(right64, grid, mode="bilinear", padding_mode="zeros", align_corners=False) * (cover >= 0.9999)


def _crop_inputs(seed=5):
    gen = torch.Generator().manual_seed(seed)
    left = torch.randn((3, 3, 192, 384), generator=gen)
    right = torch.randn((3, 3, 192, 384), generator=gen)
    disp = torch.rand((3, 192, 384), generator=gen) * 192
    return gpu(disp), gpu(left), gpu(right)


@pytest.mark.gpu
def test_fused_loss_at_reference_crop_vs_fp64_restatement(ra):
    """B = 3, 192 x 384 (run_rag_self.sh's crop), disp ~ U(0, 192): against the fp64 restatement run by torch on the GPU.  The
    gradient check leaves out the loss's kinks, where fp32 and fp64 may pick different sides: pixels whose fp64 sample abscissa
    lies within 1e-4 of an integer (bilinear kink, mask band) and pixels where left and left_est nearly tie (torch.abs).  Some 3x3
    SSIM blocks are ill-conditioned in fp32 (the one-pass E[x^2] - mu^2 of nearly flat blocks): torch's own fp32 restatement misses
    fp64 by more than 1e-4 max|g| at a few pixels of the batch, and which blocks those are depends on the rounding.  So the kernel
    must (1) stay in the class of torch's fp32 arithmetic everywhere off the kinks and (2) be within 1e-4 max|g| at all but 0.1 %
    of those pixels."""
    disp, left, right = _crop_inputs()
    d = disp.clone().requires_grad_(True)
    loss = ra.metrics.re_and_sm_loss(d, left, right)
    loss.backward()
    d64 = disp.double().requires_grad_(True)
    ref, terms = ra.metrics.re_and_sm_loss_torch(d64, left.double(), right.double())
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())
    got_terms = ra.metrics.self_supervised_terms(disp, left, right).cpu().double()
    for got, want in zip(got_terms[1:].tolist(), terms):
        assert abs(got - want.item()) <= 1e-5 * abs(want.item()), (got, want.item())
    xs = xs_of(disp.double(), 384)
    kink_xs = (xs - xs.round()).abs() < 1e-4
    # |left - left_est| is the loss's other kink: fp32 rounds xs ~ 300 to ~3e-5, i.e. left_est to ~1e-4, so where left and the fp64
    # warp agree to 1e-3 in some channel fp32 may take the other side of torch.abs' subgradient (ATen's fp32 too): a jump of
    # 0.15 / (B C H W) * |d left_est / d disp| in the gradient
    kink_l1 = ((left.double() - warped64(disp.double(), right.double())).abs() < 1e-3).any(1)
    keep = ~(kink_xs | kink_l1)
    gref = d64.grad
    gmax = float(gref.abs().max())
    d32 = disp.clone().requires_grad_(True)                  # torch's fp32 arithmetic of the same loss: the yardstick of class
    ra.metrics.re_and_sm_loss_torch(d32, left, right)[0].backward()
    err_torch = (d32.grad.double() - gref).abs()[keep]
    err = (d.grad.double() - gref).abs()[keep]
    n_over, n_over_torch = int((err > 1e-4 * gmax).sum()), int((err_torch > 1e-4 * gmax).sum())
    excluded = int((~keep).sum())
    print(f"gradient check: {excluded} of {keep.numel()} pixels excluded ({int(kink_xs.sum())} with xs within 1e-4 of an "
          f"integer, {int(kink_l1.sum())} with |left - left_est| < 1e-3); max error / max|g|: kernel {float(err.max()) / gmax:.2e}, "
          f"torch fp32 {float(err_torch.max()) / gmax:.2e}; pixels over 1e-4 max|g|: kernel {n_over}, torch fp32 {n_over_torch}")
    assert excluded < keep.numel() // 100
    assert float(err.max()) <= 4 * float(err_torch.max()) + 1e-5 * gmax, (float(err.max()), float(err_torch.max()))
    assert n_over <= keep.numel() // 1000, n_over


@pytest.mark.gpu
def test_fused_loss_is_bitwise_deterministic(ra):
    """No float atomics: two calls give the same bits, loss and gradient."""
    disp, left, right = _crop_inputs(6)
    runs = []
    for _ in range(2):
        d = disp.clone().requires_grad_(True)
        loss = ra.metrics.re_and_sm_loss(d, left, right)
        loss.backward()
        runs.append((loss.detach().clone(), d.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


@pytest.mark.gpu
def test_fused_loss_rejects_unbuilt_inputs(ra):
    g = load_golden("g12_selfsup_loss")
    d, left, right = gpu(g["a::disp"]), gpu(g["a::left"]), gpu(g["a::right"])
    with pytest.raises(RuntimeError, match="H, W >= 3"):
        ra.metrics.re_and_sm_loss(d[:, :2], left[:, :, :2], right[:, :, :2])
    five = torch.cat([left, left[:, :2]], 1)
    with pytest.raises(RuntimeError, match="not built"):
        ra.metrics.re_and_sm_loss(d, five, five)
    with pytest.raises(RuntimeError, match="float32"):
        ra.metrics.re_and_sm_loss(d.bfloat16(), left.bfloat16(), right.bfloat16())


# --------------------------------------------------------------------------- GPU: the training step (g13)
def _g13_network(ra, g6, g13):
    rows = g13["rows"]
    net = ra.Network(ra.Genotype(rows, None, rows, None), DEV, maxdisp=int(g13["maxdisp"]))
    net.load_state_dict(split_sd(g6), strict=True)                 # g13 uses g6's weights (asserted by its generator)
    net = net.to(DEV).train()
    net.stem3d0[0].eval()
    return net


@pytest.mark.gpu
def test_selfsup_train_step_golden(ra):
    """The reference's supervise=False step (g13), split so that fp32 differences in disp cannot move pixels across bilinear
    kinks: (a) disp; (b) the loss's gradient on the fixture's own disp; (c) parameter gradients from the fixture's d loss / d disp;
    (d) the end-to-end loss."""
    g6, g = load_golden("g6_train_step"), load_golden("g13_selfsup_train_step")
    net = _g13_network(ra, g6, g)
    left, right = gpu(g["left"]), gpu(g["right"])
    disp = net(left, right, 0, net.arch_init)
    err = float((disp.detach().cpu().double() - torch.from_numpy(g["disp"]).double()).abs().max())                         # (a)
    assert err <= 2e-4 * max(1.0, float(np.abs(g["disp"]).max())), err
    d_fix = gpu(g["disp"]).requires_grad_(True)                                                                             # (b)
    ra.metrics.re_and_sm_loss(d_fix, left, right).backward()
    assert rel_max(d_fix.grad, g["grad::disp"]) <= 1e-4
    disp.backward(gpu(g["grad::disp"]))                                                                                     # (c)
    named = dict(net.named_parameters())
    n = 0
    for k, ref in g.items():
        if k.startswith("grad::") and not k.endswith("_fea") and k != "grad::disp":
            assert rel_max(named[k[6:]].grad, ref) <= 5e-4, k
            n += 1
    assert n > 40
    net2 = _g13_network(ra, g6, g)                                                                                          # (d)
    loss = ra.train.self_supervised_loss(net2(left, right, 0, net2.arch_init), left, right)
    assert abs(loss.item() - float(g["loss"])) <= 1e-3 * abs(float(g["loss"])), (loss.item(), float(g["loss"]))


@pytest.mark.gpu
def test_graphed_selfsup_step_matches_eager(ra):
    """GraphedTrainStep(supervise=False, gt=None): kernel nodes only, and three replays == the eager train_step (the replay
    pattern of test_hip_train.py::test_graphed_train_step_matches_eager: a device sync and a null-stream clone between replays)."""
    from rag_amd.train import GradBucket, GraphedTrainStep, make_optimizer, train_step
    g6, g = load_golden("g6_train_step"), load_golden("g13_selfsup_train_step")
    left, right = gpu(g["left"]), gpu(g["right"])
    finals = []
    for graphed in (False, True):
        net = _g13_network(ra, g6, g)
        net.modify_param({"stem_3d0": [0]}, requires_grad=False)
        bucket = GradBucket(net.parameters())
        opt = make_optimizer(net.parameters(), lr=1e-3, bucket=bucket)
        if graphed:
            step = GraphedTrainStep(net, opt, bucket, left, right, None, warmup=2, supervise=False)
            assert step.node_census["memcpy"] == 0 and step.node_census["memset"] == 0 and step.node_census["kernel"] > 100, step.node_census
            held = []
            for _ in range(3):
                torch.cuda.synchronize()
                held.append(step().clone())
            torch.cuda.synchronize()
            losses = [None, None] + [float(x) for x in held]
        else:
            losses = [float(train_step(net, opt, bucket, left, right, None, supervise=False)) for _ in range(5)]
        finals.append((losses, {k: v.detach().clone() for k, v in net.state_dict().items()}))
    (l0, s0), (l1, s1) = finals
    for a, b in zip(l0[2:], l1[2:]):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (l0, l1)
    for k in s0:
        ref = s0[k].float().cpu()
        err = float((s1[k].float().cpu() - ref).abs().max())
        assert err <= 5e-3 * max(1.0, float(ref.abs().max())), k


@pytest.mark.gpu
def test_selfsup_step_issues_no_memcpy_or_memset(ra):
    """The eager supervise=False step under torch.profiler: no device memcpy / memset (they would become graph nodes)."""
    from rag_amd.train import GradBucket, forward_backward
    try:
        from torch.profiler import ProfilerActivity, profile
    except Exception as exc:  # noqa: BLE001
        pytest.skip(f"torch.profiler unavailable: {exc}")
    g6, g = load_golden("g6_train_step"), load_golden("g13_selfsup_train_step")
    net = _g13_network(ra, g6, g)
    bucket = GradBucket(net.parameters())
    left, right = gpu(g["left"]), gpu(g["right"])
    forward_backward(net, bucket, left, right, None, supervise=False)
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            forward_backward(net, bucket, left, right, None, supervise=False)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events()]
    except RuntimeError as exc:
        pytest.skip(f"profiler could not trace the device: {exc}")
    assert any("selfsup_loss" in n for n in names), "the profile saw no self-supervised loss kernel"
    bad = sorted({n for n in names if "memcpy" in n.lower() or "memset" in n.lower() or "copyBuffer" in n})
    assert not bad, bad
