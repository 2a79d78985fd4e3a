"""The occlusion-aware self-supervised step (rag_amd.train.forward_backward / train_step / GraphedTrainStep with supervise=False,
occlusion=True) and Network.forward_lr: the step is the composition of the public pieces - lr_stack, ONE forward of the 2B batch,
lr_consistency on the detached disparities (mirrored, partner_shift = B), the weighted re_and_sm_loss over all 2B pairs, backward,
update - and is captured as kernel nodes only.  The GPU tests run on the network and the 36 x 48 crop of the existing self-supervised
step tests (g13_selfsup_train_step with g6's weights).

Unmarked tests run without a GPU; the rest need the MI355X."""
import pytest
import torch

from conftest import load_golden, split_sd

DEV = "cuda:0"


class _TinyNet(torch.nn.Module):
    """A stand-in with Network's call signature: disparity = w0 + w1 * mean_c(left - right)."""
    maxdisp = 24
    arch_init = None

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([1.5, 2.0]))

    def forward(self, left, right, task, arch):
        return self.w[0] + self.w[1] * (left - right).mean(1)


def _cpu_pair(seed=3, B=2, H=9, W=14):
    g = torch.Generator().manual_seed(seed)
    left = torch.rand((B, 3, H, W), generator=g)
    return left, (left.roll(1, -1) + 0.3 * torch.rand((B, 3, H, W), generator=g))


# --------------------------------------------------------------------------- CPU
def test_forward_backward_occlusion_on_cpu_is_the_twin_composition():
    from rag_amd.metrics import lr_consistency_torch, re_and_sm_loss_torch
    from rag_amd.train import GradBucket, forward_backward
    left, right = _cpu_pair()
    B = left.shape[0]
    kw = dict(lr_tol=(0.5, 0.1), occluded_weight=0.25)
    net = _TinyNet()
    bucket = GradBucket(net.parameters())
    bucket.flat.fill_(7.0)                                    # stale gradient: zeroed by the step
    loss = forward_backward(net, bucket, left, right, None, supervise=False, occlusion=True, **kw)
    ref_net = _TinyNet()
    left2, right2 = torch.cat((left, right.flip(-1))), torch.cat((right, left.flip(-1)))
    disp = ref_net(left2, right2, 0, None)
    assert disp.shape[0] == 2 * B
    chk = lr_consistency_torch(disp.detach(), disp.detach(), 0.5, 0.1, 0.25, mirrored=True, partner_shift=B)
    assert 0 < int(chk.mask.sum()) < chk.mask.numel()         # the weight is neither all ones nor all 0.25
    ref = re_and_sm_loss_torch(disp, left2, right2, chk.weight)[0]
    ref.backward()
    assert torch.allclose(loss, ref.detach(), rtol=1e-6, atol=0)
    assert torch.allclose(bucket.flat, ref_net.w.grad, rtol=1e-5, atol=1e-9) and bucket.flat.abs().max() > 0
    plain = forward_backward(_TinyNet(), GradBucket(_TinyNet().parameters()), left, right, None, supervise=False)
    assert float(plain) != float(loss)                        # the default path is untouched and is another loss


def test_train_step_occlusion_on_cpu_updates_the_parameters():
    from rag_amd.train import GradBucket, train_step
    left, right = _cpu_pair()
    net = _TinyNet()
    bucket = GradBucket(net.parameters())
    before = net.w.detach().clone()
    loss = train_step(net, torch.optim.SGD(net.parameters(), lr=0.1), bucket, left, right, None, supervise=False, occlusion=True)
    assert bool(torch.isfinite(loss)) and not torch.equal(net.w.detach(), before)


def test_occlusion_step_refusals():
    """ValueError before any launch: occlusion=True with supervise=True, features=True, sampled_ops, selected_ops, uncertainty, a meter,
    a depth network, or parameters outside their ranges - from forward_backward, train_step and GraphedTrainStep alike."""
    import rag_amd
    from rag_amd.train import GradBucket, GraphedTrainStep, forward_backward, train_step
    net = _TinyNet()
    bucket = GradBucket(net.parameters())
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    x = torch.zeros(1, 3, 6, 6)
    gt = torch.ones(1, 6, 6)
    cases = (
        (dict(supervise=True), gt, "supervise"),
        (dict(supervise=False, features=True), None, "features"),
        (dict(supervise=False, sampled_ops=([0], [0])), None, "sampled_ops"),
        (dict(supervise=False, selected_ops=[0] * 18, t=0), None, "selected_ops"),
        (dict(supervise=False, uncertainty=True), None, "uncertainty"),
        (dict(supervise=False, meter=object()), None, "meter"),
        (dict(supervise=False, lr_tol=(-1.0, 0.0)), None, "lr_tol"),
        (dict(supervise=False, lr_tol=(1.0,)), None, "lr_tol"),
        (dict(supervise=False, occluded_weight=1.5), None, "occluded_weight"),
        (dict(supervise=False, occluded_weight=float("nan")), None, "occluded_weight"),
    )
    for kw, g, word in cases:
        with pytest.raises(ValueError, match=word):
            forward_backward(net, bucket, x, x, g, occlusion=True, **kw)
        with pytest.raises(ValueError, match=word):
            train_step(net, opt, bucket, x, x, g, occlusion=True, **kw)
        with pytest.raises(ValueError, match=word):
            GraphedTrainStep(net, opt, bucket, x, x, g, occlusion=True, **kw)
    depth = rag_amd.DepthNetwork.__new__(rag_amd.DepthNetwork)       # the type decides; nothing of it is run
    for call in (lambda: forward_backward(depth, bucket, x, None, None, supervise=False, occlusion=True),
                 lambda: train_step(depth, opt, bucket, x, None, None, supervise=False, occlusion=True),
                 lambda: GraphedTrainStep(depth, opt, bucket, x, None, None, supervise=False, occlusion=True)):
        with pytest.raises(ValueError, match="depth"):
            call()
    with pytest.raises(NotImplementedError, match="second view"):    # nothing is defined for the depth network
        depth.forward_lr(x, x, 0)


def test_new_names_are_exported():
    import rag_amd
    for name in ("LRCheck", "lr_consistency", "lr_consistency_torch", "lr_stack", "re_and_sm_loss", "re_and_sm_loss_torch"):
        assert name in rag_amd.__all__ and hasattr(rag_amd, name), name
    assert hasattr(rag_amd.Network, "forward_lr") and hasattr(rag_amd.checkpoint.MultiTaskStereo, "forward_lr")


# --------------------------------------------------------------------------- GPU
def gpu(x):
    return torch.as_tensor(x).to(DEV)


@pytest.fixture(scope="module")
def ra():
    import rag_amd
    rag_amd.load_library()
    return rag_amd


def _network(ra, g6, g13):
    """The network of test_selfsup_loss.py's step tests: g13's genotype rows and maxdisp, g6's weights, training mode."""
    rows = g13["rows"]
    net = ra.Network(ra.Genotype(rows, None, rows, None), DEV, maxdisp=int(g13["maxdisp"]))
    net.load_state_dict(split_sd(g6), strict=True)
    net = net.to(DEV).train()
    net.stem3d0[0].eval()
    return net


def _fixtures():
    g6, g = load_golden("g6_train_step"), load_golden("g13_selfsup_train_step")
    return g6, g, gpu(g["left"]), gpu(g["right"])


KW = dict(lr_tol=(1.0, 0.05), occluded_weight=0.25)


@pytest.mark.gpu
def test_occlusion_train_step_is_the_composition_of_the_public_pieces(ra):
    """One train_step(..., supervise=False, occlusion=True) against lr_stack -> forward of 2B -> lr_consistency -> weighted loss ->
    backward -> update written out on a second copy of the network.  Both issue the same launches in the same order; only the float
    atomics of the 1x1x1 / strided weight gradients may order differently, so the loss (computed before any of them) is compared to
    1e-6 and the updated state to 1e-5."""
    from rag_amd.train import GradBucket, exchange_and_update, make_optimizer, train_step
    g6, g, left, right = _fixtures()
    B = left.shape[0]
    states, losses = [], []
    for composed in (False, True):
        net = _network(ra, g6, g)
        bucket = GradBucket(net.parameters())
        opt = make_optimizer(net.parameters(), lr=1e-3, bucket=bucket)
        if composed:
            with ra.ops.conv_precision("fp32"):
                left2, right2 = ra.lr_stack(left, right)
                disp = net(left2, right2, 0, net.arch_init)
                chk = ra.lr_consistency(disp.detach(), disp.detach(), 1.0, 0.05, 0.25, mirrored=True, partner_shift=B)
                loss = ra.re_and_sm_loss(disp, left2, right2, weight=chk.weight)
                bucket.zero()
                loss.backward()
            exchange_and_update(opt, bucket, clip=5.0)
            share = float(chk.mask.float().mean())
            assert disp.shape == (2 * B,) + tuple(left.shape[2:]) and 0.0 < share < 1.0, share
            assert float((bucket.flat != 0).float().mean()) > 0.5
        else:
            loss = train_step(net, opt, bucket, left, right, None, supervise=False, occlusion=True, **KW)
        torch.cuda.synchronize()
        losses.append(float(loss.detach()))
        states.append({k: v.detach().float().cpu() for k, v in net.state_dict().items()})
    assert abs(losses[0] - losses[1]) <= 1e-6 * abs(losses[1]), losses
    for k, ref in states[1].items():
        assert float((states[0][k] - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())), k
    net = _network(ra, g6, g)                                  # and the step did move the weights
    moved = max(float((states[0][k] - v.detach().float().cpu()).abs().max()) for k, v in net.state_dict().items())
    assert moved > 0


@pytest.mark.gpu
def test_graphed_occlusion_step_matches_eager_with_kernel_nodes_only(ra):
    """GraphedTrainStep(supervise=False, occlusion=True) on [B, ...] static inputs: kernel nodes only, and three replays == the eager
    train_step (the pattern and the bounds of test_selfsup_loss.py::test_graphed_selfsup_step_matches_eager)."""
    from rag_amd.train import GradBucket, GraphedTrainStep, make_optimizer, train_step
    g6, g, left, right = _fixtures()
    finals = []
    for graphed in (False, True):
        net = _network(ra, g6, g)
        net.modify_param({"stem_3d0": [0]}, requires_grad=False)
        bucket = GradBucket(net.parameters())
        opt = make_optimizer(net.parameters(), lr=1e-3, bucket=bucket)
        if graphed:
            step = GraphedTrainStep(net, opt, bucket, left, right, None, warmup=2, supervise=False, occlusion=True, **KW)
            assert step.node_census["memcpy"] == 0 and step.node_census["memset"] == 0 and step.node_census["other"] == 0 \
                and step.node_census["kernel"] > 100, step.node_census
            assert step.left.shape == left.shape and step.right.shape == right.shape       # the 2B buffers are internal
            held = []
            for _ in range(3):
                torch.cuda.synchronize()
                held.append(step().clone())
            torch.cuda.synchronize()
            losses = [None, None] + [float(x) for x in held]
        else:
            losses = [float(train_step(net, opt, bucket, left, right, None, supervise=False, occlusion=True, **KW)) for _ in range(5)]
        finals.append((losses, {k: v.detach().clone() for k, v in net.state_dict().items()}))
    (l0, s0), (l1, s1) = finals
    for a, b in zip(l0[2:], l1[2:]):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (l0, l1)
    for k in s0:
        ref = s0[k].float().cpu()
        err = float((s1[k].float().cpu() - ref).abs().max())
        assert err <= 5e-3 * max(1.0, float(ref.abs().max())), k


@pytest.mark.gpu
def test_forward_lr_gives_both_views_and_their_checks(ra):
    """Each disparity within the project's 1e-3 px gate of net(...) on the corresponding (mirrored) pair, each LRCheck bit for bit
    lr_consistency on the returned disparities; MultiTaskStereo forwards to it; inputs that autograd tracks are refused."""
    g6, g, left, right = _fixtures()
    net = _network(ra, g6, g).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    kw = dict(abs_tol=1.0, rel_tol=0.05, occluded_weight=0.25)
    disp_l, disp_r, chk_l, chk_r = net.forward_lr(left, right, 0, net.arch_init, **kw)
    with torch.no_grad():
        ref_l = net(left, right, 0, net.arch_init)
        ref_r = net(right.flip(-1).contiguous(), left.flip(-1).contiguous(), 0, net.arch_init).flip(-1)
    torch.cuda.synchronize()
    assert disp_l.shape == disp_r.shape == ref_l.shape
    e_l, e_r = float((disp_l - ref_l).abs().max()), float((disp_r - ref_r).abs().max())
    print(f"FORWARD_LR e_left={e_l:.2e} e_right={e_r:.2e} px valid_left={chk_l.valid.tolist()} valid_right={chk_r.valid.tolist()}")
    assert e_l <= 1e-3 and e_r <= 1e-3
    want_l = ra.lr_consistency(disp_l, disp_r, **kw)
    want_r = ra.lr_consistency(disp_r.flip(-1), disp_l, mirrored=True, **kw)
    for got, want, back in ((chk_l, want_l, lambda v: v), (chk_r, want_r, lambda v: v.flip(-1))):
        assert torch.equal(got.weight, back(want.weight)) and torch.equal(got.error, back(want.error)) and torch.equal(got.valid, want.valid)
        assert torch.equal(got.mask, back(want.mask))
    serve = ra.checkpoint.MultiTaskStereo(net, [net.arch_init])
    again = serve.forward_lr(left, right, 0, **kw)
    assert torch.equal(again[0], disp_l) and torch.equal(again[1], disp_r) and torch.equal(again[3].weight, chk_r.weight)
    assert net.forward_lr(left, right, 0, net.arch_init, want_error=False)[2].error is None
    with pytest.raises(RuntimeError, match="inference only"):
        net.forward_lr(left.clone().requires_grad_(True), right, 0, net.arch_init)
    with pytest.raises(TypeError, match="mirrored"):
        net.forward_lr(left, right, 0, net.arch_init, mirrored=False)
