"""The head with last_3_3d's channel sum taken before the x2 upsample (rag_model.py:269, 357-365):
ops.trilinear3d_act_k1 (resample + ReLU + 1x1x1 mix into the 27 tap volumes) -> ops.uptaps3d (27 shifted x2 samples, summed), against
float64 references over ATen's fp32 F.interpolate, against today's head (trilinear3d_act -> upconv3d_c1), and inside MatchingNet.

Tolerances: 3e-5 / 3e-5 against float64 is test_upconv3d_c1_fused_head_vs_oracle's (fp32 sums of <= 324 products of O(1) values around fp32
source indices); 2e-5 / 2e-5 between the two head orders is the one that test grants between this library's two head paths."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import matching_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TOL64 = dict(rtol=3e-5, atol=3e-5)
TOL_PATHS = dict(rtol=2e-5, atol=2e-5)


def gpu(x):
    return torch.as_tensor(x).to(DEV)


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def ra():
    import rag_amd
    rag_amd.load_library()
    return rag_amd


@pytest.fixture(scope="session")
def built_lib():
    import rag_amd
    if not os.path.exists(rag_amd.lib_path()):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return rag_amd.load_library()


def _x_w(c, shape, cout=27):
    """randn activations; a [Cout, C] mix scaled as a [1, C, 3, 3, 3] conv weight"""
    B, Di, Hi, Wi = shape
    x = torch.randn((B, c, Di, Hi, Wi), generator=gen(41))
    w = torch.randn((cout, c), generator=gen(42)) * (2.0 / (27 * c)) ** 0.5
    return x, w


# --------------------------------------------------------------------------- trilinear3d_act_k1
@pytest.mark.gpu
@pytest.mark.parametrize("c,cout,shape,relu,transposed", [
    (12, 27, (1, 2, 2, 2), True, True),        # every voxel a border
    (12, 27, (2, 3, 5, 7), True, True),        # B = 2, odd sizes: partial blocks on every axis
    (4, 27, (1, 5, 9, 20), True, False),       # one channel group, [Cout][C] weight
    (12, 27, (2, 3, 5, 7), False, False),      # no ReLU
    (6, 32, (1, 3, 4, 6), True, False)])       # a partial last channel group; the 32-accumulator instantiation
def test_trilinear3d_act_k1_vs_float64(ra, c, cout, shape, relu, transposed):
    """against einsum in float64 over ATen's fp32 F.interpolate (+ReLU), and against ops.trilinear3d_act + the same float64 mix (same
    resampled bits: that comparison isolates the mix); written at a channel offset of a wider NaN-filled buffer."""
    B, Di, Hi, Wi = shape
    size = (2 * Di, 2 * Hi, 2 * Wi)
    x, w = _x_w(c, shape, cout)
    up = F.interpolate(x, size=size, mode="trilinear", align_corners=True)
    if relu:
        up = F.relu(up)
    ref = torch.einsum("oc,bcdhw->bodhw", w.double(), up.double())
    assert ra.ops.trilinear3d_act_k1_supported(c, cout, shape[1:], size, True)
    out = torch.full((B, cout + 3, *size), float("nan"), device=DEV)
    wk = w.t().contiguous() if transposed else w
    ra.ops.trilinear3d_act_k1(gpu(x), size, True, relu, gpu(wk), out, 2, transposed=transposed)
    got = out.cpu()
    assert torch.isnan(got[:, :2]).all() and torch.isnan(got[:, 2 + cout:]).all()
    err = float((got[:, 2:2 + cout].double() - ref).abs().max())
    print(f"trilinear3d_act_k1 C={c} Cout={cout} {shape}: max abs err vs float64 {err:.2e}")
    np.testing.assert_allclose(got[:, 2:2 + cout].double().numpy(), ref.numpy(), **TOL64)
    own = torch.empty((B, c, *size), device=DEV)
    ra.ops.trilinear3d_act(gpu(x), size, True, relu, own, 0)
    mixed = torch.einsum("oc,bcdhw->bodhw", w.double(), own.cpu().double())
    # fp32 FMAs over <= 12 products against their float64 sum: C * 2^-24 * sum |w x| stays far below 2e-6 at these magnitudes
    np.testing.assert_allclose(got[:, 2:2 + cout].double().numpy(), mixed.numpy(), rtol=2e-6, atol=2e-6)


@pytest.mark.gpu
def test_trilinear3d_act_k1_reads_a_channel_slice(ra):
    x, w = _x_w(12, (2, 3, 5, 7))
    wide = torch.randn((2, 16, 3, 5, 7), generator=gen(43))
    wide[:, 3:15] = x
    size = (6, 10, 14)
    a = ra.ops.trilinear3d_act_k1(gpu(wide)[:, 3:15], size, True, True, gpu(w))
    b = ra.ops.trilinear3d_act_k1(gpu(x), size, True, True, gpu(w))
    assert torch.equal(a, b)


# --------------------------------------------------------------------------- uptaps3d
def _uptaps_ref(p):
    """float64 sum_t shift_t(pad(F.interpolate(P_t))): tap t = dz*9 + dy*3 + dx reads the upsampled volume at v + (dz, dy, dx) - 1"""
    B, T, Di, Hi, Wi = p.shape
    up = F.interpolate(p, scale_factor=2, mode="trilinear", align_corners=True).double()
    D, H, W = up.shape[2:]
    pad = F.pad(up, (1, 1, 1, 1, 1, 1))
    ref = torch.zeros((B, 1, D, H, W), dtype=torch.float64)
    for t in range(27):
        dz, dy, dx = t // 9, t // 3 % 3, t % 3
        ref[:, 0] += pad[:, t, dz:dz + D, dy:dy + H, dx:dx + W]
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("shape,bn", [
    ((1, 2, 2, 2), False),          # every voxel a border
    ((2, 5, 37, 50), True),         # partial tiles everywhere, a partial depth segment, B = 2; scale / shift / ReLU
    ((1, 7, 33, 18), False)])       # a tile border one row past 64 output rows
def test_uptaps3d_vs_float64(ra, shape, bn):
    B, Di, Hi, Wi = shape
    p = torch.randn((B, 27, Di, Hi, Wi), generator=gen(51)) * (2.0 / 27) ** 0.5
    ref = _uptaps_ref(p)
    scale = shift = None
    if bn:
        scale, shift = torch.rand(1, generator=gen(52)) + 0.5, torch.randn(1, generator=gen(53)) * 0.1
        ref = F.relu(ref * scale.double() + shift.double())
    assert ra.ops.uptaps3d_supported(Di, Hi, Wi)
    out = torch.full((B, 3, 2 * Di, 2 * Hi, 2 * Wi), float("nan"), device=DEV)
    ra.ops.uptaps3d(gpu(p), gpu(scale) if bn else None, gpu(shift) if bn else None, bn, out, 1)
    got = out.cpu()
    assert torch.isnan(got[:, 0]).all() and torch.isnan(got[:, 2]).all()
    print(f"uptaps3d {shape}: max abs err vs float64 {float((got[:, 1:2].double() - ref).abs().max()):.2e}")
    np.testing.assert_allclose(got[:, 1:2].double().numpy(), ref.numpy(), **TOL64)


@pytest.mark.gpu
@pytest.mark.parametrize("tap", [0, 5, 13, 21, 26])
def test_uptaps3d_single_tap_is_a_shifted_upsample(ra, tap):
    """P zero except one tap volume: the output is that volume's upsample shifted by the tap's offset, zero where the shift leaves the
    volume — a wrong offset or padding edge is a displaced volume, not noise."""
    shape = (1, 5, 37, 50)
    p = torch.zeros((1, 27, 5, 37, 50))
    p[:, tap] = torch.randn((1, 5, 37, 50), generator=gen(54))
    ref = _uptaps_ref(p)
    got = ra.ops.uptaps3d(gpu(p), None, None, False).cpu()
    np.testing.assert_allclose(got.double().numpy(), ref.numpy(), **TOL64)
    dz, dy, dx = tap // 9 - 1, tap // 3 % 3 - 1, tap % 3 - 1
    up = F.interpolate(p[:, tap:tap + 1], scale_factor=2, mode="trilinear", align_corners=True)
    D, H, W = up.shape[2:]
    zs, ys, xs = (slice(max(-d, 0), n - max(d, 0)) for d, n in ((dz, D), (dy, H), (dx, W)))
    zt, yt, xt = (slice(max(d, 0), n + min(d, 0)) for d, n in ((dz, D), (dy, H), (dx, W)))
    np.testing.assert_allclose(got[:, :, zs, ys, xs].numpy(), up[:, :, zt, yt, xt].numpy(), **TOL64)
    edge = torch.ones((D, H, W), dtype=torch.bool)
    edge[zs, ys, xs] = False
    assert (got[0, 0][edge] == 0).all(), shape


# --------------------------------------------------------------------------- both launches against today's head
@pytest.mark.gpu
@pytest.mark.parametrize("c,shape", [
    (12, (1, 2, 2, 2)), (12, (2, 3, 5, 7)), (4, (1, 5, 9, 20)),
    (12, (1, 16, 32, 104))])        # the headline head: low [1,12,16,32,104] -> mat [1,1,64,128,416]
def test_tap_head_matches_channel_head(ra, c, shape):
    """trilinear3d_act -> upconv3d_c1 and trilinear3d_act_k1 -> uptaps3d on the same (x, w): one fp32 reassociation apart (on the CPU the
    tap-first order sits at under 7 % of this tolerance), so a failure is a bug, not rounding."""
    B, Di, Hi, Wi = shape
    x = torch.randn((B, c, Di, Hi, Wi), generator=gen(41))
    w = torch.randn((1, c, 3, 3, 3), generator=gen(42)) * (2.0 / (27 * c)) ** 0.5
    half = (2 * Di, 2 * Hi, 2 * Wi)
    xd, wd = gpu(x), gpu(w)
    y6 = torch.empty((B, c, *half), device=DEV)
    ra.ops.trilinear3d_act(xd, half, True, True, y6, 0)
    old = ra.ops.upconv3d_c1(y6, wd, None, None, False)
    p6 = ra.ops.trilinear3d_act_k1(xd, half, True, True, wd, transposed=True)
    new = ra.ops.uptaps3d(p6, None, None, False)
    assert tuple(new.shape) == tuple(old.shape) == (B, 1, 4 * Di, 4 * Hi, 4 * Wi)
    print(f"tap head vs channel head C={c} {shape}: max abs diff {float((new - old).abs().max()):.2e}")
    np.testing.assert_allclose(new.cpu().numpy(), old.cpu().numpy(), **TOL_PATHS)


# --------------------------------------------------------------------------- MatchingNet: switch on against off
def _matching_net(ra, h, w):
    rows = np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]])
    net = ra.MatchingNet(ra.Genotype(normal=rows, normal_concat=None, reduce=rows, reduce_concat=None), maxdisp=48)
    net.load_state_dict(O.random_matching_state_dict(rows, seed=0), strict=True)
    g = gen(1234)
    return net.to(DEV).eval(), gpu(torch.randn((2, 12, h, w), generator=g)), gpu(torch.randn((2, 12, h, w), generator=g))


def _captured(net, lf, rf):
    from rag_amd.train import graph_census
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net(lf, rf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        out = net(lf, rf)
    census = graph_census(graph)
    graph.instantiate()
    graph.replay()
    torch.cuda.synchronize()
    return out.clone(), census


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(16, 24), (12, 20)])      # (12: a multiple of 4 but not of 8 — odd sizes at the 1/4 level)
def test_matchingnet_head_taps_on_against_off(ra, monkeypatch, h, w):
    """MatchingNet.forward with the switch on takes the tap form (both new launches, once each) and gives the disparities of the
    switch-off forward within test_matchingnet_golden's gates; the captured forward holds as many kernel nodes, no memcpy / memset."""
    ops = ra.ops
    net, lf, rf = _matching_net(ra, h, w)
    calls = []
    for name in ("trilinear3d_act_k1", "uptaps3d", "trilinear3d_act", "upconv3d_c1"):
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(ops, name), name))
    old = ops.head_taps_enabled()
    try:
        res = {}
        with torch.no_grad():
            for on in (False, True):
                ops.set_head_taps(on)
                del calls[:]
                res[on] = net(lf, rf).cpu()
                head = [n for n in calls if n in ("trilinear3d_act_k1", "uptaps3d", "upconv3d_c1")]
                assert head == (["trilinear3d_act_k1", "uptaps3d"] if on else ["upconv3d_c1"]), calls
                res[on, "graph"], res[on, "census"] = _captured(net, lf, rf)
                assert torch.equal(res[on, "graph"].cpu(), res[on])
    finally:
        ops.set_head_taps(old)
    for on in (False, True):
        c = res[on, "census"]
        assert c["memcpy"] == 0 and c["memset"] == 0 and c["kernel"] > 0, c
    assert res[True, "census"]["kernel"] == res[False, "census"]["kernel"], (res[True, "census"], res[False, "census"])
    err = (res[True] - res[False]).abs()
    epe = O.epe(res[True], res[False])
    share_small, share_large = float((err > 2e-3).float().mean()), float((err > 5e-2).float().mean())
    print(f"head taps on vs off [{h}x{w}]: EPE {epe:.2e} px, max |diff| {float(err.max()):.2e} px")
    assert epe <= 1e-3, epe
    assert share_small < 5e-3 and share_large < 5e-4, (share_small, share_large, float(err.max()))


# --------------------------------------------------------------------------- the decision (no GPU)
def test_plan_head_taps_levels_switches_and_training(built_lib):
    import rag_amd
    from rag_amd import ops
    from rag_amd.modules import _HeadPlan, _plan_head, _plan_head_taps
    net = rag_amd.MatchingNet(rag_amd.ALL_CONV_GENOTYPE, maxdisp=48).eval()
    m3, m6, m12 = net.last_3_3d[0], net.last_6_3d[0], net.last_12_3d[0]
    vol, f32, bf16 = (16, 48, 72), torch.float32, torch.bfloat16
    sizes = {1: (16, 48, 72), 2: (8, 24, 36), 4: (4, 12, 18)}
    both = bool(built_lib.ragmi_trilinear3d_act_k1_supported(12, 27, 4, 12, 18, 8, 24, 36, 1)) and bool(built_lib.ragmi_uptaps3d_supported(8, 24, 36))
    assert both
    old = ops.chain_k1_enabled(), ops.bf16_head_fp32_enabled(), ops.head_taps_enabled()

    def taps(level, dtype=f32, train=False, vol=vol, m3=m3):
        plan = _plan_head(vol, sizes[level], dtype, m3, m6, m12, train)
        return plan, _plan_head_taps(plan, vol, sizes[level], dtype, m3, m6)

    try:
        ops.set_chain_k1(True)
        ops.set_bf16_head_fp32(True)
        ops.set_head_taps(True)
        with torch.no_grad():
            plan, on = taps(4)
            assert plan == _HeadPlan(4, False, True, True) and on is True        # _plan_head's result is what it was
            assert taps(1)[1] is False and taps(2)[1] is False                   # no 1/4-level resample launch to carry the mix
            assert taps(4, bf16)[1] is False                                     # the crossing launch, no chain
            ops.set_bf16_head_fp32(False)
            plan, on = taps(4, bf16)                                             # a bf16-stored `low`
            assert plan == _HeadPlan(4, False, True, True) and on is False
            ops.set_bf16_head_fp32(True)
            ops.set_chain_k1(False)
            assert taps(4) == (_HeadPlan(4, False, False, True), False)          # the 1/4-level step as two units
            ops.set_chain_k1(True)
            assert taps(4, train=True)[1] is False
            assert taps(4, vol=(17, 48, 72))[1] is False                         # no exact factor 2: no fused head either
            ops.set_head_taps(False)
            assert taps(4) == (_HeadPlan(4, False, True, True), False)           # the switch
            ops.set_head_taps(True)
            # the depth network's call: its own last_3_3d (no m3)
            n6, n12 = rag_amd.ConvBR_2d(24, 12, 1, 1, 0).eval(), rag_amd.ConvBR_2d(48, 24, 1, 1, 0).eval()
            plan = _plan_head((1, 48, 72), (1, 12, 18), f32, None, n6, n12, False)
            assert plan == _HeadPlan(4, False, True, False) and _plan_head_taps(plan, (1, 48, 72), (1, 12, 18), f32, None, n6) is False
    finally:
        ops.set_chain_k1(old[0])
        ops.set_bf16_head_fp32(old[1])
        ops.set_head_taps(old[2])


def test_head_taps_predicates_and_symbols(built_lib):
    for name in ("ragmi_trilinear3d_act_k1_fwd", "ragmi_trilinear3d_act_k1_supported", "ragmi_uptaps3d_fwd", "ragmi_uptaps3d_supported"):
        assert hasattr(built_lib, name)
    assert built_lib.ragmi_version() >= 570
    k1, ut = built_lib.ragmi_trilinear3d_act_k1_supported, built_lib.ragmi_uptaps3d_supported
    assert k1(12, 27, 16, 32, 104, 32, 64, 208, 1) == 1 and k1(12, 32, 2, 2, 2, 4, 4, 4, 1) == 1
    assert k1(12, 33, 2, 2, 2, 4, 4, 4, 1) == 0 and k1(65, 27, 2, 2, 2, 4, 4, 4, 1) == 0 and k1(0, 27, 2, 2, 2, 4, 4, 4, 1) == 0
    assert k1(12, 27, 4, 4, 4, 6, 8, 8, 1) == 0          # less than a factor 2 on one axis
    assert ut(32, 64, 208) == 1 and ut(2, 2, 2) == 1
    assert ut(1, 4, 4) == 0 and ut(4, 4, 5) == 0 and ut(2048, 2048, 32) == 0
