"""The head's tap form with the x blend of upsample_6 taken once, in the resample launch:
ops.trilinear3d_act_k1(xblend=True) writes the nine x-blended row volumes Q [B, 9, D6, H6, 2 W6] and ops.uptaps3d(xblended=True) is
left the y and z blends.  Checked: the window property the producer's neighbour exchange rests on (CPU), the decision (CPU), each
launch against float64, the producer against Q formed on the host in fp32 from the P6 launch's own output (equal bits), the pair
against today's pair (equal bits: the same explicit fmaf chains in the same order), inside MatchingNet, and run-to-run.

Tolerances: 3e-5 / 3e-5 against float64 is test_head_taps' TOL64 (fp32 sums of <= 324 products of O(1) values around fp32 source
indices).  Everything else is torch.equal."""
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
f32 = np.float32
# `low` at level 12: every voxel a border; B = 2 and odd sizes; level-6 width 40 (one 30-column tile edge); level-6 width 50 and
# partial tiles on every axis
SHAPES = [(1, 2, 2, 2), (2, 3, 5, 7), (1, 5, 9, 20), (2, 3, 19, 25)]
HEADLINE = (1, 16, 32, 104)      # low [1,12,16,32,104] -> mat [1,1,64,128,416]


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


# --------------------------------------------------------------------------- host twins
def lin_twin(X, n_in, n_out):
    """csrc/common.h lin_index(X, n_in, n_out, lin_scale(n_in, n_out, 1), align_corners=1) in numpy fp32: (i0, i1, w0, w1)"""
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    src = f32(scale * f32(X))
    i0 = min(int(src), n_in - 1)
    lam = min(max(f32(src - f32(i0)), f32(0)), f32(1))
    return i0, i0 + (1 if i0 < n_in - 1 else 0), f32(f32(1) - lam), f32(lam)


def lin_twin_vec(X, n_in, n_out):
    """lin_twin over an int array"""
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    src = (scale * X.astype(f32)).astype(f32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    lam = np.clip((src - i0.astype(f32)).astype(f32), f32(0), f32(1))
    return i0, i0 + (i0 < n_in - 1), (f32(1) - lam).astype(f32), lam


def window_weights(gx, x6, w6):
    """the producer's three weights of upsampled column gx over the level-6 slots x6-1, x6, x6+1 (zeros outside [0, 2 w6)), and the
    weight that falls outside the window (the window property says: none)"""
    win, outside = [f32(0)] * 3, f32(0)
    if 0 <= gx < 2 * w6:
        i0, i1, w0, w1 = lin_twin(gx, w6, 2 * w6)
        for i, w in ((i0, w0), (i1, w1)):
            if 0 <= i - (x6 - 1) < 3:
                win[i - (x6 - 1)] = f32(win[i - (x6 - 1)] + w)
            elif w != 0:
                outside = f32(outside + abs(w))
    return win, outside


def fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product is exact in float64; the sum is rounded to odd there (TwoSum's error
    term tells whether it was inexact), which makes the second rounding, to 24 bits, the only one that counts."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)
    even = (t.view(np.int64) & 1) == 0
    t = np.where((err != 0) & even, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
    return t.astype(f32)


def q_from_p_fp32(p):
    """Q [B, 9, D, H, 2 W] from P [B, 27, D, H, W] with the kernels' chain: dx ascending, window slots ascending, the first term a
    product, every later one an fmaf (fp32)."""
    p = np.ascontiguousarray(p, dtype=f32)
    B, T, D, H, W = p.shape
    p = p.reshape(B, 9, 3, D, H, W)
    q = np.empty((B, 9, D, H, 2 * W), dtype=f32)
    for gx in range(2 * W):
        x6, acc = gx // 2, None
        for dx in range(3):
            win, _ = window_weights(gx + dx - 1, x6, W)
            for s in range(3):
                v = p[:, :, dx, :, :, min(max(x6 - 1 + s, 0), W - 1)]
                acc = f32(win[s]) * v if acc is None else fma32(np.full_like(v, win[s]), v, acc)
        q[..., gx] = acc
    return q


def q_from_p_f64(p64):
    """the same sum in float64 over the fp32 source-index rule: the x2 upsample along x as a matrix, shifted by dx - 1, zero padded"""
    B, T, D, H, W = p64.shape
    U = torch.zeros((2 * W, W), dtype=torch.float64)
    for gx in range(2 * W):
        i0, i1, w0, w1 = lin_twin(gx, W, 2 * W)
        U[gx, i0] += float(w0)
        U[gx, i1] += float(w1)
    up = F.pad(torch.einsum("gx,btdhx->btdhg", U, p64), (1, 1))
    q = torch.zeros((B, 9, D, H, 2 * W), dtype=torch.float64)
    for t in range(27):
        q[:, t // 3] += up[:, t, :, :, t % 3:t % 3 + 2 * W]
    return q


def _uptaps_ref(p):
    """float64 sum_t shift_t(pad(F.interpolate(P_t))): tap t = dz*9 + dy*3 + dx reads the upsampled volume at v + (dz, dy, dx) - 1
    (test_head_taps._uptaps_ref)"""
    B, T, Di, Hi, Wi = p.shape
    up = F.interpolate(p, scale_factor=2, mode="trilinear", align_corners=True).double()
    D, H, W = up.shape[2:]
    pad = F.pad(up, (1, 1, 1, 1, 1, 1))
    ref = torch.zeros((B, 1, D, H, W), dtype=torch.float64)
    for t in range(27):
        dz, dy, dx = t // 9, t // 3 % 3, t % 3
        ref[:, 0] += pad[:, t, dz:dz + D, dy:dy + H, dx:dx + W]
    return ref


def _x_w(shape, c=12):
    B, Di, Hi, Wi = shape
    x = torch.randn((B, c, Di, Hi, Wi), generator=gen(41))
    w = torch.randn((1, c, 3, 3, 3), generator=gen(42)) * (2.0 / (27 * c)) ** 0.5
    return x, w


# --------------------------------------------------------------------------- CPU: the window property, the twins, the decision
def test_window_property_every_width():
    """exact x2, align_corners=True, every level-6 width 2..600: for level-6 column x6, both outputs gx in {2 x6, 2 x6 + 1} and every
    dx, each source index with a non-zero weight lies in {x6-1, x6, x6+1} — a thread needs its two x neighbours' P and no more."""
    for w6 in range(2, 601):
        x6 = np.arange(w6)
        for j in range(2):
            for dx in range(3):
                g = 2 * x6 + j + dx - 1
                live = (g >= 0) & (g < 2 * w6)                      # (a column outside the row has zero weights)
                i0, i1, w0, w1 = lin_twin_vec(np.clip(g, 0, 2 * w6 - 1), w6, 2 * w6)
                bad = live & (((w0 != 0) & (abs(i0 - x6) > 1)) | ((w1 != 0) & (abs(i1 - x6) > 1)))
                assert not bad.any(), (w6, j, dx, x6[bad])
    for w6 in (2, 3, 7, 104, 208, 600):                             # the array twin is the scalar twin, and the producer's window
        i0, i1, w0, w1 = lin_twin_vec(np.arange(2 * w6), w6, 2 * w6)
        for gx in range(2 * w6):
            assert (i0[gx], i1[gx], w0[gx], w1[gx]) == lin_twin(gx, w6, 2 * w6), (w6, gx)
            for dx in range(3):
                assert window_weights(gx + dx - 1, gx // 2, w6)[1] == 0, (w6, gx, dx)


def test_fma32_twin_rounds_once():
    """cases where the float64 sum rounds first and the float32 rounding of THAT differs from the single rounding of fmaf"""
    a, b = np.array([1 + 2.0 ** -12], dtype=f32), np.array([1 + 2.0 ** -12], dtype=f32)     # a*b = 1 + 2^-11 + 2^-24: a float32 tie ...
    for c, want in ((2.0 ** -80, 1 + 2.0 ** -11 + 2.0 ** -23), (-2.0 ** -80, 1 + 2.0 ** -11)):      # ... broken by a term far below
        assert fma32(a, b, np.array([c], dtype=f32))[0] == f32(want), c
    from fractions import Fraction
    r = np.random.default_rng(0)
    x, y, z = (r.standard_normal(256).astype(f32) for _ in range(3))
    got = fma32(x, y, z)
    for a, b, c, v in zip(x, y, z, got):                            # no float32 is nearer to the exact rational than the twin's
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        near = abs(exact - Fraction(float(v)))
        for other in (np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))):
            assert near <= abs(exact - Fraction(float(other))), (a, b, c, v)


def test_host_q_twins_agree():
    """the fp32 chain and the float64 matrix form of Q are the same sum (so the GPU tests that use one check what the other states)"""
    p = torch.randn((2, 27, 2, 3, 9), generator=gen(7))
    q32, q64 = q_from_p_fp32(p.numpy()), q_from_p_f64(p.double())
    np.testing.assert_allclose(q32.astype(np.float64), q64.numpy(), rtol=2e-6, atol=2e-6)      # <= 9 fp32 terms of O(1) values


def test_plan_head_xblend_levels_switches_and_training(built_lib):
    import rag_amd
    from rag_amd import ops
    from rag_amd.modules import _HeadPlan, _plan_head, _plan_head_taps, _plan_head_xblend
    net = rag_amd.MatchingNet(rag_amd.ALL_CONV_GENOTYPE, maxdisp=48).eval()
    m3, m6, m12 = net.last_3_3d[0], net.last_6_3d[0], net.last_12_3d[0]
    vol, tf32, bf16 = (16, 48, 72), torch.float32, torch.bfloat16
    sizes = {1: (16, 48, 72), 2: (8, 24, 36), 4: (4, 12, 18)}
    assert built_lib.ragmi_trilinear3d_act_k1_xblend_supported(12, 27, 4, 12, 18, 8, 24, 36, 1) == 1
    assert built_lib.ragmi_uptaps3d_xblended_supported(8, 24, 36) == 1
    old = ops.chain_k1_enabled(), ops.bf16_head_fp32_enabled(), ops.head_taps_enabled(), ops.head_xblend_enabled()

    def plans(level, dtype=tf32, train=False, vol=vol, m3=m3):
        plan = _plan_head(vol, sizes[level], dtype, m3, m6, m12, train)
        taps = _plan_head_taps(plan, vol, sizes[level], dtype, m3, m6)
        return plan, taps, _plan_head_xblend(plan, vol, sizes[level], dtype, m3, m6)

    try:
        ops.set_chain_k1(True)
        ops.set_bf16_head_fp32(True)
        ops.set_head_taps(True)
        ops.set_head_xblend(True)
        with torch.no_grad():
            assert plans(4) == (_HeadPlan(4, False, True, True), True, True)
            assert plans(1)[1:] == (False, False) and plans(2)[1:] == (False, False)       # no 1/4-level resample launch
            assert plans(4, bf16)[1:] == (False, False)                                    # the crossing launch, no chain
            ops.set_bf16_head_fp32(False)
            assert plans(4, bf16) == (_HeadPlan(4, False, True, True), False, False)       # a bf16-stored `low`
            ops.set_bf16_head_fp32(True)
            assert plans(4, train=True)[1:] == (False, False)
            assert plans(4, vol=(17, 48, 72))[1:] == (False, False)                        # no exact factor 2
            ops.set_chain_k1(False)
            assert plans(4) == (_HeadPlan(4, False, False, True), False, False)            # the three switches, one at a time
            ops.set_chain_k1(True)
            ops.set_head_taps(False)
            assert plans(4) == (_HeadPlan(4, False, True, True), False, False)
            ops.set_head_taps(True)
            ops.set_head_xblend(False)
            assert plans(4) == (_HeadPlan(4, False, True, True), True, False)              # _plan_head / _plan_head_taps as they were
            ops.set_head_xblend(True)
            # a width the head kernels do not take (odd level-6 width: no whole 16-byte rows): neither tap form
            plan = _plan_head((16, 48, 70), (4, 12, 17), tf32, m3, m6, m12, False)
            assert _plan_head_taps(plan, (16, 48, 70), (4, 12, 17), tf32, m3, m6) is False
            assert _plan_head_xblend(plan, (16, 48, 70), (4, 12, 17), tf32, m3, m6) is False
    finally:
        ops.set_chain_k1(old[0])
        ops.set_bf16_head_fp32(old[1])
        ops.set_head_taps(old[2])
        ops.set_head_xblend(old[3])


def test_head_xblend_predicates_and_symbols(built_lib):
    for name in ("ragmi_trilinear3d_act_k1_xblend_fwd", "ragmi_trilinear3d_act_k1_xblend_supported", "ragmi_uptaps3d_xblended_fwd",
                 "ragmi_uptaps3d_xblended_supported"):
        assert hasattr(built_lib, name)
    assert built_lib.ragmi_version() >= 580
    k1, ut = built_lib.ragmi_trilinear3d_act_k1_xblend_supported, built_lib.ragmi_uptaps3d_xblended_supported
    assert k1(12, 27, 16, 32, 104, 32, 64, 208, 1) == 1 and k1(64, 27, 2, 2, 2, 4, 4, 4, 1) == 1
    assert k1(12, 32, 2, 2, 2, 4, 4, 4, 1) == 0 and k1(12, 26, 2, 2, 2, 4, 4, 4, 1) == 0       # the 27 taps only
    assert k1(12, 27, 2, 2, 2, 4, 4, 6, 1) == 0                                              # x3 along x: not the exact x2
    assert k1(12, 27, 4, 4, 4, 6, 8, 8, 1) == 0 and k1(65, 27, 2, 2, 2, 4, 4, 4, 1) == 0
    assert ut(32, 64, 208) == 1 and ut(2, 2, 2) == 1
    assert ut(1, 4, 4) == 0 and ut(4, 4, 5) == 0 and ut(2048, 2048, 32) == 0


# --------------------------------------------------------------------------- GPU: the producer
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_producer_vs_float64_and_host_fp32(ra, shape):
    """Q against float64 (ATen's fp32 F.interpolate + ReLU, the float64 mix, a float64 x blend) and, bit for bit, against Q formed on
    the host in fp32 from the P6 launch's own output; written at a channel offset of a NaN-filled buffer."""
    B, Di, Hi, Wi = shape
    size = (2 * Di, 2 * Hi, 2 * Wi)
    x, w = _x_w(shape)
    assert ra.ops.trilinear3d_act_k1_supported(12, 27, shape[1:], size, True, xblend=True)
    out = torch.full((B, 9 + 3, size[0], size[1], 2 * size[2]), float("nan"), device=DEV)
    ra.ops.trilinear3d_act_k1(gpu(x), size, True, True, gpu(w), out, 2, transposed=True, xblend=True)
    got = out.cpu()
    assert torch.isnan(got[:, :2]).all() and torch.isnan(got[:, 11:]).all()
    q = got[:, 2:11]
    assert torch.isfinite(q).all()
    up = F.relu(F.interpolate(x, size=size, mode="trilinear", align_corners=True))
    p64 = torch.einsum("co,bcdhw->bodhw", w.reshape(12, 27).double(), up.double())
    ref = q_from_p_f64(p64)
    print(f"x-blend producer {shape}: max abs err vs float64 {float((q.double() - ref).abs().max()):.2e}")
    np.testing.assert_allclose(q.double().numpy(), ref.numpy(), **TOL64)
    p6 = ra.ops.trilinear3d_act_k1(gpu(x), size, True, True, gpu(w), transposed=True).cpu()
    host = torch.from_numpy(q_from_p_fp32(p6.numpy()))
    diff = (q != host)
    assert torch.equal(q, host), (int(diff.sum()), float((q - host).abs().max()))


# --------------------------------------------------------------------------- GPU: the consumer
@pytest.mark.gpu
@pytest.mark.parametrize("shape,bn", [
    ((1, 2, 2, 2), False),          # every voxel a border
    ((2, 5, 37, 50), True),         # partial tiles everywhere, a partial depth segment, B = 2; scale / shift / ReLU
    ((1, 7, 33, 18), False)])       # a tile border one row past 64 output rows
def test_consumer_vs_float64(ra, shape, bn):
    """uptaps3d(xblended=True) on Q formed on the host (fp32 chain) from a random P, against the float64 sum over P"""
    B, Di, Hi, Wi = shape
    p = torch.randn((B, 27, Di, Hi, Wi), generator=gen(51)) * (2.0 / 27) ** 0.5
    ref = _uptaps_ref(p)
    scale = shift = None
    if bn:
        scale, shift = torch.rand(1, generator=gen(52)) + 0.5, torch.randn(1, generator=gen(53)) * 0.1
        ref = F.relu(ref * scale.double() + shift.double())
    q = torch.from_numpy(q_from_p_fp32(p.numpy()))
    assert ra.ops.uptaps3d_supported(Di, Hi, Wi, xblended=True)
    out = torch.full((B, 3, 2 * Di, 2 * Hi, 2 * Wi), float("nan"), device=DEV)
    ra.ops.uptaps3d(gpu(q), gpu(scale) if bn else None, gpu(shift) if bn else None, bn, out, 1, xblended=True)
    got = out.cpu()
    assert torch.isnan(got[:, 0]).all() and torch.isnan(got[:, 2]).all()
    print(f"x-blended uptaps3d {shape}: max abs err vs float64 {float((got[:, 1:2].double() - ref).abs().max()):.2e}")
    np.testing.assert_allclose(got[:, 1:2].double().numpy(), ref.numpy(), **TOL64)


# --------------------------------------------------------------------------- GPU: the pair against today's pair, and against itself
def _pairs(ra, shape):
    B, Di, Hi, Wi = shape
    x, w = _x_w(shape)
    half = (2 * Di, 2 * Hi, 2 * Wi)
    xd, wd = gpu(x), gpu(w)
    p6 = ra.ops.trilinear3d_act_k1(xd, half, True, True, wd, transposed=True)
    old = ra.ops.uptaps3d(p6, None, None, False)

    def new():
        q6 = ra.ops.trilinear3d_act_k1(xd, half, True, True, wd, transposed=True, xblend=True)
        return ra.ops.uptaps3d(q6, None, None, False, xblended=True)
    return old, new


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + [HEADLINE])
def test_xblend_pair_equals_todays_pair(ra, shape):
    """the same explicit fmaf chains in the same order: equal bits on finite seeded inputs"""
    old, new = _pairs(ra, shape)
    got = new()
    assert tuple(got.shape) == tuple(old.shape) == (shape[0], 1, 4 * shape[1], 4 * shape[2], 4 * shape[3])
    assert torch.isfinite(old).all()
    ne = got != old
    print(f"x-blend pair vs tap pair {shape}: {int(ne.sum())} of {got.numel()} differ, max abs diff {float((got - old).abs().max()):.2e}")
    assert torch.equal(got, old)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SHAPES[3], HEADLINE])
def test_xblend_pair_repeats_its_bits(ra, shape):
    _, new = _pairs(ra, shape)
    a = new().clone()
    assert torch.equal(a, new())


# --------------------------------------------------------------------------- GPU: MatchingNet, switch on against off
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


NATIVE = ("ragmi_trilinear3d_act_k1_xblend_fwd", "ragmi_uptaps3d_xblended_fwd", "ragmi_trilinear3d_act_k1_fwd", "ragmi_uptaps3d_fwd")


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(16, 24), (12, 20)])      # (12: a multiple of 4 but not of 8 — odd sizes at the 1/4 level)
def test_matchingnet_head_xblend_on_against_off(ra, monkeypatch, h, w):
    """the switch on reaches both new native entry points exactly once (and the old two not at all) through the same two ops, and
    gives the switch-off forward's disparities bit for bit; the captured forward holds as many kernel nodes, no memcpy / memset."""
    ops, lib = ra.ops, ra.load_library()
    net, lf, rf = _matching_net(ra, h, w)
    calls = []
    for name in ("trilinear3d_act_k1", "uptaps3d"):
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(ops, name), name))
    for name in NATIVE:
        monkeypatch.setattr(lib, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(getattr(lib, name), name))
    old = ops.head_taps_enabled(), ops.head_xblend_enabled()
    try:
        ops.set_head_taps(True)
        res = {}
        with torch.no_grad():
            for on in (False, True):
                ops.set_head_xblend(on)
                del calls[:]
                res[on] = net(lf, rf).cpu()
                want = (["trilinear3d_act_k1", NATIVE[0], "uptaps3d", NATIVE[1]] if on
                        else ["trilinear3d_act_k1", NATIVE[2], "uptaps3d", NATIVE[3]])
                assert calls == want, calls
                res[on, "graph"], res[on, "census"] = _captured(net, lf, rf)
                assert torch.equal(res[on, "graph"].cpu(), res[on])
    finally:
        ops.set_head_taps(old[0])
        ops.set_head_xblend(old[1])
    for on in (False, True):
        c = res[on, "census"]
        assert c["memcpy"] == 0 and c["memset"] == 0 and c["kernel"] > 0, c
    assert res[True, "census"]["kernel"] == res[False, "census"]["kernel"], (res[True, "census"], res[False, "census"])
    print(f"head x-blend on vs off [{h}x{w}]: max |diff| {float((res[True] - res[False]).abs().max()):.2e} px")
    assert torch.equal(res[True], res[False])
