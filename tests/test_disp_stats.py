"""Per-pixel statistics of the disparity head's distribution (rag_amd/csrc/disp.hip, the STATS instantiations): variance, peak and entropy
of the softmin over the upsampled cost, written by the launch that writes the disparity.

Rows.  The head table of test_stereo_ends_sweep.py (white noise: every path, fp32 and bf16, partial tiles, the padded grid, odd depths,
the other output sizes) plus five PEAKED rows, cost = c (z - t)^2 + 0.05 N(0, 1) with t ~ U(0, d - 1) per coarse pixel: |cost| reaches
1e4 and the variance is a few px^2, like a trained network's.  On white noise (variance in the thousands) any variance formula passes;
on the peaked rows the raw moment sum p k^2 - disp^2 does not (test_raw_moment_variance_misses_the_gate keeps it that way).

References: rag_amd.metrics.disp_stats_torch (F.interpolate -> softmin -> the four definitions, centred second moment) on the CPU in
float64, tied to oracle.matching_oracle.disp_head by test_twin_fp64_matches_oracle; the same twin in float32 is the yardstick.

Gates.  The disparity of a statistics launch is compared bit for bit with the plain launch's.  Each statistics plane is gated per row at
e_kernel <= 4 e_yard + 1e-6 max|ref64| (the factor and the floor test_stereo_ends_sweep.py applies to this kernel family: hardware exp2,
fused lerps, summation order).  Every GPU case prints `STATS case=... plane=... e_kernel=... e_yard=... bound=...`.

Worst figures of the sweep on the MI355X are in DESIGN.md (section 4.8)."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from oracle import matching_oracle as O
from test_stereo_ends_sweep import DISP_ROWS, _cost_of, _path_of

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
NOISE, FLOOR = 4.0, 1e-6
PLANES = ("variance", "peak", "entropy")

# (B, d, h, w, maxdisp, Ho, Wo, c, dtype, path): the layout of DISP_ROWS with the curvature c of the parabola in the scale column
PEAKED_ROWS = (
    (1, 64, 8, 23, 192, 24, 69, 0.5, F32, "tiled_reg"),
    (1, 64, 8, 23, 192, 24, 69, 4.0, F32, "tiled_reg"),
    (1, 65, 3, 11, 195, 9, 33, 1.0, F32, "tiled_roll"),
    (1, 8, 4, 6, 23, 12, 18, 2.0, F32, "generic"),
    (1, 7, 6, 13, 21, 18, 39, 2.0, F32, "tiled_roll"),
)
ROWS = tuple(("noise",) + r for r in DISP_ROWS) + tuple(("peaked",) + r for r in PEAKED_ROWS)


def _id(case):
    kind, row = case[0], case[1:]
    return "{}_B{}d{}_{}x{}_D{}_{}x{}_s{}_{}_{}".format(kind, *row[:8], "bf16" if row[8] == BF16 else "f32", row[9])


def _peaked_cost(row):
    B, d, h, w, _m, _ho, _wo, c, dtype, _p = row
    g = torch.Generator().manual_seed(9200 + PEAKED_ROWS.index(row))
    t = torch.rand((B, 1, h, w), generator=g) * (d - 1)
    z = torch.arange(d, dtype=torch.float32).view(1, d, 1, 1)
    return (c * (z - t) ** 2 + 0.05 * torch.randn((B, d, h, w), generator=g)).to(dtype)


@functools.lru_cache(maxsize=None)
def _case(case):
    """(cost in the row's dtype, (disp, stats) of the float64 twin, (disp, stats) of the float32 twin), computed once per module."""
    from rag_amd.metrics import disp_stats_torch
    kind, row = case[0], case[1:]
    cost = _cost_of(row) if kind == "noise" else _peaked_cost(row)
    maxdisp, Ho, Wo = row[4:7]
    return cost, disp_stats_torch(cost.double(), maxdisp, (Ho, Wo)), disp_stats_torch(cost.float(), maxdisp, (Ho, Wo))


def _bounds(case):
    """Per plane (e_yard, bound) of the row."""
    _cost, (_d64, ref), (_d32, yard) = _case(case)
    out = []
    for p in range(3):
        e_yard = float((yard[:, p].double() - ref[:, p]).abs().max())
        out.append((e_yard, NOISE * e_yard + FLOOR * float(ref[:, p].abs().max())))
    return out


@pytest.fixture(scope="session")
def built_lib():
    import rag_amd
    if not os.path.exists(rag_amd.lib_path()):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return rag_amd.load_library()


# ====================================================================================================== without a GPU
def test_rows_reach_every_path():
    for r in PEAKED_ROWS:
        assert _path_of(r) == r[9], r
    assert {r[9] for r in PEAKED_ROWS} == {"tiled_reg", "tiled_roll", "generic"}
    assert len(ROWS) == len(DISP_ROWS) + 5 and len(set(ROWS)) == len(ROWS)


def test_twin_fp64_matches_oracle():
    """The twin's disparity in float64 == oracle.matching_oracle.disp_head run in float64 (the tie of test_disp_twin_fp64_matches_oracle)."""
    for case in (("noise", 1, 7, 6, 13, 21, 18, 39, 30.0, F32, "tiled_roll"), ("peaked",) + PEAKED_ROWS[4]):
        cost, (disp, _stats), _yard = _case(case)
        want = O.disp_head(cost.double()[:, None], case[5])
        assert want.dtype == torch.float64 and float((disp - want).abs().max()) <= 1e-12 * case[5], case


@pytest.mark.parametrize("case", ROWS, ids=_id)
def test_row_fp64_statistics_are_in_range(case):
    _cost, (disp, st), (_d32, yard) = _case(case)
    maxdisp = case[5]
    assert torch.isfinite(disp).all() and torch.isfinite(st).all() and torch.isfinite(yard).all()
    var, peak, ent = st[:, 0], st[:, 1], st[:, 2]
    assert float(var.min()) >= 0.0
    assert 0.0 <= float(peak.min()) and float(peak.max()) <= 1.0
    assert float(ent.min()) >= 0.0 and float(ent.max()) <= math.log(maxdisp) + 1e-12
    for name, (e_yard, bound) in zip(PLANES, _bounds(case)):
        print(f"STATS-CPU case={_id(case)} plane={name} e_yard={e_yard:.3e} bound={bound:.3e}")
        assert bound > 0.0


@pytest.mark.parametrize("row", PEAKED_ROWS, ids=lambda r: _id(("peaked",) + r))
def test_raw_moment_variance_misses_the_gate(row):
    """The variance gate is not vacuous: on every peaked row the float32 raw moment sum p k^2 - disp^2 (on ATen's own float32
    distribution) is further from float64 than the row's bound allows."""
    import torch.nn.functional as F
    case = ("peaked",) + row
    cost, (_d64, ref), _yard = _case(case)
    maxdisp, Ho, Wo = row[4:7]
    p = F.softmin(F.interpolate(cost.float()[:, None], (maxdisp, Ho, Wo), mode="trilinear", align_corners=False)[:, 0], dim=1)
    k = torch.arange(maxdisp, dtype=torch.float32).view(1, -1, 1, 1)
    raw = (p * k * k).sum(1) - (p * k).sum(1) ** 2
    e_raw = float((raw.double() - ref[:, 0]).abs().max())
    e_yard, bound = _bounds(case)[0]
    print(f"STATS-CPU case={_id(case)} raw-moment e_raw={e_raw:.3e} e_yard={e_yard:.3e} bound={bound:.3e} var_max={float(ref[:, 0].max()):.3e}")
    assert e_raw > bound, (e_raw, bound)


FAKE = ctypes.c_void_p(0x1000)


def test_abi_refuses_before_launch(built_lib):
    """Status and text of the refusals of both entry points; no pointer is dereferenced (no launch happens)."""
    lib = built_lib

    def fused(cost=FAKE, out=FAKE, stats=FAKE, B=1, d=8, h=4, w=6, maxdisp=24, Ho=12, Wo=18, dtype=0):
        return lib.ragmi_disp_softargmin_stats_fwd(cost, out, stats, B, d, h, w, maxdisp, Ho, Wo, dtype, None), lib.ragmi_last_error()

    def reg(prob=FAKE, out=FAKE, stats=FAKE, B=1, D=8, H=4, W=6, dtype=0):
        return lib.ragmi_disparity_regression_stats_fwd(prob, out, stats, B, D, H, W, dtype, None), lib.ragmi_last_error()

    for fn, who, ptrs in ((fused, b"disp_softargmin_stats", ("cost", "out", "stats")), (reg, b"disparity_regression_stats", ("prob", "out", "stats"))):
        for name in ptrs:
            st, msg = fn(**{name: None})
            assert st == -1 and who + b": null pointer" in msg, (who, name)
        st, msg = fn(dtype=7)
        assert st == -2 and who + b": dtype 7 not built" in msg
        st, msg = fn(B=65536)
        assert st == -2 and who in msg and b"too large" in msg
    for name in ("B", "d", "h", "w", "maxdisp", "Ho", "Wo"):
        for v in (0, -1):
            st, msg = fused(**{name: v})
            assert st == -1 and b"disp_softargmin_stats: non-positive size" in msg, (name, v)
    for name in ("B", "D", "H", "W"):
        for v in (0, -1):
            st, msg = reg(**{name: v})
            assert st == -1 and b"disparity_regression_stats: non-positive size" in msg, (name, v)
    st, msg = fused(maxdisp=4097)
    assert st == -2 and b"maxdisp 4097 exceeds the tap table (4096)" in msg
    st, msg = fused(h=1 << 15, w=1 << 15)
    assert st == -2 and b"disp_softargmin_stats: size too large" in msg


def test_symbols_are_declared_bound_and_exported(built_lib):
    import rag_amd
    from rag_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "rag_amd.h")).read()
    for name in ("ragmi_disp_softargmin_stats_fwd", "ragmi_disparity_regression_stats_fwd"):
        assert name + "(" in header and name in SIGNATURES and hasattr(built_lib, name), name
    assert "rag_model.py:18-44" in header
    assert rag_amd.DispStats is rag_amd.metrics.DispStats and "DispStats" in rag_amd.__all__
    st = rag_amd.DispStats(torch.zeros(2, 3, 4), torch.arange(2 * 3 * 3 * 4.0).view(2, 3, 3, 4))
    assert torch.equal(st.variance, st.tensor[:, 0]) and torch.equal(st.peak, st.tensor[:, 1]) and torch.equal(st.entropy, st.tensor[:, 2])
    assert st.disp.shape == (2, 3, 4) and torch.equal(st["entropy"], st.entropy)


def test_ops_refuse_cpu_tensors(built_lib):
    from rag_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disp_softargmin_stats(torch.zeros(1, 1, 8, 4, 6), 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disparity_regression_stats(torch.zeros(1, 24, 4, 6), 24)


def test_forward_stats_refuses_autograd():
    import rag_amd
    cost = torch.zeros(1, 1, 8, 4, 6, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.Disp(24).forward_stats(cost)
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.DisparityRegression(24).forward_stats(torch.zeros(1, 24, 4, 6, requires_grad=True))
    fea = torch.zeros(1, 12, 8, 12, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.MatchingNet(rag_amd.ALL_SKIP_GENOTYPE, 24).eval().forward_stats(fea, fea.detach())
    img = torch.zeros(1, 3, 24, 36, requires_grad=True)
    net = rag_amd.Network(rag_amd.ALL_SKIP_GENOTYPE, "cpu", maxdisp=24).eval()
    with pytest.raises(RuntimeError, match="inference only"):
        net.forward_stats(img, img.detach(), 0)
    with pytest.raises(RuntimeError, match="inference only"):
        net.search_forward_stats(img.detach(), img, 0, [0] * 18)
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.checkpoint.MultiTaskStereo(net, [net.arch_init]).forward_stats(img, img.detach(), 0)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):      # under no_grad the call goes on, to the GPU-only ops
        rag_amd.Disp(24).forward_stats(cost)


def test_depth_network_has_no_forward_stats():
    """The depth tree inherits from the stereo Network but its sigmoid head has no distribution: the two methods say so."""
    import rag_amd
    for name in ("forward_stats", "search_forward_stats"):
        with pytest.raises(NotImplementedError, match="no distribution"):
            getattr(rag_amd.depth.Network, name)(None)


# ====================================================================================================== on the MI355X
def gpu(t):
    return t.to(DEV)


def _launch(cost, maxdisp, Ho, Wo, out=None, stats=None):
    """ops.disp_softargmin_stats where it applies (Ho = 3 h, Wo = 3 w), the C ABI directly at the other output sizes -> (out, stats)."""
    from rag_amd import _lib as L, ops
    B, d, h, w = cost.shape
    if (Ho, Wo) == (3 * h, 3 * w):
        return ops.disp_softargmin_stats(cost, maxdisp, out, stats)
    out = torch.empty((B, Ho, Wo), device=cost.device, dtype=torch.float32) if out is None else out
    stats = torch.empty((B, 3, Ho, Wo), device=cost.device, dtype=torch.float32) if stats is None else stats
    L.check(L.load_library().ragmi_disp_softargmin_stats_fwd(cost.data_ptr(), out.data_ptr(), stats.data_ptr(), B, d, h, w, maxdisp, Ho, Wo,
                                                             ops._DT[cost.dtype], ops._stream()), "disp_softargmin_stats")
    return out, stats


def _plain(cost, maxdisp, Ho, Wo):
    from rag_amd import _lib as L, ops
    B, d, h, w = cost.shape
    if (Ho, Wo) == (3 * h, 3 * w):
        return ops.disp_softargmin(cost, maxdisp)
    out = torch.empty((B, Ho, Wo), device=cost.device, dtype=torch.float32)
    L.check(L.load_library().ragmi_disp_softargmin_fwd(cost.data_ptr(), out.data_ptr(), B, d, h, w, maxdisp, Ho, Wo, ops._DT[cost.dtype],
                                                       ops._stream()), "disp_softargmin")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROWS, ids=_id)
def test_disparity_is_bitwise_unchanged_and_launch_deterministic(case):
    cost = gpu(_case(case)[0]).contiguous()
    maxdisp, Ho, Wo = case[5:8]
    out, stats = _launch(cost, maxdisp, Ho, Wo)
    again, stats2 = _launch(cost, maxdisp, Ho, Wo)
    plain = _plain(cost, maxdisp, Ho, Wo)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and stats.dtype == torch.float32 and stats.shape == (cost.shape[0], 3, Ho, Wo)
    assert torch.equal(out, plain)
    assert torch.equal(out, again) and torch.equal(stats, stats2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROWS, ids=_id)
def test_statistics_vs_fp64(case):
    cost, (_d64, ref), _yard = _case(case)
    maxdisp, Ho, Wo = case[5:8]
    _out, stats = _launch(gpu(cost).contiguous(), maxdisp, Ho, Wo)
    got = stats.cpu().double()
    assert torch.isfinite(got).all()
    assert float(got[:, 0].min()) >= 0.0 and float(got[:, 1].min()) >= 0.0 and float(got[:, 1].max()) <= 1.0 and float(got[:, 2].min()) >= 0.0
    failed = []
    for p, (name, (e_yard, bound)) in enumerate(zip(PLANES, _bounds(case))):
        e_kernel = float((got[:, p] - ref[:, p]).abs().max())
        print(f"STATS case={_id(case)} plane={name} e_kernel={e_kernel:.3e} e_yard={e_yard:.3e} bound={bound:.3e}")
        if not e_kernel <= bound:
            failed.append((name, e_kernel, e_yard, bound))
    assert not failed, failed


# ---- the standalone DisparityRegression form
REG_SHAPES = tuple((D, H, W) for D in (1, 3, 192) for (H, W) in ((1, 1), (15, 17), (1, 257)))


@functools.lru_cache(maxsize=None)
def _prob(D, H, W, kind):
    g = torch.Generator().manual_seed(9300 + 7 * D + H * W)
    B = 2
    if kind == "zero":
        return torch.zeros((B, D, H, W))
    if kind == "onehot":
        idx = torch.randint(0, D, (B, 1, H, W), generator=g)
        return torch.zeros((B, D, H, W)).scatter_(1, idx, 1.0)
    p = torch.softmax(torch.randn((B, D, H, W), generator=g) * 3.0, dim=1)
    return p.to(BF16) if kind == "bf16" else p          # bf16 storage: the rounded values, no longer summing to 1, are taken as given


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("f32", "bf16", "zero", "onehot"))
@pytest.mark.parametrize("shape", REG_SHAPES, ids=lambda s: "D{}_{}x{}".format(*s))
def test_regression_stats(shape, kind):
    from rag_amd import ops
    from rag_amd.metrics import prob_stats_torch
    D, H, W = shape
    prob = _prob(D, H, W, kind)
    dev = gpu(prob).contiguous()
    out, stats = ops.disparity_regression_stats(dev, D)
    again, stats2 = ops.disparity_regression_stats(dev, D)
    plain = ops.disparity_regression(dev, D)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(out, again) and torch.equal(stats, stats2)
    _d64, ref = prob_stats_torch(prob.double())
    _d32, yard = prob_stats_torch(prob.float())
    got = stats.cpu().double()
    assert stats.shape == (2, 3, H, W) and torch.isfinite(got).all()
    failed = []
    for p, name in enumerate(PLANES):
        e_kernel = float((got[:, p] - ref[:, p]).abs().max())
        e_yard = float((yard[:, p].double() - ref[:, p]).abs().max())
        bound = NOISE * e_yard + FLOOR * float(ref[:, p].abs().max())
        print(f"STATS case=reg_{kind}_D{D}_{H}x{W} plane={name} e_kernel={e_kernel:.3e} e_yard={e_yard:.3e} bound={bound:.3e}")
        if not e_kernel <= bound:
            failed.append((name, e_kernel, e_yard, bound))
    assert not failed, failed
    if kind == "zero":
        assert not stats.any() and not out.any()
    if kind == "onehot":
        assert not stats[:, 0].any() and not stats[:, 2].any() and bool((stats[:, 1] == 1.0).all())


# ---- no stray writes
STRAY_ROWS = (
    ("noise", 3, 64, 9, 11, 192, 27, 33, 1.0, F32, "tiled_reg"),            # the last tile column is one pixel wide
    ("noise", 1, 7, 6, 13, 21, 18, 39, 30.0, F32, "tiled_roll"),
    ("noise", 1, 8, 4, 6, 23, 12, 18, 1.0, F32, "generic"),
)


@pytest.mark.gpu
@pytest.mark.parametrize("case", STRAY_ROWS, ids=_id)
def test_no_stray_writes(case):
    assert case in ROWS
    cost = gpu(_case(case)[0]).contiguous()
    B, maxdisp, Ho, Wo = case[1], case[5], case[6], case[7]
    n, pad, sentinel = B * Ho * Wo, 256, -12345.0
    big_o = torch.full((n + 2 * pad + 1,), sentinel, device=DEV)
    big_s = torch.full((3 * n + 2 * pad + 1,), sentinel, device=DEV)
    out = big_o[pad + 1:pad + 1 + n].view(B, Ho, Wo)                        # offset by one float from the allocation's alignment
    stats = big_s[pad + 1:pad + 1 + 3 * n].view(B, 3, Ho, Wo)
    got_o, got_s = _launch(cost, maxdisp, Ho, Wo, out, stats)
    ref_o, ref_s = _launch(cost, maxdisp, Ho, Wo)
    torch.cuda.synchronize()
    assert got_o.data_ptr() == out.data_ptr() and got_s.data_ptr() == stats.data_ptr()
    assert torch.equal(out, ref_o) and torch.equal(stats, ref_s)
    for big, m in ((big_o, n), (big_s, 3 * n)):
        assert bool((big[:pad + 1] == sentinel).all()) and bool((big[pad + 1 + m:] == sentinel).all())
    assert not bool((out == sentinel).any()) and not bool((stats == sentinel).any())


# ---- model level: smoke's shape (maxdisp 48, B = 2, 16 x 28 features)
def _images():
    g = torch.Generator().manual_seed(77)
    return gpu(torch.rand((2, 3, 48, 84), generator=g)), gpu(torch.rand((2, 3, 48, 84), generator=g))


def _same(res, disp, cost, maxdisp):
    import rag_amd
    from rag_amd import ops
    assert isinstance(res, rag_amd.DispStats)
    want_d, want_s = ops.disp_softargmin_stats(cost, maxdisp)
    assert torch.equal(res.disp, disp) and torch.equal(res.disp, want_d) and torch.equal(res.tensor, want_s)
    assert res.tensor.shape == (disp.shape[0], 3) + tuple(disp.shape[1:]) and torch.isfinite(res.tensor).all()
    assert torch.equal(res.variance, res.tensor[:, 0]) and torch.equal(res.peak, res.tensor[:, 1]) and torch.equal(res.entropy, res.tensor[:, 2])


@pytest.mark.gpu
def test_model_forward_stats():
    import rag_amd
    from rag_amd import checkpoint as ck
    from test_host_cpu import _grown_network
    left, right = _images()
    net, archis = _grown_network()
    net = net.to(DEV).eval()
    serve = ck.MultiTaskStereo(net, archis)
    with torch.no_grad():
        for t in (0, 1):
            lf, rf = net._features(left, right, lambda x: net.feature(x, archis[t], None))
            cost = net.matching(None, archis[t], None, features=(lf, rf))
            _same(net.forward_stats(left, right, t, archis[t]), net(left, right, t, archis[t]), cost, net.maxdisp)
            _same(serve.forward_stats(left, right, t), serve(left, right, t), cost, net.maxdisp)
    res = net.forward_stats(left, right, 1, archis[1])              # grad mode on, parameters that require grad: still the inference path
    with torch.no_grad():
        assert torch.equal(res.disp, net(left, right, 1, archis[1])) and not res.tensor.requires_grad
    # the expanded supermodel: every layer has a candidate
    torch.manual_seed(6)
    sup = rag_amd.Network(rag_amd.ALL_CONV_GENOTYPE, "cpu", maxdisp=48)
    sup.expand(1, rag_amd.ALL_CONV_GENOTYPE, "cpu")
    sup = sup.to(DEV).eval()
    sel = [0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0]
    with torch.no_grad():
        lf, rf = sup._features(left, right, lambda x: sup.search_feature(x, sel))
        cost = sup.search_matching(None, sel, 1, features=(lf, rf))
        _same(sup.search_forward_stats(left, right, 1, sel), sup.search_forward(left, right, 1, sel), cost, sup.maxdisp)


def _matching_net():
    import numpy as np
    import rag_amd
    rows = np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]])
    net = rag_amd.MatchingNet(rag_amd.Genotype(normal=rows, normal_concat=None, reduce=rows, reduce_concat=None), maxdisp=48)
    net.load_state_dict(O.random_matching_state_dict(rows, seed=0), strict=True)
    g = torch.Generator().manual_seed(1234)
    return net.to(DEV).eval(), gpu(torch.randn((2, 12, 16, 28), generator=g)), gpu(torch.randn((2, 12, 16, 28), generator=g))


@pytest.mark.gpu
def test_matchingnet_forward_stats():
    net, lf, rf = _matching_net()
    with torch.no_grad():
        cost = net.matching(None, net.arch_init, None, features=(lf, rf))
        _same(net.forward_stats(lf, rf), net(lf, rf), cost, net.maxdisp)
        _same(net.disp.forward_stats(cost), net.disp(cost), cost, net.maxdisp)


@pytest.mark.gpu
def test_forward_stats_is_graph_capturable():
    """One MatchingNet.forward_stats with caller-owned outputs as a captured graph: kernel nodes only, and a replay on new input bytes
    gives the eager result bit for bit."""
    from rag_amd.train import graph_census
    net, lf, rf = _matching_net()
    out = torch.empty((2, 48, 84), device=DEV)
    stats = torch.empty((2, 3, 48, 84), device=DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net.forward_stats(lf, rf, out=out, stats=stats)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            res = net.forward_stats(lf, rf, out=out, stats=stats)
        census = graph_census(graph)
        graph.instantiate()
        assert res.disp.data_ptr() == out.data_ptr() and res.tensor.data_ptr() == stats.data_ptr()
        g = torch.Generator().manual_seed(4321)
        new_l, new_r = gpu(torch.randn((2, 12, 16, 28), generator=g)), gpu(torch.randn((2, 12, 16, 28), generator=g))
        lf.copy_(new_l)
        rf.copy_(new_r)
        graph.replay()
        torch.cuda.synchronize()
        eager = net.forward_stats(new_l, new_r)
        torch.cuda.synchronize()
    assert census["memcpy"] == 0 and census["memset"] == 0 and census["kernel"] > 0, census
    assert torch.equal(out, eager.disp) and torch.equal(stats, eager.tensor)
