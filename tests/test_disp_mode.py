"""Mode-local disparity of the disparity head (rag_amd/csrc/disp.hip, the MODE instantiations): the fine index k* of the smallest upsampled
cost, the disparity regressed over the window |k - k*| <= r about k*, and the probability mass of that window, written by the launch that
writes the disparity and its statistics.

Rows.  ROWS of test_disp_stats.py (every dispatch path, fp32 and bf16, partial tiles, the padded grid, d in {1, 2, 7, 63, 64, 65, 213},
the other output sizes, the five peaked rows) plus three END rows: PEAKED_ROWS' parabola c (z - t)^2 + 0.05 N(0, 1) with the well forced,
coarse pixel by coarse pixel in turn, to t = 0, t = d - 1 and t = 0.5, so that every one of the three shapes clips the window at both ends
and has plane 0 and plane 1 in a near tie.  Radii {0, 1, 4, maxdisp} on every row; the definition has 0 <= r <= maxdisp, and on the two
rows with maxdisp = 3 a radius of 4 covers the whole axis exactly as 3 does, so there it runs as min(4, maxdisp).

References: rag_amd.metrics.disp_mode_torch on the CPU in float64, tied to oracle.matching_oracle.disp_head and to disp_stats_torch by
test_twin_fp64_matches_oracle_and_stats_twin; the same twin in float32 is the yardstick.

The arg-min.  Two fine costs closer than fp32 rounding have no arg-min that two arithmetics agree on, so an index is compared with the
CANDIDATE SET of the float64 reference, C = {k : v64_k - min v64 <= gap}, gap = 2^-20 max|cost| of the row: 16 units of fp32 rounding at
the row's largest magnitude (three nested two-tap lerps, at most 2 roundings each, on both samples compared = 12, rounded up).  The values
are then compared with both twins evaluated about the KERNEL's index (index=), so no pixel is excluded from any comparison.

Gates.  out and stats of a mode launch are compared bit for bit with the plain and the statistics launches.  The disp and mass planes are
gated per row and radius at e_kernel <= 4 e_yard + 1e-6 max|ref64| (1e-6 maxdisp for the disp plane), the factor and floor
test_disp_stats.py applies to this kernel family.  Every GPU case prints `MODE case=... r=... plane=... e_kernel=... e_yard=... bound=...`.

Worst figures of the sweep on the MI355X are in DESIGN.md (section 4.8.2)."""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from oracle import matching_oracle as O
from test_disp_stats import (BF16, DEV, F32, FLOOR, NOISE, PEAKED_ROWS, REG_SHAPES, STRAY_ROWS, _id, _images, _matching_net, _peaked_cost,
                             _prob, built_lib, gpu)  # noqa: F401  (built_lib is a fixture)
from test_disp_stats import ROWS as STATS_ROWS
from test_stereo_ends_sweep import _cost_of, _path_of

MODE_PLANES = ("index", "disp", "mass")
RADII = (0, 1, 4, "maxdisp")

# (B, d, h, w, maxdisp, Ho, Wo, c, dtype, path): the layout of PEAKED_ROWS
END_ROWS = (
    (1, 64, 1, 10, 192, 3, 30, 0.5, F32, "tiled_reg"),
    (1, 7, 5, 1, 21, 15, 3, 2.0, F32, "tiled_roll"),
    (1, 8, 4, 6, 23, 12, 18, 2.0, F32, "generic"),
)
ROWS = STATS_ROWS + tuple(("end",) + r for r in END_ROWS)
CASES = tuple((case, r) for case in ROWS for r in RADII)


def _radius(case, r):
    maxdisp = case[5]
    return maxdisp if r == "maxdisp" else min(r, maxdisp)


def _cid(cr):
    return f"{_id(cr[0])}-r{cr[1]}"


def _end_cost(row):
    B, d, h, w, _m, _ho, _wo, c, dtype, _p = row
    g = torch.Generator().manual_seed(9400 + END_ROWS.index(row))
    wells = torch.tensor([0.0, d - 1.0, 0.5])
    t = wells[torch.arange(B * h * w) % 3].view(B, 1, h, w)
    z = torch.arange(d, dtype=torch.float32).view(1, d, 1, 1)
    return (c * (z - t) ** 2 + 0.05 * torch.randn((B, d, h, w), generator=g)).to(dtype)


@functools.lru_cache(maxsize=None)
def _cost(case):
    kind, row = case[0], case[1:]
    return _cost_of(row) if kind == "noise" else _peaked_cost(row) if kind == "peaked" else _end_cost(row)


@functools.lru_cache(maxsize=None)
def _v64(case):
    """(the upsampled cost in float64 [B,maxdisp,Ho,Wo], the gap of the row's candidate sets), computed once per module."""
    cost = _cost(case)
    maxdisp, Ho, Wo = case[5:8]
    v = F.interpolate(cost.double()[:, None], (maxdisp, Ho, Wo), mode="trilinear", align_corners=False)[:, 0]
    return v, 2.0 ** -20 * float(cost.double().abs().max())


@functools.lru_cache(maxsize=None)
def _twins(case, radius):
    """((disp, stats, mode) of the float64 twin, the same of the float32 twin), each about its own arg-min."""
    from rag_amd.metrics import disp_mode_torch
    cost = _cost(case)
    maxdisp, Ho, Wo = case[5:8]
    return disp_mode_torch(cost.double(), maxdisp, radius, (Ho, Wo)), disp_mode_torch(cost.float(), maxdisp, radius, (Ho, Wo))


def _in_candidates(case, index):
    """Per pixel: does index [B,Ho,Wo] lie in C = {k : v64_k - min v64 <= gap}?"""
    v, gap = _v64(case)
    at = v.gather(1, index.long()[:, None])[:, 0]
    return (at - v.amin(1)) <= gap


# ====================================================================================================== without a GPU
def test_rows_and_radii():
    for r in END_ROWS:
        assert _path_of(r) == r[9], r
    assert {r[9] for r in END_ROWS} == {"tiled_reg", "tiled_roll", "generic"}
    assert [r[:7] for r in END_ROWS] == [(1, 64, 1, 10, 192, 3, 30), (1, 7, 5, 1, 21, 15, 3), (1, 8, 4, 6, 23, 12, 18)]
    assert len(ROWS) == len(STATS_ROWS) + 3 and len(set(ROWS)) == len(ROWS) and len(CASES) == 4 * len(ROWS)
    for case in ROWS:
        rs = [_radius(case, r) for r in RADII]
        assert rs[0] == 0 and rs[-1] == case[5] and all(0 <= r <= case[5] for r in rs)
        assert rs[:3] == [0, 1, 4] or case[5] < 4
    assert sum(1 for case in ROWS if case[5] < 4) == 2          # the two maxdisp = 3 rows: radius 4 is the whole axis, as 3 is
    for row in END_ROWS:            # every shape holds all three wells, and a well at 0.5 makes planes 0 and 1 a near tie
        cost = _end_cost(row)
        first = cost.argmin(1).flatten().tolist()
        assert 0 in first and row[1] - 1 in first
        near = (cost[:, 0] - cost[:, 1]).abs().flatten()[2::3]
        assert float(near.max()) < 0.5 and len(near) >= 1


def test_twin_fp64_matches_oracle_and_stats_twin():
    from rag_amd.metrics import disp_stats_torch
    for case in (("noise", 1, 7, 6, 13, 21, 18, 39, 30.0, F32, "tiled_roll"), ("peaked",) + PEAKED_ROWS[4], ("end",) + END_ROWS[1]):
        maxdisp, Ho, Wo = case[5:8]
        for r in RADII:
            (disp, stats, mode), _yard = _twins(case, _radius(case, r))
            want = O.disp_head(_cost(case).double()[:, None], maxdisp)
            assert want.dtype == torch.float64 and float((disp - want).abs().max()) <= 1e-12 * maxdisp, case
            d2, s2 = disp_stats_torch(_cost(case).double(), maxdisp, (Ho, Wo))
            assert torch.equal(disp, d2) and torch.equal(stats, s2)
            assert mode.shape == (case[1], 3, Ho, Wo) and mode.dtype == torch.float64


@pytest.mark.parametrize("case", ROWS, ids=_id)
def test_identities_fp64(case):
    maxdisp = case[5]
    for r in RADII:
        radius = _radius(case, r)
        (disp, stats, mode), _yard = _twins(case, radius)
        index, mdisp, mass = mode[:, 0], mode[:, 1], mode[:, 2]
        assert torch.isfinite(mode).all()
        assert torch.equal(index, index.round()) and float(index.min()) >= 0 and float(index.max()) <= maxdisp - 1
        assert float(mass.min()) >= 0.0 and float(mass.max()) <= 1.0 + 1e-12
        assert float((mdisp - index).abs().max()) <= radius
        if radius == 0:
            assert torch.equal(mdisp, index)
            assert float((mass - stats[:, 1]).abs().max()) <= 1e-12
        if radius == maxdisp:
            assert float((mdisp - disp).abs().max()) <= 1e-9 * maxdisp
            assert float((mass - 1.0).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", ROWS, ids=_id)
def test_fp32_argmin_lies_in_the_fp64_candidate_set(case):
    """The arg-min is well posed for the reference alone: the float32 twin's own k* is a candidate of float64 at every pixel."""
    (_d64, _s64, m64), (_d32, _s32, m32) = _twins(case, 0)
    ok = _in_candidates(case, m32[:, 0])
    differ = float((m32[:, 0].double() != m64[:, 0]).double().mean())
    print(f"MODE-CPU case={_id(case)} gap={_v64(case)[1]:.3e} fp32_vs_fp64_argmin_differ={differ:.4f} outside_C={int((~ok).sum())}")
    assert bool(ok.all())
    assert bool(_in_candidates(case, m64[:, 0]).all())


def test_index_argument_moves_the_window():
    from rag_amd.metrics import disp_mode_torch, prob_mode_torch
    case = ("peaked",) + PEAKED_ROWS[3]
    cost, maxdisp = _cost(case).double(), case[5]
    (_d, _s, own), _y = _twins(case, 1)
    _d, _s, same = disp_mode_torch(cost, maxdisp, 1, (case[6], case[7]), index=own[:, 0].float())       # any dtype holding the integers
    assert torch.equal(same, own)
    at = torch.full_like(own[:, 0], 5.0)
    _d, _s, moved = disp_mode_torch(cost, maxdisp, 1, (case[6], case[7]), index=at)
    p = F.softmin(_v64(case)[0], dim=1)
    assert torch.equal(moved[:, 0], at) and torch.allclose(moved[:, 2], p[:, 4:7].sum(1), rtol=0, atol=1e-15)
    prob = torch.tensor([0.0, 0.5, 0.0, 0.5, 0.0]).view(1, 5, 1, 1)
    _d, _s, m = prob_mode_torch(prob, 1)
    assert m.flatten().tolist() == [1.0, 1.0, 0.5]                         # the FIRST arg-max
    _d, _s, m = prob_mode_torch(prob, 1, index=torch.tensor([[[4]]]))
    assert m.flatten().tolist() == [4.0, 4.0 - 1.0, 0.5]                   # clipped at the end: {3, 4}
    _d, _s, m = prob_mode_torch(torch.zeros(1, 5, 1, 1), 2)
    assert m.flatten().tolist() == [0.0, 0.0, 0.0]                         # no mass: mode_disp = k*
    with pytest.raises(ValueError, match="radius"):
        prob_mode_torch(prob, 6)
    with pytest.raises(ValueError, match="radius"):
        prob_mode_torch(prob, -1)


def test_edge_bleeding_fp64():
    """The reason for the feature: two wells per pixel.  The mean lies on neither surface, the mode-local disparity on the stronger one,
    and the mass says that the window does not speak for the whole distribution."""
    from rag_amd.metrics import MODE_RADIUS, disp_mode_torch
    assert MODE_RADIUS == 4
    z = torch.arange(64, dtype=torch.float64).view(1, 64, 1, 1)
    cost = torch.minimum(4 * (z - 10) ** 2, 4 * (z - 40) ** 2 + 0.5).expand(1, 64, 3, 3).contiguous()
    disp, _stats, mode = disp_mode_torch(cost, 192, 4)
    assert mode.dtype == torch.float64 and bool((mode[:, 0] == 31).all())
    print(f"MODE-CPU edge: disp={float(disp.mean()):.3f} mode_disp={float(mode[:, 1].mean()):.3f} mode_mass={float(mode[:, 2].mean()):.3f}")
    assert float((mode[:, 1] - 31).abs().max()) <= 0.5
    assert float((disp - 31).abs().min()) >= 10
    assert float(mode[:, 2].max()) < 0.9


FAKE = ctypes.c_void_p(0x1000)


def test_abi_refuses_before_launch(built_lib):
    """Status and text of the refusals of both entry points; no pointer is dereferenced (no launch happens)."""
    lib = built_lib

    def fused(cost=FAKE, out=FAKE, stats=FAKE, mode=FAKE, B=1, d=8, h=4, w=6, maxdisp=24, Ho=12, Wo=18, radius=4, dtype=0):
        return lib.ragmi_disp_softargmin_mode_fwd(cost, out, stats, mode, B, d, h, w, maxdisp, Ho, Wo, radius, dtype, None), lib.ragmi_last_error()

    def reg(prob=FAKE, out=FAKE, stats=FAKE, mode=FAKE, B=1, D=8, H=4, W=6, radius=4, dtype=0):
        return lib.ragmi_disparity_regression_mode_fwd(prob, out, stats, mode, B, D, H, W, radius, dtype, None), lib.ragmi_last_error()

    for fn, who, ptrs, top in ((fused, b"disp_softargmin_mode", ("cost", "out", "stats", "mode"), 24),
                               (reg, b"disparity_regression_mode", ("prob", "out", "stats", "mode"), 8)):
        for name in ptrs:
            st, msg = fn(**{name: None})
            assert st == -1 and who + b": null pointer" in msg, (who, name)
        for radius in (-1, top + 1, 1 << 30):
            st, msg = fn(radius=radius)
            assert st == -1 and who + b": radius" in msg, (who, radius)
        st, msg = fn(dtype=7)
        assert st == -2 and who + b": dtype 7 not built" in msg
        st, msg = fn(B=65536)
        assert st == -2 and who in msg and b"too large" in msg
    for name in ("B", "d", "h", "w", "maxdisp", "Ho", "Wo"):
        for v in (0, -1):
            st, msg = fused(**{name: v})
            assert st == -1 and b"disp_softargmin_mode: non-positive size" in msg, (name, v)
    for name in ("B", "D", "H", "W"):
        for v in (0, -1):
            st, msg = reg(**{name: v})
            assert st == -1 and b"disparity_regression_mode: non-positive size" in msg, (name, v)
    st, msg = fused(maxdisp=4097)
    assert st == -2 and b"maxdisp 4097 exceeds the tap table (4096)" in msg
    st, msg = fused(h=1 << 15, w=1 << 15)
    assert st == -2 and b"disp_softargmin_mode: size too large" in msg


def test_symbols_are_declared_bound_and_exported(built_lib):
    import rag_amd
    from rag_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "rag_amd.h")).read()
    for name, nargs in (("ragmi_disp_softargmin_mode_fwd", 14), ("ragmi_disparity_regression_mode_fwd", 11)):
        assert name + "(" in header and name in SIGNATURES and hasattr(built_lib, name), name
        assert len(SIGNATURES[name][1]) == nargs and getattr(built_lib, name).argtypes == SIGNATURES[name][1]
    assert "rag_model.py:18-44" in header
    assert rag_amd.DispMode is rag_amd.metrics.DispMode and "DispMode" in rag_amd.__all__ and issubclass(rag_amd.DispMode, rag_amd.DispStats)
    assert rag_amd.metrics.MODE_NAMES == MODE_PLANES and rag_amd.metrics.MODE_RADIUS == 4
    res = rag_amd.DispMode(torch.zeros(2, 3, 4), torch.arange(72.0).view(2, 3, 3, 4), torch.arange(72.0, 144.0).view(2, 3, 3, 4), 4)
    assert torch.equal(res.mode_index, res.mode_tensor[:, 0]) and torch.equal(res.mode_disp, res.mode_tensor[:, 1])
    assert torch.equal(res.mode_mass, res.mode_tensor[:, 2]) and res.radius == 4
    assert res.mode_disp.data_ptr() == res.mode_tensor[:, 1].data_ptr()                                  # views, not copies
    assert torch.equal(res["mass"], res.mode_mass) and torch.equal(res["entropy"], res.entropy) and torch.equal(res.variance, res.tensor[:, 0])


def test_ops_refuse_cpu_tensors_and_bad_mode(built_lib):
    from rag_amd import ops
    cost, prob = torch.zeros(1, 1, 8, 4, 6), torch.zeros(1, 24, 4, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disp_softargmin_mode(cost, 24, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disparity_regression_mode(prob, 24, 4)
    bad = (torch.zeros(1, 3, 12, 17), torch.zeros(1, 2, 12, 18), torch.zeros(3, 12, 18), torch.zeros(1, 3, 12, 36)[..., ::2],
           torch.zeros(1, 3, 12, 18, dtype=torch.float64))
    for mode in bad:
        with pytest.raises(ValueError, match="mode must be a contiguous"):
            ops.disp_softargmin_mode(cost, 24, 4, mode=mode)
    for mode in (torch.zeros(1, 3, 4, 7), torch.zeros(1, 3, 6, 4).transpose(2, 3)):
        with pytest.raises(ValueError, match="mode must be a contiguous"):
            ops.disparity_regression_mode(prob, 24, 4, mode=mode)
    for radius in (-1, 25, 1.5):
        with pytest.raises(ValueError, match="radius"):
            ops.disp_softargmin_mode(cost, 24, radius)
        with pytest.raises(ValueError, match="radius"):
            ops.disparity_regression_mode(prob, 24, radius)


def test_forward_mode_refuses_autograd():
    import rag_amd
    cost = torch.zeros(1, 1, 8, 4, 6, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.Disp(24).forward_mode(cost)
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.DisparityRegression(24).forward_mode(torch.zeros(1, 24, 4, 6, requires_grad=True))
    fea = torch.zeros(1, 12, 8, 12, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.MatchingNet(rag_amd.ALL_SKIP_GENOTYPE, 24).eval().forward_mode(fea, fea.detach())
    img = torch.zeros(1, 3, 24, 36, requires_grad=True)
    net = rag_amd.Network(rag_amd.ALL_SKIP_GENOTYPE, "cpu", maxdisp=24).eval()
    with pytest.raises(RuntimeError, match="inference only"):
        net.forward_mode(img, img.detach(), 0)
    with pytest.raises(RuntimeError, match="inference only"):
        net.search_forward_mode(img.detach(), img, 0, [0] * 18)
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.checkpoint.MultiTaskStereo(net, [net.arch_init]).forward_mode(img, img.detach(), 0)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):      # under no_grad the call goes on, to the GPU-only ops
        rag_amd.Disp(24).forward_mode(cost)


def test_depth_network_has_no_forward_mode():
    import rag_amd
    for name in ("forward_mode", "search_forward_mode"):
        with pytest.raises(NotImplementedError, match="no distribution"):
            getattr(rag_amd.depth.Network, name)(None)


# ====================================================================================================== on the MI355X
def _launch(cost, maxdisp, Ho, Wo, radius, out=None, stats=None, mode=None):
    """ops.disp_softargmin_mode where it applies (Ho = 3 h, Wo = 3 w), the C ABI directly at the other output sizes -> (out, stats, mode)."""
    from rag_amd import _lib as L, ops
    B, d, h, w = cost.shape
    if (Ho, Wo) == (3 * h, 3 * w):
        return ops.disp_softargmin_mode(cost, maxdisp, radius, out, stats, mode)
    out = torch.empty((B, Ho, Wo), device=cost.device, dtype=torch.float32) if out is None else out
    stats = torch.empty((B, 3, Ho, Wo), device=cost.device, dtype=torch.float32) if stats is None else stats
    mode = torch.empty((B, 3, Ho, Wo), device=cost.device, dtype=torch.float32) if mode is None else mode
    L.check(L.load_library().ragmi_disp_softargmin_mode_fwd(cost.data_ptr(), out.data_ptr(), stats.data_ptr(), mode.data_ptr(), B, d, h, w, maxdisp,
                                                            Ho, Wo, radius, ops._DT[cost.dtype], ops._stream()), "disp_softargmin_mode")
    return out, stats, mode


def _gate(tag, got, ref, yard, maxdisp):
    """The disp and mass planes of mode tensors [B,3,...] (kernel, float64 twin, float32 twin, all about the same index) -> failures."""
    failed = []
    for p in (1, 2):
        e_kernel = float((got[:, p] - ref[:, p]).abs().max())
        e_yard = float((yard[:, p].double() - ref[:, p]).abs().max())
        bound = NOISE * e_yard + FLOOR * (maxdisp if p == 1 else float(ref[:, p].abs().max()))
        print(f"MODE {tag} plane={MODE_PLANES[p]} e_kernel={e_kernel:.3e} e_yard={e_yard:.3e} bound={bound:.3e}")
        if not e_kernel <= bound:
            failed.append((MODE_PLANES[p], e_kernel, e_yard, bound))
    return failed


@pytest.mark.gpu
@pytest.mark.parametrize("cr", CASES, ids=_cid)
def test_out_and_stats_are_bitwise_the_existing_launches(cr):
    from test_disp_stats import _launch as stats_launch, _plain
    case, radius = cr[0], _radius(*cr)
    cost = gpu(_cost(case)).contiguous()
    maxdisp, Ho, Wo = case[5:8]
    out, stats, mode = _launch(cost, maxdisp, Ho, Wo, radius)
    out2, stats2, mode2 = _launch(cost, maxdisp, Ho, Wo, radius)
    want_o, want_s = stats_launch(cost, maxdisp, Ho, Wo)
    plain = _plain(cost, maxdisp, Ho, Wo)
    torch.cuda.synchronize()
    assert mode.dtype == torch.float32 and mode.shape == (cost.shape[0], 3, Ho, Wo)
    assert torch.equal(out, plain) and torch.equal(out, want_o) and torch.equal(stats, want_s)
    assert torch.equal(out, out2) and torch.equal(stats, stats2) and torch.equal(mode, mode2)


@pytest.mark.gpu
@pytest.mark.parametrize("cr", CASES, ids=_cid)
def test_mode_vs_fp64(cr):
    from rag_amd.metrics import disp_mode_torch
    case, radius = cr[0], _radius(*cr)
    cost = _cost(case)
    maxdisp, Ho, Wo = case[5:8]
    _out, _stats, mode = _launch(gpu(cost).contiguous(), maxdisp, Ho, Wo, radius)
    got = mode.cpu().double()
    assert torch.isfinite(got).all()
    index = got[:, 0]
    assert torch.equal(index, index.round()) and float(index.min()) >= 0 and float(index.max()) <= maxdisp - 1
    ok = _in_candidates(case, index)
    assert bool(ok.all()), f"{int((~ok).sum())} of {ok.numel()} indices outside the float64 candidate set"
    _d, _s, ref = disp_mode_torch(cost.double(), maxdisp, radius, (Ho, Wo), index=index)
    _d, _s, yard = disp_mode_torch(cost.float(), maxdisp, radius, (Ho, Wo), index=index)
    assert torch.equal(ref[:, 0], index) and torch.equal(yard[:, 0].double(), index)
    failed = _gate(f"case={_id(case)} r={radius}", got, ref, yard, maxdisp)
    assert not failed, failed
    assert float((got[:, 1] - index).abs().max()) <= radius
    if radius == 0:
        assert torch.equal(got[:, 1], index)


TIE_SHAPES = ((1, 64, 1, 10, 192, 3, 30), (1, 7, 5, 1, 21, 15, 3), (1, 8, 4, 6, 23, 12, 18))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TIE_SHAPES, ids=lambda s: "d{1}_{2}x{3}_D{4}".format(*s))
def test_exact_ties_take_the_lowest_index(shape):
    """An all-zero cost makes every fine cost an exact tie in the kernel's own arithmetic: k* = 0, and the window of radius 2 holds the
    fine samples 0, 1, 2 of a uniform distribution.  A cost whose only minimum is plane 0 (a ramp) gives k* = 0, not 1: fine samples 0
    and 1 both sit on plane 0."""
    B, d, h, w, maxdisp, Ho, Wo = shape
    _out, _stats, mode = _launch(torch.zeros((B, d, h, w), device=DEV), maxdisp, Ho, Wo, 2)
    got = mode.cpu().double()
    assert not got[:, 0].any()
    assert float((got[:, 1] - 1.0).abs().max()) <= 1e-6 and float((got[:, 2] - 3.0 / maxdisp).abs().max()) <= 1e-6
    if maxdisp == 3 * d:
        ramp = torch.arange(d, dtype=torch.float32).view(1, d, 1, 1).expand(B, d, h, w).contiguous()
        _out, _stats, mode = _launch(gpu(ramp), maxdisp, Ho, Wo, 2)
        assert not mode[:, 0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("f32", "bf16", "zero", "onehot"))
@pytest.mark.parametrize("shape", REG_SHAPES, ids=lambda s: "D{}_{}x{}".format(*s))
def test_regression_mode(shape, kind):
    from rag_amd import ops
    from rag_amd.metrics import prob_mode_torch
    D, H, W = shape
    prob = _prob(D, H, W, kind)
    dev = gpu(prob).contiguous()
    want_o, want_s = ops.disparity_regression_stats(dev, D)
    plain = ops.disparity_regression(dev, D)
    failed = []
    for r in RADII:
        radius = D if r == "maxdisp" else min(r, D)
        out, stats, mode = ops.disparity_regression_mode(dev, D, radius)
        out2, stats2, mode2 = ops.disparity_regression_mode(dev, D, radius)
        torch.cuda.synchronize()
        assert mode.shape == (2, 3, H, W) and mode.dtype == torch.float32
        assert torch.equal(out, plain) and torch.equal(out, want_o) and torch.equal(stats, want_s)
        assert torch.equal(out, out2) and torch.equal(stats, stats2) and torch.equal(mode, mode2)
        got = mode.cpu().double()
        _d, _s, own = prob_mode_torch(prob.float(), radius)
        assert torch.isfinite(got).all() and torch.equal(got[:, 0], own[:, 0].double())         # the first arg-max, exactly
        _d, _s, ref = prob_mode_torch(prob.double(), radius, index=got[:, 0])
        _d, _s, yard = prob_mode_torch(prob.float(), radius, index=got[:, 0])
        failed += _gate(f"case=reg_{kind}_D{D}_{H}x{W} r={radius}", got, ref, yard, D)
        if kind == "zero":
            assert not mode.any()
        if kind == "onehot":
            assert torch.equal(mode[:, 0].cpu(), prob.argmax(1).float()) and torch.equal(mode[:, 1], mode[:, 0]) and bool((mode[:, 2] == 1.0).all())
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize("case", STRAY_ROWS, ids=_id)
def test_no_stray_writes(case):
    """Guard bands around out, stats and mode with r = maxdisp: the generic kernel's second walk runs over both ends of the axis."""
    assert case in ROWS
    cost = gpu(_cost(case)).contiguous()
    B, maxdisp, Ho, Wo = case[1], case[5], case[6], case[7]
    n, pad, sentinel = B * Ho * Wo, 256, -12345.0
    big_o = torch.full((n + 2 * pad + 1,), sentinel, device=DEV)
    big_s = torch.full((3 * n + 2 * pad + 1,), sentinel, device=DEV)
    big_m = torch.full((3 * n + 2 * pad + 1,), sentinel, device=DEV)
    out = big_o[pad + 1:pad + 1 + n].view(B, Ho, Wo)                        # offset by one float from the allocation's alignment
    stats = big_s[pad + 1:pad + 1 + 3 * n].view(B, 3, Ho, Wo)
    mode = big_m[pad + 1:pad + 1 + 3 * n].view(B, 3, Ho, Wo)
    got_o, got_s, got_m = _launch(cost, maxdisp, Ho, Wo, maxdisp, out, stats, mode)
    ref_o, ref_s, ref_m = _launch(cost, maxdisp, Ho, Wo, maxdisp)
    torch.cuda.synchronize()
    assert got_o.data_ptr() == out.data_ptr() and got_s.data_ptr() == stats.data_ptr() and got_m.data_ptr() == mode.data_ptr()
    assert torch.equal(out, ref_o) and torch.equal(stats, ref_s) and torch.equal(mode, ref_m)
    for big, m in ((big_o, n), (big_s, 3 * n), (big_m, 3 * n)):
        assert bool((big[:pad + 1] == sentinel).all()) and bool((big[pad + 1 + m:] == sentinel).all())
    assert not bool((out == sentinel).any()) and not bool((stats == sentinel).any()) and not bool((mode == sentinel).any())


# ---- model level: the small model of test_model_forward_stats
def _same(res, disp, st, cost, maxdisp, radius=4):
    import rag_amd
    from rag_amd import ops
    assert isinstance(res, rag_amd.DispMode) and isinstance(res, rag_amd.DispStats) and res.radius == radius
    want_d, want_s, want_m = ops.disp_softargmin_mode(cost, maxdisp, radius)
    assert torch.equal(res.disp, disp) and torch.equal(res.disp, want_d)
    assert torch.equal(res.tensor, st.tensor) and torch.equal(res.tensor, want_s) and torch.equal(res.mode_tensor, want_m)
    shape = (disp.shape[0], 3) + tuple(disp.shape[1:])
    assert res.tensor.shape == shape and res.mode_tensor.shape == shape and torch.isfinite(res.mode_tensor).all()
    assert res.mode_index.shape == disp.shape and res.mode_disp.shape == disp.shape and res.mode_mass.shape == disp.shape
    assert float((res.mode_disp - res.mode_index).abs().max()) <= radius
    assert 0.0 < float(res.mode_mass.min()) and float(res.mode_mass.max()) <= 1.0 + 1e-5


@pytest.mark.gpu
def test_model_forward_mode():
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
            disp, st = net(left, right, t, archis[t]), net.forward_stats(left, right, t, archis[t])
            _same(net.forward_mode(left, right, t, archis[t]), disp, st, cost, net.maxdisp)
            _same(serve.forward_mode(left, right, t), disp, st, cost, net.maxdisp)
        _same(net.forward_mode(left, right, 1, archis[1], radius=1), disp, st, cost, net.maxdisp, 1)
    res = net.forward_mode(left, right, 1, archis[1])               # grad mode on, parameters that require grad: still the inference path
    assert torch.equal(res.disp, disp) and not res.mode_tensor.requires_grad
    torch.manual_seed(6)
    sup = rag_amd.Network(rag_amd.ALL_CONV_GENOTYPE, "cpu", maxdisp=48)
    sup.expand(1, rag_amd.ALL_CONV_GENOTYPE, "cpu")
    sup = sup.to(DEV).eval()
    sel = [0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0]
    with torch.no_grad():
        lf, rf = sup._features(left, right, lambda x: sup.search_feature(x, sel))
        cost = sup.search_matching(None, sel, 1, features=(lf, rf))
        _same(sup.search_forward_mode(left, right, 1, sel), sup.search_forward(left, right, 1, sel), sup.search_forward_stats(left, right, 1, sel),
              cost, sup.maxdisp)


@pytest.mark.gpu
def test_matchingnet_forward_mode():
    net, lf, rf = _matching_net()
    with torch.no_grad():
        cost = net.matching(None, net.arch_init, None, features=(lf, rf))
        _same(net.forward_mode(lf, rf), net(lf, rf), net.forward_stats(lf, rf), cost, net.maxdisp)
        _same(net.disp.forward_mode(cost), net.disp(cost), net.disp.forward_stats(cost), cost, net.maxdisp)


@pytest.mark.gpu
def test_forward_mode_is_graph_capturable():
    """One MatchingNet.forward_mode with caller-owned outputs as a captured graph: kernel nodes only, and a replay on new input bytes
    gives the eager result bit for bit."""
    from rag_amd.train import graph_census
    net, lf, rf = _matching_net()
    out = torch.empty((2, 48, 84), device=DEV)
    stats = torch.empty((2, 3, 48, 84), device=DEV)
    mode = torch.empty((2, 3, 48, 84), device=DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net.forward_mode(lf, rf, out=out, stats=stats, mode=mode)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            res = net.forward_mode(lf, rf, out=out, stats=stats, mode=mode)
        census = graph_census(graph)
        graph.instantiate()
        assert res.disp.data_ptr() == out.data_ptr() and res.tensor.data_ptr() == stats.data_ptr() and res.mode_tensor.data_ptr() == mode.data_ptr()
        g = torch.Generator().manual_seed(4321)
        new_l, new_r = gpu(torch.randn((2, 12, 16, 28), generator=g)), gpu(torch.randn((2, 12, 16, 28), generator=g))
        lf.copy_(new_l)
        rf.copy_(new_r)
        graph.replay()
        torch.cuda.synchronize()
        eager = net.forward_mode(new_l, new_r)
        torch.cuda.synchronize()
    assert census["memcpy"] == 0 and census["memset"] == 0 and census["kernel"] > 0, census
    assert torch.equal(out, eager.disp) and torch.equal(stats, eager.tensor) and torch.equal(mode, eager.mode_tensor)
