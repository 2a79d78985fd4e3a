"""Training the head's uncertainty: the adjoint of the statistics head (disp_softargmin_stats_bwd_kernel), the fused uncertainty-aware
loss (rag_amd/csrc/disp_stats_train.hip), DispStatsFn, forward_train_stats and train_step(uncertainty=True).

Rows.  The adjoint table of test_stereo_ends_sweep.py (BWD_ROWS: white noise, every tile edge, d from 1 to 213, B up to 3) and the five
peaked rows of test_disp_stats.py (a parabola per coarse pixel: |cost| up to 1e4, a variance of a few px^2).

References, all plain torch on the CPU: float64 autograd through rag_amd.metrics.disp_stats_torch (F.interpolate -> softmin -> the four
definitions) for the adjoint; rag_amd.metrics.uncertainty_loss_torch in float64 for the loss, itself checked against the literal
expression and by gradcheck.  The same twins in float32 are the yardsticks.

Gates.  e_kernel <= NOISE e_yard + FLOOR max|g_ref64| with NOISE = 4 and FLOOR = 1e-6, the project's own (test_stereo_ends_sweep.py);
where the reference gradient vanishes (d = 1) the floor's scale is the largest cotangent.  The disparity-only set also keeps the 2e-4
ceiling of _bwd_gate (it is the plain kernel's arithmetic).  The peak's cotangent is zeroed at the pixels whose two largest fine
logits lie within tau = 2^-16 max|cost| of each other without being equal (there float32 may name the other arg-max: the derivative
of a maximum is not continuous); test_peak_table_is_admissible bounds their share.  Every GPU case prints
`STATS-BWD case=... set=... e_kernel=... e_yard=... bound=...`.

Worst figures per cotangent set on the MI355X, relative to max|g_ref64| (DESIGN.md 4.8.1 has the table by scale and the loss):
  set        rows      worst e_kernel                        e_yard there   bound there
  disp       noise     2.71e-5 (d 64, 24 x 63, scale 30)     2.74e-5        1.11e-4
  disp       peaked    5.36e-5 (d 64, 24 x 69, c = 4)        5.71e-5        2.00e-4
  variance   noise     3.72e-5 (d 64, 9 x 99, scale 30)      3.73e-5        1.50e-4
  variance   peaked    1.04e-4 (d 64, 24 x 69, c = 4)        1.02e-4        4.09e-4
  peak       noise     1.86e-5 (d 64, 9 x 99, scale 30)      1.87e-5        7.57e-5
  entropy    noise     3.57e-5 (d 64, 9 x 99, scale 30)      3.56e-5        1.44e-4
  entropy    peaked    1.15e-4 (d 64, 24 x 69, c = 4)        1.16e-4        4.63e-4
  all four   noise     3.73e-5 (d 64, 9 x 99, scale 30)      3.73e-5        1.50e-4
  three      peaked    1.03e-4 (d 64, 24 x 69, c = 4)        1.06e-4        4.26e-4
The case closest to its bound: variance on the d 65 -> 195 peaked row, 2.09e-5 against 4.05e-5 (0.52).
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_disp_stats import PEAKED_ROWS, _peaked_cost
from test_stereo_ends_sweep import BWD_ROWS, BWD_TWO_TILES, FLOOR, NOISE, _bid, _bwd_gate, _bwd_inputs

DEV = "cuda:0"
SETS = ("disp", "variance", "peak", "entropy", "all")
PEAKED_SETS = ("disp", "variance", "entropy", "three")
PLANES_OF = {"disp": (), "variance": (0,), "peak": (1,), "entropy": (2,), "all": (0, 1, 2), "three": (0, 2)}
HAS_DOUT = {"disp", "all", "three"}

# (kind, B, d, h, w, maxdisp, scale or curvature)
NOISE_KEYS = tuple(("noise",) + r for r in BWD_ROWS)
PEAKED_KEYS = tuple(("peaked",) + tuple(r[:5]) + (r[7],) for r in PEAKED_ROWS)
CASES = tuple((k, s) for k in NOISE_KEYS for s in SETS) + tuple((k, s) for k in PEAKED_KEYS for s in PEAKED_SETS)
TWO_TILE_KEYS = tuple(("noise",) + r for r in BWD_TWO_TILES)


def gpu(t):
    return None if t is None else t.to(DEV)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _kid(key):
    return key[0] + "_" + _bid(key[1:])


def _cid(case):
    return _kid(case[0]) + "_" + case[1]


def _lib():
    import rag_amd
    return rag_amd.load_library()


# ====================================================================================================== inputs and references
@functools.lru_cache(maxsize=None)
def _inputs(key):
    """(cost [B,d,h,w], dout [B,3h,3w], dstats [B,3,3h,3w], near [B,3h,3w] bool, ties): float32 inputs with N(0, 1) cotangents; `near`
    marks the pixels whose two largest fine logits of the float64 reference differ by 0 < gap < tau = 2^-16 max|cost|, and `ties` lists
    the (index, index) pairs of the exact ties."""
    kind, row = key[0], key[1:]
    B, d, h, w, maxdisp = row[:5]
    if kind == "noise":
        cost, dout = _bwd_inputs(row)
        seed = 8800 + BWD_ROWS.index(row)
    else:
        prow = PEAKED_ROWS[PEAKED_KEYS.index(key)]
        cost = _peaked_cost(prow).float()
        seed = 8900 + PEAKED_KEYS.index(key)
        dout = torch.randn((B, 3 * h, 3 * w), generator=gen(seed + 50))
    dstats = torch.randn((B, 3, 3 * h, 3 * w), generator=gen(seed))
    v = F.interpolate(cost.double()[:, None], (maxdisp, 3 * h, 3 * w), mode="trilinear", align_corners=False)[:, 0]
    if maxdisp > 1:
        top, idx = torch.topk(-v, 2, dim=1)
        gap = top[:, 0] - top[:, 1]
        tau = 2.0 ** -16 * float(cost.abs().max())
        near = (gap > 0) & (gap < tau)
        tie = gap == 0
        ties = tuple(zip(idx[:, 0][tie].tolist(), idx[:, 1][tie].tolist()))
    else:
        near, ties = torch.zeros((B, 3 * h, 3 * w), dtype=torch.bool), ()
    return cost, dout, dstats, near, ties


def _cotangents(key, cset):
    """(dout or None, dstats or None) of a cotangent set; the peak plane is zeroed at the near-tie pixels."""
    _cost, dout, dstats, near, _ties = _inputs(key)
    planes = PLANES_OF[cset]
    ds = None
    if planes:
        ds = torch.zeros_like(dstats)
        for p in planes:
            ds[:, p] = dstats[:, p]
        if 1 in planes:
            ds[:, 1][near] = 0.0
    return (dout if cset in HAS_DOUT else None), ds


def _twin_grad(cost, maxdisp, dout, dstats, dtype):
    """Autograd through disp_stats_torch in `dtype`: d (sum disp dout + sum stats dstats) / d cost."""
    from rag_amd.metrics import disp_stats_torch
    c = cost.detach().clone().to(dtype).requires_grad_(True)
    disp, st = disp_stats_torch(c, maxdisp)
    loss = torch.zeros((), dtype=dtype)
    if dout is not None:
        loss = loss + (disp * dout.to(dtype)).sum()
    if dstats is not None:
        loss = loss + (st * dstats.to(dtype)).sum()
    loss.backward()
    return c.grad


@functools.lru_cache(maxsize=None)
def _refs(case):
    """(float64 reference gradient, float32 yardstick gradient) of a case, computed once per module."""
    key, cset = case
    dout, ds = _cotangents(key, cset)
    cost = _inputs(key)[0]
    return _twin_grad(cost, key[5], dout, ds, torch.float64), _twin_grad(cost, key[5], dout, ds, torch.float32)


def _gate(case, got, ref, yard, cots):
    """The project's gate without a ceiling: e_kernel <= NOISE e_yard + FLOOR max|g_ref64| (max|cotangent| where the reference vanishes)."""
    cmax = max(float(c.abs().max()) for c in cots if c is not None)
    gmax = float(ref.abs().max())
    if gmax <= 1e-12 * cmax:
        gmax = cmax
    e_kernel, e_yard = float((got.cpu().double() - ref).abs().max()), float((yard.double() - ref).abs().max())
    bound = NOISE * e_yard + FLOOR * gmax
    print(f"STATS-BWD case={_kid(case[0])} set={case[1]} e_kernel={e_kernel / gmax:.3e} e_yard={e_yard / gmax:.3e} "
          f"bound={bound / gmax:.3e} max|g|={gmax:.3e}")
    assert e_kernel <= bound, (case, e_kernel, e_yard, bound)


# ====================================================================================================== without a GPU
CLOSED_ROWS = tuple((d, h, w, m, s) for (d, h, w, m) in ((8, 4, 6, 24), (16, 7, 11, 48), (2, 1, 1, 6), (64, 6, 6, 192)) for s in (0.1, 1.0, 30.0))


@pytest.mark.parametrize("row", CLOSED_ROWS, ids=lambda r: "d{}_{}x{}_D{}_s{}".format(*r))
def test_closed_form_vs_fp64_autograd(row):
    """disp_stats_bwd_torch (the formula the kernel implements) against float64 autograd through disp_stats_torch: each cotangent
    alone, then all four; relative error <= 1e-12."""
    from rag_amd.metrics import disp_stats_bwd_torch
    d, h, w, maxdisp, scale = row
    g = gen(7100 + CLOSED_ROWS.index(row))
    cost = (torch.randn((2, d, h, w), generator=g) * scale).double()
    dout = torch.randn((2, 3 * h, 3 * w), generator=g).double()
    dstats = torch.randn((2, 3, 3 * h, 3 * w), generator=g).double()
    sets = [(dout, None)]
    for p in range(3):
        one = torch.zeros_like(dstats)
        one[:, p] = dstats[:, p]
        sets.append((None, one))
    sets.append((dout, dstats))
    for n, (do, ds) in enumerate(sets):
        ref = _twin_grad(cost, maxdisp, do, ds, torch.float64)
        got = disp_stats_bwd_torch(cost, maxdisp, do, ds)
        assert got.dtype == torch.float64 and got.shape == cost.shape
        rel = float((got - ref).abs().max()) / float(ref.abs().max())
        print(f"STATS-BWD-CPU row={row} set={n} rel={rel:.3e}")
        assert rel <= 1e-12, (row, n, rel)
    got5 = disp_stats_bwd_torch(cost[:, None], maxdisp, dout, dstats)
    assert got5.shape == (2, 1, d, h, w) and torch.equal(got5[:, 0], got)
    assert disp_stats_bwd_torch(cost.float(), maxdisp, dout.float(), None).dtype == torch.float32


def _literal_loss(disp, stats, gt, maxdisp, var_floor):
    mask = (gt > 0) & (gt < maxdisp)
    s = stats[:, 0][mask] + var_floor
    return (F.smooth_l1_loss(disp[mask], gt[mask], reduction="none") / s.sqrt() + 0.5 * s.log()).mean()


def test_uncertainty_loss_torch():
    """The twin equals the literal expression; gradcheck in float64; the mask rule; the default var_floor; the empty-mask convention."""
    import inspect
    import rag_amd
    from rag_amd.metrics import VAR_FLOOR, uncertainty_loss_torch
    from rag_amd.train import masked_smooth_l1
    assert VAR_FLOOR == 1.0 / 12.0
    for fn in (uncertainty_loss_torch, rag_amd.uncertainty_loss, rag_amd.metrics.uncertainty_loss):
        assert inspect.signature(fn).parameters["var_floor"].default == 1.0 / 12.0
    assert rag_amd.uncertainty_loss is rag_amd.metrics.uncertainty_loss and "uncertainty_loss" in rag_amd.__all__
    g = gen(7200)
    maxdisp = 24.0
    gt = torch.rand((2, 5, 7), generator=g, dtype=torch.float64) * 30.0 - 3.0
    gt[0, 0, 0], gt[0, 0, 1], gt[0, 0, 2] = 0.0, maxdisp, 5.0            # the mask is strict at both ends
    disp = (gt + torch.randn((2, 5, 7), generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    stats = (torch.rand((2, 3, 5, 7), generator=g, dtype=torch.float64) * 4.0).requires_grad_(True)
    mask = (gt > 0) & (gt < maxdisp)
    assert not bool(mask[0, 0, 0]) and not bool(mask[0, 0, 1]) and bool(mask[0, 0, 2]) and 0 < int(mask.sum()) < mask.numel()
    for vf in (1.0 / 12.0, 0.5):
        a, b = uncertainty_loss_torch(disp, stats, gt, maxdisp, vf), _literal_loss(disp, stats, gt, maxdisp, vf)
        assert abs(float(a.detach()) - float(b.detach())) <= 1e-13 * abs(float(b.detach()))
    assert torch.equal(uncertainty_loss_torch(disp, stats, gt, maxdisp), uncertainty_loss_torch(disp, stats, gt, maxdisp, 1.0 / 12.0))
    assert torch.equal(rag_amd.uncertainty_loss(disp, stats, gt, maxdisp), uncertainty_loss_torch(disp, stats, gt, maxdisp))   # CPU path
    ga = torch.autograd.grad(uncertainty_loss_torch(disp, stats, gt, maxdisp), (disp, stats))
    gb = torch.autograd.grad(_literal_loss(disp, stats, gt, maxdisp, 1.0 / 12.0), (disp, stats))
    for x, y in zip(ga, gb):
        assert float((x - y).abs().max()) <= 1e-13
    assert not ga[0][~mask].any() and not ga[1][:, 1:].any() and not ga[1][:, 0][~mask].any()
    far = gt + torch.where(torch.rand((2, 5, 7), generator=g) < 0.5, 0.4, 2.5).double()    # away from the |e| = 1 kink of the second derivative
    assert torch.autograd.gradcheck(lambda d_, s_: uncertainty_loss_torch(d_, s_, gt, maxdisp), (far.requires_grad_(True), stats))
    empty = torch.full((2, 5, 7), maxdisp + 1.0, dtype=torch.float64)
    lo = uncertainty_loss_torch(disp, stats, empty, maxdisp)
    assert bool(torch.isnan(lo)) and bool(torch.isnan(masked_smooth_l1(disp, empty, maxdisp)))           # 0 / 0 in both
    ge = torch.autograd.grad(lo, (disp, stats))
    assert bool(torch.isnan(ge[0]).all()) or not ge[0].any()


@pytest.mark.parametrize("row", BWD_ROWS, ids=_bid)
def test_peak_table_is_admissible(row):
    """A condition on the INPUTS: at most 0.1 % of a row's pixels have their two largest fine logits within tau = 2^-16 max|cost| of each
    other (64 x a 4-ulp bound on an 8-tap fp32 interpolation of values up to max|cost|) without being equal, and every exact tie has
    one of its two indices at an end of the disparity axis, where the tied samples share their taps."""
    key = ("noise",) + row
    _cost, _dout, _dstats, near, ties = _inputs(key)
    share = float(near.double().mean())
    print(f"STATS-BWD-CPU case={_kid(key)} near-ties={int(near.sum())}/{near.numel()} ({100 * share:.4f} %) exact-ties={len(ties)}")
    assert share <= 1e-3, (row, share)
    last = row[4] - 1
    for i, j in ties:
        assert min(i, j) == 0 or max(i, j) == last, (row, i, j)


FAKE = ctypes.c_void_p(0x1000)


def test_abi_refuses_before_launch():
    """Status and text of every refusal of the adjoint's entry point; the pointers are never dereferenced (no launch happens)."""
    lib = _lib()

    def call(cost=FAKE, dout=FAKE, dstats=FAKE, dcost=FAKE, B=1, d=8, h=4, w=6, maxdisp=24, Ho=12, Wo=18):
        return lib.ragmi_disp_softargmin_stats_bwd(cost, dout, dstats, dcost, B, d, h, w, maxdisp, Ho, Wo, None), lib.ragmi_last_error()

    for name in ("B", "d", "h", "w", "maxdisp", "Ho", "Wo"):
        for v in (0, -1):
            st, msg = call(**{name: v})
            assert st == -1 and b"disp_softargmin_stats_bwd: bad size" in msg, (name, v)
    st, msg = call(B=65536)
    assert st == -1 and b"disp_softargmin_stats_bwd: bad size" in msg
    for bad in (dict(Ho=13), dict(Wo=17), dict(Ho=9, Wo=6), dict(Ho=4, Wo=24)):
        st, msg = call(**bad)
        assert st == -2 and b"Ho = 3h, Wo = 3w" in msg, bad
    st, msg = call(maxdisp=3073)
    assert st == -2 and b"maxdisp = 3073 exceeds the tap table (3072)" in msg
    st, msg = call(dout=None, dstats=None)
    assert st == -1 and b"both cotangents are null" in msg
    for name in ("cost", "dcost"):
        st, msg = call(**{name: None})
        assert st == -1 and b"disp_softargmin_stats_bwd: null pointer" in msg, name
    # the loss
    assert lib.ragmi_uncertainty_loss_workspace_elems(2, 3, 257) == 4 * 2 * 1 and lib.ragmi_uncertainty_loss_workspace_elems(1, 1024, 1024) == 4 * 64
    assert lib.ragmi_uncertainty_loss_workspace_elems(0, 3, 3) == 0
    f = ctypes.c_float
    assert lib.ragmi_uncertainty_loss_fwd(None, FAKE, FAKE, 1, 4, 4, f(24), f(1 / 12), FAKE, FAKE, None) == -1 and b"null pointer" in lib.ragmi_last_error()
    assert lib.ragmi_uncertainty_loss_fwd(FAKE, FAKE, FAKE, 1, 0, 4, f(24), f(1 / 12), FAKE, FAKE, None) == -1 and b"bad size" in lib.ragmi_last_error()
    assert lib.ragmi_uncertainty_loss_fwd(FAKE, FAKE, FAKE, 1, 4, 4, f(24), f(0), FAKE, FAKE, None) == -1 and b"var_floor" in lib.ragmi_last_error()
    assert lib.ragmi_uncertainty_loss_bwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, 1, 4, 4, f(24), f(1 / 12), None) == -1 and b"null pointer" in lib.ragmi_last_error()
    assert lib.ragmi_uncertainty_loss_bwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 4, -1, f(24), f(1 / 12), None) == -1 and b"bad size" in lib.ragmi_last_error()


def test_symbols_are_declared_and_bound():
    import os
    from conftest import ROOT
    from rag_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "rag_amd.h")).read()
    for name in ("ragmi_disp_softargmin_stats_bwd", "ragmi_uncertainty_loss_workspace_elems", "ragmi_uncertainty_loss_fwd", "ragmi_uncertainty_loss_bwd"):
        assert name + "(" in header and name in SIGNATURES and hasattr(_lib(), name), name


def test_python_refusals():
    import rag_amd
    from rag_amd import ops
    from rag_amd.train import GradBucket, GraphedTrainStep, forward_backward, train_step
    net = rag_amd.Network(rag_amd.ALL_SKIP_GENOTYPE, "cpu", maxdisp=24)
    img, gt = torch.zeros(1, 3, 24, 36), torch.ones(1, 24, 36)
    bucket = GradBucket(net.parameters())
    dnet = rag_amd.depth.Network.__new__(rag_amd.depth.Network)          # an instance for isinstance() only: the check comes before any use
    torch.nn.Module.__init__(dnet)
    meter = object()
    bad = [
        (net, dict(supervise=False), "supervise=False"),
        (net, dict(selected_ops=[0] * 18, t=0), "selected_ops"),
        (net, dict(sampled_ops=([0], [0])), "sampled_ops"),
        (dnet, dict(), "depth network"),
        (net, dict(meter=meter), "meter"),
    ]
    for who, kw, text in bad:
        with pytest.raises(ValueError, match=text):
            forward_backward(who, bucket, img, img, gt, uncertainty=True, **kw)
        with pytest.raises(ValueError, match=text):
            train_step(who, None, bucket, img, img, gt, uncertainty=True, **kw)
        with pytest.raises(ValueError, match=text):
            GraphedTrainStep(who, None, bucket, img, img, gt, uncertainty=True, **kw)
    with pytest.raises(NotImplementedError, match="no distribution"):
        rag_amd.depth.Network.forward_train_stats(None)
    cost = torch.zeros(1, 8, 4, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disp_softargmin_stats_bwd(cost, torch.zeros(1, 12, 18), None, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.uncertainty_loss_fwd(torch.zeros(1, 12, 18), torch.zeros(1, 3, 12, 18), torch.zeros(1, 12, 18), 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.uncertainty_loss_bwd(torch.zeros(1, 12, 18), torch.zeros(1, 3, 12, 18), torch.zeros(1, 12, 18), torch.zeros(4), torch.zeros(1), 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag_amd.Disp(24).forward_train_stats(cost[:, None].requires_grad_(True))
    with pytest.raises(RuntimeError, match="fp32 only"):
        rag_amd.Disp(24).forward_train_stats(cost[:, None].bfloat16())
    fea = torch.zeros(1, 12, 8, 12, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="fp32 only"):
        rag_amd.MatchingNet(rag_amd.ALL_SKIP_GENOTYPE, 24).forward_train_stats(fea, fea)
    with pytest.raises(RuntimeError, match="fp32 only"):
        net.forward_train_stats(img.double(), img.double(), 0)


# ====================================================================================================== on the MI355X: the adjoint
def _run(key, dout, ds):
    from rag_amd import ops
    return ops.disp_softargmin_stats_bwd(gpu(_inputs(key)[0]), gpu(dout), gpu(ds), key[5])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_adjoint_vs_fp64_autograd(case):
    key, cset = case
    dout, ds = _cotangents(key, cset)
    ref, yard = _refs(case)
    got = _run(key, dout, ds)
    torch.cuda.synchronize()
    assert got.shape == ref.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    if cset == "disp":
        _bwd_gate(_cid(case), got, ref, yard, dout)
    else:
        _gate(case, got, ref, yard, (dout, ds))


@pytest.mark.gpu
@pytest.mark.parametrize("key", NOISE_KEYS, ids=_kid)
def test_adjoint_exact_cases(key):
    """All cotangents zero give exactly zero; a zero plane in place of a NULL one passes the NULL run's gate; with cotangents on the
    last image only the other images get exactly nothing."""
    cost, dout, dstats, _near, _ties = _inputs(key)
    zero = _run(key, torch.zeros_like(dout), torch.zeros_like(dstats))
    assert torch.equal(zero.cpu(), torch.zeros_like(cost))
    ref, yard = _refs((key, "disp"))
    _bwd_gate(_kid(key) + "/zero-dstats", _run(key, dout, torch.zeros_like(dstats)), ref, yard, dout)
    do, ds = _cotangents(key, "all")
    ref, yard = _refs((key, "entropy"))
    _gate((key, "entropy/zero-dout"), _run(key, torch.zeros_like(dout), _cotangents(key, "entropy")[1]), ref, yard, (dstats,))
    if key[1] > 1:
        do, ds = do.clone(), ds.clone()
        do[:-1] = 0.0
        ds[:-1] = 0.0
        got = _run(key, do, ds)
        assert torch.equal(got[:-1].cpu(), torch.zeros_like(cost[:-1])) and bool(got[-1].any())
        got = _run(key, None, ds)
        assert torch.equal(got[:-1].cpu(), torch.zeros_like(cost[:-1])) and bool(got[-1].any())


@pytest.mark.gpu
@pytest.mark.parametrize("key", TWO_TILE_KEYS, ids=_kid)
def test_adjoint_bitwise_on_two_tiles(key):
    """Rows of at most two tiles (the float atomics are order-independent there): a NULL plane equals a zero plane, two runs are equal,
    and without a cotangent of the statistics DispStatsFn's backward is ops.disp_softargmin_bwd bit for bit."""
    import rag_amd
    from rag_amd import ops
    cost, dout, dstats, _near, _ties = _inputs(key)
    do, ds = _cotangents(key, "all")
    assert torch.equal(_run(key, do, None), _run(key, do, torch.zeros_like(ds)))
    assert torch.equal(_run(key, None, ds), _run(key, torch.zeros_like(do), ds))
    assert torch.equal(_run(key, do, ds), _run(key, do, ds))
    x = gpu(cost)[:, None].requires_grad_(True)
    res = rag_amd.Disp(key[5]).forward_train_stats(x)
    res.disp.backward(gpu(dout))
    assert torch.equal(x.grad[:, 0], ops.disp_softargmin_bwd(gpu(cost), gpu(dout), key[5]))
    x.grad = None
    res = rag_amd.Disp(key[5]).forward_train_stats(x)
    ((res.disp * gpu(do)).sum() + (res.tensor * gpu(ds)).sum()).backward()
    assert torch.equal(x.grad[:, 0], _run(key, do, ds))


STRAY_KEYS = (TWO_TILE_KEYS[0], TWO_TILE_KEYS[-1], ("noise", 3, 64, 9, 11, 192, 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("key", STRAY_KEYS, ids=_kid)
def test_adjoint_no_stray_writes(key):
    """dcost inside a sentinel-filled allocation, one float off its alignment: the sentinels on both sides stay intact."""
    from rag_amd import _lib as L, ops
    assert key in NOISE_KEYS
    cost = gpu(_inputs(key)[0]).contiguous()
    do, ds = (gpu(t).contiguous() for t in _cotangents(key, "all"))
    B, d, h, w, maxdisp = key[1:6]
    n, pad, sentinel = cost.numel(), 256, -12345.0
    big = torch.full((n + 2 * pad + 1,), sentinel, device=DEV)
    dc = big[pad + 1:pad + 1 + n].view(B, d, h, w)
    dc.zero_()
    L.check(L.load_library().ragmi_disp_softargmin_stats_bwd(cost.data_ptr(), do.data_ptr(), ds.data_ptr(), dc.data_ptr(), B, d, h, w, maxdisp,
                                                             3 * h, 3 * w, ops._stream()), "disp_softargmin_stats_bwd")
    torch.cuda.synchronize()
    assert bool((big[:pad + 1] == sentinel).all()) and bool((big[pad + 1 + n:] == sentinel).all())
    assert not bool((dc == sentinel).any())
    if key in TWO_TILE_KEYS:
        assert torch.equal(dc, _run(key, do.cpu(), ds.cpu()))
    else:
        ref, yard = _refs((key, "all"))
        _gate((key, "all/own-buffer"), dc, ref, yard, (do.cpu(), ds.cpu()))


@pytest.mark.gpu
@pytest.mark.parametrize("key", (NOISE_KEYS[2], PEAKED_KEYS[0], PEAKED_KEYS[3]), ids=_kid)
def test_forward_of_the_autograd_function_is_forward_stats(key):
    import rag_amd
    head = rag_amd.Disp(key[5])
    x = gpu(_inputs(key)[0])[:, None].requires_grad_(True)
    res = head.forward_train_stats(x)
    with torch.no_grad():
        want = head.forward_stats(x)
        plain = head(x)
    assert isinstance(res, rag_amd.DispStats) and res.disp.requires_grad and res.tensor.requires_grad
    assert torch.equal(res.disp, want.disp) and torch.equal(res.tensor, want.tensor) and torch.equal(res.disp, plain)


# ====================================================================================================== on the MI355X: the loss
LOSS_SHAPES = ((1, 1, 1), (2, 3, 257), (1, 16, 255))
LOSS_KINDS = ("mixed", "allvalid", "empty")
LOSS_MAXDISP = 192.0
VARIANCES = (0.0, 1e-6, 1.0, 1e4)


@functools.lru_cache(maxsize=None)
def _loss_inputs(shape, kind):
    """(est, stats, gt) float32.  The variance plane cycles over VARIANCES; peak and entropy planes hold noise the loss must ignore.
    mixed: gt ~ U(-2, 1.1 maxdisp) (some <= 0, some >= maxdisp), pixel (0, 0) of the last image valid, and with B > 1 the first image
    has no valid pixel; allvalid: every gt inside the mask; empty: every gt >= maxdisp or <= 0."""
    B, H, W = shape
    m = LOSS_MAXDISP
    g = gen(9700 + 10 * LOSS_SHAPES.index(shape) + LOSS_KINDS.index(kind))
    gt = torch.rand(shape, generator=g) * (1.1 * m + 2.0) - 2.0
    if kind == "mixed":
        gt[-1, 0, 0] = 0.37 * m
        if B > 1:
            gt[0] = torch.where(torch.rand((H, W), generator=g) < 0.5, torch.zeros(()), torch.full((), m + 3.0))
    elif kind == "allvalid":
        gt = torch.rand(shape, generator=g) * (m - 2.0) + 1.0
    else:
        gt = torch.where(torch.rand(shape, generator=g) < 0.5, -torch.rand(shape, generator=g), m + torch.rand(shape, generator=g) * 9.0)
        gt.view(-1)[0] = m                                                       # gt == maxdisp is outside the mask
    est = gt + (torch.rand(shape, generator=g) * 9.0 - 4.5)
    stats = torch.randn((B, 3, H, W), generator=g)
    stats[:, 0] = torch.tensor(VARIANCES)[torch.arange(B * H * W) % 4].view(shape)
    return est, stats, gt


def _loss_twin(est, stats, gt, dtype, gout):
    """(out[4], ddisp, dstats) of the twin in `dtype`: loss, masked smooth-L1 mean, mean sqrt(s), N and the gradients of gout * loss."""
    from rag_amd.metrics import VAR_FLOOR, uncertainty_loss_torch
    e, s, g = est.detach().clone().to(dtype).requires_grad_(True), stats.detach().clone().to(dtype).requires_grad_(True), gt.to(dtype)
    loss = uncertainty_loss_torch(e, s, g, LOSS_MAXDISP)
    mask = (g > 0) & (g < LOSS_MAXDISP)
    n = mask.sum()
    with torch.no_grad():
        sl1 = torch.where(mask, F.smooth_l1_loss(e, g, reduction="none"), torch.zeros((), dtype=dtype)).sum() / n
        sig = torch.where(mask, (s[:, 0] + VAR_FLOOR).sqrt(), torch.zeros((), dtype=dtype)).sum() / n
    if int(n):
        (loss * gout).backward()
        de, ds = e.grad, s.grad
    else:
        de, ds = torch.zeros_like(e), torch.zeros_like(s)
    return torch.stack((loss.detach(), sl1, sig, n.to(dtype))), de, ds


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LOSS_KINDS)
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "B{}_{}x{}".format(*s))
def test_loss_vs_fp64(shape, kind):
    """out, ddisp and dstats under the gate of the float32 twin; N exact; planes 1 and 2 of dstats exactly zero; an empty mask gives
    nan in out[0..2] (the masked smooth-L1's convention) and all-zero gradients; two runs are bitwise equal."""
    import rag_amd
    from rag_amd import ops
    est, stats, gt = _loss_inputs(shape, kind)
    gout = -2.5
    out64, de64, ds64 = _loss_twin(est, stats, gt, torch.float64, gout)
    out32, de32, ds32 = _loss_twin(est, stats, gt, torch.float32, gout)
    runs = []
    for _ in range(2):
        e, s = gpu(est).requires_grad_(True), gpu(stats).requires_grad_(True)
        loss = rag_amd.uncertainty_loss(e, s, gpu(gt), LOSS_MAXDISP)
        (loss * gout).backward()
        vec = ops.uncertainty_loss_fwd(e.detach(), s.detach(), gpu(gt), LOSS_MAXDISP)
        torch.cuda.synchronize()
        runs.append((loss.detach().cpu(), vec.cpu(), e.grad.cpu(), s.grad.cpu()))
    (loss, vec, de, ds), again = runs
    for a, b in zip(runs[0], again):
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))
    assert float(vec[3]) == float(out64[3])
    assert not ds[:, 1:].any()
    if kind == "empty" or float(out64[3]) == 0:
        assert float(out64[3]) == 0 and bool(torch.isnan(vec[:3]).all()) and bool(torch.isnan(loss)) and bool(torch.isnan(out64[0]))
        assert not de.any() and not ds.any()
        nomask = rag_amd.metrics.masked_smooth_l1(gpu(est), gpu(gt), LOSS_MAXDISP)
        assert bool(torch.isnan(nomask))
        return
    assert float(loss) == float(vec[0])
    failed = []
    for name, got, ref, yard in (("loss", vec[0], out64[0], out32[0]), ("sl1", vec[1], out64[1], out32[1]), ("sigma", vec[2], out64[2], out32[2]),
                                 ("ddisp", de, de64, de32), ("dvar", ds[:, 0], ds64[:, 0], ds32[:, 0])):
        e_kernel, e_yard = float((got.double() - ref).abs().max()), float((yard.double() - ref).abs().max())
        bound = NOISE * e_yard + FLOOR * float(ref.abs().max())
        print(f"UNC case=B{shape[0]}_{shape[1]}x{shape[2]}_{kind} tensor={name} e_kernel={e_kernel:.3e} e_yard={e_yard:.3e} bound={bound:.3e}")
        if not e_kernel <= bound:
            failed.append((name, e_kernel, e_yard, bound))
    assert not failed, failed
    mask = (gt > 0) & (gt < LOSS_MAXDISP)
    assert not de[~mask].any() and not ds[:, 0][~mask].any()


@pytest.mark.gpu
def test_loss_caller_owned_outputs_and_layouts():
    from rag_amd import ops
    est, stats, gt = (gpu(t) for t in _loss_inputs((2, 3, 257), "mixed"))
    out = torch.full((4,), 7.0, device=DEV)
    assert ops.uncertainty_loss_fwd(est, stats, gt, LOSS_MAXDISP, out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out, ops.uncertainty_loss_fwd(est, stats, gt, LOSS_MAXDISP))
    gout = torch.ones((1,), device=DEV)
    dd, ds = torch.full_like(est, 7.0), torch.full_like(stats, 7.0)
    a = ops.uncertainty_loss_bwd(est, stats, gt, out, gout, LOSS_MAXDISP, ddisp=dd, dstats=ds)
    b = ops.uncertainty_loss_bwd(est, stats, gt, out, gout, LOSS_MAXDISP)
    assert a[0].data_ptr() == dd.data_ptr() and a[1].data_ptr() == ds.data_ptr() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    wide = torch.zeros((2, 3, 2 * 257), device=DEV)
    wide[:, :, ::2] = est
    assert torch.equal(ops.uncertainty_loss_fwd(wide[:, :, ::2], stats, gt, LOSS_MAXDISP), out)


# ====================================================================================================== on the MI355X: model level
def _batch(seed, B=2, H=24, W=36, maxdisp=24):
    g = gen(seed)
    left, right = torch.rand((B, 3, H, W), generator=g), torch.rand((B, 3, H, W), generator=g)
    gt = torch.rand((B, H, W), generator=g) * (maxdisp + 4.0) - 2.0             # some pixels outside the mask at both ends
    return gpu(left), gpu(right), gpu(gt)


def _network(seed=11):
    import rag_amd
    torch.manual_seed(seed)
    return rag_amd.Network(rag_amd.ALL_SKIP_GENOTYPE, "cpu", maxdisp=24).to(DEV).train()


def _twin_step_loss(net, left, right, gt, features):
    """The same trunk under autograd, the head and the loss replaced by the torch twins on the trunk's own cost."""
    from rag_amd.metrics import disp_stats_torch, uncertainty_loss_torch
    if features:
        cost = net.matching(None, net.arch_init, None, features=(left, right))
    else:
        lf, rf = net._features(left, right, lambda x: net.feature(x, net.arch_init, None))
        cost = net.matching(None, net.arch_init, None, features=(lf, rf))
    disp, stats = disp_stats_torch(cost, net.maxdisp)
    return uncertainty_loss_torch(disp, stats, gt, net.maxdisp)


def _close(got, ref, tol, what):
    from test_hip_train import close
    close(got, ref, tol, what)


def _compare_grads(a, b):
    n = 0
    for (name, p), (_n, q) in zip(a.named_parameters(), b.named_parameters()):
        if q.grad is None:
            assert p.grad is None or not p.grad.any(), name
            continue
        _close(p.grad, q.grad, 2e-4, name)
        n += int(bool(q.grad.any()))
    return n


@pytest.mark.gpu
def test_network_uncertainty_step_vs_torch_twins():
    """forward_train_stats + uncertainty_loss + backward against the twin composition: loss and parameter gradients; train_step
    (uncertainty=True) returns that loss and moves the parameters as the twin step does; a plain train_step on the same seed returns the
    bits of the plain composition's loss."""
    import copy
    import rag_amd
    from rag_amd.train import GradBucket, exchange_and_update, make_optimizer, masked_smooth_l1, train_step
    left, right, gt = _batch(21)
    a = _network()
    b = copy.deepcopy(a)
    res = a.forward_train_stats(left, right, 0, a.arch_init)
    assert isinstance(res, rag_amd.DispStats) and res.disp.shape == (2, 24, 36) and res.tensor.shape == (2, 3, 24, 36)
    loss = rag_amd.uncertainty_loss(res.disp, res.tensor, gt, a.maxdisp)
    loss.backward()
    ref = _twin_step_loss(b, left, right, gt, False)
    ref.backward()
    loss, ref = loss.detach(), ref.detach()
    assert abs(float(loss) - float(ref)) <= 2e-4 * max(1.0, abs(float(ref))), (float(loss), float(ref))
    assert _compare_grads(a, b) > 5
    # the step
    c, d = _network(), _network()
    bc, bd = GradBucket(c.parameters()), GradBucket(d.parameters())
    oc, od = make_optimizer(c.parameters(), lr=1e-2), make_optimizer(d.parameters(), lr=1e-2)
    before = {k: v.detach().clone() for k, v in c.named_parameters()}
    got = train_step(c, oc, bc, left, right, gt, uncertainty=True)
    ref = _twin_step_loss(d, left, right, gt, False)
    bd.zero()
    ref.backward()
    exchange_and_update(od, bd, clip=5.0)
    ref = ref.detach()
    assert not got.requires_grad and abs(float(got) - float(ref)) <= 2e-4 * max(1.0, abs(float(ref)))
    assert abs(float(got) - float(loss)) <= 1e-6 * max(1.0, abs(float(loss)))
    moved = 0
    for (name, p), (_n, q) in zip(c.named_parameters(), d.named_parameters()):
        _close(p, q, 2e-4, name)
        assert torch.equal(p, before[name]) == torch.equal(q, before[name]), name
        moved += int(not torch.equal(p, before[name]))
    assert moved > 5
    # the plain step is the plain composition (its forward and loss are deterministic: the same bits)
    e, f = _network(), _network()
    be = GradBucket(e.parameters())
    plain = train_step(e, make_optimizer(e.parameters(), lr=1e-2), be, left, right, gt)
    want = masked_smooth_l1(f(left, right, 0, f.arch_init), gt, f.maxdisp)
    assert torch.equal(plain, want.detach()) and not torch.equal(plain, got)


@pytest.mark.gpu
def test_matchingnet_uncertainty_step_vs_torch_twins():
    import copy
    import rag_amd
    from rag_amd.train import GradBucket, make_optimizer, train_step
    torch.manual_seed(12)
    a = rag_amd.MatchingNet(rag_amd.ALL_SKIP_GENOTYPE, 24).to(DEV).train()
    b, c = copy.deepcopy(a), copy.deepcopy(a)
    g = gen(31)
    lf, rf = gpu(torch.randn((2, 12, 8, 12), generator=g)), gpu(torch.randn((2, 12, 8, 12), generator=g))
    gt = gpu(torch.rand((2, 24, 36), generator=g) * 28.0 - 2.0)
    la, ra_ = lf.clone().requires_grad_(True), rf.clone().requires_grad_(True)
    lb, rb = lf.clone().requires_grad_(True), rf.clone().requires_grad_(True)
    res = a.forward_train_stats(la, ra_)
    loss = rag_amd.uncertainty_loss(res.disp, res.tensor, gt, 24)
    loss.backward()
    ref = _twin_step_loss(b, lb, rb, gt, True)
    ref.backward()
    loss, ref = loss.detach(), ref.detach()
    assert abs(float(loss) - float(ref)) <= 2e-4 * max(1.0, abs(float(ref)))
    assert _compare_grads(a, b) > 3
    _close(la.grad, lb.grad, 2e-4, "dleft_fea")
    _close(ra_.grad, rb.grad, 2e-4, "dright_fea")
    bc = GradBucket(c.parameters())
    got = train_step(c, make_optimizer(c.parameters(), lr=1e-2), bc, lf, rf, gt, features=True, uncertainty=True)
    assert abs(float(got) - float(loss)) <= 1e-6 * max(1.0, abs(float(loss)))


# ====================================================================================================== on the MI355X: the captured step
@pytest.mark.gpu
def test_graphed_uncertainty_step():
    """GraphedTrainStep(uncertainty=True) at B = 2: kernel nodes only, and a replay on new input bytes gives the eager step's loss (the
    eager run takes the same number of steps; float atomics in the adjoints make two runs differ in the last bits, which three SGD steps
    amplify: the 2e-3 of test_graphed_train_step_matches_eager)."""
    from rag_amd.train import GradBucket, GraphedTrainStep, make_optimizer, train_step
    left, right, gt = _batch(41)
    left2, right2, gt2 = _batch(42)
    eager, graphed = _network(13), _network(13)
    be, bg = GradBucket(eager.parameters()), GradBucket(graphed.parameters())
    oe, og = make_optimizer(eager.parameters(), lr=1e-3, bucket=be), make_optimizer(graphed.parameters(), lr=1e-3, bucket=bg)
    want = [float(train_step(eager, oe, be, left, right, gt, uncertainty=True)) for _ in range(2)]
    want.append(float(train_step(eager, oe, be, left2, right2, gt2, uncertainty=True)))
    step = GraphedTrainStep(graphed, og, bg, left, right, gt, warmup=2, uncertainty=True)
    census = step.node_census
    assert census["memcpy"] == 0 and census["memset"] == 0 and census["kernel"] > 100, census
    torch.cuda.synchronize()
    got = float(step(left2, right2, gt2).clone())
    torch.cuda.synchronize()
    assert abs(float(step.first_loss) - want[0]) <= 1e-6 * max(1.0, abs(want[0]))
    assert abs(got - want[2]) <= 2e-3 * max(1.0, abs(want[2])), (got, want)
