"""Sparsification curves, AUSE and AURG of a per-pixel uncertainty: rag_amd.metrics.sparsification (rag_amd/csrc/sparsify.hip),
its plain-torch twin sparsification_torch, CalibrationMeter and DispStats.sparsification.

The CPU tests pin the definition on the twin (a hand-computed example, the properties a sparsification curve must have, the mask rules)
and the C ABI's refusals.  The GPU tests compare the kernels with the twin run on the CPU.

Gate.  Both sides form the error sums as integer sums of e_q = rint(|disp - gt| 2^20) and then evaluate the same float64 expressions, so
the curves are expected to agree bit for bit; the areas are float64 means of the stored floats taken in the same order.  The gate is
<= 1 fp32 ulp on every finite entry (room for a differently ordered float64 mean, nothing else), equal NaN positions, N and Nbad exact.
It is derived from the definition, not measured.  Every GPU case prints `SPARSIFY case=... max_ulp=...`.
"""
import ctypes
import functools

import pytest
import torch

DEV = "cuda:0"
MAXDISP = 48
SHAPES = ((1, 3, 5), (2, 33, 65), (3, 17, 129), (2, 96, 160))
FRACTIONS = (1, 4, 20, 32)
KINDS = ("white", "correlated", "quant4", "constant", "lowbits", "signs", "nonfinite", "empty_image", "one_pixel", "equal_errors",
         "big_errors")


def gpu(t):
    return t.to(DEV)


def _lib():
    import rag_amd
    return rag_amd.load_library()


def _twin(disp, unc, gt, maxdisp=MAXDISP, K=20, meter=None):
    from rag_amd.metrics import sparsification_torch
    return sparsification_torch(disp, unc, gt, maxdisp, K, meter)


# ====================================================================================================== inputs
@functools.lru_cache(maxsize=None)
def _inputs(kind, shape, seed=0):
    """(disp, unc, gt) on the CPU: disp = gt + noise, about a fifth of gt outside the mask (0 or >= maxdisp)."""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * KINDS.index(kind) + B * H * W)
    gt = 1.0 + (MAXDISP - 2.0) * torch.rand(shape, generator=g)
    out = torch.rand(shape, generator=g)
    gt = torch.where(out < 0.1, torch.zeros_like(gt), gt)
    gt = torch.where(out > 0.9, torch.full_like(gt, float(MAXDISP)) + 5 * (out - 0.9), gt)
    noise = torch.randn(shape, generator=g) * torch.where(torch.rand(shape, generator=g) < 0.2, 6.0, 0.7)
    disp = gt + noise
    unc = torch.rand(shape, generator=g)
    if kind == "correlated":
        unc = noise.abs() * (1 + 0.3 * torch.randn(shape, generator=g)).abs()
    elif kind == "quant4":
        unc = torch.randint(0, 4, shape, generator=g).float() * 0.5
    elif kind == "constant":
        unc = torch.full(shape, 0.7)
    elif kind == "lowbits":        # one value, its lowest 8 mantissa bits varied: the keys differ in the last radix level only
        unc = (torch.randint(0, 256, shape, generator=g, dtype=torch.int32) + 0x3FC00000).view(torch.float32)
    elif kind == "signs":          # negatives, both zeros, denormals of both signs, among ordinary values
        pool = torch.tensor([-3.5, -1e-3, -1e-40, -1.4e-45, -0.0, 0.0, 1.4e-45, 1e-40, 1e-3, 2.0])
        pick = pool[torch.randint(0, len(pool), shape, generator=g)]
        unc = torch.where(torch.rand(shape, generator=g) < 0.6, pick, torch.randn(shape, generator=g))
    elif kind == "nonfinite":
        bad = torch.tensor([float("nan"), float("inf"), float("-inf")])
        where = torch.rand(shape, generator=g)
        unc = torch.where(where < 0.15, bad[torch.randint(0, 3, shape, generator=g)], unc)
        disp = torch.where(where > 0.9, bad[torch.randint(0, 3, shape, generator=g)], disp)
    elif kind == "empty_image":
        gt = gt.clone()
        gt[0] = torch.where(out[0] < 0.5, torch.zeros_like(gt[0]), torch.full_like(gt[0], float(MAXDISP)))
    elif kind == "one_pixel":
        gt = gt.clone()
        gt[0] = 0.0
        gt[0, H // 2, W // 2] = 7.25
    elif kind == "equal_errors":   # gt on a grid of 1/8 px and a constant offset: every e_q is the same, the oracle is one tie group
        gt = torch.where((gt > 0) & (gt < MAXDISP), torch.round(gt * 8) / 8, gt).clamp(max=MAXDISP + 1)
        disp = gt + 3.5
    elif kind == "big_errors":     # errors up to maxdisp - eps
        top = torch.nextafter(torch.tensor(float(MAXDISP)), torch.tensor(0.0))
        far = torch.rand(shape, generator=g) < 0.3
        gt = torch.where(far, top.expand(shape), gt)
        disp = torch.where(far, torch.zeros_like(disp), disp)
    return disp.contiguous(), unc.contiguous(), gt.contiguous()


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, K, seed=0):
    res = _twin(*_inputs(kind, shape, seed), K=K)
    return res.tensor.clone(), res.scalars.clone()


def _ordered(x):
    i = x.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))


def max_ulp(a, b):
    """largest distance in fp32 ulps between the finite entries of a and b; NaN positions must coincide."""
    a, b = a.detach().cpu().float().reshape(-1), b.detach().cpu().float().reshape(-1)
    assert torch.equal(torch.isnan(a), torch.isnan(b)), "NaN positions differ"
    keep = ~torch.isnan(a)
    if not bool(keep.any()):
        return 0
    return int((_ordered(a[keep]) - _ordered(b[keep])).abs().max())


def _check(case, got, ref_curves, ref_scalars):
    u = max(max_ulp(got.tensor, ref_curves), max_ulp(got.scalars[:, :4], ref_scalars[:, :4]))
    print(f"SPARSIFY case={case} max_ulp={u}")
    assert torch.equal(got.scalars[:, 4:].cpu(), ref_scalars[:, 4:]), case       # N and Nbad: exact
    assert u <= 1, (case, u)


# ====================================================================================================== the definition (CPU)
def test_hand_computed_example():
    """8 pixels, K = 4: n = 8, 6, 4, 2.  unc sorted: 0 | 1 | 2 2 2 | 5 5 | 9 with errors .25 | .5 | 1 2 1.5 | 4 4 | 8; the cuts at 6
    and at 4 fall inside the groups {5, 5} (keeps 1 of 2: 8 / 2) and {2, 2, 2} (keeps 2 of 3: 4.5 * 2 / 3)."""
    gt = torch.full((1, 2, 4), 10.0)
    err = torch.tensor([0.5, 1.0, 4.0, 2.0, 8.0, 0.25, 4.0, 1.5]).view(1, 2, 4)
    unc = torch.tensor([1.0, 2.0, 5.0, 2.0, 9.0, 0.0, 5.0, 2.0]).view(1, 2, 4)
    res = _twin(gt + err, unc, gt, 192, 4)
    curves = torch.tensor([[[2.65625, 1.5416666, 0.9375, 0.375],        # 21.25/8, (5.25 + 4)/6, (.75 + 3)/4, (.25 + .5)/2
                            [2.65625, 1.5416666, 0.8125, 0.375],        # oracle: .25 .5 1 1.5 2 | 4 4 | 8
                            [0.375, 0.16666667, 0.0, 0.0],              # the bad pixels are the errors 4, 4, 8
                            [0.375, 0.16666667, 0.0, 0.0]]])
    # AUSE_epe = .125 / 4; AURG_epe = (0 + 1.1145834 + 1.71875 + 2.28125) / 4; AURG_d1 = (0 + .20833333 + .375 + .375) / 4
    scalars = torch.tensor([[0.03125, 1.2786459, 0.0, 0.23958333, 8.0, 3.0]])      # 1.27864584...: the nearest float is ...587
    assert torch.equal(res.tensor, curves), res.tensor
    assert torch.equal(res.scalars, scalars), res.scalars
    assert torch.equal(res.S_epe, curves[:, 0]) and torch.equal(res["O_d1"], curves[:, 3]) and torch.equal(res.AUSE_epe, scalars[:, 0])
    fl = res.floats()
    assert fl["S_epe"] == curves[:, 0].tolist() and fl["N"] == [8.0] and fl["AURG_d1"] == scalars[:, 3].tolist()


def test_properties_of_the_curves():
    import rag_amd
    from rag_amd.metrics import sparsification_torch
    assert rag_amd.sparsification is rag_amd.metrics.sparsification
    assert {"sparsification", "Sparsification", "CalibrationMeter"} <= set(rag_amd.__all__)
    disp, unc, gt = _inputs("white", (2, 33, 65))
    mask = (gt > 0) & (gt < MAXDISP)
    e_q = torch.round((disp.double() - gt.double()).abs() * 2 ** 20)
    # unc proportional to the error: the uncertainty curve IS the oracle
    res = _twin(disp, e_q.float() * 0.25, gt)
    assert torch.equal(res.S_epe, res.O_epe) and torch.equal(res.AUSE_epe, torch.zeros(2))
    # constant unc: one tie group, every cut keeps the masked EPE
    res = _twin(disp, torch.full_like(disp, 3.0), gt)
    for b in range(2):
        epe = (e_q[b][mask[b]].sum() * 2.0 ** -20 / mask[b].sum()).float()
        assert bool((res.S_epe[b] - epe).abs().max() <= 2 * torch.finfo(torch.float32).eps * epe)
        assert bool((res.S_epe[b] - res.S_epe[b, 0]).abs().max() <= 2 * torch.finfo(torch.float32).eps * epe)
    assert bool((res.AURG_epe.abs() <= 1e-6).all())
    # unc = -error: the most accurate pixels go first, so the curve cannot fall
    res = _twin(disp, -(disp - gt).abs(), gt)
    assert bool((res.S_epe[:, 1:] >= res.S_epe[:, :-1]).all()) and bool((res.AURG_epe <= 0).all())
    # the CPU path of the public call is the twin
    a, b = rag_amd.sparsification(disp, unc, gt, MAXDISP), sparsification_torch(disp, unc, gt, MAXDISP)
    assert torch.equal(a.tensor, b.tensor) and torch.equal(a.scalars, b.scalars)
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.sparsification(disp.clone().requires_grad_(True), unc, gt)


def test_tie_order_independence():
    disp, unc, gt = _inputs("quant4", (2, 33, 65))
    ref = _twin(disp, unc, gt)
    perm = torch.randperm(33 * 65, generator=torch.Generator().manual_seed(5))
    p = lambda t: t.reshape(2, -1)[:, perm].reshape(2, 33, 65).contiguous()
    got = _twin(p(disp), p(unc), p(gt))
    assert torch.equal(got.tensor, ref.tensor) and torch.equal(got.scalars, ref.scalars)


def test_agrees_with_the_existing_epe_and_d1():
    """S[0] keeps every masked pixel: the EPE and D1 of rag_amd.metrics (metrics.hip restated in torch, per image)."""
    disp, unc, gt = _inputs("white", (3, 17, 129))
    res = _twin(disp, unc, gt)
    for b in range(3):
        m = (gt[b] > 0) & (gt[b] < MAXDISP)
        E = (gt[b] - disp[b]).abs()[m]
        epe = E.double().sum() / m.sum()
        d1 = ((E > 3) & (E / gt[b][m].abs() > 0.05)).double().sum() / m.sum()
        assert abs(float(res.S_epe[b, 0]) - float(epe)) <= 2.0 ** -21 + float(epe) * 2.0 ** -23      # e_q's quantum, the store's rounding
        assert float(res.S_d1[b, 0]) == float(d1.float())
        assert float(res.O_epe[b, 0]) == float(res.S_epe[b, 0]) and float(res.O_d1[b, 0]) == float(res.S_d1[b, 0])


def test_mask_rules():
    nan, inf = float("nan"), float("inf")
    gt = torch.tensor([[[0.0, 48.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 6.0]]])
    unc = torch.tensor([[[1.0, 1.0, nan, inf, -inf, 1.0, 1.0, 1.0, 2.0]]])
    disp = torch.tensor([[[1.0, 1.0, 5.0, 5.0, 5.0, nan, inf, -inf, 8.0]]])
    res = _twin(disp, unc, gt, 48, 3)
    assert res.scalars[0, 4:].tolist() == [1.0, 0.0] and res.S_epe[0].tolist() == [2.0, 2.0, 2.0]
    res = _twin(disp[..., :8], unc[..., :8], gt[..., :8], 48, 3)          # nothing left
    assert bool(torch.isnan(res.tensor).all()) and bool(torch.isnan(res.scalars[0, :4]).all()) and res.scalars[0, 4:].tolist() == [0.0, 0.0]
    both = _twin(torch.cat((disp[..., :8], disp[..., 1:])), torch.cat((unc[..., :8], unc[..., 1:])), torch.cat((gt[..., :8], gt[..., 1:])), 48, 3)
    assert bool(torch.isnan(both.tensor[0]).all()) and both.S_epe[1].tolist() == [2.0, 2.0, 2.0]


def test_twin_arguments():
    from rag_amd import CalibrationMeter
    z = torch.zeros(1, 4, 4)
    for K in (0, 33, -1, 2.5):
        with pytest.raises(ValueError, match="fractions"):
            _twin(z, z, z, 48, K)
    for bad in ((torch.zeros(1, 4, 5), z, z), (z, torch.zeros(2, 4, 4), z), (z, z, torch.zeros(4, 4)), (z[0], z[0], z[0])):
        with pytest.raises(ValueError, match=r"\[B, H, W\]"):
            _twin(*bad)
    with pytest.raises(ValueError, match="maxdisp"):
        _twin(z, z, z, 0)
    with pytest.raises(ValueError, match="meter"):
        _twin(z, z, z, 48, 20, meter=CalibrationMeter("cpu", 4))
    with pytest.raises(ValueError, match="fractions"):
        CalibrationMeter("cpu", 40)


def test_meter_on_the_cpu():
    from rag_amd import CalibrationMeter
    meter = CalibrationMeter("cpu", 4)
    assert all(v != v for v in meter.mean()["S_epe"]) and meter.mean()["AUSE_epe"] != meter.mean()["AUSE_epe"] and meter.mean()["images"] == 0
    a, b = _inputs("white", (2, 33, 65)), _inputs("empty_image", (2, 33, 65))
    ra, rb = _twin(*a, K=4, meter=meter), _twin(*b, K=4, meter=meter)
    rows = torch.cat((ra.tensor[0:2], rb.tensor[1:2])).double().mean(0)          # image 0 of b has an empty mask: not counted
    got = meter.mean()
    assert got["images"] == 3
    assert torch.allclose(torch.tensor([got[n] for n in ("S_epe", "O_epe", "S_d1", "O_d1")], dtype=torch.float64), rows, rtol=1e-14, atol=0)
    assert got["N"] == float(torch.cat((ra.N, rb.N[1:])).double().mean())
    meter.reset()
    assert meter.mean()["images"] == 0


def test_which_of_the_head_statistics():
    from rag_amd import DispMode, DispStats
    from rag_amd.metrics import sparsification_torch
    g = torch.Generator().manual_seed(3)
    disp, gt = 40 * torch.rand((1, 6, 7), generator=g), 40 * torch.rand((1, 6, 7), generator=g)
    stats, mode = torch.rand((1, 3, 6, 7), generator=g), torch.rand((1, 3, 6, 7), generator=g)
    st, md = DispStats(disp, stats), DispMode(disp, stats, mode, 4)
    for obj in (st, md):
        for which, unc in (("variance", stats[:, 0]), ("entropy", stats[:, 2]), ("one_minus_peak", 1.0 - stats[:, 1])):
            assert torch.equal(obj.sparsification(gt, which, maxdisp=48, fractions=5).tensor, sparsification_torch(disp, unc, gt, 48, 5).tensor)
    assert torch.equal(md.sparsification(gt, "one_minus_mode_mass", maxdisp=48).tensor, sparsification_torch(disp, 1.0 - mode[:, 2], gt, 48).tensor)
    with pytest.raises(ValueError, match="needs a DispMode"):
        st.sparsification(gt, which="one_minus_mode_mass")
    with pytest.raises(ValueError, match="which must be one of"):
        md.sparsification(gt, which="sigma")


# ====================================================================================================== the C ABI (CPU)
FAKE = ctypes.c_void_p(4096)


def test_symbols_are_declared_and_bound():
    import os
    from conftest import ROOT
    from rag_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "rag_amd.h")).read()
    for name in ("ragmi_sparsification_workspace_elems", "ragmi_sparsification_fwd"):
        assert name + "(" in header and name in SIGNATURES and hasattr(_lib(), name), name


def test_abi_refusals_and_workspace():
    lib = _lib()
    elems = lib.ragmi_sparsification_workspace_elems
    # 16-byte elements: 2 B (2048 + 3 K 128) bins + 2 B (4 * 32 * 3 + 1) records
    assert elems(1, 3, 5, 20) == 2 * (2048 + 20 * 384) + 2 * 385
    assert elems(8, 384, 1248, 32) == 16 * (2048 + 32 * 384) + 16 * 385
    assert elems(1, 3, 5, 20) == elems(1, 384, 1248, 20)                     # O(B K bins): the image size does not enter
    assert elems(0, 3, 5, 20) == 0 and elems(1, 3, 5, 0) == 0 and elems(1, 3, 5, 33) == 0
    f = ctypes.c_float

    def call(disp=FAKE, unc=FAKE, gt=FAKE, B=1, H=4, W=4, maxdisp=48.0, K=20, ws=FAKE, curves=FAKE, scalars=FAKE, meter=None):
        st = lib.ragmi_sparsification_fwd(disp, unc, gt, B, H, W, f(maxdisp), K, ws, curves, scalars, meter, None)
        return st, lib.ragmi_last_error()

    for name in ("disp", "unc", "gt", "ws", "curves", "scalars"):
        st, msg = call(**{name: None})
        assert st == -1 and b"sparsification: null pointer" in msg, name
    for name in ("B", "H", "W"):
        for v in (0, -1):
            st, msg = call(**{name: v})
            assert st == -1 and b"sparsification: bad size" in msg, (name, v)
    for K in (0, 33, -5):
        st, msg = call(K=K)
        assert st == -1 and b"outside 1..32" in msg, K
    st, msg = call(H=65536, W=32768)
    assert st == -1 and b"below 2^31" in msg
    for md in (0.0, -1.0):
        st, msg = call(maxdisp=md)
        assert st == -1 and b"maxdisp must be positive" in msg
    st, msg = call(ws=ctypes.c_void_p(4096 + 8))
    assert st == -1 and b"workspace must be 16-byte aligned" in msg
    st, msg = call(meter=ctypes.c_void_p(4096 + 4))
    assert st == -1 and b"meter must be 8-byte aligned" in msg


# ====================================================================================================== the kernels (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("K", FRACTIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_against_the_twin(kind, shape, K):
    import rag_amd
    disp, unc, gt = _inputs(kind, shape)
    got = rag_amd.sparsification(gpu(disp), gpu(unc), gpu(gt), MAXDISP, K)
    assert got.tensor.shape == (shape[0], 4, K) and got.scalars.shape == (shape[0], 6) and got.tensor.dtype == torch.float32
    _check(f"{kind}_{'x'.join(map(str, shape))}_K{K}", got, *_reference(kind, shape, K))


@pytest.mark.gpu
def test_reproducible_and_per_image():
    import rag_amd
    disp, unc, gt = (gpu(t) for t in _inputs("quant4", (2, 96, 160)))
    a, b = rag_amd.sparsification(disp, unc, gt, MAXDISP), rag_amd.sparsification(disp, unc, gt, MAXDISP)
    assert torch.equal(a.tensor, b.tensor) and torch.equal(a.scalars, b.scalars)
    disp, unc, gt = (gpu(t) for t in _inputs("empty_image", (3, 17, 129)))
    a = rag_amd.sparsification(disp, unc, gt, MAXDISP, 4)
    f = rag_amd.sparsification(disp.flip(0), unc.flip(0), gt.flip(0), MAXDISP, 4)
    same = lambda x, y: torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0))
    assert same(f.tensor, a.tensor.flip(0)) and same(f.scalars, a.scalars.flip(0))
    strided = gpu(torch.zeros(3, 17, 258))
    strided[:, :, ::2] = unc
    assert same(rag_amd.sparsification(disp, strided[:, :, ::2], gt, MAXDISP, 4).tensor, a.tensor)
    fl = a.floats()
    assert fl["N"] == a.scalars[:, 4].tolist() and fl["S_d1"][1] == a.tensor[1, 2].tolist()
    with pytest.raises(RuntimeError, match="inference only"):
        rag_amd.sparsification(disp.clone().requires_grad_(True), unc, gt)
    with pytest.raises(ValueError, match="meter"):
        rag_amd.sparsification(disp, unc, gt, MAXDISP, 4, meter=rag_amd.CalibrationMeter("cpu", 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag_amd.sparsification(disp, unc.cpu(), gt)


@pytest.mark.gpu
def test_meter_over_two_batches():
    import rag_amd
    K = 20
    meter = rag_amd.CalibrationMeter(DEV, K)
    empty = meter.mean()
    assert empty["images"] == 0 and all(v != v for v in empty["S_epe"]) and empty["AUSE_d1"] != empty["AUSE_d1"]
    batches = (_inputs("correlated", (2, 33, 65)), _inputs("empty_image", (2, 33, 65)))
    for disp, unc, gt in batches:
        got = rag_amd.sparsification(gpu(disp), gpu(unc), gpu(gt), MAXDISP, K, meter=meter)
        plain = rag_amd.sparsification(gpu(disp), gpu(unc), gpu(gt), MAXDISP, K)
        assert torch.equal(torch.nan_to_num(got.tensor), torch.nan_to_num(plain.tensor))      # the meter does not change the result
    refs = [_reference("correlated", (2, 33, 65), K), _reference("empty_image", (2, 33, 65), K)]
    curves = torch.cat((refs[0][0], refs[1][0][1:])).double()                    # image 0 of the second batch: empty mask, not counted
    scalars = torch.cat((refs[0][1], refs[1][1][1:])).double()
    got = meter.mean()
    assert got["images"] == 3
    for c, name in enumerate(("S_epe", "O_epe", "S_d1", "O_d1")):
        assert torch.allclose(torch.tensor(got[name], dtype=torch.float64), curves[:, c].mean(0), rtol=1e-14, atol=1e-300), name
    for c, name in enumerate(("AUSE_epe", "AURG_epe", "AUSE_d1", "AURG_d1", "N", "Nbad")):
        assert got[name] == pytest.approx(float(scalars[:, c].mean()), rel=1e-14, abs=1e-300), name
    meter.reset()
    assert meter.mean()["images"] == 0


@pytest.mark.gpu
def test_graph_capture_with_a_meter():
    import rag_amd
    from rag_amd.train import graph_census
    K, shape = 20, (2, 33, 65)
    first, second = _inputs("white", shape), _inputs("quant4", shape)
    static = [gpu(t).clone() for t in first]
    meter = rag_amd.CalibrationMeter(DEV, K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rag_amd.sparsification(*static, MAXDISP, K, meter=meter)
    torch.cuda.current_stream().wait_stream(side)
    meter.reset()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        res = rag_amd.sparsification(*static, MAXDISP, K, meter=meter)
    census = graph_census(graph)
    assert census["kernel"] == 11 and census["memcpy"] == 0 and census["memset"] == 0 and census["other"] == 0, census
    graph.instantiate()
    eager_meter = rag_amd.CalibrationMeter(DEV, K)
    for k, batch in enumerate((first, second)):
        for s, t in zip(static, batch):
            s.copy_(gpu(t))
        graph.replay()
        eager = rag_amd.sparsification(*(gpu(t) for t in batch), MAXDISP, K, meter=eager_meter)
        assert torch.equal(res.tensor, eager.tensor) and torch.equal(res.scalars, eager.scalars), k
        _check(f"graph_replay{k}", res, *_reference(("white", "quant4")[k], shape, K))
    assert torch.equal(meter.sums, eager_meter.sums) and meter.mean()["images"] == 4


@pytest.mark.gpu
def test_disp_stats_sparsification():
    import rag_amd
    g = torch.Generator().manual_seed(11)
    cost = gpu(torch.randn((1, 1, 8, 6, 10), generator=g))
    gt = gpu(1.0 + 20 * torch.rand((1, 18, 30), generator=g))
    head = rag_amd.Disp(24).to(DEV)
    st = head.forward_stats(cost)
    a, b = st.sparsification(gt, maxdisp=24), rag_amd.sparsification(st.disp, st.variance, gt, 24)
    assert torch.equal(a.tensor, b.tensor) and torch.equal(a.scalars, b.scalars)
    _check("disp_stats_variance", a, *(lambda r: (r.tensor, r.scalars))(_twin(st.disp.cpu(), st.variance.cpu(), gt.cpu(), 24)))
    with pytest.raises(ValueError, match="needs a DispMode"):
        st.sparsification(gt, which="one_minus_mode_mass")
    md = head.forward_mode(cost)
    a, b = md.sparsification(gt, "one_minus_mode_mass", maxdisp=24), rag_amd.sparsification(md.disp, 1.0 - md.mode_mass, gt, 24)
    assert torch.equal(a.tensor, b.tensor) and torch.equal(a.scalars, b.scalars)
