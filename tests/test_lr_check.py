"""Left-right consistency check and the stack-and-mirror launch (rag_amd/csrc/lr_check.hip; rag_amd.metrics.lr_consistency, lr_stack,
Network.forward_lr) against the plain-torch twin rag_amd.metrics.lr_consistency_torch in float64.

The rule, per pixel: d = disp[b, y, x], xr = x - d; in view iff d finite and 0 <= xr <= W - 1; d' = the partner row at xr (linear);
e = |d - d'|; consistent iff in view, e finite and e <= max(abs_tol, rel_tol |d|).

Gates.  `weight` equal EXACTLY at every pixel (CASES keeps every pixel 1e-3 clear of the threshold and every xr 1e-3 clear of 0 and
W - 1: test_case_table_is_conditioned; no pixel is excused).  `err`: max |err - err64| <= 4 x max |twin32 - twin64| + 1e-6 max |err64|
over the finite entries, and the same set of +inf entries.  `valid` = float(count / (H W)) exactly.  What is the same arithmetic twice
(two runs, NaN-prefilled outputs, pixels that do not read a planted NaN / Inf) is compared bit for bit.

Measured on the MI355X, max |err - err64| in px (the kernel's equals the twin's own float32 run in every case: the same arithmetic in
the same order; it grows with W because x - d is rounded at the size of x):
  B1_3x3 8.4e-8   B2_4x5_shift 1.2e-7   B2_4x5 2.9e-7   B1_3x64 1.9e-6   B1_5x65 2.0e-6   B3_7x130 1.1e-5   B3_7x130_m 7.6e-6   B2_6x257 1.1e-5

Unmarked tests run without a GPU; the rest need the MI355X."""
import ctypes
import functools
import math

import pytest
import torch

DEV = "cuda:0"
CLEAR = 1e-3

# tag -> (B, H, W, partner_shift, mirrored, abs_tol, rel_tol, occluded_weight, seed).  The shapes: one thread's worth of rows, rows
# shorter than a wave, exactly one wave, a wave boundary inside a row, more than one 256-thread workgroup per image, B > 1.  Seeds:
# the first for which the case is conditioned (test_case_table_is_conditioned).
CASES = {
    "B1_3x3": (1, 3, 3, 0, 0, 0.5, 0.0, 0.0, 0),
    "B2_4x5_shift": (2, 4, 5, 1, 1, 0.5, 0.25, 0.25, 0),
    "B2_4x5": (2, 4, 5, 0, 0, 1.0, 0.0, 0.5, 0),
    "B1_3x64": (1, 3, 64, 0, 1, 0.5, 0.25, 0.0, 2),
    "B1_5x65": (1, 5, 65, 0, 0, 0.5, 0.25, 0.125, 1),
    "B3_7x130": (3, 7, 130, 1, 0, 1.0, 0.0, 0.25, 10),
    "B3_7x130_m": (3, 7, 130, 2, 1, 0.5, 0.25, 0.0, 230),
    "B2_6x257": (2, 6, 257, 1, 1, 0.5, 0.25, 0.75, 155),
}
TAGS = tuple(CASES)


def draw(tag, seed=None):
    """(disp, partner) float32 [B, H, W]: a per-row base disparity in (-3, 4) (the same in both maps, so that the maps agree up to
    their noise whatever the shift and the mirroring) plus independent noise of the size of the tolerance: some pixels agree, some do
    not, and the rows' ends look outside the image."""
    B, H, W, _shift, _mirrored, abs_tol, _rel, _occ, seed0 = CASES[tag]
    g = torch.Generator().manual_seed(1000 * TAGS.index(tag) + (seed0 if seed is None else seed))
    base = (torch.rand((1, H, 1), generator=g) * 7 - 3) * min(1.0, W / 8)
    amp = 1.6 * abs_tol
    disp = base + (torch.rand((B, H, W), generator=g) * 2 - 1) * amp
    partner = base + (torch.rand((B, H, W), generator=g) * 2 - 1) * amp
    return disp.float(), partner.float()


def twin(tag, disp, partner, dtype, **kw):
    from rag_amd.metrics import lr_consistency_torch
    _B, _H, _W, shift, mirrored, abs_tol, rel_tol, occ, _seed = CASES[tag]
    return lr_consistency_torch(disp.to(dtype), partner.to(dtype), abs_tol, rel_tol, occ, bool(mirrored), shift, **kw)


def kinds(tag, disp, partner):
    """(out of view, inconsistent, consistent, margin) of the float64 twin: three boolean maps and the smallest distance of any
    decision from its threshold (xr from 0 and W - 1 at every pixel with a finite d; e from the tolerance at every pixel in view)."""
    _B, _H, W, _shift, _mirrored, abs_tol, rel_tol, _occ, _seed = CASES[tag]
    d = disp.double()
    c = twin(tag, disp, partner, torch.float64)
    xr = torch.arange(W, dtype=torch.float64).view(1, 1, W) - d
    seen = torch.isfinite(c.error)
    tol = torch.maximum(torch.tensor(float(torch.tensor(abs_tol, dtype=torch.float32)), dtype=torch.float64),
                        float(torch.tensor(rel_tol, dtype=torch.float32)) * d.abs())
    margin = min(float(xr.abs().min()), float((xr - (W - 1)).abs().min()), float((c.error - tol)[seen].abs().min()))
    return ~seen, seen & ~c.mask, c.mask, margin


def conditioned(tag, disp, partner):
    out, bad, ok, margin = kinds(tag, disp, partner)
    both_signs = bool((disp > 0).any()) and bool((disp < 0).any())
    return bool(out.any()) and bool(bad.any()) and bool(ok.any()) and margin >= CLEAR and both_signs


# --------------------------------------------------------------------------- CPU
def test_occluder_scene_marks_exactly_the_stated_columns():
    """A background at disparity 2 with a foreground box at 6 over left columns [20, 30) of 40: the left view loses columns {0, 1}
    (out of view) and {16..19} (occluded, width 6 - 2), the right view {24..27} and {38, 39}; the stacked / mirrored call gives both."""
    from rag_amd.metrics import lr_consistency_torch
    W = 40
    for dt in (torch.float32, torch.float64):
        d_l = torch.full((1, 2, W), 2.0, dtype=dt)
        d_l[..., 20:30] = 6
        d_r = torch.full((1, 2, W), 2.0, dtype=dt)
        d_r[..., 14:24] = 6                                  # the box seen from the right camera: its columns less its disparity
        want_l = [0, 1, 16, 17, 18, 19]
        want_r = [24, 25, 26, 27, 38, 39]
        left = lr_consistency_torch(d_l, d_r)
        right = lr_consistency_torch(d_r.flip(-1), d_l, mirrored=True)           # the right camera's pair is the mirrored one
        stack = torch.cat((d_l, d_r.flip(-1)))
        both = lr_consistency_torch(stack, stack, mirrored=True, partner_shift=1)
        for row in range(2):
            assert (~left.mask[0, row]).nonzero().flatten().tolist() == want_l
            assert (~right.mask[0, row].flip(-1)).nonzero().flatten().tolist() == want_r
            assert (~both.mask[0, row]).nonzero().flatten().tolist() == want_l
            assert (~both.mask[1, row].flip(-1)).nonzero().flatten().tolist() == want_r
        assert left.weight.dtype == dt and left.valid.dtype == torch.float32
        assert left.valid.tolist() == [pytest.approx(34 / 40)] and both.valid.tolist() == [pytest.approx(34 / 40)] * 2
        assert torch.isinf(left.error[0, 0, :2]).all() and float(left.error[0, 0, 16]) == 4.0 and float(left.error[0, 0, 25]) == 0.0
        assert torch.equal(both.weight[:1], left.weight) and torch.equal(both.error[1:], right.error)


def test_twin_options():
    from rag_amd.metrics import LRCheck, lr_consistency, lr_consistency_torch
    d = torch.tensor([[[0.0, 0.5, 1.0, 9.0, float("nan")]]])
    p = torch.tensor([[[0.0, 0.0, 3.0, 0.0, 0.0]]])
    c = lr_consistency(d, p, abs_tol=0.75, occluded_weight=0.25, want_error=False)        # a CPU tensor: the twin
    assert isinstance(c, LRCheck) and c.error is None
    # x = 2: xr = 1 -> d' = 0, e = 1 > 0.75; x = 3: out of view; x = 4: NaN
    assert c.weight.tolist() == [[[1.0, 1.0, 0.25, 0.25, 0.25]]] and c.mask.tolist() == [[[True, True, False, False, False]]]
    assert c.valid.tolist() == [pytest.approx(0.4)]
    assert lr_consistency_torch(d, p, abs_tol=0.0, rel_tol=1.0).mask.tolist() == [[[True, True, True, False, False]]]
    with pytest.raises(RuntimeError, match="inference only"):
        lr_consistency(d.clone().requires_grad_(True), p)
    for kw in (dict(abs_tol=-1.0), dict(rel_tol=float("nan")), dict(occluded_weight=1.5), dict(partner_shift=1)):
        with pytest.raises(ValueError):
            lr_consistency_torch(d, p, **kw)
    with pytest.raises(ValueError):
        lr_consistency_torch(d[..., :1], p[..., :1])                                      # W < 2


def test_lr_stack_on_cpu():
    from rag_amd.metrics import lr_stack
    left, right = torch.randn(2, 3, 4, 5), torch.randn(2, 3, 4, 5)
    l2, r2 = lr_stack(left, right)
    assert torch.equal(l2, torch.cat((left, right.flip(-1)))) and torch.equal(r2, torch.cat((right, left.flip(-1))))
    out = (torch.empty(4, 3, 4, 5), torch.empty(4, 3, 4, 5))
    a, b = lr_stack(left, right, out=out)
    assert a is out[0] and b is out[1] and torch.equal(a, l2) and torch.equal(b, r2)
    with pytest.raises(ValueError):
        lr_stack(left, right[:1])
    with pytest.raises(ValueError):
        lr_stack(left, right, out=(torch.empty(2, 3, 4, 5), torch.empty(4, 3, 4, 5)))


def test_lr_abi_validates_before_launch():
    """Argument checks of ragmi_lr_check_fwd / ragmi_lr_stack_fwd run before any launch (pointers are never dereferenced)."""
    import rag_amd
    lib = rag_amd.load_library()
    fake = ctypes.c_void_p(0x1000)
    assert lib.ragmi_version() >= 590
    assert lib.ragmi_lr_check_workspace_elems(8, 192, 384) == 8 * (192 * 384 // 256)
    assert lib.ragmi_lr_check_workspace_elems(2, 6, 257) == 2 * 7
    assert lib.ragmi_lr_check_workspace_elems(1, 3, 1) == 0

    def call(disp=fake, partner=fake, B=2, H=4, W=5, shift=0, mirrored=0, a=1.0, r=0.0, occ=0.0, ws=fake, weight=fake, err=None, valid=fake):
        return lib.ragmi_lr_check_fwd(disp, partner, B, H, W, shift, mirrored, a, r, occ, ws, weight, err, valid, None)
    for kw in (dict(disp=None), dict(partner=None), dict(ws=None), dict(weight=None), dict(valid=None)):
        assert call(**kw) == -1 and b"null" in lib.ragmi_last_error(), kw
    for kw in (dict(B=0), dict(H=0), dict(W=1)):
        assert call(**kw) == -1 and b"bad size" in lib.ragmi_last_error(), kw
    for kw in (dict(shift=-1), dict(shift=2)):
        assert call(**kw) == -1 and b"partner_shift" in lib.ragmi_last_error(), kw
    for kw in (dict(a=-0.5), dict(a=math.inf), dict(r=-1.0), dict(r=math.nan)):
        assert call(**kw) == -1 and b"abs_tol" in lib.ragmi_last_error(), kw
    for kw in (dict(occ=-0.25), dict(occ=math.nan), dict(occ=math.inf)):
        assert call(**kw) == -1 and b"occluded_weight" in lib.ragmi_last_error(), kw
    assert lib.ragmi_lr_stack_fwd(None, fake, fake, fake, 1, 3, 4, 5, None) == -1
    assert lib.ragmi_lr_stack_fwd(fake, fake, fake, None, 1, 3, 4, 5, None) == -1
    assert lib.ragmi_lr_stack_fwd(fake, fake, fake, fake, 0, 3, 4, 5, None) == -1


def test_case_table_reaches_every_path():
    shapes = {CASES[t][:3] for t in TAGS}
    assert shapes == {(1, 3, 3), (2, 4, 5), (1, 3, 64), (1, 5, 65), (3, 7, 130), (2, 6, 257)}
    assert {CASES[t][4] for t in TAGS} == {0, 1}
    assert any(CASES[t][3] == 0 for t in TAGS) and any(0 < CASES[t][3] < CASES[t][0] for t in TAGS)
    assert any(CASES[t][6] > 0 for t in TAGS) and any(0 < CASES[t][7] < 1 for t in TAGS)
    assert any(CASES[t][1] * CASES[t][2] > 256 and CASES[t][0] > 1 for t in TAGS)      # more than one workgroup per image, B > 1


@pytest.mark.parametrize("tag", TAGS)
def test_case_table_is_conditioned(tag):
    """In float64: every pixel at least 1e-3 clear of the consistency threshold, every xr at least 1e-3 clear of 0 and W - 1, pixels
    of all three kinds and disparities of both signs; where rel_tol is set, it decides some pixel's tolerance."""
    disp, partner = draw(tag)
    out, bad, ok, margin = kinds(tag, disp, partner)
    assert margin >= CLEAR, margin
    assert bool(out.any()) and bool(bad.any()) and bool(ok.any())
    assert bool((disp > 0).any()) and bool((disp < 0).any())
    assert not bool((out & bad).any() or (out & ok).any() or (bad & ok).any()) and bool((out | bad | ok).all())
    abs_tol, rel_tol = CASES[tag][5], CASES[tag][6]
    if rel_tol and CASES[tag][2] >= 64:
        assert bool((rel_tol * disp.abs() > abs_tol).any())
    c32, c64 = twin(tag, disp, partner, torch.float32), twin(tag, disp, partner, torch.float64)
    assert torch.equal(c32.weight.double(), c64.weight) and torch.equal(c32.valid, c64.valid)       # the twin's float32 run agrees


# --------------------------------------------------------------------------- GPU
def _same_bits(a, b):
    """Equal as bit patterns (NaN == NaN, -0.0 != 0.0)."""
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _raw(tag, disp, partner, want_error=True):
    """ragmi_lr_check_fwd on workspace and outputs pre-filled with NaN (workspace: 0x7fc00000 as integers)."""
    import rag_amd
    lib = rag_amd.load_library()
    B, H, W, shift, mirrored, abs_tol, rel_tol, occ, _seed = CASES[tag]
    nan = float("nan")
    ws = torch.full((lib.ragmi_lr_check_workspace_elems(B, H, W),), nan, device=DEV).view(torch.int32)
    weight, err, valid = (torch.full(s, nan, device=DEV) for s in ((B, H, W), (B, H, W), (B,)))
    rc = lib.ragmi_lr_check_fwd(disp.data_ptr(), partner.data_ptr(), B, H, W, shift, mirrored, abs_tol, rel_tol, occ, ws.data_ptr(),
                                weight.data_ptr(), err.data_ptr() if want_error else None, valid.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ragmi_last_error()
    torch.cuda.synchronize()
    return weight, err, valid


@functools.lru_cache(maxsize=None)
def _run(tag):
    """One run per case, shared by the tests and never modified: inputs on the device, the wrapper's LRCheck, the two twins."""
    from rag_amd.metrics import lr_consistency
    _B, _H, _W, shift, mirrored, abs_tol, rel_tol, occ, _seed = CASES[tag]
    disp, partner = draw(tag)
    d, p = disp.to(DEV), partner.to(DEV)
    got = lr_consistency(d, p, abs_tol, rel_tol, occ, bool(mirrored), shift)
    torch.cuda.synchronize()
    return d, p, got, twin(tag, disp, partner, torch.float32), twin(tag, disp, partner, torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_check_vs_fp64_twin(tag):
    B, H, W = CASES[tag][:3]
    _d, _p, got, c32, c64 = _run(tag)
    assert torch.equal(got.weight.cpu().double(), c64.weight), (got.weight.cpu().double() != c64.weight).nonzero().tolist()
    assert torch.equal(got.mask.cpu(), c64.mask)
    err = got.error.cpu()
    fin = torch.isfinite(c64.error)
    assert torch.equal(torch.isinf(err) & (err > 0), ~fin) and not bool(torch.isnan(err).any())
    e_kernel = float((err.double() - c64.error)[fin].abs().max())
    e_twin32 = float((c32.error.double() - c64.error)[fin].abs().max())
    emax = float(c64.error[fin].max())
    print(f"LRCHECK case={tag} e_kernel={e_kernel:.2e} e_twin32={e_twin32:.2e} bound={4 * e_twin32 + 1e-6 * emax:.2e} max|err64|={emax:.3f}")
    assert e_kernel <= 4 * e_twin32 + 1e-6 * emax
    count = c64.mask.sum((1, 2)).double()
    assert torch.equal(got.valid.cpu(), (count / (H * W)).float()) and got.valid.shape == (B,)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_check_overwrites_nan_filled_outputs_and_repeats_bitwise(tag):
    d, p, got, _c32, _c64 = _run(tag)
    first, second = _raw(tag, d, p), _raw(tag, d, p)
    for a, b, c in zip(first, second, (got.weight, got.error, got.valid)):
        assert not bool(torch.isnan(a).any())
        assert _same_bits(a, b) and _same_bits(a, c)
    weight, err, valid = _raw(tag, d, p, want_error=False)                       # err = NULL: the other outputs are the same
    assert _same_bits(weight, got.weight) and _same_bits(valid, got.valid) and bool(torch.isnan(err).all())


def _readers(tag, disp, b_p, y, x_p):
    """Pixels [B, H, W] whose lookup reads partner[b_p, y, x_p]: in view, in the image that b_p is the partner of, with tap x0 or
    x1 (mirrored where the case says so) on x_p."""
    B, H, W, shift, mirrored, *_ = CASES[tag]
    d = disp.double()
    xr = torch.arange(W, dtype=torch.float64).view(1, 1, W) - d
    in_view = torch.isfinite(d) & (xr >= 0) & (xr <= W - 1)
    x0 = torch.floor(torch.where(in_view, xr, torch.zeros_like(xr))).long()
    x1 = torch.clamp(x0 + 1, max=W - 1)
    col = (lambda v: W - 1 - v) if mirrored else (lambda v: v)
    hit = in_view & ((col(x0) == x_p) | (col(x1) == x_p))
    keep = torch.zeros_like(hit)
    keep[(b_p - shift) % B, y] = hit[(b_p - shift) % B, y]
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("value", (math.nan, math.inf, -math.inf), ids=("nan", "inf", "minf"))
@pytest.mark.parametrize("tag", ("B2_4x5_shift", "B3_7x130", "B2_6x257"))
def test_nonfinite_values_stay_local(tag, value):
    """A NaN / Inf planted in disp changes its own pixel only; planted in partner, only the pixels whose taps read it.  Those get
    weight = occluded_weight and err = +inf; every other pixel is the clean run's, bit for bit; valid follows the twin."""
    from rag_amd.metrics import lr_consistency
    B, H, W, shift, mirrored, abs_tol, rel_tol, occ, _seed = CASES[tag]
    d, p, clean, _c32, _c64 = _run(tag)
    b, y, x = B - 1, H // 2, W // 2
    for which in ("disp", "partner"):
        d2, p2 = d.clone(), p.clone()
        (d2 if which == "disp" else p2)[b, y, x] = value
        if which == "disp":
            touched = torch.zeros((B, H, W), dtype=torch.bool)
            touched[b, y, x] = True
        else:
            touched = _readers(tag, d.cpu(), b, y, x)
            assert bool(touched.any()), "the planted tap is read by no pixel: move it"
        got = lr_consistency(d2, p2, abs_tol, rel_tol, occ, bool(mirrored), shift)
        torch.cuda.synchronize()
        want = twin(tag, d2.cpu(), p2.cpu(), torch.float64)
        assert _same_bits(got.weight.cpu()[~touched], clean.weight.cpu()[~touched]), which
        assert _same_bits(got.error.cpu()[~touched], clean.error.cpu()[~touched]), which
        assert bool((got.weight.cpu()[touched] == torch.tensor(occ)).all()) and bool(torch.isposinf(got.error.cpu()[touched]).all()), which
        assert torch.equal(got.weight.cpu().double(), want.weight) and torch.equal(got.valid.cpu(), want.valid), which


@pytest.mark.gpu
def test_check_refuses_unbuilt_inputs():
    from rag_amd.metrics import lr_consistency
    d = torch.zeros((1, 3, 4), device=DEV)
    with pytest.raises(RuntimeError, match="fp32|float32"):
        lr_consistency(d.double(), d.double())
    with pytest.raises(RuntimeError, match="CPU"):
        lr_consistency(d, d.cpu())
    with pytest.raises(ValueError):
        lr_consistency(d, d, partner_shift=1)


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 3))
@pytest.mark.parametrize("W", (5, 64, 65))
def test_stack_is_bitwise_cat_and_flip(C, W):
    from rag_amd.metrics import lr_stack
    g = torch.Generator().manual_seed(7 * W + C)
    left, right = torch.randn((2, C, 3, W), generator=g).to(DEV), torch.randn((2, C, 3, W), generator=g).to(DEV)
    want_l, want_r = torch.cat((left, right.flip(-1))), torch.cat((right, left.flip(-1)))
    l2, r2 = lr_stack(left, right)
    out = tuple(torch.full((4, C, 3, W), float("nan"), device=DEV) for _ in range(2))
    a, b = lr_stack(left, right, out=out)
    torch.cuda.synchronize()
    assert a is out[0] and b is out[1]
    assert _same_bits(l2, want_l) and _same_bits(r2, want_r) and _same_bits(a, want_l) and _same_bits(b, want_r)
    wide = torch.randn((2, C + 1, 3, W), generator=g).to(DEV)                   # a channel slice is not contiguous
    l3, _r3 = lr_stack(wide[:, 1:], right)
    assert _same_bits(l3[:2], wide[:, 1:]) and _same_bits(l3[2:], right.flip(-1))
