"""Sweep of the fused self-supervised loss (rag_amd/csrc/selfsup_loss.hip: warp + SSIM + L1 + smoothness and d loss / d disp) over
channel counts, remainder shapes, workgroup boundaries and disparity ranges, against the REFERENCE's own float64 run of
re_and_sm_loss (src_self/models/loss.py:112-141) on the same inputs: tests/golden/g14_selfsup_edges.npz, written by
tests/golden/make_golden_selfsup.py, whose row table (G14_ROWS, G14_TILED), probes and conditioning rules this file loads and checks
again on the committed arrays.

Gates.  Loss and terms: 1e-5 relative (test_selfsup_loss.py's bound).  Gradient: max |err| <= 4 x err_ref32 + 1e-5 max|grad64| over
EVERY pixel, where err_ref32 is the error of the reference's own float32 run (the fixture's grad32) against its float64 run; the
inputs are kept 1e-3 clear of each of the loss's kinks (ill_conditioned), so no pixel is excused.  Everything that is the same
arithmetic twice (the two kernel instantiations, a raw call on NaN-filled buffers, layouts, the backward's scaling, pixels outside a
changed disparity's footprint) is compared bit for bit.  Every GPU row prints `SELFSUP case=... e_kernel=... e_ref32=...`.

Measured on the MI355X, gradient error as a fraction of max|grad64| (kernel / the reference's float32):
  B1C3_3x3   6.6e-8 / 1.4e-7    B1C1_4x5   9.5e-8 / 9.5e-8    B2C2_5x4   5.0e-8 / 2.9e-7    B1C4_6x9   6.8e-7 / 7.4e-7
  B1C1_3x7   8.6e-8 / 2.8e-7    B1C2_8x3   3.2e-7 / 1.3e-7    B1C3_6x9   2.8e-7 / 3.8e-7    B1C3_6x10  1.4e-6 / 1.5e-6
  B1C3_6x11  4.5e-7 / 4.2e-7    B1C3_7x9   1.7e-6 / 1.9e-6    B1C3_7x10  1.2e-6 / 4.1e-6    B1C3_7x11  3.0e-7 / 3.6e-7
  B1C3_8x9   4.5e-6 / 4.4e-6    B1C3_8x10  1.2e-6 / 1.3e-6    B1C3_8x11  3.7e-6 / 4.1e-6    B1C3_21x27 9.1e-5 / 9.1e-5
  B1C3_24x24 3.9e-6 / 3.9e-6    B1C1_17x41 1.4e-6 / 1.7e-6    B3C3_16x17 4.1e-6 / 4.1e-6    B2C4_13x22 4.6e-6 / 4.6e-6
  B1C3_23x29 1.2e-5 / 1.2e-5    tiled: 7x10 1.9e-6 / 2.0e-6   16x17 5.1e-6 / 4.7e-6         13x22 2.1e-6 / 2.1e-6
Worst loss error 6.3e-8 (B1C2_8x3), worst term error 1.6e-7 (smoothness, B1C1_4x5).  21x27 holds one 3x3 block that the one-pass
variance makes ill-conditioned in float32, for the reference as for the kernel.

Unmarked tests run without a GPU; the rest need the MI355X."""
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

DEV = "cuda:0"
NOISE = 4.0                      # kernel gradient error <= NOISE x the reference's own float32 error + FLOOR x max|grad64|
FLOOR = 1e-5
YARD_MAX = 2.5e-4                # a row whose reference-float32 error exceeds this share of max|grad64| is no yardstick: redraw it
SS_WG = 64                       # threads per workgroup of selfsup_loss_kernel, one 3x3 block per thread


def _generator():
    """tests/golden/make_golden_selfsup.py as a module: its table and rules are plain numpy / torch; only its main() needs the
    reference."""
    spec = importlib.util.spec_from_file_location("make_golden_selfsup", os.path.join(GOLDEN, "make_golden_selfsup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MG = _generator()
CASES = MG.g14_cases()                                      # [(tag, (B, C, H, W, d_lo, d_hi), tile or None)]
TAGS = tuple(tag for tag, _row, _tile in CASES)
ROW = {tag: row for tag, row, _tile in CASES}
PROBE_TAG = "B1C3_8x11"
RAW_TAGS = ("B1C3_3x3", "B1C1_4x5", "B2C2_5x4") + tuple(f"B1C3_{H}x{W}" for H in (6, 7, 8) for W in (9, 10, 11)) \
    + ("B1C1_17x41", "B3C3_16x17")
SCALE_TAGS = ("B1C3_7x10", "B3C3_16x17")                    # 70 and 816 gradient elements: under and over one 256-thread workgroup
LAYOUT_TAGS = ("B2C2_5x4", "B3C3_16x17", "B2C4_13x22")      # B > 1: a channel slice of a wider tensor is not contiguous


@functools.lru_cache(maxsize=None)
def _g14():
    return load_golden("g14_selfsup_edges")


def _arrays(tag):
    g = _g14()
    return {k: g[f"{tag}::{k}"] for k in ("left", "right", "disp", "loss32", "loss64", "terms32", "terms64", "grad32", "grad64")}


def _threads(row):
    return row[0] * (row[2] // 3) * (row[3] // 3)


def rel_max(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _yardstick(a):
    """(max |grad32 - grad64| of the reference's two runs, max |grad64|)"""
    return float(np.abs(a["grad32"].astype(np.float64) - a["grad64"]).max()), float(np.abs(a["grad64"]).max())


# --------------------------------------------------------------------------- CPU: the table, the fixture, the host twin
def test_table_reaches_every_path():
    """From the rows alone: every channel count, every (H % 3, W % 3), one block per column / row, 63 / 64 / 65 threads, and a
    workgroup boundary strictly inside the blocks of a batch item b > 0."""
    rows = [row for _tag, row, _tile in CASES]
    assert len(set(TAGS)) == len(TAGS) == 24 and PROBE_TAG in TAGS and ROW[PROBE_TAG] == MG.PROBE_ROW
    assert set(RAW_TAGS + SCALE_TAGS + LAYOUT_TAGS) <= set(TAGS)
    assert {r[1] for r in rows} == {1, 2, 3, 4}
    assert {(r[2] % 3, r[3] % 3) for r in rows if r[2] // 3 >= 2 and r[3] // 3 >= 2} == {(a, b) for a in range(3) for b in range(3)}
    assert any(r[2] // 3 == 1 for r in rows) and any(r[3] // 3 == 1 for r in rows)
    assert any(r[2] // 3 == 1 and r[3] // 3 > 1 for r in rows) and any(r[3] // 3 == 1 and r[2] // 3 > 1 for r in rows)
    assert {3, 4, 5} <= {r[2] for r in rows} and {3, 4, 5} <= {r[3] for r in rows}
    assert any(r[2] % 3 == 2 for r in rows) and any(r[3] % 3 == 0 and r[2] % 3 != 0 for r in rows)
    assert {1, 63, 64, 65} <= {_threads(r) for r in rows}
    inside = [r for r in rows for b in range(1, r[0])
              if any(b * (_threads(r) // r[0]) < m < (b + 1) * (_threads(r) // r[0]) for m in range(SS_WG, _threads(r), SS_WG))]
    assert (3, 3, 16, 17, -4.0, 24.0) in inside
    assert all(r[4] < 0 < r[5] for r in rows)                       # disparities of both signs in every row
    for tag in SCALE_TAGS:
        assert (ROW[tag][0] * ROW[tag][2] * ROW[tag][3]) % 256 != 0
    assert ROW["B3C3_16x17"][0] * 16 * 17 > 256
    for tag in LAYOUT_TAGS:
        assert ROW[tag][0] > 1


def test_fixture_matches_table():
    g = _g14()
    assert tuple(g["cases"].tolist()) == TAGS
    assert [tuple(p) for p in g["probes"].tolist()] == list(MG.PROBES)
    for tag, (B, C, H, W, lo, hi), tile in CASES:
        a = _arrays(tag)
        assert a["left"].shape == a["right"].shape == (B, C, H, W) and a["disp"].shape == a["grad32"].shape == a["grad64"].shape == (B, H, W)
        assert a["left"].dtype == a["right"].dtype == a["disp"].dtype == a["grad32"].dtype == np.float32 and a["grad64"].dtype == np.float64
        assert a["terms32"].shape == a["terms64"].shape == (3,)
        assert lo <= float(a["disp"].min()) < 0 < float(a["disp"].max()) <= hi, tag
        xs = MG.xs_of(a["disp"].astype(np.float64), W)
        if W >= 9:                                                    # a negative disparity takes a sample past the right edge
            assert bool((xs[:, :, :W - 1] > W - 1).any()), tag
        if tile:
            d = a["disp"]
            assert all(len(np.unique(d[b, y:y + tile, x:x + tile])) == 1 for b in range(B) for y in range(0, H, tile) for x in range(0, W, tile))


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_is_conditioned(tag):
    """The generator's rules, again on the committed arrays: no pixel within 1e-3 of a bilinear kink, of a |left - left_est| tie
    (where the mask keeps it), of the SSIM clamp or of a smoothness tie that is not exact; some pixel unmasked, a quarter of them from
    6 x 9 on; and the reference's own float32 gradient within 2.5e-4 max|g| of its float64 one."""
    _B, _C, H, W, _lo, _hi = ROW[tag]
    a = _arrays(tag)
    assert not MG.ill_conditioned(a["left"], a["right"], a["disp"]).any()
    assert not MG.near_kink(a["disp"], W).any()
    est, kept, half = MG.selfsup_parts64(a["left"], a["right"], a["disp"])
    tie = (torch.from_numpy(a["left"]).double() - est).abs().amin(1)
    assert float(tie[kept].min()) >= 1e-3
    assert float(torch.minimum(half.abs(), (half - 1).abs()).min()) >= 1e-3
    d = a["disp"].astype(np.float64)
    for gap in (np.abs(d[:, :, :-1] - d[:, :, 1:]), np.abs(d[:, :-1] - d[:, 1:])):
        assert not ((gap < 1e-3) & (gap != 0)).any()
    share = float(kept.double().mean())
    assert bool(kept.any()) and not bool(kept[:, 0].any()) and not bool(kept[:, -1].any())
    assert share >= 0.25 or H < 6 or W < 9, share
    yard, gmax = _yardstick(a)
    assert yard <= YARD_MAX * gmax, (yard / gmax)
    if tag == PROBE_TAG:
        for probe in MG.PROBES:
            assert not MG.ill_conditioned(a["left"], a["right"], MG.probe_disp(a["disp"], probe)).any(), probe


@pytest.mark.parametrize("tag", TAGS)
def test_host_twin_matches_reference_at_every_row(tag):
    """re_and_sm_loss_torch in float64 against the reference's float64 loss, terms and gradient, to 1e-6 relative, at every C."""
    from rag_amd.metrics import re_and_sm_loss_torch
    a = _arrays(tag)
    d = torch.from_numpy(a["disp"]).double().requires_grad_(True)
    loss, terms = re_and_sm_loss_torch(d, torch.from_numpy(a["left"]).double(), torch.from_numpy(a["right"]).double())
    loss.backward()
    ref = float(a["loss64"])
    assert abs(loss.item() - ref) <= 1e-6 * abs(ref), (loss.item(), ref)
    for got, want in zip(terms, a["terms64"]):
        assert abs(got.item() - want) <= 1e-6 * abs(want), (got.item(), want)
    assert rel_max(d.grad, a["grad64"]) <= 1e-6


# --------------------------------------------------------------------------- GPU
def gpu(x):
    return torch.as_tensor(x).to(DEV)


def _metrics():
    import rag_amd
    rag_amd.load_library()
    return rag_amd.metrics


def _unit_grad(disp, left, right):
    """(loss, d loss / d disp) through the autograd Function with a unit incoming gradient."""
    d = disp.detach().clone().requires_grad_(True)
    loss = _metrics().re_and_sm_loss(d, left, right)
    loss.backward()
    return loss.detach(), d.grad


@functools.lru_cache(maxsize=None)
def _run(tag):
    """One run per row, shared by the tests: inputs on the device, (loss, gradient) through .backward(), and (out[4], unit_grad) of the
    raw GRAD=true call behind it."""
    a = _arrays(tag)
    d, lt, rt = gpu(a["disp"]), gpu(a["left"]), gpu(a["right"])
    loss, grad = _unit_grad(d, lt, rt)
    out, ug = _metrics()._selfsup_raw(d, lt, rt, True)
    torch.cuda.synchronize()
    return d, lt, rt, loss, grad, out, ug


def _same_bits(a, b):
    """Equal as bit patterns (NaN == NaN, -0.0 != 0.0)."""
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_forward_and_gradient_vs_fp64(tag):
    """(a) loss and terms within 1e-5 of the reference's float64; the gradient of .backward() within 4 x the reference's own float32
    error + 1e-5 max|grad64|, no pixel left out."""
    a = _arrays(tag)
    _d, _lt, _rt, loss, grad, out, ug = _run(tag)
    ref = float(a["loss64"])
    got = out.cpu().double()
    e_loss = abs(float(loss) - ref) / abs(ref)
    e_terms = [abs(float(g) - w) / abs(w) for g, w in zip(got[1:], a["terms64"])]
    yard, gmax = _yardstick(a)
    err = float((grad.cpu().double() - torch.from_numpy(a["grad64"])).abs().max())
    print(f"SELFSUP case={tag} e_kernel={err / gmax:.2e} e_ref32={yard / gmax:.2e} bound={(NOISE * yard + FLOOR * gmax) / gmax:.2e} "
          f"e_loss={e_loss:.1e} e_terms={[f'{v:.1e}' for v in e_terms]}")
    assert all(w != 0 for w in a["terms64"]) and gmax > 0
    assert e_loss <= 1e-5 and abs(float(got[0]) - ref) <= 1e-5 * abs(ref)
    assert max(e_terms) <= 1e-5, e_terms
    assert yard <= YARD_MAX * gmax
    assert grad.shape == a["grad64"].shape and bool(torch.isfinite(grad).all())
    assert err <= NOISE * yard + FLOOR * gmax, (err / gmax, yard / gmax)
    assert _same_bits(loss.reshape(1), out[:1]) and _same_bits(grad, ug)      # the Function adds nothing to the raw call


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_terms_kernel_equals_gradient_kernel_bitwise(tag):
    """(b) selfsup_loss_kernel<C, false> behind self_supervised_terms and <C, true> behind re_and_sm_loss: the same four floats."""
    d, lt, rt, _loss, _grad, out, _ug = _run(tag)
    terms = _metrics().self_supervised_terms(d, lt, rt)
    assert terms.shape == (4,) and _same_bits(terms, out), (terms.tolist(), out.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("tag", RAW_TAGS)
def test_raw_call_writes_every_gradient_pixel(tag):
    """(c) ragmi_selfsup_loss_fwd on workspace, out and unit_grad pre-filled with NaN: every gradient pixel is written (unit_grad comes
    from torch.empty and nothing is memset), and the results are the wrapper's, bit for bit."""
    import rag_amd
    lib = rag_amd.load_library()
    B, C, H, W = ROW[tag][:4]
    d, lt, rt, _loss, _grad, out, ug = _run(tag)
    nws = lib.ragmi_selfsup_loss_workspace_elems(B, H, W)
    assert nws == 2 * 3 * -(-_threads(ROW[tag]) // SS_WG)
    nan = float("nan")
    ws = torch.full((nws,), nan, device=DEV, dtype=torch.float32)
    out2 = torch.full((4,), nan, device=DEV, dtype=torch.float32)
    ug2 = torch.full((B, H, W), nan, device=DEV, dtype=torch.float32)
    rc = lib.ragmi_selfsup_loss_fwd(lt.data_ptr(), rt.data_ptr(), d.data_ptr(), B, C, H, W, 0, ws.data_ptr(), out2.data_ptr(),
                                    ug2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ragmi_last_error()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ug2).any()), torch.isnan(ug2).nonzero().tolist()
    assert not bool(torch.isnan(out2).any())
    assert _same_bits(out2, out) and _same_bits(ug2, ug)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", SCALE_TAGS)
def test_backward_scales_the_unit_gradient_bitwise(tag):
    """(d) the gradient for an incoming gradient g is float32(g) x unit_grad bit for bit; g = 0 gives zeros of either sign."""
    d, lt, rt, _loss, _grad, _out, ug = _run(tag)
    for gout in (1.0, -2.5, 0.0):
        x = d.detach().clone().requires_grad_(True)
        _metrics().re_and_sm_loss(x, lt, rt).backward(torch.tensor(gout, device=DEV))
        want = torch.tensor(gout, dtype=torch.float32, device=DEV) * ug
        assert _same_bits(x.grad, want), gout
        if gout == 0.0:
            assert bool((x.grad == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("tag", LAYOUT_TAGS)
def test_noncontiguous_inputs_give_the_same_bits(tag):
    """(e) left and right as channel slices of a wider tensor, disp as a [:, :, ::2] view: bitwise the contiguous call."""
    B, C, H, W = ROW[tag][:4]
    d, lt, rt, loss, grad, _out, _ug = _run(tag)
    wide_l = torch.full((B, C + 2, H, W), 7.0, device=DEV)
    wide_r = torch.full((B, C + 3, H, W), -7.0, device=DEV)
    wide_l[:, 1:C + 1] = lt
    wide_r[:, 2:C + 2] = rt
    wide_d = torch.full((B, H, 2 * W), 3.0, device=DEV)
    wide_d[:, :, ::2] = d
    ls, rs, ds = wide_l[:, 1:C + 1], wide_r[:, 2:C + 2], wide_d[:, :, ::2]
    assert not ls.is_contiguous() and not rs.is_contiguous() and not ds.is_contiguous()
    assert torch.equal(ls, lt) and torch.equal(rs, rt) and torch.equal(ds, d)
    loss2, grad2 = _unit_grad(ds, ls, rs)
    assert _same_bits(loss2.reshape(1), loss.reshape(1)) and _same_bits(grad2, grad)
    assert _same_bits(_metrics().self_supervised_terms(ds, ls, rs), _metrics().self_supervised_terms(d, lt, rt))


def _footprint(H, W, y, x):
    """Pixels whose gradient may depend on disp[y, x]: the pixel and its four neighbours (smoothness), and its 3x3 SSIM block if it
    lies in one (rows < 3 (H // 3) and columns < 3 (W // 3))."""
    m = torch.zeros((H, W), dtype=torch.bool)
    for yy, xx in ((y, x), (y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
        if 0 <= yy < H and 0 <= xx < W:
            m[yy, xx] = True
    if y < 3 * (H // 3) and x < 3 * (W // 3):
        m[3 * (y // 3):3 * (y // 3) + 3, 3 * (x // 3):3 * (x // 3) + 3] = True
    return m


def test_probe_footprints():
    _B, _C, H, W = ROW[PROBE_TAG][:4]
    sizes = [int(_footprint(H, W, y, x).sum()) for y, x in MG.PROBES]
    assert sizes == [10, 5, 5]                      # (4, 5): its block and the neighbour (4, 6); the remainder pixels: 1 + 4
    (y0, x0), (y1, x1), (y2, x2) = MG.PROBES
    assert y0 < 3 * (H // 3) and x0 < 3 * (W // 3) and y1 >= 3 * (H // 3) and x1 < 3 * (W // 3) and y2 < 3 * (H // 3) and x2 >= 3 * (W // 3)
    assert all(0 < y < H - 1 and 0 < x < W - 1 for y, x in MG.PROBES)


@pytest.mark.gpu
@pytest.mark.parametrize("probe", MG.PROBES, ids=lambda p: f"y{p[0]}x{p[1]}")
def test_gradient_is_local(probe):
    """(f) one disparity moved by +0.37: the unit gradient is bitwise unchanged outside the pixel's 3x3 block and four neighbours (a
    remainder pixel: itself and its four neighbours), and the loss does change."""
    _B, _C, H, W = ROW[PROBE_TAG][:4]
    d, lt, rt, loss, grad, _out, _ug = _run(PROBE_TAG)
    moved = gpu(MG.probe_disp(_arrays(PROBE_TAG)["disp"], probe))
    assert int((moved != d).sum()) == 1
    loss2, grad2 = _unit_grad(moved, lt, rt)
    outside = ~_footprint(H, W, *probe)
    assert _same_bits(grad2[0].cpu()[outside], grad[0].cpu()[outside])
    assert float(loss2) != float(loss)                         # the moved disparity did reach the kernel


@pytest.mark.gpu
@pytest.mark.parametrize("value", (1e30, -1e30, math.inf, math.nan), ids=("p1e30", "m1e30", "inf", "nan"))
def test_out_of_range_disparity_selects_no_taps(value):
    """(g) one interior disparity set to a huge, infinite or NaN value: warp_px selects its taps on the clamped corner, so the call
    returns, a finite huge value keeps the loss finite, and outside that pixel's footprint the gradient is the clean run's."""
    _B, _C, H, W = ROW[PROBE_TAG][:4]
    d, lt, rt, _loss, grad, _out, _ug = _run(PROBE_TAG)
    y, x = MG.PROBES[0]
    bad = d.detach().clone()
    bad[0, y, x] = value
    loss2, grad2 = _unit_grad(bad, lt, rt)
    torch.cuda.synchronize()
    if math.isfinite(value):
        assert math.isfinite(float(loss2))
    outside = ~_footprint(H, W, y, x)
    assert _same_bits(grad2[0].cpu()[outside], grad[0].cpu()[outside])
