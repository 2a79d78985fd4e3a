"""The weighted self-supervised loss (rag_amd/csrc/selfsup_loss.hip; rag_amd.metrics.re_and_sm_loss(..., weight=)) against
its plain-torch twin re_and_sm_loss_torch(..., weight=) in float64, on the remainder and workgroup-boundary rows of
test_selfsup_sweep.py (tests/golden/g14_selfsup_edges.npz: inputs 1e-3 clear of each of the loss's kinks, which the weight, a constant
factor per pixel, does not move).

  L1 = sum w |left - left_est| / (C sum w),  SSIM = sum wb term / (C sum wb) with wb = avg_pool2d(w, 3),  smoothness unweighted,
  total = 0.85 SSIM + 0.15 L1 + 0.1 smooth;  a term whose weights sum to 0 is 0, and so is its gradient.

Gates.  Loss and terms: 1e-5 relative (a term that is 0 by definition must be 0).  Gradient: max |err| <= 4 x err_twin32 + 1e-5
max|grad64| over every pixel, err_twin32 the twin's own float32 run against its float64 run.  All-ones weight against the unweighted
kernel: loss within 1e-6 relative, gradient under the same rule.  Same arithmetic twice: bit for bit.

Measured on the MI355X, gradient error as a fraction of max|grad64| (kernel / the twin's float32), mask, fraction, ones, zeros:
  B1C3_3x3    3.5e-7 / 5.6e-7   4.1e-8 / 4.1e-8   6.6e-8 / 1.4e-7   7.4e-8 / 8.5e-8
  B2C2_5x4    5.6e-8 / 1.6e-7   7.0e-8 / 3.4e-7   5.0e-8 / 2.9e-7   9.1e-8 / 8.3e-8
  B1C3_7x10   1.6e-6 / 4.4e-6   1.3e-6 / 4.3e-6   1.2e-6 / 4.1e-6   9.5e-8 / 7.8e-8
  B1C4_6x9    6.4e-7 / 7.0e-7   6.5e-7 / 7.4e-7   6.8e-7 / 7.4e-7   6.6e-8 / 1.1e-7
  B3C3_16x17  2.2e-6 / 2.1e-6   4.0e-6 / 4.0e-6   4.1e-6 / 4.1e-6   1.2e-7 / 1.4e-7
  B1C1_17x41  1.7e-6 / 2.0e-6   1.2e-6 / 1.2e-6   1.4e-6 / 1.7e-6   1.0e-7 / 9.3e-8
Worst loss error 5.1e-8.  All-ones weight against the unweighted kernel: gradient difference 0 to 1.2e-8 of max|grad64|.

Unmarked tests run without a GPU; the rest need the MI355X."""
import ctypes
import functools

import pytest
import torch

from conftest import load_golden

DEV = "cuda:0"
NOISE, FLOOR = 4.0, 1e-5
TAGS = ("B1C3_3x3", "B2C2_5x4", "B1C3_7x10", "B1C4_6x9", "B3C3_16x17", "B1C1_17x41")
SHAPES = {"B1C3_3x3": (1, 3, 3, 3), "B2C2_5x4": (2, 2, 5, 4), "B1C3_7x10": (1, 3, 7, 10), "B1C4_6x9": (1, 4, 6, 9),
          "B3C3_16x17": (3, 3, 16, 17), "B1C1_17x41": (1, 1, 17, 41)}
KINDS = ("mask", "fraction", "ones", "zeros")


@functools.lru_cache(maxsize=None)
def _inputs(tag):
    g = load_golden("g14_selfsup_edges")
    return tuple(torch.from_numpy(g[f"{tag}::{k}"]) for k in ("disp", "left", "right"))


def weight_of(tag, kind):
    """[B, H, W] float32: a 0/1 mask (about two in three kept; both values present, also inside the SSIM blocks), a fractional weight in
    {0, 1/8, ..., 1}, all ones, all zeros."""
    B, _C, H, W = SHAPES[tag]
    g = torch.Generator().manual_seed(100 * TAGS.index(tag) + KINDS.index(kind))
    if kind == "ones":
        return torch.ones((B, H, W))
    if kind == "zeros":
        return torch.zeros((B, H, W))
    if kind == "fraction":
        return torch.randint(0, 9, (B, H, W), generator=g).float() / 8
    w = (torch.rand((B, H, W), generator=g) < 0.67).float()
    w[0, 0, 0], w[0, 1, 1] = 1.0, 0.0
    return w


@functools.lru_cache(maxsize=None)
def _twin(tag, kind, dtype):
    """(loss, terms[3], gradient) of the twin in `dtype` on the CPU; kind None: the unweighted twin."""
    from rag_amd.metrics import re_and_sm_loss_torch
    disp, left, right = _inputs(tag)
    d = disp.detach().to(dtype).clone().requires_grad_(True)          # a copy: the shared fixture tensor never requires grad
    w = weight_of(tag, kind).to(dtype) if kind is not None else None
    loss, terms = re_and_sm_loss_torch(d, left.to(dtype), right.to(dtype), w)
    loss.backward()
    return loss.detach(), torch.stack([t.detach() for t in terms]), d.grad


# --------------------------------------------------------------------------- CPU
def test_inputs_are_the_sweeps_rows():
    for tag in TAGS:
        disp, left, right = _inputs(tag)
        B, C, H, W = SHAPES[tag]
        assert left.shape == right.shape == (B, C, H, W) and disp.shape == (B, H, W) and disp.dtype == torch.float32
    for tag in TAGS:
        for kind in ("mask", "fraction"):
            w = weight_of(tag, kind)
            H, W = SHAPES[tag][2:]
            inside = w[:, :3 * (H // 3), :3 * (W // 3)]
            assert float(w.min()) == 0 and float(w.max()) == 1 and float(inside.sum()) > 0 and bool(torch.isfinite(w).all())
    assert any(0 < float(v) < 1 for v in weight_of("B3C3_16x17", "fraction").flatten())


@pytest.mark.parametrize("tag", TAGS)
def test_twin_all_ones_equals_unweighted_twin(tag):
    """weight = 1 in re_and_sm_loss_torch equals the unweighted twin to float64 rounding: loss, terms and gradient."""
    loss1, terms1, grad1 = _twin(tag, "ones", torch.float64)
    loss0, terms0, grad0 = _twin(tag, None, torch.float64)
    assert abs(float(loss1 - loss0)) <= 1e-13 * abs(float(loss0))
    assert float((terms1 - terms0).abs().max()) <= 1e-13 * float(terms0.abs().max())
    assert float((grad1 - grad0).abs().max()) <= 1e-13 * float(grad0.abs().max())


@pytest.mark.parametrize("tag", TAGS)
def test_twin_all_zeros_is_the_smoothness_term(tag):
    """weight = 0: SSIM = L1 = 0 (never 0 / 0), the loss is 0.1 x smoothness, finite, with a finite gradient (the smoothness term's)."""
    loss, terms, grad = _twin(tag, "zeros", torch.float64)
    _loss0, terms0, _grad0 = _twin(tag, None, torch.float64)
    assert float(terms[0]) == 0 and float(terms[1]) == 0 and float(terms[2]) == float(terms0[2]) > 0
    assert float(loss) == pytest.approx(0.1 * float(terms[2]), rel=1e-15) and bool(torch.isfinite(loss))
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    disp, left, _right = _inputs(tag)
    d = disp.double().requires_grad_(True)
    lt = left.double()
    B, _C, H, W = SHAPES[tag]
    wx = torch.exp(-(lt[..., :, :-1] - lt[..., :, 1:]).mean(1).abs())
    wy = torch.exp(-(lt[..., :-1, :] - lt[..., 1:, :]).mean(1).abs())
    (0.1 * (((d[..., :, :-1] - d[..., :, 1:]).abs() * wx).sum() + ((d[..., :-1, :] - d[..., 1:, :]).abs() * wy).sum()) / (B * H * W)).backward()
    assert float((grad - d.grad).abs().max()) <= 1e-13 * float(d.grad.abs().max())


def test_twin_is_the_references_masked_mean():
    """L1 against the reference's mean_l1(x, y, mask) form written out, with the mask broadcast over the channels, and SSIM against
    the block-weighted mean written out; no gradient reaches the weight."""
    import torch.nn.functional as F
    from rag_amd.metrics import re_and_sm_loss_torch
    tag = "B3C3_16x17"
    disp, left, right = (t.double() for t in _inputs(tag))
    w = weight_of(tag, "fraction").double().requires_grad_(True)
    _loss, (ssim, l1, _sm) = re_and_sm_loss_torch(disp, left, right, w)
    assert not ssim.requires_grad and not l1.requires_grad                     # the weight is a constant
    _l0, (ssim0, l10, _s0) = re_and_sm_loss_torch(disp, left, right, torch.ones_like(w))
    assert float(ssim) != float(ssim0) and float(l1) != float(l10)
    # recover the per-pixel |left - est| and the per-block term from one-hot weights, then apply the definition
    B, C, H, W = SHAPES[tag]
    one = torch.zeros((B, H, W), dtype=torch.float64)
    one[1, 4, 7] = 1.0
    _l, (s_blk, a_px, _s) = re_and_sm_loss_torch(disp, left, right, one)        # L1 = mean_c |.| at (1, 4, 7); SSIM = its block's mean term
    two = torch.zeros((B, H, W), dtype=torch.float64)
    two[1, 4, 7], two[2, 0, 16] = 1.0, 3.0                                      # (2, 0, 16): a remainder column, outside every block
    _l, (s2, a2, _s) = re_and_sm_loss_torch(disp, left, right, two)
    _l, (_s3, a_rem, _s) = re_and_sm_loss_torch(disp, left, right, (two == 3).double())
    assert float(a2) == pytest.approx((float(a_px) + 3 * float(a_rem)) / 4, rel=1e-12)
    assert float(s2) == pytest.approx(float(s_blk), rel=1e-12)                  # the remainder pixel has no block: wb is unchanged
    assert float(F.avg_pool2d(two[:, None], 3).sum()) == pytest.approx(1 / 9)


def test_weighted_abi_validates_before_launch():
    """Argument checks of ragmi_selfsup_loss_weighted_fwd run before any launch (pointers are never dereferenced)."""
    import rag_amd
    lib = rag_amd.load_library()
    fake = ctypes.c_void_p(0x1000)
    # wsum[2] + 2 pre-pass partials per slot + 3 main partials per slot, in doubles (two floats each)
    assert lib.ragmi_selfsup_loss_weighted_workspace_elems(1, 3, 3) == 2 * (2 + 2 * 1 + 3 * 1)
    assert lib.ragmi_selfsup_loss_weighted_workspace_elems(8, 192, 384) == 2 * (2 + 2 * 256 + 3 * (8 * 64 * 128 // 64))
    assert lib.ragmi_selfsup_loss_weighted_workspace_elems(1, 2, 8) == 0
    f = lib.ragmi_selfsup_loss_weighted_fwd
    assert f(fake, fake, fake, fake, 1, 3, 2, 8, 0, fake, fake, None, None) == -1        # H < 3
    assert b"H, W >= 3" in lib.ragmi_last_error()
    assert f(fake, fake, fake, fake, 1, 5, 6, 8, 0, fake, fake, None, None) == -2        # C = 5
    assert f(fake, fake, fake, fake, 1, 3, 6, 8, 1, fake, fake, None, None) == -2        # bf16
    assert b"float32" in lib.ragmi_last_error()
    assert f(fake, fake, fake, None, 1, 3, 6, 8, 0, fake, fake, None, None) == -1        # no weight
    assert f(fake, fake, fake, fake, 1, 3, 6, 8, 0, ctypes.c_void_p(0x1004), fake, None, None) == -1
    assert b"aligned" in lib.ragmi_last_error()
    assert lib.ragmi_selfsup_loss_weighted_bwd(fake, fake, fake, 0, None) == -1


def test_weight_argument_is_checked():
    from rag_amd.metrics import re_and_sm_loss
    with pytest.raises(RuntimeError, match="CPU"):
        re_and_sm_loss(torch.zeros(1, 3, 3), torch.zeros(1, 1, 3, 3), torch.zeros(1, 1, 3, 3), torch.ones(1, 3, 3))


# --------------------------------------------------------------------------- GPU
def _same_bits(a, b):
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def _run(tag, kind):
    """One run per (row, weight), shared and never modified: (loss, gradient) through .backward() and the logging vector; kind None:
    the unweighted kernel."""
    from rag_amd import metrics
    disp, left, right = (t.to(DEV) for t in _inputs(tag))
    w = weight_of(tag, kind).to(DEV) if kind is not None else None
    d = disp.clone().requires_grad_(True)
    loss = metrics.re_and_sm_loss(d, left, right, w)
    loss.backward()
    terms = metrics.self_supervised_terms(disp, left, right, w)
    torch.cuda.synchronize()
    return disp, left, right, w, loss.detach(), d.grad, terms


def _grad_gate(grad, tag, kind, ref64=None):
    """max |grad - ref64| <= 4 x max |twin32 - twin64| + 1e-5 max |twin64| over every pixel -> (err, yardstick, max |grad64|)"""
    _l64, _t64, g64 = _twin(tag, kind, torch.float64)
    _l32, _t32, g32 = _twin(tag, kind, torch.float32)
    yard, gmax = float((g32.double() - g64).abs().max()), float(g64.abs().max())
    ref = g64 if ref64 is None else ref64
    err = float((grad.cpu().double() - ref).abs().max())
    return err, yard, gmax


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag", TAGS)
def test_weighted_loss_and_gradient_vs_fp64_twin(tag, kind):
    _disp, _left, _right, _w, loss, grad, terms = _run(tag, kind)
    l64, t64, _g64 = _twin(tag, kind, torch.float64)
    got = terms.cpu().double()
    err, yard, gmax = _grad_gate(grad, tag, kind)
    e_loss = abs(float(loss) - float(l64)) / abs(float(l64))
    e_terms = [abs(float(g) - float(w)) / abs(float(w)) if float(w) != 0 else abs(float(g)) for g, w in zip(got[1:], t64)]
    print(f"SELFSUPW case={tag}/{kind} e_kernel={err / gmax:.2e} e_twin32={yard / gmax:.2e} bound={(NOISE * yard + FLOOR * gmax) / gmax:.2e} "
          f"e_loss={e_loss:.1e} e_terms={[f'{v:.1e}' for v in e_terms]}")
    assert _same_bits(loss.reshape(1), terms[:1])                              # GRAD = true and GRAD = false: the same loss bits
    assert e_loss <= 1e-5 and max(e_terms) <= 1e-5, (e_loss, e_terms)
    if kind == "zeros":
        assert float(got[1]) == 0 and float(got[2]) == 0
    assert grad.shape == _g64.shape and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(terms).all())
    assert err <= NOISE * yard + FLOOR * gmax, (err / gmax, yard / gmax)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_all_ones_weight_equals_unweighted_kernel(tag):
    _d, _l, _r, _w, loss1, grad1, terms1 = _run(tag, "ones")
    _d, _l, _r, _none, loss0, grad0, terms0 = _run(tag, None)
    assert abs(float(loss1) - float(loss0)) <= 1e-6 * abs(float(loss0))
    assert float((terms1 - terms0).abs().max()) <= 1e-6 * float(terms0.abs().max())
    err, yard, gmax = _grad_gate(grad1, tag, "ones", ref64=grad0.cpu().double())
    print(f"SELFSUPW ones-vs-plain case={tag} e={err / gmax:.2e} e_twin32={yard / gmax:.2e}")
    assert err <= NOISE * yard + FLOOR * gmax


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_all_zeros_weight_leaves_the_smoothness_gradient(tag):
    """Finite everywhere, and the gradient is that of 0.1 x smoothness alone (the float64 twin's at weight 0 is exactly that:
    test_twin_all_zeros_is_the_smoothness_term)."""
    _d, _l, _r, _w, loss, grad, terms = _run(tag, "zeros")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    assert float(terms[0]) == pytest.approx(0.1 * float(terms[3]), rel=1e-6)
    err, yard, gmax = _grad_gate(grad, tag, "zeros")
    assert err <= NOISE * yard + FLOOR * gmax


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("mask", "fraction"))
@pytest.mark.parametrize("tag", TAGS)
def test_raw_call_is_deterministic_and_overwrites_nan(tag, kind):
    """ragmi_selfsup_loss_weighted_fwd on workspace, out and unit_grad pre-filled with NaN, twice: everything is written, and both runs
    are the wrapper's bits."""
    import rag_amd
    lib = rag_amd.load_library()
    B, C, H, W = SHAPES[tag]
    disp, left, right, w, loss, grad, terms = _run(tag, kind)
    nan = float("nan")
    runs = []
    for _ in range(2):
        ws = torch.full((lib.ragmi_selfsup_loss_weighted_workspace_elems(B, H, W),), nan, device=DEV)
        out, ug = torch.full((4,), nan, device=DEV), torch.full((B, H, W), nan, device=DEV)
        rc = lib.ragmi_selfsup_loss_weighted_fwd(left.data_ptr(), right.data_ptr(), disp.data_ptr(), w.data_ptr(), B, C, H, W, 0,
                                                 ws.data_ptr(), out.data_ptr(), ug.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ragmi_last_error()
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(ug).any())
        runs.append((out, ug))
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])
    assert _same_bits(runs[0][0], terms) and _same_bits(runs[0][1], grad) and _same_bits(runs[0][0][:1], loss.reshape(1))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("mask", "fraction"))
@pytest.mark.parametrize("tag", TAGS)
def test_terms_kernel_equals_gradient_kernel_bitwise(tag, kind):
    """The terms-only instantiation (self_supervised_terms) returns the four floats of the raw call that also writes the gradient, bit
    for bit: test_selfsup_sweep.py's property of the plain form, for the weighted one."""
    from rag_amd import metrics
    disp, left, right, w, _loss, grad, terms = _run(tag, kind)
    out, ug = metrics._selfsup_raw(disp, left, right, True, w)
    torch.cuda.synchronize()
    assert _same_bits(out, terms) and _same_bits(ug, grad)


@pytest.mark.gpu
def test_backward_scales_and_weight_gets_no_gradient():
    from rag_amd import metrics
    tag = "B3C3_16x17"
    disp, left, right, w, _loss, grad, _terms = _run(tag, "fraction")
    d, w2 = disp.clone().requires_grad_(True), w.clone().requires_grad_(True)
    metrics.re_and_sm_loss(d, left, right, w2).backward(torch.tensor(-2.5, device=DEV))
    assert w2.grad is None and _same_bits(d.grad, torch.tensor(-2.5, device=DEV) * grad)
    with pytest.raises(RuntimeError, match="float32"):
        metrics.re_and_sm_loss(disp, left, right, w.double())
    with pytest.raises(ValueError, match="weight"):
        metrics.re_and_sm_loss(disp, left, right, w[:, :-1])
