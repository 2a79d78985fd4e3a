"""Sweep of the kernels at the two ends of the stereo branch against float64: the disparity head (rag_amd/csrc/disp.hip) and its adjoint
(disp_softargmin_bwd_kernel of train.hip), the masked smooth-L1 loss and stereo metrics (metrics.hip) and the self-supervised loss
(selfsup_loss.hip).  Organised like test_depth_kernel_sweep.py: row tables at module level, unmarked tests that check the tables
themselves without a GPU, and `gpu` tests that run the rows.

References (all plain torch on the CPU in float64):
  head      trilinear F.interpolate (align_corners=False) -> softmin -> sum(p * arange(maxdisp)); tied to oracle.matching_oracle.disp_head
            run in float64 by test_disp_twin_fp64_matches_oracle; the backward is autograd through it
  metrics   _metrics_twin below, the per-image accumulators and the eight outputs of metrics.hip restated from the rules of
            oracle.matching_oracle.stereo_metrics (pinned to the reference's own numbers by test_oracle_golden.py) and tied to it by
            test_metrics_twin_matches_oracle
  selfsup   rag_amd.metrics.re_and_sm_loss_torch in float64 (pinned to the reference's fixture by test_selfsup_loss.py)

Gates.  No tolerance of the head or of the self-supervised gradient is a literal: each is 4 x the error of torch's own float32 evaluation
of the same reference on that row (the yardstick; 4 x because the kernels use the hardware exp2, fused lerps and another summation
order than ATen) plus a floor of 1e-6 of the tensor's scale, and never looser than what the fixture tests already apply
(test_disp_vs_oracle, test_disp_backward_vs_oracle).  Counts, determinism, layouts and the scaling of a gradient are compared bit for
bit.  Every GPU test prints `ENDS case=... e_kernel=... e_yard=... bound=...`.  Unmarked tests run without a GPU; the rest need the
MI355X."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import matching_oracle as O
from test_selfsup_loss import warped64

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
NOISE = 4.0                      # kernel error <= NOISE x the float32 yardstick's + floor (hardware exp2, fused lerps, summation order)
FLOOR = 1e-6                     # x maxdisp (forward) or x max|g| (backward)
# Worst figures of the sweep on the MI355X, max |. - ref64| in pixels (forward) and relative to max|g| (backward):
#   path        scale   worst e_kernel                       e_yard there   bound there
#   tiled_reg   <= 1    1.11e-4 (bf16, 3 x 195, 7 tiles)     7.70e-5        5.00e-4
#   tiled_reg   30      5.21e-3 (bf16, 24 x 69, 9 tiles)     5.21e-3        2.10e-2
#   tiled_roll  <= 1    9.08e-5 (d 65 -> 195)                6.79e-5        4.67e-4
#   tiled_roll  30      1.09e-3 (bf16, d 65 -> 195)          1.09e-3        4.55e-3
#   generic     <= 1    2.96e-4 (d 213 -> 639)               1.99e-4        1.44e-3
#   generic     30      7.96e-5 (d 8 -> 25)                  7.77e-5        3.36e-4
#   backward    <= 1    3.16e-6 (d 64, 129 x 30)             3.19e-6        1.38e-5
#   backward    30      2.71e-5 (d 64, 24 x 63)              2.74e-5        1.11e-4
# The float32 error at maxdisp 192 is ATen's own source index: 1/3 is not a float, and the kernels reproduce its arithmetic bit for bit.


def gpu(t):
    return t.to(DEV)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _lib():
    import rag_amd
    return rag_amd.load_library()


# ====================================================================================================== A. disparity head, forward
# (B, d, h, w, maxdisp, Ho, Wo, scale, dtype, path).  disp.hip chooses the tiled kernel when maxdisp == 3 d, Ho == 3 h, Wo == 3 w and
# the tap table (16 bytes per fine disparity) plus the staged cost block (d x 5 x 13 floats) fit 64 KiB of LDS; inside it d == 64 takes
# the register form and every other d the rolling window.  Everything else runs the generic online-softmax kernel.  A tile is 32 x 8
# output pixels and the tiled kernel decodes its tile from a grid padded to a multiple of 8 (one chunk of the tile list per XCD).
DISP_ROWS = (
    # ---- tiled_reg: tile counts 1, 7, 8, 8, 9, 17 and 6
    (1, 64, 1, 10, 192, 3, 30, 1.0, F32, "tiled_reg"),          # one partial tile, h = 1
    (1, 64, 1, 65, 192, 3, 195, 0.1, F32, "tiled_reg"),         # 7 tiles: the padded grid's last workgroup decodes tidx == ntile
    (3, 64, 9, 11, 192, 27, 33, 1.0, F32, "tiled_reg"),         # 2 x 4 = 8 tiles (chunk 1), the last tile column one pixel wide, B 3
    (1, 64, 3, 33, 192, 9, 99, 30.0, F32, "tiled_reg"),         # 4 x 2 = 8 tiles
    (1, 64, 8, 23, 192, 24, 69, 1.0, F32, "tiled_reg"),         # 3 x 3 = 9 tiles (chunk 2: seven padded workgroups return early)
    (1, 64, 43, 10, 192, 129, 30, 0.1, F32, "tiled_reg"),       # 1 x 17 tiles (chunk 3)
    (1, 64, 8, 21, 192, 24, 63, 30.0, F32, "tiled_reg"),        # 2 x 3 = 6 tiles
    (1, 64, 8, 23, 192, 24, 69, 30.0, BF16, "tiled_reg"),
    (3, 64, 9, 11, 192, 27, 33, 0.1, BF16, "tiled_reg"),
    (1, 64, 1, 65, 192, 3, 195, 1.0, BF16, "tiled_reg"),
    # ---- tiled_roll: d in {1, 2, 7, 63, 65}; h = 1, w = 1, h = w = 1
    (1, 1, 1, 1, 3, 3, 3, 1.0, F32, "tiled_roll"),
    (1, 1, 4, 5, 3, 12, 15, 30.0, F32, "tiled_roll"),
    (2, 2, 1, 5, 6, 3, 15, 30.0, F32, "tiled_roll"),
    (1, 2, 3, 3, 6, 9, 9, 0.1, F32, "tiled_roll"),
    (1, 7, 5, 1, 21, 15, 3, 1.0, F32, "tiled_roll"),
    (1, 7, 6, 13, 21, 18, 39, 30.0, F32, "tiled_roll"),
    (1, 63, 4, 12, 189, 12, 36, 0.1, F32, "tiled_roll"),
    (1, 65, 3, 11, 195, 9, 33, 1.0, F32, "tiled_roll"),
    (1, 65, 3, 11, 195, 9, 33, 30.0, BF16, "tiled_roll"),
    (2, 2, 1, 5, 6, 3, 15, 1.0, BF16, "tiled_roll"),
    (1, 63, 4, 12, 189, 12, 36, 1.0, BF16, "tiled_roll"),
    # ---- generic: ratios 3 d +- 1, a shrinking disparity axis, d = 1, the 3 d ratio past the LDS test, other output sizes (C ABI)
    (1, 8, 4, 6, 23, 12, 18, 1.0, F32, "generic"),
    (2, 8, 4, 6, 25, 12, 18, 30.0, F32, "generic"),
    (1, 16, 3, 5, 5, 9, 15, 1.0, F32, "generic"),               # maxdisp < d: the coarse pair moves three planes per fine sample
    (1, 16, 3, 5, 7, 9, 15, 0.1, F32, "generic"),
    (1, 1, 2, 3, 4, 6, 9, 1.0, F32, "generic"),
    (1, 213, 2, 2, 639, 6, 6, 1.0, F32, "generic"),             # 16 * 639 + 260 * 213 = 65604 > 65536
    (1, 8, 4, 6, 24, 9, 6, 1.0, F32, "generic"),                # Ho = 2 h + 1, Wo = w
    (1, 8, 4, 6, 24, 4, 24, 30.0, F32, "generic"),              # Ho = h, Wo = 4 w
    (1, 213, 2, 2, 639, 6, 6, 0.1, BF16, "generic"),
    (1, 16, 3, 5, 5, 9, 15, 30.0, BF16, "generic"),
    (1, 8, 4, 6, 24, 9, 6, 1.0, BF16, "generic"),
)
PATHS = ("tiled_reg", "tiled_roll", "generic")


def _did(row):
    return "B{}d{}_{}x{}_D{}_{}x{}_s{}_{}_{}".format(*row[:8], "bf16" if row[8] == BF16 else "f32", row[9])


def _path_of(row):
    """The label disp.hip's dispatch gives the row, restated as arithmetic."""
    _B, d, h, w, maxdisp, Ho, Wo = row[:7]
    tiled = maxdisp == 3 * d and Ho == 3 * h and Wo == 3 * w and 16 * maxdisp + 4 * 65 * d <= 65536
    return ("tiled_reg" if d == 64 else "tiled_roll") if tiled else "generic"


def _tiles(row):
    return -(-row[6] // 32) * -(-row[5] // 8)


def _disp_twin(cost, maxdisp, Ho, Wo):
    """The head in cost's dtype: [B, d, h, w] -> [B, Ho, Wo]."""
    v = F.interpolate(cost[:, None], (maxdisp, Ho, Wo), mode="trilinear", align_corners=False)[:, 0]
    return (F.softmin(v, dim=1) * torch.arange(maxdisp, dtype=cost.dtype).view(1, -1, 1, 1)).sum(1)


def _disp_yard(cost32, maxdisp, Ho, Wo):
    """The float32 restatement of the reference on the CPU: oracle.disp_head where it applies (Ho = 3 h, Wo = 3 w), the same ATen calls
    through the twin at the two other output sizes."""
    if (Ho, Wo) == (3 * cost32.shape[2], 3 * cost32.shape[3]):
        return O.disp_head(cost32[:, None], maxdisp)
    return _disp_twin(cost32, maxdisp, Ho, Wo)


def _cost_of(row):
    B, d, h, w, _m, _ho, _wo, scale, dtype, _p = row
    cost = torch.randn((B, d, h, w), generator=gen(8100 + DISP_ROWS.index(row))) * scale
    return cost.to(dtype)        # bf16 storage: the rounded values are what the kernel and the twin both see


@functools.lru_cache(maxsize=None)
def _disp_case(row):
    """(cost in the row's dtype, float64 twin, float32 yardstick), computed once per module."""
    cost = _cost_of(row)
    maxdisp, Ho, Wo = row[4:7]
    return cost, _disp_twin(cost.double(), maxdisp, Ho, Wo), _disp_yard(cost.float(), maxdisp, Ho, Wo)


def _fwd_bound(row, e_yard):
    maxdisp, scale = row[4], row[7]
    bound = NOISE * e_yard + FLOOR * maxdisp
    if scale < 30:               # test_disp_vs_oracle's atol; above, the error grows with the cost (argued there)
        bound = min(bound, 2e-4 * max(1.0, maxdisp / 48))
    return bound


# ------------------------------------------------------------------------------------------------------ CPU: the table
def test_disp_table_reaches_every_path():
    assert len(set(DISP_ROWS)) == len(DISP_ROWS)
    assert {r[9] for r in DISP_ROWS} == set(PATHS)
    for r in DISP_ROWS:
        assert _path_of(r) == r[9], r
    for p in PATHS:
        rows = [r for r in DISP_ROWS if r[9] == p]
        assert {r[8] for r in rows} == {F32, BF16}, p
        assert {r[7] for r in rows} == {0.1, 1.0, 30.0}, p
    reg = [r for r in DISP_ROWS if r[9] == "tiled_reg"]
    assert {1, 7, 8, 9, 17} <= {_tiles(r) for r in reg}
    assert {30, 33, 63, 99} <= {r[6] for r in reg} and {3, 9, 24, 27} <= {r[5] for r in reg}
    assert {1, 3} <= {r[0] for r in reg}
    roll = [r for r in DISP_ROWS if r[9] == "tiled_roll"]
    assert {r[1] for r in roll} == {1, 2, 7, 63, 65}
    assert any(r[2] == 1 and r[3] > 1 for r in roll) and any(r[3] == 1 and r[2] > 1 for r in roll) and any(r[2] == r[3] == 1 for r in roll)
    g = [r for r in DISP_ROWS if r[9] == "generic"]
    assert any(r[4] == 3 * r[1] + 1 for r in g) and any(r[4] == 3 * r[1] - 1 for r in g)
    assert any(r[4] < r[1] for r in g) and (1, 16, 3, 5, 5, 9, 15, 1.0, F32, "generic") in g
    assert any(r[1] == 213 and r[4] == 639 and r[2] == r[3] == 2 for r in g)                 # 3 d, through the LDS test
    assert 16 * 636 + 260 * 212 <= 65536 < 16 * 639 + 260 * 213                             # and d = 213 is the first to fall through
    assert any(r[5] == 2 * r[2] + 1 and r[6] == r[3] for r in g) and any(r[5] == r[2] and r[6] == 4 * r[3] for r in g)
    assert all(r[0] * r[4] * r[5] * r[6] <= 1 << 21 for r in DISP_ROWS)                      # the upsampled volume stays small


def test_disp_twin_fp64_matches_oracle():
    """The twin in float64 == oracle.matching_oracle.disp_head run in float64, on the odd-sized rolling-window row."""
    row = (1, 7, 6, 13, 21, 18, 39, 30.0, F32, "tiled_roll")
    cost, ref, _yard = _disp_case(row)
    want = O.disp_head(cost.double()[:, None], row[4])
    assert want.dtype == torch.float64 and float((ref - want).abs().max()) <= 1e-12 * row[4]


@pytest.mark.parametrize("row", DISP_ROWS, ids=_did)
def test_disp_row_yardstick_is_finite(row):
    """Every row's reference and yardstick are finite, the output spans part of [0, maxdisp) and the bound is positive."""
    _cost, ref, yard = _disp_case(row)
    assert torch.isfinite(ref).all() and torch.isfinite(yard).all()
    assert 0.0 <= float(ref.min()) and float(ref.max()) <= row[4] - 1
    e_yard = float((yard.double() - ref).abs().max())
    print(f"ENDS-CPU case={_did(row)} e_yard={e_yard:.3e} bound={_fwd_bound(row, e_yard):.3e}")
    assert e_yard <= 5e-6 * max(1.0, row[7]) * row[4]            # ATen's own float32 is no further than this: the row is well-conditioned


# ------------------------------------------------------------------------------------------------------ CPU: refusals
FAKE = ctypes.c_void_p(0x1000)


def _fwd_status(B=1, d=8, h=4, w=6, maxdisp=24, Ho=12, Wo=18):
    lib = _lib()
    return lib.ragmi_disp_softargmin_fwd(FAKE, FAKE, B, d, h, w, maxdisp, Ho, Wo, 0, None), lib.ragmi_last_error()


def _bwd_status(B=1, d=8, h=4, w=6, maxdisp=24, Ho=12, Wo=18):
    lib = _lib()
    return lib.ragmi_disp_softargmin_bwd(FAKE, FAKE, FAKE, B, d, h, w, maxdisp, Ho, Wo, None), lib.ragmi_last_error()


def test_disp_abi_refuses_before_launch():
    """Status and text of every refusal; the pointers are never dereferenced (no launch happens)."""
    st, msg = _fwd_status(maxdisp=4097)
    assert st == -2 and b"maxdisp 4097 exceeds the tap table (4096)" in msg
    st, msg = _bwd_status(maxdisp=3073)
    assert st == -2 and b"maxdisp = 3073 exceeds the tap table (3072)" in msg
    for bad in (dict(Ho=13), dict(Wo=17), dict(Ho=9, Wo=6), dict(Ho=4, Wo=24)):
        st, msg = _bwd_status(**bad)
        assert st == -2 and b"Ho = 3h, Wo = 3w" in msg, bad
    for name in ("B", "d", "h", "w", "maxdisp", "Ho", "Wo"):
        for v in (0, -1):
            st, msg = _fwd_status(**{name: v})
            assert st == -1 and b"disp_softargmin: non-positive size" in msg, (name, v)
            st, msg = _bwd_status(**{name: v})
            assert st == -1 and b"disp_softargmin_bwd: bad size" in msg, (name, v)
    st, msg = _fwd_status(B=65536)
    assert st == -2 and b"disp_softargmin: size too large" in msg
    st, msg = _bwd_status(B=65536)
    assert st == -1 and b"disp_softargmin_bwd: bad size" in msg
    lib = _lib()
    assert lib.ragmi_disp_softargmin_fwd(None, FAKE, 1, 8, 4, 6, 24, 12, 18, 0, None) == -1 and b"null pointer" in lib.ragmi_last_error()
    assert lib.ragmi_disp_softargmin_bwd(FAKE, None, FAKE, 1, 8, 4, 6, 24, 12, 18, None) == -1 and b"null pointer" in lib.ragmi_last_error()
    assert lib.ragmi_disp_softargmin_fwd(FAKE, FAKE, 1, 8, 4, 6, 24, 12, 18, 7, None) == -2 and b"dtype 7 not built" in lib.ragmi_last_error()


# ------------------------------------------------------------------------------------------------------ GPU: forward
def _disp_fwd(cost, maxdisp, Ho, Wo):
    """ops.disp_softargmin where it applies (Ho = 3 h, Wo = 3 w), the C ABI directly at the other output sizes."""
    from rag_amd import _lib as L, ops
    B, d, h, w = cost.shape
    if (Ho, Wo) == (3 * h, 3 * w):
        return ops.disp_softargmin(cost, maxdisp)
    out = torch.empty((B, Ho, Wo), device=cost.device, dtype=torch.float32)
    L.check(L.load_library().ragmi_disp_softargmin_fwd(cost.data_ptr(), out.data_ptr(), B, d, h, w, maxdisp, Ho, Wo, ops._DT[cost.dtype],
                                                       ops._stream()), "disp_softargmin")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("row", DISP_ROWS, ids=_did)
def test_disp_fwd_vs_fp64(row):
    cost, ref, yard = _disp_case(row)
    maxdisp, Ho, Wo = row[4:7]
    dev = gpu(cost).contiguous()
    out, again = _disp_fwd(dev, maxdisp, Ho, Wo), _disp_fwd(dev, maxdisp, Ho, Wo)
    torch.cuda.synchronize()
    assert out.shape == ref.shape and out.dtype == torch.float32
    e_kernel = float((out.cpu().double() - ref).abs().max())
    e_yard = float((yard.double() - ref).abs().max())
    bound = _fwd_bound(row, e_yard)
    print(f"ENDS case={_did(row)} tiles={_tiles(row)} e_kernel={e_kernel:.3e} e_yard={e_yard:.3e} bound={bound:.3e}")
    assert torch.isfinite(out).all()
    assert e_kernel <= bound, (e_kernel, e_yard, bound)
    assert torch.equal(out, again)


# ====================================================================================================== B. disparity head, backward
# (B, d, h, w, maxdisp, scale): the Ho = 3 h rows of A in float32, rows whose (Ho, Wo) sit either side of the adjoint's 16 x 16 tile
# (15, 18, 33, 48), and d = 64 at B = 2.
BWD_EXTRA = ((1, 8, 5, 6, 24, 1.0), (1, 8, 6, 5, 24, 1.0), (1, 8, 11, 16, 24, 1.0), (1, 8, 16, 11, 24, 30.0), (2, 64, 4, 6, 192, 1.0))
BWD_ROWS = tuple(dict.fromkeys(tuple(r[:5]) + (r[7],) for r in DISP_ROWS if r[8] == F32 and (r[5], r[6]) == (3 * r[2], 3 * r[3]))) + BWD_EXTRA
# a bit-for-bit comparison of two runs needs a deterministic sum: the adjoint adds one partial per tile to a coarse cell with float
# atomics, and only up to two partials (0 + a + b) add to the same bits in either order
BWD_TWO_TILES = tuple(r for r in BWD_ROWS if -(-3 * r[2] // 16) * -(-3 * r[3] // 16) <= 2 and r[0] == 1)


def _bid(row):
    return "B{}d{}_{}x{}_D{}_s{}".format(*row)


def _bwd_inputs(row):
    B, d, h, w, _maxdisp, scale = row
    g = gen(8600 + BWD_ROWS.index(row))
    return torch.randn((B, d, h, w), generator=g) * scale, torch.randn((B, 3 * h, 3 * w), generator=g)


def _corner_dout(row):
    """A single 1 at each of the four output corners of the last image, zero elsewhere."""
    B, _d, h, w = row[:4]
    dout = torch.zeros((B, 3 * h, 3 * w))
    for y in (0, -1):
        for x in (0, -1):
            dout[B - 1, y, x] = 1.0
    return dout


def _twin_grad(cost, dout, maxdisp, dtype):
    c = cost.detach().clone().to(dtype).requires_grad_(True)
    _disp_twin(c, maxdisp, dout.shape[1], dout.shape[2]).backward(dout.to(dtype))
    return c.grad


@functools.lru_cache(maxsize=None)
def _bwd_case(row, variant):
    cost, dout = _bwd_inputs(row)
    if variant == "corners":
        dout = _corner_dout(row)
    return cost, dout, _twin_grad(cost, dout, row[4], torch.float64), _twin_grad(cost, dout, row[4], torch.float32)


def _bwd_gate(case, got, ref, yard, dout):
    """max|g| is the float64 gradient's; where that gradient is zero (d = 1: every fine sample is the one coarse plane, so the expectation
    does not depend on the cost) the scale of the floor is max|dout|, which bounds every term of the adjoint's sums."""
    gmax = float(ref.abs().max())
    if gmax <= 1e-12 * float(dout.abs().max()):
        gmax = float(dout.abs().max())
    e_kernel, e_yard = float((got.cpu().double() - ref).abs().max()), float((yard.double() - ref).abs().max())
    bound = min(NOISE * e_yard + FLOOR * gmax, 2e-4 * max(1.0, gmax))        # test_hip_train.py::close at 2e-4 is the ceiling
    print(f"ENDS case={case} tensor=dcost e_kernel={e_kernel / gmax:.3e} e_yard={e_yard / gmax:.3e} bound={bound / gmax:.3e} max|g|={gmax:.3e}")
    assert e_kernel <= bound, (case, e_kernel, e_yard, bound)


def test_bwd_table_covers_the_tile_edges():
    assert len(set(BWD_ROWS)) == len(BWD_ROWS)
    sizes = {(3 * r[2], 3 * r[3]) for r in BWD_ROWS}
    assert {(15, 18), (18, 15), (33, 48), (48, 33)} <= sizes
    assert any(r[1] == 64 and r[0] == 2 for r in BWD_ROWS)
    assert {r[1] for r in BWD_ROWS} >= {1, 2, 7, 63, 64, 65, 213} and any(r[4] < r[1] for r in BWD_ROWS)
    assert all(r[4] <= 3072 for r in BWD_ROWS)
    assert len(BWD_TWO_TILES) >= 4 and any(-(-3 * r[2] // 16) * -(-3 * r[3] // 16) == 2 for r in BWD_TWO_TILES)
    for r in BWD_ROWS[:3]:
        _c, _do, ref, yard = _bwd_case(r, "random")
        assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0 and torch.isfinite(yard).all()


@pytest.mark.gpu
@pytest.mark.parametrize("row", BWD_ROWS, ids=_bid)
def test_disp_bwd_random_dout_vs_fp64_autograd(row):
    from rag_amd import ops
    cost, dout, ref, yard = _bwd_case(row, "random")
    got = ops.disp_softargmin_bwd(gpu(cost), gpu(dout), row[4])
    torch.cuda.synchronize()
    assert got.shape == cost.shape
    _bwd_gate(_bid(row), got, ref, yard, dout)


@pytest.mark.gpu
@pytest.mark.parametrize("row", BWD_ROWS, ids=_bid)
def test_disp_bwd_zero_and_corner_dout(row):
    """An all-zero dout gives exactly zero.  A dout with a single 1 at each of the four output corners (of the last image) passes the gate
    of its own yardstick, and the other images get exactly nothing.  The four corners share one dout, hence one max|g|: gated alone, a
    corner pixel with a peaky softmin (scale 30) has a gradient that is the rounding of `out` itself, and torch's own float32 gradient is
    100 % of max|g| off float64 there (measured at the bottom-left corner of the 24 x 63 row), so a ratio of two such errors says nothing."""
    from rag_amd import ops
    cost, dout, _ref, _yard = _bwd_case(row, "random")
    zero = ops.disp_softargmin_bwd(gpu(cost), gpu(torch.zeros_like(dout)), row[4])
    assert torch.equal(zero.cpu(), torch.zeros_like(cost))
    _c, do, ref, yard = _bwd_case(row, "corners")
    got = ops.disp_softargmin_bwd(gpu(cost), gpu(do), row[4])
    _bwd_gate(_bid(row) + "/corners", got, ref, yard, do)
    if row[0] > 1:
        assert torch.equal(got[:-1].cpu(), torch.zeros_like(cost[:-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("row", BWD_TWO_TILES, ids=_bid)
def test_disp_bwd_non_contiguous_dout(row):
    """A dout that is a transposed-then-sliced view gives the contiguous run's bits (rows of at most two tiles: see BWD_TWO_TILES)."""
    from rag_amd import ops
    cost, dout, _ref, _yard = _bwd_case(row, "random")
    big = torch.zeros((dout.shape[0], dout.shape[2] + 3, dout.shape[1] + 2))
    big[:, 1:-2, 2:] = dout.transpose(1, 2)
    view = gpu(big).transpose(1, 2)[:, 2:, 1:-2]
    assert not view.is_contiguous() and torch.equal(view.cpu(), dout)
    a = ops.disp_softargmin_bwd(gpu(cost), gpu(dout), row[4])
    b = ops.disp_softargmin_bwd(gpu(cost), view, row[4])
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_disp_autograd_function_runs_the_adjoint():
    """rag_amd.Disp under autograd at the d = 64, B = 2 row: output and gradient under the gates above."""
    import rag_amd
    row = (2, 64, 4, 6, 192, 1.0)
    cost, dout, ref, yard = _bwd_case(row, "random")
    x = gpu(cost)[:, None].requires_grad_(True)
    out = rag_amd.Disp(row[4])(x)
    out.backward(gpu(dout))
    _bwd_gate(_bid(row) + "/Disp", x.grad[:, 0], ref, yard, dout)


# ====================================================================================================== C. masked smooth-L1 and metrics
MET_SHAPES = ((1, 1, 1), (1, 1, 255), (1, 16, 16), (2, 1, 257), (1, 257, 256), (3, 1, 65537))     # the last two wrap the grid-stride loop
MET_RULES = ("nogt", "skip", "allskip", "nomask", "nomask_nogt")
MET_CASES = tuple((s, "random") for s in MET_SHAPES) + tuple(((3, 8, 40), r) for r in MET_RULES)
MET_MAXDISP = 192.0
MET_TOL = 2e-5                   # test_hip_train.py::test_stereo_metrics_vs_oracle: |got - ref| <= 2e-5 max(1, |ref|); a ceiling
EQ_MAXDISP = 96.0                # the equality case: 4 / 80 == 0.05 needs gt = 80 inside the mask


def _mid(case):
    return "B{}_{}x{}_".format(*case[0]) + case[1]


def _near_threshold(est, gt, maxdisp):
    """Pixels of the float32 inputs, evaluated in float64, within 1e-3 of a strict comparison of metrics.hip: e against 1, 2, 3; e / g
    against 0.05 (1e-4); g against 0 and maxdisp."""
    e, g = (gt.double() - est.double()).abs(), gt.double()
    near = (g.abs() < 1e-3) | ((g - maxdisp).abs() < 1e-3)
    for t in (1.0, 2.0, 3.0):
        near |= (e - t).abs() < 1e-3
    return near | ((g > 0) & ((e / g.abs().clamp_min(1e-30) - 0.05).abs() < 1e-4))


@functools.lru_cache(maxsize=None)
def _metric_inputs(case):
    """(est, gt) float32.  gt ~ U(-2, 1.1 maxdisp), est = gt +- U(0, 4.5); pixels that land near a threshold are redrawn.  Pixel (0, 0) of
    every image is masked.  The rule cases then overwrite whole images of gt (positive values >= maxdisp + 1, or values <= 0)."""
    (B, H, W), kind = case
    m = MET_MAXDISP
    g = gen(9100 + MET_CASES.index(case))
    gt = torch.rand((B, H, W), generator=g) * (1.1 * m + 2.0) - 2.0
    e = torch.rand((B, H, W), generator=g) * 4.5 * (torch.randint(0, 2, (B, H, W), generator=g) * 2 - 1)
    gt[:, 0, 0], e[:, 0, 0] = 0.37 * m, 0.5
    outside = m + 1.0 + torch.rand((B, H, W), generator=g) * 10.0
    nonpos = -torch.rand((B, H, W), generator=g) * (torch.rand((B, H, W), generator=g) < 0.7)       # 30 % exact zeros
    if kind == "nogt":
        gt[1] = nonpos[1]
    elif kind in ("skip", "allskip"):
        for b in ((1,) if kind == "skip" else range(B)):
            keep = gt[b, 0, :5].clone()
            gt[b] = outside[b]
            gt[b, 0, :5] = keep.clamp(5.0, m - 5.0)                                                # 5 of 320 positive pixels: 1.6 % < 10 %
    elif kind == "nomask":
        gt = outside
    elif kind == "nomask_nogt":
        gt = nonpos
    for _ in range(50):
        bad = _near_threshold(gt + e, gt, m)
        if not bool(bad.any()):
            break
        n = int(bad.sum())
        e[bad] = torch.rand((n,), generator=g) * 4.5 * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
        inside = bad & (gt > 0) & (gt < m)
        gt[inside] = torch.rand((int(inside.sum()),), generator=g) * (m - 2.0) + 1.0
    return gt + e, gt


@functools.lru_cache(maxsize=None)
def _equality_inputs():
    """Integer-valued floats: gt cycles over 0 .. maxdisp (both ends included, period 97), est = gt + k with k cycling over
    0, +-1, +-2, +-3, +-4 (period 9): every pair occurs, e sits ON 1, 2, 3 and e / g ON 0.05 (e = 4, g = 80).  float32 and float64
    agree exactly on every comparison, count and sum."""
    n = 2 * 7 * 63
    idx = torch.arange(n)
    gt = (idx % 97).float()
    k = torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0])[idx % 9]
    return (gt + k).reshape(2, 7, 63), gt.reshape(2, 7, 63)


def _metrics_twin(est, gt, maxdisp):
    """metrics.hip restated in est's dtype: (acc [B, 8] = n_mask, n_gt_pos, sum smooth-L1, sum |e|, n_D1, n_thr1, n_thr2, n_thr3 per image,
    out [8] = loss, EPE, D1, Thres1, Thres2, Thres3, masked pixels of the batch, images kept).  The rules are those of
    oracle.matching_oracle.stereo_metrics: an image is skipped when mask.mean() / (gt > 0).mean() < 0.1 (nan compares false: kept, and its
    means are nan); the metrics are 0 when no image is kept."""
    B, dt = est.shape[0], est.dtype
    e_, g_ = est.reshape(B, -1), gt.reshape(B, -1)
    pos = g_ > 0
    mask = pos & (g_ < maxdisp)
    e = (g_ - e_).abs()
    zero = torch.zeros_like(e)
    sl1 = torch.where(e < 1, 0.5 * e * e, e - 0.5)
    ratio = e / torch.where(mask, g_.abs(), torch.ones_like(g_))

    def count(c):
        return (c & mask).sum(1).to(dt)
    acc = torch.stack([count(mask), pos.sum(1).to(dt), torch.where(mask, sl1, zero).sum(1), torch.where(mask, e, zero).sum(1),
                       count((e > 3) & (ratio > 0.05)), count(e > 1), count(e > 2), count(e > 3)], 1)
    skip = (acc[:, 1] > 0) & (acc[:, 0] / acc[:, 1].clamp_min(1) < 0.1)
    kept = int((~skip).sum())
    out = torch.zeros((8,), dtype=dt)
    out[0] = acc[:, 2].sum() / acc[:, 0].sum()
    if kept:
        out[1:6] = (acc[~skip, 3:8] / acc[~skip, 0:1]).mean(0)
    out[6], out[7] = acc[:, 0].sum(), kept
    return acc, out


def _metric_case(case):
    if case == "equality":
        est, gt = _equality_inputs()
        return est, gt, EQ_MAXDISP
    est, gt = _metric_inputs(case)
    return est, gt, MET_MAXDISP


ALL_MET = MET_CASES + ("equality",)


def _amid(case):
    return case if isinstance(case, str) else _mid(case)


@pytest.mark.parametrize("case", MET_CASES, ids=_mid)
def test_metric_inputs_keep_clear_of_the_thresholds(case):
    """No pixel of a random case within 1e-3 of e = 1, 2, 3, of g = 0 (unless exactly <= 0: the rule cases), of g = maxdisp, or within
    1e-4 of e / g = 0.05, so a float32 evaluation cannot fall on the other side; no image's mask ratio near 0.1; and the float32 twin
    counts what the float64 twin counts."""
    est, gt = _metric_inputs(case)
    near = _near_threshold(est, gt, MET_MAXDISP)
    if case[1] in ("nogt", "nomask_nogt"):
        near &= gt > 0                                    # planted zeros and negatives are on the far side by construction (g > 0 is false)
    assert not bool(near.any()), int(near.sum())
    assert bool(((gt[:, 0, 0] > 0) & (gt[:, 0, 0] < MET_MAXDISP)).all()) or case[1] in ("nomask", "nomask_nogt", "nogt")
    acc64, out64 = _metrics_twin(est.double(), gt.double(), MET_MAXDISP)
    acc32, _out32 = _metrics_twin(est, gt, MET_MAXDISP)
    cols = [0, 1, 4, 5, 6, 7]
    assert torch.equal(acc32[:, cols].double(), acc64[:, cols])
    ratio = acc64[:, 0] / acc64[:, 1]
    assert not bool(((ratio - 0.1).abs() < 0.02).any())
    want = {"random": None, "nogt": 3, "skip": 2, "allskip": 0, "nomask": 0, "nomask_nogt": 3}[case[1]]
    if want is not None:
        assert int(out64[7]) == want
    assert (int(out64[6]) == 0) == case[1].startswith("nomask")
    if case[0][1] * case[0][2] > 65536:
        assert -(-case[0][1] * case[0][2] // 1024) > 64                                             # more work than 64 workgroups x 256 x 1 pass


@pytest.mark.parametrize("case", ALL_MET, ids=_amid)
def test_metrics_twin_matches_oracle(case):
    """The six scalars of the twin in float64 == oracle.matching_oracle.stereo_metrics on the same float64 inputs (nan where it is nan)."""
    est, gt, m = _metric_case(case)
    _acc, out = _metrics_twin(est.double(), gt.double(), m)
    ref = O.stereo_metrics(est.double(), gt.double(), m)
    want = torch.tensor([ref[k] for k in ("loss", "EPE", "D1", "Thres1", "Thres2", "Thres3")], dtype=torch.float64)
    assert torch.allclose(out[:2], want[:2], rtol=1e-12, atol=1e-12, equal_nan=True), (out[:2], want[:2])
    assert torch.allclose(out[2:6], want[2:], rtol=0, atol=1e-7, equal_nan=True), (out[2:6], want[2:])    # the oracle's ratios are float32 means
    if case != "equality" and case[1] in ("nogt", "nomask_nogt"):
        assert bool(torch.isnan(out[1:6]).all())
    if case != "equality" and case[1].startswith("nomask"):
        assert bool(torch.isnan(out[0]))


def test_equality_case_sits_on_every_threshold():
    est, gt = _equality_inputs()
    e = (gt - est).abs()
    mask = (gt > 0) & (gt < EQ_MAXDISP)
    assert float(gt.min()) == 0.0 and float(gt.max()) == EQ_MAXDISP
    for t in (1.0, 2.0, 3.0):
        assert bool(((e == t) & mask).any())
    assert bool(((e == 4.0) & (gt == 80.0)).any()) and 4.0 / 80.0 == 0.05 and bool(torch.tensor(4.0) / torch.tensor(80.0) == torch.tensor(0.05))
    assert {float(v) for v in (est - gt).unique()} == {0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0}
    a64, o64 = _metrics_twin(est.double(), gt.double(), EQ_MAXDISP)
    a32, o32 = _metrics_twin(est, gt, EQ_MAXDISP)
    assert torch.equal(a32.double(), a64) and torch.equal(o32[6:].double(), o64[6:])
    # a `>=` in place of `>` would count more: the ties exist in numbers that matter
    assert int(((e >= 3) & mask).sum()) > int(((e > 3) & mask).sum()) and int((gt >= EQ_MAXDISP).sum()) > 0 and int((gt <= 0).sum()) > 0


def _metrics_gpu(est, gt, maxdisp):
    """ragmi_stereo_metrics_fwd into a buffer of this test's own (as rag_amd.metrics._raw lays it out): acc [B, 8] and out [8]."""
    from rag_amd import _lib as L, ops
    B, H, W = est.shape
    e, g = gpu(est).contiguous(), gpu(gt).contiguous()
    buf = torch.full((B + 1, 8), 7.0, device=DEV)                       # stale values: the call zeroes its accumulators itself
    L.check(L.load_library().ragmi_stereo_metrics_fwd(e.data_ptr(), g.data_ptr(), B, H, W, float(maxdisp), buf.data_ptr(), buf[B].data_ptr(),
                                                      ops._stream()), "stereo_metrics")
    torch.cuda.synchronize()
    host = buf.cpu()
    return host[:B], host[B]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_MET, ids=_amid)
def test_metrics_vs_fp64(case):
    """Per-image counts exact; sums, loss and metrics within the ceiling of test_stereo_metrics_vs_oracle; nan exactly where the twin is."""
    import rag_amd
    est, gt, m = _metric_case(case)
    acc64, out64 = _metrics_twin(est.double(), gt.double(), m)
    acc, out = _metrics_gpu(est, gt, m)
    cols = [0, 1, 4, 5, 6, 7]
    print(f"ENDS case={_amid(case)} counts kernel={acc[:, cols].sum(0).tolist()} twin64={acc64[:, cols].sum(0).tolist()}")
    assert torch.equal(acc[:, cols].double(), acc64[:, cols])
    assert float(out[6]) == float(out64[6]) and float(out[7]) == float(out64[7])
    for name, got, ref in (("sum_sl1", acc[:, 2], acc64[:, 2]), ("sum_abs", acc[:, 3], acc64[:, 3]), ("out", out[:6], out64[:6])):
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), (name, got, ref)
        ok = ~torch.isnan(ref)
        err = (got.double() - ref)[ok].abs() / ref[ok].abs().clamp_min(1.0)
        print(f"ENDS case={_amid(case)} tensor={name} e_kernel={float(err.max()) if err.numel() else 0.0:.3e} bound={MET_TOL:.1e}")
        assert bool((err <= MET_TOL).all()), (name, got, ref)
    if case == "equality":
        assert torch.equal(acc.double(), acc64)                          # halves and integers: the float32 sums are exact too
        assert torch.equal(out, out64.float())
    again = rag_amd.metrics.stereo_metrics(gpu(est), gpu(gt), m).tensor.cpu()
    assert torch.equal(again[6:], out[6:]) and torch.equal(torch.isnan(again), torch.isnan(out))
    assert torch.allclose(again, out, rtol=1e-6, atol=0, equal_nan=True)                            # float atomics: the order is free


def _ulp32(ref):
    """Spacing of float32 at |ref| (float64 tensor)."""
    _m, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref), e - 24)


@pytest.mark.gpu
@pytest.mark.parametrize("gout", (1.0, -2.5))
@pytest.mark.parametrize("case", ALL_MET, ids=_amid)
def test_masked_smooth_l1_fwd_bwd_vs_fp64(case, gout):
    """loss as the twin's; d loss / d est == gout * clamp(est - gt, -1, 1) / n_mask on the mask and 0 off it, evaluated in float64, to
    2 ulp of float32.  With no masked pixel: a nan loss and an all-zero gradient, which is what torch gives for F.smooth_l1_loss on an
    empty selection."""
    import rag_amd
    est, gt, m = _metric_case(case)
    _acc64, out64 = _metrics_twin(est.double(), gt.double(), m)
    x = gpu(est).requires_grad_(True)
    loss = rag_amd.metrics.masked_smooth_l1(x, gpu(gt), m)
    (loss * gout).backward()
    torch.cuda.synchronize()
    grad = x.grad.cpu()
    mask = (gt > 0) & (gt < m)
    if int(mask.sum()) == 0:
        xe = est.clone().requires_grad_(True)
        ref = F.smooth_l1_loss(xe[mask], gt[mask], reduction="mean")
        (ref * gout).backward()
        assert bool(torch.isnan(ref)) and torch.equal(xe.grad, torch.zeros_like(est))
        assert bool(torch.isnan(loss)) and torch.equal(grad, torch.zeros_like(est))
        return
    assert abs(float(loss) - float(out64[0])) <= MET_TOL * max(1.0, abs(float(out64[0])))
    ref = torch.where(mask, gout * (est.double() - gt.double()).clamp(-1, 1) / out64[6], torch.zeros((), dtype=torch.float64))
    ulps = ((grad.double() - ref).abs() / _ulp32(ref))[mask]
    print(f"ENDS case={_amid(case)} gout={gout} tensor=dest worst={float(ulps.max()):.2f} ulp")
    assert float(ulps.max()) <= 2.0
    assert torch.equal(grad[~mask], torch.zeros_like(grad[~mask]))


# ====================================================================================================== D. self-supervised loss
# (B, C, H, W, regime).  One thread owns one 3 x 3 SSIM block for all channels; the last block row / column owns the H % 3 / W % 3
# remainder; 64 threads per workgroup, one slot of partials per workgroup, the finalize kernel strides over the slots by 256.
SS_ROWS = (
    (1, 3, 3, 3, "inview"),          # one thread
    (2, 1, 3, 5, "negative"),
    (1, 2, 5, 3, "inview"),
    (2, 4, 4, 4, "outview"),
    (1, 1, 5, 5, "huge"),
    (2, 2, 6, 7, "inview"),
    (1, 4, 8, 6, "negative"),
    (2, 3, 7, 9, "outview"),
    (1, 3, 7, 8, "inview"),          # (H % 3, W % 3) = (1, 2)
    (1, 2, 8, 7, "huge"),            # (2, 1)
    (1, 3, 13, 22, "inview"),
    (1, 1, 13, 22, "negative"),
    (2, 2, 13, 22, "huge"),
    (1, 4, 13, 22, "outview"),
    (2, 3, 13, 22, "negative"),
    (1, 4, 11, 14, "huge"),          # (2, 2) remainder with four channels
    (7, 3, 9, 9, "inview"),          # 63 threads
    (1, 1, 24, 24, "negative"),      # 64 threads: exactly one full workgroup
    (5, 4, 5, 41, "inview"),         # 65 threads: a second workgroup of one thread
    (1, 2, 24, 24, "outview"),
    (2, 3, 288, 288, "inview"),      # 18432 threads, 288 slots > 256: the finalize kernel's strided loop
)
REGIMES = ("inview", "negative", "outview", "huge")
# seed of a row: 9500 + its position, unless listed here (a row whose first seed put more than the allowed share of pixels on the
# |left - left_est| < 1e-3 kink, or that torch's own float32 could not pass; test_selfsup_row_yardstick_passes decides)
SS_RESEED = {}
HUGE = 1.0e6
EPS_XS = 1e-3


def _sid(row):
    return "B{}c{}_{}x{}_{}".format(*row)


def _smooth_images(g, B, C, H, W):
    """tests/golden/make_golden_selfsup.py::smooth_images for C channels: noise upsampled x 4, bilinear (at least one coarse pixel)."""
    lo = torch.randn((B, C, max(1, H // 4), max(1, W // 4)), generator=g)
    return F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).contiguous()


def _near_kink(d32, W):
    """make_golden_selfsup.py::near_kink: the sample abscissa within 1e-3 of an integer, in float64 or in the reference's float32 order."""
    x = np.arange(W, dtype=np.float64)
    a = (2.0 * (x - d32.astype(np.float64)) / (W - 1) - 1.0 + 1.0) * W / 2.0 - 0.5
    x32 = np.arange(W, dtype=np.float32)
    gx = np.float32(2.0) * (x32 - d32) / np.float32(W - 1) - np.float32(1.0)
    b = (((gx + np.float32(1.0)) * np.float32(W) - np.float32(1.0)) / np.float32(2.0)).astype(np.float64)
    return (np.abs(a - np.round(a)) < EPS_XS) | (np.abs(b - np.round(b)) < EPS_XS)


def _draw_disp(g, B, H, W, regime):
    """make_golden_selfsup.py::draw_disp over [lo, hi): redrawn until no abscissa is within 1e-3 of an integer.  `huge` then sets a
    quarter of the pixels to 1e6: their samples lie ~1e6 pixels left of the image, where no tap is taken and float32 has no
    fraction left to compare with an integer, so the redraw rule does not apply to them."""
    lo, hi = {"inview": (0.0, W / 3), "negative": (-W / 3, 0.0), "outview": (0.0, 2.0 * W), "huge": (0.0, W / 3)}[regime]
    d = (torch.rand((B, H, W), generator=g) * (hi - lo) + lo).numpy()
    for _ in range(100):
        bad = _near_kink(d, W)
        if not bad.any():
            break
        d[bad] = (torch.rand((int(bad.sum()),), generator=g) * (hi - lo) + lo).numpy()
    assert not _near_kink(d, W).any()
    d = torch.from_numpy(d.astype(np.float32))
    if regime == "huge":
        d[torch.rand((B, H, W), generator=g) < 0.25] = HUGE
    return d


def _ss_inputs(row):
    B, C, H, W, regime = row
    g = gen(SS_RESEED.get(row, 9500 + SS_ROWS.index(row)))
    left, right = _smooth_images(g, B, C, H, W), _smooth_images(g, B, C, H, W)
    return _draw_disp(g, B, H, W, regime), left, right


def _ss_twin(disp, left, right, dtype):
    from rag_amd.metrics import re_and_sm_loss_torch
    d = disp.detach().clone().to(dtype).requires_grad_(True)
    loss, terms = re_and_sm_loss_torch(d, left.to(dtype), right.to(dtype))
    loss.backward()
    return loss.detach().double(), torch.stack([t.detach().double() for t in terms]), d.grad


@functools.lru_cache(maxsize=None)
def _ss_case(row):
    """(disp, left, right, float64 twin, float32 yardstick, keep): the twins as (loss, terms[3], gradient); keep excludes the pixels with
    |left - left_est| < 1e-3 in a channel, where float32 may take the other side of torch.abs' subgradient."""
    disp, left, right = _ss_inputs(row)
    ref, yard = _ss_twin(disp, left, right, torch.float64), _ss_twin(disp, left, right, torch.float32)
    keep = ~((left.double() - warped64(disp.double(), right.double())).abs() < 1e-3).any(1)
    return disp, left, right, ref, yard, keep


def _grad_errors(got, ref, keep):
    """(max error on keep, pixels of keep over 1e-4 max|g|, max|g|)"""
    gmax = float(ref.abs().max())
    err = (got.detach().cpu().double() - ref).abs()[keep]
    return float(err.max()), int((err > 1e-4 * gmax).sum()), gmax


def test_selfsup_table_covers_every_remainder_and_thread_count():
    assert len(set(SS_ROWS)) == len(SS_ROWS)
    assert {(r[2] % 3, r[3] % 3) for r in SS_ROWS} == {(a, b) for a in range(3) for b in range(3)}
    assert {(3, 3), (3, 5), (5, 3), (4, 4), (5, 5), (6, 7), (8, 6), (7, 9), (13, 22)} <= {r[2:4] for r in SS_ROWS}
    assert {r[1] for r in SS_ROWS} == {1, 2, 3, 4} and {r[4] for r in SS_ROWS} == set(REGIMES)
    for c in (1, 2, 3, 4):                                               # every template meets a remainder row and a remainder column
        assert any(r[1] == c and r[2] % 3 for r in SS_ROWS) and any(r[1] == c and r[3] % 3 for r in SS_ROWS), c
    threads = {r[0] * (r[2] // 3) * (r[3] // 3) for r in SS_ROWS}
    assert {1, 63, 64, 65} <= threads
    assert (2, 3, 288, 288, "inview") in SS_ROWS and -(-2 * 96 * 96 // 64) > 256
    lib = _lib()
    for r in SS_ROWS:                                                    # the library's own slot count: one per 64 threads
        assert lib.ragmi_selfsup_loss_workspace_elems(r[0], r[2], r[3]) == 2 * 3 * -(-r[0] * (r[2] // 3) * (r[3] // 3) // 64), r
    assert set(SS_RESEED) <= set(SS_ROWS)


@pytest.mark.parametrize("row", SS_ROWS, ids=_sid)
def test_selfsup_row_yardstick_passes(row):
    """What the GPU test relies on, checked without a GPU: the regime does what its name says, at most 1 % of the pixels (2 % under 100
    pixels) are excluded from the gradient check, and torch's own float32 meets the zero-pixel condition (no kept pixel over
    1e-4 max|g| from float64) and the 1e-5 term tolerance: a row it cannot pass is reseeded or dropped, never gated wider."""
    B, C, H, W, regime = row
    disp, left, right, ref, yard, keep = _ss_case(row)
    n = keep.numel()
    excluded = int((~keep).sum())
    assert excluded <= n * (0.02 if n < 100 else 0.01), (excluded, n)
    xs = (torch.arange(W, dtype=torch.float64) - disp.double()) * W / (W - 1) - 0.5
    if regime == "inview":
        assert float(disp.min()) >= 0 and float(disp.max()) < W / 3
    elif regime == "negative":
        assert float(disp.max()) <= 0 and bool((xs > W - 1).any())                                 # samples past the right edge
    elif regime == "outview":
        assert float(((xs < 0) | (xs > W - 1)).double().mean()) > 0.5                              # most of the image is masked
    else:
        share = float((disp == HUGE).double().mean())
        assert 0.0 < share < 0.6 and bool((disp == HUGE).any()) and bool((disp < W).any())
    assert torch.isfinite(ref[2]).all() and float(ref[2].abs().max()) > 0
    e_yard, n_over, gmax = _grad_errors(yard[2], ref[2], keep)
    t_yard = float(((yard[1] - ref[1]).abs() / ref[1].abs().clamp_min(1e-30)).max())
    print(f"ENDS-CPU case={_sid(row)} excluded={excluded}/{n} e_yard={e_yard / gmax:.3e} over={n_over} term_yard={t_yard:.3e} max|g|={gmax:.3e}")
    assert n_over == 0, (n_over, e_yard / gmax)
    assert abs(float(yard[0] - ref[0])) <= 1e-5 * abs(float(ref[0])) and t_yard <= 1e-5


def _ss_run(disp, left, right):
    import rag_amd
    d = disp.clone().requires_grad_(True)
    loss = rag_amd.metrics.re_and_sm_loss(d, left, right)
    loss.backward()
    return loss.detach(), d.grad


@pytest.mark.gpu
@pytest.mark.parametrize("row", SS_ROWS, ids=_sid)
def test_selfsup_vs_fp64(row):
    """Loss and terms (both instantiations) within 1e-5 relative of float64; the gradient within 4 x torch's float32 error + 1e-5 max|g|
    and no kept pixel over 1e-4 max|g|; a gradient scaled by -2.5 equals unit * float32(-2.5) bit for bit."""
    import rag_amd
    disp, left, right, ref, yard, keep = _ss_case(row)
    d, lt, rt = gpu(disp), gpu(left), gpu(right)
    loss, unit = _ss_run(d, lt, rt)
    terms = rag_amd.metrics.self_supervised_terms(d, lt, rt).cpu().double()
    x = d.clone().requires_grad_(True)
    (rag_amd.metrics.re_and_sm_loss(x, lt, rt) * -2.5).backward()
    torch.cuda.synchronize()
    e_kernel, n_over, gmax = _grad_errors(unit, ref[2], keep)
    e_yard, _n, _g = _grad_errors(yard[2], ref[2], keep)
    e_loss = abs(float(loss) - float(ref[0])) / abs(float(ref[0]))
    e_terms = ((terms[1:] - ref[1]).abs() / ref[1].abs().clamp_min(1e-30))
    print(f"ENDS case={_sid(row)} e_kernel={e_kernel / gmax:.3e} e_yard={e_yard / gmax:.3e} over={n_over} e_loss={e_loss:.3e} "
          f"e_terms={[f'{float(v):.1e}' for v in e_terms]}")
    assert e_loss <= 1e-5 and abs(float(terms[0]) - float(ref[0])) <= 1e-5 * abs(float(ref[0]))
    assert bool((e_terms <= 1e-5).all()), e_terms
    assert torch.isfinite(unit).all()
    assert e_kernel <= NOISE * e_yard + 1e-5 * gmax, (e_kernel, e_yard, gmax)
    assert n_over == 0
    assert torch.equal(x.grad.cpu(), unit.cpu() * torch.tensor(-2.5, dtype=torch.float32))


SS_LAYOUT_ROWS = ((2, 3, 13, 22, "negative"), (1, 4, 11, 14, "huge"), (5, 4, 5, 41, "inview"), (1, 1, 24, 24, "negative"))


@pytest.mark.gpu
@pytest.mark.parametrize("row", SS_LAYOUT_ROWS, ids=_sid)
def test_selfsup_layouts_give_the_same_bits(row):
    """channels-last left / right and a strided disp == the contiguous run, loss and gradient."""
    disp, left, right, _ref, _yard, _keep = _ss_case(row)
    d, lt, rt = gpu(disp), gpu(left), gpu(right)
    base = _ss_run(d, lt, rt)
    lcl, rcl = lt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), rt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    wide = torch.zeros((d.shape[0], d.shape[1], 2 * d.shape[2]), device=DEV)
    wide[:, :, ::2] = d
    ds = wide[:, :, ::2]
    assert torch.equal(lcl, lt) and torch.equal(ds, d) and not ds.is_contiguous() and (row[1] == 1 or not lcl.is_contiguous())
    other = _ss_run(ds, lcl, rcl)
    assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1])


@pytest.mark.gpu
def test_selfsup_is_deterministic_past_256_slots():
    row = (2, 3, 288, 288, "inview")
    disp, left, right, _ref, _yard, _keep = _ss_case(row)
    d, lt, rt = gpu(disp), gpu(left), gpu(right)
    a, b = _ss_run(d, lt, rt), _ss_run(d, lt, rt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
