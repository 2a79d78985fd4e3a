"""Sweep of the monocular-depth kernels (rag_amd/csrc/depth_head.hip, depth_train.hip, depth_metrics.hip) over scales, shapes, channel
counts, tile remainders, masks and sizes, against the project's plain-torch twins (rag_amd.depth.depth_head_torch, silog_loss_torch,
depth_metrics_torch and the fp64 silog restatement of test_depth_train.py) evaluated on the CPU in float64 with autograd.

Gate of every tensor of every case (the pattern of test_depth_train.py::fp32_tol and test_hip_train.py::NOISE_FACTOR):
    e_kernel = max|kernel - ref64| / max|ref64|  <=  max(floor, 3 * e_twin),   e_twin = max|twin32 - ref64| / max|ref64|
where twin32 is the same twin in float32 on the CPU.  The kernels do the twin's fp32 per-pixel arithmetic in another order, with double
sums where the twin has float sums; 3x allows for the order.  The floors are the ones the existing tests apply to these kernels:
1e-4 * max_depth / 80 absolute for the depth map, 1e-4 relative for the head gradients, 1e-5 relative for the silog loss and gradient,
rtol 1e-5 / atol 1e-6 for the non-count metrics.  Determinism, accumulation, the non-contiguous d_out run, the threshold counts and the
sentinel floats are compared bit for bit.  A case whose e_twin exceeds 10x its floor is ill-conditioned and must be replaced, not
gated wider: the unmarked tests below assert that for every row, without a GPU.

Every GPU test prints `SWEEP case=... tensor=... e_kernel=... e_twin=...`, one line per tensor (DESIGN.md section 4.6 carries the
worst figures).  Unmarked tests run without a GPU; the rest need the MI355X."""
import functools

import pytest
import torch

from test_depth_train import _silog64, rel_max

DEV = "cuda:0"
NOISE = 3.0                      # test_depth_train.py::fp32_tol
ILL = 10.0                       # e_twin above ILL x floor: the case is ill-conditioned, replace it
FLOOR_GRAD = 1e-4                # test_depth_train.py::test_depth_head_bwd_vs_fp64_reference
FLOOR_SILOG = 1e-5               # test_depth_train.py::test_silog_at_training_crop_vs_fp64
HEAD_NAMES = ("out", "dy", "dw3", "dw1", "db1")

# ------------------------------------------------------------------------------------------------------------------ head cases
# (B, Cin, Hi, Wi, H, W, S): y [B, Cin, Hi, Wi] -> (H, W) -> x S.  The s map is tiled DH_TH x DH_TW = 8 x 32 (depth_common.h); the
# forward stores 16 bytes at a time when S*W % 4 == 0 and `out` is 16-byte aligned (a.vec), one float at a time otherwise.
SATURATING = (2, 12, 10, 16, 20, 32, 3)
HEAD_ROWS = (
    # ---- store path: scalar branch (S*W % 4 != 0)
    (2, 12, 4, 4, 8, 7, 3),          # OW 21: scalar stores, one tile narrower than DH_TW, H == DH_TH
    (2, 12, 7, 11, 15, 25, 3),       # OW 75: scalar; non-integer ratios 7 -> 15 and 11 -> 25; two tile rows, the last of 7
    (1, 12, 8, 17, 16, 33, 3),       # OW 99: scalar; the last tile column holds one s pixel = 3 output pixels (< 4)
    (1, 5, 9, 33, 9, 33, 1),         # OW 33, S 1: scalar; Hi == H and Wi == W (sy = sx = 1); last tile column 1 output pixel; H 9 = 8 + 1
    (1, 12, 4, 17, 9, 33, 2),        # OW 66, S 2: scalar; last tile column 2 output pixels
    # ---- store path: vector branch (S*W % 4 == 0) with a narrow last tile column
    (1, 12, 9, 17, 17, 33, 4),       # OW 132, S 4: vector; last tile column exactly 4 output pixels (one 16-byte store per row); H 17
    (2, 12, 4, 9, 8, 33, 8),         # OW 264, S 8: vector; last tile column 8 output pixels; the widest x S adjoint window
    (1, 12, 4, 17, 8, 34, 2),        # OW 68, S 2: vector; last tile column 2 s pixels = 4 output pixels
    # ---- tile edges: H in {1, 7, 8, 9, 17}, W in {1, 31, 32, 33, 65}
    (1, 12, 1, 1, 1, 1, 3),          # H = W = Hi = Wi = 1: sy = sx = 0 from the size-1 output, OW 3 scalar
    (3, 12, 1, 16, 1, 32, 3),        # H 1 with Hi 1, W == DH_TW exactly, B 3; OW 96 vector
    (2, 12, 4, 1, 7, 1, 5),          # W 1 with Wi 1 (sx = 0), H 7, S 5; OW 5 scalar
    (1, 12, 4, 16, 8, 31, 4),        # H == DH_TH, W = DH_TW - 1, S 4; OW 124 vector
    (1, 16, 5, 20, 9, 32, 2),        # Cin 16 (DH_CMAX), H 9, W 32, S 2; OW 64 vector
    (3, 1, 9, 33, 17, 65, 1),        # Cin 1, B 3, H 17 (three tile rows), W 65 (three tile columns, the last of 1), S 1; OW 65 scalar
    (1, 12, 8, 31, 17, 65, 6),       # S 6, OW 390 scalar; W 65, H 17
    (1, 12, 4, 8, 8, 16, 7),         # S 7, OW 112 vector
    (1, 5, 3, 5, 7, 9, 7),           # S 7, OW 63 scalar; Cin 5; H 7
    # ---- upsample ratios
    (1, 12, 1, 1, 9, 12, 3),         # Hi = Wi = 1 with H, W > 1 (sy = sx = 0: ac_window's scale == 0 branch on both axes); small
    (1, 5, 1, 6, 8, 12, 2),          # Hi 1 with H 8 (sy = 0), Wi 6 -> 12; small
    (1, 12, 2, 2, 40, 40, 3),        # large ratio 2 -> 40 (sy = 1/39): every y pixel gathers half the grid
    (2, 12, 16, 32, 16, 32, 3),      # Hi == H and Wi == W at S 3 (identity first upsample), exactly 2 x 1 tiles
    (1, 12, 17, 20, 17, 33, 5),      # Hi == H, Wi < W, S 5; OW 165 scalar
    (1, 16, 6, 40, 12, 80, 8),       # Cin 16 at S 8, W 80 = 2.5 tiles; OW 640 vector
    # ---- saturation: |z| reaches about 30 on part of the image (as g16 case 3)
    SATURATING,
    # ---- production
    (1, 12, 64, 208, 128, 416, 3),   # y [1, 12, 64, 208] -> (128, 416) x 3
    (8, 12, 64, 128, 128, 256, 3),   # y [8, 12, 64, 128] -> (128, 256) x 3
)
# outside ragmi_depth_head_supported's contract
HEAD_UNSUPPORTED = (
    (1, 17, 4, 4, 8, 8, 3),          # Cin 17 > DH_CMAX
    (1, 12, 4, 4, 8, 8, 9),          # S 9
    (1, 12, 9, 4, 8, 8, 3),          # Hi > H
    (1, 12, 4, 9, 8, 8, 3),          # Wi > W
    (1, 12, 4, 4, 8, 8, 0),          # S 0
)


def _rid(row):
    return "B{}c{}_{}x{}_{}x{}_x{}".format(*row)


def _max_depth(row):
    return 1.0 if row[1] == 1 else 80.0      # a one-channel head is the standalone DispHead, which runs at max_depth 1


def _head_inputs(row):
    """fp32 inputs of one row, seeded by its position in the table: |m| ~ 1 as a trained head's, d_out = randn + 0.5 so that db1 does
    not cancel."""
    B, Cin, Hi, Wi, H, W, S = row
    g = torch.Generator().manual_seed(4600 + HEAD_ROWS.index(row))
    y = torch.randn((B, Cin, Hi, Wi), generator=g)
    w3 = torch.randn((1, Cin, 3, 3), generator=g) * (0.35 / Cin ** 0.5)
    w1 = torch.randn((1, 1, 3, 3), generator=g)
    b1 = torch.randn((1,), generator=g)
    dout = torch.randn((B, S * H, S * W), generator=g) + 0.5
    if row == SATURATING:
        y = y * torch.linspace(0.2, 12.0, Wi)            # |z| grows from ~ 1 on the left to ~ 30 on the right
    if Hi * Wi > 4096:
        # the production sizes: ATen's own fp32 source index sx * x is ~ 1e-5 pixel off at x ~ 200, which white noise (a unit step
        # between neighbours) turns into 2e-3 m of depth in the fp32 twin itself.  Features of a trained trunk are smooth at that
        # scale: a coarse field interpolated x 16 plus 3 % of white noise.
        coarse = torch.randn((B, Cin, Hi // 16, Wi // 16), generator=g)
        y = 1.5 * torch.nn.functional.interpolate(coarse, size=(Hi, Wi), mode="bilinear", align_corners=True) + 0.03 * y
    return y, w3, w1, b1, dout


def _head_twin(row, inputs, dtype):
    from rag_amd.depth import depth_head_torch
    y, w3, w1, b1 = (t.detach().clone().to(dtype).requires_grad_(True) for t in inputs[:4])
    out = depth_head_torch(y, w3, w1, b1, row[4:6], row[6], _max_depth(row))
    out.backward(inputs[4].to(dtype))
    return tuple(t.detach() for t in (out, y.grad, w3.grad, w1.grad, b1.grad))


@functools.lru_cache(maxsize=None)
def _head_case(row):
    """(fp32 inputs, fp64 twin, fp32 twin) of one row, each twin as (out, dy, dw3, dw1, db1); computed once per module."""
    inputs = _head_inputs(row)
    return inputs, _head_twin(row, inputs, torch.float64), _head_twin(row, inputs, torch.float32)


def _head_floor(row, name, ref):
    """The floor of one head tensor, relative to max|ref| (the depth map's is absolute: 1e-4 * max_depth / 80)."""
    if name == "out":
        return 1e-4 * _max_depth(row) / 80.0 / max(float(ref.abs().max()), 1e-30)
    return FLOOR_GRAD


def _gate(case, name, got, ref, twin, floor):
    e_kernel, e_twin = rel_max(got.reshape(ref.shape), ref), rel_max(twin, ref)
    print(f"SWEEP case={case} tensor={name} e_kernel={e_kernel:.3e} e_twin={e_twin:.3e}")
    assert e_kernel <= max(floor, NOISE * e_twin), (case, name, e_kernel, e_twin, floor)


def gpu(t):
    return t.to(DEV)


# ------------------------------------------------------------------------------------------------------------------ CPU: the table
def test_head_table_reaches_every_path():
    """The paths the issue lists, read off the table against the kernel's own conditions."""
    rows = HEAD_ROWS
    assert len(set(rows)) == len(rows)
    assert all(B * S * H * S * W <= 1 << 20 for B, _c, _hi, _wi, H, W, S in rows[:-2])     # all but the two production rows
    vec = [r for r in rows if (r[6] * r[5]) % 4 == 0]
    assert vec and len(vec) < len(rows)                                                   # both store branches
    last = lambda r: r[6] * (r[5] - 32 * ((r[5] - 1) // 32))  # noqa: E731                output pixels of the last tile column
    assert any(last(r) < 4 for r in rows if r not in vec)                                 # narrower than one 16-byte store
    assert any(last(r) == 4 for r in vec)
    assert {r[6] for r in rows} == set(range(1, 9))                                       # every scale
    assert {1, 5, 12, 16} <= {r[1] for r in rows}
    assert {1, 7, 8, 9, 17} <= {r[4] for r in rows} and {1, 31, 32, 33, 65} <= {r[5] for r in rows}
    assert any(r[0] == 3 for r in rows)
    assert any(r[2] == r[4] and r[3] == r[5] for r in rows)                               # identity first upsample
    assert any(r[2] == 1 and r[4] > 1 for r in rows) and any(r[3] == 1 and r[5] > 1 for r in rows)
    assert any(r[2] == 1 and r[4] == 1 for r in rows)
    assert (2, 12, 7, 11, 15, 25, 3) in rows and any(r[2] == 2 and r[4] == 40 for r in rows)
    assert (1, 12, 64, 208, 128, 416, 3) in rows and (8, 12, 64, 128, 128, 256, 3) in rows
    # Hi = 1 rows stay small: the backward's dy thread then walks the whole (H, W) grid
    assert all(r[4] * r[5] <= 128 for r in rows if r[2] == 1 and r[3] == 1)


@pytest.mark.parametrize("row", HEAD_ROWS, ids=_rid)
def test_head_row_is_well_conditioned(row):
    """e_twin <= 10 x floor for the depth map and the four gradients of every row: no gate of the GPU sweep is wider than 30 floors."""
    _inputs, ref, twin = _head_case(row)
    for name, r, t in zip(HEAD_NAMES, ref, twin):
        assert torch.isfinite(r).all() and float(r.abs().max()) > 0, name
        e_twin, floor = rel_max(t, r), _head_floor(row, name, r)
        print(f"SWEEP-CPU case={_rid(row)} tensor={name} e_twin={e_twin:.3e} floor={floor:.3e} max|ref|={float(r.abs().max()):.3e}")
        assert e_twin <= ILL * floor, (name, e_twin, floor)


def test_head_saturating_row_saturates_part_of_the_image():
    import torch.nn.functional as F
    y, w3, w1, b1, _dout = (t.double() for t in _head_inputs(SATURATING))
    u = F.interpolate(y, size=SATURATING[4:6], mode="bilinear", align_corners=True)
    z = F.conv2d(F.conv2d(u, w3, padding=1), w1, b1, padding=1).abs()
    assert 25.0 <= float(z.max()) <= 60.0, float(z.max())
    assert float((z < 5.0).double().mean()) >= 0.2                                        # and part of it does not


def test_head_twin_fp64_matches_separable_restatement():
    """The yardstick itself: depth_head_torch in fp64 == explicit align_corners=True / half-pixel interpolation matrices around the two
    convolutions, on the odd-ratio row (so a failure of the sweep points at a kernel, not at the twin)."""
    import torch.nn.functional as F
    row = (2, 12, 7, 11, 15, 25, 3)
    y, w3, w1, b1, _dout = (t.double() for t in _head_inputs(row))

    def matrix(n_out, n_in, src):
        m = torch.zeros((n_out, n_in), dtype=torch.float64)
        for o in range(n_out):
            r = src(o)
            i0 = min(int(r), n_in - 1)
            i1 = min(i0 + 1, n_in - 1)
            m[o, i0] += 1.0 - (r - i0)
            m[o, i1] += r - i0
        return m
    _B, _C, Hi, Wi, H, W, S = row
    ay = matrix(H, Hi, lambda o: o * (Hi - 1) / (H - 1))
    ax = matrix(W, Wi, lambda o: o * (Wi - 1) / (W - 1))
    hy = matrix(S * H, H, lambda o: max((o + 0.5) / S - 0.5, 0.0))
    hx = matrix(S * W, W, lambda o: max((o + 0.5) / S - 0.5, 0.0))
    u = torch.einsum("gh,bchw,xw->bcgx", ay, y, ax)
    s = torch.sigmoid(F.conv2d(F.conv2d(u, w3, padding=1), w1, b1, padding=1))[:, 0]
    want = 80.0 * torch.einsum("oh,bhw,xw->box", hy, s, hx)
    assert rel_max(_head_case(row)[1][0], want) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ GPU: forward
@pytest.mark.gpu
@pytest.mark.parametrize("row", HEAD_ROWS, ids=_rid)
def test_head_fwd_vs_fp64(row):
    from rag_amd import ops
    B, Cin, Hi, Wi, H, W, S = row
    assert ops.depth_head_supported(Cin, Hi, Wi, H, W, S)
    inputs, ref, twin = _head_case(row)
    out = ops.depth_head(*(gpu(t) for t in inputs[:4]), (H, W), S, _max_depth(row))
    again = ops.depth_head(*(gpu(t) for t in inputs[:4]), (H, W), S, _max_depth(row))
    torch.cuda.synchronize()
    assert out.shape == (B, S * H, S * W) and out.dtype == torch.float32
    _gate(_rid(row), "out", out, ref[0], twin[0], _head_floor(row, "out", ref[0]))
    assert torch.equal(out, again)


SENTINEL = 0x7FC0BEEF            # a quiet NaN with a payload: no arithmetic of the kernel produces these bits


@pytest.mark.gpu
@pytest.mark.parametrize("offset", (1, 4), ids=("unaligned", "aligned"))
@pytest.mark.parametrize("row", ((2, 12, 4, 9, 8, 33, 8), (1, 12, 9, 17, 17, 33, 4), (3, 12, 1, 16, 1, 32, 3), (1, 12, 8, 17, 16, 33, 3)),
                         ids=_rid)
def test_head_fwd_into_a_view_of_a_larger_buffer(row, offset):
    """ragmi_depth_head_fwd with `out` `offset` floats into a sentinel-filled buffer.  At one float in, a row with S*W % 4 == 0 must fall
    back to scalar stores (`vec` off); at four floats in it keeps its 16-byte stores.  Either way the values pass the forward gate and the
    floats before and after the view keep their bits."""
    from rag_amd import _lib, ops
    B, Cin, Hi, Wi, H, W, S = row
    inputs, ref, twin = _head_case(row)
    y, w3, w1, b1 = (gpu(t).contiguous() for t in inputs[:4])
    n, pad = B * S * H * S * W, 64
    buf = torch.full((offset + n + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    _lib.check(_lib.load_library().ragmi_depth_head_fwd(y.data_ptr(), w3.data_ptr(), w1.data_ptr(), b1.data_ptr(), buf.data_ptr() + 4 * offset,
                                                        B, Cin, Hi, Wi, H, W, S, _max_depth(row), ops.F32, ops._stream()), "depth_head")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:offset] == SENTINEL).all()) and bool((host[offset + n:] == SENTINEL).all())
    out = host[offset:offset + n].view(torch.float32).reshape(B, S * H, S * W)
    assert not bool((host[offset:offset + n] == SENTINEL).any())                          # every pixel of the view was written
    _gate(f"{_rid(row)}+{offset}", "out", out, ref[0], twin[0], _head_floor(row, "out", ref[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("row", HEAD_UNSUPPORTED, ids=_rid)
def test_head_refuses_rows_outside_the_contract(row):
    from rag_amd import ops
    B, Cin, Hi, Wi, H, W, S = row
    assert not ops.depth_head_supported(Cin, Hi, Wi, H, W, S)
    g = torch.Generator().manual_seed(1)
    y, w3 = torch.randn((B, Cin, Hi, Wi), generator=g), torch.randn((1, Cin, 3, 3), generator=g)
    w1, b1 = torch.randn((1, 1, 3, 3), generator=g), torch.randn((1,), generator=g)
    with pytest.raises(RuntimeError):
        ops.depth_head(gpu(y), gpu(w3), gpu(w1), gpu(b1), (H, W), S, 80.0)


def test_head_supported_refuses_rows_outside_the_contract_without_a_gpu():
    from rag_amd import ops
    for B, Cin, Hi, Wi, H, W, S in HEAD_UNSUPPORTED:
        assert not ops.depth_head_supported(Cin, Hi, Wi, H, W, S)
    for B, Cin, Hi, Wi, H, W, S in HEAD_ROWS:
        assert ops.depth_head_supported(Cin, Hi, Wi, H, W, S)


# ------------------------------------------------------------------------------------------------------------------ GPU: backward
def _head_bwd(row, inputs, **into):
    from rag_amd import ops
    return ops.depth_head_bwd(*(t if t.is_cuda else gpu(t) for t in inputs), row[4:6], row[6], _max_depth(row), **into)


@pytest.mark.gpu
@pytest.mark.parametrize("row", HEAD_ROWS, ids=_rid)
def test_head_bwd_vs_fp64_autograd(row):
    """dy, dw3, dw1, db1 against fp64 autograd of the twin; two runs bitwise equal."""
    inputs, ref, twin = _head_case(row)
    dev = [gpu(t) for t in inputs]
    r1, r2 = _head_bwd(row, dev), _head_bwd(row, dev)
    torch.cuda.synchronize()
    for name, got, again, r, t in zip(HEAD_NAMES[1:], r1, r2, ref[1:], twin[1:]):
        assert torch.equal(got, again), name
        _gate(_rid(row), name, got, r, t, FLOOR_GRAD)


INTO_ROWS = ((2, 12, 7, 11, 15, 25, 3), (3, 1, 9, 33, 17, 65, 1), (1, 16, 6, 40, 12, 80, 8))
INTO_SETS = (("dw3_into",), ("dw1_into",), ("db1_into",), ("dw3_into", "db1_into"), ("dw1_into", "db1_into"))


@pytest.mark.gpu
@pytest.mark.parametrize("which", INTO_SETS, ids="+".join)
@pytest.mark.parametrize("row", INTO_ROWS, ids=_rid)
def test_head_bwd_accumulates_per_output(row, which):
    """Each `*_into` on its own and in pairs (the accumulate bits of ragmi_depth_head_bwd): a tensor given `into` ends as pre + fresh
    exactly, the others and dy are bit-equal to a fresh run."""
    inputs, _ref, _twin = _head_case(row)
    dev = [gpu(t) for t in inputs]
    fresh = _head_bwd(row, dev)
    names = ("dw3_into", "dw1_into", "db1_into")
    g = torch.Generator().manual_seed(9)
    pre = {n: gpu(torch.randn(f.shape, generator=g)) for n, f in zip(names, fresh[1:]) if n in which}
    into = {n: p.clone() for n, p in pre.items()}
    out = _head_bwd(row, dev, **into)
    torch.cuda.synchronize()
    assert torch.equal(out[0], fresh[0])
    for n, f, o in zip(names, fresh[1:], out[1:]):
        if n in which:
            assert o.data_ptr() == into[n].data_ptr()
            assert torch.equal(into[n], pre[n] + f), n
        else:
            assert torch.equal(o, f), n


@pytest.mark.gpu
@pytest.mark.parametrize("need", ("y", "weights"))
def test_head_fn_with_part_of_the_inputs_requiring_grad(need):
    """DepthHeadFn with only y, or only the three weights, requiring grad: the gradients asked for pass the gate, the others are None."""
    from rag_amd.depth import DepthHeadFn
    row = (1, 12, 8, 31, 17, 65, 6)
    inputs, ref, twin = _head_case(row)
    ins = [gpu(t) for t in inputs[:4]]
    wants = (need == "y", need != "y", need != "y", need != "y")
    for t, w in zip(ins, wants):
        t.requires_grad_(w)
    out = DepthHeadFn.apply(*ins, row[4:6], row[6], _max_depth(row))
    out.backward(gpu(inputs[4]))
    torch.cuda.synchronize()
    _gate(_rid(row) + "/" + need, "out", out.detach(), ref[0], twin[0], _head_floor(row, "out", ref[0]))
    for name, t, w, r, tw in zip(HEAD_NAMES[1:], ins, wants, ref[1:], twin[1:]):
        if w:
            _gate(_rid(row) + "/" + need, name, t.grad, r, tw, FLOOR_GRAD)
        else:
            assert t.grad is None, name


@pytest.mark.gpu
@pytest.mark.parametrize("row", ((2, 12, 7, 11, 15, 25, 3), (2, 12, 4, 9, 8, 33, 8)), ids=_rid)
def test_head_bwd_non_contiguous_d_out(row):
    """A d_out that is a transposed view on entry gives the contiguous run's results bit for bit."""
    inputs, _ref, _twin = _head_case(row)
    dev = [gpu(t) for t in inputs]
    view = dev[4].transpose(1, 2).contiguous().transpose(1, 2)
    assert not view.is_contiguous() and torch.equal(view, dev[4])
    for a, b in zip(_head_bwd(row, dev), _head_bwd(row, dev[:4] + [view])):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ silog and metrics
# rag_amd/csrc/depth_train.hip: SL_WG = 256, SL_MAXWG = 1024; the forward launches min(ceil(n / (4 * SL_WG)), SL_MAXWG) workgroups and
# the backward min(ceil(n / (4 * SL_WG)), 2048).  rag_amd/csrc/depth_metrics.hip: DM_WG = 256, DM_MAXWG = 1024, the same slot count.
WG, FWD_CAP, BWD_CAP = 256, 1024 * 4 * 256, 2048 * 4 * 256
ABOVE = 2_500_001                # odd, above every cap: 9 full forward strides of 1024 * 256 and 4 backward strides of 2048 * 256, then a tail
TAIL = 9 * 1024 * 256 + 77       # inside the grid-stride tail of both passes at n = ABOVE
SIZES = (1, 255, 256, 257, 1023, 1024, 1025, FWD_CAP - 1, FWD_CAP + 1, BWD_CAP + 1, ABOVE)
MASKS = ("all", "holes")
# (n, mask, variance_focus)
LOSS_CASES = tuple((n, m, 0.85) for n in SIZES for m in MASKS if not (n == 1 and m == "holes")) + tuple(
    (n, "holes", vf) for n in (257, FWD_CAP + 1, ABOVE) for vf in (0.0, 0.5)) + (
    (1, "first", 0.5), (257, "first", 0.85), (257, "last", 0.85), (FWD_CAP + 1, "last", 0.0), (ABOVE, "first", 0.85), (ABOVE, "last", 0.85),
    (ABOVE, "tail", 0.85), (ABOVE, "tail", 0.0), (1025, "badgt", 0.85), (ABOVE, "badgt", 0.5))
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
TIES = ((4.0, 5.0), (5.0, 4.0), (16.0, 25.0), (25.0, 16.0), (64.0, 125.0), (125.0, 64.0))    # (est, gt): max ratio exactly on a threshold


def _lid(case):
    return f"n{case[0]}_{case[1]}_vf{case[2]}"


@functools.lru_cache(maxsize=4)
def _pixels(n, mask):
    """Flat fp32 (est, gt): est in [0.5, 79.5), log(est / gt) ~ N(0, 0.3) (sigma >= 0.1 keeps silog's variance clear of cancellation).
    `holes`: about 60 % of gt = 0.  `badgt`: holes of 0, negative and NaN.  `first` / `last` / `tail`: one valid pixel, 40 % off.
    `none`: no valid pixel.  No pixel lies within 1e-5 relative of a d1 / d2 / d3 threshold: those that the draw puts within 1e-4 are moved
    by 0.1 %.  Where they fit, exact ties are then planted on valid pixels: they must count as NOT below the threshold."""
    g = torch.Generator().manual_seed(7700 + n % 1000 + sum(map(ord, mask)))
    est = torch.rand((n,), generator=g) * 79 + 0.5
    gt = est * torch.exp(torch.randn((n,), generator=g) * 0.3)
    for _ in range(2):
        th = torch.maximum(gt.double() / est.double(), est.double() / gt.double())
        near = torch.zeros_like(th, dtype=torch.bool)
        for t in THRESHOLDS:
            near |= (th / t - 1.0).abs() < 1e-4
        gt = torch.where(near, gt * 1.001, gt)
    if mask in ("all", "holes", "badgt") and n >= 255:
        for k, (e, t) in enumerate(TIES):
            est[11 + 40 * k], gt[11 + 40 * k] = e, t
    hole = torch.rand((n,), generator=g) < 0.6
    hole[11:11 + 40 * len(TIES):40] = False
    if mask == "holes":
        gt[hole] = 0.0
    elif mask == "badgt":
        kind = torch.randint(0, 3, (n,), generator=g)
        gt = torch.where(hole, torch.where(kind == 0, torch.zeros(()), torch.where(kind == 1, -gt, torch.full((), float("nan")))), gt)
    elif mask in ("first", "last", "tail"):
        at = {"first": 0, "last": n - 1, "tail": TAIL}[mask] if n > 1 else 0
        keep = est[at] * 1.4
        gt = torch.where(torch.rand((n,), generator=g) < 0.5, torch.zeros(()), -gt)
        gt[at] = keep
    elif mask == "none":
        kind = torch.randint(0, 3, (n,), generator=g)
        gt = torch.where(kind == 0, torch.zeros(()), torch.where(kind == 1, -gt, torch.full((), float("nan"))))
    return est, gt


def _tie_mask(est, gt):
    tie = torch.zeros_like(est, dtype=torch.bool)
    for e, t in TIES:
        tie |= (est == e) & (gt == t)
    return tie


def _silog_twin32(est, gt, vf, upstream):
    from rag_amd.depth import silog_loss_torch
    e = est.clone().requires_grad_(True)
    loss = silog_loss_torch(e, gt, vf)
    (loss * upstream).backward()
    return loss.detach(), e.grad


UPSTREAM = 1.5                   # the loss's incoming gradient, other than 1


def _loss_refs(case):
    n, mask, vf = case
    est, gt = _pixels(n, mask)
    loss64, grad64 = _silog64(est, gt, vf)
    return est, gt, (loss64, grad64 * UPSTREAM), _silog_twin32(est, gt, vf, UPSTREAM)


def _metric_floor(ref):
    return 1e-6 + 1e-5 * ref.abs()                     # test_depth.py: rtol 1e-5 / atol 1e-6, per output


def _metric_refs(n, mask):
    from rag_amd.depth import depth_metrics_torch
    est, gt = _pixels(n, mask)
    return est, gt, depth_metrics_torch(est.double(), gt.double(), 0.85), depth_metrics_torch(est, gt, 0.85).double()


def _metric_gated(gt):
    """Indices of the outputs under the tolerance gate: 0..6 (7..9 are counts, compared as integers).  With ONE valid pixel `silog`
    (index 1) is 100 sqrt(d^2 - d d), the variance_focus = 1 formula, whose rounding decides between 0, 1e-2 and NaN in any fp32
    evaluation (the issue leaves variance_focus 1.0 out for that reason): not a property of the kernel, so it is left out there."""
    return (0, 2, 3, 4, 5, 6) if int((gt > 0).sum()) == 1 else (0, 1, 2, 3, 4, 5, 6)


METRIC_CASES = tuple((n, m) for n in SIZES for m in MASKS if not (n == 1 and m == "holes")) + (
    (1, "first"), (257, "last"), (ABOVE, "first"), (ABOVE, "last"), (ABOVE, "tail"), (1025, "badgt"), (ABOVE, "badgt"))


def test_size_list_straddles_the_librarys_own_caps():
    """The literals above against the library: one slot (3 or 10 doubles) per workgroup, min(ceil(n / (4 * 256)), 1024) of them, so the
    sizes of SIZES do sit either side of one workgroup, of two, and of the cap."""
    from rag_amd import _lib
    L = _lib.load_library()
    for n in SIZES + (FWD_CAP, 4 * WG + 1):
        slots = min(-(-n // (4 * WG)), FWD_CAP // (4 * WG))
        assert L.ragmi_silog_loss_workspace_elems(n) == slots * 3 * 2, n
        assert L.ragmi_depth_metrics_workspace_elems(n) == slots * 10 * 2, n
    assert TAIL < ABOVE and TAIL >= (ABOVE // (1024 * WG)) * 1024 * WG and TAIL >= (ABOVE // (2048 * WG)) * 2048 * WG


@pytest.mark.parametrize("case", LOSS_CASES, ids=_lid)
def test_silog_case_is_well_conditioned(case):
    est, gt, ref, twin = _loss_refs(case)
    d = torch.log(est.double()[gt > 0]) - torch.log(gt.double()[gt > 0])
    assert d.numel() == 1 or float(d.std()) >= 0.1
    if case[1] in ("first", "last", "tail"):
        assert int((gt > 0).sum()) == 1 and bool(gt[{"first": 0, "last": -1, "tail": TAIL if case[0] > 1 else 0}[case[1]]] > 0)
    if case[1] == "badgt":
        assert bool(torch.isnan(gt).any()) and bool((gt < 0).any()) and bool((gt == 0).any())
    for name, r, t in zip(("loss", "grad"), ref, twin):
        assert torch.isfinite(r).all() and float(r.abs().max()) > 0
        e_twin = rel_max(t, r)
        print(f"SWEEP-CPU case={_lid(case)} tensor=silog_{name} e_twin={e_twin:.3e}")
        assert e_twin <= ILL * FLOOR_SILOG, (name, e_twin)


@pytest.mark.parametrize("case", METRIC_CASES, ids=lambda c: f"n{c[0]}_{c[1]}")
def test_metrics_inputs_keep_clear_of_the_thresholds(case):
    """No valid pixel within 1e-5 relative of 1.25, 1.25^2 or 1.25^3 (th in fp64 from the fp32 inputs), apart from the planted exact ties,
    so an fp32 evaluation of th cannot fall on the other side; and the non-count outputs are well-conditioned."""
    n, mask = case
    est, gt, ref, twin = _metric_refs(n, mask)
    valid = gt > 0
    tie = _tie_mask(est, gt)
    e, t = est.double()[valid & ~tie], gt.double()[valid & ~tie]
    th = torch.maximum(t / e, e / t)
    for thr in THRESHOLDS:
        assert not bool(((th / thr - 1.0).abs() <= 1e-5).any()), thr
    if mask in MASKS + ("badgt",) and n >= 255:
        assert int((valid & tie).sum()) >= len(TIES)
        for (te, tg), thr in zip(TIES, (1.25, 1.25, 1.5625, 1.5625, 1.953125, 1.953125)):
            assert max(torch.tensor(te) / torch.tensor(tg), torch.tensor(tg) / torch.tensor(te)).item() == thr     # exact in fp32
    floor = _metric_floor(ref)
    for k in _metric_gated(gt):
        assert torch.isfinite(ref[k]), k
        assert float((twin[k] - ref[k]).abs()) <= ILL * float(floor[k]), (k, float(twin[k]), float(ref[k]))
    assert bool((twin[7:] == ref[7:]).all())             # the fp32 twin counts what the fp64 twin counts


@pytest.mark.gpu
@pytest.mark.parametrize("case", LOSS_CASES, ids=_lid)
def test_silog_fwd_bwd_vs_fp64(case):
    """Loss and gradient (upstream gradient 1.5) against the fp64 restatement; two runs bitwise equal; zero gradient on invalid pixels."""
    from rag_amd.depth import silog_loss
    n, mask, vf = case
    est, gt, ref, twin = _loss_refs(case)
    runs = []
    for _ in range(2):
        e = gpu(est).requires_grad_(True)
        loss = silog_loss(e, gpu(gt), vf)
        (loss * UPSTREAM).backward()
        runs.append((loss.detach(), e.grad))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    _gate(_lid(case), "silog_loss", runs[0][0].reshape(()), ref[0], twin[0], FLOOR_SILOG)
    _gate(_lid(case), "silog_grad", runs[0][1], ref[1], twin[1], FLOOR_SILOG)
    assert bool((runs[0][1].cpu()[~(gt > 0)] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", METRIC_CASES, ids=lambda c: f"n{c[0]}_{c[1]}")
def test_metrics_vs_fp64(case):
    """The seven non-count outputs under the gate, d1 / d2 / d3 as integer counts equal to the fp64 twin's; two runs bitwise equal."""
    from rag_amd.depth import depth_metrics
    n, mask = case
    est, gt, ref, twin = _metric_refs(n, mask)
    a, b = depth_metrics(gpu(est), gpu(gt)).tensor, depth_metrics(gpu(est), gpu(gt)).tensor
    torch.cuda.synchronize()
    got = a.cpu().double()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    floor = _metric_floor(ref)
    for k in _metric_gated(gt):
        e_kernel, e_twin = float((got[k] - ref[k]).abs()), float((twin[k] - ref[k]).abs())
        scale = max(float(ref[k].abs()), 1e-30)
        print(f"SWEEP case=n{n}_{mask} tensor=metric{k} e_kernel={e_kernel / scale:.3e} e_twin={e_twin / scale:.3e}")
        assert e_kernel <= max(float(floor[k]), NOISE * e_twin), (k, float(got[k]), float(ref[k]))
    valid = int((gt > 0).sum())
    counts = [int(round(float(got[k]) * valid)) for k in (7, 8, 9)]
    want = [int(round(float(ref[k]) * valid)) for k in (7, 8, 9)]
    print(f"SWEEP case=n{n}_{mask} tensor=counts kernel={counts} twin64={want} valid={valid}")
    assert counts == want


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 257, FWD_CAP + 1, ABOVE))
def test_no_valid_pixel(n):
    """gt of zeros, negatives and NaN only: the metrics are ten NaNs, the loss is NaN and its gradient all zero."""
    from rag_amd.depth import depth_metrics, silog_loss
    est, gt = _pixels(n, "none")
    assert not bool((gt > 0).any())
    m = depth_metrics(gpu(est), gpu(gt)).tensor
    e = gpu(est).requires_grad_(True)
    loss = silog_loss(e, gpu(gt), 0.85)
    (loss * UPSTREAM).backward()
    torch.cuda.synchronize()
    assert m.shape == (10,) and bool(torch.isnan(m).all())
    assert bool(torch.isnan(loss))
    assert torch.equal(e.grad, torch.zeros_like(e.grad))
