"""Device-side Lanczos resize and the Cityscapes half-resolution branch of batch preparation (rag_amd.data: lanczos_taps,
resize_lanczos, prepare_batch(resize_hw=...); rag_amd/csrc/prep_resize.hip), against the REFERENCE's own loader (g22_cityscapes;
generator tests/golden/make_golden_cityscapes.py), against Pillow, and against the plain-torch twins.

Everything is compared for EQUALITY (torch.equal / np.array_equal): Pillow's 8-bit pass is integer arithmetic, its 16-bit pass a
float64 sum in a fixed order with separately rounded products, and both are restated operation for operation.  There is no
tolerance anywhere in this file.

Unmarked tests run without a GPU; the rest need the MI355X.  The GPU shapes are small and straddle the kernel's 16 x 64 output
tile; the workload's 2048x1024 size is covered by tools/bench_prep_resize.py, which checks equality before it times."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

DEV = "cuda:0"
# (Hs, Ws) -> (Hr, Wr): both axes down x2; odd sizes, non-integer scales; UPSCALE in y; y skipped (not filtered); the fixture's shape
PILLOW_CASES = [((46, 70), (23, 35)), ((45, 71), (20, 33)), ((12, 70), (20, 33)), ((23, 70), (23, 35)), ((24, 1802), (512, 1024))]
GPU_CASES = PILLOW_CASES[:4] + [((100, 200), (50, 100))]            # the last: several tiles in both directions


@pytest.fixture(scope="module")
def g22():
    return load_golden("g22_cityscapes")


@pytest.fixture(scope="module")
def lib():
    import rag_amd
    return rag_amd.load_library()


def _t(a, dev="cpu"):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _bytes(seed, B, H, W):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (B, H, W, 3)).astype(np.uint8))


def _holes16(seed, B, H, W):
    """Random 16-bit values with 40 % zero holes: the ringing next to a hole undershoots below 0 and next to a bright value
    overshoots past 65535, so both clips of the 16-bit path are exercised."""
    r = np.random.RandomState(seed)
    d = r.randint(0, 65536, (B, H, W)).astype(np.uint16)
    d[r.rand(B, H, W) < 0.4] = 0
    return torch.from_numpy(d)


@pytest.fixture(scope="module")
def twin_cases():
    """Inputs and twin results of the GPU resize cases, computed once: {(case, B): (u8, u16, twin_u8, twin_u16)}."""
    from rag_amd.data import resize_lanczos_torch
    out = {}
    for k, (src, dst) in enumerate(GPU_CASES):
        for B in (1, 3):
            u8, u16 = _bytes(300 + k, B, *src), _holes16(400 + k, B, *src)
            out[(k, B)] = (u8, u16, resize_lanczos_torch(u8, dst), resize_lanczos_torch(u16, dst))
    return out


# --------------------------------------------------------------------------- CPU
def test_prepare_batch_torch_matches_reference_cityscapes(g22):
    from rag_amd.data import CITYSCAPES_HALF, prepare_batch_torch
    assert CITYSCAPES_HALF == dict(resize_hw=(512, 1024), gt_scale=1 / 512)
    assert g22["left_u8"].shape == (24, 1802, 3) and g22["gt_u16"].dtype == np.uint16
    out = prepare_batch_torch(_t(g22["left_u8"])[None], _t(g22["right_u8"])[None], _t(g22["gt_u16"])[None], out_hw=(192, 384),
                              origin=_t(g22["origin"])[None], **CITYSCAPES_HALF)
    _check_g22(g22, out)


def _check_g22(g, out):
    rows = int(g["rows"])
    for k, o in zip(("left", "right", "disparity"), out):
        ref = _t(g[k])
        assert o.dtype == torch.float32 and tuple(o.shape[-2:]) == (192, 384)
        assert torch.equal(o[0, ..., :rows, :].cpu(), ref), k
    assert bool((out[2] == 0).any()) and bool((out[2] > 0).any())            # holes and disparities both inside the crop


@pytest.mark.parametrize("src,dst", PILLOW_CASES)
def test_resize_twin_matches_pillow_rgb(src, dst):
    Image = pytest.importorskip("PIL.Image")
    from rag_amd.data import resize_lanczos_torch
    a = _bytes(sum(src), 1, *src)
    ref = np.array(Image.fromarray(a[0].numpy()).resize((dst[1], dst[0]), Image.LANCZOS))
    got = resize_lanczos_torch(a, dst)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, *dst, 3)
    assert np.array_equal(got[0].numpy(), ref)


@pytest.mark.parametrize("src,dst", PILLOW_CASES)
def test_resize_twin_matches_pillow_i16(src, dst):
    Image = pytest.importorskip("PIL.Image")
    from rag_amd.data import resize_lanczos_torch
    d = _holes16(sum(src), 1, *src)
    im = Image.fromarray(d[0].numpy())
    assert im.mode == "I;16"
    ref = np.array(im.resize((dst[1], dst[0]), Image.LANCZOS))
    got = resize_lanczos_torch(d, dst)
    assert got.dtype == torch.uint16 and ref.dtype == np.uint16 and tuple(got.shape) == (1, *dst)
    assert np.array_equal(got[0].numpy(), ref)
    if src[1] != dst[1]:                                             # the input does exercise the negative clip
        assert int((ref == 0).sum()) > 0


@pytest.mark.parametrize("n,m", [(70, 35), (71, 33), (12, 20), (1802, 1024), (24, 512), (2048, 1024), (4096, 8)])
def test_lanczos_taps_tables(n, m):
    import math
    from rag_amd.data import lanczos_taps
    b, ki, kd = lanczos_taps(n, m)
    ks = 2 * math.ceil(3 * max(n / m, 1.0)) + 1
    assert b.dtype == torch.int32 and tuple(b.shape) == (m, 2) and not b.is_cuda
    assert ki.dtype == torch.int32 and kd.dtype == torch.float64 and tuple(ki.shape) == tuple(kd.shape) == (m, ks)
    xmin, ln = b[:, 0].to(torch.int64), b[:, 1].to(torch.int64)
    assert int(xmin.min()) >= 0 and int(ln.min()) >= 1 and int((xmin + ln).max()) <= n and int(ln.max()) <= ks
    assert bool((xmin[1:] >= xmin[:-1]).all()) and bool(((xmin + ln)[1:] >= (xmin + ln)[:-1]).all())     # the window rule relies on it
    past = torch.arange(ks)[None, :] >= ln[:, None]
    assert not ki[past].any() and not kd[past].any()
    # each fixed-point tap is within 1/2 of k * 2^22 and the float taps sum to 1: the integer taps sum to 2^22 +- len / 2 (+- len asked)
    assert bool(((ki.to(torch.int64).sum(1) - (1 << 22)).abs() <= ln).all())
    assert float((kd.sum(1) - 1.0).abs().max()) < 1e-12


def test_lanczos_taps_periodic_and_identity():
    from rag_amd.data import lanczos_taps
    b, ki, kd = lanczos_taps(2048, 1024)
    inner = slice(3, 1021)                                           # outputs whose 12 taps all lie inside the source
    assert ki.shape[1] == 13 and bool((b[inner, 1] == 12).all()) and torch.equal(b[inner, 0], 2 * torch.arange(3, 1021, dtype=torch.int32) - 5)
    assert bool((ki[inner] == ki[3]).all()) and bool((kd[inner] == kd[3]).all())      # (i + 0.5) * 2 is exact: the same taps for every i
    b, ki, kd = lanczos_taps(23, 23)                                 # an axis Pillow does not filter
    assert torch.equal(b, torch.stack((torch.arange(23, dtype=torch.int32), torch.ones(23, dtype=torch.int32)), 1))
    assert tuple(ki.shape) == (23, 1) and bool((ki == 1 << 22).all()) and bool((kd == 1.0).all())
    with pytest.raises(ValueError):
        lanczos_taps(0, 5)


def test_argument_checks_resize(lib):
    import rag_amd
    from rag_amd.data import CITYSCAPES_HALF, prepare_batch, prepare_batch_torch, resize_lanczos, resize_lanczos_torch
    assert rag_amd.resize_lanczos is resize_lanczos and rag_amd.lanczos_taps is rag_amd.data.lanczos_taps
    left, right, g16 = _bytes(1, 2, 20, 30), _bytes(2, 2, 20, 30), _holes16(3, 2, 20, 30)
    stats = tuple(torch.zeros((2, 3, 2), dtype=torch.float64) for _ in range(3))
    for fn in (prepare_batch, prepare_batch_torch):                  # raised before any launch, so checkable without a GPU
        with pytest.raises(ValueError, match="color"):
            fn(left, right, g16, out_hw=(8, 8), origin=(0, 0), resize_hw=(10, 15), color=stats)
        with pytest.raises(ValueError, match="float32"):
            fn(left, right, g16.float(), out_hw=(8, 8), origin=(0, 0), resize_hw=(10, 15))
        with pytest.raises(ValueError):
            fn(left, right, g16, out_hw=(8, 8), origin=(0, 0), resize_hw=(0, 15))
        with pytest.raises(ValueError):
            fn(left, right, g16, out_hw=(24, 40), pad=(4, 10), resize_hw=(10, 15))       # the pad addresses the RESIZED 10x15 image
    o = prepare_batch_torch(left, right, g16, out_hw=(14, 25), pad=(4, 10), resize_hw=(10, 15))
    assert tuple(o[0].shape) == (2, 3, 14, 25) and not o[0][:, :, :4].any() and not o[2][:, :, 15:].any()
    # gt_scale alone (no resize) only rescales the ground truth
    a = prepare_batch_torch(left, None, g16, out_hw=(8, 8), origin=(1, 2), gt_scale=1 / 512)
    b = prepare_batch_torch(left, None, g16, out_hw=(8, 8), origin=(1, 2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2] / 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prepare_batch(left, right, g16, out_hw=(8, 8), origin=(0, 0), **CITYSCAPES_HALF)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resize_lanczos(left, (10, 15))
    for fn in (resize_lanczos, resize_lanczos_torch):
        with pytest.raises(ValueError):
            fn(left.float(), (10, 15))
        with pytest.raises(ValueError):
            fn(left[..., 0], (10, 15))                               # a single-channel uint8 image is not built
        with pytest.raises(ValueError):
            fn(left, (10, 0))


def test_abi_validation_resize(lib):
    P = ctypes.c_void_p
    x = (ctypes.c_double * 64)()                                     # a valid, aligned host address: validation never dereferences it
    p = ctypes.cast(x, P)
    mean_std = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
    for name in ("ragmi_prep_batch_resized", "ragmi_resize_lanczos_u8", "ragmi_resize_lanczos_u16"):
        assert hasattr(lib, name)

    def prep(left_u8=p, right_u8=None, gt=None, gt_dtype=1, origin=p, left=p, right=None, gt_out=None, B=1, src=(16, 16), res=(8, 8), H=8, W=8,
             yt=(p, p, p, 13), xt=(p, p, p, 13)):
        return lib.ragmi_prep_batch_resized(left_u8, right_u8, gt, gt_dtype, 1.0, origin, left, right, gt_out, B, *src, *res, H, W, *mean_std,
                                            *yt, *xt, None)

    assert prep(left_u8=None) == -1 and b"null" in lib.ragmi_last_error()
    assert prep(left=None) == -1 and prep(origin=None) == -1
    assert prep(right_u8=p) == -1 and prep(gt=p) == -1               # the pairs go together
    assert prep(yt=(None, p, p, 13)) == -1 and prep(xt=(p, None, p, 13)) == -1
    assert prep(gt=p, gt_out=p, yt=(p, p, None, 13)) == -1           # a gt needs the float64 taps
    assert prep(B=0) == -1 and prep(res=(0, 8)) == -1 and prep(W=-3) == -1
    assert prep(gt=p, gt_out=p, gt_dtype=0) == -2 and b"dtype" in lib.ragmi_last_error()
    assert prep(yt=(p, p, p, 12)) == -1 and b"tap tables" in lib.ragmi_last_error()      # 16 -> 8 has 2 * ceil(3 * 2) + 1 = 13 taps
    # a window that cannot fit the LDS is refused from the sizes alone, before anything touches the device
    assert prep(src=(4096, 64), res=(8, 8), yt=(p, p, p, 3073), xt=(p, p, p, 49)) == -2 and b"LDS" in lib.ragmi_last_error()
    assert lib.ragmi_resize_lanczos_u8(None, p, 1, 16, 16, 8, 8, p, p, 13, p, p, 13, None) == -1 and b"null" in lib.ragmi_last_error()
    assert lib.ragmi_resize_lanczos_u16(p, p, 1, 16, 0, 8, 8, p, p, 13, p, p, 13, None) == -1
    assert lib.ragmi_resize_lanczos_u16(p, p, 1, 4096, 64, 8, 8, p, p, 3073, p, p, 49, None) == -2


# --------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_resize_lanczos_matches_twin(twin_cases, case, B):
    from rag_amd.data import resize_lanczos
    u8, u16, ref8, ref16 = twin_cases[(case, B)]
    dst = GPU_CASES[case][1]
    got8, got16 = resize_lanczos(u8.to(DEV), dst), resize_lanczos(u16.to(DEV), dst)
    assert got8.dtype == torch.uint8 and got16.dtype == torch.uint16
    assert torch.equal(got8.cpu(), ref8) and torch.equal(got16.cpu(), ref16)
    assert int((ref16 == 0).sum()) > 0                               # clipped undershoots are in the comparison


def _batch(seed, B, H, W):
    return _bytes(seed, B, H, W), _bytes(seed + 1, B, H, W), _holes16(seed + 2, B, H, W)


def _both(left, right, gt, **kw):
    """(kernel outputs, twin outputs computed on the CPU) for the same call."""
    from rag_amd.data import prepare_batch, prepare_batch_torch
    kw_dev = dict(kw)
    if isinstance(kw.get("origin"), torch.Tensor):
        kw_dev["origin"] = kw["origin"].to(DEV)
    dev = lambda t: t.to(DEV) if t is not None else None  # noqa: E731
    return prepare_batch(dev(left), dev(right), dev(gt), **kw_dev), prepare_batch_torch(left, right, gt, **kw)


def _assert_equal(out, ref):
    for k, (o, r) in enumerate(zip(out, ref)):
        assert (o is None) == (r is None)
        if o is not None:
            assert o.dtype == torch.float32 and o.shape == r.shape and torch.equal(o.cpu(), r), f"output {k}"


@pytest.mark.gpu
def test_fused_crop_origins_match_twin():
    """100x200 -> 50x100 and a 32x72 crop (3 x 2 tiles, the last column tile 8 wide): origin (0,0), the far corner, origins that put
    tile edges inside the image at odd offsets, one per sample."""
    left, right, gt = _batch(500, 4, 100, 200)
    origin = torch.tensor([[0, 0], [18, 28], [7, 13], [15, 27]], dtype=torch.int32)
    _assert_equal(*_both(left, right, gt, out_hw=(32, 72), origin=origin, resize_hw=(50, 100), gt_scale=1 / 512))
    _assert_equal(*_both(left, right, gt, out_hw=(33, 71), origin=origin, resize_hw=(50, 100)))      # W % 4 != 0: scalar stores
    _assert_equal(*_both(left, right, gt, out_hw=(20, 33), origin=(0, 0), resize_hw=(20, 33)))        # non-integer scales, whole image


@pytest.mark.gpu
def test_fused_pad_and_origin_partly_outside():
    left, right, gt = _batch(510, 4, 45, 71)
    out, ref = _both(left, right, gt, out_hw=(36, 80), pad=(16, 47), resize_hw=(20, 33), gt_scale=1 / 512)      # the evaluation pad
    _assert_equal(out, ref)
    assert not out[0][:, :, :16].any() and not out[0][:, :, :, 33:].any() and out[0][:, :, 16:, :33].any()
    origin = torch.tensor([[-7, -5], [12, 20], [-30, 30], [19, 32]], dtype=torch.int32)      # before, past the far edge, mixed, one pixel
    _assert_equal(*_both(left, right, gt, out_hw=(24, 68), origin=origin, resize_hw=(20, 33)))
    far = torch.tensor([[1000, 0], [0, -1000], [-2 ** 31, 2 ** 31 - 1], [2 ** 31 - 1, -2 ** 31]], dtype=torch.int32)       # nothing inside
    out, ref = _both(left, right, gt, out_hw=(24, 68), origin=far, resize_hw=(20, 33))
    _assert_equal(out, ref)
    assert not out[0].any() and not out[2].any()


@pytest.mark.gpu
def test_fused_optional_inputs_upscale_and_skipped_axis():
    left, right, gt = _batch(520, 2, 12, 70)
    kw = dict(out_hw=(16, 24), origin=(3, 5), resize_hw=(20, 33))                        # an upscale in y
    out, ref = _both(left, None, gt, **kw)                                               # the depth network's case
    _assert_equal(out, ref)
    assert out[1] is None
    out, ref = _both(left, right, None, **kw)
    _assert_equal(out, ref)
    assert out[2] is None
    _assert_equal(*_both(left, None, None, **kw))
    left, right, gt = _batch(523, 2, 23, 70)
    _assert_equal(*_both(left, right, gt, out_hw=(23, 35), origin=(0, 0), resize_hw=(23, 35)))       # y is not filtered


@pytest.mark.gpu
def test_fused_out_and_custom_mean_std():
    from rag_amd.data import prepare_batch, prepare_batch_torch
    left, right, gt = _batch(530, 2, 46, 70)
    bufs = (torch.full((2, 3, 20, 32), 7.0, device=DEV), torch.full((2, 3, 20, 32), 7.0, device=DEV), torch.full((2, 20, 32), 7.0, device=DEV))
    ptrs = [b.data_ptr() for b in bufs]
    kw = dict(out_hw=(20, 32), origin=(-2, 6), mean=(0.1, 0.25, 0.7), std=(0.3, 1.7, 0.013), resize_hw=(23, 35), gt_scale=1 / 512)
    out = prepare_batch(left.to(DEV), right.to(DEV), gt.to(DEV), out=bufs, **kw)
    assert [o.data_ptr() for o in out] == ptrs
    _assert_equal(out, prepare_batch_torch(left, right, gt, **kw))


@pytest.mark.gpu
def test_fused_equals_unfused_route():
    """prepare_batch(resize_hw=...) == prepare_batch(resize_lanczos(...)): the existing kernel on the stand-alone resize."""
    from rag_amd.data import prepare_batch, resize_lanczos
    left, right, gt = (t.to(DEV) for t in _batch(540, 3, 100, 200))
    origin = torch.tensor([[0, 0], [18, 28], [-3, 13]], dtype=torch.int32, device=DEV)
    fused = prepare_batch(left, right, gt, out_hw=(32, 72), origin=origin, resize_hw=(50, 100), gt_scale=1 / 512)
    small = [resize_lanczos(t, (50, 100)) for t in (left, right, gt)]
    unfused = prepare_batch(*small, out_hw=(32, 72), origin=origin, gt_scale=1 / 512)
    assert all(torch.equal(a, b) for a, b in zip(fused, unfused))


@pytest.mark.gpu
def test_fused_matches_reference_cityscapes(g22):
    from rag_amd.data import CITYSCAPES_HALF, prepare_batch
    out = prepare_batch(_t(g22["left_u8"], DEV)[None], _t(g22["right_u8"], DEV)[None], _t(g22["gt_u16"], DEV)[None], out_hw=(192, 384),
                        origin=_t(g22["origin"], DEV)[None], **CITYSCAPES_HALF)
    _check_g22(g22, out)


@pytest.mark.gpu
def test_determinism_resize():
    from rag_amd.data import prepare_batch, resize_lanczos
    left, right, gt = (t.to(DEV) for t in _batch(550, 3, 100, 200))
    origin = torch.tensor([[0, 1], [10, 2], [18, 28]], dtype=torch.int32, device=DEV)
    kw = dict(out_hw=(32, 72), origin=origin, resize_hw=(50, 100))
    a, b = prepare_batch(left, right, gt, **kw), prepare_batch(left, right, gt, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(resize_lanczos(gt, (50, 100)), resize_lanczos(gt, (50, 100)))


@pytest.mark.gpu
def test_graph_capture_replays_with_new_origin_and_bytes_resized():
    from rag_amd.data import prepare_batch
    from rag_amd.train import graph_census
    B, hw, rhw, out_hw = 2, (100, 200), (50, 100), (32, 72)
    left, right, gt = (t.to(DEV) for t in _batch(560, B, *hw))
    origin = torch.tensor([[0, 1], [10, 2]], dtype=torch.int32, device=DEV)
    bufs = (torch.empty((B, 3, *out_hw), device=DEV), torch.empty((B, 3, *out_hw), device=DEV), torch.empty((B, *out_hw), device=DEV))

    def step():
        return prepare_batch(left, right, gt, out_hw=out_hw, origin=origin, resize_hw=rhw, gt_scale=1 / 512, out=bufs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                       # also uploads the tap tables, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step()
    census = graph_census(graph)
    assert census["kernel"] == 1 and census["memcpy"] == 0 and census["memset"] == 0 and census["other"] == 0, census
    graph.instantiate()
    graph.replay()
    first = [b.clone() for b in bufs]
    assert all(torch.equal(x, y) for x, y in zip(first, [t.clone() for t in step()]))
    # new crops and new bytes, in place
    l2, r2, g2 = (t.to(DEV) for t in _batch(563, B, *hw))
    left.copy_(l2), right.copy_(r2), gt.copy_(g2)
    origin.copy_(torch.tensor([[18, 28], [3, 0]], dtype=torch.int32, device=DEV))
    graph.replay()
    replayed = [b.clone() for b in bufs]
    fresh = prepare_batch(left, right, gt, out_hw=out_hw, origin=origin.clone(), resize_hw=rhw, gt_scale=1 / 512)
    assert all(torch.equal(x, y) for x, y in zip(replayed, fresh))
    assert not torch.equal(replayed[0], first[0])


@pytest.mark.gpu
def test_window_past_lds_is_refused():
    """4096x64 -> 8x8: a tile would need all 4096 source rows in LDS.  A refused argument (RAGMI_EUNSUPPORTED from the sizes alone):
    nothing is launched, and the device works afterwards."""
    from rag_amd.data import prepare_batch, resize_lanczos
    left, gt = _bytes(570, 1, 4096, 64).to(DEV), _holes16(571, 1, 4096, 64).to(DEV)
    with pytest.raises(RuntimeError, match="LDS"):
        resize_lanczos(left, (8, 8))
    with pytest.raises(RuntimeError, match="LDS"):
        resize_lanczos(gt, (8, 8))
    with pytest.raises(RuntimeError, match="LDS"):
        prepare_batch(left, None, gt, out_hw=(8, 8), origin=(0, 0), resize_hw=(8, 8))
    torch.cuda.synchronize()
    assert tuple(resize_lanczos(left[:, :64], (8, 8)).shape) == (1, 8, 8, 3)
