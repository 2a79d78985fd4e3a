"""Device-side batch preparation (rag_amd.data, rag_amd/csrc/prep.hip): the fused crop / pad / normalise / gt launch, the colour
statistics and the colour transfer, against the REFERENCE's own loaders (g21_prep; generator tests/golden/make_golden_prep.py)
and against the plain-torch twins (prepare_batch_torch, color_stats_torch, transfer_color_torch).

Images and ground truth are compared for EQUALITY (torch.equal): the arithmetic is the reference's fp32 expression, and a byte has
only 256 values.  The colour statistics are float64 reductions whose order differs between numpy, torch and the kernel: their gate
is 1e-12 relative, about 20x the 5.5e-14 by which a differently ordered float64 restatement differed from numpy on synthetic
images up to 540x960.  The transferred uint8 image may then differ where a pixel sits within that error of a truncation boundary:
at most 1 level, on at most 1e-5 of the pixels (a condition; 0 were found in 1.5 M pixels with statistics perturbed at 5e-14).
Measured on the MI355X: statistics 8.8e-16 relative to the reference's, 2.0e-16 to the float64 twin; 0 of 251 301 pixels differ.

Unmarked tests run without a GPU; the rest need the MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

DEV = "cuda:0"
STATS_RTOL = 1e-12
TC_MAX_SHARE = 1e-5


@pytest.fixture(scope="module")
def g21():
    return load_golden("g21_prep")


@pytest.fixture(scope="module")
def lib():
    import rag_amd
    return rag_amd.load_library()


def _t(a, dev="cpu"):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _sources(g, tag, dev="cpu"):
    """(left_u8, right_u8, gt) of a fixture sample as B = 1 batches; gt is uint16 (src) or float32 (self)."""
    gt = g["src::gt_u16"] if tag == "src" else g["self::gt_f32"]
    return [_t(g[f"{tag}::left_u8"], dev)[None], _t(g[f"{tag}::right_u8"], dev)[None], _t(gt, dev)[None]]


def _color(g, dev="cpu"):
    return tuple(_t(g[f"self::stats_{n}"], dev)[None] for n in ("left", "right", "real"))


def _check_train(g, tag, out):
    for k, o in zip(("left", "right", "gt"), out):
        ref = _t(g[f"{tag}::train::{k}"])[None]
        assert o.dtype == torch.float32 and torch.equal(o.cpu(), ref), (tag, k)


def _check_eval(g, tag, out):
    top, _ = (int(v) for v in g[f"{tag}::eval::pad"])
    H, W = (int(v) for v in g[f"{tag}::eval::out_hw"])
    for k, o in zip(("left", "right", "gt"), out):
        o = o.cpu()
        win = _t(g[f"{tag}::eval::{k}"])[None]
        w = win.shape[-1]
        assert tuple(o.shape[-2:]) == (H, W)
        assert torch.equal(o[..., top:, :w], win), (tag, k)
        assert not o[..., :top, :].any() and not o[..., :, w:].any(), (tag, k)       # the generator asserted the same of the reference


def _rel(a, b):
    return float(((a - b).abs() / b.abs()).max())


def _image(seed, H, W):
    """Synthetic uint8 image without a constant channel: noise blocks + ramps + per-pixel noise."""
    r = np.random.RandomState(seed)
    blocks = np.kron(r.rand(H // 8 + 1, W // 8 + 1, 3), np.ones((8, 8, 1)))[:H, :W]
    ramp = np.linspace(0, 1, W)[None, :, None] * r.rand(3) + np.linspace(0, 1, H)[:, None, None] * r.rand(3)
    x = 0.5 * blocks + 0.4 * ramp + 0.1 * r.rand(H, W, 3)
    return np.clip(x * 255 * r.uniform(0.6, 1.1), 0, 255).astype(np.uint8)


def _batch(seed, B, H, W, gt="u16"):
    r = np.random.RandomState(seed + 1000)
    left = torch.from_numpy(np.stack([_image(seed + 2 * b, H, W) for b in range(B)]))
    right = torch.from_numpy(np.stack([_image(seed + 2 * b + 1, H, W) for b in range(B)]))
    if gt == "u16":
        g = torch.from_numpy(r.randint(0, 65536, (B, H, W)).astype(np.uint16))
    else:
        g = torch.from_numpy((r.rand(B, H, W) * 192).astype(np.float32))
    return left, right, g


# --------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("tag", ["src", "self"])
def test_prepare_batch_torch_matches_reference_crop(g21, tag):
    from rag_amd.data import prepare_batch_torch
    left, right, gt = _sources(g21, tag)
    origin = _t(g21[f"{tag}::train::origin"])[None]
    out = prepare_batch_torch(left, right, gt, out_hw=(192, 384), origin=origin, color=_color(g21) if tag == "self" else None)
    _check_train(g21, tag, out)


@pytest.mark.parametrize("tag", ["src", "self"])
def test_prepare_batch_torch_matches_reference_pad(g21, tag):
    from rag_amd.data import prepare_batch_torch
    left, right, gt = _sources(g21, tag)
    out = prepare_batch_torch(left, right, gt, out_hw=tuple(g21[f"{tag}::eval::out_hw"]), pad=tuple(g21[f"{tag}::eval::pad"]),
                              color=_color(g21) if tag == "self" else None)
    _check_eval(g21, tag, out)


def test_color_twins_match_reference(g21):
    from rag_amd.data import color_stats_torch, transfer_color_torch
    real = _t(g21["self::real_u8"])[None]
    for name in ("left", "right", "real"):
        st = color_stats_torch(_t(g21[f"self::{name}_u8"])[None])
        assert st.dtype == torch.float64 and tuple(st.shape) == (1, 3, 2)
        rel = _rel(st[0], _t(g21[f"self::stats_{name}"]))
        print(f"color_stats_torch vs reference, {name}: {rel:.3e} relative")
        assert rel <= STATS_RTOL
    for name in ("left", "right"):
        out = transfer_color_torch(_t(g21[f"self::{name}_u8"])[None], real)
        assert out.dtype == torch.uint8 and torch.equal(out[0], _t(g21[f"self::tc_{name}"]))


def test_abi_validation(lib):
    P = ctypes.c_void_p
    x = (ctypes.c_double * 64)()                      # a valid, aligned host address: validation never dereferences it
    p = ctypes.cast(x, P)
    mean_std = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)

    def prep(left_u8=p, right_u8=None, gt=None, gt_dtype=0, origin=p, left=p, right=None, gt_out=None, B=1, Hs=8, Ws=8, H=8, W=8,
             stats=(None, None, None)):
        return lib.ragmi_prep_batch(left_u8, right_u8, gt, gt_dtype, 1.0, origin, left, right, gt_out, B, Hs, Ws, H, W, *mean_std,
                                    *stats, None)

    assert prep(left_u8=None) == -1 and b"null" in lib.ragmi_last_error()
    assert prep(left=None) == -1 and prep(origin=None) == -1
    assert prep(right_u8=p) == -1 and prep(right=p) == -1            # the pair goes together
    assert prep(gt=p) == -1 and prep(gt_out=p) == -1
    assert prep(B=0) == -1 and prep(Hs=0) == -1 and prep(W=-3) == -1
    assert prep(stats=(p, None, None)) == -1                          # view statistics without the source's
    assert prep(gt=p, gt_out=p, gt_dtype=7) == -2 and b"dtype" in lib.ragmi_last_error()
    assert lib.ragmi_color_stats(None, 1, 8, 8, p, p, None) == -1 and b"null" in lib.ragmi_last_error()
    assert lib.ragmi_color_stats(p, 1, 0, 8, p, p, None) == -1
    assert lib.ragmi_color_transfer(p, None, p, p, 1, 8, 8, None) == -1
    assert lib.ragmi_color_transfer(p, p, p, p, 1, 8, 0, None) == -1
    # (sum u, sum u^2) per (32-row chunk, column, channel), in 8-byte elements
    assert lib.ragmi_color_stats_workspace_elems(2, 400, 881) == 2 * 13 * 881 * 3 * 2
    assert lib.ragmi_color_stats_workspace_elems(1, 32, 5) == 1 * 1 * 5 * 3 * 2
    assert lib.ragmi_color_stats_workspace_elems(0, 32, 5) == 0


def test_random_crop_origin_in_range():
    from rag_amd.data import random_crop_origin
    gen = torch.Generator().manual_seed(5)
    o = random_crop_origin(4096, (200, 400), (192, 384), generator=gen, device="cpu")
    assert o.dtype == torch.int32 and tuple(o.shape) == (4096, 2)
    assert int(o[:, 0].min()) == 0 and int(o[:, 0].max()) == 8 and int(o[:, 1].min()) == 0 and int(o[:, 1].max()) == 16
    assert int(random_crop_origin(16, (192, 384), (192, 384), device="cpu").abs().max()) == 0
    with pytest.raises(ValueError):
        random_crop_origin(1, (100, 384), (192, 384), device="cpu")


def test_argument_checks(lib):
    import rag_amd
    from rag_amd.data import prepare_batch, prepare_batch_torch
    left, right, gt = _batch(3, 2, 20, 30)
    assert rag_amd.prepare_batch is prepare_batch
    for fn in (prepare_batch, prepare_batch_torch):                  # raised before any launch, so checkable without a GPU
        with pytest.raises(ValueError):
            fn(left, right, gt, out_hw=(24, 40), pad=(4, 9))         # 20+4 x 30+9 is not 24 x 40
        with pytest.raises(ValueError):
            fn(left, right, gt, out_hw=(24, 40))                     # neither origin nor pad
        with pytest.raises(ValueError):
            fn(left, right, gt, out_hw=(24, 40), origin=(0, 0), pad=(4, 10))
        with pytest.raises(ValueError):
            fn(left.permute(0, 3, 1, 2), out_hw=(8, 8), origin=(0, 0))            # not HWC
        with pytest.raises(ValueError):
            fn(left.float(), out_hw=(8, 8), origin=(0, 0))
        with pytest.raises(ValueError):
            fn(left, right, gt.to(torch.int32), out_hw=(8, 8), origin=(0, 0))     # gt dtype
        with pytest.raises(ValueError):
            fn(left, right[:1], out_hw=(8, 8), origin=(0, 0))
        with pytest.raises(ValueError):
            fn(left, out_hw=(8, 8), origin=torch.zeros((3, 2), dtype=torch.int32))
        with pytest.raises(ValueError):
            fn(left, out_hw=(8, 8), origin=(0, 0), color=(torch.zeros((2, 3, 2)), None, torch.zeros((2, 3, 2))))   # float32 statistics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prepare_batch(left, right, gt, out_hw=(8, 8), origin=(0, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag_amd.color_stats(left)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag_amd.transfer_color(left, right)


def test_twin_origin_rule_outside_source():
    """The one rule, on the twin: a window partly outside the source on every side is zero there and the source elsewhere."""
    from rag_amd.data import prepare_batch_torch
    left, _, gt = _batch(9, 2, 12, 10, gt="f32")
    origin = torch.tensor([[-3, -2], [5, 4]], dtype=torch.int32)
    lo, _, go = prepare_batch_torch(left, None, gt, out_hw=(16, 14), origin=origin, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    full = left.permute(0, 3, 1, 2).float() / 255
    assert torch.equal(lo[0, :, 3:15, 2:12], full[0]) and not lo[0, :, :3].any() and not lo[0, :, 15:].any() and not lo[0, :, :, :2].any() \
        and not lo[0, :, :, 12:].any()
    assert torch.equal(lo[1, :, :7, :6], full[1, :, 5:, 4:]) and not lo[1, :, 7:].any() and not lo[1, :, :, 6:].any()
    assert torch.equal(go[1, :7, :6], gt[1, 5:, 4:]) and not go[1, 7:].any()


# --------------------------------------------------------------------------- GPU
def _both(left, right, gt, **kw):
    """(kernel outputs, twin outputs computed on the CPU) for the same call; color statistics move with the inputs."""
    from rag_amd.data import prepare_batch, prepare_batch_torch
    kw_dev = dict(kw)
    if isinstance(kw.get("origin"), torch.Tensor):
        kw_dev["origin"] = kw["origin"].to(DEV)
    if kw.get("color") is not None:
        kw_dev["color"] = tuple(s.to(DEV) if s is not None else None for s in kw["color"])
    dev = lambda t: t.to(DEV) if t is not None else None  # noqa: E731
    out = prepare_batch(dev(left), dev(right), dev(gt), **kw_dev)
    ref = prepare_batch_torch(left, right, gt, **kw)
    return out, ref


def _assert_equal(out, ref):
    for k, (o, r) in enumerate(zip(out, ref)):
        assert (o is None) == (r is None)
        if o is not None:
            assert o.dtype == torch.float32 and o.shape == r.shape and torch.equal(o.cpu(), r), f"output {k}"


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["src", "self"])
def test_prepare_batch_matches_reference(g21, tag):
    from rag_amd.data import prepare_batch
    left, right, gt = _sources(g21, tag, DEV)
    color = _color(g21, DEV) if tag == "self" else None
    out = prepare_batch(left, right, gt, out_hw=(192, 384), origin=_t(g21[f"{tag}::train::origin"], DEV)[None], color=color)
    _check_train(g21, tag, out)
    out = prepare_batch(left, right, gt, out_hw=tuple(g21[f"{tag}::eval::out_hw"]), pad=tuple(g21[f"{tag}::eval::pad"]), color=color)
    _check_eval(g21, tag, out)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(200, 400), (211, 397)])
def test_prepare_batch_crop_and_pad_match_twin(B, hw):
    from rag_amd.data import random_crop_origin
    left, right, gt = _batch(11, B, *hw)
    origin = random_crop_origin(B, hw, (192, 384), generator=torch.Generator().manual_seed(B), device="cpu")
    _assert_equal(*_both(left, right, gt, out_hw=(192, 384), origin=origin))
    _assert_equal(*_both(left, right, gt, out_hw=(480, 960), pad=(480 - hw[0], 960 - hw[1])))


@pytest.mark.gpu
def test_prepare_batch_odd_width_and_byte_phases():
    """W % 4 != 0 (the scalar-store path), and crops whose first source byte 3 * x1 has every phase modulo 4."""
    left, right, gt = _batch(21, 4, 211, 397, gt="f32")
    _assert_equal(*_both(left, right, gt, out_hw=(211, 397), origin=(0, 0)))
    _assert_equal(*_both(left, right, gt, out_hw=(190, 391), origin=torch.tensor([[3, 0], [0, 1], [21, 2], [7, 3]], dtype=torch.int32)))
    origin = torch.tensor([[0, 4], [1, 7], [2, 10], [3, 13]], dtype=torch.int32)
    assert sorted(int(3 * x) % 4 for x in origin[:, 1]) == [0, 1, 2, 3]
    _assert_equal(*_both(left, right, gt, out_hw=(192, 384), origin=origin))


@pytest.mark.gpu
def test_prepare_batch_origin_partly_outside():
    left, right, gt = _batch(31, 4, 100, 150)
    origin = torch.tensor([[-7, -5], [40, 90], [-30, 100], [99, 149]], dtype=torch.int32)       # before, past the far edge, mixed, one pixel
    out, ref = _both(left, right, gt, out_hw=(96, 128), origin=origin)
    _assert_equal(out, ref)
    assert not out[0][0, :, :7].any() and not out[0][0, :, :, :5].any() and not out[0][1, :, 60:].any() and not out[0][1, :, :, 60:].any()
    far = torch.tensor([[1000, 0], [0, -1000], [-2 ** 31, 2 ** 31 - 1], [2 ** 31 - 1, -2 ** 31]], dtype=torch.int32)   # nothing inside
    out, ref = _both(left, right, gt, out_hw=(96, 128), origin=far)
    _assert_equal(out, ref)
    assert not out[0].any() and not out[2].any()
    _assert_equal(*_both(left, right, gt, out_hw=(96, 127), origin=origin))                     # the same through the scalar path


@pytest.mark.gpu
def test_prepare_batch_optional_inputs_and_gt_dtypes():
    left, right, g16 = _batch(41, 2, 60, 84)
    _, _, g32 = _batch(41, 2, 60, 84, gt="f32")
    out, ref = _both(left, None, g16, out_hw=(48, 64), origin=(5, 9))          # the depth network's case
    _assert_equal(out, ref)
    assert out[1] is None and torch.equal(out[2].cpu(), (g16.view(torch.int16).to(torch.int32) & 0xFFFF)[:, 5:53, 9:73].float() / 256)
    out, ref = _both(left, right, g32, out_hw=(48, 64), origin=(5, 9))
    _assert_equal(out, ref)
    assert torch.equal(out[2].cpu(), g32[:, 5:53, 9:73])
    out, ref = _both(left, right, None, out_hw=(48, 64), origin=(5, 9))
    _assert_equal(out, ref)
    assert out[2] is None
    _assert_equal(*_both(left, None, None, out_hw=(48, 64), origin=(5, 9)))


@pytest.mark.gpu
def test_prepare_batch_out_and_custom_mean_std():
    from rag_amd.data import prepare_batch, prepare_batch_torch
    left, right, gt = _batch(51, 2, 60, 84)
    bufs = (torch.full((2, 3, 48, 64), 7.0, device=DEV), torch.full((2, 3, 48, 64), 7.0, device=DEV), torch.full((2, 48, 64), 7.0, device=DEV))
    ptrs = [b.data_ptr() for b in bufs]
    kw = dict(out_hw=(48, 64), origin=(-4, 30), mean=(0.1, 0.25, 0.7), std=(0.3, 1.7, 0.013))
    out = prepare_batch(left.to(DEV), right.to(DEV), gt.to(DEV), out=bufs, **kw)
    assert [o.data_ptr() for o in out] == ptrs
    _assert_equal(out, prepare_batch_torch(left, right, gt, **kw))
    with pytest.raises(ValueError):
        prepare_batch(left.to(DEV), right.to(DEV), gt.to(DEV), out=(bufs[0], bufs[1], None), **kw)
    with pytest.raises(ValueError):
        prepare_batch(left.to(DEV), right.to(DEV), gt.to(DEV), out=(bufs[0], bufs[1][:, :, :, :32], bufs[2]), **kw)


@pytest.mark.gpu
def test_prepare_batch_depth_sizes():
    """rag_depth's sizes: 400x881 -> a 384x768 crop and the 480x960 pad (too large for a fixture: against the twin)."""
    from rag_amd.data import random_crop_origin
    left, _, gt = _batch(61, 2, 400, 881)
    origin = random_crop_origin(2, (400, 881), (384, 768), generator=torch.Generator().manual_seed(6), device="cpu")
    _assert_equal(*_both(left, None, gt, out_hw=(384, 768), origin=origin))
    _assert_equal(*_both(left, None, gt, out_hw=(480, 960), pad=(80, 79)))


@pytest.mark.gpu
def test_color_stats_matches_reference(g21):
    from rag_amd.data import color_stats, color_stats_torch
    worst = 0.0
    for name in ("left", "right", "real"):
        st = color_stats(_t(g21[f"self::{name}_u8"], DEV)[None])
        assert st.dtype == torch.float64 and tuple(st.shape) == (1, 3, 2)
        worst = max(worst, _rel(st[0].cpu(), _t(g21[f"self::stats_{name}"])))
    big = torch.from_numpy(np.stack([_image(70 + b, 400, 881) for b in range(3)]))        # batched, against the float64 twin
    worst_twin = _rel(color_stats(big.to(DEV)).cpu(), color_stats_torch(big))
    print(f"color_stats: {worst:.3e} relative to the reference's float64 statistics, {worst_twin:.3e} to the twin at 3x400x881")
    assert worst <= STATS_RTOL and worst_twin <= STATS_RTOL


def _tc_check(got, ref, what):
    d = (got.to(torch.int32) - ref.to(torch.int32)).abs()
    share = float((d > 0).float().mean())
    print(f"{what}: {int((d > 0).sum())} of {d.numel()} pixels differ, max {int(d.max())} level(s)")
    assert int(d.max()) <= 1 and share <= TC_MAX_SHARE


@pytest.mark.gpu
def test_transfer_color_standalone_and_fused(g21):
    from rag_amd.data import color_stats, prepare_batch, prepare_batch_torch, transfer_color
    left, right, _ = _sources(g21, "self", DEV)
    real = _t(g21["self::real_u8"], DEV)[None]
    tc = {n: transfer_color(v, real) for n, v in (("left", left), ("right", right))}
    for n in ("left", "right"):
        assert tc[n].dtype == torch.uint8
        _tc_check(tc[n][0].cpu(), _t(g21[f"self::tc_{n}"]), f"transfer_color({n}) vs the reference")
    # the fused path with the kernel's own statistics == the normalisation of the stand-alone uint8 image, exactly
    stats = (color_stats(left), color_stats(right), color_stats(real))
    fused = prepare_batch(left, right, None, out_hw=(224, 400), origin=(-6, -2), color=stats)
    plain = prepare_batch_torch(tc["left"].cpu(), tc["right"].cpu(), None, out_hw=(224, 400), origin=(-6, -2))
    _assert_equal(fused, plain)
    # a larger batch with odd byte counts per sample (the scalar path of the stand-alone kernel) against the float64 twin
    from rag_amd.data import transfer_color_torch
    tgt = torch.from_numpy(np.stack([_image(80 + b, 131, 97) for b in range(3)]))
    src = torch.from_numpy(np.stack([_image(90 + b, 60, 75) for b in range(3)]))
    _tc_check(transfer_color(tgt.to(DEV), src.to(DEV)).cpu(), transfer_color_torch(tgt, src), "transfer_color 3x131x97 vs the twin")


@pytest.mark.gpu
def test_determinism():
    from rag_amd.data import color_stats, prepare_batch
    left, right, gt = (t.to(DEV) for t in _batch(101, 3, 211, 397))
    s1, s2 = color_stats(left), color_stats(left)
    assert torch.equal(s1, s2)
    color = (s1, color_stats(right), color_stats(left.flip(0)))
    origin = torch.tensor([[0, 1], [10, 2], [19, 13]], dtype=torch.int32, device=DEV)
    a = prepare_batch(left, right, gt, out_hw=(192, 384), origin=origin, color=color)
    b = prepare_batch(left, right, gt, out_hw=(192, 384), origin=origin, color=color)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_graph_capture_replays_with_new_origin_and_bytes():
    from rag_amd.data import color_stats, prepare_batch
    from rag_amd.train import graph_census
    B, hw, out_hw = 2, (211, 397), (192, 384)
    left, right, gt = (t.to(DEV) for t in _batch(111, B, *hw))
    real = torch.from_numpy(np.stack([_image(120 + b, 150, 230) for b in range(B)])).to(DEV)
    stats_real = color_stats(real)
    origin = torch.tensor([[0, 1], [10, 2]], dtype=torch.int32, device=DEV)
    bufs = (torch.empty((B, 3, *out_hw), device=DEV), torch.empty((B, 3, *out_hw), device=DEV), torch.empty((B, *out_hw), device=DEV))

    def step():
        return prepare_batch(left, right, gt, out_hw=out_hw, origin=origin, color=(color_stats(left), color_stats(right), stats_real), out=bufs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step()
    census = graph_census(graph)
    assert census["kernel"] == 5 and census["memcpy"] == 0 and census["memset"] == 0 and census["other"] == 0, census
    graph.instantiate()
    graph.replay()
    first = [b.clone() for b in bufs]
    assert all(torch.equal(x, y) for x, y in zip(first, [t.clone() for t in step()]))
    # new crops and new bytes, in place
    l2, r2, g2 = (t.to(DEV) for t in _batch(113, B, *hw))
    left.copy_(l2), right.copy_(r2), gt.copy_(g2)
    origin.copy_(torch.tensor([[19, 13], [3, 0]], dtype=torch.int32, device=DEV))
    graph.replay()
    replayed = [b.clone() for b in bufs]
    fresh = prepare_batch(left, right, gt, out_hw=out_hw, origin=origin.clone(), color=(color_stats(left), color_stats(right), stats_real))
    assert all(torch.equal(x, y) for x, y in zip(replayed, fresh))
    assert not torch.equal(replayed[0], first[0])


@pytest.mark.gpu
def test_network_from_prepared_batch(g21):
    """rag_amd.Network fed by prepare_batch and by the twin's output uploaded as fp32: identical inputs, identical disparities."""
    import rag_amd
    from rag_amd.data import prepare_batch, prepare_batch_torch
    left, right, gt = _batch(131, 1, 80, 130)
    kw = dict(out_hw=(48, 96), origin=(7, 11))
    dl, dr, _ = prepare_batch(left.to(DEV), right.to(DEV), gt.to(DEV), **kw)
    tl, tr, _ = prepare_batch_torch(left, right, gt, **kw)
    assert torch.equal(dl.cpu(), tl) and torch.equal(dr.cpu(), tr)
    torch.manual_seed(7)
    net = rag_amd.Network(rag_amd.ALL_CONV_GENOTYPE, DEV, maxdisp=48).to(DEV).eval()
    with torch.no_grad():
        a = net(dl, dr, 0, net.arch_init)
        b = net(tl.to(DEV), tr.to(DEV), 0, net.arch_init)
    assert a.shape[-2:] == (48, 96) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
