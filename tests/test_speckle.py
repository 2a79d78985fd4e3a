"""Speckle filter (rag_amd/csrc/speckle.hip; rag_amd.metrics.filter_speckles, Speckles, Network.forward_dense(speckle=...)) against the
plain-torch twin rag_amd.metrics.filter_speckles_torch, and the twin against a breadth-first search written here.

The rule.  A pixel is reliable iff it is kept and its disparity is finite.  Two 4-neighbours are joined iff both are reliable and
fabsf(d_p - d_q) <= max_diff in fp32; a segment is a connected component.  label = the smallest y*W + x of the segment (-1:
unreliable), size = its pixels (0: unreliable), keep = reliable and size > max_size, counts = (reliable, segments, removed pixels,
removed segments, largest), density = float(double(reliable - removed pixels) / double(H W)).

Gates.  Every output is an integer, a flag or a quotient of two integers, and nothing depends on an order of execution, so EVERY
comparison is torch.equal: no tolerance.

Unmarked tests run without a GPU; the rest need the MI355X."""
import ctypes
import functools
import inspect
import math
import re
from collections import deque
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_golden, split_sd
from rag_amd.metrics import SPECKLE_COUNTS, SPECKLE_TILE

DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("ragmi_speckle_workspace_elems", "ragmi_speckle_fwd")
TR, TC = SPECKLE_TILE


# --------------------------------------------------------------------------- references written here
def brute_speckles(disp, keep, max_size, max_diff):
    """The definition as a breadth-first search in raster order -> (label, size, keep, counts).  keep: bool [B,H,W]."""
    B, H, W = disp.shape
    d = disp.numpy().astype(np.float32)
    md = np.float32(max_diff)
    rel = (keep & torch.isfinite(disp)).numpy()
    label = np.full((B, H, W), -1, dtype=np.int32)
    size = np.zeros((B, H, W), dtype=np.int32)
    counts = np.zeros((B, 5), dtype=np.int32)
    with np.errstate(over="ignore"):
        for b in range(B):
            for y0 in range(H):
                for x0 in range(W):
                    if not rel[b, y0, x0] or label[b, y0, x0] >= 0:
                        continue
                    root, members, queue = y0 * W + x0, [], deque([(y0, x0)])      # raster order: the first pixel met is the smallest
                    label[b, y0, x0] = root
                    while queue:
                        y, x = queue.popleft()
                        members.append((y, x))
                        for ny, nx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                            if 0 <= ny < H and 0 <= nx < W and rel[b, ny, nx] and label[b, ny, nx] < 0 \
                                    and np.abs(d[b, y, x] - d[b, ny, nx]) <= md:
                                label[b, ny, nx] = root
                                queue.append((ny, nx))
                    for y, x in members:
                        size[b, y, x] = len(members)
                    gone = len(members) <= max_size
                    counts[b] += np.array([len(members), 1, len(members) * gone, gone, 0], dtype=np.int32)
                    counts[b, 4] = max(counts[b, 4], len(members))
    size_t = torch.from_numpy(size)
    return torch.from_numpy(label), size_t, torch.from_numpy(rel) & (size_t > max_size), torch.from_numpy(counts)


def plant(disp, keep, g, n=3):
    """NaN, +Inf and -Inf under kept and under unkept pixels where the map has them (in place)."""
    flat_d, flat_k = disp.view(-1), keep.reshape(-1)
    for want in (True, False):
        idx = (flat_k == want).nonzero().flatten()
        if idx.numel() == 0:
            continue
        pick = idx[torch.randperm(idx.numel(), generator=g)[:n]]
        for i, value in zip(pick.tolist(), (math.nan, math.inf, -math.inf)):
            flat_d[i] = value


def draw(shape, density, g):
    """9 x 9 cells of levels 3 px apart plus uniform noise of +-0.45 px (neighbours inside a cell differ by at most 0.9, cells of
    different levels by at least 2.1), a random keep of the given density, non-finite values planted under both -> (disp, keep)."""
    B, H, W = shape
    cells = torch.randint(0, 6, (B, (H + 8) // 9, (W + 8) // 9), generator=g)
    level = cells.repeat_interleave(9, 1).repeat_interleave(9, 2)[:, :H, :W].float() * 3
    disp = (level + (torch.rand(shape, generator=g) * 0.9 - 0.45)).float().contiguous()
    keep = torch.rand(shape, generator=g) < density
    plant(disp, keep, g)
    return disp, keep


def same(got, want):
    """Speckles against Speckles: the five outputs each equal, dtypes as documented."""
    return (got.keep.dtype == torch.bool and got.label.dtype == torch.int32 and got.size.dtype == torch.int32
            and got.counts.dtype == torch.int32 and got.density.dtype == torch.float32
            and torch.equal(got.keep.cpu(), want.keep.cpu()) and torch.equal(got.label.cpu(), want.label.cpu())
            and torch.equal(got.size.cpu(), want.size.cpu()) and torch.equal(got.counts.cpu(), want.counts.cpu())
            and torch.equal(got.density.cpu(), want.density.cpu()))


def same_fill(got, want):
    return (torch.equal(got.disp.cpu(), want.disp.cpu()) and torch.equal(got.code.cpu(), want.code.cpu())
            and torch.equal(got.counts.cpu(), want.counts.cpu()) and torch.equal(got.density.cpu(), want.density.cpu()))


def next_up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


# --------------------------------------------------------------------------- CPU
def test_worked_example():
    from rag_amd.metrics import filter_speckles_torch
    nan, inf = math.nan, math.inf
    disp = torch.tensor([[[5.0, 5.8, 6.6, 9.0, 9.0, nan],
                          [1.0, 1.0, 6.6, 9.0, 20.0, 20.0],
                          [1.0, 30.0, 30.0, 9.0, 20.0, 21.0],
                          [1.0, 30.0, 40.0, 9.0, inf, 21.0]]])
    got = filter_speckles_torch(disp, None, max_size=3, max_diff=1.0)
    assert got.label.tolist() == [[[0, 0, 0, 3, 3, -1], [6, 6, 0, 3, 10, 10], [6, 13, 13, 3, 10, 10], [6, 13, 20, 3, -1, 10]]]
    assert got.size.tolist() == [[[4, 4, 4, 5, 5, 0], [4, 4, 4, 5, 5, 5], [4, 3, 3, 5, 5, 5], [4, 3, 1, 5, 0, 5]]]
    t, f = True, False
    assert got.keep.tolist() == [[[t, t, t, t, t, f], [t, t, t, t, t, t], [t, f, f, t, t, t], [t, f, f, t, f, t]]]
    assert got.removed.tolist() == [[[f, f, f, f, f, f], [f, f, f, f, f, f], [f, t, t, f, f, f], [f, t, t, f, f, f]]]
    assert got.counts.tolist() == [[22, 6, 4, 2, 5]] and got.density.tolist() == [0.75]
    assert len(SPECKLE_COUNTS) == 5 and SPECKLE_COUNTS[2] == "removed_pixels"
    label, size, keep, counts = brute_speckles(disp, torch.ones_like(disp, dtype=torch.bool), 3, 1.0)
    assert torch.equal(label, got.label) and torch.equal(size, got.size) and torch.equal(keep, got.keep) and torch.equal(counts, got.counts)


@pytest.mark.parametrize("shape,density", (((2, 37, 131), 0.85), ((2, 37, 131), 0.6), ((1, 70, 67), 0.7)),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_twin_is_the_brute_force(shape, density):
    from rag_amd.metrics import filter_speckles_torch
    g = torch.Generator().manual_seed(int(1000 * density) + shape[2])
    disp, keep = draw(shape, density, g)
    got = filter_speckles_torch(disp, keep, max_size=12, max_diff=1.0)
    label, size, kept, counts = brute_speckles(disp, keep, 12, 1.0)
    print(f"SPECKLE_TWIN {shape} density={density} counts={got.counts.tolist()}")
    assert torch.equal(got.label, label) and torch.equal(got.size, size)
    assert torch.equal(got.keep, kept) and torch.equal(got.counts, counts)
    H, W = shape[1:]
    assert torch.equal(got.density, ((counts[:, 0] - counts[:, 2]).double() / (H * W)).float())
    assert torch.equal(got.removed, (label >= 0) & ~kept)
    for b in range(shape[0]):                                  # the draw holds a removed and a kept segment in every image
        assert 0 < int(counts[b, 3]) < int(counts[b, 1]) and int(counts[b, 4]) > 12, counts[b].tolist()
    assert bool(((got.label < 0) & keep & ~torch.isfinite(disp)).any()) and bool(((got.label < 0) & ~keep).any())


def test_semantics():
    from rag_amd.metrics import filter_speckles_torch as twin
    # a segment of exactly max_size pixels goes, one of max_size + 1 stays
    disp = torch.tensor([[[1.0, 1.0, 1.0, 9.0, 9.0, 9.0, 9.0]]])
    got = twin(disp, None, max_size=3)
    assert got.keep.tolist() == [[[False] * 3 + [True] * 4]] and got.counts.tolist() == [[7, 2, 3, 1, 4]]
    # |d_p - d_q| == max_diff joins; the next float above does not
    assert twin(torch.tensor([[[5.0, 6.0]]]), None, 0, 1.0).label.tolist() == [[[0, 0]]]
    assert twin(torch.tensor([[[5.0, next_up(6.0)]]]), None, 0, 1.0).label.tolist() == [[[0, 1]]]
    assert twin(torch.tensor([[[5.0], [6.0]]]), None, 0, 1.0).label.tolist() == [[[0], [0]]]
    assert twin(torch.tensor([[[5.0], [next_up(6.0)]]]), None, 0, 1.0).label.tolist() == [[[0], [1]]]
    assert twin(torch.tensor([[[5.0, 5.0]]]), None, 0, 0.0).label.tolist() == [[[0, 0]]]
    # similarity is per edge: the ramp is one segment although its ends are 1.6 apart
    assert twin(torch.tensor([[[5.0, 5.8, 6.6]]]), None, 0, 1.0).size.tolist() == [[[3, 3, 3]]]
    # a difference that overflows to Inf does not join
    assert twin(torch.tensor([[[3e38, -3e38]]]), None, 0, 3.4e38).label.tolist() == [[[0, 1]]]
    # diagonal contact does not join
    diag = twin(torch.tensor([[[1.0, 50.0], [50.0, 1.0]]]), torch.tensor([[[1, 0], [0, 1]]], dtype=torch.bool), 0, 1.0)
    assert diag.label.tolist() == [[[0, -1], [-1, 3]]] and diag.counts.tolist() == [[2, 2, 0, 0, 1]]
    # max_size = 0: keep == reliable; keep=None is an all-true mask; the keep dtypes agree
    g = torch.Generator().manual_seed(2)
    disp, keep = draw((2, 11, 23), 0.6, g)
    pure = twin(disp, keep, max_size=0)
    assert torch.equal(pure.keep, keep & torch.isfinite(disp)) and torch.equal(pure.keep, pure.label >= 0)
    assert pure.counts[:, 2:4].tolist() == [[0, 0], [0, 0]]
    assert same(twin(disp, None, 5), twin(disp, torch.ones_like(keep), 5))
    want = twin(disp, keep, 5)
    weight = torch.where(keep, torch.tensor(1.0), torch.tensor(0.25))
    from rag_amd.metrics import LRCheck, filter_speckles
    for form in (keep.to(torch.uint8) * 7, weight, weight.double(), LRCheck(weight, None, torch.zeros(2))):
        assert same(twin(disp, form, 5), want)
        assert same(filter_speckles(disp, form, 5), want)                                    # CPU tensors: the twin
    both = twin(disp.double(), keep, 5)                                                      # the twin works in the inputs' dtype
    assert same(both, want)
    everything = twin(disp, keep, max_size=11 * 23)
    assert not bool(everything.keep.any()) and torch.equal(everything.counts[:, 2], everything.counts[:, 0])
    assert everything.density.tolist() == [0.0, 0.0]


def test_symmetry():
    """keep and size commute with a flip along x, a flip along y and a transpose of the inputs; label need not."""
    from rag_amd.metrics import filter_speckles_torch as twin
    g = torch.Generator().manual_seed(4)
    disp, keep = draw((2, 23, 31), 0.7, g)
    want = twin(disp, keep, 6)
    for name, op in (("flip_x", lambda t: t.flip(-1)), ("flip_y", lambda t: t.flip(-2)), ("transpose", lambda t: t.transpose(1, 2))):
        got = twin(op(disp).contiguous(), op(keep).contiguous(), 6)
        assert torch.equal(got.keep, op(want.keep)) and torch.equal(got.size, op(want.size)), name
        assert torch.equal(got.counts, want.counts) and torch.equal(got.density, want.density), name


def test_wrapper_refusals_and_the_fill_takes_speckles():
    from rag_amd.metrics import fill_disparity, fill_disparity_torch, filter_speckles, filter_speckles_torch
    disp, keep = torch.zeros(1, 3, 4), torch.ones(1, 3, 4, dtype=torch.bool)
    for fn in (filter_speckles, filter_speckles_torch):
        with pytest.raises(ValueError, match="B, H, W"):
            fn(disp[0], keep[0])
        with pytest.raises(ValueError, match="B, H, W"):
            fn(disp, keep[:, :2])
        with pytest.raises(ValueError, match="B, H, W"):
            fn(disp[:, :0], None)
        with pytest.raises(TypeError, match="keep"):
            fn(disp, keep.to(torch.int32))
        with pytest.raises(TypeError, match="floating"):
            fn(disp.to(torch.int32), keep)
        with pytest.raises(TypeError, match="tensor"):
            fn(disp, [[1]])
        for bad in (-1, True, 2.0, 2.5, None):
            with pytest.raises(ValueError, match="max_size"):
                fn(disp, keep, max_size=bad)
        for bad in (-0.5, math.nan, math.inf, 1e39, True, None):
            with pytest.raises(ValueError, match="max_diff"):
                fn(disp, keep, max_diff=bad)
        with pytest.raises(RuntimeError, match="CPU and a GPU"):
            fn(disp, keep.to("meta"))
    with pytest.raises(RuntimeError, match="inference only"):
        filter_speckles(disp.clone().requires_grad_(True), keep)
    with pytest.raises(RuntimeError, match="inference only"):
        filter_speckles(disp, torch.ones(1, 3, 4).requires_grad_(True))
    with torch.no_grad():
        assert filter_speckles(disp.clone().requires_grad_(True), keep).keep.requires_grad is False
    g = torch.Generator().manual_seed(6)
    disp, keep = draw((2, 19, 40), 0.7, g)
    spk = filter_speckles(disp, keep, 8)
    assert int(spk.removed.sum()) > 0
    for median in (0, 3):
        for fill in (fill_disparity, fill_disparity_torch):
            assert same_fill(fill(disp, spk, median=median), fill_disparity_torch(disp, spk.keep, median=median))
    assert torch.equal(fill_disparity_torch(disp, spk).density, spk.density)


def test_abi_validates_before_launch():
    """Status -1 with its message before any launch: the pointers are fake and never dereferenced."""
    import rag_amd
    lib = rag_amd.load_library()
    assert lib.ragmi_version() >= 610
    fake = ctypes.c_void_p(0x1000)

    def call(disp=fake, keep=fake, kind=1, B=2, H=4, W=5, max_size=3, max_diff=1.0, ws=fake, label=fake, size=fake, keep_out=fake,
             counts=fake, density=fake):
        return lib.ragmi_speckle_fwd(disp, keep, kind, B, H, W, max_size, max_diff, ws, label, size, keep_out, counts, density, None)
    for name in ("disp", "keep", "ws", "label", "size", "keep_out", "counts", "density"):
        assert call(**{name: None}) == -1 and b"null" in lib.ragmi_last_error(), name
    assert call(keep=None, kind=0) == -1 and b"null" in lib.ragmi_last_error()
    assert call(keep=None, kind=2, B=0) == -1 and b"bad size" in lib.ragmi_last_error()       # kind 2 may come without a keep
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(W=-3)):
        assert call(**kw) == -1 and b"bad size" in lib.ragmi_last_error(), kw
    assert call(max_size=-1) == -1 and b"max_size" in lib.ragmi_last_error()
    for value in (-1.0, math.nan, math.inf, -math.inf):
        assert call(max_diff=value) == -1 and b"max_diff" in lib.ragmi_last_error(), value
    for kind in (-1, 3, 7):
        assert call(kind=kind) == -1 and b"keep_kind" in lib.ragmi_last_error(), kind
    assert call(ws=ctypes.c_void_p(0x1002)) == -1 and b"aligned" in lib.ragmi_last_error()
    for kw in (dict(B=0x7fffffff, H=TR + 1, W=1), dict(B=1, H=0x10000, W=0x10000), dict(B=0x7fffffff, H=1, W=TC + 1)):
        assert call(**kw) == -1 and b"too many" in lib.ragmi_last_error(), kw


def test_workspace_formula_and_tile():
    """Three elements per pixel (parent, tile-local count, total) and five counts per workgroup of 1024 pixels."""
    import rag_amd
    lib = rag_amd.load_library()
    for B, H, W in ((1, 1, 1), (3, 7, 257), (2, 32, 32), (16, 384, 1248)):
        assert lib.ragmi_speckle_workspace_elems(B, H, W) == 3 * B * H * W + 5 * B * ((H * W + 1023) // 1024), (B, H, W)
    assert lib.ragmi_speckle_workspace_elems(0, 4, 4) == 0
    for B, H, W in ((0x7fffffff, 0x7fffffff, 0x7fffffff), (1, 0x10000, 0x10000), (0x7fffffff, TR + 1, 1)):   # sizes the launch refuses
        assert lib.ragmi_speckle_workspace_elems(B, H, W) == 0, (B, H, W)
    header = (ROOT / "include" / "rag_amd.h").read_text()
    assert int(re.search(r"#define RAGMI_SPECKLE_TILE_ROWS (\d+)", header).group(1)) == TR
    assert int(re.search(r"#define RAGMI_SPECKLE_TILE_COLS (\d+)", header).group(1)) == TC
    assert int(re.search(r"#define RAGMI_SPECKLE_COUNTS (\d+)", header).group(1)) == len(SPECKLE_COUNTS)


def test_symbols_are_declared_bound_and_exported():
    import rag_amd
    from rag_amd._lib import SIGNATURES
    header = (ROOT / "include" / "rag_amd.h").read_text()
    lib = rag_amd.load_library()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in SIGNATURES and hasattr(lib, name), name
    assert len(SIGNATURES["ragmi_speckle_fwd"][1]) == 15 and len(SIGNATURES["ragmi_speckle_workspace_elems"][1]) == 3
    for name in ("Speckles", "filter_speckles", "filter_speckles_torch"):
        assert name in rag_amd.__all__ and hasattr(rag_amd, name), name
    assert rag_amd.metrics.SPECKLE_TILE == (TR, TC)
    for cls in (rag_amd.Network, rag_amd.checkpoint.MultiTaskStereo):
        assert inspect.signature(cls.forward_dense).parameters["speckle"].default is None, cls
    d, c, n, s = torch.zeros(1, 1, 1), torch.zeros(1, 1, 1, dtype=torch.uint8), torch.zeros(1, 6, dtype=torch.int32), torch.ones(1)
    assert rag_amd.FilledDisp(d, c, n, s).speckles is None
    assert rag_amd.FilledDisp(d, c, n, s, "spk").speckles == "spk"
    depth = rag_amd.DepthNetwork.__new__(rag_amd.DepthNetwork)          # the type decides; nothing of it is run
    with pytest.raises(NotImplementedError, match="second view"):
        depth.forward_dense(torch.zeros(1, 3, 6, 6), torch.zeros(1, 3, 6, 6), 0, speckle=(12, 1.0))


# --------------------------------------------------------------------------- GPU
HEIGHTS = (1, 2, TR - 1, TR, TR + 1, 2 * TR + 1)
WIDTHS = (1, 2, TC - 1, TC, TC + 1, 2 * TC - 1, 2 * TC, 2 * TC + 1, 4 * TC + 1)
LOW, HIGH = 5.0, 50.0                                          # two levels that never join at max_diff = 1


def serpentine(H, W):
    """Corridor rows (LOW) at even y, wall rows (HIGH) at odd y with one corridor pixel at alternating ends: one segment that visits
    every even row, whose smallest index is at one end and which crosses every seam; the walls are segments of their own."""
    disp = torch.full((H, W), LOW)
    for y in range(1, H, 2):
        disp[y] = HIGH
        disp[y, W - 1 if (y // 2) % 2 == 0 else 0] = LOW
    return disp


def spiral(H, W):
    """A one-pixel corridor that winds inwards from (0, 0), one pixel of wall between its turns."""
    m = torch.zeros((H, W), dtype=torch.bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True

    def free(y, x, dy, dx):
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= ny < H and 0 <= nx < W) or m[ny, nx]:
            return False
        return not (0 <= ay < H and 0 <= ax < W and m[ay, ax])
    while True:
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy
            if not free(y, x, dy, dx):
                break
        y, x = y + dy, x + dx
        m[y, x] = True
    return torch.where(m, torch.tensor(LOW), torch.tensor(HIGH))


def patterns(H, W, g):
    """[(name, disp [H,W], keep bool [H,W])]: the cases of the sweep at one shape; the patterns that keep every pixel stand together,
    so that batches of them can also run with keep=None."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    every = torch.ones((H, W), dtype=torch.bool)
    out = []

    def add(name, disp, keep=every):
        out.append((name, disp.float().contiguous(), keep.clone()))
    add("none", torch.full((H, W), LOW), ~every)
    add("checker_keep", torch.full((H, W), LOW), (yy + xx) % 2 == 0)                           # singletons
    corner = ~every                                                                            # two blocks that touch only diagonally,
    cy, cx = (TR, TC) if H > TR and W > TC else (H // 2, W // 2)                               # at a tile corner where there is one
    corner[max(0, cy - 3):cy, max(0, cx - 3):cx] = True
    corner[cy:cy + 3, cx:cx + 3] = True
    add("diagonal_corner", torch.full((H, W), LOW), corner)
    for density in (0.4, 0.7, 0.95):
        disp, keep = draw((1, H, W), density, g)
        add(f"random_{density}", disp[0], keep[0])
    add("all_equal", torch.full((H, W), LOW))                                                  # one segment of H W
    add("checker_levels", torch.where((yy + xx) % 2 == 0, LOW, HIGH))                          # all reliable, no edge
    add("row_stripes", torch.where(yy % 2 == 0, LOW, HIGH))
    add("column_stripes", torch.where(xx % 2 == 0, LOW, HIGH))
    add("serpentine_x", serpentine(H, W))
    add("serpentine_y", serpentine(W, H).t())
    add("spiral", spiral(H, W))
    add("comb", torch.where((xx % 2 == 0) | (yy == H - 1), LOW, HIGH))                         # the teeth meet on the last row only
    add("ramp_exact", xx.float())                                                              # slope == max_diff: one segment
    add("ramp_above", xx.float() * (1 + 2.0 ** -10))                                           # exact in fp32: every step is 1 + 2^-10
    # a segment that crosses a seam through exactly one pixel: the first column (row) behind the seam is wall but for one pixel
    if W > TC:
        for r0 in sorted({0, TR // 2, TR - 1, TR, H - 1} & set(range(H))):
            add(f"vertical_seam_at_{r0}", torch.where((xx == TC) & (yy != r0), HIGH, LOW))
    if H > TR:
        for x0 in sorted({0, TC // 2, TC - 1, TC, W - 1} & set(range(W))):
            add(f"horizontal_seam_at_{x0}", torch.where((yy == TR) & (xx != x0), HIGH, LOW))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("W", WIDTHS)
def test_speckle_sweep_against_the_twin(W):
    """Every pattern at every height, in batches of three (consecutive patterns) and alone, the keep as bool / uint8 / fp32 weight and,
    where every pixel is kept, None; max_size 0, 12 and H W.  The twin runs once per shape and max_size on the stacked patterns."""
    from rag_amd.metrics import filter_speckles, filter_speckles_torch
    for H in HEIGHTS:
        g = torch.Generator().manual_seed(1000 * H + W)
        pats = patterns(H, W, g)
        names = [p[0] for p in pats]
        disp, keep = torch.stack([p[1] for p in pats]), torch.stack([p[2] for p in pats])
        d_dev, k_dev = disp.to(DEV), keep.to(DEV)
        forms = (k_dev, k_dev.to(torch.uint8) * 3, torch.where(k_dev, 1.0, 0.25))
        full = [bool(p[2].all()) for p in pats]
        n = len(pats)
        batches = [[i, (i + 1) % n, (i + 2) % n] for i in range(0, n, 3)] + [[i] for i in range(n)]
        for max_size in (0, 12, H * W):
            want = filter_speckles_torch(disp, keep, max_size, 1.0)
            one = names.index("all_equal")
            assert want.counts[one].tolist() == [H * W, 1, H * W * (max_size >= H * W), int(max_size >= H * W), H * W]
            assert want.counts[names.index("none")].tolist() == [0, 0, 0, 0, 0]
            assert want.counts[names.index("ramp_exact")].tolist()[:2] == [H * W, 1]
            assert want.counts[names.index("ramp_above")].tolist()[:2] == [H * W, W]
            assert want.counts[names.index("serpentine_x")].tolist()[4] == int((disp[names.index("serpentine_x")] == LOW).sum())
            if H > TR and W > TC:                              # the two blocks at the tile corner stay two
                assert want.counts[names.index("diagonal_corner")].tolist()[:2] == [9 + min(3, H - TR) * min(3, W - TC), 2]
            if max_size == H * W:
                assert not bool(want.keep.any())
            for j, idx in enumerate(batches):
                ks = [forms[j % 3][idx]] + ([None] if all(full[i] for i in idx) else [])
                for k in ks:
                    got = filter_speckles(d_dev[idx], k, max_size, 1.0)
                    tag = (H, W, max_size, [names[i] for i in idx], None if k is None else k.dtype)
                    assert got.keep.dtype == torch.bool and got.label.dtype == torch.int32 and got.size.dtype == torch.int32, tag
                    assert torch.equal(got.label.cpu(), want.label[idx]), tag
                    assert torch.equal(got.size.cpu(), want.size[idx]), tag
                    assert torch.equal(got.keep.cpu(), want.keep[idx]), tag
                    assert torch.equal(got.counts.cpu(), want.counts[idx]) and got.counts.dtype == torch.int32, tag
                    assert torch.equal(got.density.cpu(), want.density[idx]) and got.density.dtype == torch.float32, tag
                    assert torch.equal(got.removed.cpu(), want.removed[idx]), tag


@pytest.mark.gpu
def test_the_bench_width_once():
    """(2, 70, 1248): 19.5 tiles along x, 4.4 along y; the random draw and a serpentine, at max_size 12 and 100."""
    from rag_amd.metrics import filter_speckles, filter_speckles_torch
    g = torch.Generator().manual_seed(1248)
    disp, keep = draw((2, 70, 1248), 0.8, g)
    disp[1] = serpentine(70, 1248)
    keep[1] = True
    for max_size in (12, 100):
        want = filter_speckles_torch(disp, keep, max_size, 1.0)
        print(f"SPECKLE_BENCH_WIDTH max_size={max_size} counts={want.counts.tolist()}")
        assert int(want.counts[0, 3]) > 0 and int(want.counts[1, 4]) == 35 * 1248 + 35
        assert same(filter_speckles(disp.to(DEV), keep.to(DEV), max_size, 1.0), want), max_size


def _raw(disp, keep, max_size, max_diff, poison):
    """ragmi_speckle_fwd on outputs and a workspace pre-filled with NaN / 0xFF patterns -> (label, size, keep_out, counts, density)."""
    import rag_amd
    lib = rag_amd.load_library()
    B, H, W = disp.shape
    ws = torch.full((lib.ragmi_speckle_workspace_elems(B, H, W),), poison, device=DEV, dtype=torch.int32)
    label = torch.full((B, H, W), poison, device=DEV, dtype=torch.int32)
    size = torch.full((B, H, W), poison, device=DEV, dtype=torch.int32)
    keep_out = torch.full((B, H, W), 0xFF, device=DEV, dtype=torch.uint8)
    counts = torch.full((B, 5), poison, device=DEV, dtype=torch.int32)
    density = torch.full((B,), math.nan, device=DEV)
    if keep is None:
        kind, ptr = 2, None
    else:
        k = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
        kind, ptr = int(k.dtype == torch.uint8), k.data_ptr()
    rc = lib.ragmi_speckle_fwd(disp.data_ptr(), ptr, kind, B, H, W, max_size, max_diff, ws.data_ptr(), label.data_ptr(), size.data_ptr(),
                               keep_out.data_ptr(), counts.data_ptr(), density.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ragmi_last_error()
    torch.cuda.synchronize()
    return label, size, keep_out, counts, density


@functools.lru_cache(maxsize=None)
def _case(B, H, W, seed=0):
    """One shared, never modified case: the random draw at 0.7, one image of it with nothing kept when there are several."""
    g = torch.Generator().manual_seed(7 * H + W + seed)
    disp, keep = draw((B, H, W), 0.7, g)
    if B > 1:
        keep[1] = False
    return disp.to(DEV), keep.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((3, TR + 1, 2 * TC + 1), (1, 7, 257), (3, 3, 65)), ids=lambda s: "x".join(map(str, s)))
def test_abi_writes_everything_it_reads_and_repeats_bitwise(shape):
    from rag_amd.metrics import filter_speckles, filter_speckles_torch
    disp, keep = _case(*shape)
    want = filter_speckles_torch(disp.cpu(), keep.cpu(), 5, 1.0)
    weight = torch.where(keep, 1.0, 0.0)
    runs = [_raw(disp, keep, 5, 1.0, -1), _raw(disp, keep, 5, 1.0, 0x7fc00000), _raw(disp, keep, 5, 1.0, 0x7fc00000),
            _raw(disp, weight, 5, 1.0, -1), _raw(disp, weight, 5, 1.0, 0x01010101)]
    for label, size, keep_out, counts, density in runs:
        assert torch.equal(label.cpu(), want.label) and torch.equal(size.cpu(), want.size)
        assert torch.equal(keep_out.cpu(), want.keep.to(torch.uint8))                         # 0 / 1 bytes: nothing of 0xFF is left
        assert torch.equal(counts.cpu(), want.counts) and torch.equal(density.cpu(), want.density)
    every = _raw(disp, None, 5, 1.0, -1)
    want_all = filter_speckles_torch(disp.cpu(), None, 5, 1.0)
    assert torch.equal(every[0].cpu(), want_all.label) and torch.equal(every[3].cpu(), want_all.counts)
    again = filter_speckles(disp, keep, 5, 1.0)
    assert torch.equal(again.label, runs[0][0]) and torch.equal(again.keep.view(torch.uint8), runs[0][2])


@pytest.mark.gpu
def test_graph_capture_replays_with_new_inputs():
    """filter_speckles -> fill_disparity(median=3) captured once on static inputs; each replay after new inputs were copied in equals
    the twin chain on those inputs."""
    from rag_amd.metrics import fill_disparity, fill_disparity_torch, filter_speckles, filter_speckles_torch
    shape = (3, TR + 1, 2 * TC + 1)
    static_d, static_k = (t.clone() for t in _case(*shape))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fill_disparity(static_d, filter_speckles(static_d, static_k, 5, 1.0), median=3, fill_value=2.0)   # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            spk = filter_speckles(static_d, static_k, 5, 1.0)
            dense = fill_disparity(static_d, spk, median=3, fill_value=2.0)
    torch.cuda.current_stream().wait_stream(side)
    for seed in (1, 2):
        disp, keep = _case(*shape, seed=seed)
        static_d.copy_(disp)
        static_k.copy_(keep)
        for t in (spk.keep, spk.label, spk.size, spk.counts, spk.density, dense.disp, dense.code, dense.counts, dense.density):
            t.fill_(0)                                                                       # only a replay can put the values back
        graph.replay()
        torch.cuda.synchronize()
        want = filter_speckles_torch(disp.cpu(), keep.cpu(), 5, 1.0)
        assert int(want.counts[:, 3].sum()) > 0
        assert same(spk, want), seed
        assert same_fill(dense, fill_disparity_torch(disp.cpu(), want, median=3, fill_value=2.0)), seed


@pytest.mark.gpu
def test_non_contiguous_inputs_and_unbuilt_dtypes():
    from rag_amd.metrics import filter_speckles, filter_speckles_torch
    g = torch.Generator().manual_seed(3)
    wide, _ = draw((2, 20, 150), 1.0, g)
    _, keep = draw((2, 20, 70), 0.7, g)
    wide_dev, keep_dev = wide.to(DEV), keep.to(DEV)
    assert not wide_dev[..., 3:73].is_contiguous()
    assert same(filter_speckles(wide_dev[..., 3:73], keep_dev, 5), filter_speckles_torch(wide[..., 3:73], keep, 5))
    assert same(filter_speckles(wide_dev[..., 3:73], None, 5), filter_speckles_torch(wide[..., 3:73], None, 5))
    keep_t = keep_dev.transpose(1, 2).contiguous().transpose(1, 2)                           # a keep map with permuted strides
    assert not keep_t.is_contiguous()
    assert same(filter_speckles(wide_dev[..., 3:143:2], keep_t, 5), filter_speckles_torch(wide[..., 3:143:2], keep, 5))
    d = torch.zeros((1, 3, 4), device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        filter_speckles(d.double(), torch.ones((1, 3, 4), device=DEV, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="float32"):
        filter_speckles(d, torch.ones((1, 3, 4), device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="float32"):
        filter_speckles(d.half(), None)
    with pytest.raises(RuntimeError, match="CPU and a GPU"):
        filter_speckles(d, torch.ones((1, 3, 4), dtype=torch.bool))


def _network(ra, g6, g13):
    """The network of test_disp_fill.py: g13's genotype rows and maxdisp, g6's weights, evaluation mode, no gradients."""
    rows = g13["rows"]
    net = ra.Network(ra.Genotype(rows, None, rows, None), DEV, maxdisp=int(g13["maxdisp"]))
    net.load_state_dict(split_sd(g6), strict=True)
    net = net.to(DEV).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net


@pytest.mark.gpu
def test_forward_dense_with_speckle_is_filter_then_fill_per_view():
    import rag_amd as ra
    ra.load_library()
    g6, g = load_golden("g6_train_step"), load_golden("g13_selfsup_train_step")
    left, right = torch.as_tensor(g["left"]).to(DEV), torch.as_tensor(g["right"]).to(DEV)
    net = _network(ra, g6, g)
    kw = dict(abs_tol=1.0, rel_tol=0.05, occluded_weight=0.25)
    disp_l, disp_r, chk_l, chk_r = net.forward_lr(left, right, 0, net.arch_init, **kw)
    serve = ra.checkpoint.MultiTaskStereo(net, [net.arch_init])
    for median in (0, 3):
        dense_l, dense_r, got_l, got_r = net.forward_dense(left, right, 0, net.arch_init, median=median, fill_value=1.0,
                                                           speckle=(12, 1.0), **kw)
        torch.cuda.synchronize()
        assert torch.equal(got_l.weight, chk_l.weight) and torch.equal(got_r.weight, chk_r.weight)
        for dense, disp, chk in ((dense_l, disp_l, chk_l), (dense_r, disp_r, chk_r)):
            want = ra.filter_speckles_torch(disp, chk, 12, 1.0)
            print(f"FORWARD_DENSE_SPECKLE median={median} counts={dense.speckles.counts.tolist()}")
            assert isinstance(dense, ra.FilledDisp) and isinstance(dense.speckles, ra.Speckles)
            assert same(dense.speckles, want)
            assert same_fill(dense, ra.fill_disparity_torch(disp, dense.speckles.keep, median=median, fill_value=1.0))
            assert torch.equal(dense.density, dense.speckles.density)
            assert bool(torch.isfinite(dense.disp).all())
        again = serve.forward_dense(left, right, 0, median=median, fill_value=1.0, speckle=(12, 1.0), **kw)
        assert same_fill(again[0], dense_l) and same_fill(again[1], dense_r)
        assert same(again[0].speckles, dense_l.speckles) and same(again[1].speckles, dense_r.speckles)
        plain = net.forward_dense(left, right, 0, net.arch_init, median=median, fill_value=1.0, **kw)
        none = net.forward_dense(left, right, 0, net.arch_init, median=median, fill_value=1.0, speckle=None, **kw)
        for a, b in zip(plain[:2], none[:2]):
            assert same_fill(a, b) and a.speckles is None and b.speckles is None
        assert serve.forward_dense(left, right, 0, median=median, fill_value=1.0, **kw)[0].speckles is None
    with pytest.raises(ValueError, match="speckle"):
        net.forward_dense(left, right, 0, net.arch_init, speckle=12)
    with pytest.raises(ValueError, match="max_size"):
        net.forward_dense(left, right, 0, net.arch_init, speckle=(-1, 1.0))
