"""Dense disparity by background interpolation (rag_amd/csrc/disp_fill.hip; rag_amd.metrics.fill_disparity, FilledDisp,
Network.forward_dense) against the plain-torch twin rag_amd.metrics.fill_disparity_torch, and the twin against a three-loop brute force.

The rule.  A pixel is reliable iff it is kept and its disparity is finite.  On a row with a reliable pixel an unreliable pixel takes
(v[R] < v[L]) ? v[R] : v[L] of its nearest reliable neighbours (code 1) or the only one (code 2); a reliable pixel keeps its bits
(code 0).  A row without one takes the same rule along the columns from the nearest rows that have one (codes 3, 4), or fill_value
(code 5).  median = 3 / 5: the m x m median of the filled map over windows clamped to the image.

Gates.  Every output value is a copy of an input value and every count an integer, so EVERY comparison is torch.equal: no tolerance.
The inputs hold no -0.0 (draw: a zero could only be +0.0).

Unmarked tests run without a GPU; the rest need the MI355X."""
import ctypes
import functools
import math
import re
from pathlib import Path

import pytest
import torch

from conftest import load_golden, split_sd

DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("ragmi_disp_fill_workspace_elems", "ragmi_disp_fill_fwd", "ragmi_disp_median_fwd")


# --------------------------------------------------------------------------- references written here
def brute_fill(disp, keep, fill_value=0.0):
    """The definition in three loops -> (out, code, counts).  keep: bool [B,H,W]."""
    B, H, W = disp.shape
    out = torch.full((B, H, W), float("nan"), dtype=disp.dtype)
    code = torch.full((B, H, W), 255, dtype=torch.uint8)
    rel = keep & torch.isfinite(disp)
    for b in range(B):
        ok_rows = [bool(rel[b, y].any()) for y in range(H)]
        for y in range(H):
            if not ok_rows[y]:
                continue
            for x in range(W):
                if rel[b, y, x]:
                    out[b, y, x], code[b, y, x] = disp[b, y, x], 0
                    continue
                left = next((i for i in range(x - 1, -1, -1) if rel[b, y, i]), None)
                right = next((i for i in range(x + 1, W) if rel[b, y, i]), None)
                if left is not None and right is not None:
                    vl, vr = disp[b, y, left], disp[b, y, right]
                    out[b, y, x], code[b, y, x] = (vr if float(vr) < float(vl) else vl), 1
                else:
                    out[b, y, x], code[b, y, x] = disp[b, y, left if left is not None else right], 2
        for y in range(H):
            if ok_rows[y]:
                continue
            up = next((i for i in range(y - 1, -1, -1) if ok_rows[i]), None)
            down = next((i for i in range(y + 1, H) if ok_rows[i]), None)
            for x in range(W):
                if up is not None and down is not None:
                    vu, vd = out[b, up, x], out[b, down, x]
                    out[b, y, x], code[b, y, x] = (vd if float(vd) < float(vu) else vu), 3
                elif up is not None or down is not None:
                    out[b, y, x], code[b, y, x] = out[b, up if up is not None else down, x], 4
                else:
                    out[b, y, x], code[b, y, x] = fill_value, 5
    counts = torch.stack([(code == c).sum((1, 2)) for c in range(6)], 1).to(torch.int32)
    return out, code, counts


def brute_median(v, m):
    """Sort and pick over windows whose coordinates are clamped to the image (replicate padding)."""
    B, H, W = v.shape
    r = m // 2
    out = torch.empty_like(v)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                win = sorted(float(v[b, min(max(y + j, 0), H - 1), min(max(x + i, 0), W - 1)])
                             for j in range(-r, r + 1) for i in range(-r, r + 1))
                out[b, y, x] = win[(m * m) // 2]
    return out


def draw(shape, g):
    """Disparities of both signs in (-6, 14), float32, no -0.0."""
    return (torch.rand(shape, generator=g) * 20 - 6).float()


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


def same(got, want):
    """FilledDisp against FilledDisp: disp, code, counts, density each equal, dtypes as documented."""
    return (got.disp.dtype == want.disp.dtype and got.code.dtype == torch.uint8 and got.counts.dtype == torch.int32
            and got.density.dtype == torch.float32 and torch.equal(got.disp.cpu(), want.disp.cpu())
            and torch.equal(got.code.cpu(), want.code.cpu()) and torch.equal(got.counts.cpu(), want.counts.cpu())
            and torch.equal(got.density.cpu(), want.density.cpu()))


# --------------------------------------------------------------------------- CPU
def test_worked_row():
    from rag_amd.metrics import fill_disparity_torch
    disp = torch.tensor([[[7.0, 9.0, 3.0, 8.0, 5.0, 6.0]]])
    keep = torch.tensor([[[0, 1, 0, 0, 1, 0]]], dtype=torch.bool)
    got = fill_disparity_torch(disp, keep)
    assert got.disp.tolist() == [[[9.0, 9.0, 5.0, 5.0, 5.0, 5.0]]]
    assert got.code.tolist() == [[[2, 0, 1, 1, 0, 2]]]
    assert got.counts.tolist() == [[2, 2, 2, 0, 0, 0]] and got.density.tolist() == [float(torch.tensor(2 / 6, dtype=torch.float64).float())]
    assert got.filled.tolist() == [[[True, False, True, True, False, True]]]
    out, code, counts = brute_fill(disp, keep)
    assert torch.equal(out, got.disp) and torch.equal(code, got.code) and torch.equal(counts, got.counts)


@pytest.mark.parametrize("W", (1, 2, 7))
@pytest.mark.parametrize("H", (1, 2, 5))
def test_twin_is_the_brute_force(H, W):
    from rag_amd.metrics import fill_disparity_torch
    g = torch.Generator().manual_seed(100 * H + W)
    for B in (1, 2):
        for density in (0.0, 0.1, 0.5, 0.9, 1.0):
            for variant in ("plain", "nonfinite", "empty_row"):
                disp = draw((B, H, W), g)
                keep = torch.rand((B, H, W), generator=g) < density
                if variant == "nonfinite":
                    plant(disp, keep, g)
                if variant == "empty_row":
                    keep[B - 1, H // 2] = False
                    if H > 1:
                        disp[0, 0] = math.nan                     # kept or not, this row has no reliable pixel either
                fill = 0.0 if variant == "plain" else -2.5
                got = fill_disparity_torch(disp, keep, fill_value=fill)
                out, code, counts = brute_fill(disp, keep, fill)
                tag = (B, H, W, density, variant)
                assert torch.equal(got.disp, out) and not bool(torch.isnan(out).any()), tag
                assert torch.equal(got.code, code) and torch.equal(got.counts, counts), tag
                assert torch.equal(got.density, (counts[:, 0].double() / (H * W)).float()), tag
                assert torch.equal(got.counts.sum(1), torch.full((B,), H * W)), tag
                assert bool(torch.isfinite(got.disp).all()), tag
                for m in (3, 5):
                    assert torch.equal(fill_disparity_torch(disp, keep, median=m, fill_value=fill).disp, brute_median(out, m)), (tag, m)


def test_median_twin_is_sort_and_pick():
    from rag_amd.metrics import median_disparity_torch
    g = torch.Generator().manual_seed(5)
    for H, W in ((1, 1), (1, 6), (4, 2), (6, 5)):
        v = draw((2, H, W), g)
        for m in (3, 5):
            assert torch.equal(median_disparity_torch(v, m), brute_median(v, m)), (H, W, m)
    with pytest.raises(ValueError):
        median_disparity_torch(torch.zeros(1, 2, 2), 4)


def test_keep_forms_agree_and_cpu_runs_the_twin():
    from rag_amd.metrics import FilledDisp, LRCheck, fill_disparity, fill_disparity_torch
    g = torch.Generator().manual_seed(11)
    disp = draw((2, 5, 9), g)
    mask = torch.rand((2, 5, 9), generator=g) < 0.5
    weight = torch.where(mask, torch.tensor(1.0), torch.tensor(0.25))
    want = fill_disparity_torch(disp, mask, median=3, fill_value=1.5)
    assert isinstance(want, FilledDisp)
    forms = (mask, mask.to(torch.uint8) * 7, weight, LRCheck(weight, None, torch.zeros(2)), weight.double())
    for keep in forms:
        assert same(fill_disparity_torch(disp, keep, median=3, fill_value=1.5), want)
        assert same(fill_disparity(disp, keep, median=3, fill_value=1.5), want)              # CPU tensors: the twin
    assert same(fill_disparity(disp.double(), mask), fill_disparity_torch(disp.double(), mask))   # the twin works in the inputs' dtype
    assert fill_disparity(disp.double(), mask).disp.dtype == torch.float64
    assert torch.equal(want.filled, want.code != 0)
    plain = fill_disparity(disp, mask)
    assert torch.equal(plain.disp[mask], disp[mask])                                         # median=0: kept pixels keep their bits


def test_wrapper_refusals():
    from rag_amd.metrics import fill_disparity, fill_disparity_torch
    disp, keep = torch.zeros(1, 3, 4), torch.ones(1, 3, 4, dtype=torch.bool)
    for fn in (fill_disparity, fill_disparity_torch):
        with pytest.raises(ValueError, match="B, H, W"):
            fn(disp[0], keep[0])
        with pytest.raises(ValueError, match="B, H, W"):
            fn(disp, keep[:, :2])
        with pytest.raises(ValueError, match="median"):
            fn(disp, keep, median=4)
        with pytest.raises(ValueError, match="fill_value"):
            fn(disp, keep, fill_value=math.nan)
        with pytest.raises(ValueError, match="fill_value"):
            fn(disp, keep, fill_value=math.inf)
        with pytest.raises(TypeError, match="keep"):
            fn(disp, keep.to(torch.int32))
    with pytest.raises(RuntimeError, match="inference only"):
        fill_disparity(disp.clone().requires_grad_(True), keep)
    with pytest.raises(RuntimeError, match="inference only"):
        fill_disparity(disp, torch.ones(1, 3, 4).requires_grad_(True))
    with torch.no_grad():
        assert fill_disparity(disp.clone().requires_grad_(True), keep).disp.requires_grad is False


def test_abi_validates_before_launch():
    """Status -1 with its message before any launch: the pointers are fake and never dereferenced."""
    import rag_amd
    lib = rag_amd.load_library()
    assert lib.ragmi_version() >= 600
    fake, other = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)

    def fill(disp=fake, keep=fake, u8=1, B=2, H=4, W=5, value=0.0, ws=fake, out=fake, code=fake, counts=fake, density=fake):
        return lib.ragmi_disp_fill_fwd(disp, keep, u8, B, H, W, value, ws, out, code, counts, density, None)
    for name in ("disp", "keep", "ws", "out", "code", "counts", "density"):
        assert fill(**{name: None}) == -1 and b"null" in lib.ragmi_last_error(), name
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(W=-3)):
        assert fill(**kw) == -1 and b"bad size" in lib.ragmi_last_error(), kw
    for value in (math.nan, math.inf, -math.inf):
        assert fill(value=value) == -1 and b"fill_value" in lib.ragmi_last_error(), value
    assert fill(ws=ctypes.c_void_p(0x1002)) == -1 and b"aligned" in lib.ragmi_last_error()
    for kw in (dict(B=0x7fffffff, H=8, W=1), dict(B=1, H=0x10000, W=0x10000)):
        assert fill(**kw) == -1 and b"too many" in lib.ragmi_last_error(), kw

    def median(src=fake, dst=other, B=2, H=4, W=5, m=3):
        return lib.ragmi_disp_median_fwd(src, dst, B, H, W, m, None)
    for kw in (dict(src=None), dict(dst=None)):
        assert median(**kw) == -1 and b"null" in lib.ragmi_last_error(), kw
    assert median(dst=fake) == -1 and b"differ" in lib.ragmi_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert median(**kw) == -1 and b"bad size" in lib.ragmi_last_error(), kw
    for m in (0, 1, 4, 7, -3):
        assert median(m=m) == -1 and b"3 or 5" in lib.ragmi_last_error(), m
    assert median(B=0x7fffffff, H=9, W=1) == -1 and b"too many" in lib.ragmi_last_error()


def test_workspace_formula():
    """A flag per row and six counts per workgroup of four rows."""
    import rag_amd
    lib = rag_amd.load_library()
    for B, H, W in ((1, 1, 1), (3, 7, 257), (16, 384, 1248)):
        assert lib.ragmi_disp_fill_workspace_elems(B, H, W) == B * H + 6 * B * ((H + 3) // 4), (B, H, W)
    assert lib.ragmi_disp_fill_workspace_elems(0, 4, 4) == 0


def test_symbols_are_declared_bound_and_exported():
    import rag_amd
    from rag_amd._lib import SIGNATURES
    header = (ROOT / "include" / "rag_amd.h").read_text()
    lib = rag_amd.load_library()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in SIGNATURES and hasattr(lib, name), name
    assert len(SIGNATURES["ragmi_disp_fill_fwd"][1]) == 13 and len(SIGNATURES["ragmi_disp_median_fwd"][1]) == 7
    for name in ("FilledDisp", "fill_disparity", "fill_disparity_torch"):
        assert name in rag_amd.__all__ and hasattr(rag_amd, name), name
    assert hasattr(rag_amd.Network, "forward_dense") and hasattr(rag_amd.checkpoint.MultiTaskStereo, "forward_dense")
    depth = rag_amd.DepthNetwork.__new__(rag_amd.DepthNetwork)          # the type decides; nothing of it is run
    with pytest.raises(NotImplementedError, match="second view"):
        depth.forward_dense(torch.zeros(1, 3, 6, 6), torch.zeros(1, 3, 6, 6), 0)


# --------------------------------------------------------------------------- GPU
WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 257)
HEIGHTS = (1, 2, 3, 5, 7)


def patterns(H, W, g):
    """[(name, disp [H,W], keep bool [H,W])]: the cases of the sweep at one shape.  "none" stands second, so that the batches of three
    (consecutive patterns) hold an empty image between two others."""
    def rnd(density):
        return torch.rand((H, W), generator=g) < density
    out = []

    def add(name, keep, nonfinite=False):
        disp = draw((H, W), g)
        if nonfinite:
            plant(disp, keep, g)
        out.append((name, disp, keep))
    add("all", torch.ones((H, W), dtype=torch.bool))
    add("none", torch.zeros((H, W), dtype=torch.bool))
    add("half", rnd(0.5), nonfinite=True)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        keep = torch.zeros((H, W), dtype=torch.bool)
        keep[y, x] = True
        add(f"corner_{y}_{x}", keep)
    for x in (0, W - 1):
        keep = torch.zeros((H, W), dtype=torch.bool)
        keep[:, x] = True
        add(f"column_{x}", keep)
    for end in (63, 64, 65):                                  # an unreliable run whose last column is `end`: a tile's last lane, the next
        if end < W:                                           # tile's first, and its second
            keep = torch.ones((H, W), dtype=torch.bool)
            keep[:, max(0, end - 5):end + 1] = False
            add(f"run_ends_{end}", keep)
    keep = torch.ones((H, W), dtype=torch.bool)               # a run over every tile but the row's two ends (W = 257: five tiles)
    keep[:, 1:max(1, W - 1)] = False
    add("long_run", keep)
    if W > 200:
        keep = rnd(0.5)
        keep[:, 30:200] = False                               # starts inside tile 0, ends inside tile 3
        add("run_30_199", keep, nonfinite=True)
    for name, rows in (("empty_top", [0]), ("empty_bottom", [H - 1]), ("empty_middle", [H // 2 - 1, H // 2] if H >= 4 else [H // 2]),
                       ("one_row_left", [y for y in range(H) if y != H // 2])):
        keep = rnd(0.5)
        keep[:, W // 2] = True                                # no other row is empty by chance
        keep[rows] = False
        add(name, keep, nonfinite=name == "empty_middle")
    keep = rnd(0.5)                                           # a row that is kept but not finite is empty too
    disp = draw((H, W), g)
    disp[H // 2] = math.nan
    out.append(("nan_row", disp, keep))
    for density in (0.02, 0.5, 0.98):
        add(f"random_{density}", rnd(density), nonfinite=True)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("W", WIDTHS)
def test_fill_sweep_against_the_twin(W):
    """Every pattern at every height, in batches of three (consecutive patterns) and alone, both keep dtypes; the twin runs once per
    shape on the stacked patterns (images are independent of each other)."""
    from rag_amd.metrics import fill_disparity, fill_disparity_torch
    for H in HEIGHTS:
        g = torch.Generator().manual_seed(1000 * H + W)
        pats = patterns(H, W, g)
        names = [p[0] for p in pats]
        disp, keep = torch.stack([p[1] for p in pats]), torch.stack([p[2] for p in pats])
        want = fill_disparity_torch(disp, keep, fill_value=-1.0)
        assert torch.equal(want.counts.sum(1), torch.full((len(pats),), H * W))
        assert want.counts[names.index("none")].tolist() == [0, 0, 0, 0, 0, H * W]
        assert want.counts[names.index("all")].tolist() == [H * W, 0, 0, 0, 0, 0]
        d_dev, k_dev = disp.to(DEV), keep.to(DEV)
        w_dev = torch.where(k_dev, 1.0, 0.25)
        n = len(pats)
        batches = [[i, (i + 1) % n, (i + 2) % n] for i in range(0, n, 3)] + [[i] for i in range(n)]
        for j, idx in enumerate(batches):
            forms = (k_dev[idx], w_dev[idx]) if len(idx) == 3 else ((k_dev[idx], w_dev[idx], k_dev[idx].to(torch.uint8))[j % 3],)
            for k in forms:
                got = fill_disparity(d_dev[idx], k, fill_value=-1.0)
                tag = (H, W, [names[i] for i in idx], k.dtype)
                assert torch.equal(got.disp.cpu(), want.disp[idx]), tag
                assert torch.equal(got.code.cpu(), want.code[idx]), tag
                assert torch.equal(got.counts.cpu(), want.counts[idx]) and got.counts.dtype == torch.int32, tag
                assert torch.equal(got.density.cpu(), want.density[idx]), tag
                assert torch.equal(got.counts.sum(1).cpu(), torch.full((len(idx),), H * W)), tag
                assert torch.equal(got.filled.cpu(), want.code[idx] != 0), tag


@pytest.mark.gpu
@pytest.mark.parametrize("W", (512, 513, 1248))
def test_fill_rows_longer_than_one_batch_of_tiles(W):
    """The row pass loads eight 64-column tiles at a time: exactly one batch, one column more, and the width of the bench (19.5
    tiles), with runs that cross the batches and carries that come from several tiles away."""
    from rag_amd.metrics import fill_disparity, fill_disparity_torch
    g = torch.Generator().manual_seed(W)
    H = 6
    disp = draw((2, H, W), g)
    keep = torch.rand((2, H, W), generator=g) < 0.5
    keep[0, 0] = False
    keep[0, 0, 5] = True                                      # one reliable pixel near the left end: carried to every tile
    keep[0, 1] = False
    keep[0, 1, W - 3] = True                                  # and one near the right end
    keep[0, 2, 100:W - 100] = False                           # a run over the batch boundary
    keep[0, 3] = False                                        # an empty row
    keep[1] = torch.rand((H, W), generator=g) < 0.01
    plant(disp, keep, g)
    want = fill_disparity_torch(disp, keep)
    for k in (keep.to(DEV), torch.where(keep, 1.0, 0.5).to(DEV)):
        assert same(fill_disparity(disp.to(DEV), k), want), k.dtype
    assert same(fill_disparity(disp.to(DEV), keep.to(DEV), median=5), fill_disparity_torch(disp, keep, median=5))


def _raw(disp, keep, fill_value, poison):
    """ragmi_disp_fill_fwd on outputs and a workspace pre-filled with NaN / 0xFF patterns."""
    import rag_amd
    lib = rag_amd.load_library()
    B, H, W = disp.shape
    ws = torch.full((lib.ragmi_disp_fill_workspace_elems(B, H, W),), poison, device=DEV, dtype=torch.int32)
    out = torch.full((B, H, W), math.nan, device=DEV)
    code = torch.full((B, H, W), 0xFF, device=DEV, dtype=torch.uint8)
    counts = torch.full((B, 6), poison, device=DEV, dtype=torch.int32)
    density = torch.full((B,), math.nan, device=DEV)
    k = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
    rc = lib.ragmi_disp_fill_fwd(disp.data_ptr(), k.data_ptr(), int(k.dtype == torch.uint8), B, H, W, fill_value, ws.data_ptr(),
                                 out.data_ptr(), code.data_ptr(), counts.data_ptr(), density.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ragmi_last_error()
    torch.cuda.synchronize()
    return out, code, counts, density


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """One shared, never modified case: random keep at 0.4 with planted non-finite values, an empty row and an empty image."""
    g = torch.Generator().manual_seed(7 * H + W)
    disp = draw((B, H, W), g)
    keep = torch.rand((B, H, W), generator=g) < 0.4
    plant(disp, keep, g)
    keep[0, H // 2] = False
    if B > 1:
        keep[1] = False
    return disp.to(DEV), keep.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((3, 5, 129), (1, 7, 257), (3, 3, 65)), ids=lambda s: "x".join(map(str, s)))
def test_abi_writes_everything_it_reads_and_repeats_bitwise(shape):
    from rag_amd.metrics import fill_disparity, fill_disparity_torch
    disp, keep = _case(*shape)
    want = fill_disparity_torch(disp.cpu(), keep.cpu(), fill_value=2.0)
    weight = torch.where(keep, 1.0, 0.0)
    runs = [_raw(disp, keep, 2.0, -1), _raw(disp, keep, 2.0, 0x7fc00000), _raw(disp, weight, 2.0, -1), _raw(disp, weight, 2.0, 0x7fc00000)]
    for out, code, counts, density in runs:
        assert torch.equal(out.cpu(), want.disp) and torch.equal(code.cpu(), want.code)
        assert torch.equal(counts.cpu(), want.counts) and torch.equal(density.cpu(), want.density)
    again = fill_disparity(disp, keep, fill_value=2.0)
    assert torch.equal(again.disp.view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(again.code, runs[0][1])


@pytest.mark.gpu
def test_graph_capture_replays_to_the_eager_result():
    from rag_amd.metrics import fill_disparity
    disp, keep = _case(3, 5, 129)
    eager = fill_disparity(disp, keep, median=3, fill_value=2.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fill_disparity(disp, keep, median=3, fill_value=2.0)                                 # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            got = fill_disparity(disp, keep, median=3, fill_value=2.0)
    torch.cuda.current_stream().wait_stream(side)
    for t in (got.disp, got.code, got.counts, got.density):
        t.fill_(0)                                                                           # only a replay can put the values back
    graph.replay()
    torch.cuda.synchronize()
    assert same(got, eager)


@pytest.mark.gpu
def test_non_contiguous_inputs_and_unbuilt_dtypes():
    from rag_amd.metrics import fill_disparity, fill_disparity_torch
    g = torch.Generator().manual_seed(3)
    wide, keep = draw((2, 5, 150), g), torch.rand((2, 5, 70), generator=g) < 0.3
    wide_dev, keep_dev = wide.to(DEV), keep.to(DEV)
    want = fill_disparity_torch(wide[..., 3:73], keep)
    assert not wide_dev[..., 3:73].is_contiguous()
    assert same(fill_disparity(wide_dev[..., 3:73], keep_dev), want)
    keep_t = keep_dev.transpose(1, 2).contiguous().transpose(1, 2)                           # a keep map with permuted strides
    assert not keep_t.is_contiguous()
    assert same(fill_disparity(wide_dev[..., 3:143:2], keep_t), fill_disparity_torch(wide[..., 3:143:2], keep))
    d = torch.zeros((1, 3, 4), device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        fill_disparity(d.double(), torch.ones((1, 3, 4), device=DEV, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="float32"):
        fill_disparity(d, torch.ones((1, 3, 4), device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="CPU and a GPU"):
        fill_disparity(d, torch.ones((1, 3, 4), dtype=torch.bool))


@pytest.mark.gpu
@pytest.mark.parametrize("m", (3, 5))
def test_median_against_the_twin(m):
    from rag_amd.metrics import fill_disparity, fill_disparity_torch, median_disparity_torch
    for H in (1, 2, 4, 9):
        for W in (1, 3, 64, 65, 130):
            g = torch.Generator().manual_seed(100 * H + W + m)
            disp = draw((2, H, W), g)
            every = torch.ones((2, H, W), dtype=torch.bool)
            got = fill_disparity(disp.to(DEV), every.to(DEV), median=m)
            assert torch.equal(got.disp.cpu(), median_disparity_torch(disp, m)), (H, W)       # nothing to fill: the median alone
            assert got.counts.cpu().tolist() == [[H * W, 0, 0, 0, 0, 0]] * 2
            keep = torch.rand((2, H, W), generator=g) < 0.3
            plant(disp, keep, g)
            assert same(fill_disparity(disp.to(DEV), keep.to(DEV), median=m, fill_value=1.0),
                        fill_disparity_torch(disp, keep, median=m, fill_value=1.0)), (H, W)
    flat = torch.full((2, 9, 65), 3.25, device=DEV)
    assert torch.equal(fill_disparity(flat, torch.ones_like(flat), median=m).disp, flat)      # a constant map comes back as it is


def _network(ra, g6, g13):
    """The network of test_occlusion_step.py: g13's genotype rows and maxdisp, g6's weights, evaluation mode, no gradients."""
    rows = g13["rows"]
    net = ra.Network(ra.Genotype(rows, None, rows, None), DEV, maxdisp=int(g13["maxdisp"]))
    net.load_state_dict(split_sd(g6), strict=True)
    net = net.to(DEV).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net


@pytest.mark.gpu
def test_forward_dense_is_forward_lr_then_fill_per_view():
    import rag_amd as ra
    ra.load_library()
    g6, g = load_golden("g6_train_step"), load_golden("g13_selfsup_train_step")
    left, right = torch.as_tensor(g["left"]).to(DEV), torch.as_tensor(g["right"]).to(DEV)
    net = _network(ra, g6, g)
    kw = dict(abs_tol=1.0, rel_tol=0.05, occluded_weight=0.25)
    disp_l, disp_r, chk_l, chk_r = net.forward_lr(left, right, 0, net.arch_init, **kw)
    print(f"FORWARD_DENSE kept share left={chk_l.valid.tolist()} right={chk_r.valid.tolist()}")
    serve = ra.checkpoint.MultiTaskStereo(net, [net.arch_init])
    for median in (0, 3):
        dense_l, dense_r, got_l, got_r = net.forward_dense(left, right, 0, net.arch_init, median=median, fill_value=1.0, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got_l.weight, chk_l.weight) and torch.equal(got_r.weight, chk_r.weight)
        assert torch.equal(got_l.error, chk_l.error) and torch.equal(got_r.valid, chk_r.valid)
        for dense, disp, chk in ((dense_l, disp_l, chk_l), (dense_r, disp_r, chk_r)):
            assert isinstance(dense, ra.FilledDisp) and dense.disp.shape == disp.shape
            assert same(dense, ra.fill_disparity(disp, chk, median=median, fill_value=1.0))
            assert same(dense, ra.fill_disparity_torch(disp, chk, median=median, fill_value=1.0))
            assert bool(torch.isfinite(dense.disp).all())
            assert torch.equal(dense.density, chk.valid)                                    # finite disparities: kept = consistent
            if median == 0:
                assert torch.equal(dense.disp[chk.mask], disp[chk.mask])
        again = serve.forward_dense(left, right, 0, median=median, fill_value=1.0, **kw)
        assert same(again[0], dense_l) and same(again[1], dense_r) and torch.equal(again[3].weight, chk_r.weight)
    with pytest.raises(RuntimeError, match="inference only"):
        net.forward_dense(left.clone().requires_grad_(True), right, 0, net.arch_init)
    with pytest.raises(ValueError, match="median"):
        net.forward_dense(left, right, 0, net.arch_init, median=4)
