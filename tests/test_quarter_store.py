"""Quarter store (round 6): cell 2's level-3 main output is read by ONE consumer, cell 4's pre_preprocess behind a x0.25 trilinear
align_corners=True resample, which touches two source indices per output and axis, both inside the aligned group [4X, 4X + 3].  The
producing launch (conv3d_x3q_kernel, RAGMI_STORE_QUARTER_ROWS) skips the main store of every plane and row that is no output's source.

What is checked: the pair property itself and the library's tables against a Python twin of lin_index (CPU); the plan (CPU); on the GPU
that the launch really leaves the other (plane, row)s unwritten, writes the rest bit for bit as the full store does, and that cell 4's
s0|s1 buffer and the disparity map keep their bits.  Shapes: the smallest level-3 volumes the host predicates still send to the dual
launch with down-sampling tails (2^18 voxels per sample: ragmi_conv3d_k3_uses_x3), so each case is a forward of a millisecond or two."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import matching_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
f32 = np.float32


@pytest.fixture(scope="module")
def ra():
    import rag_amd
    if not os.path.exists(rag_amd.lib_path()):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    rag_amd.load_library()
    return rag_amd


@pytest.fixture
def switches(ra):
    """every executor switch at its default, f16x3 precision; restored afterwards"""
    ops = ra.ops
    old = ops.set_conv_precision("f16x3")
    ops.set_quarter_store(True)
    yield ops
    ops.set_conv_precision(old)
    ops.set_quarter_store(True)
    ops.set_g4(True)


def lin_twin(X, n_in, n_out):
    """csrc/common.h lin_index(X, n_in, n_out, lin_scale(n_in, n_out, 1), align_corners=1) in numpy fp32: (i0, i1, w0, w1)"""
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    src = f32(scale * f32(X))
    i0 = min(int(src), n_in - 1)
    lam = min(max(f32(src - f32(i0)), f32(0)), f32(1))
    return i0, i0 + (1 if i0 < n_in - 1 else 0), f32(f32(1) - lam), f32(lam)


def twin_rows(n_in):
    used = [False] * n_in
    for X in range(n_in // 4):
        i0, i1, _w0, _w1 = lin_twin(X, n_in, n_in // 4)
        used[i0] = used[i1] = True
    return used


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_pairs_stay_inside_their_aligned_group():
    """n_in = 4 n_out, align_corners=True: every source pair lies in [4X, 4X + 3], off = i0 - 4X is 0, 1 or 2 below the last output and
    the last output sits on the clamped last voxel; at most two of every four source indices are read."""
    for n_out in range(2, 301):
        n_in = 4 * n_out
        for X in range(n_out):
            i0, i1, w0, w1 = lin_twin(X, n_in, n_out)
            assert 4 * X <= i0 <= i1 <= 4 * X + 3, (n_out, X, i0, i1)
            if X < n_out - 1:
                assert i0 - 4 * X <= 2 and i1 == i0 + 1, (n_out, X, i0, i1)
        i0, i1, w0, w1 = lin_twin(n_out - 1, n_in, n_out)
        assert i1 == n_in - 1 and (i0 == n_in - 1 or w1 > 0.5), (n_out, i0, i1, w0, w1)      # the clamped last voxel carries the output
        used = twin_rows(n_in)
        assert all(sum(used[4 * X:4 * X + 4]) in (1, 2) for X in range(n_out)), n_out


def test_twin_matches_interpolate_on_a_ramp():
    """the twin is ATen's arithmetic: on a ramp (neighbouring sources differ by 1, so a wrong index shows as an error of ~1) the
    interpolated values agree bit for bit (lerp2: the second product rounded, the first fused into the sum — exact in float64 here)"""
    for n_out in range(2, 301):
        n_in = 4 * n_out
        ramp = torch.arange(n_in, dtype=torch.float32)
        ref = F.interpolate(ramp.view(1, 1, -1), size=n_out, mode="linear", align_corners=True).view(-1).numpy()
        got = np.empty(n_out, dtype=f32)
        for X in range(n_out):
            i0, i1, w0, w1 = lin_twin(X, n_in, n_out)
            got[X] = f32(float(w0) * float(i0) + float(f32(w1 * f32(i1))))
        assert np.array_equal(got, ref), n_out


def test_library_tables_equal_the_twin(ra):
    """the (plane, row) set the launch writes — built on the host from the resample kernel's own lin_index — is the twin's"""
    for n_out in range(2, 301):
        assert ra.ops.quarter_store_rows(4 * n_out) == twin_rows(4 * n_out), n_out
    for n_in in (0, 4, 6, 10, 33):
        assert ra.ops.quarter_store_rows(n_in) is None, n_in


def _chain_plan(ra, fea_shape, maxdisp, dtype=torch.float32):
    from rag_amd.modules import _plan_chain
    rows = O.ALL_CONV
    net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=maxdisp).eval()
    cells = [c[0] for c in net.cells_3d]
    B, C, h, w = fea_shape
    return _plan_chain(net.stem3d0[0], net.stem3d1[0], cells, B, C, (maxdisp // 3, h, w), dtype, True)


def test_plan_marks_cell_2_only(ra, switches):
    ops = switches
    headline = ((1, 12, 128, 416), 192)
    plan = _chain_plan(ra, *headline)
    assert [cp.quarter for cp in plan.cells] == [False, False, True] + [False] * 5, plan
    assert plan.stored[2] and plan.consumers[2] == ((3, 1, True),)      # T[2] stays a stored tensor; cell 3 rides as down-sampling tails
    assert tuple(4 * v for v in plan.sizes[4]) == tuple(plan.sizes[2]) == (64, 128, 416)
    assert ops.quarter_store_supported(8, 12, 1, 64, 128, 416, ndown=2)
    ops.set_quarter_store(False)
    assert not any(cp.quarter for cp in _chain_plan(ra, *headline).cells)
    ops.set_quarter_store(True)
    assert not any(cp.quarter for cp in _chain_plan(ra, *headline, dtype=torch.bfloat16).cells)
    with ops.conv_precision("fp32"):
        assert not any(cp.quarter for cp in _chain_plan(ra, *headline).cells)
    assert not any(cp.quarter for cp in _chain_plan(ra, (1, 12, 128, 416), 186).cells)      # D = 62: no multiple of 4
    assert not ops.quarter_store_supported(8, 12, 1, 62, 128, 416, ndown=2)
    assert not ops.quarter_store_supported(8, 12, 1, 64, 128, 416, ndown=0)                # no down-sampling tails: another instantiation
    assert not ops.quarter_store_supported(8, 12, 1, 64, 128, 416, ntail=1, ndown=2)
    assert not ops.quarter_store_supported(8, 12, 1, 64, 126, 416, ndown=2)
    assert not ops.quarter_store_supported(8, 12, 1, 16, 32, 64, ndown=2)                  # too small for the z-marching kernel


# ------------------------------------------------------------------------------------------------------------------ GPU
def _net(ra, maxdisp):
    rows = O.ALL_CONV
    net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=maxdisp)
    net.load_state_dict(O.random_matching_state_dict(rows, seed=0), strict=True)
    return net.to(DEV).eval()


def _forward_captured(ra, monkeypatch, net, lf, rf, vol):
    """one forward; returns (disparity, T[2] as cell 2's dual launch left it, cell 4's s0|s1 buffer, the launch's quarter flag).  The
    main output of a quarter launch is filled with NaN first, so what the launch does not write is still NaN afterwards."""
    ops = ra.ops
    real_dual, real_pair = ops.conv3d_k3_dual, ops.conv3d_k1_resample_pair
    seen = {"level3": [], "pair": []}

    def dual(x, *args, **kw):
        out = args[9]
        if tuple(x.shape[2:]) == tuple(vol):
            if kw.get("quarter"):
                out.fill_(float("nan"))
            seen["level3"].append((out, bool(kw.get("quarter")), bool(kw.get("store_main", True))))
        return real_dual(x, *args, **kw)

    def pair(specs, size, out):
        seen["pair"].append((tuple(size), tuple(specs[0][0].shape[2:]), out))
        return real_pair(specs, size, out)

    monkeypatch.setattr(ops, "conv3d_k3_dual", dual)
    monkeypatch.setattr(ops, "conv3d_k1_resample_pair", pair)
    with torch.no_grad():
        disp = net(lf, rf)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "conv3d_k3_dual", real_dual)
    monkeypatch.setattr(ops, "conv3d_k1_resample_pair", real_pair)
    assert len(seen["level3"]) == 3, "cells 0, 1, 2 are one dual launch each"
    t2, quarter, stored = seen["level3"][2]
    assert stored and not any(q for (_o, q, _s) in seen["level3"][:2])
    quarter_size = tuple(v // 4 for v in vol)
    pre4 = [o for (size, src, o) in seen["pair"] if size == quarter_size and src == tuple(vol)]      # (T[2] x0.25 | T[3] x0.5)
    assert len(pre4) == 1, "cell 4's paired resample launch"
    return disp, t2, pre4[0], quarter


# (B, level-3 volume D x H x W).  All: W / 4 >= 16, so the x offset inside a group reaches 2, and the last output of every axis sits on
# the clamped last voxel.  D = 32 is cut into four depth segments whose items are split into halves of 4 planes; 16 x 128 x 384 runs two
# segments of whole items (no half items) over 12 column tiles; H = 68: H / 4 = 17 is odd and the last row tile hangs over the volume.
CASES = [(2, (32, 64, 128)), (1, (32, 68, 128)), (1, (16, 128, 384))]


@pytest.mark.gpu
@pytest.mark.parametrize("B,vol", CASES)
def test_quarter_store_keeps_every_bit(ra, switches, monkeypatch, B, vol):
    ops = switches
    D, H, W = vol
    assert ops.conv3d_k3_uses_x3(8, 12, B, D, H, W, nset=2, ntail=1) and ops.down2_tail_supported(D, H, W)
    assert ops.quarter_store_supported(8, 12, B, D, H, W, ndown=2)
    net = _net(ra, 3 * D)
    g = torch.Generator().manual_seed(611)
    lf, rf = torch.randn((B, 12, H, W), generator=g).to(DEV), torch.randn((B, 12, H, W), generator=g).to(DEV)
    ops.set_quarter_store(False)
    d_off, t_off, p_off, q_off = _forward_captured(ra, monkeypatch, net, lf, rf, vol)
    assert not q_off and not net.last_g4_plan["quarter"][2]
    ops.set_quarter_store(True)
    d_on, t_on, p_on, q_on = _forward_captured(ra, monkeypatch, net, lf, rf, vol)
    assert q_on and net.last_g4_plan["quarter"] == {j: j == 2 for j in range(8)}, "the quarter path was not taken"
    zs = torch.tensor(twin_rows(D), device=DEV)
    ys = torch.tensor(twin_rows(H), device=DEV)
    written = (zs[:, None] & ys[None, :])[None, None, :, :, None].expand_as(t_on)
    # the launch wrote exactly the (plane, row)s the resample reads — the same bits as the full store — and nothing else
    assert torch.isnan(t_on[~written]).all()
    assert not torch.isnan(t_off).any()
    assert torch.equal(t_on[written], t_off[written])
    assert int(written[0, 0, :, :, 0].sum()) * 4 <= D * H + 2 * (D + H)      # about a quarter of the planes x rows
    # cell 4's s0|s1 buffer and the disparity map
    assert torch.equal(p_on, p_off)
    assert torch.equal(d_on, d_off)
    assert torch.isfinite(d_on).all()


@pytest.mark.gpu
def test_quarter_store_run_to_run_bits(ra, switches):
    B, (D, H, W) = CASES[0]
    net = _net(ra, 3 * D)
    g = torch.Generator().manual_seed(612)
    lf, rf = torch.randn((B, 12, H, W), generator=g).to(DEV), torch.randn((B, 12, H, W), generator=g).to(DEV)
    with torch.no_grad():
        outs = [net(lf, rf) for _ in range(4)]
    assert net.last_g4_plan["quarter"][2]
    assert all(torch.equal(o, outs[0]) for o in outs[1:])


@pytest.mark.gpu
def test_quarter_store_on_channel_planes_input(ra, switches, monkeypatch):
    """G4 off: cell 2 reads channel planes (the other instantiation of the quarter launch)"""
    ops = switches
    B, vol = 1, CASES[0][1]
    D, H, W = vol
    net = _net(ra, 3 * D)
    g = torch.Generator().manual_seed(613)
    lf, rf = torch.randn((B, 12, H, W), generator=g).to(DEV), torch.randn((B, 12, H, W), generator=g).to(DEV)
    ops.set_g4(False)
    ops.set_quarter_store(False)
    d_off, _t, p_off, q_off = _forward_captured(ra, monkeypatch, net, lf, rf, vol)
    ops.set_quarter_store(True)
    d_on, _t, p_on, q_on = _forward_captured(ra, monkeypatch, net, lf, rf, vol)
    assert q_on and not q_off and not net.last_g4_plan["pre"][2]
    assert torch.equal(p_on, p_off) and torch.equal(d_on, d_off)


@pytest.mark.gpu
def test_unsupported_depth_takes_the_full_store(ra, switches, monkeypatch):
    """D % 4 == 2: the plan keeps the full store, same output with the switch on or off"""
    ops = switches
    B, vol = 1, (34, 64, 128)
    D, H, W = vol
    assert ops.conv3d_k3_uses_x3(8, 12, B, D, H, W, nset=2, ntail=1) and not ops.quarter_store_supported(8, 12, B, D, H, W, ndown=2)
    net = _net(ra, 3 * D)
    g = torch.Generator().manual_seed(614)
    lf, rf = torch.randn((B, 12, H, W), generator=g).to(DEV), torch.randn((B, 12, H, W), generator=g).to(DEV)
    outs = []
    for on in (False, True):
        ops.set_quarter_store(on)
        with torch.no_grad():
            outs.append(net(lf, rf))
        assert not any(net.last_g4_plan["quarter"].values())
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()


@pytest.mark.gpu
def test_quarter_flag_is_refused_where_the_launch_does_not_take_it(ra, switches):
    """asked of a call that lands elsewhere the flag is an error (RAGMI_EUNSUPPORTED), never a silently full or silently partial store"""
    ops = switches
    x = torch.randn((1, 8, 8, 16, 32), generator=torch.Generator().manual_seed(615)).to(DEV)
    w = torch.randn((12, 4, 3, 3, 3), generator=torch.Generator().manual_seed(616)).to(DEV) * 0.1
    pk = ops.conv3d_k3_pack(w)
    out = torch.zeros((1, 12, 8, 16, 32), device=DEV)
    with pytest.raises(RuntimeError):
        ops.conv3d_k3_dual(x, 4, pk, None, None, pk, None, None, 12, True, out, quarter=True)
    torch.cuda.synchronize()
    assert not out.any()
