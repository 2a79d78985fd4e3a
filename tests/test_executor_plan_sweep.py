"""The fused inference executor — MatchingNet._run_chain and _head, driven by _plan_chain, _plan_head, _plan_head_taps and
_plan_head_xblend — end to end against the fp64 oracle, on the folded path (net(lf, rf) / matching(None, ..., features=...)) and at the
shapes where the plan and the library's routes change.  The kernels have their own sweeps; this file checks what strings them together.

1. signature(genotype, B, (d, h, w), storage): every field of the chain plan's cells plus consumers / stored / stem0_g4 / stems_fused /
   stem_tail_rows; the head plan with taps and xblend; for stem3d1 and every Dual / Conv step of every cell the route of
   ops.conv3d_k3_route with (nseg, nsplit > 0), asked with the cin / cout / nset / ntail / ndown _plan_chain hands to caps(); last_3_3d's
   ops.conv3d_k3_small_route where the head runs it; and ops.conv3d_k1_plan / conv3d_k1_resample_plan / trilinear3d_route for the 1x1x1
   and resample launches the plan runs.  Computed without a GPU; no probe was added to the library.  (ops.cell2d has no place in it: the
   Matching Net never meets its condition on the grid — see the defect below.)
2. TABLE, chosen by enumeration over GRID_D x GRID_H x GRID_W x B in {1, 2} x four genotypes x three storage / precision settings.
   Three kinds of class must each have a row (test_table_covers_every_class_of_the_grid):
   - the chain class: storage, every plan boolean, the head plan, and per 3x3x3 launch the route name with nsplit zero or not;
   - the head class: storage, head plan, last_3_3d's small route (None, 0 = conv3d_c1, 2 / 3 = the VALU form's tile configuration) and
     the trilinear routes of the head's resamples;
   - every kind of 1x1x1 / resample launch in front of a cell (k1, k1r, pair, multi, tri + its trilinear route) per storage and cell.
   The head runs behind the chain on T[7] alone and each 1x1x1 launch's instantiation depends on its own arguments only, so these are
   covered one by one and not as a product with the chain class (the product has 249 classes, 129 more rows under the voxel cap).
   The exact nseg is outside the class: the grid reaches nseg {1, 2, 3, 4} and so does the table (NSEG_GRID, NSEG_TABLE, asserted).
   The full signature (nseg and slab widths included) is what each row's digest pins.  Rows are capped at 2^19 voxels per call; two
   exceed it (BIG_ROWS: cells 3..7 all on Box needs 32x128x256; a finer search found nothing smaller); ten more chain classes of
   the grid exist only above the cap and have no row — they are listed, not silent (UNCOVERED_ABOVE_CAP).
3. test_row_on_gpu, per row: (a) e = max |mat - mat64| / max |mat64| <= K x E(row); (b) EPE of the disparity map <= EPE_GATE, under
   bf16 storage <= max(0.08, 2 x the EPE of the oracle with the plan's bf16 roundings) — a deviation from the one EPE gate: no bf16
   forward meets 1e-3 px, the suite holds bf16 to 0.08 px at reduced sizes, and that oracle alone is at 0.10 px at 17x8x8; (c) the switch matrix
   of tools/fuzz_fused.py: quarter store off = the same bits; tail rows off = inside gate (a); with the tail rows off, G4 off / stem
   fusion off / everything off = the same bits (test_matchingnet_g4_plan_and_bitwise, test_quarter_store.py); (e) a third run
   = the same bits; (d) the forward once more on an allocator whose every free block holds 0xFF bytes: finite and the same bits.
4. E(row) is the oracle's own error for the row, computed in the test on the CPU: E32 = the fp32 oracle against the fp64 one (fp32
   storage), Ebf = the fp32 oracle with the plan's bf16 tensors rounded to bf16 when produced (bf16 storage).  K = the smallest power
   of two >= twice the worst e / E measured on the MI355X, under the caps K32 <= 16, Kx3 <= 128, Kbf <= 8:
   fp32: worst e / E = 1.31 (conv-B1-4x8x8-fp32) -> K = 4
   f16x3: worst e / E = 1.43 (mixed-B1-4x8x33-f16x3) -> K = 4
   bf16: worst e / E = 2.12 (unsorted-B1-4x8x64-bf16) -> K = 8
5. test_planted_defects_exceed_ten_times_the_capped_gate: six wiring / edge defects planted in the oracle move `mat` by >= 10 x cap x E
   on every row up to 2^18 voxels.  Under bf16 storage 10 x 8 x Ebf is 0.07 .. 0.9 of max |mat|, and each of plane / row / col / groups /
   qshift stays below it on some row (INVISIBLE_UNDER_BF16); every one of them passes the fp32-f16x3 threshold (10 x 128 x E32) of the
   same genotype, shape and weights, which the test asserts on those rows.  In the all-skip genotype `groups` (and `plane` at d = 4)
   changes nothing at all: the three new states are the same sum, and depth planes never mix.
   What EPE alone would have let through (EPE of the planted defect <= EPE_GATE = 1e-3 px, printed by the test; CPU, fp32 oracle):
   plane: on 5 rows, e.g. mixed-B1-4x8x8-f16x3, conv-B1-4x8x33-fp32, unsorted-B1-4x8x64-bf16
   row: on 7 rows, e.g. mixed-B1-4x8x8-f16x3, skip-B1-4x8x8-fp32, conv-B1-4x128x256-bf16
   col: on 10 rows, e.g. mixed-B1-4x8x8-f16x3, skip-B1-4x8x33-fp32, conv-B1-4x128x256-bf16
   groups: on 2 rows, e.g. mixed-B1-4x8x8-f16x3, unsorted-B1-4x8x64-bf16
   qshift: on 4 rows, e.g. mixed-B1-4x8x8-f16x3, skip-B1-4x8x8-f16x3, unsorted-B1-4x8x64-bf16
   `batch` was above the EPE gate on every B = 2 row.

The defect this sweep found (fixed in rag_amd/modules.py): on a d = 4 cost volume cell 5 of the all-conv genotype ends at depth 1 and took
the one-launch 2-D cell (ops.cell2d), which resamples in 2-D, although its prev_prev input T[3] has depth 2: the launch read T[3]'s
channel planes at half their stride.  e was 0.35 .. 0.69 of max |mat| at 4x8x32, 4x8x33 and 4x128x256 (EPE 0.04 .. 3 px); the golden
tests never ran a d = 4 volume.  _one_launch_2d now asks for depth-1 inputs and ops.cell2d refuses anything else.

Measured on the MI355X (e, E, e / E per row; EPE of the disparity map in px):
  conv-B1-4x8x8-bf16 1.5e-03 2.1e-03 0.73 2e-03 | mixed-B1-4x8x8-bf16 3.4e-03 3.0e-03 1.12 9e-03
  skip-B1-4x8x8-bf16 7.1e-03 7.1e-03 1.00 2e-03 | conv-B1-4x8x8-f16x3 2.6e-07 5.8e-07 0.45 3e-07
  mixed-B1-4x8x8-f16x3 2.6e-07 3.6e-07 0.73 0e+00 | skip-B1-4x8x8-f16x3 3.0e-07 5.2e-07 0.57 4e-06
  conv-B1-4x8x8-fp32 8.1e-07 6.2e-07 1.31 1e-06 | mixed-B1-4x8x8-fp32 7.4e-07 1.3e-06 0.59 2e-06
  skip-B1-4x8x8-fp32 2.0e-07 2.6e-07 0.78 5e-16 | conv-B1-4x8x32-bf16 1.2e-03 1.8e-03 0.69 1e-05
  mixed-B1-4x8x32-bf16 8.6e-03 6.1e-03 1.41 4e-02 | unsorted-B1-4x8x32-bf16 2.6e-03 3.5e-03 0.74 9e-04
  conv-B1-4x8x32-f16x3 5.6e-07 6.5e-07 0.87 1e-06 | mixed-B1-4x8x32-f16x3 1.3e-06 9.3e-07 1.38 4e-06
  unsorted-B1-4x8x32-f16x3 3.2e-07 5.6e-07 0.56 2e-06 | conv-B1-4x8x33-bf16 5.5e-03 7.7e-03 0.71 1e-02
  mixed-B1-4x8x33-bf16 2.1e-03 2.6e-03 0.79 2e-02 | skip-B1-4x8x33-bf16 8.1e-03 1.1e-02 0.73 6e-04
  unsorted-B1-4x8x33-bf16 2.8e-03 2.9e-03 0.97 2e-02 | conv-B1-4x8x33-f16x3 1.5e-06 1.1e-06 1.41 3e-06
  mixed-B1-4x8x33-f16x3 1.0e-06 7.2e-07 1.43 8e-07 | skip-B1-4x8x33-f16x3 6.8e-07 9.8e-07 0.70 1e-08
  unsorted-B1-4x8x33-f16x3 5.1e-07 4.9e-07 1.05 6e-06 | conv-B1-4x8x33-fp32 4.7e-07 5.7e-07 0.82 2e-07
  mixed-B1-4x8x33-fp32 8.2e-07 8.8e-07 0.93 3e-06 | skip-B1-4x8x33-fp32 5.4e-07 5.8e-07 0.93 2e-06
  conv-B1-17x8x8-bf16 3.7e-03 4.5e-03 0.81 3e-03 | mixed-B1-17x8x8-bf16 2.8e-03 4.1e-03 0.68 9e-02
  conv-B1-17x8x8-f16x3 7.1e-07 8.2e-07 0.88 9e-06 | mixed-B1-17x8x8-f16x3 8.3e-07 9.4e-07 0.88 2e-06
  mixed-B1-4x8x64-bf16 2.7e-03 2.2e-03 1.22 2e-03 | unsorted-B1-4x8x64-bf16 3.8e-03 1.8e-03 2.12 1e-06
  mixed-B1-4x8x64-f16x3 5.9e-07 8.0e-07 0.74 3e-06 | unsorted-B1-4x8x64-f16x3 1.7e-06 2.0e-06 0.85 2e-05
  mixed-B1-4x8x131-bf16 4.3e-03 3.4e-03 1.26 5e-03 | unsorted-B1-4x8x131-bf16 5.7e-03 6.2e-03 0.92 6e-03
  mixed-B1-4x8x131-f16x3 8.2e-07 8.0e-07 1.03 7e-06 | unsorted-B1-4x8x131-f16x3 6.8e-07 5.9e-07 1.14 2e-06
  conv-B1-17x32x228-bf16 1.9e-03 2.4e-03 0.79 2e-02 | mixed-B1-17x32x228-bf16 1.2e-03 1.4e-03 0.90 5e-03
  unsorted-B1-17x32x228-bf16 5.7e-03 4.0e-03 1.45 6e-02 | conv-B1-17x32x228-f16x3 1.2e-05 1.1e-05 1.12 6e-05
  mixed-B1-17x32x228-f16x3 9.0e-06 8.7e-06 1.04 9e-06 | unsorted-B1-17x32x228-f16x3 2.0e-06 1.8e-06 1.09 2e-04
  conv-B1-17x48x160-bf16 2.9e-03 3.7e-03 0.76 2e-02 | mixed-B1-17x48x160-bf16 5.3e-03 4.0e-03 1.31 4e-02
  unsorted-B1-17x48x160-bf16 1.9e-03 1.7e-03 1.15 9e-15 | conv-B1-17x48x160-f16x3 5.3e-06 5.1e-06 1.05 3e-05
  mixed-B1-17x48x160-f16x3 3.7e-06 3.6e-06 1.03 1e-05 | unsorted-B1-17x48x160-f16x3 3.6e-06 3.7e-06 0.97 2e-05
  conv-B1-4x128x256-bf16 1.2e-03 1.7e-03 0.67 7e-06 | conv-B1-8x64x256-bf16 2.8e-03 3.3e-03 0.82 7e-04
  mixed-B1-4x128x256-bf16 1.3e-02 1.0e-02 1.24 2e-02 | mixed-B1-8x64x256-bf16 2.1e-03 2.3e-03 0.93 1e-04
  unsorted-B1-4x128x256-bf16 5.5e-03 4.6e-03 1.21 1e-03 | unsorted-B1-8x64x256-bf16 1.5e-03 8.9e-04 1.62 3e-03
  conv-B1-4x128x256-f16x3 4.7e-06 4.7e-06 0.99 2e-06 | conv-B1-8x64x256-f16x3 5.2e-06 5.1e-06 1.03 3e-05
  mixed-B1-4x128x256-f16x3 3.1e-06 3.2e-06 0.98 3e-07 | mixed-B1-8x64x256-f16x3 5.4e-06 6.1e-06 0.90 5e-05
  unsorted-B1-4x128x256-f16x3 2.7e-06 2.7e-06 1.01 2e-05 | unsorted-B1-8x64x256-f16x3 1.7e-06 1.7e-06 1.01 1e-06
  conv-B1-8x100x164-bf16 2.9e-03 4.2e-03 0.68 7e-04 | mixed-B1-8x100x164-bf16 7.3e-03 5.4e-03 1.34 4e-03
  unsorted-B1-8x100x164-bf16 1.2e-03 9.5e-04 1.27 2e-03 | conv-B1-8x100x164-f16x3 6.4e-06 6.2e-06 1.02 7e-07
  mixed-B1-8x100x164-f16x3 6.6e-06 7.0e-06 0.94 4e-06 | unsorted-B1-8x100x164-f16x3 4.7e-06 5.0e-06 0.95 1e-05
  conv-B1-8x128x256-bf16 4.0e-03 6.6e-03 0.60 2e-02 | mixed-B1-8x128x256-bf16 3.3e-03 2.7e-03 1.21 2e-04
  skip-B1-8x128x256-bf16 3.4e-03 4.0e-03 0.85 4e-04 | unsorted-B1-8x128x256-bf16 6.5e-03 3.4e-03 1.88 2e-02
  conv-B1-8x128x256-f16x3 8.1e-06 8.3e-06 0.97 9e-07 | mixed-B1-8x128x256-f16x3 5.7e-06 6.2e-06 0.93 5e-07
  skip-B1-8x128x256-f16x3 1.4e-05 1.4e-05 1.00 9e-06 | unsorted-B1-8x128x256-f16x3 3.4e-06 3.8e-06 0.92 3e-05
  conv-B1-16x100x164-bf16 5.9e-03 7.5e-03 0.79 3e-02 | mixed-B1-16x100x164-bf16 2.8e-03 3.1e-03 0.90 2e-04
  skip-B1-16x100x164-bf16 2.8e-03 2.4e-03 1.18 1e-03 | unsorted-B1-16x100x164-bf16 3.9e-03 3.8e-03 1.02 1e-03
  conv-B1-16x100x164-f16x3 8.4e-06 8.8e-06 0.95 1e-05 | mixed-B1-16x100x164-f16x3 2.2e-06 2.3e-06 0.96 6e-06
  skip-B1-16x100x164-f16x3 1.1e-05 1.1e-05 0.99 9e-05 | unsorted-B1-16x100x164-f16x3 5.2e-06 5.1e-06 1.02 3e-05
  conv-B1-12x96x228-bf16 2.0e-03 3.5e-03 0.57 4e-04 | conv-B1-12x96x228-f16x3 6.5e-06 6.5e-06 0.99 2e-05
  conv-B1-17x84x184-bf16 9.8e-03 1.2e-02 0.83 3e-02 | conv-B1-17x92x168-bf16 1.7e-03 2.1e-03 0.78 4e-02
  mixed-B1-17x84x184-bf16 2.1e-03 2.1e-03 0.98 5e-04 | mixed-B1-17x92x168-bf16 6.0e-03 6.2e-03 0.96 1e-02
  skip-B1-17x84x184-bf16 7.9e-03 8.3e-03 0.95 3e-03 | skip-B1-17x92x168-bf16 5.4e-03 5.0e-03 1.08 7e-02
  unsorted-B1-17x84x184-bf16 2.5e-03 1.8e-03 1.41 7e-04 | unsorted-B1-17x92x168-bf16 3.0e-03 3.4e-03 0.87 9e-04
  conv-B1-17x84x184-f16x3 1.0e-05 1.0e-05 1.04 4e-05 | conv-B1-17x92x168-f16x3 7.4e-06 7.5e-06 0.97 3e-05
  mixed-B1-17x84x184-f16x3 4.1e-06 4.6e-06 0.90 4e-05 | mixed-B1-17x92x168-f16x3 7.6e-06 7.3e-06 1.04 9e-05
  skip-B1-17x84x184-f16x3 5.0e-06 5.1e-06 0.98 7e-05 | skip-B1-17x92x168-f16x3 5.8e-06 5.9e-06 0.99 3e-06
  unsorted-B1-17x84x184-f16x3 4.0e-06 4.1e-06 0.98 9e-05 | unsorted-B1-17x92x168-f16x3 3.0e-06 2.9e-06 1.03 2e-05
  conv-B1-12x112x196-f16x3 5.1e-06 5.2e-06 0.98 9e-06 | conv-B1-28x48x196-f16x3 2.8e-06 3.0e-06 0.94 6e-06
  conv-B1-32x128x256-bf16 6.8e-03 5.4e-03 1.25 1e-02 | conv-B1-32x128x256-f16x3 5.2e-06 5.1e-06 1.02 4e-05
  conv-B1-17x132x172-f16x3 7.2e-06 7.0e-06 1.03 9e-05 | conv-B1-17x132x172-bf16 3.0e-03 3.8e-03 0.79 6e-02
  conv-B1-8x128x256-fp32 2.4e-06 2.5e-06 0.95 2e-06 | conv-B2-8x128x256-f16x3 6.6e-06 7.0e-06 0.95 1e-05
  mixed-B2-17x20x33-fp32 8.2e-07 9.8e-07 0.84 8e-06 | conv-B1-16x128x131-f16x3 6.5e-06 6.7e-06 0.96 2e-05
  conv-B1-16x128x131-bf16 2.2e-03 3.2e-03 0.71 1e-02 | conv-B2-17x20x33-f16x3 9.4e-07 1.2e-06 0.75 1e-05
  mixed-B2-12x32x33-bf16 2.9e-03 2.7e-03 1.05 4e-03
  conv-B1-4x8x131-fp32 5.9e-07 7.1e-07 0.84 4e-06 | conv-B1-17x32x256-bf16 9.9e-04 1.1e-03 0.87 2e-03
  conv-B1-17x32x256-f16x3 1.0e-05 1.0e-05 1.02 2e-05 | conv-B1-17x32x256-fp32 7.7e-06 8.0e-06 0.96 7e-05
  conv-B1-17x64x256-fp32 8.1e-06 8.1e-06 1.00 4e-05
"""
import collections
import contextlib
import hashlib
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import matching_oracle as O
from test_hip_parity import EPE_GATE, gen, gpu, ra  # noqa: F401  (ra: fixture)
from test_host_cpu import MIXED_ROWS, UNSORTED_ROWS, built_lib  # noqa: F401  (built_lib: fixture)

f32, bf16, f64 = torch.float32, torch.bfloat16, torch.float64
GENOTYPES = {"conv": O.ALL_CONV, "skip": O.ALL_SKIP, "mixed": MIXED_ROWS, "unsorted": UNSORTED_ROWS}
STORAGES = {"fp32": (f32, "fp32"), "f16x3": (f32, "f16x3"), "bf16": (bf16, "f16x3")}      # name -> (storage type, conv precision)
C_FEA = 12


# ---------------------------------------------------------------------------------------------------------------- 1. the signature
@contextlib.contextmanager
def defaults(ops, precision="f16x3"):
    """every executor switch at its default under `precision`; put back afterwards"""
    old = (ops.g4_enabled(), ops.stem_fusion_enabled(), ops.stem_tail_rows_enabled(), ops.quarter_store_enabled(),
           ops.bf16_deep_fp32_enabled(), ops.bf16_head_fp32_enabled(), ops.chain_k1_enabled(), ops.head_taps_enabled(),
           ops.head_xblend_enabled())
    setters = (ops.set_g4, ops.set_stem_fusion, ops.set_stem_tail_rows, ops.set_quarter_store, ops.set_bf16_deep_fp32,
               ops.set_bf16_head_fp32, ops.set_chain_k1, ops.set_head_taps, ops.set_head_xblend)
    try:
        for s in setters:
            s(True)
        with ops.conv_precision(precision):
            yield
    finally:
        for s, v in zip(setters, old):
            s(v)


_NETS = {}


def _cpu_net(gname):
    """one CPU MatchingNet per genotype, for planning only (maxdisp is not read by the planners)"""
    import rag_amd
    if gname not in _NETS:
        rows = GENOTYPES[gname]
        _NETS[gname] = rag_amd.MatchingNet(rag_amd.Genotype(rows, None, rows, None), maxdisp=48).eval()
    return _NETS[gname]


def _vol(s):
    return int(s[0]) * int(s[1]) * int(s[2])


def _convbr_launch(ops, cin, cout, B, in_size, in_dt, out_size, out_dt, y_channels):
    """What ConvBR_3d.forward(x, out=buffer, resample_to=out_size) launches for a 1x1x1 unit, as probe answers."""
    mixed = in_dt != out_dt
    if not mixed and tuple(in_size) == tuple(out_size):
        return ("k1",) + ops.conv3d_k1_plan(B, cin, cout, _vol(in_size), y_bstride=y_channels * _vol(out_size), dtype=in_dt)
    if not mixed and _vol(out_size) > _vol(in_size) and cout <= cin:
        return (("k1",) + ops.conv3d_k1_plan(B, cin, cout, _vol(in_size), dtype=in_dt),
                ("tri", ops.trilinear3d_route(in_size, out_size, cout, True)))
    return ("k1r", ops.conv3d_k1_resample_plan([cin], [cout], [in_size], B, out_size, in_dt))


def plans(gname, B, vol, storage):
    """(cells, chain plan, head plan, taps, xblend) of the folded forward at the switches in force"""
    from rag_amd.modules import _plan_chain, _plan_head, _plan_head_taps, _plan_head_xblend
    adt = STORAGES[storage][0]
    net = _cpu_net(gname)
    cells = [c[0] for c in net.cells_3d]
    plan = _plan_chain(net.stem3d0[0], net.stem3d1[0], cells, B, C_FEA, tuple(vol), adt, True)
    n = len(cells)
    m3, m6, m12 = net.last_3_3d[0], net.last_6_3d[0], net.last_12_3d[0]
    hp = _plan_head(vol, plan.sizes[n - 1], plan.cdt[n - 1], m3, m6, m12, False)
    taps = bool(_plan_head_taps(hp, vol, plan.sizes[n - 1], plan.cdt[n - 1], m3, m6))
    xb = bool(_plan_head_xblend(hp, vol, plan.sizes[n - 1], plan.cdt[n - 1], m3, m6))
    return net, cells, plan, hp, taps, xb


def signature_parts(gname, B, vol, storage):
    """(plan part, head part, 3x3x3 routes, 1x1x1 / resample probes) for one case; call under defaults(ops, precision).
    Every size, channel count and storage type is read from the plan itself; the tail counts are those _plan_chain hands to caps().
    This is a MODEL of the executor: which launches run is decided again here, mirroring MatchingNet._run_chain (shared_pre, the plain
    launches behind a cell without tails), _Cell._run (pair / grows / s0 / s1), _Cell._schedule, ConvBR_3d.forward (_convbr_launch) and
    MatchingNet._head / _head_quarter.  A change to one of those that leaves the plan and the probes alone must be repeated here."""
    from rag_amd import ops
    from rag_amd.modules import Conv, Dual
    vol = tuple(int(v) for v in vol)
    net, cells, plan, hp, taps, xb = plans(gname, B, vol, storage)
    n = len(cells)
    sizes, cdt, cons = plan.sizes, plan.cdt, plan.consumers
    cout = {-2: net.stem3d0[0].conv.out_channels, -1: net.stem3d1[0].conv.out_channels}
    for i, c in enumerate(cells):
        cout[i] = c.block_multiplier * c.C_out
    nfull = {i: sum(not d for (_j, _r, d) in cons[i]) for i in cons}
    ndown = {i: sum((cells[j].C_out + 3) // 4 for (j, _r, d) in cons[i] if d) for i in cons}
    dts = {f32: "f32", bf16: "bf16"}

    p_plan = (tuple((cp.g4, cp.dual, cp.store_main, cp.tails, cp.shared_pre, cp.quarter, tuple(cp.has), dts[cp.dtype]) for cp in plan.cells),
              tuple(cons[i] for i in range(-2, n)), tuple(bool(plan.stored[i]) for i in range(-2, n)),
              bool(plan.stem0_g4), bool(plan.stems_fused), bool(plan.stem_tail_rows))
    p_head = (tuple(hp), taps, xb)

    # 3x3x3 launches: stem3d1 (the second kernel of the fused stems runs on the same routes) and every Dual / Conv step of every cell
    k3 = [("stem1", ops.conv3d_k3_route(cout[-2], cout[-1], B, *vol, nset=1, ntail=nfull[-1], dtype=cdt[-1]))]
    k1 = []
    for i, (c, cp) in enumerate(zip(cells, plan.cells)):
        C = c.C_out
        s0_in_pre = cp.has[0] or cout[i - 2] != C
        for step in c._schedule(s0_in_pre):
            if isinstance(step, Dual):
                nt, nd = (nfull[i], ndown[i]) if cp.tails else (0, 0)
                k3.append((i, "dual", ops.conv3d_k3_route(2 * C, C * len(step.dst_states), B, *sizes[i], nset=2, ntail=nt, ndown=nd, dtype=cdt[i])))
            elif isinstance(step, Conv):
                k3.append((i, "conv", ops.conv3d_k3_route(C, C * len(step.mods), B, *sizes[i], nset=1, has_res=step.res_states is not None,
                                                          dtype=cdt[i])))
        # the 1x1x1 / resample launches in front of the cell (MatchingNet._run_chain, _Cell._run)
        if cp.shared_pre:
            cj = cells[i + 1]
            k1.append((i, "multi", ops.conv3d_k1_resample_plan([cout[i - 2], cout[i - 1], cout[i - 1]], [C, C, cj.C_out],
                                                               [sizes[i - 2], sizes[i - 1], sizes[i - 1]], B, sizes[i], cdt[i])))
        has = cp.has
        grows = any(plan.stored[k] and _vol(sizes[i]) > _vol(sizes[k]) and C <= cout[k] for k in (i - 2, i - 1))
        if not has[0] and not has[1] and cout[i - 2] != C and not grows and cdt[i - 2] == cdt[i - 1] == cdt[i]:
            k1.append((i, "pair", ops.conv3d_k1_resample_plan([cout[i - 2], cout[i - 1]], [C, C], [sizes[i - 2], sizes[i - 1]], B, sizes[i], cdt[i])))
        else:
            if s0_in_pre and not has[0]:
                k1.append((i, "s0", _convbr_launch(ops, cout[i - 2], C, B, sizes[i - 2], cdt[i - 2], sizes[i], cdt[i], 2 * C)))
            elif not s0_in_pre and sizes[i - 2] != sizes[i]:
                k1.append((i, "s0", ("tri", ops.trilinear3d_route(sizes[i - 2], sizes[i], cout[i - 2], True))))
            if not has[1]:
                k1.append((i, "s1", _convbr_launch(ops, cout[i - 1], C, B, sizes[i - 1], cdt[i - 1], sizes[i], cdt[i], 2 * C)))
        if not cp.tails:      # the would-be tails of a producer that is not one dual launch: plain launches behind it
            for (j, role, down) in cons[i]:
                k1.append((i, "after", j, role, _convbr_launch(ops, cout[i], cells[j].C_out, B, sizes[i], cdt[i], sizes[j], cdt[j], 2 * cells[j].C_out)))
    # the head
    last, ldt = sizes[n - 1], cdt[n - 1]
    d, h, w = vol
    half = (max(d // 2, 1), h // 2, w // 2)
    small = None
    if hp.level == 4:
        if hp.chain:
            if not taps:
                k1.append(("head", "tri12", ops.trilinear3d_route(last, half, 12, True)))
        else:
            k1.append(("head", "m12", _convbr_launch(ops, 48, 24, B, last, ldt, last, f32 if hp.cross_f32 else ldt, 24)))
            k1.append(("head", "m6", _convbr_launch(ops, 24, 12, B, last, f32 if hp.cross_f32 else ldt, half, f32 if hp.cross_f32 else ldt, 12)))
    if not taps and not hp.upconv:
        ydt = f32 if (hp.cross_f32 or ldt == f32) else bf16
        k1.append(("head", "tri6", ops.trilinear3d_route(half, vol, 12, True)))
        small = ops.conv3d_k3_small_route(12, 1, B, d, h, w, ydt, f32)
    return p_plan, p_head, tuple(k3), small, tuple(k1)


def signature(rows_name, B, vol, storage, precision=None):
    """The hashable signature of one case: plan fields, head plan, 3x3x3 route + schedule class (nseg, nsplit > 0) + last_3_3d's small
    route, and the 1x1x1 / resample probes.  `precision` defaults to the storage's own."""
    from rag_amd import ops
    with defaults(ops, precision or STORAGES[storage][1]):
        p_plan, p_head, k3, small, k1 = signature_parts(rows_name, B, vol, storage)
    k3 = tuple(e[:-1] + ((e[-1][0], e[-1][1][1], e[-1][1][2] > 0),) for e in k3)
    return (storage, p_plan, p_head, k3, small, k1)


def sig_class(sig):
    """The chain class: storage, plan booleans, head plan, the 3x3x3 route names with nsplit zero or not (the exact nseg left out)."""
    storage, p_plan, p_head, k3, small, k1 = sig
    k3c = tuple(e[:-1] + ((e[-1][0], e[-1][2]),) for e in k3)
    return (storage, p_plan, p_head, k3c)


def _names(x):
    """the strings of a nested probe answer: launch kinds and route names (slab widths and the vector flag left out — the table of
    test_pointwise_resample_sweep.py covers those)"""
    return tuple(_names(v) for v in x if isinstance(v, (str, tuple))) if isinstance(x, tuple) else x


def head_class(sig):
    """storage, head plan, last_3_3d's small route and the kinds / trilinear routes of the head's own launches"""
    storage, p_plan, p_head, k3, small, k1 = sig
    return (storage, p_head, small, tuple(_names(e) for e in k1 if e[0] == "head"))


def k1_kinds(sig):
    """{(storage, cell, where, launch kind and route names)} of the 1x1x1 / resample launches in front of and behind the cells"""
    storage, p_plan, p_head, k3, small, k1 = sig
    return {(storage, e[0], e[1]) + _names(e[2:]) for e in k1 if e[0] != "head"}


def digest(x):
    return hashlib.sha1(repr(x).encode()).hexdigest()[:10]


GRID_D = (4, 8, 12, 16, 17, 20, 24, 32)
GRID_H = (8, 12, 16, 20, 32, 48, 64, 96, 128, 132, 136)
GRID_W = (8, 12, 16, 20, 32, 33, 64, 96, 128, 131, 132, 160, 256)


def enumerate_grid():
    """{signature: (voxels per call, genotype, B, d, h, w, storage)} — the smallest case of every signature over the grid above"""
    best = {}
    for storage in STORAGES:
        for gname, B, d, h, w in itertools.product(GENOTYPES, (1, 2), GRID_D, GRID_H, GRID_W):
            s = signature(gname, B, (d, h, w), storage)
            key = (B * d * h * w, gname, B, d, h, w, storage)
            if s not in best or key < best[s]:
                best[s] = key
    return best


# ------------------------------------------------------------------------------------------------------------- 2. the case table
# One row per class (sig_class) of the grid above: the case with the fewest voxels per call, found over the grid and, for the classes
# that the grid first reaches above 2^17 voxels, over a finer one (d step 4 plus 17, h and w step 4 from 32, plus w 33 and 131).  Then
# the ragged and regime rows of test_table_reaches_every_regime.  (genotype, B, d, h, w, storage, digest of the FULL signature — nseg and slab widths
# included, so a changed host predicate shows here even where the class stays.)  Regenerate: python tests/test_executor_plan_sweep.py
Row = collections.namedtuple("Row", "geno B d h w storage digest")
TABLE = [Row(*r) for r in (
    ("conv", 1, 4, 8, 8, "bf16", "fbc9cec822"),
    ("mixed", 1, 4, 8, 8, "bf16", "4eafac1648"),
    ("skip", 1, 4, 8, 8, "bf16", "43fd2d54b5"),
    ("conv", 1, 4, 8, 8, "f16x3", "39f455e080"),
    ("mixed", 1, 4, 8, 8, "f16x3", "06e415c53a"),
    ("skip", 1, 4, 8, 8, "f16x3", "93d0e1ba40"),
    ("conv", 1, 4, 8, 8, "fp32", "2bf4309c59"),
    ("mixed", 1, 4, 8, 8, "fp32", "3eb36b7372"),
    ("skip", 1, 4, 8, 8, "fp32", "cf04917c9d"),
    ("conv", 1, 4, 8, 32, "bf16", "18e80eeb22"),
    ("mixed", 1, 4, 8, 32, "bf16", "9dd10fd627"),
    ("unsorted", 1, 4, 8, 32, "bf16", "8be866b743"),
    ("conv", 1, 4, 8, 32, "f16x3", "16f01a14a6"),
    ("mixed", 1, 4, 8, 32, "f16x3", "5373f30e7f"),
    ("unsorted", 1, 4, 8, 32, "f16x3", "844c01743b"),
    ("conv", 1, 4, 8, 33, "bf16", "edf355a45e"),
    ("mixed", 1, 4, 8, 33, "bf16", "0876295a9f"),
    ("skip", 1, 4, 8, 33, "bf16", "5cd1a4e6bf"),
    ("unsorted", 1, 4, 8, 33, "bf16", "213c330a2f"),
    ("conv", 1, 4, 8, 33, "f16x3", "dd303beff0"),
    ("mixed", 1, 4, 8, 33, "f16x3", "7912628434"),
    ("skip", 1, 4, 8, 33, "f16x3", "923e297a39"),
    ("unsorted", 1, 4, 8, 33, "f16x3", "5d56a6e373"),
    ("conv", 1, 4, 8, 33, "fp32", "065cffb084"),
    ("mixed", 1, 4, 8, 33, "fp32", "5c2ef3f6b6"),
    ("skip", 1, 4, 8, 33, "fp32", "e2c0f32c44"),
    ("conv", 1, 17, 8, 8, "bf16", "78067a8c8f"),
    ("mixed", 1, 17, 8, 8, "bf16", "774dab0ace"),
    ("conv", 1, 17, 8, 8, "f16x3", "ae9dd7b988"),
    ("mixed", 1, 17, 8, 8, "f16x3", "e333b6985a"),
    ("mixed", 1, 4, 8, 64, "bf16", "6f140abe66"),
    ("unsorted", 1, 4, 8, 64, "bf16", "5791025799"),
    ("mixed", 1, 4, 8, 64, "f16x3", "de33fc4534"),
    ("unsorted", 1, 4, 8, 64, "f16x3", "627b8fb1c8"),
    ("mixed", 1, 4, 8, 131, "bf16", "339a2eff30"),
    ("unsorted", 1, 4, 8, 131, "bf16", "ee00323ca9"),
    ("mixed", 1, 4, 8, 131, "f16x3", "030ad817f0"),
    ("unsorted", 1, 4, 8, 131, "f16x3", "03fd479f95"),
    ("conv", 1, 17, 32, 228, "bf16", "036c01b78b"),
    ("mixed", 1, 17, 32, 228, "bf16", "0263dbd0e5"),
    ("unsorted", 1, 17, 32, 228, "bf16", "456bbea293"),
    ("conv", 1, 17, 32, 228, "f16x3", "101157fc3d"),
    ("mixed", 1, 17, 32, 228, "f16x3", "f8141c73b0"),
    ("unsorted", 1, 17, 32, 228, "f16x3", "bdd5f8bd25"),
    ("conv", 1, 17, 48, 160, "bf16", "fe8e6e7644"),
    ("mixed", 1, 17, 48, 160, "bf16", "9abd626f46"),
    ("unsorted", 1, 17, 48, 160, "bf16", "05f7a8901a"),
    ("conv", 1, 17, 48, 160, "f16x3", "be9199bfc7"),
    ("mixed", 1, 17, 48, 160, "f16x3", "f4be7cdd06"),
    ("unsorted", 1, 17, 48, 160, "f16x3", "b07db5a3af"),
    ("conv", 1, 4, 128, 256, "bf16", "932260c1c1"),
    ("conv", 1, 8, 64, 256, "bf16", "62789b0cdf"),
    ("mixed", 1, 4, 128, 256, "bf16", "7e9396948e"),
    ("mixed", 1, 8, 64, 256, "bf16", "0a154632c2"),
    ("unsorted", 1, 4, 128, 256, "bf16", "bc742c2fc6"),
    ("unsorted", 1, 8, 64, 256, "bf16", "aee9789cb0"),
    ("conv", 1, 4, 128, 256, "f16x3", "d7e5e57506"),
    ("conv", 1, 8, 64, 256, "f16x3", "4dc6428cfc"),
    ("mixed", 1, 4, 128, 256, "f16x3", "90c115fb49"),
    ("mixed", 1, 8, 64, 256, "f16x3", "27cc4ffba6"),
    ("unsorted", 1, 4, 128, 256, "f16x3", "f6dbbdf84f"),
    ("unsorted", 1, 8, 64, 256, "f16x3", "73c4919300"),
    ("conv", 1, 8, 100, 164, "bf16", "a224e65039"),
    ("mixed", 1, 8, 100, 164, "bf16", "9634326dbf"),
    ("unsorted", 1, 8, 100, 164, "bf16", "b83049a0a2"),
    ("conv", 1, 8, 100, 164, "f16x3", "984665e116"),
    ("mixed", 1, 8, 100, 164, "f16x3", "1cc4df258b"),
    ("unsorted", 1, 8, 100, 164, "f16x3", "98e392fde2"),
    ("conv", 1, 8, 128, 256, "bf16", "feb74127cc"),
    ("mixed", 1, 8, 128, 256, "bf16", "ae8bf42e19"),
    ("skip", 1, 8, 128, 256, "bf16", "6033d0d304"),
    ("unsorted", 1, 8, 128, 256, "bf16", "65279ff8ba"),
    ("conv", 1, 8, 128, 256, "f16x3", "1fcada12c9"),
    ("mixed", 1, 8, 128, 256, "f16x3", "d15845ae13"),
    ("skip", 1, 8, 128, 256, "f16x3", "8e1738aa07"),
    ("unsorted", 1, 8, 128, 256, "f16x3", "e65821a233"),
    ("conv", 1, 16, 100, 164, "bf16", "2369abe600"),
    ("mixed", 1, 16, 100, 164, "bf16", "ab19bb2ad0"),
    ("skip", 1, 16, 100, 164, "bf16", "d90901bb1d"),
    ("unsorted", 1, 16, 100, 164, "bf16", "dc9c565aee"),
    ("conv", 1, 16, 100, 164, "f16x3", "66057850ce"),
    ("mixed", 1, 16, 100, 164, "f16x3", "12efbf9a4c"),
    ("skip", 1, 16, 100, 164, "f16x3", "688e9904b2"),
    ("unsorted", 1, 16, 100, 164, "f16x3", "e44a9aa35c"),
    ("conv", 1, 12, 96, 228, "bf16", "7616b5ba67"),
    ("conv", 1, 12, 96, 228, "f16x3", "4b967741d9"),
    ("conv", 1, 17, 84, 184, "bf16", "a46a94f1e1"),
    ("conv", 1, 17, 92, 168, "bf16", "a9de34b114"),
    ("mixed", 1, 17, 84, 184, "bf16", "c6712337f9"),
    ("mixed", 1, 17, 92, 168, "bf16", "e7b19bb27c"),
    ("skip", 1, 17, 84, 184, "bf16", "77dbbe4999"),
    ("skip", 1, 17, 92, 168, "bf16", "7e45a4ed78"),
    ("unsorted", 1, 17, 84, 184, "bf16", "ea254b8c3a"),
    ("unsorted", 1, 17, 92, 168, "bf16", "9496ac0fe9"),
    ("conv", 1, 17, 84, 184, "f16x3", "88cbd3eca5"),
    ("conv", 1, 17, 92, 168, "f16x3", "98f2b20381"),
    ("mixed", 1, 17, 84, 184, "f16x3", "c3c3987c24"),
    ("mixed", 1, 17, 92, 168, "f16x3", "72b2df9620"),
    ("skip", 1, 17, 84, 184, "f16x3", "cc3e5f6710"),
    ("skip", 1, 17, 92, 168, "f16x3", "dd64c448be"),
    ("unsorted", 1, 17, 84, 184, "f16x3", "397d14efa0"),
    ("unsorted", 1, 17, 92, 168, "f16x3", "31c1cdf1d3"),
    ("conv", 1, 12, 112, 196, "f16x3", "f0e776419f"),
    ("conv", 1, 28, 48, 196, "f16x3", "76e39372a0"),
    ("conv", 1, 32, 128, 256, "bf16", "481858ed91"),
    ("conv", 1, 32, 128, 256, "f16x3", "a1f0156d2e"),
    ("conv", 1, 17, 132, 172, "f16x3", "88cbd3eca5"),
    ("conv", 1, 17, 132, 172, "bf16", "a46a94f1e1"),
    ("conv", 1, 8, 128, 256, "fp32", "e9803974d0"),
    ("conv", 2, 8, 128, 256, "f16x3", "1fcada12c9"),
    ("mixed", 2, 17, 20, 33, "fp32", "5c2ef3f6b6"),
    ("conv", 1, 16, 128, 131, "f16x3", "af50e6f602"),
    ("conv", 1, 16, 128, 131, "bf16", "6c3d9aaa2e"),
    ("conv", 2, 17, 20, 33, "f16x3", "94ddbfd43b"),
    ("mixed", 2, 12, 32, 33, "bf16", "774dab0ace"),
    # the head's classes that no chain class brought along: last_3_3d on the VALU form's tile configuration 1 (small route 2) under each
    # storage, on conv3d_c1 (0) under strict fp32, and the Staged resamples with small route 3 under strict fp32
    ("conv", 1, 4, 8, 131, "fp32", "c50bd1c107"),
    ("conv", 1, 17, 32, 256, "bf16", "ed8ffd5e3b"),
    ("conv", 1, 17, 32, 256, "f16x3", "ebdc6ac7be"),
    ("conv", 1, 17, 32, 256, "fp32", "349e0f1ee4"),
    ("conv", 1, 17, 64, 256, "fp32", "10c7f2fe49"),
)]
CAP = 2 ** 19
# Rows above the cap, one per storage type that has such a class: cells 3..7 all on the Box route is first reached at 32x128x256.
BIG_ROWS = {("conv", 1, 32, 128, 256, "f16x3"), ("conv", 1, 32, 128, 256, "bf16")}
# Classes of the grid that are reachable only above the cap and have NO row (one row per storage type may exceed the cap): the
# all-Box deep levels under the other genotypes, and the nsplit > 0 schedules of the level-3 launches at 32x132x256.  Digest of the
# class -> its smallest case.  test_table_covers_every_class_of_the_grid fails if this set changes in either direction.
UNCOVERED_ABOVE_CAP = {
    "82481c05bc": ('mixed', 1, 32, 128, 256, 'bf16'),
    "e58fb946c9": ('unsorted', 1, 32, 128, 256, 'bf16'),
    "7c360eeb05": ('mixed', 1, 32, 128, 256, 'f16x3'),
    "26fd2c5ec1": ('unsorted', 1, 32, 128, 256, 'f16x3'),
    "f984e76438": ('conv', 1, 32, 132, 256, 'bf16'),
    "ed9eba2108": ('mixed', 1, 32, 132, 256, 'bf16'),
    "1d1c244648": ('unsorted', 1, 32, 132, 256, 'bf16'),
    "b4b3458575": ('conv', 1, 32, 132, 256, 'f16x3'),
    "b664b3dba5": ('mixed', 1, 32, 132, 256, 'f16x3'),
    "7c0fb70d2b": ('unsorted', 1, 32, 132, 256, 'f16x3'),
}
# nseg of the z-marching schedules: the grid reaches these values, the table these (the class leaves the exact nseg out).
NSEG_GRID = {1, 2, 3, 4}
NSEG_TABLE = {1, 2, 3, 4}


def row_id(r):
    return f"{r.geno}-B{r.B}-{r.d}x{r.h}x{r.w}-{r.storage}"


def row_sig(r):
    return signature(r.geno, r.B, (r.d, r.h, r.w), r.storage)


def _nsegs(sig):
    return {e[-1][1] for e in sig[3] if e[-1][0] in ("ZMarch", "QuadRing")}


def test_table_digests(built_lib):
    """a changed host predicate, plan rule or route changes a row's signature: regenerate the table (and look at what moved)"""
    bad = [(row_id(r), r.digest, digest(row_sig(r))) for r in TABLE if digest(row_sig(r)) != r.digest]
    assert not bad, f"signatures moved — regenerate the table with `python tests/test_executor_plan_sweep.py`: {bad}"
    assert len({(r.geno, r.B, r.d, r.h, r.w, r.storage) for r in TABLE}) == len(TABLE)
    over = {(r.geno, r.B, r.d, r.h, r.w, r.storage) for r in TABLE if r.B * r.d * r.h * r.w > CAP}
    assert over == BIG_ROWS and len(over) <= 3


def test_table_covers_every_class_of_the_grid(built_lib):
    best = enumerate_grid()
    classes = {}
    for s, key in best.items():
        c = sig_class(s)
        if c not in classes or key < classes[c]:
            classes[c] = key
    sigs = [row_sig(r) for r in TABLE]
    covered = {sig_class(s) for s in sigs}
    missing = {digest(c): key[1:] for c, key in classes.items() if c not in covered}
    assert missing == UNCOVERED_ABOVE_CAP, (sorted(set(missing) ^ set(UNCOVERED_ABOVE_CAP)), "regenerate the table")
    # the classes without a row are out of reach below the cap on the grid (the finer search found none either)
    assert all(key[0] > CAP for c, key in classes.items() if c not in covered)
    # the head's classes (small route, resample routes) and every kind of 1x1x1 / resample launch: one by one, not as a product
    assert {head_class(s) for s in best} == {head_class(s) for s in sigs}
    assert set().union(*[k1_kinds(s) for s in best]) <= set().union(*[k1_kinds(s) for s in sigs])
    assert set().union(*[_nsegs(s) for s in best]) == NSEG_GRID
    assert set().union(*[_nsegs(s) for s in sigs]) == NSEG_TABLE


def test_table_reaches_every_regime(built_lib):
    """every regime of the plan and of the routes under it, each by at least one row"""
    seen = collections.Counter()
    for r in TABLE:
        storage, p_plan, p_head, k3, small, k1 = row_sig(r)
        cellsp, _cons, _stored, stem0_g4, fused, tail_rows = p_plan
        quarter, g4 = any(c[5] for c in cellsp), any(c[0] for c in cellsp)
        routes = {(e[0], e[-1][0]) for e in k3}
        vox, odd = r.d * r.h * r.w, (r.d % 2 == 1, r.w % 4 != 0)
        for name, hit in (("fused+quarter", fused and quarter), ("fused, quarter off", fused and not quarter and r.geno == "conv" and storage == "f16x3"),
                          ("g4 bf16", g4 and storage == "bf16"), ("Split2d", any(rt == "Split2d" for _i, rt in routes)),
                          ("Box cell 3", (3, "Box") in routes), ("QuadRing", any(rt == "QuadRing" for _i, rt in routes)),
                          ("ZMarch", any(rt == "ZMarch" for _i, rt in routes)),
                          ("all Box deep", all((i, "Box") in routes for i in range(3, 8))),
                          ("strict fp32 above 2^18", storage == "fp32" and vox >= 2 ** 18),
                          ("B=2 lower", r.B == 2 and not fused and vox < 2 ** 18 and storage != "fp32"), ("B=2 upper", r.B == 2 and fused),
                          ("odd d lower", odd[0] and not fused), ("odd d upper", odd[0] and fused),
                          ("ragged w lower", odd[1] and not fused), ("ragged w upper", odd[1] and fused),
                          ("17x132x172", (r.d, r.h, r.w) == (17, 132, 172)),
                          ("fused stems, no dual cell", fused and not any(c[1] for c in cellsp)),
                          ("small route", small is not None), ("taps+xblend", p_head[1] and p_head[2])):
            seen[name] += bool(hit)
    assert all(seen.values()), {k: v for k, v in seen.items() if not v}


# ------------------------------------------------------------------------------------------------------------ the oracle's side
@contextlib.contextmanager
def patched_oracle(bf_prefixes=(), bf_cells=(), defect=None, record=None, replay=None):
    """O.matching with O.conv_br_3d / O.cell_3d replaced for the length of the block (the oracle itself is not edited):
    bf_prefixes / bf_cells: units and cells whose output is rounded to bf16 when produced; defect: one of DEFECTS planted;
    record: dict that receives the stems' and cells' outputs; replay: such a dict from a clean run, returned instead of recomputing."""
    real_conv, real_cell = O.conv_br_3d, O.cell_3d

    def rnd(y):
        return y.to(bf16).to(y.dtype)

    def conv(x, sd, prefix, **kw):
        if replay is not None and prefix in replay:
            y = replay[prefix]
        else:
            y = real_conv(x, sd, prefix, **kw)
            if prefix in bf_prefixes:
                y = rnd(y)
        if record is not None and prefix.startswith("stem3d"):
            record[prefix] = y
        if defect == "batch" and prefix.startswith("stem3d1."):      # sample 1 given sample 0's T[-1]
            y = y.clone()
            y[1] = y[0]
        return y

    def cell(prev_prev, prev, sd, prefix, rows, fm, downup, training=False):
        i = int(prefix.split(".")[1])
        if replay is not None and i in replay:
            cat = replay[i]
        else:
            pp, p = prev_prev, prev
            if defect == "plane" and i == 0:        # the last depth plane of T[-1] zeroed before cell 0 reads it
                p = p.clone()
                p[:, :, -1] = 0
            if defect == "qshift" and i == 4:       # cell 4's pre_preprocess input resampled from T[2] shifted by one source row
                pp = torch.cat([pp[:, :, :, 1:], pp[:, :, :, -1:]], dim=3)
            _p, cat = real_cell(pp, p, sd, prefix, rows, fm, downup, training)
            if i in bf_cells:
                cat = rnd(cat)
        if record is not None:
            record[i] = cat
        if defect == "row" and i == 2:              # the last row of T[2] replaced by row h-2
            cat = cat.clone()
            cat[:, :, :, -1] = cat[:, :, :, -2]
        if defect == "col" and i == 5:              # the last column of cell 5's output replaced by column w-2
            cat = cat.clone()
            cat[..., -1] = cat[..., -2]
        if defect == "groups" and i == 0:           # two 4-channel groups of cell 0's concat swapped
            cat = cat[:, [4, 5, 6, 7, 0, 1, 2, 3] + list(range(8, cat.shape[1]))]
        return prev, cat

    O.conv_br_3d, O.cell_3d = conv, cell
    try:
        yield
    finally:
        O.conv_br_3d, O.cell_3d = real_conv, real_cell


# defect -> what a clean run's record may replay in front of it (the stems' prefixes are always replayable up to the defect)
DEFECTS = {"plane": ("stem3d0.0.", "stem3d1.0."), "row": ("stem3d0.0.", "stem3d1.0.", 0, 1, 2), "col": ("stem3d0.0.", "stem3d1.0.", 0, 1, 2, 3, 4, 5),
           "groups": ("stem3d0.0.", "stem3d1.0.", 0), "batch": ("stem3d0.0.", "stem3d1.0."), "qshift": ("stem3d0.0.", "stem3d1.0.", 0, 1, 2, 3)}


def row_inputs(idx):
    """(genotype rows, state dict, left, right, maxdisp) of table row idx: weights seeded by the row index, B different samples;
    under bf16 storage the features are the bf16-rounded ones for every run, the oracle's included"""
    r = TABLE[idx]
    rows = GENOTYPES[r.geno]
    sd = O.random_matching_state_dict(rows, seed=idx)
    g = gen(7000 + idx)
    lf, rf = torch.randn((r.B, C_FEA, r.h, r.w), generator=g), torch.randn((r.B, C_FEA, r.h, r.w), generator=g)
    if r.storage == "bf16":
        lf, rf = lf.to(bf16).float(), rf.to(bf16).float()
    return rows, sd, lf, rf, 3 * r.d


def _oracle(rows, sd, lf, rf, maxdisp, dtype, **patch):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    with patched_oracle(**patch), torch.no_grad():
        disp, inter = O.matching_net_forward(lf.to(dtype), rf.to(dtype), sd, rows, maxdisp, return_intermediates=True)
    return inter["mat"], disp


def rel_err(mat, mat64):
    return float((mat.double() - mat64).abs().max()) / float(mat64.abs().max())


_REF = {}
Ref = collections.namedtuple("Ref", "mat64 disp64 E32 Ebf epe32 epebf")


def reference(idx, want_e32=False):
    """The fp64 oracle of row idx and the error the oracle ALONE shows for it: E32 = the fp32 oracle against the fp64 one (fp32
    storage rows, and on request), Ebf = the fp32 oracle with the tensors the plan stores as bf16 rounded to bf16 when produced (the
    stems' outputs, the cells' outputs and pre-processed inputs with plan.cdt == bfloat16).  Computed once per row and process."""
    from rag_amd import ops
    r = TABLE[idx]
    hit = _REF.get(idx)
    if hit is None or (want_e32 and hit.E32 is None):
        torch.set_num_threads(min(16, max(torch.get_num_threads(), 1)))
        rows, sd, lf, rf, maxdisp = row_inputs(idx)
        mat64, disp64 = (hit.mat64, hit.disp64) if hit is not None else _oracle(rows, sd, lf, rf, maxdisp, f64)
        E32 = Ebf = epe32 = epebf = None
        if r.storage != "bf16" or want_e32:
            m32, d32 = _oracle(rows, sd, lf, rf, maxdisp, f32)
            E32, epe32 = rel_err(m32, mat64), O.epe(d32, disp64)
        if r.storage == "bf16":
            if hit is not None:
                Ebf, epebf = hit.Ebf, hit.epebf
            else:
                with defaults(ops, STORAGES[r.storage][1]):
                    plan = plans(r.geno, r.B, (r.d, r.h, r.w), r.storage)[2]
                cells_bf = {i for i in range(8) if plan.cdt[i] == bf16}
                prefixes = {f"stem3d{k}.0." for k in (0, 1)} | {f"cells_3d.{i}.0.{u}." for i in cells_bf for u in ("pre_preprocess", "preprocess")}
                mbf, dbf = _oracle(rows, sd, lf, rf, maxdisp, f32, bf_prefixes=prefixes, bf_cells=cells_bf)
                Ebf, epebf = rel_err(mbf, mat64), O.epe(dbf, disp64)
        hit = _REF[idx] = Ref(mat64, disp64, E32, Ebf, epe32, epebf)
    return hit


# ------------------------------------------------------------------------------------------------------- 4. the gates of check (a)
# e <= K * E(row): E is the oracle's own error for the row (reference()), K the smallest power of two at least twice the worst e / E
# measured on the MI355X (the table in the docstring), under the caps K_CAP (conditions, not measurements).
K_CAP = {"fp32": 16, "f16x3": 128, "bf16": 8}
K = {"fp32": 4, "f16x3": 4, "bf16": 8}
assert all(K[s] <= K_CAP[s] for s in K)
# bf16 storage at reduced sizes, as test_hip_parity.test_bf16_matchingnet_epe_report gates it; a row whose ORACLE, with nothing but the
# plan's bf16 roundings, is already past half of that (tiny maps, nearly an argmax: 0.10 px at 17x8x8) is held to twice the oracle's own
BF16_EPE_GATE = 0.08


def gate(idx):
    r, ref = TABLE[idx], reference(idx)
    return K[r.storage] * (ref.Ebf if r.storage == "bf16" else ref.E32)


# ------------------------------------------------------------------------------------- 5. the caps leave the test sharp (CPU only)
# defects that stay below 10 x (cap x Ebf) on bf16-storage rows although the fp32-f16x3 threshold of the same genotype and shape sees
# them: bf16 storage alone moves `mat` by ~4e-3 of its largest magnitude, a one-plane / one-row defect of a deep tensor by less
INVISIBLE_UNDER_BF16 = {"plane", "row", "col", "groups", "qshift"}
COND_ROWS = [i for i, r in enumerate(TABLE) if r.B * r.d * r.h * r.w <= 2 ** 18]
assert {TABLE[i].storage for i in COND_ROWS} == set(STORAGES)


@pytest.mark.parametrize("idx", COND_ROWS, ids=[row_id(TABLE[i]) for i in COND_ROWS])
def test_planted_defects_exceed_ten_times_the_capped_gate(built_lib, idx):
    """Each wiring / edge defect planted in the ORACLE moves `mat` by at least 10 x (cap x E(row)): the capped gate of check (a) cannot
    let it through.  The EPE each one causes is printed next to EPE_GATE: the ones below it are what the EPE-only checks let through."""
    r = TABLE[idx]
    ref = reference(idx, want_e32=True)
    rows, sd, lf, rf, maxdisp = row_inputs(idx)
    clean = {}
    m32, _d = _oracle(rows, sd, lf, rf, maxdisp, f32, record=clean)
    bad = []
    for name, replayable in DEFECTS.items():
        if name == "batch" and r.B < 2:
            continue
        mat, disp = _oracle(rows, sd, lf, rf, maxdisp, f32, defect=name, replay={k: clean[k] for k in replayable})
        if torch.equal(mat, m32):
            # The planted change changes nothing here, so there is nothing to see.  Only the all-skip genotype does that: its three new
            # states are the same sum s0 + s1, so two swapped groups of the concat are equal planes; and without a 3x3x3 conv depth
            # planes never mix, and at d = 4 the 1/4 level (one plane, align_corners) reads plane 0 only.
            assert r.geno == "skip" and (name == "groups" or (name == "plane" and r.d == 4)), (row_id(r), name)
            print(f"{row_id(r)} defect {name:6s}: no change of `mat` in this genotype and shape")
            continue
        e, epe = rel_err(mat, ref.mat64), O.epe(disp, ref.disp64)
        thr32 = 10 * K_CAP["fp32" if r.storage == "fp32" else "f16x3"] * ref.E32
        thr = 10 * K_CAP["bf16"] * ref.Ebf if r.storage == "bf16" else thr32
        print(f"{row_id(r)} defect {name:6s}: e {e:.2e} (10 x cap x E = {thr:.2e}{'' if r.storage != 'bf16' else f'; the f16x3 threshold {thr32:.2e}'}); "
              f"EPE {epe:.2e} px {'<=' if epe <= EPE_GATE else '>'} EPE_GATE {EPE_GATE:g}")
        if e < thr32:
            bad.append((name, e, thr32))
        elif e < thr and name not in INVISIBLE_UNDER_BF16:
            bad.append((name, e, thr, "bf16"))
    assert not bad, (row_id(r), bad)


# -------------------------------------------------------------------------------------------------------------- 3. the GPU sweep
def _poison_and_rerun(run, peak, first_numel, dtype):
    """check (d): every cached block of the allocator holds 0xFF bytes (NaN as fp32 and as bf16) when the forward runs again, so a
    launch that reads what no launch wrote shows as a NaN or as other bits.  Returns (outputs, whether the poison really arrived).
    One freed block of twice the peak is not enough: the allocator serves a request from the smallest cached block that fits, and the
    free parts of segments that live tensors pin (outputs, features, weights) fit before the big block does, as do the 2 MiB
    segments of the small-block pool.  With the big block alone the guard below failed on most rows, with the walk over the inactive
    blocks added on 14 of 115; with the guard poisoning what it is handed, on none."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # what stays cached after empty_cache() are the free parts of segments that live tensors pin: take each of them exactly (best fit)
    free = sorted((b["size"] for seg in torch.cuda.memory_snapshot() for b in seg["blocks"] if b["state"] == "inactive"), reverse=True)
    hold = [torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda:0") for n in free]
    big = torch.full((max(2 * peak, 64 << 20),), 0xFF, dtype=torch.uint8, device="cuda:0")
    small = [torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device="cuda:0") for _ in range(2 * (peak >> 20) + 8)]      # the small-block pool
    torch.cuda.synchronize()
    del hold
    del big, small
    # the guard: an empty() of cell 0's buffer size must read back NaN.  A block it gets that was not poisoned (one the walk above could
    # not take exactly, or fresh memory) is poisoned now and held, and the guard asks again; the last answer counts.
    held = []
    for _ in range(24):
        probe = torch.empty((first_numel,), dtype=dtype, device="cuda:0")
        if bool(torch.isnan(probe.float()).all()):
            break
        probe.view(torch.uint8).fill_(0xFF)
        held.append(probe)
    del probe, held
    probe = torch.empty((first_numel,), dtype=dtype, device="cuda:0")
    arrived = bool(torch.isnan(probe.float()).all())
    del probe
    return run(), arrived


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(TABLE)), ids=[row_id(r) for r in TABLE])
def test_row_on_gpu(ra, idx):
    r = TABLE[idx]
    ops = ra.ops
    sdt, prec = STORAGES[r.storage]
    rows, sd, lf, rf, maxdisp = row_inputs(idx)
    ref = reference(idx)
    E = ref.Ebf if r.storage == "bf16" else ref.E32
    net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=maxdisp)
    net.load_state_dict(sd, strict=True)
    net = net.to("cuda:0").eval()
    glf, grf = gpu(lf).to(sdt), gpu(rf).to(sdt)

    def run():
        with torch.no_grad():
            mat = net.matching(None, net.arch_init, None, features=(glf, grf))
            disp = net(glf, grf)
        return mat, disp

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    bad = []
    with defaults(ops, prec):
        assert digest(row_sig(r)) == r.digest      # the plan that runs is the one the row stands for
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = run()
        torch.cuda.synchronize()
        peak = int(torch.cuda.max_memory_allocated())
        live_plan = dict(net.last_g4_plan)
        # (a) mat element by element
        mat, disp = base[0].cpu(), base[1].cpu()
        assert mat.dtype == f32 and tuple(mat.shape) == (r.B, 1, r.d, r.h, r.w)
        err = (mat.double() - ref.mat64).abs()
        e, g = float(err.max()) / float(ref.mat64.abs().max()), gate(idx)
        epe = O.epe(disp, ref.disp64)
        print(f"SWEEP {idx:3d} {row_id(r):34s} e {e:.3e} E {E:.3e} e/E {e / E:7.2f} gate {g:.3e} | EPE {epe:.3e} px (oracle alone: "
              f"{ref.epebf if r.storage == 'bf16' else ref.epe32:.3e})")
        if not (torch.isfinite(mat).all() and e <= g):
            at = np.unravel_index(int(err.argmax()), err.shape)
            print(f"  worst at (b, d, h, w) = {(at[0],) + tuple(at[2:])}; per-axis maxima of |err| / max |mat64|:")
            for ax, nm in ((2, "d"), (3, "h"), (4, "w")):
                prof = err.amax(dim=[a for a in range(5) if a != ax]) / float(ref.mat64.abs().max())
                print(f"  {nm}: " + " ".join(f"{v:.1e}" for v in prof.tolist()))
            bad.append(("a", e, g))
        # (b) the disparity map
        epe_gate = max(BF16_EPE_GATE, 2 * ref.epebf) if r.storage == "bf16" else EPE_GATE
        if not (torch.isfinite(disp).all() and epe <= epe_gate):
            bad.append(("b", epe, epe_gate))
        # (c) switch invariance (tools/fuzz_fused.py's matrix): the quarter store keeps every bit; with the tail rows off, G4 and the
        # stem fusion keep every bit; the tail rows themselves are another arithmetic for one 1x1x1 conv: inside gate (a)
        try:
            ops.set_quarter_store(False)
            if not same(run(), base):
                bad.append(("c", "quarter store off"))
            ops.set_quarter_store(True)
            ops.set_stem_tail_rows(False)
            r0 = run()
            e0 = rel_err(r0[0].cpu(), ref.mat64)
            if not e0 <= g:
                bad.append(("c", "tail rows off", e0, g))
            if not live_plan.get("stem_tail_rows", False) and not same(r0, base):
                bad.append(("c", "tail rows off where the plan has none"))
            for g4, fuse, quarter in ((False, True, True), (True, False, True), (False, False, False)):
                ops.set_g4(g4)
                ops.set_stem_fusion(fuse)
                ops.set_quarter_store(quarter)
                if not same(run(), r0):
                    bad.append(("c", f"g4={g4} fusion={fuse} quarter={quarter} (tail rows off)"))
        finally:
            ops.set_g4(True)
            ops.set_stem_fusion(True)
            ops.set_quarter_store(True)
            ops.set_stem_tail_rows(True)
        # (e) determinism
        if not same(run(), base):
            bad.append(("e", "a third default run has other bits"))
        # (d) nothing unwritten is read
        again, arrived = _poison_and_rerun(run, peak, r.B * 8 * r.d * r.h * r.w, sdt)
        if not (torch.isfinite(again[0]).all() and torch.isfinite(again[1]).all() and same(again, base)):
            bad.append(("d", "the forward on poisoned memory has other bits or a non-finite value"))
    assert not bad, (row_id(r), bad)
    if not arrived:
        pytest.xfail("check (d): the allocator did not hand the poisoned block back (an empty() of cell 0's buffer size read no NaN)")


def regenerate():
    """print the table rows for the current library (the classes' smallest cases over the grid; then the named rows by hand)"""
    import rag_amd
    rag_amd.load_library()
    classes = {}
    for s, key in enumerate_grid().items():
        c = sig_class(s)
        if c not in classes or key < classes[c]:
            classes[c] = key
    for c, (v, g, B, d, h, w, st) in sorted(classes.items(), key=lambda kv: (kv[1][0], kv[1][6], kv[1][1], kv[1][2:])):
        print(f'    ("{g}", {B}, {d}, {h}, {w}, "{st}", "{digest(signature(g, B, (d, h, w), st))}"),   # class {digest(c)}' + ("  ABOVE THE CAP" if v > CAP else ""))
    heads = {}
    for s, key in enumerate_grid().items():
        heads[head_class(s)] = min(heads.get(head_class(s), key), key)
    have = {head_class(signature(g, B, (d, h, w), st)) for (_v, g, B, d, h, w, st) in classes.values()}
    for hc, (v, g, B, d, h, w, st) in sorted(heads.items(), key=lambda kv: kv[1]):
        if hc not in have:
            print(f'    ("{g}", {B}, {d}, {h}, {w}, "{st}", "{digest(signature(g, B, (d, h, w), st))}"),   # head class {digest(hc)}')


if __name__ == "__main__":
    regenerate()
