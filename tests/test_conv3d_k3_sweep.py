"""Sweep of the packed-weight 3x3x3 forward convolutions (ragmi_conv3d_k3_fwd_ex / ragmi_conv3d_k3_dual_fwd_ex) over every route of
k3_dispatch (rag_amd/csrc/conv3d.hip) — Mfma conv3d_k3_kernel, ZMarch conv3d_x3_kernel, QuadRing conv3d_x3q_kernel, Box
conv3d_x3d_kernel, Split2d conv2d_x3_kernel — and every form of their launch switches, through ops.conv3d_k3, ops.conv3d_k3_dual,
ops.Tail and ops.conv3d_k3_pack only, against per set
    pre = F.conv3d(x.double(), w.double(), padding=1)          from the values the kernel reads (bf16-rounded under bf16 storage)
then scale / shift / ReLU, the sum of the sets, the residual and the tails in float64.

Gate, per element, nothing excused; mag = F.conv3d(|x|, |w|), block = Xmax * sum|w| + Wmax * sum|x| (Xmax tensor-wide), float64:
    arith, route Mfma            1e-6 * mag                                             (include/rag_amd.h: an fmaf chain)
    arith, the four split routes (2^-20 + 1e-6) * mag + 2^-33 * block                   (F32X3)
    arith, split routes, bf16    (2^-18 + 1e-6) * mag                                    (bf16 storage: departure 1 below)
    a set after BatchNorm        b_s = |scale| * arith + 2^-23 * (|scale * pre| + |shift|)      (no BatchNorm: b_s = arith)
    main output                  sum_s b_s + 2^-23 * (sum_s |act(u_s)| + |res|)
    bf16 storage                 + 2^-8 * |ref| for every stored tensor
    full-resolution tail k       |s_t| * (sum_co |W_t[k,co]| * bound_main[co] + 1e-6 * sum_co |W_t[k,co] * main_ref[co]|)
                                 + 2^-23 * (|s_t * (W_t @ main)| + |h_t|)
    down-sampling tail           reference in the reference's order: F.interpolate(main.float(), half, 'trilinear',
                                 align_corners=True), then the mix in float64.  Bound: the same interpolation of the pre-BN tail bound
                                 + 1e-6 * the interpolated sum_co |W_t[k,co] * main[co]| + 2^-22 * the largest of the eight corners'
                                 sum_co |W_t[k,co] * main[co]| (the fp32 lambdas, and ATen's own fp32 interpolation in the reference),
                                 then |s_t| and the fma term as above.
bound_main of a tail is the main bound WITHOUT the storage term: conv3d_k3_kernel's epilogue feeds the tails from `fin` and
conv3d_x3_kernel's from `v`, the fp32 values before the store rounds them (conv3d_x3q_kernel runs under fp32 storage only; the box
and depth-1 kernels take no tails).  Channels no store may touch — two guard channels either side of every destination, the unused
groups of a permuted out_group_ch, the whole main output under store_main=False — are prefilled with NaN and must come back NaN.

Departures from the plan this file was written to, each forced by arithmetic and written down before the rerun:
  1. bf16 storage on the split routes.  The plan held it to the F32X3 arithmetic term.  conv3d_x3_kernel<bf16_t> and
     conv3d_x3d_kernel<bf16_t> multiply the exact bf16 activations with TWO bf16 halves of each weight, w = hi + lo + r with
     hi = bf16(w), lo = bf16(w - hi), both rounded to nearest: |w - hi| <= 2^-9 |w| and |lo - (w - hi)| <= 2^-9 |w - hi|, so
     |r| <= 2^-18 |w| and the dropped products are at most 2^-18 * mag (include/rag_amd.h grants this path 2^-16 per weight).  bf16
     has fp32's exponent range and nothing is scaled, so there is no block term.  On N(0,1) data the 2^-8 |ref| storage term hides
     the difference; on the "spread" family, where |ref| << mag, the two bf16 rows measured 1.72 (ZMarch) and 1.17 (Box) times the
     F32X3 gate, about 3.4e-6 * mag, which is 0.70 of (2^-18 + 1e-6) * mag.  Every other row passed the plan's gate as written.
  2. The yardstick on the "spread" family.  1e-6 * mag is no a-priori bound for a 324-term fp32 sum in an arbitrary order
     (27 * Cin * 2^-24 * mag is): ATen's fp32 convolution measured 1.07e-6 * mag on ONE of the 6.4 M outputs of the 12 -> 12
     z-marching spread row (8.2e-7 and below on the other spread rows).  No spread row runs under the fp32 gate — the family
     belongs to the split routes — so on those rows ATen is held to the gate the row itself is held to and to the a-priori bound.

Non-finite inputs (one Inf, NaN or 3e38 on a tile corner of sample 1; the reference is computed with that element zeroed and
reach = F.conv3d(indicator, |w|) > 0).  Without ReLU the non-finite outputs are exactly the reach and every other voxel keeps the
gate.  With BN + ReLU every value inside the reach is non-finite or exactly +0 — the epilogues apply fmaxf(u, 0.f), which stores a
NaN pre-activation as 0 (include/rag_amd.h says so now); the assertion is there to catch a finite WRONG value, not to bless the
flush.  Two departures, both forced by arithmetic and not by a measurement:
  * a dual launch adds the other set's finite act(u_B) to that +0, so inside the reach a finite value must be act(u_B) within the
    gate of set B alone;
  * 3e38 is finite: a product 3e38 * w with |w| < 1.13 does not overflow fp32, so on route Mfma — and under bf16 storage, whose
    operands hold 3e38 — a voxel of the reach may be finite; it must then be inside the row's gate of the float64 result WITH the
    element.  Under F32X3 the split routes cannot scale 3e38 into fp16's range (include/rag_amd.h: operands above ~2^110) and give
    non-finite values over the whole reach.

Rows are the smallest shapes that reach their class; the CPU tests make the probe ops.conv3d_k3_route (and ops.conv3d_k3_plan for the
Mfma tile configuration and G) the authority on that: every row's route and instantiation key is checked, the keys written out below
from the launch switches are all covered, and the Python restatement of x3_schedule that chose the z-marching rows equals the probe.
k3_probe answers for two equal sets of whole chunks only, so the ragged dual rows (4 + 3, 8 + 4, 4 + 8: all under
conv_precision("fp32"), where the route is Mfma whatever the channels) are probed as 4 + 4.

Every GPU row prints `K3 case=... route=... worst=err/bound`.  Measured on the MI355X, worst err / bound (records, not gates):
  Mfma      fp32 storage: matrix 0.363 (cfg 0, 4 -> 12), geometry 0.371 (1x2x1x524288), epilogue 0.331 (transpose), tails 0.058,
            offset family 0.138, non-finite 0.309          bf16 storage: matrix 0.995, tails 0.993, offset family 0.941
  ZMarch    fp32 storage: instantiations 0.135, wide outputs 0.124, schedule classes 0.138, with down-sampling tails 0.120, tails 0.054,
            down-sampling tails 0.030, families n01 0.138 / offset 0.053 / spread 0.472 / steps 0.141 / sparse 0.155, non-finite 0.138
            bf16 storage: main 0.993, tails 0.985, down-sampling tails 0.977, families 0.990 / 0.952 / 0.996 / 0.992 / 0.994
  QuadRing  instantiations 0.077, tails 0.036, down-sampling tails 0.019, schedule classes 0.092, families n01 0.074 / offset 0.039 /
            spread 0.316 / steps 0.087 / sparse 0.139, non-finite 0.076
  Box       fp32 storage: instantiations 0.090, geometry 0.064, families 0.062 / 0.031 / 0.342 / 0.071 / 0.102, non-finite 0.062
            bf16 storage: instantiations 0.990, geometry 0.988, families 0.988 / 0.969 / 0.995 / 0.995 / 0.991
  Split2d   instantiations 0.095, geometry 0.102, families n01 0.092 / offset 0.076 / spread 0.249 / steps 0.132 / sparse 0.144,
            non-finite 0.105
The bf16 rows sit at 0.94..0.996 of their gate by construction: round to nearest moves a value just above a power of two by up to
2^-8 of itself, which is the storage term of the gate; the fp32 rows above are the arithmetic underneath.  No row failed for a
wrong kernel; the two bf16 "spread" rows failed the plan's arithmetic term (departure 1).

Unmarked tests run without a GPU; the rest need the MI355X."""
import collections
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
E8, E18, E20, E22, E23, E33 = 2.0 ** -8, 2.0 ** -18, 2.0 ** -20, 2.0 ** -22, 2.0 ** -23, 2.0 ** -33
NAN = float("nan")
GUARD = 2
FAR = 10 ** 9

Row = collections.namedtuple("Row", "tag route shape cins cout bf prec bn relu res tails store_main fam slices perm transpose bad")


def R(tag, route, shape, cins, cout, bf=False, prec="f16x3", bn=True, relu=True, res=None, tails=(), store_main=True, fam="n01",
      slices=False, perm=False, transpose=False, bad=None):
    """tails: ((k, down, bn, relu), ...); res: None | "other" | "alias"; bad: (value, (z, y, x)) in channel 1 of sample 1"""
    return Row(tag, route, tuple(shape), tuple(cins), cout, bf, prec, bn, relu, res, tuple(tails), store_main, fam, slices, perm, transpose, bad)


def rid(r):
    return "{}-{}_{}_c{}o{}_{}{}".format(r.route, r.tag, "x".join(map(str, r.shape)), "+".join(map(str, r.cins)), r.cout,
                                          "bf16" if r.bf else "f32", "" if r.prec == "f16x3" else "_fp32")


# --------------------------------------------------------------------------- host restatements (checked against the probes below)
def cdiv(a, b):
    return -(-a // b)


def split_groups(ng):
    return next((g for g in (4, 3, 2) if ng % g == 0), 1)


def choose_cfg(B, D, H, W, cout):
    vol = B * D * H * W
    waste = lambda tx: cdiv(W, tx) * tx / W      # noqa: E731
    if W > 16 and waste(32) <= waste(16) + 1e-9 and vol >= 1 << 20:
        return 0
    if W > 8 and waste(16) <= waste(8) + 1e-9 and vol >= 1 << 17 and not (cout >= 20 and vol < 1 << 19):
        return 1
    return 2


def x3_schedule(B, D, H, W, cout, bf, ndown):
    """(seg_len, nseg, nsplit, ngrp) of x3_schedule in rag_amd/csrc/conv3d_x3.hip"""
    tx, ty, ncog = cdiv(W, 32), cdiv(H, 8), cdiv(cout, 16)
    cols_seg = tx * ty * (B if bf else 1)
    nseg = max(1, min(cdiv(1536, cols_seg * ncog), cdiv(D, 8)))
    seg_len = cdiv(D, nseg)
    if ndown:
        seg_len += seg_len & 1
    nseg = cdiv(D, seg_len)
    per = tx * ty * nseg
    ngrp = 8 if per % 8 == 0 else 1
    nsplit = 0
    if ngrp == 8 and seg_len >= 4 and 0 < (per // 8) % 64 <= 32:
        nsplit = (per // 8) % 64
    if ndown and (seg_len % 4 or (D - (nseg - 1) * seg_len) % 4):
        nsplit = 0
    return seg_len, nseg, nsplit, ngrp


def ntails(r):
    return sum(1 for t in r.tails if not t[1]), sum(1 for t in r.tails if t[1])


def inst_key(r):
    """the template instantiation a row lands on, as the launch switches of its route pick it"""
    nset, (nt, nd) = len(r.cins), ntails(r)
    B, D, H, W = r.shape
    if r.route == "Mfma":
        return ("k3", r.bf, nset, choose_cfg(B, D, H, W, r.cout), split_groups(cdiv(r.cout, 4)))
    tl = 2 if nd else 1 if nt else 0
    if r.route == "ZMarch":
        return ("x3", r.bf, sum(r.cins) // 4, nset, tl)
    if r.route == "QuadRing":
        return ("x3q", tl)
    if r.route == "Box":
        ch8 = r.cins[0] // 8
        return ("x3d", r.bf, ch8, nset, 2 if (ch8 == 1 and nset == 2 and r.cout > 16) else 1, ch8 == 2 and nset == 2)
    return ("x2d", r.cins[0] // 4, nset)


# conv3d_k3_kernel<T, G, cfg, NSET>: k3_dispatch's table x launch_cfg's switch
ALL_KEYS = {("k3", bf, nset, cfg, G) for bf in (False, True) for nset in (1, 2) for cfg in (0, 1, 2) for G in (1, 2, 3, 4)}
# conv3d_x3_kernel<T, NCG, NSET, TAILS>: x3_launch's switches.  One set: 1..6 groups; TAILS = 2 for <= 3 groups; 8 and 16 channels
# without tails belong to the box kernel.  Two sets: 4 + 4 (fp32 storage: only past the quad-ring kernel's 16 outputs, hence without
# tails) and 8 + 8 with full-resolution tails (without: the box kernel; down-sampling tails: not instantiated)
ALL_KEYS |= {("x3", bf, ncg, 1, 0) for bf in (False, True) for ncg in (1, 3, 5, 6)}
ALL_KEYS |= {("x3", bf, ncg, 1, 1) for bf in (False, True) for ncg in (1, 2, 3, 4, 5, 6)}
ALL_KEYS |= {("x3", bf, ncg, 1, 2) for bf in (False, True) for ncg in (1, 2, 3)}
ALL_KEYS |= {("x3", True, 2, 2, t) for t in (0, 1, 2)} | {("x3", False, 2, 2, 0)} | {("x3", bf, 4, 2, 1) for bf in (False, True)}
ALL_KEYS |= {("x3q", t) for t in (0, 1, 2)}                                            # conv3d_x3q_kernel<2, TAILS, false, false>
# conv3d_x3d_kernel<T, CH8, NSET, COGS, false, W16>: the five branches of x3d_launch
ALL_KEYS |= {("x3d", bf) + k for bf in (False, True) for k in ((1, 1, 1, False), (1, 2, 1, False), (1, 2, 2, False), (2, 1, 1, False), (2, 2, 1, True))}
ALL_KEYS |= {("x2d", n, 1) for n in (1, 2, 3, 4)} | {("x2d", 1, 2), ("x2d", 2, 2)}      # conv2d_x3_kernel<NCGS, NSET>

# --------------------------------------------------------------------------- rows
S2, S1, S0 = (2, 5, 9, 33), (1, 4, 128, 256), (4, 4, 128, 512)      # tile configurations 2, 1, 0 of the fp32-MFMA kernel (D < 8: bf16 storage stays off the z-marching kernel)
CFG_SHAPE = {2: S2, 1: S1, 0: S0}
FULL1 = ((3, False, True, True),)
FULL2 = ((1, False, True, True), (3, False, False, False))
FULL2B = ((4, False, True, False), (2, False, True, True))
FULL4 = ((4, False, True, True),)
DOWN1 = ((4, True, True, True),)
DOWN2 = ((4, True, True, True), (4, True, False, False))
BOTH = ((4, False, True, True), (4, True, True, False))


def mfma_matrix():
    one = {4: (3,), 8: (7,), 12: (10,), 16: (12,)}
    two = {4: (4, 3), 8: (4, 4), 12: (8, 4), 16: (4, 8)}
    rows = []
    for bf in (False, True):
        for nset in (1, 2):
            for cfg in (0, 1, 2):
                for cout in (4, 8, 12, 16):
                    cins = (one if nset == 1 else two)[cout] if cfg == 2 else (4,) * nset
                    rows.append(R(f"cell_cfg{cfg}", "Mfma", CFG_SHAPE[cfg], cins, cout, bf, "fp32"))
    return rows


MFMA_MATRIX = mfma_matrix()
MFMA_COUT = [R("cout", "Mfma", S2, (4,), co, False, "fp32") for co in (5, 13, 20, 24, 48, 64)]
MFMA_COUT += [R("cout", "Mfma", S2, (4, 4), co, False, "fp32") for co in (5, 20, 48)]
MFMA_COUT += [R("cout", "Mfma", S2, (4,), co, True, "fp32") for co in (5, 13)]
MFMA_DEFAULT = [      # the default precision on shapes the split-operand kernels do not take: the same kernel
    R("res_on_box_shape", "Mfma", (1, 2, 64, 128), (8,), 8, res="other"),
    R("ragged_cin", "Mfma", (1, 2, 64, 128), (10,), 12),
    R("ragged_cout", "Mfma", (1, 2, 64, 128), (8,), 13),
    R("res_on_zmarch_shape", "Mfma", (1, 8, 128, 256), (4,), 4, res="alias"),
    R("res_on_depth1_shape", "Mfma", (2, 1, 8, 32), (4,), 4, res="other"),
    R("res_on_box_shape", "Mfma", (1, 2, 64, 128), (16,), 8, True, res="other"),
]
# D around the 4-plane tiles; H, W at 1 and at tile size - 1, the size, + 1 (8 x 8, 16 x 8, 32 x 8 — 32 x 4 for two sets) where
# choose_cfg lets them (configuration 1 wants W % 16 in {0, 9..15}, configuration 0 W % 32 in {0, 17..31}); the last of each: >= 4096 tiles
MFMA_GEOM_SHAPES = {
    2: [(1, 1, 1, 1), (1, 2, 3, 5), (2, 3, 7, 9), (1, 4, 8, 7), (2, 5, 9, 8), (1, 7, 1, 9), (1, 3, 9, 1), (2, 64, 1024, 8)],
    1: [(16, 1, 512, 16), (1, 2, 4097, 16), (1, 3, 2735, 16), (1, 4, 1, 32768), (2, 5, 57, 240), (3, 7, 417, 15), (1, 64, 2048, 16)],
    0: [(1, 1, 1024, 1024), (1, 2, 1, 524288), (1, 3, 10923, 32), (1, 4, 8193, 32), (1, 5, 6559, 32), (1, 7, 4682, 32), (3, 9, 68, 575)],
}
MFMA_GEOM = [R(f"geom_cfg{cfg}", "Mfma", s, (4,) * nset, 4, False, "fp32") for cfg in (2, 1, 0) for s in MFMA_GEOM_SHAPES[cfg] for nset in (1, 2)]
# >= 4096 tiles of configuration 0: 32 x 8 x 4 voxels for one set, 32 x 4 x 4 (2 rows per lane) for two
MFMA_GEOM += [R("geom_cfg0_4096tiles", "Mfma", (1, 64, 256, 256), (4,), 4, False, "fp32"), R("geom_cfg0_4096tiles", "Mfma", (1, 64, 128, 256), (4, 4), 4, False, "fp32")]


def mfma_epilogue():
    rows = []
    for s in (S2, S1):
        k = dict(shape=s, prec="fp32")
        rows += [R(f"bn{int(bn)}relu{int(relu)}", "Mfma", cins=(8,), cout=12, bn=bn, relu=relu, **k) for bn, relu in ((False, False), (True, False), (False, True))]
        rows += [R("res_other", "Mfma", cins=(8,), cout=12, res="other", **k), R("res_alias", "Mfma", cins=(8,), cout=12, res="alias", **k),
                 R("res_alias", "Mfma", cins=(4, 4), cout=8, res="alias", **k), R("perm", "Mfma", cins=(8,), cout=12, perm=True, **k),
                 R("perm_res", "Mfma", cins=(4, 4), cout=24, perm=True, res="other", **k),
                 R("slices", "Mfma", cins=(10,), cout=13, slices=True, res="other", **k), R("slices", "Mfma", cins=(4, 3), cout=5, slices=True, res="other", **k),
                 R("slices", "Mfma", cins=(10,), cout=13, bf=True, slices=True, res="other", **k),
                 R("tails", "Mfma", cins=(8,), cout=12, tails=FULL2, **k), R("tails_nomain", "Mfma", cins=(8,), cout=16, tails=FULL2B, store_main=False, **k),
                 R("tails", "Mfma", cins=(4, 4), cout=8, tails=FULL2B, **k), R("tails_nomain", "Mfma", cins=(8,), cout=4, bf=True, tails=FULL2, store_main=False, **k),
                 R("tails", "Mfma", cins=(8,), cout=12, bf=True, tails=FULL2B, res="other", **k),
                 R("transpose", "Mfma", cins=(7,), cout=12, transpose=True, **k)]
    return rows


MFMA_EPI = mfma_epilogue()

Z0 = (1, 8, 128, 256)
Z_SCHED = [(1, 8, 128, 256), (2, 9, 131, 227), (1, 13, 160, 128), (1, 33, 90, 93), (1, 8, 993, 33), (1, 64, 64, 64)]
Z_SCHED_DOWN = [(1, 8, 128, 256), (2, 10, 132, 200), (1, 14, 128, 160), (1, 24, 64, 176), (1, 8, 130, 254)]


def zmarch_rows():
    rows = []
    for bf in (False, True):
        rows += [R("inst", "ZMarch", Z0, (c,), co, bf) for c, co in ((4, 4), (12, 12), (20, 16), (24, 12))]
        rows += [R("inst_tail", "ZMarch", Z0, (c,), co, bf, tails=t) for c, co, t in ((4, 12, FULL2), (8, 4, FULL1), (12, 16, FULL2B), (16, 12, FULL1), (20, 4, FULL2), (24, 16, FULL1))]
        rows += [R("inst_down", "ZMarch", Z0, (c,), co, bf, tails=t) for c, co, t in ((4, 16, DOWN1), (8, 12, DOWN2), (12, 4, BOTH))]
        rows += [R("inst_tail", "ZMarch", Z0, (8, 8), 12, bf, tails=FULL2), R("wide", "ZMarch", Z0, (12,), 20, bf), R("wide", "ZMarch", Z0, (12,), 48, bf)]
        rows += [R("sched", "ZMarch", s, (12,), 12, bf) for s in Z_SCHED]
        rows += [R("sched_down", "ZMarch", s, (12,), 12, bf, tails=DOWN1, store_main=(s != Z_SCHED_DOWN[1])) for s in Z_SCHED_DOWN]
    rows += [R("inst", "ZMarch", Z0, (4, 4), 12, True), R("inst_tail", "ZMarch", Z0, (4, 4), 4, True, tails=FULL1), R("inst_down", "ZMarch", Z0, (4, 4), 16, True, tails=BOTH),
             R("wide", "ZMarch", Z0, (4, 4), 20, False)]
    rows += [R("sched_down", "ZMarch", s, (4, 4), 12, True, tails=DOWN2) for s in Z_SCHED_DOWN[1:]]
    return rows


ZMARCH = zmarch_rows()
QUAD = [R("inst", "QuadRing", Z0, (4, 4), 12), R("inst_tail", "QuadRing", Z0, (4, 4), 4, tails=FULL4), R("inst_down", "QuadRing", Z0, (4, 4), 16, tails=BOTH),
        R("inst_tail", "QuadRing", Z0, (4, 4), 16, tails=FULL4 + FULL4, store_main=False)]
QUAD += [R("sched", "QuadRing", s, (4, 4), 12) for s in Z_SCHED[1:]] + [R("sched_down", "QuadRing", s, (4, 4), 12, tails=DOWN2) for s in Z_SCHED_DOWN[1:]]

BX = (1, 2, 64, 128)
BOX_GEOM = [(1, 2, 64, 128), (1, 2, 1024, 8), (1, 16, 1, 1024), (2, 5, 61, 57), (1, 33, 64, 8), (1, 3, 8, 683)]
BOX = [R("inst", "Box", BX, c, co, bf) for bf in (False, True) for c, co in (((8,), 12), ((8, 8), 16), ((8, 8), 24), ((8, 8), 40), ((16,), 12), ((16, 16), 12))]
BOX += [R("geom", "Box", s, c, co, bf) for s in BOX_GEOM[1:] for c, co, bf in (((8, 8), 24, False), ((16,), 8, True))]
BOX += [R("geom", "Box", s, (16, 16), 4, False) for s in BOX_GEOM[3:5]]

D1_GEOM = [(1, 1, 2, 16), (3, 1, 9, 33), (2, 1, 8, 32), (1, 1, 7, 31), (1, 1, 17, 65), (2, 1, 64, 208)]
SPLIT2D = [R("inst", "Split2d", D1_GEOM[1], c, 20) for c in ((4,), (8,), (12,), (16,), (4, 4), (8, 8))]
SPLIT2D += [R("geom", "Split2d", s, c, co) for s in D1_GEOM for c, co in (((8,), 4), ((4, 4), 48))]

FAMILIES = ("n01", "offset", "spread", "steps", "sparse")
FAM_BASE = [("ZMarch", (2, 9, 131, 227), (12,), 12, False), ("ZMarch", (2, 9, 131, 227), (12,), 12, True), ("QuadRing", (2, 9, 131, 227), (4, 4), 12, False),
            ("Box", (2, 5, 61, 57), (8, 8), 24, False), ("Box", (2, 5, 61, 57), (8, 8), 24, True), ("Split2d", (2, 1, 64, 208), (8,), 20, False)]
FAMILY_ROWS = [R("fam_" + fam, route, s, c, co, bf, fam=fam) for route, s, c, co, bf in FAM_BASE for fam in FAMILIES]
FAMILY_ROWS += [R("fam_offset", "Mfma", S2, (8,), 12, bf, "fp32", fam="offset") for bf in (False, True)]

# the bad element sits on a tile corner: the halo of the neighbouring tile, box or depth segment holds it
BAD_AT = [("Mfma", S2, (8,), 12, False, "fp32", (4, 8, 8)), ("ZMarch", (2, 9, 131, 227), (12,), 12, False, "f16x3", (5, 8, 32)),
          ("ZMarch", (2, 9, 131, 227), (12,), 12, True, "f16x3", (5, 8, 32)), ("QuadRing", (2, 9, 131, 227), (4, 4), 12, False, "f16x3", (5, 8, 32)),
          ("Box", (2, 5, 61, 57), (8, 8), 24, False, "f16x3", (2, 8, 16)), ("Box", (2, 5, 61, 57), (16,), 8, True, "f16x3", (2, 8, 16)),
          ("Split2d", (2, 1, 64, 208), (8,), 20, False, "f16x3", (0, 8, 32))]
BAD_VALUES = (float("inf"), NAN, 3e38)
NONFINITE = [R(f"bad_{v}_{'bnrelu' if act else 'plain'}", route, s, c, co, bf, prec, bn=act, relu=act, bad=(v, at))
             for route, s, c, co, bf, prec, at in BAD_AT for v in BAD_VALUES for act in (False, True)]

GATED = MFMA_MATRIX + MFMA_COUT + MFMA_DEFAULT + MFMA_GEOM + MFMA_EPI + ZMARCH + QUAD + BOX + SPLIT2D + FAMILY_ROWS
ALL_ROWS = GATED + NONFINITE

# the schedule classes the z-marching shapes were chosen for, (seg_len, nseg, split?, ngrp) under fp32 storage, 12 outputs
SCHED_CLASS = {(1, 8, 128, 256): (8, 1, True, 8), (2, 9, 131, 227): (5, 2, False, 8), (1, 13, 160, 128): (7, 2, True, 8), (1, 33, 90, 93): (7, 5, False, 1),
               (1, 8, 993, 33): (8, 1, None, None), (1, 64, 64, 64): (8, 8, None, 8)}
SCHED_CLASS_DOWN = {(1, 8, 128, 256): (8, 1, True, 8), (2, 10, 132, 200): (6, 2, False, None), (1, 14, 128, 160): (8, 2, False, 8), (1, 24, 64, 176): (None, None, True, 8),
                    (1, 8, 130, 254): (8, 1, True, 8)}


# --------------------------------------------------------------------------- inputs and float64 yardsticks
def gen(seed):
    return torch.Generator().manual_seed(seed)


def v5(t):
    return t.view(1, -1, 1, 1, 1)


def unit_index(route, D, H, W, tiles_only=False):
    """index of the plane (z-marching routes), box (Box) or tile (Split2d, and everyone under tiles_only) a voxel belongs to"""
    uz, uy, ux = {"Box": (2, 8, 16), "Split2d": (FAR, 8, 32)}.get(route, (FAR, 8, 32) if tiles_only else (1, FAR, FAR))
    z, y, x = torch.arange(D).view(-1, 1, 1) // uz, torch.arange(H).view(1, -1, 1) // uy, torch.arange(W).view(1, 1, -1) // ux
    return z + y + x


def base_key(r):
    return (r.route if r.fam in ("steps", "sparse") else "", r.shape, r.cins, r.cout, r.bf, r.fam, r.bad)


@functools.lru_cache(maxsize=3)
def base(route, shape, cins, cout, bf, fam, bad):
    """Inputs of a row and, per set, its float64 pre-activation, mag and block, computed once and shared (never modified)."""
    B, D, H, W = shape
    cin = sum(cins)
    g1 = gen(zlib.crc32(repr((route, shape, cins, cout, fam)).encode()) & 0x7fffffff)
    x = torch.randn((B, cin, D, H, W), generator=g1)
    ws = [torch.randn((cout, c, 3, 3, 3), generator=g1) * 0.1 for c in cins]
    if fam == "offset":
        x += 1000.0
        ws = [w - w.mean(dim=(1, 2, 3, 4), keepdim=True) for w in ws]
    elif fam == "spread":
        x *= torch.exp2(torch.rand(x.shape, generator=g1) * 40 - 20)
        ws = [w * torch.exp2(torch.rand(w.shape, generator=g1) * 40 - 20) for w in ws]
    elif fam == "steps":
        x *= torch.tensor([0.0, 1.0, 1e3, 1e7, 1e-3])[unit_index(route, D, H, W) % 5]
    elif fam == "sparse":
        x = x.abs() * (torch.rand(x.shape, generator=g1) > 0.7) * (unit_index(route, D, H, W, True) % 3 != 0)
        x[B - 1] = 0.0
    if bf:
        x = x.to(torch.bfloat16).float()
    c = {"ws": ws, "shape": shape, "cins": cins, "cout": cout, "bf": bf}
    c["scale"] = [(torch.rand(cout, generator=g1) + 0.5) * (1 - 2 * (torch.rand(cout, generator=g1) < 0.25).float()) for _ in cins]
    c["shift"] = [torch.randn(cout, generator=g1) * 0.1 for _ in cins]
    c["tw"] = [torch.randn((4, cout), generator=g1) * 0.3 for _ in range(4)]
    c["ts"] = [(torch.rand(4, generator=g1) + 0.5) * (1 - 2 * (torch.rand(4, generator=g1) < 0.25).float()) for _ in range(4)]
    c["th"] = [torch.randn(4, generator=g1) * 0.1 for _ in range(4)]
    c["res"] = torch.randn((B, cout, D, H, W), generator=g1)
    if bf:
        c["res"] = c["res"].to(torch.bfloat16).float()
    xr = x
    if bad is not None:
        val, (z, y, xx) = bad
        ind = torch.zeros((1, cins[0], D, H, W), dtype=torch.float64)
        ind[0, 1, z, y, xx] = 1.0
        c["touch"] = F.conv3d(ind, ws[0].double().abs(), padding=1)[0]            # > 0: the reach, in sample 1
        c["touch_signed"] = F.conv3d(ind, ws[0].double(), padding=1)[0]
        xr = x.clone()
        xr[1, 1, z, y, xx] = 0.0
        x = x.clone()
        x[1, 1, z, y, xx] = val
    c["x"] = x
    xmax = float(xr.abs().max())
    c["pre"], c["mag"], c["block"] = [], [], []
    c0 = 0
    for w, ci in zip(ws, cins):
        xs, w64 = xr[:, c0:c0 + ci].double(), w.double()
        c0 += ci
        c["pre"].append(F.conv3d(xs, w64, padding=1))
        c["mag"].append(F.conv3d(xs.abs(), w64.abs(), padding=1))
        sum_x = F.conv3d(xs.abs(), torch.ones((1, ci, 3, 3, 3), dtype=torch.float64), padding=1)
        c["block"].append(xmax * v5(w64.abs().flatten(1).sum(dim=1)) + v5(w64.abs().flatten(1).max(dim=1).values) * sum_x)
    c["xr"] = xr
    return c


def base_of(r):
    return base(*base_key(r))


def set_terms(c, r, s, split=None):
    """(act(u_s), b_s) of set s in float64"""
    split = (r.route != "Mfma") if split is None else split
    pre, mag = c["pre"][s], c["mag"][s]
    if not split:
        arith = 1e-6 * mag
    elif r.bf:
        arith = (E18 + 1e-6) * mag                       # exact bf16 activations x two bf16 halves of each weight (the docstring)
    else:
        arith = (E20 + 1e-6) * mag + E33 * c["block"][s]
    if r.bn:
        sc, sh = v5(c["scale"][s].double()), v5(c["shift"][s].double())
        u, b = pre * sc + sh, sc.abs() * arith + E23 * ((sc * pre).abs() + sh.abs())
    else:
        u, b = pre, arith
    return (F.relu(u) if r.relu else u), b


def gate_main(c, r, split=None, sets=None):
    """(ref, bound without the storage term) of the main output"""
    terms = [set_terms(c, r, s, split) for s in (range(len(r.cins)) if sets is None else sets)]
    ref, bound, size = sum(t[0] for t in terms), sum(t[1] for t in terms), sum(t[0].abs() for t in terms)
    if r.res:
        ref, size = ref + c["res"].double(), size + c["res"].double().abs()
    return ref, bound + E23 * size


def stored(r, ref, bound):
    return bound + E8 * ref.abs() if r.bf else bound


def mix(w, t):
    return torch.einsum("kc,bcdhw->bkdhw", w, t)


def tri(t, size):
    return F.interpolate(t, size=size, mode="trilinear", align_corners=True)


def gate_tail(c, r, i, main_ref, main_bound):
    """(ref, bound with the storage term) of tail i of the row"""
    k, down, tbn, trelu = r.tails[i]
    w = c["tw"][i][:k].double()
    prod = mix(w.abs(), main_ref.abs())
    if down:
        half = tuple(n // 2 for n in r.shape[1:])
        t = mix(w, tri(main_ref.float(), half).double())
        bt = tri(mix(w.abs(), main_bound), half) + 1e-6 * tri(prod, half) + E22 * F.max_pool3d(prod, 2)
    else:
        t, bt = mix(w, main_ref), mix(w.abs(), main_bound) + 1e-6 * prod
    if tbn:
        s, h = v5(c["ts"][i][:k].double()), v5(c["th"][i][:k].double())
        t, bt = s * t + h, s.abs() * bt + E23 * ((s * t).abs() + h.abs())
    t = F.relu(t) if trelu else t
    return t, stored(r, t, bt)


def check(tag, route, got, ref, bound, where=None):
    """every element (of `where`) finite and inside the bound; returns the worst err / bound"""
    g64 = got.detach().cpu().double()
    assert g64.shape == ref.shape, (tag, g64.shape, ref.shape)
    sel = torch.ones_like(ref, dtype=torch.bool) if where is None else where.expand_as(ref)
    assert torch.isfinite(g64[sel]).all(), (tag, route, "non-finite output")
    ratio = ((g64 - ref).abs() / bound.clamp_min(1e-300))[sel]
    k = int(ratio.argmax())
    err = float((g64 - ref).abs()[sel][k])
    print(f"K3 case={tag} route={route} worst={err:.3e}/{float(bound[sel][k]):.3e} = {float(ratio[k]):.3f}")
    assert float(ratio[k]) <= 1.0, (tag, route, float(ratio[k]))
    return float(ratio[k])


# --------------------------------------------------------------------------- CPU: the rows and the yardstick themselves
@pytest.fixture(scope="module")
def ops():
    import rag_amd
    rag_amd.load_library()
    return rag_amd.ops


def probe(ops, r):
    """(route, schedule) the library answers for the row; ragged dual rows are probed as 4 + 4 (the file's docstring)"""
    nset, (nt, nd) = len(r.cins), ntails(r)
    cin = sum(r.cins)
    if nset == 2 and (r.cins[0] != r.cins[1] or r.cins[0] % 4):
        assert r.prec == "fp32"
        cin = 8
    B, D, H, W = r.shape
    with ops.conv_precision(r.prec):
        return ops.conv3d_k3_route(cin, r.cout, B, D, H, W, nset, r.res is not None, nt, nd, torch.bfloat16 if r.bf else torch.float32)


def test_every_row_reaches_its_route_and_every_instantiation_is_covered(ops):
    seen = set()
    for r in ALL_ROWS:
        route, sched = probe(ops, r)
        assert route == r.route, (rid(r), route)
        B, D, H, W = r.shape
        if r.route == "Mfma":
            assert sched == (0, 0, 0, 0)
            cfg = choose_cfg(B, D, H, W, r.cout)
            log_tx, rows, groups = ops.conv3d_k3_plan(r.cout, B, D, H, W, len(r.cins))
            assert (log_tx, rows) == ((5, 4 if len(r.cins) == 1 else 2), (4, 2), (3, 1))[cfg], (rid(r), log_tx, rows)
            assert groups == [split_groups(cdiv(r.cout, 4))]
            if r.tag.startswith(("cell_cfg", "geom_cfg")):
                assert cfg == int(r.tag[8]), rid(r)
        elif r.route in ("ZMarch", "QuadRing"):
            assert sched == x3_schedule(B, D, H, W, r.cout, r.bf, ntails(r)[1]), (rid(r), sched)
        else:
            assert sched == (0, 0, 0, 0)
        if ntails(r)[1]:
            assert ops.down2_tail_supported(D, H, W), rid(r)
        seen.add(inst_key(r))
    assert seen >= ALL_KEYS, sorted(ALL_KEYS - seen, key=repr)
    # k3_route's order of precedence at its thresholds
    assert ops.conv3d_k3_route(12, 12, 1, 8, 128, 255)[0] == "Mfma" and ops.conv3d_k3_route(8, 8, 1, 2, 64, 127)[0] == "Mfma"
    assert ops.conv3d_k3_route(8, 8, 1, 8, 128, 256)[0] == "Box" and ops.conv3d_k3_route(8, 8, 1, 8, 128, 256, ntail=1)[0] == "ZMarch"
    assert ops.conv3d_k3_route(8, 8, 1, 1, 2, 16)[0] == "Split2d" and ops.conv3d_k3_route(8, 8, 1, 1, 2, 16, dtype=torch.bfloat16)[0] == "Mfma"
    with pytest.raises(RuntimeError):
        ops.conv3d_k3_route(12, 12, 1, 8, 128, 256, nset=2)


def test_zmarch_shapes_reach_their_schedule_classes(ops):
    """the classes of the row tables: segments, the cut into half items, the dealing in groups — None: not part of the class"""
    for table, nd in ((SCHED_CLASS, 0), (SCHED_CLASS_DOWN, 1)):
        for shape, (seg_len, nseg, cut, ngrp) in table.items():
            got = ops.conv3d_k3_route(12, 12, *shape, ndown=nd)[1]
            assert got == x3_schedule(*shape, 12, False, nd)
            for want, have in ((seg_len, got[0]), (nseg, got[1]), (cut, got[2] > 0), (ngrp, got[3])):
                assert want is None or want == have, (shape, nd, got)
    s = ops.conv3d_k3_route(12, 12, 1, 13, 160, 128)[1]
    assert 13 - (s[1] - 1) * s[0] == 6                                     # the last segment is shorter
    s = ops.conv3d_k3_route(12, 12, 1, 33, 90, 93)[1]
    assert 33 - (s[1] - 1) * s[0] == 5
    assert cdiv(33, 32) == 2 and 33 % 32 == 1                              # (1, 8, 993, 33): a one-column second tile


UNIQUE = list({base_key(r): r for r in GATED}.values())


@pytest.mark.parametrize("r", UNIQUE, ids=rid)
def test_yardstick_is_sound_on_every_row(r):
    """ATen's own fp32 convolution passes the fp32 gate on every row (the "spread" rows: the split gate they are held to, see the
    docstring); on N(0,1) rows mag > 0 everywhere and the gate is tight"""
    c = base_of(r)
    c0 = 0
    for s, ci in enumerate(r.cins):
        y32 = F.conv3d(c["xr"][:, c0:c0 + ci], c["ws"][s], padding=1).double()
        c0 += ci
        err = (y32 - c["pre"][s]).abs()
        if r.fam == "spread":
            assert r.route != "Mfma" and bool((err <= (E20 + 1e-6) * c["mag"][s] + E33 * c["block"][s]).all()), rid(r)
            assert bool((err <= 27 * ci * 2.0 ** -24 * c["mag"][s]).all())
        else:
            assert bool((err <= 1e-6 * c["mag"][s]).all()), rid(r)
    if r.fam == "n01":
        assert all(bool((m > 0).all()) for m in c["mag"])
        ref, bound = gate_main(c, r._replace(res=None, relu=False))
        assert float((bound / ref.abs().clamp_min(1e-300)).median()) < 1e-3


def test_gates_reject_a_wrong_kernel():
    """The split gate rejects a float64 convolution of operands rounded to fp16 (a kernel that lost its low halves); both gates
    reject a reference with one tap of one output channel zeroed."""
    for r in (R("sens", "ZMarch", (1, 8, 40, 48), (12,), 12, bn=True, relu=True), R("sens", "Mfma", (1, 8, 40, 48), (12,), 12, prec="fp32")):
        c = base_of(r)
        ref, bound = gate_main(c, r)
        sc, sh = v5(c["scale"][0].double()), v5(c["shift"][0].double())
        act = lambda pre: F.relu(pre * sc + sh)      # noqa: E731
        assert bool(((act(c["pre"][0]) - ref).abs() <= bound).all())
        half = F.conv3d(c["x"].half().double(), c["ws"][0].half().double(), padding=1)
        assert not bool(((act(half) - ref).abs() <= bound).all()), r.route
        w = c["ws"][0].double().clone()
        w[5, 7, 0, 2, 1] = 0.0
        out = act(F.conv3d(c["x"].double(), w, padding=1))
        assert not bool(((out - ref).abs() <= bound).all()), r.route
        assert bool(((out - ref).abs() <= bound)[:, [i for i in range(12) if i != 5]].all())


# --------------------------------------------------------------------------- GPU
def run(ops, c, r, dev=DEV):
    """Runs the row; returns (main or None, [tail outputs]) on the CPU after checking every channel no store may touch."""
    dt = torch.bfloat16 if r.bf else torch.float32
    B, D, H, W = r.shape
    cin, cout, nset = sum(r.cins), r.cout, len(r.cins)
    nan = lambda *shape: torch.full(shape, NAN, device=dev, dtype=dt)      # noqa: E731
    if r.slices:
        xb = nan(B, cin + 6, D, H, W)
        xb[:, 3:3 + cin] = c["x"].to(dev, dt)
        x = xb[:, 3:3 + cin]
    else:
        x = c["x"].to(dev, dt)
    ng = cdiv(cout, 4)
    gch = [8 * ((g + 1) % ng) for g in range(ng)] if r.perm else None      # every other group of the span stays unused
    span = 8 * ng - 4 if r.perm else cout
    buf = nan(B, span + 2 * GUARD, D, H, W)
    out = buf[:, GUARD:GUARD + span]
    dest = [GUARD + (gch[co // 4] if gch else 4 * (co // 4)) + co % 4 for co in range(cout)]
    res = rgch = None
    if r.res == "alias":
        buf[:, dest] = c["res"].to(dev, dt)
        res = out
    elif r.res == "other":
        rgch = [4 * (ng - 1 - g) + 2 for g in range(ng)]
        res = nan(B, 4 * ng + 4, D, H, W)
        res[:, [rgch[co // 4] + co % 4 for co in range(cout)]] = c["res"].to(dev, dt)
        if r.slices:
            res = res[:, 1:]
            rgch = [ch - 1 for ch in rgch]
    gpu = lambda t: t.to(dev).contiguous()      # noqa: E731
    tails, tbufs = [], []
    for i, (k, down, tbn, trelu) in enumerate(r.tails):
        dims = (D // 2, H // 2, W // 2) if down else (D, H, W)
        tb = nan(B, k + 2 * GUARD, *dims)
        tbufs.append(tb)
        tails.append(ops.Tail(gpu(c["tw"][i][:k]), gpu(c["ts"][i][:k]) if tbn else None, gpu(c["th"][i][:k]) if tbn else None, trelu, tb, GUARD, down=down))
    with ops.conv_precision(r.prec):
        packs = [ops.conv3d_k3_pack(gpu(w.flip(2, 3, 4).transpose(0, 1)) if r.transpose else gpu(w), transpose=r.transpose) for w in c["ws"]]
        bn = [(gpu(c["scale"][s]), gpu(c["shift"][s])) if r.bn else (None, None) for s in range(nset)]
        kw = dict(res=res, res_group_ch=rgch, tails=tails or None, store_main=r.store_main)
        if nset == 1:
            ops.conv3d_k3(x, packs[0], cout, bn[0][0], bn[0][1], r.relu, out, gch, **kw)
        else:
            ops.conv3d_k3_dual(x, r.cins[0], packs[0], bn[0][0], bn[0][1], packs[1], bn[1][0], bn[1][1], cout, r.relu, out, gch, **kw)
    if dev != "cpu":
        torch.cuda.synchronize()
    full = buf.cpu()
    untouched = [ch for ch in range(full.shape[1]) if ch not in dest or (not r.store_main and r.res != "alias")]
    assert bool(torch.isnan(full[:, untouched]).all()), (rid(r), "a store left the main destination")
    touts = []
    for (k, _d, _b, _r), tb in zip(r.tails, tbufs):
        t = tb.cpu()
        assert bool(torch.isnan(t[:, :GUARD]).all()) and bool(torch.isnan(t[:, GUARD + k:]).all()), (rid(r), "a tail wrote outside its channels")
        touts.append(t[:, GUARD:GUARD + k])
    return (full[:, dest] if r.store_main else None), touts


def run_and_check(ops, r, dev=DEV):
    c = base_of(r)
    main, touts = run(ops, c, r, dev)
    ref, bound = gate_main(c, r)
    worst = 0.0
    if main is not None:
        worst = check(rid(r), r.route, main, ref, stored(r, ref, bound))
    for i, t in enumerate(touts):
        tref, tbound = gate_tail(c, r, i, ref, bound)
        worst = max(worst, check(f"{rid(r)}:tail{i}{'down' if r.tails[i][1] else ''}_k{r.tails[i][0]}", r.route, t, tref, tbound))
    return worst


@pytest.fixture(scope="module")
def gops():
    import rag_amd
    rag_amd.load_library()
    return rag_amd.ops


@pytest.mark.gpu
@pytest.mark.parametrize("r", MFMA_MATRIX + MFMA_COUT + MFMA_DEFAULT, ids=rid)
def test_mfma_instantiation_matrix(gops, r):
    """every (storage, nset, cfg, G) cell, ragged and wide Cout, partial input chunks, and the default precision on ineligible shapes"""
    run_and_check(gops, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", MFMA_GEOM, ids=rid)
def test_mfma_geometry(gops, r):
    """D around the 4-plane tiles, H and W at 1 and around the tile sizes, and >= 4096 tiles per configuration"""
    run_and_check(gops, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", MFMA_EPI, ids=rid)
def test_mfma_epilogue_and_addressing(gops, r):
    run_and_check(gops, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ZMARCH + QUAD, ids=rid)
def test_zmarch_and_quadring(gops, r):
    """every instantiation of x3_launch / xq_launch, wide outputs over blockIdx.y, and the schedule classes with and without down-sampling tails"""
    run_and_check(gops, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", BOX, ids=rid)
def test_box(gops, r):
    run_and_check(gops, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", SPLIT2D, ids=rid)
def test_split2d(gops, r):
    run_and_check(gops, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", FAMILY_ROWS, ids=rid)
def test_conditioning_families(gops, r):
    """cancelling sums, element-wise and per-unit magnitude spreads (the scale choice and the restart), post-ReLU-like zeros: BN + ReLU on"""
    run_and_check(gops, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", NONFINITE, ids=rid)
def test_non_finite_inputs_stay_local(gops, r):
    c = base_of(r)
    main, _ = run(gops, c, r)
    val = r.bad[0]
    reach = torch.zeros(main.shape, dtype=torch.bool)
    reach[1] = c["touch"] > 0
    assert reach.any() and not reach[0].any() and reach.sum() < reach.numel() // 20
    ref, bound = gate_main(c, r)
    bound = stored(r, ref, bound)
    check(rid(r), r.route, torch.where(reach, torch.zeros_like(main), main), ref, bound, where=~reach)
    inside, fin = main[reach].double(), torch.isfinite(main[reach])
    if val == 3e38 and (r.route == "Mfma" or r.bf):
        # finite products (fp32 operands, or bf16 ones, which hold 3e38): a finite value inside the reach is the float64 result WITH
        # the element, inside the row's own gate with the element's share in mag and block
        assert len(r.cins) == 1
        v = float(torch.tensor(val).to(main.dtype))
        w64 = c["ws"][0].double().abs().flatten(1)
        c2 = dict(c, pre=[c["pre"][0].clone()], mag=[c["mag"][0].clone()], block=[c["block"][0] + v * v5(w64.sum(dim=1) + w64.max(dim=1).values)])
        c2["pre"][0][1] += v * c["touch_signed"]
        c2["mag"][0][1] += v * c["touch"]
        want, wb = gate_main(c2, r)
        wb = stored(r, want, wb)
        assert bool(((inside - want[reach]).abs() <= wb[reach])[fin].all()), (rid(r), "a finite wrong value inside the reach")
    elif not r.relu:
        assert not fin.any(), (rid(r), "a non-finite input left a finite output inside its reach")
    elif len(r.cins) == 1:
        assert bool((main[reach][fin] == 0).all()) and not bool(torch.signbit(main[reach][fin]).any()), (rid(r), "a finite value other than +0 inside the reach")
    else:
        other, ob = gate_main(c, r, sets=(1,))
        ob = stored(r, other, ob)
        assert bool(((inside - other[reach]).abs() <= ob[reach])[fin].all()), (rid(r), "a finite value other than act(u_B) inside the reach")
