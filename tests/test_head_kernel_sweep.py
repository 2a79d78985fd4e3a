"""Sweep of the kernels that end the Matching-Net (the head) against float64, through rag_amd.ops only:
    small    ops.conv3d_k3_small          conv3d_k3_kernel<.., VALU> (conv3d.hip, conv3d_k3_inst_valu_*.hip): 3 tile configurations x Cout {1, 2} x
                                          {f32, bf16, bf16 -> f32}, and conv3d_c1_kernel (conv3d_c1.hip) in its three dtype pairs
    upconv   ops.upconv3d_c1              upconv3d_c1_kernel in its three dtype pairs
    uptaps   ops.uptaps3d                 uptaps3d_kernel<false> (from P) and <true> (from Q, xblended=True)
    k1       ops.trilinear3d_act_k1       trilinear_up_k1_kernel<28, false>, <32, false> and <28, true> (xblend=True)

References are float64 over the values the kernel reads (bf16-rounded under bf16 storage).  Interpolation indices and lambdas are
the fp32 rule of csrc/common.h lin_index restated in lin_tables (tests/test_head_xblend.py lin_twin, generalised to
align_corners=False and any sizes); everything after the tables is float64.  conv27 is the 3x3x3 convolution as 27 shifted
multiply-adds in plain torch ops: rows of 2^18 voxels or more take it on the device in float64
(test_conv27_is_conv3d holds it to F.conv3d on the CPU).

Gates, per element, nothing excused (E24 = 2^-24, E23 = 2^-23, E8 = 2^-8; mag = sum |w| * |operand|; A = the interpolation of |x| with
the same weights; conv(., |w|) = conv27 with |w|):
    small (VALU and c1)     (27 Cin + 1) * E24 * mag                                    one fmaf chain over Cin * 27 products
    upconv                  conv(3 * E23 * A, |w|) + (27 Cin + 1) * E24 * conv(A, |w|)
    k1                      (3 * E23 + (C + 1) * E24) * mix(|w|, A)                     include/rag_amd.h "resample + 1x1x1"
    uptaps (from P)         25 * E24 * M,   M = sum_t shift_t(U(|P_t|))
    uptaps (from Q)         16 * E24 * MQ,  MQ = sum_g shift_g(Uyz(|Q_g|))
    k1 (xblend) -> Q        (3 * E23 + (C + 1) * E24 + 9 * E24) * sum_dx shift_dx(Ux(mix(|w|, A)))
    tap pair k1 -> uptaps   sum_t shift_t(U(b_P)) + 25 * E24 * sum_t shift_t(U(mix(|w_t|, A))),   b_P the k1 bound
    folded BN               |scale| * arith + E23 * (|scale * pre| + |shift|); ReLU leaves a bound unchanged
    residual (small)        + E23 * (|act(u)| + |res|)
    bf16 storage            + E8 * |ref|
Derivation for uptaps3d_kernel (conv3d_c1.hip), checked against the code: the x stage forms Q[i] from three dx volumes of up to
three window slots each — the first term a product, every later one an fmaf: at most 9 roundings.  The y stage adds wy * Q to
R[p][ro] once per (dy, slot) that is not skipped: 2 + 3 + 3 = 8 fmaf at most (<= 9).  The z stage adds wk * R to acc for the two
non-zero plane weights of each dz: 6.  The epilogue is one fmaf (exact without scale / shift).  A product passes through at most
9 + 9 + 6 = 24 roundings of sums no larger than M; 25 covers the second-order terms.  A zero-weight fmaf leaves a finite sum
unchanged.  From Q the x stage is gone: 9 + 6 + 1 = 16.  The producer of Q adds the 9-term x chain to the k1 bound of P.

Unreached branches.  upconv3d_c1_kernel and uptaps3d_kernel carry code for "a source pair that starts one lower than the x2
pattern (the last output of an axis in fp32)": ylow, xlow, row0_dy2 and the shifted wz.  test_x2_pattern_is_exact asserts on the
CPU that for every axis length 2..4096 and EVERY output index X of the x2 align_corners=True resample i0 == max((X - 1) // 2, 0)
under the fp32 rule: no input shape reaches those branches, and no row here tries to.

Rows are the smallest shapes that reach their class; test_every_row_reaches_its_class asserts the class of every row through
ops.conv3d_k3_small_route (0 = conv3d_c1, 1 + cfg = VALU) and the *_supported predicates, and that every instantiation above is
named by a GPU row.  Two cases the plan asked for cannot exist and are asserted as such: a VALU row with W one past the x-tile on
tile configurations 0 and 1 (choose_cfg sends W = 33 and W = 17 to configuration 2; the rows use the narrowest second tile it
allows, W = 49 and W = 25), and xblend rows with an odd Wo (the entry point needs Wo == 2 Wi; 31 and 61 are refused).

Non-finite inputs: one Inf or NaN on a tile-corner voxel of channel 1 of sample 1; the reference is taken with the element zeroed.
Without ReLU the non-finite outputs are exactly the reach (the outputs whose tap index sets hold the element, whatever the
weights) and everything else keeps its gate.  With ReLU every value in the reach is non-finite or exactly +0.  One departure,
forced by arithmetic: trilinear_up_k1_kernel applies its ReLU BEFORE the mix, so a NaN (or 0 * Inf) sample becomes 0 and the
output is the mix of the other channels — a finite value in the reach must be the reference without that channel, within the gate.

Mutants (test_gates_reject_*, CPU): a dropped tap, a dropped input channel, replicate padding at a volume face, a halo column taken
from the clamped neighbour at a tile edge, dz and dx swapped, and lambdas from the exact source index around index 400 on an
`offset` row each fail the gate on the affected elements and pass elsewhere.

`offset` rows: the exact-lambda mutant is rejected on 2 of the 308 outputs past source index 256 (on N(0, 1) data on 293 of them):
with A = 100 the gate is a hundred times wider than the data's differences, and no sound gate sees more of it.

Every GPU row prints `HEAD case=... kernel=... worst=err/bound`.  Measured on the MI355X, worst err / bound (records, not gates;
families in the order n01 / offset / nonneg / sparse):
    small, VALU form   fp32 storage: tile configuration 0 / 1 / 2 0.052 / 0.047 / 0.038; bf16 storage 0.993 / 0.990 / 0.982;
                       families (12 -> 2, BN + ReLU + residual) 0.010 / 0.003 / 0.012 / 0.421; non-finite 0.041
    small, conv3d_c1   fp32 rows 0.063, bf16 -> bf16 0.985; families 0.050 / 0.017 / 0.038 / 0.039; non-finite 0.050
    upconv3d_c1        fp32 rows 0.087, bf16 -> bf16 0.942; families 0.008 / 0.006 / 0.009 / 0.246; non-finite 0.018
    k1                 <28> rows 0.234, <32> rows 0.275; families 0.107 / 0.088 / 0.214 / 0.213; non-finite 0.147
    k1 (xblend)        rows 0.073; families 0.051 / 0.033 / 0.085 / 0.115; non-finite 0.051
    uptaps3d (from P)  rows 0.056, single taps 0.121; families 0.054 / 0.013 / 0.121 / 0.238; non-finite 0.054
    uptaps3d (from Q)  rows 0.139, single rows 0.162; families 0.125 / 0.036 / 0.196 / 0.452; non-finite 0.128
    tap pair           0.010 on every shape, and the x-blended pair has the plain pair's bits on all six
The bf16 -> bf16 rows sit just under 1 by construction (round to nearest moves a value by up to 2^-8 of itself: the storage term);
the fp32 rows are the arithmetic underneath.  No gate was taken from these numbers and none departs from the list above.

The kernel change this file forced.  uptaps3d_kernel blended over fixed windows — three slots per upsampled column and row where
the x2 pattern uses two, and the convolution's zero padding as zero weights over clamped loads — and multiplied the unused slot by
a weight of 0: 0 * Inf is NaN, so a non-finite P (Q) value also reached outputs whose windows held it without reading it.
test_uptaps_non_finite measured, with the element at (1, 31, 15) of tap volume 1 of sample 1 on 3 x 33 x 18, 32 non-finite outputs
beyond a reach of 80 from P and 4 beyond 20 from Q (behind BN + ReLU: +0 at 1.9e5 and 3.1e5 times the gate).  The kernel now
multiplies a slot only where it belongs to the source pair (i0, i1) — whatever its weight, as ATen does — and takes the terms of
halo rows and columns outside the volume back; all eight rows pass and finite results keep their values (profiles/head_nonfinite_ab.md).
Unmarked tests run without a GPU; the rest need the MI355X."""
import collections
import functools
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
E8, E23, E24 = 2.0 ** -8, 2.0 ** -23, 2.0 ** -24
NAN, INF = float("nan"), float("inf")
GUARD = 2
F64 = torch.float64
BIG = 1 << 18
FAMILIES = ("n01", "offset", "nonneg", "sparse")
PAIRS = {"f32": (torch.float32, torch.float32), "bf16": (torch.bfloat16, torch.bfloat16), "bf16_f32": (torch.bfloat16, torch.float32)}


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def cdiv(a, b):
    return -(-a // b)


def prod(s):
    n = 1
    for v in s:
        n *= v
    return n


def x2(s):
    return tuple(2 * v for v in s)


# --------------------------------------------------------------------------- the fp32 index rule and the float64 references
def lin_tables(n_in, n_out, align):
    """(i0, i1, w0, w1) per output index: lin_index of csrc/common.h (ATen's fp32 rule).  align_corners: src = fl32(scale * dst);
    otherwise src = fl32(scale * (dst + 0.5) - 0.5) in ONE rounding, clamped at 0; i0 = min(int(src), n - 1), i1 = min(i0 + 1, n - 1),
    lambda = fl32(src - i0) clamped to [0, 1], w0 = fl32(1 - lambda); equal sizes: the identity."""
    dst = torch.arange(n_out)
    if n_in == n_out:
        return dst, dst.clone(), torch.ones(n_out, dtype=F64), torch.zeros(n_out, dtype=F64)
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)      # noqa: E731
    if align:
        scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
        src = scale * dst.float()
    else:
        scale = f32(n_in) / f32(n_out)
        src = (scale.double() * (dst.double() + 0.5) - 0.5).clamp_min(0).float()      # exact in float64: one rounding
    i0 = src.long().clamp_max(n_in - 1)
    lam = (src - i0.float()).clamp(0, 1)
    return i0, (i0 + 1).clamp_max(n_in - 1), (1 - lam).double(), lam.double()


def exact_tables(n_in, n_out):
    """the mutant: align_corners=True lambdas from the exact (float64) source index"""
    dst = torch.arange(n_out).double()
    src = dst * (n_in - 1) / (n_out - 1)
    i0 = src.long().clamp_max(n_in - 1)
    lam = (src - i0.double()).clamp(0, 1)
    return i0, (i0 + 1).clamp_max(n_in - 1), 1 - lam, lam


def tables(in_size, size, align=True):
    return [lin_tables(a, b, align) for a, b in zip(in_size, size)]


def ident(n):
    return lin_tables(n, n, True)


def interp(x, tabs):
    """interpolation of x[B, C, D, H, W] along x, y, z with the given tables, in x's dtype on x's device"""
    for dim, (i0, i1, w0, w1) in zip((4, 3, 2), reversed(tabs)):
        shape = [1] * x.dim()
        shape[dim] = -1
        i0, i1 = i0.to(x.device), i1.to(x.device)
        x = x.index_select(dim, i0) * w0.to(x.device, x.dtype).view(shape) + x.index_select(dim, i1) * w1.to(x.device, x.dtype).view(shape)
    return x


def tap_reach(ind, tabs):
    """1.0 on the outputs whose tap index set holds a marked input element, whatever the weights"""
    return (interp(ind, [(i0, i1, torch.ones_like(w0), torch.ones_like(w1)) for i0, i1, w0, w1 in tabs]) > 0).to(ind.dtype)


def conv27(x, w, replicate=False):
    """F.conv3d(x, w, padding=1) as 27 shifted multiply-adds in x's dtype on x's device (replicate: the padding of a mutant)"""
    B, C, D, H, W = x.shape
    xp = F.pad(x, (1,) * 6, mode="replicate") if replicate else F.pad(x, (1,) * 6)
    w = w.to(x.device, x.dtype)
    out = torch.zeros((B, w.shape[0], D, H, W), dtype=x.dtype, device=x.device)
    for t in range(27):
        dz, dy, dx = t // 9, t // 3 % 3, t % 3
        out += torch.einsum("oc,bcdhw->bodhw", w[:, :, dz, dy, dx], xp[:, :, dz:dz + D, dy:dy + H, dx:dx + W])
    return out


def tapsum(up):
    """sum_t shift_t(pad(up[:, t])): up [B, 27, D, H, W] with t = dz*9 + dy*3 + dx, or [B, 9, D, H, W] with g = dz*3 + dy (no x shift)"""
    B, T, D, H, W = up.shape
    pad = F.pad(up, (1, 1, 1, 1, 1, 1) if T == 27 else (0, 0, 1, 1, 1, 1))
    out = torch.zeros((B, 1, D, H, W), dtype=up.dtype, device=up.device)
    for t in range(T):
        dz, dy, dx = (t // 9, t // 3 % 3, t % 3) if T == 27 else (t // 3, t % 3, 0)
        out[:, 0] += pad[:, t, dz:dz + D, dy:dy + H, dx:dx + W]
    return out


def qblend(p, tx):
    """Q[g](.., gx) = sum_dx Ux(P[3g + dx])(gx + dx - 1), zero outside the row: p [B, 27, D, H, W] -> [B, 9, D, H, 2 W]"""
    B, T, D, H, W = p.shape
    up = F.pad(interp(p, [ident(D), ident(H), tx]), (1, 1))
    q = torch.zeros((B, 9, D, H, 2 * W), dtype=p.dtype, device=p.device)
    for t in range(27):
        q[:, t // 3] += up[:, t, :, :, t % 3:t % 3 + 2 * W]
    return q


def mix(w, x):
    return torch.einsum("oc,bc...->bo...", w.to(x.device, x.dtype), x)


def vb(t, like):
    return t.to(like.device, F64).view([1, -1] + [1] * (like.dim() - 2))


def bn_act(pre, arith, bn, relu):
    if bn is not None:
        sc, sh = vb(bn[0], pre), vb(bn[1], pre)
        u, b = pre * sc + sh, sc.abs() * arith + E23 * ((sc * pre).abs() + sh.abs())
    else:
        u, b = pre, arith
    return (F.relu(u) if relu else u), b


def stored(bf, ref, bound):
    return bound + E8 * ref.abs() if bf else bound


def check(tag, kernel, got, ref, bound, where=None):
    """every element (of `where`) finite and inside the bound, on the reference's device; returns the worst err / bound"""
    g64 = got.detach().to(ref.device).double()
    assert g64.shape == ref.shape, (tag, g64.shape, ref.shape)
    sel = torch.ones_like(ref, dtype=torch.bool) if where is None else where.to(ref.device).expand_as(ref)
    assert torch.isfinite(g64[sel]).all(), (tag, kernel, "non-finite output")
    err = (g64 - ref).abs()
    ratio = (err / bound.clamp_min(1e-300))[sel]
    k = int(ratio.argmax())
    print(f"HEAD case={tag} kernel={kernel} worst={float(err[sel][k]):.3e}/{float(bound[sel][k]):.3e} = {float(ratio[k]):.3f}")
    assert float(ratio[k]) <= 1.0, (tag, kernel, float(ratio[k]))
    return float(ratio[k])


def inside(got, ref, bound):
    return (got.double() - ref).abs() <= bound


def check_reach(tag, kernel, got, reach, ref, bound, relu):
    """the non-finite rule of the docstring; ref / bound: the reference with the element zeroed"""
    got = got.detach().cpu()
    ref, bound, reach = ref.cpu(), bound.cpu(), reach.cpu().expand_as(got)
    assert reach.any() and not reach[0].any() and reach.sum() <= reach.numel() // 8, (tag, int(reach.sum()))
    leak = ~torch.isfinite(got) & ~reach
    print(f"HEAD case={tag} kernel={kernel} reach={int(reach.sum())} non-finite outside the reach={int(leak.sum())}")
    assert not leak.any(), (tag, kernel, f"{int(leak.sum())} non-finite outputs outside the reach of {int(reach.sum())}")
    check(tag, kernel, torch.where(reach, torch.zeros_like(got), got), ref, bound, where=~reach)
    fin = torch.isfinite(got[reach])
    if not relu:
        assert not fin.any(), (tag, kernel, f"{int(fin.sum())} finite outputs inside the reach of a non-finite input")
    else:
        v = got[reach][fin]
        assert bool((v == 0).all()) and not bool(torch.signbit(v).any()), (tag, kernel, "a finite value other than +0 inside the reach")


# --------------------------------------------------------------------------- inputs
def make_x(shape, fam, g, unit=256):
    """[B, C, *spatial] of a conditioning family; the units of "sparse" are runs of `unit` voxels"""
    x = torch.randn(shape, generator=g)
    if fam == "offset":
        x += 100.0
    elif fam == "nonneg":
        x = F.relu(x)
    elif fam == "sparse":
        idx = (torch.arange(prod(shape[2:])) // unit).view(shape[2:])
        x = x.abs() * (torch.rand(x.shape, generator=g) > 0.7) * (idx % 3 != 0)
        x[shape[0] - 1] = 0.0
    return x


def make_bn(c, g):
    return (torch.rand(c, generator=g) + 0.5) * (1 - 2 * (torch.rand(c, generator=g) < 0.25).float()), torch.randn(c, generator=g) * 0.1


def rnd(x, bf):
    return x.to(torch.bfloat16).float() if bf else x


def poison(x, bad, ch=1):
    """(x with the element, x with it zeroed); bad = (value, spatial index) in channel `ch` of sample 1"""
    if bad is None:
        return x, x
    val, at = bad
    xz, xv = x.clone(), x.clone()
    xz[(1, ch) + tuple(at)] = 0.0
    xv[(1, ch) + tuple(at)] = val
    return xv, xz


def indicator(shape, bad, ch=1):
    ind = torch.zeros(shape, dtype=F64)
    ind[(1, ch) + tuple(bad[1])] = 1.0
    return ind


def ref_dev(nvox):
    return DEV if nvox >= BIG and torch.cuda.is_available() else "cpu"


# =========================================================================== conv3d_k3_small: the VALU form and conv3d_c1
S = collections.namedtuple("S", "tag route shape cin cout pair bn relu res bview misalign fam bad")


def s(tag, route, shape, cin, cout, pair="f32", bn=False, relu=False, res=False, bview=False, misalign=False, fam="n01", bad=None):
    return S(tag, route, tuple(shape), cin, cout, pair, bn, relu, res, bview, misalign, fam, bad)


def s_id(r):
    return "{}-{}_{}_c{}o{}_{}".format("c1" if r.route == 0 else f"valu{r.route - 1}", r.tag, "x".join(map(str, r.shape)), r.cin, r.cout, r.pair)


def choose_cfg(B, D, H, W):
    """choose_cfg of rag_amd/csrc/conv3d.hip for Cout <= 2 (checked against the probe)"""
    vol = B * D * H * W
    waste = lambda tx: cdiv(W, tx) * tx / W      # noqa: E731
    if W > 16 and waste(32) <= waste(16) + 1e-9 and vol >= 1 << 20:
        return 0
    if W > 8 and waste(16) <= waste(8) + 1e-9 and vol >= 1 << 17:
        return 1
    return 2


# tiles of the VALU form: TX x 8 x 4 with TX = 32, 16, 8.  Per configuration: a partial tile on every axis, and the narrowest second
# x-tile choose_cfg allows (the docstring).  Configuration 0 needs B*D*H*W >= 2^20; Cout = 1 stays off conv3d_c1 there through
# W % 4 != 0, a residual, or a batch of samples under 2^18 voxels each
V_PART = {2: (2, 5, 11, 13), 1: (1, 5, 105, 250), 0: (1, 5, 950, 221)}
V_PAST = {2: (2, 5, 9, 9), 1: (1, 4, 1312, 25), 0: (1, 4, 5352, 49)}


def valu_rows():
    rows = []
    for cfg in (2, 1, 0):
        for i, (cout, pair) in enumerate((co, p) for co in (1, 2) for p in PAIRS):
            rows.append(s("part", 1 + cfg, V_PART[cfg], 4, cout, pair, bn=i % 2 == 0, relu=i % 3 == 0, res=i % 2 == 1))
        rows += [s("past", 1 + cfg, V_PAST[cfg], 4, 1, "f32", res=True), s("past", 1 + cfg, V_PAST[cfg], 4, 2, "bf16_f32", bn=True, relu=True)]
    rows += [s("cin12", 3, V_PART[2], 12, 2, "f32", bn=True, res=True), s("cin12", 2, V_PART[1], 12, 1, "bf16", bn=True, relu=True),
             s("cin68_abi", 3, (1, 3, 7, 9), 68, 2, "f32"), s("cin128_lds_limit", 3, (1, 3, 7, 9), 128, 2, "f32"),
             s("c1shape_res", 1, (1, 4, 128, 2048), 4, 1, "f32", res=True), s("c1shape_batch", 1, (5, 4, 208, 256), 4, 1, "bf16_f32", bn=True),
             s("c1shape_misaligned_out", 2, (1, 4, 256, 256), 4, 1, "f32", misalign=True)]
    return rows


VALU = valu_rows()
C1 = [s("exact", 0, (1, 4, 256, 256), 4, 1), s("depth1", 0, (1, 1, 512, 512), 4, 1, bn=True, relu=True),
      s("ragged", 0, (1, 5, 228, 232), 12, 1, "bf16_f32", bn=True), s("past_nwork116", 0, (1, 113, 65, 36), 4, 1),
      s("w4", 0, (1, 16, 4096, 4), 4, 1, "bf16", bn=True, relu=True), s("cin64", 0, (1, 4, 256, 256), 64, 1, "bf16"),
      s("cin12", 0, (1, 4, 256, 256), 12, 1, "f32", relu=True), s("batch_view", 0, (2, 5, 228, 232), 4, 1, "f32", bn=True, bview=True)]
S_FAM = [s("fam_" + f, 3, (2, 9, 19, 21), 12, 2, "f32", bn=True, relu=True, res=True, fam=f) for f in FAMILIES]
S_FAM += [s("fam_" + f, 0, (2, 5, 228, 232), 4, 1, "f32", bn=True, fam=f) for f in FAMILIES]
# the bad voxel is the last one of the first tile: the halos of its seven neighbours hold it
S_BAD = [s(f"bad_{v}", 3, (2, 9, 19, 21), 4, 2, "f32", bn=a, relu=a, bad=(v, (3, 7, 7))) for v in (INF, NAN) for a in (False, True)]
S_BAD += [s(f"bad_{v}", 0, (2, 5, 228, 232), 4, 1, "f32", bn=a, relu=a, bad=(v, (3, 63, 31))) for v in (INF, NAN) for a in (False, True)]
S_ROWS = VALU + C1 + S_FAM


class Box(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=2)
def s_base(shape, cin, bf, fam, bad, dev):
    """inputs of a small-route row and the float64 pre-activation and mag of BOTH output channels (a Cout = 1 row reads the first)"""
    B, D, H, W = shape
    g = gen("small", shape, cin, fam)
    x = rnd(make_x((B, cin, D, H, W), fam, g), bf)
    w = torch.randn((2, cin, 3, 3, 3), generator=g) * 0.1
    if fam == "offset":
        w -= w.mean(dim=(1, 2, 3, 4), keepdim=True)
    c = Box(w=w, bn=make_bn(2, g), res=rnd(torch.randn((B, 2, D, H, W), generator=g), bf))
    c.x, xz = poison(x, bad)
    x64 = xz.to(dev).double()
    c.xz, c.pre, c.mag = xz, conv27(x64, w.double()), conv27(x64.abs(), w.double().abs())
    if bad is not None:
        c.reach = (conv27(indicator((2, cin, D, H, W), bad), torch.ones((1, cin, 3, 3, 3), dtype=F64)) > 0)
        c.reach = torch.cat([c.reach] + [torch.zeros_like(c.reach[:1])] * (B - 2)) if B > 2 else c.reach
    return c


def s_base_of(r, dev=None):
    return s_base(r.shape, r.cin, r.pair != "f32", r.fam, r.bad, dev or ref_dev(prod(r.shape)))


def s_gate(r, c):
    """(ref, bound with storage) of a small-route row"""
    pre, mag = c.pre[:, :r.cout], c.mag[:, :r.cout]
    ref, b = bn_act(pre, (27 * r.cin + 1) * E24 * mag, (c.bn[0][:r.cout], c.bn[1][:r.cout]) if r.bn else None, r.relu)
    if r.res:
        res = c.res[:, :r.cout].to(pre.device).double()
        ref, b = ref + res, b + E23 * (ref.abs() + res.abs())
    return ref, stored(r.pair == "bf16", ref, b)


def s_probe(ops, r):
    B, D, H, W = r.shape
    xdt, ydt = PAIRS[r.pair]
    dhw = D * H * W
    return ops.conv3d_k3_small_route(r.cin, r.cout, B, D, H, W, xdt, ydt, r.res, (r.cin + 4 if r.bview else r.cin) * dhw,
                                     (r.cout + 2 * GUARD) * dhw, True, not r.misalign)


# =========================================================================== upconv3d_c1 and uptaps3d: input sizes (Di, Hi, Wi)
# (2,2,2): every voxel a border, nwork 1 < 8; Hi 31 / 32 / 33 and Wi 14 / 16 / 18: one short of, at and one pair past the 64 x 32 tile;
# Di 3 and 5: a ragged 2-plane last segment; (5,33,18): 2 x 2 tiles x 3 segments = 12 work items, not a multiple of 8; B = 2
HEAD_SHAPES = [(1, (2, 2, 2)), (1, (3, 31, 14)), (2, (2, 32, 16)), (1, (5, 33, 18)), (2, (3, 33, 18))]
MULTI = (2, (3, 33, 18))

U = collections.namedtuple("U", "tag B in_size cin pair bn relu sl fam bad")


def u(tag, B, in_size, cin, pair="f32", bn=False, relu=False, sl=False, fam="n01", bad=None):
    return U(tag, B, tuple(in_size), cin, pair, bn, relu, sl, fam, bad)


def u_id(r):
    return "{}_b{}_{}_c{}_{}".format(r.tag, r.B, "x".join(map(str, r.in_size)), r.cin, r.pair)


U_ROWS = [u("shape", B, sz, cin, pair, bn=i % 2 == 1, relu=i % 2 == 1, sl=i % 2 == 0)
          for i, ((B, sz), cin, pair) in enumerate(zip(HEAD_SHAPES, (12, 5, 1, 12, 12), ("f32", "bf16_f32", "f32", "bf16", "f32")))]
U_ROWS += [u("cin64", 1, (2, 5, 6), 64, "bf16", bn=True), u("cin64", 1, (3, 33, 18), 64, "f32", relu=True, sl=True), u("cin1", 2, (3, 33, 18), 1, "bf16_f32", bn=True, relu=True),
           u("cin5", 1, (5, 33, 18), 5, "f32", sl=True)]
U_FAM = [u("fam_" + f, *MULTI, 12, "f32", bn=True, fam=f) for f in FAMILIES]
U_BAD = [u(f"bad_{v}", *MULTI, 5, "f32", bn=a, relu=a, bad=(v, (1, 31, 15))) for v in (INF, NAN) for a in (False, True)]


@functools.lru_cache(maxsize=2)
def u_base(B, in_size, cin, bf, fam, bad):
    g = gen("upconv", B, in_size, cin, fam)
    x = rnd(make_x((B, cin) + in_size, fam, g, unit=64), bf)
    w = torch.randn((1, cin, 3, 3, 3), generator=g) * 0.1
    if fam == "offset" and cin > 1:
        w -= w.mean()
    c = Box(w=w, bn=make_bn(1, g), tabs=tables(in_size, x2(in_size)))
    c.x, xz = poison(x, bad)
    c.xz = xz
    w64 = w.double()
    c.pre = conv27(interp(xz.double(), c.tabs), w64)
    c.amag = conv27(interp(xz.double().abs(), c.tabs), w64.abs())
    if bad is not None:
        c.reach = conv27(tap_reach(indicator((B, cin) + in_size, bad), c.tabs), torch.ones((1, cin, 3, 3, 3), dtype=F64)) > 0
    return c


def u_base_of(r):
    return u_base(r.B, r.in_size, r.cin, r.pair != "f32", r.fam, r.bad)


def u_gate(r, c):
    ref, b = bn_act(c.pre, (3 * E23 + (27 * r.cin + 1) * E24) * c.amag, c.bn if r.bn else None, r.relu)
    return ref, stored(r.pair == "bf16", ref, b)


T = collections.namedtuple("T", "tag B in_size xb bn relu fam bad only")


def t(tag, B, in_size, xb, bn=False, relu=False, fam="n01", bad=None, only=None):
    return T(tag, B, tuple(in_size), xb, bn, relu, fam, bad, only)


def t_id(r):
    return "{}{}_b{}_{}".format("xb_" if r.xb else "", r.tag, r.B, "x".join(map(str, r.in_size))) + ("" if r.only is None else f"_tap{r.only}")


T_ROWS = [t("shape", B, sz, xb, bn=act, relu=act) for B, sz in HEAD_SHAPES for xb in (False, True) for act in (False, True)]
# test_head_taps' single-tap rows on every tap: P (Q) is zero but for one tap volume, on two y-tiles; M is zero where the shifted
# upsample of that volume is not, so the gate is `exactly 0` there
T_SINGLE = [t("single", 1, (3, 33, 8), False, only=k) for k in range(27)] + [t("single", 1, (3, 33, 8), True, only=k) for k in range(9)]
T_FAM = [t("fam_" + f, *MULTI, xb, bn=True, fam=f) for xb in (False, True) for f in FAMILIES]
T_BAD = [t(f"bad_{v}", *MULTI, xb, bn=a, relu=a, bad=(v, (1, 31, 15))) for xb in (False, True) for v in (INF, NAN) for a in (False, True)]


@functools.lru_cache(maxsize=2)
def t_base(B, in_size, xb, fam, bad, only):
    """p: P [B, 27, Di, Hi, Wi], or Q [B, 9, Di, Hi, 2 Wi] taken as data (the consumer's contract does not depend on where Q came from)"""
    Di, Hi, Wi = in_size
    g = gen("uptaps", B, in_size, xb, fam)
    nt, shape = (9, (Di, Hi, 2 * Wi)) if xb else (27, in_size)
    p = make_x((B, nt) + shape, fam, g, unit=64) * (2.0 / 27) ** 0.5
    if fam == "offset":
        p[:, 1::2] *= -1.0                      # 13 (4) of the 27 (9) volumes negative: the tap sum cancels
    if only is not None:
        keep = p[:, only].clone()
        p.zero_()
        p[:, only] = keep
    c = Box(bn=make_bn(1, g))
    c.p, pz = poison(p, bad)
    tz, ty, tx = tables(in_size, x2(in_size))
    tabs = [tz, ty, ident(2 * Wi)] if xb else [tz, ty, tx]
    c.pre, c.m = tapsum(interp(pz.double(), tabs)), tapsum(interp(pz.double().abs(), tabs))
    if bad is not None:
        c.reach = tapsum(tap_reach(indicator((B, nt) + shape, bad), tabs)) > 0
    return c


def t_base_of(r):
    return t_base(r.B, r.in_size, r.xb, r.fam, r.bad, r.only)


def t_gate(r, c):
    return bn_act(c.pre, (16 if r.xb else 25) * E24 * c.m, c.bn if r.bn else None, r.relu)


# =========================================================================== trilinear3d_act_k1 (and its xblend form)
K = collections.namedtuple("K", "tag B C cout in_size size align relu tr xb sl fam bad")


def k(tag, B, C, cout, in_size, size, align=True, relu=True, tr=False, xb=False, sl=False, fam="n01", bad=None):
    return K(tag, B, C, cout, tuple(in_size), tuple(size), align, relu, tr, xb, sl, fam, bad)


def k_id(r):
    return "{}{}_b{}_c{}o{}_{}to{}_{}{}".format("xb_" if r.xb else "", r.tag, r.B, r.C, r.cout, "x".join(map(str, r.in_size)), "x".join(map(str, r.size)),
                                              "al" if r.align else "na", "_tr" if r.tr else "")


K_ROWS = [k("x2_partial_tiles", 2, 12, 27, (3, 5, 17), (6, 10, 34), tr=True, sl=True),      # 4 x 8 x 32 tiles: 4 + 2, 8 + 2, 32 + 2
          k("all_borders", 1, 1, 1, (2, 2, 2), (4, 4, 4), relu=False),
          k("half_align", 1, 3, 28, (3, 5, 6), (5, 9, 11), relu=False),                         # scale exactly 0.5: (n - 1) / (2n - 2)
          k("half_noalign", 2, 4, 29, (3, 5, 9), (6, 10, 18), align=False),                     # scale exactly 0.5: n -> 2n
          k("half_noalign_wide", 1, 4, 27, (2, 4, 33), (4, 8, 66), align=False, tr=True),       # three x-tiles at scale 0.5
          k("x3", 1, 5, 32, (2, 3, 11), (6, 9, 33), tr=True),
          k("x3_noalign", 1, 5, 27, (2, 3, 11), (6, 9, 33), align=False, relu=False, tr=True),
          k("size1_axis", 1, 12, 27, (1, 4, 6), (3, 8, 13), tr=True, sl=True),
          k("ratios_per_axis", 2, 3, 32, (2, 3, 5), (4, 9, 20), align=False, relu=False),
          k("c64", 1, 64, 27, (2, 3, 4), (4, 6, 8), tr=True), k("c64_co32", 1, 64, 32, (2, 3, 4), (5, 7, 9), sl=True)]
K_XB_W = (1, 15, 16, 30, 31)                                                                     # Wo = 2, 30, 32, 60, 62 around the 30-column tiles
K_ROWS += [k("wo", 2 if wi == 16 else 1, 12 if wi != 15 else 5, 27, (2, 3, wi), (4, 6 if wi != 30 else 9, 2 * wi), relu=wi != 31, tr=True, xb=True, sl=wi == 16) for wi in K_XB_W]
K_MULTI = dict(B=2, C=12, cout=27, in_size=(3, 5, 17), size=(6, 10, 34), tr=True)
K_FAM = [k("fam_" + f, xb=xb, fam=f, **K_MULTI) for xb in (False, True) for f in FAMILIES]
K_BAD = [k(f"bad_{v}", xb=xb, relu=a, bad=(v, (1, 3, 15)), **K_MULTI) for xb in (False, True) for v in (INF, NAN) for a in (False, True)]


@functools.lru_cache(maxsize=2)
def k_base(B, C, cout, in_size, size, align, relu, fam, bad):
    g = gen("k1", B, C, cout, in_size, size, fam)
    x = make_x((B, C) + in_size, fam, g, unit=32)
    w = torch.randn((cout, C), generator=g) * 0.3
    if fam == "offset" and C > 1:
        w -= w.mean(dim=1, keepdim=True)
    c = Box(w=w, tabs=tables(in_size, size, align))
    c.x, xz = poison(x, bad)
    c.xz = xz
    xi, c.A = interp(xz.double(), c.tabs), interp(xz.double().abs(), c.tabs)
    c.xi = F.relu(xi) if relu else xi
    c.pre, c.wA = mix(w.double(), c.xi), mix(w.double().abs(), c.A)
    c.bound = (3 * E23 + (C + 1) * E24) * c.wA
    if bad is not None:
        c.reach1 = tap_reach(indicator((B, C) + in_size, bad), c.tabs)[:, 1:2] > 0      # per voxel: every output channel of it
        keep = torch.ones(C, dtype=F64)
        keep[1] = 0.0
        c.pre_without = mix(w.double() * keep, c.xi)                                    # the ReLU departure of the docstring
    return c


def k_base_of(r):
    return k_base(r.B, r.C, r.cout, r.in_size, r.size, r.align, r.relu, r.fam, r.bad)


def k_gate(r, c, pre=None):
    """(ref, bound): P of the plain form, Q of the xblend form"""
    pre = c.pre if pre is None else pre
    if not r.xb:
        return pre, c.bound
    tx = lin_tables(r.size[2], 2 * r.size[2], True)
    return qblend(pre, tx), (3 * E23 + (r.C + 10) * E24) * qblend(c.wA, tx)


def k_reach(r, c):
    if not r.xb:
        return c.reach1
    tx = lin_tables(r.size[2], 2 * r.size[2], True)
    tx1 = (tx[0], tx[1], torch.ones_like(tx[2]), torch.ones_like(tx[3]))
    return qblend(c.reach1.double().expand(-1, 27, -1, -1, -1), tx1)[:, :1] > 0


# =========================================================================== CPU: classes, properties, yardsticks, mutants
@pytest.fixture(scope="module")
def ops():
    import rag_amd
    rag_amd.load_library()
    return rag_amd.ops


ALL_INST = ({("valu", cfg, cout, pair) for cfg in (0, 1, 2) for cout in (1, 2) for pair in PAIRS} | {("c1", pair) for pair in PAIRS}
            | {("upconv", pair) for pair in PAIRS} | {("uptaps", False), ("uptaps", True)} | {("k1", 28, False), ("k1", 32, False), ("k1", 28, True)})


def test_every_row_reaches_its_class(ops):
    seen = set()
    for r in S_ROWS + S_BAD:
        B, D, H, W = r.shape
        route = s_probe(ops, r)
        assert route == r.route, (s_id(r), route)
        if route:
            assert route - 1 == choose_cfg(B, D, H, W), s_id(r)
            if route == 1:
                assert B * D * H * W >= 1 << 20
            if r.cout == 1 and r.cin <= 64:      # off conv3d_c1 for one of the reasons the route names
                assert r.res or r.misalign or W % 4 or D * H * W < BIG, s_id(r)
            seen.add(("valu", route - 1, r.cout, r.pair))
        else:
            assert D * H * W >= BIG and W % 4 == 0 and r.cout == 1 and not r.res and r.cin <= 64
            seen.add(("c1", r.pair))
    for cfg, tx in ((2, 8), (1, 16), (0, 32)):
        D, H, W = V_PART[cfg][1:]
        assert D % 4 and H % 8 and W % tx and cdiv(W, tx) > 1, cfg
        assert V_PAST[cfg][3] > tx
    # W one past the x-tile: configuration 2 only (the docstring)
    assert ops.conv3d_k3_small_route(4, 2, 1, 4, 8192, 33) == 3 and ops.conv3d_k3_small_route(4, 2, 1, 4, 8192, 17) == 3 and V_PAST[2][3] == 9
    # conv3d_c1's work list: nwork = 116 (not a multiple of 8) on the ragged row, one 4-plane segment pair on the exact one
    assert cdiv(36, 32) * cdiv(65, 64) * cdiv(113, 4) == 116 and 113 % 4 == 1 and 65 % 64 == 1 and 36 % 32 == 4
    # the thresholds of c1_eligible, one at a time
    base = dict(cin=4, cout=1, B=1, D=4, H=256, W=256)
    assert ops.conv3d_k3_small_route(**base) == 0
    assert ops.conv3d_k3_small_route(**dict(base, H=255)) != 0 and ops.conv3d_k3_small_route(**dict(base, cin=68)) != 0
    assert ops.conv3d_k3_small_route(**base, has_res=True) != 0 and ops.conv3d_k3_small_route(**base, x_align_ok=False) != 0
    assert ops.conv3d_k3_small_route(**base, y_align_ok=False) == 2 and ops.conv3d_k3_small_route(**base, y_bstride=4 * 65536 + 2) != 0
    assert ops.conv3d_k3_small_route(**dict(base, cout=2)) != 0 and ops.conv3d_k3_small_route(**dict(base, B=4)) == 0
    assert ops.conv3d_k3_small_route(**base, dtype=torch.bfloat16, out_dtype=torch.float32) == 0
    for bad in (dict(cout=3), dict(cin=6), dict(cin=132, cout=2)):
        with pytest.raises(RuntimeError, match="status -2"):
            ops.conv3d_k3_small_route(**dict(base, **bad))
    with pytest.raises(RuntimeError, match="status -2"):
        ops.conv3d_k3_small_route(**base, dtype=torch.float32, out_dtype=torch.bfloat16)
    assert ops.conv3d_k3_small_route(128, 2, 1, 3, 7, 9) == 3                 # the weight-LDS limit: Cout * Cin <= 256

    for r in U_ROWS + U_FAM + U_BAD:
        assert ops.upconv3d_c1_supported(r.cin, *r.in_size), u_id(r)
        seen.add(("upconv", r.pair))
    for r in T_ROWS + T_SINGLE + T_FAM + T_BAD:
        assert ops.uptaps3d_supported(*r.in_size, xblended=r.xb), t_id(r)
        seen.add(("uptaps", r.xb))
    nwork = lambda B, sz: cdiv(2 * sz[2], 32) * cdiv(2 * sz[1], 64) * cdiv(2 * sz[0], 4) * B      # noqa: E731
    assert [nwork(B, sz) for B, sz in HEAD_SHAPES] == [1, 2, 2, 12, 16]
    assert {2 * sz[1] for _, sz in HEAD_SHAPES} >= {62, 64, 66} and {2 * sz[2] for _, sz in HEAD_SHAPES} >= {28, 32, 36}
    assert {r.cin for r in U_ROWS} >= {1, 5, 12, 64} and any(r.sl for r in U_ROWS) and {r.pair for r in U_ROWS} == set(PAIRS)
    for r in K_ROWS + K_FAM + K_BAD:
        assert ops.trilinear3d_act_k1_supported(r.C, r.cout, r.in_size, r.size, r.align, xblend=r.xb), k_id(r)
        assert ops.trilinear3d_route(r.in_size, r.size, r.C, r.align) == "Staged"
        seen.add(("k1", 28 if r.cout <= 28 else 32, r.xb))
    plain = [r for r in K_ROWS if not r.xb]
    assert {r.C for r in plain} >= {1, 3, 4, 5, 12, 64} and {r.cout for r in plain} >= {1, 27, 28, 29, 32}
    assert {(r.tr, r.relu) for r in plain} == {(a, b) for a in (False, True) for b in (False, True)}
    half = lambda a, b, al: (float(torch.tensor(a - 1.0) / torch.tensor(b - 1.0)) if al else float(torch.tensor(float(a)) / torch.tensor(float(b)))) == 0.5      # noqa: E731
    assert all(half(a, b, True) for a, b in zip((3, 5, 6), (5, 9, 11))) and all(half(a, b, False) for a, b in zip((3, 5, 9), (6, 10, 18)))
    assert {r.size[2] for r in K_ROWS if r.xb} == {2, 30, 32, 60, 62}
    for wo in (31, 61):                                                        # an odd Wo has no Wi with Wo == 2 Wi
        assert not any(ops.trilinear3d_act_k1_supported(12, 27, (2, 3, wi), (4, 6, wo), True, xblend=True) for wi in range(1, wo + 1))
    assert ops.trilinear3d_act_k1_supported(12, 27, (3, 4, 4), (5, 8, 8), True)           # scale 2/4 on z is the boundary ...
    assert not ops.trilinear3d_act_k1_supported(12, 27, (4, 4, 4), (6, 8, 8), True)       # ... 3/5 is past it
    assert seen >= ALL_INST, sorted(ALL_INST - seen, key=repr)


def test_x2_pattern_is_exact():
    """x2, align_corners=True, the fp32 rule, every axis length 2..4096 and every output index X: i0 == max((X - 1) // 2, 0) — output 2k
    reads (k - 1, k), output 2k + 1 reads (k, k + 1), never one lower: the ylow / xlow / row0_dy2 / shifted-wz branches of
    upconv3d_c1_kernel and uptaps3d_kernel are unreached (the docstring)"""
    for n in range(2, 4097):
        i0, i1, w0, w1 = lin_tables(n, 2 * n, True)
        want = ((torch.arange(2 * n) - 1) // 2).clamp_min(0)
        assert torch.equal(i0, want), (n, (i0 != want).nonzero().flatten()[:4].tolist())
        assert torch.equal(i1, (want + 1).clamp_max(n - 1))


def test_conv27_is_conv3d():
    """the device reference path is the CPU one: the 27 shifted multiply-adds are F.conv3d in float64"""
    g = gen("conv27")
    x, w = torch.randn((2, 5, 4, 7, 9), generator=g).double(), torch.randn((3, 5, 3, 3, 3), generator=g).double()
    assert torch.allclose(conv27(x, w), F.conv3d(x, w, padding=1), rtol=1e-13, atol=1e-13)
    p = torch.randn((2, 27, 3, 4, 5), generator=g).double()
    eye = torch.zeros((1, 27, 3, 3, 3), dtype=F64)
    for tap in range(27):
        eye[0, tap, tap // 9, tap // 3 % 3, tap % 3] = 1.0
    assert torch.allclose(tapsum(p), F.conv3d(p, eye, padding=1), rtol=1e-13, atol=1e-13)      # tap t reads v + (dz, dy, dx) - 1
    tx = lin_tables(5, 10, True)
    q9 = qblend(p, tx)
    assert torch.allclose(tapsum(interp(q9, [ident(3), ident(4), ident(10)])), tapsum(interp(p, [ident(3), ident(4), tx])), rtol=1e-13, atol=1e-13)


RESAMPLE = sorted({(r.in_size, x2(r.in_size), True) for r in U_ROWS + U_FAM} | {(r.in_size, r.size, r.align) for r in K_ROWS + K_FAM} | {((3, 33, 8), (6, 66, 16), True)})


@pytest.mark.parametrize("in_size,size,align", RESAMPLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_restatement_matches_aten(in_size, size, align):
    """F.interpolate in fp32 sits within 3 * 2^-23 * A of the float64 interpolation built on lin_tables, on every resample row"""
    x = torch.randn((2, 3) + in_size, generator=gen("restate", in_size, size))
    tabs = tables(in_size, size, align)
    ref, bound = interp(x.double(), tabs), 3 * E23 * interp(x.double().abs(), tabs)
    aten = F.interpolate(x, size, mode="trilinear", align_corners=align)
    worst = float(((aten.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"HEAD restatement {in_size} -> {size} align={align}: ATen fp32 at {worst:.3f} of the gate")
    assert worst <= 1.0


def uniq(rows, key):
    return list({key(r): r for r in rows}.values())


@pytest.mark.parametrize("r", uniq(S_ROWS, lambda r: (r.shape, r.cin, r.pair != "f32", r.fam)), ids=s_id)
def test_small_yardstick(r):
    """ATen's fp32 F.conv3d passes the row's arithmetic gate on both output channels; on N(0,1) rows the gate is tight"""
    c = s_base_of(r, "cpu")
    err = (F.conv3d(c.xz, c.w, padding=1).double() - c.pre).abs()
    assert bool((err <= (27 * r.cin + 1) * E24 * c.mag).all()), s_id(r)
    if r.fam == "n01":
        assert bool((c.mag > 0).all()) and float(((27 * r.cin + 1) * E24 * c.mag / c.pre.abs().clamp_min(1e-300)).median()) < 1e-2


@pytest.mark.parametrize("r", uniq(U_ROWS + U_FAM, lambda r: (r.B, r.in_size, r.cin, r.pair != "f32", r.fam)), ids=u_id)
def test_upconv_yardstick(r):
    c = u_base_of(r)
    aten = F.conv3d(F.interpolate(c.xz, scale_factor=2, mode="trilinear", align_corners=True), c.w, padding=1).double()
    assert bool(inside(aten, c.pre, (3 * E23 + (27 * r.cin + 1) * E24) * c.amag).all()), u_id(r)


@pytest.mark.parametrize("r", uniq(T_ROWS + T_FAM + T_SINGLE[::9], lambda r: (r.B, r.in_size, r.xb, r.fam, r.only)), ids=t_id)
def test_uptaps_yardstick(r):
    """ATen's fp32 F.interpolate (Q: along z and y only) and a plain fp32 sum of the shifted volumes pass the row's gate"""
    c = t_base_of(r)
    aten = tapsum(F.interpolate(c.p, size=x2(r.in_size)[:2] + (c.p.shape[4] if r.xb else 2 * r.in_size[2],), mode="trilinear", align_corners=True)).double()
    assert bool(inside(aten, c.pre, (16 if r.xb else 25) * E24 * c.m).all()), t_id(r)
    if r.only is not None:
        assert bool((c.m == 0).any()) and bool((aten[c.m == 0] == 0).all())


@pytest.mark.parametrize("r", K_ROWS + K_FAM, ids=k_id)
def test_k1_yardstick(r):
    """ATen's fp32 F.interpolate (+ ReLU), an fp32 einsum and, for xblend, an fp32 x blend pass the row's gate"""
    c = k_base_of(r)
    up = F.interpolate(c.xz, r.size, mode="trilinear", align_corners=r.align)
    p32 = torch.einsum("oc,bcdhw->bodhw", c.w, F.relu(up) if r.relu else up)
    ref, bound = k_gate(r, c)
    if r.xb:
        tx = lin_tables(r.size[2], 2 * r.size[2], True)
        p32 = qblend(p32, (tx[0], tx[1], tx[2].float(), tx[3].float()))
    assert bool(inside(p32, ref, bound).all()), k_id(r)


def test_pair_gate_holds_the_fp32_pair():
    """the tap pair's gate (k1 bound pushed through U, plus the uptaps chain) holds an fp32 evaluation of the pair"""
    r = k("pair", 2, 12, 27, (2, 17, 9), (3, 33, 18), tr=True)
    c = k_base_of(r)
    ref, bound = pair_gate(r, c)
    up = F.relu(F.interpolate(c.xz, r.size, mode="trilinear", align_corners=True))
    p32 = torch.einsum("oc,bcdhw->bodhw", c.w, up)
    got = tapsum(F.interpolate(p32, scale_factor=2, mode="trilinear", align_corners=True))
    assert bool(inside(got, ref, bound).all())


def pair_gate(r, c):
    tabs = tables(r.size, x2(r.size))
    return tapsum(interp(c.pre, tabs)), tapsum(interp(c.bound, tabs)) + 25 * E24 * tapsum(interp(c.wA, tabs))


def rejected(got, ref, bound, where):
    """the mutant fails the gate somewhere on `where` and passes everywhere else"""
    ok = inside(got, ref, bound)
    where = where.expand_as(ok)
    return bool((~ok[where]).any()) and bool(ok[~where].all())


def test_gates_reject_a_wrong_small_conv():
    """a dropped tap, a dropped channel, replicate padding at the faces, a clamped halo column at a tile edge, dz / dx swapped"""
    r = s("mutant", 3, (1, 5, 9, 40), 4, 2, bn=True, relu=False)
    c = s_base_of(r, "cpu")
    ref, bound = s_gate(r, c)
    x64, w64 = c.xz.double(), c.w.double()
    act = lambda pre: bn_act(pre, pre, c.bn, False)[0]      # noqa: E731
    everywhere, ch1 = torch.ones(1, dtype=torch.bool).view(1, 1, 1, 1, 1), torch.tensor([False, True]).view(1, 2, 1, 1, 1)
    assert bool(inside(act(conv27(x64, w64)), ref, bound).all())
    w = w64.clone()
    w[1, 2, 0, 2, 1] = 0.0
    assert rejected(act(conv27(x64, w)), ref, bound, ch1), "a dropped tap"
    w = w64.clone()
    w[:, 3] = 0.0
    assert rejected(act(conv27(x64, w)), ref, bound, everywhere), "a dropped channel"
    face = torch.ones((1, 1, 5, 9, 40), dtype=torch.bool)
    face[:, :, 1:-1, 1:-1, 1:-1] = False
    assert rejected(act(conv27(x64, w64, replicate=True)), ref, bound, face), "replicate padding"
    xm = x64.clone()
    xm[..., 32] = xm[..., 31]                                 # the halo column x0 + 32 of tile 0 read from the clamped neighbour 31
    mut = conv27(x64, w64)
    mut[..., 31] = conv27(xm, w64)[..., 31]
    col = torch.zeros((1, 1, 1, 1, 40), dtype=torch.bool)
    col[..., 31] = True
    assert rejected(act(mut), ref, bound, col), "a clamped halo column"
    assert rejected(act(conv27(x64, w64.transpose(2, 4))), ref, bound, everywhere), "dz and dx swapped"


def test_gates_reject_a_wrong_head():
    """the same mutants behind the upsample (upconv), a dropped tap volume (uptaps, both forms), a dropped channel and an untransposed
    weight (k1, both forms)"""
    r = u("mutant", 1, (3, 9, 10), 5, bn=True)
    c = u_base_of(r)
    ref, bound = u_gate(r, c)
    up, w64 = interp(c.xz.double(), c.tabs), c.w.double()
    act = lambda pre: bn_act(pre, pre, c.bn, False)[0]      # noqa: E731
    everywhere = torch.ones(1, dtype=torch.bool).view(1, 1, 1, 1, 1)
    assert bool(inside(act(conv27(up, w64)), ref, bound).all())
    w = w64.clone()
    w[0, 2, 0, 2, 1] = 0.0
    assert rejected(act(conv27(up, w)), ref, bound, everywhere), "a dropped tap"
    w = w64.clone()
    w[:, 4] = 0.0
    assert rejected(act(conv27(up, w)), ref, bound, everywhere), "a dropped channel"
    face = torch.ones((1, 1, 6, 18, 20), dtype=torch.bool)
    face[:, :, 1:-1, 1:-1, 1:-1] = False
    assert rejected(act(conv27(up, w64, replicate=True)), ref, bound, face), "replicate padding"
    assert rejected(act(conv27(up, w64.transpose(2, 4))), ref, bound, everywhere), "dz and dx swapped"
    for xb in (False, True):
        rt = t("mutant", 1, (3, 9, 10), xb)
        ct = t_base_of(rt)
        ref, bound = t_gate(rt, ct)
        tz, ty, tx = tables(rt.in_size, x2(rt.in_size))
        tabs = [tz, ty, ident(20)] if xb else [tz, ty, tx]
        p = ct.p.double().clone()
        assert bool(inside(tapsum(interp(p, tabs)), ref, bound).all())
        p[:, 4] = 0.0
        assert rejected(tapsum(interp(p, tabs)), ref, bound, everywhere), "a dropped tap volume"
        rk = k("mutant", 1, 12, 27, (2, 3, 5), (4, 6, 10), tr=True, xb=xb)
        ck = k_base_of(rk)
        ref, bound = k_gate(rk, ck)
        assert bool(inside(k_gate(rk, ck, mix(ck.w.double(), ck.xi))[0], ref, bound).all())
        w = ck.w.double().clone()
        w[:, 11] = 0.0
        assert rejected(k_gate(rk, ck, mix(w, ck.xi))[0], ref, bound, everywhere), "a dropped channel"
        wt = ck.w.t().contiguous().view(27, 12).double()
        assert rejected(k_gate(rk, ck, mix(wt, ck.xi))[0], ref, bound, everywhere), "an untransposed weight"


def test_gates_reject_exact_lambdas_at_index_400():
    """lambdas from the exact source index differ from the fp32 rule's by up to half an ulp of src (2^-16 for src in [256, 512));
    on an `offset` row (100 + n01) the k1 gate is about 3.6e-5 there and the blend differs by that lambda error times the
    difference of two neighbours — the gate rejects it on the elements where that product is largest, and on N(0, 1) data everywhere"""
    for fam, must in (("offset", True), ("n01", True)):
        r = k("lambda", 1, 1, 1, (1, 1, 410), (1, 1, 820), relu=False, fam=fam)
        c = k_base_of(r)
        ref, bound = k_gate(r, c)
        mut = mix(c.w.double(), interp(c.xz.double(), [ident(1), ident(1), exact_tables(410, 820)]))
        far = torch.arange(820).view(1, 1, 1, 1, -1) >= 512
        n_out = int((~inside(mut, ref, bound))[far.expand_as(ref)].sum())
        print(f"HEAD exact-lambda mutant on {fam}: {n_out} of {int(far.sum())} outputs past index 256 outside the gate")
        assert (n_out > 0) == must, (fam, n_out)


# =========================================================================== GPU
@pytest.fixture(scope="module")
def gops():
    import rag_amd
    rag_amd.load_library()
    return rag_amd.ops


def nan_buf(shape, dt):
    return torch.full(shape, NAN, device=DEV, dtype=dt)


def sliced(x, dt, on):
    """x on the device; `on`: as channels 3 .. 3 + C of a wider NaN-filled buffer (a channel-slice view)"""
    x = x.to(DEV, dt)
    if not on:
        return x
    buf = nan_buf((x.shape[0], x.shape[1] + 5) + tuple(x.shape[2:]), dt)
    buf[:, 3:3 + x.shape[1]] = x
    return buf[:, 3:3 + x.shape[1]]


def guarded_out(B, ch, spatial, dt, misalign=False):
    """(buffer, view of its middle `ch` channels' owner): GUARD NaN channels either side; misalign: the buffer starts one element into
    its allocation (4-byte but not 16-byte aligned)"""
    shape = (B, ch + 2 * GUARD) + tuple(spatial)
    if not misalign:
        return nan_buf(shape, dt)
    flat = nan_buf((prod(shape) + 1,), dt)
    buf = flat[1:].view(shape)
    assert buf.data_ptr() % 16 == 4
    return buf


def taken(buf, ch, tag):
    full = buf.cpu()
    assert bool(torch.isnan(full[:, :GUARD]).all()) and bool(torch.isnan(full[:, GUARD + ch:]).all()), (tag, "a store left its destination channels")
    return full[:, GUARD:GUARD + ch]


def g32(v):
    return v.to(DEV).float().contiguous()


def s_run(ops, r, c):
    xdt, ydt = PAIRS[r.pair]
    B, D, H, W = r.shape
    if r.bview:
        xb = nan_buf((B, r.cin + 4, D, H, W), xdt)
        xb[:, 2:2 + r.cin] = c.x.to(DEV, xdt)
        x = xb[:, 2:2 + r.cin]
    else:
        x = c.x.to(DEV, xdt)
    buf = guarded_out(B, r.cout, (D, H, W), ydt, r.misalign)
    res = None
    if r.res:
        res = nan_buf((B, r.cout + 2, D, H, W), xdt)
        res[:, 1:1 + r.cout] = c.res[:, :r.cout].to(DEV, xdt)
    bn = (g32(c.bn[0][:r.cout]), g32(c.bn[1][:r.cout])) if r.bn else (None, None)
    ops.conv3d_k3_small(x, g32(c.w[:r.cout]), bn[0], bn[1], r.relu, buf, GUARD, res, 1)
    torch.cuda.synchronize()
    return taken(buf, r.cout, s_id(r)), (lambda: ops.conv3d_k3_small(x, g32(c.w[:r.cout]), bn[0], bn[1], r.relu, buf, GUARD, res, 1)[:, GUARD:GUARD + r.cout].cpu())


def s_kernel(r):
    return "conv3d_c1" if r.route == 0 else f"valu_cfg{r.route - 1}"


@pytest.mark.gpu
@pytest.mark.parametrize("r", S_ROWS, ids=s_id)
def test_small(gops, r):
    """every VALU instantiation and conv3d_c1 class of the row tables, residual and destination at channel offsets of NaN-guarded buffers"""
    c = s_base_of(r)
    got, _ = s_run(gops, r, c)
    check(s_id(r), s_kernel(r), got, *s_gate(r, c))


@pytest.mark.gpu
@pytest.mark.parametrize("r", S_BAD, ids=s_id)
def test_small_non_finite(gops, r):
    c = s_base_of(r)
    got, _ = s_run(gops, r, c)
    ref, bound = s_gate(r, c)
    check_reach(s_id(r), s_kernel(r), got, c.reach, ref, bound, r.relu)


def u_run(ops, r, c):
    xdt, ydt = PAIRS[r.pair]
    x = sliced(c.x, xdt, r.sl)
    buf = guarded_out(r.B, 1, x2(r.in_size), ydt)
    bn = (g32(c.bn[0]), g32(c.bn[1])) if r.bn else (None, None)
    call = lambda: ops.upconv3d_c1(x, g32(c.w), bn[0], bn[1], r.relu, buf, GUARD)      # noqa: E731
    call()
    torch.cuda.synchronize()
    return taken(buf, 1, u_id(r)), (lambda: call()[:, GUARD:GUARD + 1].cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("r", U_ROWS + U_FAM, ids=u_id)
def test_upconv(gops, r):
    c = u_base_of(r)
    got, _ = u_run(gops, r, c)
    check(u_id(r), "upconv3d_c1", got, *u_gate(r, c))


@pytest.mark.gpu
@pytest.mark.parametrize("r", U_BAD, ids=u_id)
def test_upconv_non_finite(gops, r):
    c = u_base_of(r)
    got, _ = u_run(gops, r, c)
    ref, bound = u_gate(r, c)
    check_reach(u_id(r), "upconv3d_c1", got, c.reach, ref, bound, r.relu)


def t_run(ops, r, c):
    p = c.p.to(DEV)
    buf = guarded_out(r.B, 1, x2(r.in_size), torch.float32)
    bn = (g32(c.bn[0]), g32(c.bn[1])) if r.bn else (None, None)
    call = lambda: ops.uptaps3d(p, bn[0], bn[1], r.relu, buf, GUARD, xblended=r.xb)      # noqa: E731
    call()
    torch.cuda.synchronize()
    return taken(buf, 1, t_id(r)), (lambda: call()[:, GUARD:GUARD + 1].cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("r", T_ROWS + T_SINGLE + T_FAM, ids=t_id)
def test_uptaps(gops, r):
    """both forms on every head shape; one tap volume at a time: a wrong offset or padding edge is a displaced volume, and where
    the shifted upsample is zero the gate is zero"""
    c = t_base_of(r)
    got, _ = t_run(gops, r, c)
    ref, bound = t_gate(r, c)
    check(t_id(r), "uptaps3d_xb" if r.xb else "uptaps3d", got, ref, bound)
    if r.only is not None:                                   # (the centre tap alone shifts nothing out of the volume)
        assert bool((c.m == 0).any()) == (r.only != (4 if r.xb else 13)) and bool((got[c.m == 0] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("r", T_BAD, ids=t_id)
def test_uptaps_non_finite(gops, r):
    """the rows that found uptaps3d_kernel's zero-weight window slots (the file's docstring): the non-finite outputs are exactly the reach"""
    c = t_base_of(r)
    got, _ = t_run(gops, r, c)
    ref, bound = t_gate(r, c)
    check_reach(t_id(r), "uptaps3d_xb" if r.xb else "uptaps3d", got, c.reach, ref, bound, r.relu)


def k_run(ops, r, c):
    x = sliced(c.x, torch.float32, r.sl)
    ch, spatial = (9, r.size[:2] + (2 * r.size[2],)) if r.xb else (r.cout, r.size)
    buf = guarded_out(r.B, ch, spatial, torch.float32)
    w = g32(c.w.t() if r.tr else c.w)
    call = lambda: ops.trilinear3d_act_k1(x, r.size, r.align, r.relu, w, buf, GUARD, transposed=r.tr, xblend=r.xb)      # noqa: E731
    call()
    torch.cuda.synchronize()
    return taken(buf, ch, k_id(r)), (lambda: call()[:, GUARD:GUARD + ch].cpu())


def k_kernel(r):
    return f"up_k1<{28 if r.cout <= 28 else 32},{'xb' if r.xb else 'plain'}>"


@pytest.mark.gpu
@pytest.mark.parametrize("r", K_ROWS + K_FAM, ids=k_id)
def test_k1(gops, r):
    c = k_base_of(r)
    got, _ = k_run(gops, r, c)
    check(k_id(r), k_kernel(r), got, *k_gate(r, c))


@pytest.mark.gpu
@pytest.mark.parametrize("r", K_BAD, ids=k_id)
def test_k1_non_finite(gops, r):
    """all Cout channels (all nine rows of Q) of the reach are affected; behind the ReLU a NaN sample is 0 and the output the mix of the
    other channels (the docstring)"""
    c = k_base_of(r)
    got, _ = k_run(gops, r, c)
    ref, bound = k_gate(r, c)
    reach = k_reach(r, c).expand_as(ref)
    assert reach.any() and not reach[0].any() and reach.sum() <= reach.numel() // 8
    check(k_id(r), k_kernel(r), torch.where(reach, torch.zeros_like(got), got), ref, bound, where=~reach)
    fin = torch.isfinite(got) & reach
    if not r.relu:
        assert not fin.any(), (k_id(r), f"{int(fin.sum())} finite outputs inside the reach of a non-finite input")
    else:
        want, _ = k_gate(r, c, torch.where(c.reach1, c.pre_without, c.pre))
        assert bool(inside(got, want, bound)[fin].all()), (k_id(r), "a finite value inside the reach that is not the mix of the other channels")


PAIR_ROWS = [(B, sz) for B, sz in HEAD_SHAPES] + [(1, (3, 33, 8))]


@pytest.mark.gpu
@pytest.mark.parametrize("B,size", PAIR_ROWS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"b{v}")
def test_xblend_pair_equals_tap_pair_and_holds_its_gate(gops, B, size):
    """act_k1(xblend) -> uptaps3d(xblended) has the bits of act_k1 -> uptaps3d on every tap-form shape, and the pair holds its gate"""
    in12 = (cdiv(size[0], 2), cdiv(size[1], 2), size[2] // 2)
    r = k("pair", B, 12, 27, in12, size, tr=True)
    assert gops.trilinear3d_act_k1_supported(12, 27, in12, size, True, xblend=True) and gops.uptaps3d_supported(*size, xblended=True)
    c = k_base_of(r)
    x, w = c.x.to(DEV), g32(c.w.t())
    p6 = gops.trilinear3d_act_k1(x, size, True, True, w, transposed=True)
    old = gops.uptaps3d(p6, None, None, False)
    q6 = gops.trilinear3d_act_k1(x, size, True, True, w, transposed=True, xblend=True)
    new = gops.uptaps3d(q6, None, None, False, xblended=True)
    assert torch.isfinite(old).all() and torch.equal(new, old), int((new != old).sum())
    check(f"pair_b{B}_{size}", "k1->uptaps3d", old.cpu(), *pair_gate(r, c))


REPEAT = [("small", S_FAM[0]), ("small", S_FAM[4]), ("upconv", U_FAM[0]), ("uptaps", T_FAM[0]), ("uptaps", T_FAM[4]), ("k1", K_FAM[0]), ("k1", K_FAM[4])]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,r", REPEAT, ids=[f"{kind}{i}" for i, (kind, _) in enumerate(REPEAT)])
def test_every_kernel_repeats_its_bits(gops, kind, r):
    base_of, run = {"small": (s_base_of, s_run), "upconv": (u_base_of, u_run), "uptaps": (t_base_of, t_run), "k1": (k_base_of, k_run)}[kind]
    got, again = run(gops, r, base_of(r))
    assert torch.isfinite(got).all() and torch.equal(got, again())


def refused(code, call, *outs):
    """the call raises with the documented status before any launch: every NaN-prefilled output comes back untouched"""
    with pytest.raises(RuntimeError) as e:
        call()
    torch.cuda.synchronize()
    m = re.search(r"status (-?\d+)", str(e.value))
    assert m and int(m.group(1)) == code, str(e.value)
    for o in outs:
        assert bool(torch.isnan(o).all()), "a refused call wrote its output"


@pytest.mark.gpu
def test_abi_refusals_before_any_launch(gops):
    ops, EINVAL, EUNSUP = gops, -1, -2
    f32, bf16 = torch.float32, torch.bfloat16
    dev = lambda *shape, dt=f32: torch.zeros(shape, device=DEV, dtype=dt)      # noqa: E731
    one = torch.ones(1, device=DEV)
    w12, w1 = dev(1, 12, 3, 3, 3), dev(1, 4, 3, 3, 3)
    # upconv3d_c1
    for in_size in ((2, 2, 3), (1, 4, 4), (4, 1, 4)):                           # odd Wi; an axis of length 1
        out = nan_buf((1, 1) + x2(in_size), f32)
        refused(EUNSUP, lambda: ops.upconv3d_c1(dev(1, 12, *in_size), w12, None, None, False, out), out)
    out = nan_buf((1, 1, 4, 4, 4), f32)
    refused(EINVAL, lambda: ops.upconv3d_c1(dev(1, 12, 2, 2, 2), w12, one, None, False, out), out)
    refused(EUNSUP, lambda: ops.upconv3d_c1(dev(1, 65, 2, 2, 2), dev(1, 65, 3, 3, 3), None, None, False, out), out)
    outb = nan_buf((1, 1, 4, 4, 4), bf16)
    refused(EUNSUP, lambda: ops.upconv3d_c1(dev(1, 12, 2, 2, 2), w12, None, None, False, outb), outb)      # f32 -> bf16 is not built
    flat = nan_buf((65,), f32)
    refused(EUNSUP, lambda: ops.upconv3d_c1(dev(1, 12, 2, 2, 2), w12, None, None, False, flat[1:].view(1, 1, 4, 4, 4)), flat)
    # conv3d_k3_small
    out = nan_buf((1, 3, 2, 4, 8), f32)
    refused(EUNSUP, lambda: ops.conv3d_k3_small(dev(1, 4, 2, 4, 8), dev(3, 4, 3, 3, 3), None, None, False, out), out)
    refused(EUNSUP, lambda: ops.conv3d_k3_small(dev(1, 6, 2, 4, 8), dev(1, 6, 3, 3, 3), None, None, False, out), out)
    refused(EUNSUP, lambda: ops.conv3d_k3_small(dev(1, 132, 2, 4, 8), dev(2, 132, 3, 3, 3), None, None, False, out), out)
    refused(EINVAL, lambda: ops.conv3d_k3_small(dev(1, 4, 2, 4, 8), w1, None, one, False, out), out)
    outb = nan_buf((1, 1, 2, 4, 8), bf16)
    with pytest.raises(RuntimeError):                                           # f32 -> bf16: the wrapper's own refusal
        ops.conv3d_k3_small(dev(1, 4, 2, 4, 8), w1, None, None, False, outb)
    assert bool(torch.isnan(outb).all())
    # uptaps3d, both forms
    for xb in (False, True):
        nt = 9 if xb else 27
        wide = lambda wi: 2 * wi if xb else wi      # noqa: E731
        out = nan_buf((1, 1, 4, 4, 4), f32)
        refused(EINVAL, lambda: ops.uptaps3d(dev(1, nt, 2, 2, wide(2)), one, None, False, out, xblended=xb), out)
        refused(EUNSUP, lambda: ops.uptaps3d(dev(1, nt, 2, 2, wide(2), dt=bf16), None, None, False, xblended=xb))
        for in_size in ((2, 2, 3), (1, 4, 4), (4, 4, 1)):
            out = nan_buf((1, 1) + x2(in_size), f32)
            refused(EUNSUP, lambda: ops.uptaps3d(dev(1, nt, in_size[0], in_size[1], wide(in_size[2])), None, None, False, out, xblended=xb), out)
        flat = nan_buf((65,), f32)
        refused(EUNSUP, lambda: ops.uptaps3d(dev(1, nt, 2, 2, wide(2)), None, None, False, flat[1:].view(1, 1, 4, 4, 4), xblended=xb), flat)      # a misaligned y
    qflat = torch.zeros(9 * 2 * 2 * 4 + 1, device=DEV)
    out = nan_buf((1, 1, 4, 4, 4), f32)
    refused(EUNSUP, lambda: ops.uptaps3d(qflat[1:].view(1, 9, 2, 2, 4), None, None, False, out, xblended=True), out)                                # a misaligned q
    # trilinear3d_act_k1
    w = dev(12, 27)
    out = nan_buf((1, 27, 6, 8, 8), f32)
    refused(EUNSUP, lambda: ops.trilinear3d_act_k1(dev(1, 12, 4, 4, 4), (6, 8, 8), True, True, w, out, transposed=True), out)                      # scale 3/5 > 0.5
    out = nan_buf((1, 27, 4, 8, 7), f32)
    refused(EUNSUP, lambda: ops.trilinear3d_act_k1(dev(1, 12, 2, 4, 4), (4, 8, 7), False, True, w, out, transposed=True), out)                     # 4/7 without align
    out = nan_buf((1, 33, 4, 4, 4), f32)
    refused(EUNSUP, lambda: ops.trilinear3d_act_k1(dev(1, 12, 2, 2, 2), (4, 4, 4), True, True, dev(33, 12), out), out)
    refused(EUNSUP, lambda: ops.trilinear3d_act_k1(dev(1, 12, 2, 2, 2, dt=bf16), (4, 4, 4), True, True, w, transposed=True))
    out = nan_buf((1, 9, 4, 4, 12), f32)
    refused(EUNSUP, lambda: ops.trilinear3d_act_k1(dev(1, 12, 2, 2, 2), (4, 4, 6), True, True, w, out, transposed=True, xblend=True), out)         # Wo != 2 Wi
    out = nan_buf((1, 9, 4, 4, 62), f32)
    refused(EUNSUP, lambda: ops.trilinear3d_act_k1(dev(1, 12, 2, 2, 15), (4, 4, 31), True, True, w, out, transposed=True, xblend=True), out)       # an odd Wo
