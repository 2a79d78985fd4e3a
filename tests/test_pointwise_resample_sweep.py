"""Sweep of the kernels between the cells and in the head that no derived gate held yet — conv_k1_kernel, conv_k1_chain_kernel,
conv_k1_resample_kernel, add_kernel (rag_amd/csrc/pointwise.hip), trilinear_kernel, trilinear_up_kernel (resample.hip),
conv2d_k3_strided_kernel (conv2d_strided.hip) and the staging half of cell2d_x3_kernel (conv2d_x3.hip) — through rag_amd.ops only,
per element against float64 computed from the values the kernel reads (bf16-rounded under bf16 storage).

Reference.  The trilinear indices and lambdas are ATen's fp32 rule restated in lin_tables (include/rag_amd.h, csrc/common.h):
align_corners: src = fl32(scale * dst); otherwise src = fl32(scale * (dst + 0.5) - 0.5) in ONE rounding, clamped at 0;
i0 = min(int(src), n - 1), i1 = min(i0 + 1, n - 1), lambda = fl32(src - i0) clamped to [0, 1], w0 = fl32(1 - lambda); equal sizes: the
identity (i, i, 1, 0).  Everything after that is float64.  test_restatement_matches_aten proves the restatement against
F.interpolate in fp32 over down, up, non-integer, depth-1 and 200 -> 400 shapes.

Gates, per element, nothing excused (E24 = 2^-24 ...; A = the same interpolation of |x|; mag = sum |w| * |operand|):
    trilinear                     3 * 2^-23 * A
    1x1x1 fmaf chain, n channels  (n + 1) * 2^-24 * mag
    resample + 1x1x1              sum_ci |w| * 3 * 2^-23 * A_ci + (Cin + 1) * 2^-24 * sum_ci |w| A_ci
    folded BN                     b = |scale| * arith + 2^-23 * (|scale * pre| + |shift|); no BN: b = arith; ReLU leaves b unchanged
    bf16 storage                  + 2^-8 * |ref| per stored tensor
    chain Cin -> 24 -> 12         b1 through |W2| (+ 2^-8 * |h_ref| under bf16), then the second chain and BN terms; and the bits of
                                  two conv3d_k1 calls
    add                           the bits of torch's CPU a + b in the storage type
    strided 3x3                   (9 Cin + 1) * 2^-24 * mag, then the BN term
    cell2d, staged s0 / s1        the resample + 1x1x1 + BN bound: b_s
    cell2d, convolution           conv(b_s, |w3|) + (2^-20 + 1e-6) * mag3 + 2^-33 * block      (block as tests/test_conv3d_k3_sweep.py)
    cell2d, after it              BN per set, then sum_s b + 2^-23 * sum_s |act(u_s)|
    guards                        two NaN channels either side of every destination slice, and the unused groups of a permuted
                                  out_group_ch, come back NaN

Non-finite inputs: one Inf, NaN or 3e38 in channel 1 of sample 1.  reach = the outputs whose tap index set holds the element,
whatever the weights (0 * Inf is NaN, as in ATen).  Outside the reach the row's gate holds against the reference with the element
zeroed.  Inside it, for Inf / NaN every value is non-finite or exactly +0 behind a ReLU (fmaxf stores a NaN pre-activation as 0:
include/rag_amd.h); 3e38 is finite, so a finite value there must be inside the gate of the float64 result WITH the element.
cell2d: the pre-conv of the poisoned input runs without ReLU (so s0 is non-finite over the staged reach); behind the final ReLU the
output is +0 + act(u_B), so a finite value inside the reach must be act(u_B) within set B's gate — the dual-launch departure of the
k3 sweep, for the same reason.  3e38 there: s0 = w1 * 3e38 is finite for |w1| < 1.13 but above the 2^110 that no scale brings into
fp16's range (include/rag_amd.h), so set A may come out non-finite where float64 is finite; a finite output must be inside the gate
of the float64 result with the element or, behind the ReLU, be act(u_B) as above.  Without the ReLU only the first is accepted.

Mutants (test_gates_reject_*): the torch emulation of each kernel (exact fmaf through float64, ATen's lerp nesting) passes every
gate; with the last channel of a U trip dropped, the neighbouring channel's BN in a ragged slab, w0 / w1 swapped on one axis, the
clamped i1 read as (i0 + 1) modulo the row, the weight read untransposed, it fails on the named row.  (Under align_corners = 1 the
clamped column has lambda == 0 exactly, so the unclamped tap shows on finite data under align_corners = 0 only; the non-finite row
with its element in column 0 holds it otherwise.)  Lambdas from a contracted (more accurate) src differ from the reference's by up
to 2^-24 * src: the gate sees that at the sweep's own sizes on every fp32 row whose scale is no dyadic fraction
(test_gates_reject_contracted_lambdas); tests/test_hip_parity.py::test_trilinear_bit_identical_to_aten_cpu holds it bit for bit.

Rows are the smallest shapes that reach their class; the probes ops.conv3d_k1_plan, ops.conv3d_k1_resample_plan and
ops.trilinear3d_route are the authority (test_every_row_reaches_its_instantiation).

Every GPU row prints `K1 case=... inst=... worst=err/bound`.  Measured on the MI355X, worst err / bound (records, not gates):
  conv_k1           fp32, one voxel per thread, NCO 24 / 16 / 12 / 8 / 4: 0.537 / 0.500 / 0.504 / 0.478 / 0.426; four voxels per thread:
                    0.547 / 0.554 / 0.600 / 0.506 / 0.563; families n01 0.357 / offset 0.185 / spread 0.457 / steps 0.466 / sparse 0.423;
                    non-finite 0.525          bf16: every width and form 0.996, families 0.995 / 0.960 / 0.993 / 0.990 / 0.993
  conv_k1_chain     fp32 rows 0.079, families 0.041 / 0.010 / 0.147 / 0.063 / 0.052; bf16 rows 0.721, families 0.790 / 0.620 / 0.875 / 0.690 /
                    0.704 (and the bits of two conv3d_k1 calls on every row)
  conv_k1_resample  fp32, NCO 24 / 16 / 12 / 8 / 4: 0.292 / 0.312 / 0.340 / 0.382 / 0.366; families 0.145 / 0.126 / 0.258 / 0.378 / 0.305;
                    non-finite 0.173          bf16 (and bf16 -> fp32): 0.996
  trilinear         staged kernel: rows 0.464, families 0.411 / 0.412 / 0.524 / 0.493 / 0.481, non-finite 0.407, bf16 0.996
                    generic kernel: rows 0.393, families 0.323 / 0.314 / 0.404 / 0.427 / 0.281, non-finite 0.323, bf16 0.995
  add               0 on every row (exact)
  conv2d_k3_strided fp32 rows 0.228, families 0.052 / 0.029 / 0.113 / 0.073 / 0.078; bf16 rows 0.993, families 0.974 / 0.960 / 0.969 / 0.971 / 0.955
  cell2d            rows 0.023, families 0.021 / 0.005 / 0.077 / 0.032 / 0.035, non-finite 0.024
The bf16 rows sit just under 1 by construction (round to nearest moves a value by up to 2^-8 of itself: the storage term); the fp32
rows are the arithmetic underneath.  cell2d's gate is dominated by the F32X3 term of the 3x3 convolutions, which the kernel's
scaled-fp16 products use a fortieth of.  No row failed on the device and no kernel was changed; no gate departs from the gates listed above.

Unmarked tests run without a GPU; the rest need the MI355X."""
import collections
import ctypes
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
E8, E20, E23, E24, E33 = 2.0 ** -8, 2.0 ** -20, 2.0 ** -23, 2.0 ** -24, 2.0 ** -33
NAN, INF = float("nan"), float("inf")
GUARD = 2
FAMILIES = ("n01", "offset", "spread", "steps", "sparse")
BAD_VALUES = (INF, NAN, 3e38)
F64 = torch.float64


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def cdiv(a, b):
    return -(-a // b)


def prod(s):
    n = 1
    for v in s:
        n *= v
    return n


# --------------------------------------------------------------------------- the fp32 index rule and the float64 references
def lin_tables(n_in, n_out, align, contracted=False):
    """(i0, i1, w0, w1) per output index: ATen's fp32 rule (the docstring).  contracted: the lambda of a fused scale * dst - i0 (a mutant)"""
    dst = torch.arange(n_out)
    if n_in == n_out:
        return dst, dst.clone(), torch.ones(n_out, dtype=F64), torch.zeros(n_out, dtype=F64)
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)      # noqa: E731
    if align:
        scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
        exact = scale.double() * dst.double()
        src = scale * dst.float()
    else:
        scale = f32(n_in) / f32(n_out)
        exact = (scale.double() * (dst.double() + 0.5) - 0.5).clamp_min(0)      # exact in float64: one rounding below
        src = exact.float()
    i0 = src.long().clamp_max(n_in - 1)
    lam = ((exact - i0.double()).float() if contracted else src - i0.float()).clamp(0, 1)
    return i0, (i0 + 1).clamp_max(n_in - 1), (1 - lam).double(), lam.double()


def tables(in_size, size, align, contracted=False):
    return [lin_tables(a, b, align, contracted) for a, b in zip(in_size, size)]


def interp(x, tabs):
    """float64 (or any dtype's own) interpolation of x[B, C, D, H, W] along x, y, z with the given tables"""
    for dim, (i0, i1, w0, w1) in zip((4, 3, 2), reversed(tabs)):
        shape = [1] * x.dim()
        shape[dim] = -1
        i0, i1 = i0.to(x.device), i1.to(x.device)
        x = x.index_select(dim, i0) * w0.to(x.device, x.dtype).view(shape) + x.index_select(dim, i1) * w1.to(x.device, x.dtype).view(shape)
    return x


def tap_reach(ind, tabs):
    """outputs whose tap index set holds a marked input element, whatever the weights"""
    return interp(ind, [(i0, i1, torch.ones_like(w0), torch.ones_like(w1)) for i0, i1, w0, w1 in tabs]) > 0


def vb(t, like):
    return t.to(like.device, F64).view([1, -1] + [1] * (like.dim() - 2))


def mix(w, x):
    return torch.einsum("oc,bc...->bo...", w.to(x.device, x.dtype), x)


def bn_act(pre, arith, scale, shift, relu):
    if scale is not None:
        sc, sh = vb(scale, pre), vb(shift, pre)
        u, b = pre * sc + sh, sc.abs() * arith + E23 * ((sc * pre).abs() + sh.abs())
    else:
        u, b = pre, arith
    return (F.relu(u) if relu else u), b


def stored(bf, ref, bound):
    return bound + E8 * ref.abs() if bf else bound


def gate_k1(x, w, scale, shift, relu):
    """x: float64 [B, Cin, ...] as read; (ref, bound) before storage"""
    w = w.double()
    return bn_act(mix(w, x), (w.shape[1] + 1) * E24 * mix(w.abs(), x.abs()), scale, shift, relu)


def gate_k1r(x, tabs, w, scale, shift, relu):
    w = w.double()
    xi, A = interp(x, tabs), interp(x.abs(), tabs)
    return bn_act(mix(w, xi), (3 * E23 + (w.shape[1] + 1) * E24) * mix(w.abs(), A), scale, shift, relu)


def gate_tri(x, tabs, relu):
    v = interp(x, tabs)
    return (F.relu(v) if relu else v), 3 * E23 * interp(x.abs(), tabs)


def check(tag, inst, got, ref, bound, where=None):
    """every element (of `where`) finite and inside the bound, on whichever device the reference lives; returns the worst err / bound"""
    g64 = got.detach().to(ref.device).double()
    assert g64.shape == ref.shape, (tag, g64.shape, ref.shape)
    sel = torch.ones_like(ref, dtype=torch.bool) if where is None else where.expand_as(ref)
    assert torch.isfinite(g64[sel]).all(), (tag, inst, "non-finite output")
    err = (g64 - ref).abs()
    ratio = (err / bound.clamp_min(1e-300))[sel]
    k = int(ratio.argmax())
    print(f"K1 case={tag} inst={inst} worst={float(err[sel][k]):.3e}/{float(bound[sel][k]):.3e} = {float(ratio[k]):.3f}")
    assert float(ratio[k]) <= 1.0, (tag, inst, float(ratio[k]))
    return float(ratio[k])


def check_reach(tag, inst, got, reach, gate_zeroed, gate_with, val, relu):
    """the non-finite rule of the docstring; gate_zeroed / gate_with: () -> (ref, bound with storage)"""
    got = got.detach().cpu()
    assert reach.any() and not reach[0].any() and reach.sum() <= reach.numel() // 8, (tag, int(reach.sum()))
    ref, bound = gate_zeroed()
    check(tag, inst, torch.where(reach, torch.zeros_like(got), got), ref, bound, where=~reach)
    inside, fin = got[reach].double(), torch.isfinite(got[reach])
    if val == 3e38:
        want, wb = gate_with()
        assert bool(((inside - want[reach]).abs() <= wb[reach])[fin].all()), (tag, "a finite wrong value inside the reach")
    elif not relu:
        assert not fin.any(), (tag, "a non-finite input left a finite output inside its reach")
    else:
        assert bool((inside[fin] == 0).all()) and not bool(torch.signbit(inside[fin]).any()), (tag, "a finite value other than +0 inside the reach")


# --------------------------------------------------------------------------- inputs
def make_x(shape, fam, g, unit=256):
    """[B, C, *spatial] of a conditioning family, built as tests/test_conv3d_k3_sweep.py does; the units of "steps" and "sparse" are
    runs of `unit` voxels (a workgroup's)"""
    x = torch.randn(shape, generator=g)
    idx = (torch.arange(prod(shape[2:])) // unit).view(shape[2:])
    if fam == "offset":
        x += 100.0
    elif fam == "spread":
        x *= torch.exp2(torch.rand(x.shape, generator=g) * 40 - 20)
    elif fam == "steps":
        x *= torch.tensor([0.0, 1.0, 1e3, 1e7, 1e-3])[idx % 5]
    elif fam == "sparse":
        x = x.abs() * (torch.rand(x.shape, generator=g) > 0.7) * (idx % 3 != 0)
        x[shape[0] - 1] = 0.0
    return x


def make_w(cout, cin, fam, g, amp=0.3):
    w = torch.randn((cout, cin), generator=g) * amp
    if fam == "offset" and cin > 1:
        w -= w.mean(dim=1, keepdim=True)          # cancelling sums
    elif fam == "spread":
        w *= torch.exp2(torch.rand(w.shape, generator=g) * 40 - 20)
    return w


def make_bn(c, g):
    return (torch.rand(c, generator=g) + 0.5) * (1 - 2 * (torch.rand(c, generator=g) < 0.25).float()), torch.randn(c, generator=g) * 0.1


def rnd(x, bf):
    return x.to(torch.bfloat16).float() if bf else x


def poison(x, bad, ch=1):
    """(x with the element, x with it zeroed); bad = (value, spatial index) in channel `ch` of sample 1"""
    val, at = bad
    xz, xv = x.clone(), x.clone()
    xz[(1, ch) + tuple(at)] = 0.0
    xv[(1, ch) + tuple(at)] = val
    return xv, xz


# --------------------------------------------------------------------------- rows: conv3d_k1
K1 = collections.namedtuple("K1", "tag B cin cout V bf nco vec bn relu tr sl fam bad big")


def k1(tag, B, cin, cout, V, nco, vec=False, bf=False, bn=True, relu=True, tr=False, sl=False, fam="n01", bad=None, big=False):
    return K1(tag, B, cin, cout, V, bf, nco, vec, bn, relu, tr, sl, fam, bad, big)


def k1_id(r):
    return f"{r.tag}_b{r.B}c{r.cin}o{r.cout}v{r.V}_{'bf16' if r.bf else 'f32'}_n{r.nco}{'v' if r.vec else ''}"


M = 1 << 20
K1_ROWS = []
for _bf in (False, True):
    K1_ROWS += [k1("vec_cover", 1, 3 + (co // 4) % 2, co, M, co, True, _bf, big=True) for co in (24, 16, 12, 8, 4)]
    K1_ROWS += [k1("vec_narrow", 2, 4, 24, 1 << 17, 4, True, _bf, big=True), k1("vec_narrow", 1, 3, 40, 1 << 18, 12, True, _bf, big=True),
                k1("slab", 1, 4, 24, 100000, 8, bf=_bf), k1("slab", 1, 4, 24, 160000, 16, bf=_bf), k1("slab", 1, 4, 16, 140000, 12, bf=_bf),
                k1("slab", 1, 3, 36, 160000, 24, bf=_bf), k1("slab", 1, 4, 48, 70000, 12, bf=_bf),
                k1("misaligned", 1, 3, 24, (1 << 18) + 3, 24, bf=_bf, big=True), k1("misaligned", 1, 4, 12, (1 << 18) + 1, 12, bf=_bf, big=True),
                k1("small", 2, 7, 5, 777, 4, bf=_bf)]
K1_ROWS += [k1("cout", 2, 4, co, 777, 4) for co in (1, 25, 36)] + [k1("cin", 2, ci, 12, 515, 4) for ci in (1, 3, 64)]
K1_ROWS += [k1("transposed", 2, 7, 12, 777, 4, tr=True), k1("transposed", 1, 5, 24, 160000, 16, tr=True),
            k1("slices", 2, 7, 13, 777, 4, sl=True), k1("slices", 2, 7, 13, 777, 4, sl=True, bf=True), k1("slices_vec", 2, 4, 8, 1 << 17, 4, True, sl=True, big=True),
            k1("nobn", 2, 7, 12, 777, 4, bn=False), k1("norelu", 2, 7, 12, 777, 4, relu=False), k1("plain", 2, 7, 12, 777, 4, bn=False, relu=False)]
K1_FAM = [k1("fam_" + f, 2, 7, 25, 1300, 4, fam=f) for f in FAMILIES] + [k1("fam_" + f, 2, 7, 25, 1300, 4, fam=f, bf=True) for f in FAMILIES]
# the bad voxel: the first of a workgroup's 256 (non-VEC), the last column of a thread's four at a workgroup's end (VEC)
K1_BAD = [k1(f"bad_{v}", 2, 7, 25, 1300, 4, bn=a, relu=a, bad=(v, (256,))) for v in BAD_VALUES for a in (False, True)]
K1_BAD += [k1(f"bad_{v}", 2, 4, 8, 1 << 17, 4, True, bn=a, relu=a, bad=(v, (1023,)), big=True) for v in BAD_VALUES for a in (False, True)]

# conv_k1_kernel<T, NCO, VEC>: launch_k1's switch x the two storages x the vector form
K1_KEYS = {(bf, nco, vec) for bf in (False, True) for nco in (24, 16, 12, 8, 4) for vec in (False, True)}


@functools.lru_cache(maxsize=2)
def k1_base(B, cin, cout, V, bf, fam, bad):
    g = gen("k1", B, cin, cout, V, fam)
    x = rnd(make_x((B, cin, V), fam, g), bf)
    c = {"w": make_w(cout, cin, fam, g), "x": x, "xz": x}
    c["scale"], c["shift"] = make_bn(cout, g)
    if bad is not None:
        c["x"], c["xz"] = poison(x, bad)
    return c


def k1_base_of(r):
    return k1_base(r.B, r.cin, r.cout, r.V, r.bf, r.fam, r.bad)


def k1_gate(r, c, x, dev="cpu"):
    ref, b = gate_k1(x.to(dev).double(), c["w"], c["scale"] if r.bn else None, c["shift"] if r.bn else None, r.relu)
    return ref, stored(r.bf, ref, b)


# --------------------------------------------------------------------------- rows: conv3d_k1_chain
CH = collections.namedtuple("CH", "B cin V bf bn1 relu1 bn2 relu2 fam", defaults=("n01",))
CH_ROWS = [CH(2, ci, v, bf, True, True, True, False) for ci in (1, 17, 64) for v in (1, 255, 257) for bf in (False, True)]
CH_ROWS += [CH(2, 17, 257, bf, a, b, c, d) for bf in (False, True) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True)
            if (a, b, c, d) != (True, True, True, False)]
CH_FAM = [CH(2, 17, 1300, bf, True, True, True, False, f) for bf in (False, True) for f in FAMILIES]


def ch_id(r):
    return f"{'' if r.fam == 'n01' and r.V != 1300 else 'fam_' + r.fam + '_'}c{r.cin}v{r.V}_{'bf16' if r.bf else 'f32'}_bn{int(r.bn1)}{int(r.relu1)}{int(r.bn2)}{int(r.relu2)}"


@functools.lru_cache(maxsize=2)
def ch_base(B, cin, V, bf, fam="n01"):
    g = gen("chain", B, cin, V, fam)
    c = {"x": rnd(make_x((B, cin, V), fam, g), bf), "w1": make_w(24, cin, fam, g), "w2": make_w(12, 24, fam, g)}
    c["s1"], c["h1"] = make_bn(24, g)
    c["s2"], c["h2"] = make_bn(12, g)
    return c


def ch_gate(r, c):
    h, b1 = gate_k1(c["x"].double(), c["w1"], c["s1"] if r.bn1 else None, c["h1"] if r.bn1 else None, r.relu1)
    b1 = stored(r.bf, h, b1)                                                        # the rounded intermediate
    w2 = c["w2"].double()
    ref, b = bn_act(mix(w2, h), mix(w2.abs(), b1) + 25 * E24 * mix(w2.abs(), h.abs()), c["s2"] if r.bn2 else None, c["h2"] if r.bn2 else None, r.relu2)
    return ref, stored(r.bf, ref, b)


# --------------------------------------------------------------------------- rows: conv3d_k1_resample, _pair, _multi
KR = collections.namedtuple("KR", "tag form B specs size align bf f32out nco bn relu fam bad")


def kr(tag, form, B, specs, size, nco, align=True, bf=False, f32out=False, bn=True, relu=True, fam="n01", bad=None):
    """specs: ((cin, cout, in_size), ...); bad: (value, (z, y, x)) in channel min(1, cin - 1) of sample 1 of input 0"""
    return KR(tag, form, B, tuple((ci, co, tuple(s)) for ci, co, s in specs), tuple(size), align, bf, f32out, nco, bn, relu, fam, bad)


def kr_id(r):
    sp = "+".join(f"c{ci}o{co}_{'x'.join(map(str, s))}" for ci, co, s in r.specs)
    return f"{r.tag}_{r.form}_b{r.B}_{sp}_to_{'x'.join(map(str, r.size))}_{'bf16' if r.bf else 'f32'}{'_f32out' if r.f32out else ''}{'' if r.align else '_ac0'}_n{r.nco}{'_at' + '.'.join(map(str, r.bad[1])) if r.bad else ''}"


RATIOS = [((8, 10, 14), (4, 5, 7)), ((7, 9, 13), (4, 5, 7)), ((3, 5, 6), (6, 10, 12)), ((5, 7, 9), (13, 15, 40)), ((4, 6, 1), (8, 12, 5)), ((1, 6, 9), (1, 12, 18)),
          ((4, 5, 7), (4, 5, 7))]
KR_ROWS = [kr("ratio", "single", 2, ((ci, 12, a),), b, 4) for (a, b), ci in zip(RATIOS, (5, 3, 17, 1, 5, 3, 17))]
KR_ROWS += [kr("ratio", "single", 2, ((5, 12, a),), b, 4, align=False) for a, b in RATIOS[:5]]
KR_ROWS += [kr("cin_u8", "single", 2, ((ci, 4, (8, 10, 14)),), (4, 5, 7), 4) for ci in (1, 3, 5, 17, 33, 48)]
KR_ROWS += [kr("cin_same_u16", "single", 2, ((ci, 8, (4, 5, 7)),), (4, 5, 7), 4) for ci in (1, 5, 17, 33)]
# the wider slabs (U = 4 trips) need 2^16 .. 2^17 output voxels: the plan's `want`
BIGO, HALF = (32, 64, 64), (16, 64, 64)
for _bf in (False, True):
    KR_ROWS += [kr("slab", "single", 1, ((3, 24, (16, 32, 32)),), BIGO, 24, bf=_bf), kr("slab", "single", 1, ((5, 16, (16, 32, 32)),), BIGO, 16, bf=_bf),
                kr("slab", "single", 1, ((17, 12, (8, 16, 16)),), BIGO, 12, bf=_bf), kr("slab", "single", 1, ((1, 16, (32, 128, 128)),), HALF, 8, bf=_bf),
                kr("slab_ragged", "single", 1, ((5, 25, (16, 32, 32)),), HALF, 24, bf=_bf), kr("slab_ragged", "single", 2, ((3, 25, (8, 10, 14)),), (4, 5, 7), 4, bf=_bf)]
KR_ROWS += [kr("slab_same", "single", 1, ((17, 24, HALF),), HALF, 12), kr("slab", "single", 1, ((33, 24, (8, 32, 32)),), HALF, 12),
            kr("slab_ac0", "single", 1, ((5, 16, (16, 32, 32)),), BIGO, 16, align=False),
            kr("f32out", "single", 2, ((5, 12, (8, 10, 14)),), (4, 5, 7), 4, bf=True, f32out=True), kr("f32out", "single", 1, ((5, 16, (16, 32, 32)),), BIGO, 16, bf=True, f32out=True),
            kr("nobn", "single", 2, ((5, 12, (8, 10, 14)),), (4, 5, 7), 4, bn=False, relu=False),
            kr("pair", "pair", 1, ((5, 16, (32, 128, 128)), (17, 12, (8, 32, 32))), HALF, 16), kr("pair", "pair", 1, ((5, 16, (32, 128, 128)), (17, 12, (8, 32, 32))), HALF, 16, bf=True),
            kr("pair_ident", "pair", 2, ((3, 8, (8, 10, 14)), (4, 8, (4, 5, 7))), (4, 5, 7), 4), kr("pair_ident", "pair", 1, ((3, 8, HALF), (4, 8, (8, 32, 32))), HALF, 8),
            kr("triple", "multi", 2, ((3, 8, (8, 10, 14)), (17, 12, (4, 5, 7)), (5, 4, (8, 10, 14))), (4, 5, 7), 4),
            kr("triple", "multi", 1, ((3, 8, (32, 128, 128)), (17, 12, HALF), (5, 4, (32, 128, 128))), HALF, 12),
            kr("triple", "multi", 2, ((3, 8, (8, 10, 14)), (17, 12, (4, 5, 7)), (5, 4, (8, 10, 14))), (4, 5, 7), 4, bf=True)]
KR_FAM = [kr("fam_" + f, "single", 2, ((5, 12, (8, 10, 14)),), (4, 5, 7), 4, fam=f) for f in FAMILIES]
# (1, 2, 6): taps of a `pair` load; (1, 2, 13): the clamped last column (i1 == i0 there, and only there); (1, 2, 0): the column an
# unclamped i1 read modulo the row would take into the last one
KR_BAD = [kr(f"bad_{v}", form, 2, specs, (4, 5, 7), 4, bn=a, relu=a, bad=(v, at)) for v in BAD_VALUES for a in (False, True)
          for form, specs, at in (("single", ((5, 12, (8, 10, 14)),), (1, 2, 6)), ("single", ((5, 12, (8, 10, 14)),), (1, 2, 13)),
                                  ("single", ((5, 12, (8, 10, 14)),), (1, 2, 0)), ("pair", ((5, 8, (8, 10, 14)), (4, 8, (4, 5, 7))), (1, 2, 13)))]
KR_KEYS = {(bf, nco) for bf in (False, True) for nco in (24, 16, 12, 8, 4)}      # conv_k1_resample_kernel<T, NCO>


@functools.lru_cache(maxsize=2)
def kr_base(B, specs, size, bf, fam, bad):
    g = gen("k1r", B, specs, size, fam)
    c = {"x": [], "xz": [], "w": [], "scale": [], "shift": []}
    for i, (ci, co, s) in enumerate(specs):
        x = rnd(make_x((B, ci) + s, fam, g), bf)
        xz = x
        if bad is not None and i == 0:
            x, xz = poison(x, bad, min(1, ci - 1))
        c["x"].append(x)
        c["xz"].append(xz)
        c["w"].append(make_w(co, ci, fam, g))
        sc, sh = make_bn(co, g)
        c["scale"].append(sc)
        c["shift"].append(sh)
    return c


def kr_base_of(r):
    return kr_base(r.B, r.specs, r.size, r.bf, r.fam, r.bad)


def kr_gate(r, c, i, x, dev="cpu"):
    tabs = tables(r.specs[i][2], r.size, r.align)
    ref, b = gate_k1r(x.to(dev).double(), tabs, c["w"][i], c["scale"][i] if r.bn else None, c["shift"][i] if r.bn else None, r.relu)
    return ref, stored(r.bf and not r.f32out, ref, b)


# --------------------------------------------------------------------------- rows: trilinear3d, trilinear3d_act
TR = collections.namedtuple("TR", "tag B C in_size size align route bf relu sl plain fam bad")


def tr(tag, B, C, in_size, size, route, align=True, bf=False, relu=False, sl=False, plain=False, fam="n01", bad=None):
    return TR(tag, B, C, tuple(in_size), tuple(size), align, route, bf, relu, sl, plain, fam, bad)


def tr_id(r):
    return (f"{r.tag}_b{r.B}c{r.C}_{'x'.join(map(str, r.in_size))}_to_{'x'.join(map(str, r.size))}_{'bf16' if r.bf else 'f32'}"
            f"{'' if r.align else '_ac0'}{'_relu' if r.relu else ''}_{r.route}")


TR_ROWS = [tr("x2_channels", 2, C, (3, 5, 17), (6, 10, 34), "Staged") for C in (1, 3, 4, 6, 9)]
TR_ROWS += [tr("tile_edge", 2, 6, (2, 4, 16), (5, 9, 33), "Staged"), tr("tile_exact", 2, 5, (2, 4, 16), (4, 8, 32), "Staged"), tr("depth1_out", 2, 3, (3, 4, 16), (1, 8, 32), "Staged"),
            tr("depth1", 2, 6, (1, 4, 17), (1, 8, 34), "Staged"), tr("x2", 2, 6, (2, 4, 11), (4, 8, 22), "Staged", align=False), tr("x3", 2, 5, (2, 3, 12), (6, 9, 36), "Staged", align=False),
            tr("noninteger_up", 2, 3, (5, 7, 9), (13, 15, 40), "Staged"), tr("noninteger_up", 2, 6, (3, 5, 7), (7, 11, 16), "Staged", align=False),
            tr("plain", 2, 9, (3, 5, 17), (6, 10, 34), "Staged", plain=True), tr("slices", 2, 6, (3, 5, 17), (6, 10, 34), "Staged", sl=True, relu=True),
            tr("relu", 2, 3, (2, 4, 16), (5, 9, 33), "Staged", relu=True), tr("bf16", 2, 6, (2, 4, 16), (5, 9, 33), "Staged", bf=True), tr("bf16", 2, 3, (3, 5, 17), (6, 10, 34), "Staged", bf=True, sl=True, relu=True),
            tr("down", 2, 5, (7, 9, 13), (4, 5, 7), "Generic"), tr("down", 2, 4, (8, 10, 14), (4, 5, 7), "Generic", align=False), tr("axis_unchanged", 2, 3, (4, 6, 10), (4, 12, 20), "Generic"),
            tr("up_less_than_2", 2, 6, (4, 6, 10), (6, 9, 15), "Generic"), tr("up_less_than_2", 2, 1, (4, 6, 10), (6, 9, 15), "Generic", align=False),
            tr("plain", 2, 9, (8, 10, 14), (4, 5, 7), "Generic", plain=True), tr("slices", 2, 6, (8, 10, 14), (4, 5, 7), "Generic", sl=True, relu=True),
            tr("bf16", 2, 3, (8, 10, 14), (4, 5, 7), "Generic", bf=True, sl=True, relu=True), tr("bf16", 2, 4, (4, 6, 10), (4, 12, 20), "Generic", bf=True)]
TR_FAM = [tr("fam_" + f, 2, 6, s, o, route, fam=f) for f in FAMILIES for s, o, route in (((2, 4, 16), (5, 9, 33), "Staged"), ((8, 10, 14), (4, 5, 7), "Generic"))]
# Staged: input column 15 is the last one the first x tile stages and the first of the second; Generic: a 256-voxel block's end
TR_BAD = [tr(f"bad_{v}", 2, 6, s, o, route, relu=a, bad=(v, at)) for v in BAD_VALUES for a in (False, True)
          for s, o, route, at in (((2, 4, 18), (5, 9, 37), "Staged", (1, 3, 15)), ((8, 10, 14), (4, 5, 7), "Generic", (3, 7, 11)))]
TR_KEYS = {(bf, route) for bf in (False, True) for route in ("Staged", "Generic")}


@functools.lru_cache(maxsize=2)
def tr_base(B, C, in_size, bf, fam, bad):
    x = rnd(make_x((B, C) + in_size, fam, gen("tri", B, C, in_size, fam), unit=16), bf)
    return poison(x, bad, min(1, C - 1)) if bad is not None else (x, x)


def tr_gate(r, x):
    ref, b = gate_tri(x.double(), tables(r.in_size, r.size, r.align), r.relu)
    return ref, stored(r.bf, ref, b)


# --------------------------------------------------------------------------- rows: add, conv2d_k3_strided
AD = collections.namedtuple("AD", "tag B C V ca cb cy a0 b0 y0 bf")
AD_ROWS = [AD("vector", 2, 5, 1028, 9, 9, 9, 2, 2, 2, bf) for bf in (False, True)]
AD_ROWS += [AD("scalar_odd_volume", 2, 5, 777, 9, 9, 9, 2, 1, 3, bf) for bf in (False, True)]
AD_ROWS += [AD("scalar_misaligned_offset", 2, 4, 1030, 8, 9, 8, 1, 2, 2, bf) for bf in (False, True)]      # ch0 * DHW % 4 == 2: off a 16-byte boundary
AD_ROWS += [AD("scalar_misaligned_base", 2, 5, 1028, 9, 9, 9, 2, 2, 2, bf) for bf in (False, True)]
AD_ROWS += [AD("vector_two_blocks", 1, 3, 4096, 3, 5, 7, 0, 2, 2, False), AD("scalar_one_voxel", 3, 7, 1, 9, 9, 11, 1, 2, 2, False)]

CS = collections.namedtuple("CS", "B cin cout H W stride bf bn relu fam", defaults=("n01",))
CS_ROWS = [CS(2, ci, co, h, w, s, False, True, True) for ci, co, h, w, s in
           ((6, 12, 17, 35, 3), (3, 13, 17, 35, 2), (1, 25, 17, 17, 1), (6, 5, 17, 33, 4), (3, 1, 1, 17, 2), (3, 12, 17, 1, 3), (6, 25, 2, 17, 2), (1, 5, 2, 2, 1), (3, 13, 1, 1, 1),
            (6, 12, 40, 61, 1), (3, 25, 33, 47, 3))]
CS_ROWS += [CS(2, 6, 13, 17, 35, 3, True, True, True), CS(2, 3, 25, 17, 17, 2, True, True, False), CS(2, 3, 13, 17, 35, 2, False, False, False), CS(2, 6, 12, 17, 35, 4, False, False, True)]
CS_FAM = [CS(2, 6, 13, 33, 47, 3, bf, True, True, f) for bf in (False, True) for f in FAMILIES]      # 6 x 9 = 54 taps: the longest chain here


def cs_id(r):
    return "{}c{}o{}_{}x{}_s{}_{}_bn{}relu{}".format("" if r.fam == "n01" and r not in CS_FAM else "fam_" + r.fam + "_", r.cin, r.cout, r.H, r.W, r.stride,
                                                    "bf16" if r.bf else "f32", int(r.bn), int(r.relu))


# --------------------------------------------------------------------------- rows: cell2d
CE = collections.namedtuple("CE", "tag B C cin0 size0 cin1 size1 size cout pre0 pre1 bnA bnB relu perm fam bad")


def ce(tag, B, C, cin0, size0, cin1, size1, size, cout, pre0=(True, True), pre1=(True, True), bnA=True, bnB=True, relu=True, perm=False, fam="n01", bad=None):
    """pre0 / pre1: (BN given?, ReLU) of pre_preprocess / preprocess"""
    return CE(tag, B, C, cin0, tuple(size0), cin1, tuple(size1), tuple(size), cout, pre0, pre1, bnA, bnB, relu, perm, fam, bad)


def ce_id(r):
    return (f"{r.tag}_b{r.B}C{r.C}_c{r.cin0}_{'x'.join(map(str, r.size0))}+c{r.cin1}_{'x'.join(map(str, r.size1))}_to_{'x'.join(map(str, r.size))}_o{r.cout}"
            f"{'_perm' if r.perm else ''}")


CE_ROWS = [ce("both_resampled", 2, 8, 17, (18, 66), 5, (5, 17), (9, 33), 12), ce("both_resampled", 1, 4, 1, (34, 140), 48, (9, 35), (17, 70), 20),
           ce("one_identity", 2, 4, 24, (2, 16), 24, (4, 32), (2, 16), 4), ce("one_identity", 1, 8, 17, (19, 65), 5, (9, 33), (9, 33), 12, perm=True),
           ce("both_identity", 2, 8, 1, (9, 33), 48, (9, 33), (9, 33), 4), ce("both_identity", 1, 4, 24, (17, 70), 24, (17, 70), (17, 70), 12),
           ce("null_scale", 2, 4, 17, (18, 66), 5, (9, 33), (9, 33), 12, pre0=(False, True), pre1=(True, False)),
           ce("null_scale", 2, 8, 5, (4, 32), 17, (2, 16), (2, 16), 20, pre0=(True, False), pre1=(False, False), bnA=False, relu=False, perm=True)]
CE_FAM = [ce("fam_" + f, 2, 8, 17, (18, 66), 5, (5, 17), (9, 33), 12, fam=f) for f in FAMILIES]
# the last input pixel of s0 is staged pixel (8, 32) of the 9 x 33 cell and no other: the halo of all four tiles reads it
CE_BAD = [ce(f"bad_{v}", 2, 8, 17, (18, 66), 5, (5, 17), (9, 33), 12, pre0=(True, False), relu=a, bad=(v, (17, 65))) for v in BAD_VALUES for a in (False, True)]


@functools.lru_cache(maxsize=2)
def ce_base(B, C, cin0, size0, cin1, size1, cout, fam, bad):
    g = gen("cell2d", B, C, cin0, size0, cin1, size1, cout, fam)
    c = {"x": [], "xz": [], "w1": [], "bn1": [], "w3": [], "bn3": []}
    for i, (ci, s) in enumerate(((cin0, size0), (cin1, size1))):
        x = make_x((B, ci) + s, fam, g, unit=32)
        xz = x
        if bad is not None and i == 0:
            x, xz = poison(x, bad)
        c["x"].append(x)
        c["xz"].append(xz)
        c["w1"].append(make_w(C, ci, fam, g, 0.4))
        c["bn1"].append(make_bn(C, g))
        c["w3"].append(torch.randn((cout, C, 3, 3), generator=g) * (2.0 / (9 * C)) ** 0.5)
        c["bn3"].append(make_bn(cout, g))
    return c


def ce_base_of(r):
    return ce_base(r.B, r.C, r.cin0, r.size0, r.cin1, r.size1, r.cout, r.fam, r.bad)


def ce_set_gate(r, c, s, x):
    """(act(u_s), b_s after the set's BN) of set s in float64; x: the set's input as read"""
    cin, size_in = ((r.cin0, r.size0), (r.cin1, r.size1))[s]
    (pbn, prelu), bn3 = (r.pre0, r.pre1)[s], (r.bnA, r.bnB)[s]
    tabs = tables((1,) + size_in, (1,) + r.size, True)
    sref, bs = gate_k1r(x.double().unsqueeze(2), tabs, c["w1"][s], c["bn1"][s][0] if pbn else None, c["bn1"][s][1] if pbn else None, prelu)
    sref, bs = sref.squeeze(2), bs.squeeze(2)
    w3 = c["w3"][s].double()
    pre, mag = F.conv2d(sref, w3, padding=1), F.conv2d(sref.abs(), w3.abs(), padding=1)
    sum_x = F.conv2d(sref.abs(), torch.ones((1, r.C, 3, 3), dtype=F64), padding=1)
    xmax = float(sref.abs().max())
    block = xmax * w3.abs().flatten(1).sum(dim=1).view(1, -1, 1, 1) + w3.abs().flatten(1).max(dim=1).values.view(1, -1, 1, 1) * sum_x
    arith = F.conv2d(bs, w3.abs(), padding=1) + (E20 + 1e-6) * mag + E33 * block
    return bn_act(pre, arith, c["bn3"][s][0] if bn3 else None, c["bn3"][s][1] if bn3 else None, r.relu)


def ce_gate(r, c, xs, sets=(0, 1)):
    terms = [ce_set_gate(r, c, s, xs[s]) for s in sets]
    return sum(t[0] for t in terms), sum(t[1] for t in terms) + E23 * sum(t[0].abs() for t in terms)


# --------------------------------------------------------------------------- torch emulations of the kernels (the yardstick, and the mutants' host)
def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 tensors: the product is exact in float64, the sum is rounded once (to 53 bits, then to 24: 2^-29 relative apart)"""
    return (a.double() * b.double() + c.double()).float()


def emu_interp(x, tabs, swap_axis=None, wrap_i1=False):
    """the kernels' interpolation in fp32: lerp2(w0, a, w1, b) = fmaf(w0, a, fl(w1 * b)), x innermost, then y, then z"""
    for dim, (i0, i1, w0, w1) in zip((4, 3, 2), reversed(tabs)):
        shape = [1] * x.dim()
        shape[dim] = -1
        if wrap_i1 and dim == 4:
            i1 = (i0 + 1) % x.shape[4]                                 # mutant: no clamp, the row read modulo its length
        w0, w1 = (w1, w0) if swap_axis == dim else (w0, w1)            # mutant: the weights swapped on one axis
        x = fma32(w0.float().view(shape), x.index_select(dim, i0), w1.float().view(shape) * x.index_select(dim, i1))
    return x


def emu_k1(xv, w, scale, shift, relu, drop=None):
    """the fmaf chain over the input channels in order, folded BN as one fmaf, fmaxf; drop: an input channel left out (a mutant)"""
    acc = torch.zeros((xv.shape[0], w.shape[0]) + xv.shape[2:])
    wv = lambda t: t.view([1, -1] + [1] * (xv.dim() - 2))      # noqa: E731
    for ci in range(w.shape[1]):
        if ci != drop:
            acc = fma32(wv(w[:, ci]), xv[:, ci:ci + 1], acc)
    if scale is not None:
        acc = fma32(acc, wv(scale), wv(shift))
    return acc.clamp_min(0) if relu else acc


def inside(got, ref, bound):
    return bool(((got.double() - ref).abs() <= bound).all())


# --------------------------------------------------------------------------- CPU tests
@pytest.fixture(scope="module")
def ops():
    import rag_amd
    rag_amd.load_library()
    return rag_amd.ops


def tdt(bf):
    return torch.bfloat16 if bf else torch.float32


def test_every_row_reaches_its_instantiation(ops):
    """The probes are the authority: every conv3d_k1 row's (NCO, VEC), every resample row's NCO, every trilinear row's route; all
    20 + 10 + 2 x 2 instantiations are covered by a GPU row."""
    seen = set()
    for r in K1_ROWS + K1_FAM + K1_BAD:
        # the tensors of run_k1: x starts 3 planes into its buffer when sliced; the destination pointer is its buffer's (an allocation:
        # aligned), but the kernel's first store lies y_ch0 planes in, which conv3d_k1's own test (DHW % 4 == 0) covers — the flag
        # passed here is the stricter one, the alignment of that first plane, so the probe can only answer VEC where every plane is aligned
        x_ok, y_ok = ((3 if r.sl else 0) * r.V) % 4 == 0, ((3 if r.sl else GUARD) * r.V) % 4 == 0
        xbs, ybs = (r.cin + 6 if r.sl else r.cin) * r.V, ((3 if r.sl else GUARD) + r.cout + GUARD) * r.V
        assert ops.conv3d_k1_plan(r.B, r.cin, r.cout, r.V, xbs, ybs, x_ok, y_ok, tdt(r.bf)) == (r.nco, r.vec), k1_id(r)
        assert r.big == (r.B * r.V >= 1 << 18), k1_id(r)
        seen.add((r.bf, r.nco, r.vec))
    assert seen == K1_KEYS, sorted(K1_KEYS - seen)
    seen = set()
    for r in KR_ROWS + KR_FAM + KR_BAD:
        nco = ops.conv3d_k1_resample_plan([s[0] for s in r.specs], [s[1] for s in r.specs], [s[2] for s in r.specs], r.B, r.size, tdt(r.bf))
        assert nco == r.nco, (kr_id(r), nco)
        assert len(r.specs) == {"single": 1, "pair": 2, "multi": 3}[r.form] and (r.align or r.form == "single")
        seen.add((r.bf, r.nco))
    assert seen == KR_KEYS, sorted(KR_KEYS - seen)
    seen = set()
    for r in TR_ROWS + TR_FAM + TR_BAD:
        assert ops.trilinear3d_route(r.in_size, r.size, r.C, r.align) == r.route, tr_id(r)
        seen.add((r.bf, r.route))
    assert seen == TR_KEYS
    for r in CE_ROWS + CE_FAM + CE_BAD:
        assert ops.cell2d_supported(r.C, r.cin0, r.cin1, r.cout, *r.size), ce_id(r)


def test_plan_classes_without_a_gpu_row(ops):
    """launch_k1 / launch_k1r restated: ragged slabs, Cout > 24, the thread thresholds and the >= 128 MB branch agree with the probes"""
    widths = (24, 16, 12, 8, 4)

    def k1_plan(B, cout, V, aligned=True):
        vec = V % 4 == 0 and aligned and B * V >= 1 << 18
        threads, cover = B * cdiv(V, 4 if vec else 1), min([w for w in widths if w >= cout] or [24])
        if threads >= 1 << 18:
            return cover, vec
        return next((w for w in widths if w <= cover and threads * cdiv(cout, w) >= 1 << 18), 4), vec

    def k1r_plan(cins, couts, ins, B, size, esize):
        cmax, threads = max(couts), B * prod(size) * len(cins)
        cover = min([w for w in widths if w >= cmax] or [24])
        if threads >= 1 << 17 or sum(B * ci * prod(s) * esize for ci, s in zip(cins, ins)) >= 128 << 20:
            return cover
        return next((w for w in widths if w <= cover and (w == cover or cmax % w == 0) and threads * cdiv(cmax, w) >= 1 << 17), 4)

    for B in (1, 2, 3):
        for cout in (1, 4, 5, 8, 12, 13, 16, 24, 25, 36, 48, 49, 96):
            for V in (1, 255, 65535, 65536, 87381, 87382, 100000, 131071, 131072, 160000, (1 << 18) - 4, 1 << 18, (1 << 18) + 1, 1 << 20, (1 << 20) - 4, 1 << 22):
                for al in (True, False):
                    assert ops.conv3d_k1_plan(B, 4, cout, V, x_align_ok=al) == k1_plan(B, cout, V, al), (B, cout, V, al)
    # Cout = 24 in slabs of 16 + 8, 36 in 24 + 12, 25 in 24 + 1
    assert ops.conv3d_k1_plan(1, 4, 24, 160000) == (16, False) and ops.conv3d_k1_plan(1, 4, 36, 160000) == (24, False) and ops.conv3d_k1_plan(1, 4, 25, 1 << 20) == (24, True)
    # batch strides that are no multiple of four elements switch the vector form off
    assert ops.conv3d_k1_plan(1, 4, 24, 1 << 20, x_bstride=(4 << 20) + 2) == (24, False) and ops.conv3d_k1_plan(1, 4, 24, 1 << 20, y_bstride=(24 << 20) + 1)[1] is False
    for dt, es in ((torch.float32, 4), (torch.bfloat16, 2)):
        for cins, couts, ins, B, size in (((12,), (16,), ((64, 256, 512),), 1, (16, 32, 64)), ((12,), (16,), ((64, 256, 256),), 1, (16, 32, 64)), ((12,), (16,), ((64, 256, 512),), 1, (8, 16, 32)),
                                          ((6, 6), (16, 12), ((64, 256, 512), (8, 16, 32)), 1, (8, 16, 32)), ((3,), (25,), ((4, 5, 7),), 1, (16, 64, 64)), ((3,), (36,), ((4, 5, 7),), 1, (32, 64, 64)),
                                          ((3,), (36,), ((4, 5, 7),), 1, (16, 32, 64)), ((3,), (48,), ((4, 5, 7),), 1, (16, 32, 64)), ((3, 3, 3), (8, 12, 4), ((4, 5, 7),) * 3, 2, (8, 32, 32)),
                                          ((3,), (5,), ((4, 5, 7),), 1, (32, 64, 64)), ((3,), (24,), ((4, 5, 7),), 1, (8, 32, 64)), ((3,), (24,), ((4, 5, 7),), 1, (4, 32, 64))):
            assert ops.conv3d_k1_resample_plan(cins, couts, ins, B, size, dt) == k1r_plan(cins, couts, ins, B, size, es), (cins, couts, ins, B, size, dt)
    # 12 x 64 x 256 x 512 fp32 inputs are 384 MB (bf16: 192 MB): one slab whatever the thread count; half the width is 96 MB in bf16 only
    assert ops.conv3d_k1_resample_plan((12,), (16,), ((64, 256, 512),), 1, (8, 16, 32)) == 16
    assert ops.conv3d_k1_resample_plan((12,), (16,), ((64, 128, 256),), 1, (8, 16, 32)) == 4
    assert ops.conv3d_k1_resample_plan((12,), (16,), ((64, 256, 256),), 1, (8, 16, 32)) == 16 and ops.conv3d_k1_resample_plan((12,), (16,), ((64, 256, 256),), 1, (8, 16, 32), torch.bfloat16) == 4
    assert ops.trilinear3d_route((4, 8, 8), (8, 16, 16), 3, True) == "Staged" and ops.trilinear3d_route((4, 8, 8), (7, 16, 16), 3, True) == "Staged"
    assert ops.trilinear3d_route((4, 8, 8), (6, 16, 16), 3, True) == "Generic" and ops.trilinear3d_route((4, 8, 8), (7, 16, 16), 3, False) == "Generic"
    assert ops.trilinear3d_route((4, 8, 8), (1, 16, 16), 3, True) == "Staged" and ops.trilinear3d_route((4, 8, 8), (1, 16, 16), 3, False) == "Generic"
    with pytest.raises(RuntimeError):
        ops.trilinear3d_route((4, 0, 8), (8, 16, 16), 3, True)
    with pytest.raises(RuntimeError):
        ops.conv3d_k1_resample_plan((3,) * 4, (4,) * 4, ((4, 5, 7),) * 4, 1, (4, 5, 7))
    with pytest.raises(RuntimeError):
        ops.conv3d_k1_plan(1, 513, 4, 100)


def test_the_clamped_column_is_the_last_one_only():
    """the rows that aim at conv_k1_resample_kernel's `pair` test: i1 == i0 + 1 everywhere but in the last output column"""
    for r in KR_BAD + [q for q in KR_ROWS if q.tag == "ratio" and q.align and q.size == (4, 5, 7) and q.specs[0][2] != q.size]:
        i0, i1, _, _ = lin_tables(r.specs[0][2][2], r.size[2], True)
        assert bool((i1[:-1] == i0[:-1] + 1).all()) and int(i1[-1]) == int(i0[-1]) == r.specs[0][2][2] - 1, kr_id(r)
    i0, i1, _, _ = lin_tables(1, 5, True)                                       # Wi = 1: never a pair
    assert bool((i0 == 0).all()) and bool((i1 == 0).all())


RESTATE = [((2, 3, 7, 9, 13), (4, 5, 7)), ((2, 3, 8, 10, 14), (4, 5, 7)), ((2, 3, 3, 5, 6), (6, 10, 12)), ((1, 2, 5, 7, 9), (13, 15, 40)), ((2, 2, 1, 6, 9), (1, 12, 18)),
           ((2, 2, 3, 4, 16), (1, 8, 32)), ((1, 2, 1, 1, 200), (1, 1, 400)), ((1, 2, 2, 3, 12), (6, 9, 36)), ((1, 2, 4, 6, 1), (8, 12, 5))]


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("shape,size", RESTATE)
def test_restatement_matches_aten(shape, size, align):
    """F.interpolate in fp32 sits inside the interpolation gate around the float64 reference built on lin_tables: the tables are ATen's"""
    x = torch.randn(shape, generator=gen("restate", shape, size))
    tabs = tables(shape[2:], size, align)
    ref, bound = gate_tri(x.double(), tabs, False)
    aten = F.interpolate(x, size, mode="trilinear", align_corners=align)
    worst = float(((aten.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"K1 restatement {shape} -> {size} align={align}: ATen fp32 at {worst:.3f} of the gate")
    assert worst <= 1.0
    assert inside(emu_interp(x, tabs), ref, bound)


def test_device_reference_path_is_the_cpu_one():
    """the million-voxel rows take their float64 reference on the device through the very functions checked here on the CPU (the GPU
    test test_k1_device_reference_equals_cpu_reference compares the two paths' numbers)"""
    r = K1_ROWS[0]._replace(V=4096, big=False)
    c = k1_base_of(r)
    ref, bound = k1_gate(r, c, c["x"])
    want = F.relu(torch.einsum("oc,bcv->bov", c["w"].double(), c["x"].double()) * c["scale"].double().view(1, -1, 1) + c["shift"].double().view(1, -1, 1))
    assert torch.allclose(ref, want, rtol=1e-14, atol=1e-14) and bool((bound > 0).all())


SMALL_K1 = [r for r in list({(r.B, r.cin, r.cout, r.V, r.bf, r.fam, r.bn, r.relu): r for r in K1_ROWS + K1_FAM}.values()) if r.B * r.V <= 4096]


@pytest.mark.parametrize("r", SMALL_K1, ids=k1_id)
def test_k1_yardstick(r):
    c = k1_base_of(r)
    ref, bound = k1_gate(r, c, c["x"])
    got = rnd(emu_k1(c["x"], c["w"], c["scale"] if r.bn else None, c["shift"] if r.bn else None, r.relu), r.bf)
    assert inside(got, ref, bound), k1_id(r)
    aten = F.conv1d(c["x"], c["w"].unsqueeze(2)).double()
    assert inside(aten, *gate_k1(c["x"].double(), c["w"], None, None, False)), k1_id(r)
    if r.fam == "n01" and r.bn and not r.relu:
        assert float((bound / ref.abs().clamp_min(1e-300)).median()) < (2e-2 if r.bf else 1e-5)      # the gate is tight


def test_chain_yardstick():
    for r in CH_FAM + [CH(2, 17, 257, False, True, True, True, False), CH(2, 64, 255, True, True, True, True, True), CH(2, 1, 257, False, False, False, False, False)]:
        c = ch_base(r.B, r.cin, r.V, r.bf, r.fam)
        ref, bound = ch_gate(r, c)
        h = rnd(emu_k1(c["x"], c["w1"], c["s1"] if r.bn1 else None, c["h1"] if r.bn1 else None, r.relu1), r.bf)
        got = rnd(emu_k1(h, c["w2"], c["s2"] if r.bn2 else None, c["h2"] if r.bn2 else None, r.relu2), r.bf)
        assert inside(got, ref, bound), ch_id(r)
        wrong = rnd(emu_k1(h, c["w2"], c["s2"] if r.bn2 else None, c["h2"] if r.bn2 else None, r.relu2, drop=23), r.bf)
        assert not inside(wrong, ref, bound), ch_id(r)


SMALL_KR = [r for r in KR_ROWS + KR_FAM if prod(r.size) <= 4096]


@pytest.mark.parametrize("r", SMALL_KR, ids=kr_id)
def test_k1r_yardstick(r):
    c = kr_base_of(r)
    for i, (ci, co, s) in enumerate(r.specs):
        ref, bound = kr_gate(r, c, i, c["x"][i])
        xi = emu_interp(c["x"][i], tables(s, r.size, r.align))
        got = emu_k1(xi, c["w"][i], c["scale"][i] if r.bn else None, c["shift"][i] if r.bn else None, r.relu)
        assert inside(rnd(got, r.bf and not r.f32out), ref, bound), kr_id(r)


@pytest.mark.parametrize("r", TR_ROWS + TR_FAM, ids=tr_id)
def test_trilinear_yardstick(r):
    x, _ = tr_base(r.B, r.C, r.in_size, r.bf, r.fam, r.bad)
    ref, bound = tr_gate(r, x)
    got = emu_interp(x, tables(r.in_size, r.size, r.align))
    assert inside(rnd(F.relu(got) if r.relu else got, r.bf), ref, bound), tr_id(r)
    if not r.bf:
        aten = F.interpolate(x, r.size, mode="trilinear", align_corners=r.align)
        assert inside(F.relu(aten) if r.relu else aten, ref, bound), tr_id(r)


def emu_strided(r, x, w, sc, sh):
    """conv2d_k3_strided_kernel's chain: input channels in order, the nine taps of each in order, then one fmaf for the BN (F.unfold
    lists a window's elements in exactly that order)"""
    Ho, Wo = (r.H - 1) // r.stride + 1, (r.W - 1) // r.stride + 1
    cols = F.unfold(x, 3, padding=1, stride=r.stride)
    out = emu_k1(cols, w.reshape(r.cout, -1), sc if r.bn else None, sh if r.bn else None, r.relu)
    return out.view(r.B, r.cout, Ho, Wo)


@pytest.mark.parametrize("r", CS_ROWS[:6] + CS_ROWS[-4:] + CS_FAM, ids=cs_id)
def test_strided_yardstick(r):
    x, w, sc, sh = cs_base(r)
    ref, bound = cs_gate(r, x, w, sc, sh)
    assert inside(rnd(emu_strided(r, x, w, sc, sh), r.bf), ref, bound)
    if r.fam == "n01":
        got = F.conv2d(x, w, stride=r.stride, padding=1)                            # ATen's own order
        if r.bn:
            got = fma32(got, sc.view(1, -1, 1, 1), sh.view(1, -1, 1, 1))
        assert inside(rnd(F.relu(got) if r.relu else got, r.bf), ref, bound)
    w2 = w.clone()
    w2[r.cout - 1, r.cin - 1, 2, 2] = 0.0                                       # a wrong kernel: one tap of the last output channel lost
    if r.H > 2 and r.W > 2 and r.fam in ("n01", "offset"):
        assert not inside(rnd(emu_strided(r, x, w2, sc, sh), r.bf), ref, bound)


def emu_cell2d(r, c, xs, drop=None):
    out = 0
    for s, (size_in, (pbn, prelu), bn3) in enumerate(((r.size0, r.pre0, r.bnA), (r.size1, r.pre1, r.bnB))):
        xi = emu_interp(xs[s].unsqueeze(2), tables((1,) + size_in, (1,) + r.size, True))
        sv = emu_k1(xi, c["w1"][s], c["bn1"][s][0] if pbn else None, c["bn1"][s][1] if pbn else None, prelu, drop=drop if s == 0 else None).squeeze(2)
        u = F.conv2d(sv, c["w3"][s], padding=1)
        if bn3:
            u = fma32(u, c["bn3"][s][0].view(1, -1, 1, 1), c["bn3"][s][1].view(1, -1, 1, 1))
        out = out + (F.relu(u) if r.relu else u)
    return out


@pytest.mark.parametrize("r", CE_ROWS + CE_FAM, ids=ce_id)
def test_cell2d_yardstick(r):
    c = ce_base_of(r)
    ref, bound = ce_gate(r, c, c["x"])
    assert inside(emu_cell2d(r, c, c["x"]), ref, bound), ce_id(r)
    if r.fam in ("n01", "offset") and r.cin0 > 1:
        assert not inside(emu_cell2d(r, c, c["x"], drop=min(7, r.cin0 - 1)), ref, bound), ce_id(r)      # the staging lost the last channel of its first U = 8 trip


def named(rows, tag, **kw):
    return next(r for r in rows if r.tag == tag and all(getattr(r, k) == v for k, v in kw.items()))


def test_gates_reject_a_dropped_channel_of_a_trip():
    """the last input channel of a U trip dropped: U = 8 (slabs of 4: Cin = 17 loses channel 7 or 15), UI = 16 (same size: Cin = 17 loses
    channel 15), U = 4 (wider slabs: the 16-wide row's Cin = 5 loses channel 3)"""
    for r, i, drop in ((named(KR_ROWS, "cin_u8", specs=((17, 4, (8, 10, 14)),)), 0, 7), (named(KR_ROWS, "cin_u8", specs=((17, 4, (8, 10, 14)),)), 0, 15),
                       (named(KR_ROWS, "cin_same_u16", specs=((17, 8, (4, 5, 7)),)), 0, 15), (named(KR_ROWS, "slab", nco=16, bf=False), 0, 3)):
        c = kr_base_of(r)
        ref, bound = kr_gate(r, c, i, c["x"][i])
        xi = emu_interp(c["x"][i], tables(r.specs[i][2], r.size, r.align))
        assert inside(emu_k1(xi, c["w"][i], c["scale"][i], c["shift"][i], r.relu), ref, bound)
        assert not inside(emu_k1(xi, c["w"][i], c["scale"][i], c["shift"][i], r.relu, drop=drop), ref, bound), (kr_id(r), drop)
    r = named(K1_ROWS, "small", bf=False)
    c = k1_base_of(r)
    assert not inside(emu_k1(c["x"], c["w"], c["scale"], c["shift"], True, drop=3), *k1_gate(r, c, c["x"]))      # conv_k1_kernel's `unroll 4`


def test_gates_reject_the_neighbours_bn_in_a_ragged_slab():
    """Cout = 25 in slabs of 4 (k1) and of 24 + 1 (resample): the last slab's one channel takes channel 23's scale and shift"""
    r = named(K1_ROWS, "cout", cout=25)
    c = k1_base_of(r)
    sc, sh = c["scale"].clone(), c["shift"].clone()
    sc[24], sh[24] = sc[23], sh[23]
    ref, bound = k1_gate(r, c, c["x"])
    assert inside(emu_k1(c["x"], c["w"], c["scale"], c["shift"], True), ref, bound) and not inside(emu_k1(c["x"], c["w"], sc, sh, True), ref, bound)
    r = named(KR_ROWS, "slab_ragged", B=2, bf=False)
    c = kr_base_of(r)
    sc, sh = c["scale"][0].clone(), c["shift"][0].clone()
    sc[24], sh[24] = sc[23], sh[23]
    xi = emu_interp(c["x"][0], tables(r.specs[0][2], r.size, True))
    ref, bound = kr_gate(r, c, 0, c["x"][0])
    assert inside(emu_k1(xi, c["w"][0], c["scale"][0], c["shift"][0], True), ref, bound) and not inside(emu_k1(xi, c["w"][0], sc, sh, True), ref, bound)


def test_gates_reject_swapped_weights_and_an_unclamped_tap():
    """w0 / w1 swapped on one axis, on the trilinear rows of both routes and on a resample row; the clamped i1 read as (i0 + 1) modulo
    the row.  Under align_corners = 1 the clamped column has lambda == 0 exactly, so that mutant cannot show on finite data: there
    it is the non-finite row with the element in column 0 that holds it (0 * Inf reaches the last column).  Under align_corners = 0
    an up-sampling clamps with lambda > 0 and the last column, and only it, leaves the gate."""
    for r in (named(TR_ROWS, "tile_edge"), named(TR_ROWS, "down", align=True), named(TR_ROWS, "x2", align=False)):
        x, _ = tr_base(r.B, r.C, r.in_size, r.bf, r.fam, r.bad)
        tabs = tables(r.in_size, r.size, r.align)
        ref, bound = tr_gate(r, x)
        assert inside(emu_interp(x, tabs), ref, bound)
        for dim in (2, 3, 4):
            assert not inside(emu_interp(x, tabs, swap_axis=dim), ref, bound), (tr_id(r), dim)
        if r.align:
            assert inside(emu_interp(x, tabs, wrap_i1=True), ref, bound), tr_id(r)
            xi = x.clone()
            xi[1, 1, :, :, 0] = INF
            assert bool(torch.isfinite(emu_interp(xi, tabs)[..., -1]).all()) and not bool(torch.isfinite(emu_interp(xi, tabs, wrap_i1=True)[1, 1, ..., -1]).any())
        else:
            ok = (emu_interp(x, tabs, wrap_i1=True).double() - ref).abs() <= bound
            assert bool(ok[..., :-1].all()) and not bool(ok[..., -1].any()), tr_id(r)     # only the clamped column shows it, and all of it does
    for r in (named(KR_ROWS, "ratio", specs=((3, 12, (7, 9, 13)),), align=True), named(KR_ROWS, "ratio", specs=((5, 12, (3, 5, 6)),), align=False)):
        c = kr_base_of(r)
        tabs = tables(r.specs[0][2], r.size, r.align)
        ref, bound = kr_gate(r, c, 0, c["x"][0])
        for kw in ({"swap_axis": 2}, {"swap_axis": 3}, {"swap_axis": 4}) + (() if r.align else ({"wrap_i1": True},)):
            assert not inside(emu_k1(emu_interp(c["x"][0], tabs, **kw), c["w"][0], c["scale"][0], c["shift"][0], True), ref, bound), (kr_id(r), kw)


def test_gates_reject_an_untransposed_weight():
    r = named(K1_ROWS, "transposed", V=777)
    c = k1_base_of(r)
    ref, bound = k1_gate(r, c, c["x"])
    wt = c["w"].t().contiguous()                                                  # what the kernel is handed: [Cin][Cout]
    assert inside(emu_k1(c["x"], wt.t(), c["scale"], c["shift"], True), ref, bound)
    assert not inside(emu_k1(c["x"], wt.view(r.cout, r.cin), c["scale"], c["shift"], True), ref, bound)


def test_gates_reject_contracted_lambdas():
    """Lambdas taken from a fused scale * dst - i0 are MORE accurate than ATen's and differ from the reference's by up to 2^-24 * src:
    an output moves by that times |b - a|, against a gate of 3 * 2^-23 * A.  The gate sees it on every fp32 row whose scale is no
    dyadic fraction, at the sweep's own sizes (src of 4 .. 16) as on the 200 -> 400 row; where scale * dst is exact in fp32 (15 / 32,
    3 / 8, 2, 0.5) the two lambdas are the same bits and there is nothing to see.  tests/test_hip_parity.py::
    test_trilinear_bit_identical_to_aten_cpu holds the same property on the device bit for bit."""
    x = torch.randn((1, 2, 1, 1, 200), generator=gen("lambda"))
    ref, bound = gate_tri(x.double(), tables((1, 1, 200), (1, 1, 400), True), False)
    assert inside(emu_interp(x, tables((1, 1, 200), (1, 1, 400), True)), ref, bound)
    assert not inside(emu_interp(x, tables((1, 1, 200), (1, 1, 400), True, contracted=True)), ref, bound)
    seen = 0
    for r in TR_ROWS:
        xr, _ = tr_base(r.B, r.C, r.in_size, r.bf, r.fam, r.bad)
        got = emu_interp(xr, tables(r.in_size, r.size, r.align, contracted=True))
        rejected = not inside(rnd(F.relu(got) if r.relu else got, r.bf), *tr_gate(r, xr))
        seen += rejected
        if r.tag in ("x2_channels", "tile_exact", "depth1_out", "depth1", "x3", "noninteger_up", "axis_unchanged", "up_less_than_2"):
            assert rejected, tr_id(r)
        if r.tag in ("tile_edge", "relu", "down"):
            assert not rejected and torch.equal(got, emu_interp(xr, tables(r.in_size, r.size, r.align))), tr_id(r)
    print(f"K1 contracted-lambda mutant rejected on {seen} of {len(TR_ROWS)} sweep rows")


def test_strided_shared_memory_limit_is_refused_before_any_launch():
    """Cout * Cin * 9 + 2 * Cout floats above 48 KB: RAGMI_EUNSUPPORTED from the host checks alone (fake, never dereferenced pointers)"""
    import rag_amd
    lib = rag_amd.load_library()
    fake = ctypes.c_void_p(4096)
    assert (64 * 22 * 9 + 128) * 4 > 48 * 1024 >= (64 * 21 * 9 + 128) * 4
    assert lib.ragmi_conv2d_k3_strided_fwd(fake, fake, None, None, 1, fake, 1, 22, 64, 8, 8, 2, 0, None) == -2
    assert b"too large" in lib.ragmi_last_error()
    assert lib.ragmi_conv2d_k3_strided_fwd(fake, fake, fake, None, 1, fake, 1, 3, 4, 8, 8, 2, 0, None) == -1      # scale without shift


def cs_base(r):
    g = gen("strided", r.cin, r.cout, r.H, r.W, r.stride, r.fam)
    x = rnd(make_x((r.B, r.cin, r.H, r.W), r.fam, g, unit=32), r.bf)
    w = torch.randn((r.cout, r.cin, 3, 3), generator=g) * 0.2
    if r.fam == "offset":
        w -= w.mean(dim=(1, 2, 3), keepdim=True)                                   # cancelling sums
    elif r.fam == "spread":
        w *= torch.exp2(torch.rand(w.shape, generator=g) * 40 - 20)
    sc, sh = make_bn(r.cout, g)
    return x, w, sc, sh


def cs_gate(r, x, w, sc, sh):
    pre = F.conv2d(x.double(), w.double(), stride=r.stride, padding=1)
    mag = F.conv2d(x.double().abs(), w.double().abs(), stride=r.stride, padding=1)
    ref, b = bn_act(pre, (9 * r.cin + 1) * E24 * mag, sc if r.bn else None, sh if r.bn else None, r.relu)
    return ref, stored(r.bf, ref, b)


# --------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gops():
    import rag_amd
    rag_amd.load_library()
    return rag_amd.ops


def nan_buf(shape, dt):
    return torch.full(shape, NAN, device=DEV, dtype=dt)


def sliced(x, dt, on):
    """x on the device, as a channel slice at offset 3 of a NaN buffer when `on`"""
    if not on:
        return x.to(DEV, dt)
    xb = nan_buf((x.shape[0], x.shape[1] + 6) + tuple(x.shape[2:]), dt)
    xb[:, 3:3 + x.shape[1]] = x.to(DEV, dt)
    return xb[:, 3:3 + x.shape[1]]


def taken(buf, spans, tag):
    """the destination slices of buf (ch0, n), after checking that every other channel still holds its NaN"""
    keep = {ch for ch0, n in spans for ch in range(ch0, ch0 + n)}
    rest = [ch for ch in range(buf.shape[1]) if ch not in keep]
    assert bool(torch.isnan(buf[:, rest]).all()), (tag, "a store left its destination")
    return [buf[:, ch0:ch0 + n] for ch0, n in spans]


def g32(t):
    return None if t is None else t.to(DEV).contiguous()


def run_k1(ops, r, c):
    dt = tdt(r.bf)
    x = sliced(c["x"], dt, r.sl)
    ch0 = 3 if r.sl else GUARD
    buf = nan_buf((r.B, ch0 + r.cout + GUARD, r.V), dt)
    w = g32(c["w"].t()) if r.tr else g32(c["w"])
    ops.conv3d_k1(x, w, g32(c["scale"]) if r.bn else None, g32(c["shift"]) if r.bn else None, r.relu, buf, ch0, transposed=r.tr)
    torch.cuda.synchronize()
    return taken(buf, [(ch0, r.cout)], k1_id(r))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("r", K1_ROWS + K1_FAM, ids=k1_id)
def test_k1(gops, r):
    c = k1_base_of(r)
    got = run_k1(gops, r, c)
    ref, bound = k1_gate(r, c, c["x"], DEV if r.big else "cpu")
    check(k1_id(r), f"conv_k1<{'bf16' if r.bf else 'f32'},{r.nco},{int(r.vec)}>", got, ref, bound)


@pytest.mark.gpu
def test_k1_device_reference_equals_cpu_reference(gops):
    r = named(K1_ROWS, "slab", V=100000, bf=False)
    c = k1_base_of(r)
    (rc, bc), (rd, bd) = k1_gate(r, c, c["x"]), k1_gate(r, c, c["x"], DEV)
    assert torch.allclose(rd.cpu(), rc, rtol=1e-13, atol=1e-13) and torch.allclose(bd.cpu(), bc, rtol=1e-12, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("r", K1_BAD, ids=k1_id)
def test_k1_non_finite(gops, r):
    c = k1_base_of(r)
    got = run_k1(gops, r, c).cpu()
    reach = torch.zeros(got.shape, dtype=torch.bool)
    reach[1, :, r.bad[1][0]] = True
    check_reach(k1_id(r), "conv_k1", got, reach, lambda: k1_gate(r, c, c["xz"]), lambda: k1_gate(r, c, c["x"]), r.bad[0], r.relu)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CH_ROWS + CH_FAM, ids=ch_id)
def test_k1_chain(gops, r):
    c = ch_base(r.B, r.cin, r.V, r.bf, r.fam)
    dt = tdt(r.bf)
    x = c["x"].to(DEV, dt)
    bn = lambda on, s, h: (g32(c[s]), g32(c[h])) if on else (None, None)      # noqa: E731
    (s1, h1), (s2, h2) = bn(r.bn1, "s1", "h1"), bn(r.bn2, "s2", "h2")
    buf = nan_buf((r.B, 3 + 12 + GUARD, r.V), dt)
    gops.conv3d_k1_chain(x, g32(c["w1"]), s1, h1, r.relu1, g32(c["w2"]), s2, h2, r.relu2, buf, 3)
    mid, two = torch.empty((r.B, 24, r.V), device=DEV, dtype=dt), torch.empty((r.B, 12, r.V), device=DEV, dtype=dt)
    gops.conv3d_k1(x, g32(c["w1"]), s1, h1, r.relu1, mid)
    gops.conv3d_k1(mid, g32(c["w2"]), s2, h2, r.relu2, two)
    torch.cuda.synchronize()
    got = taken(buf, [(3, 12)], ch_id(r))[0]
    assert torch.equal(got, two), (ch_id(r), "not the bits of two conv3d_k1 calls")
    check("chain_" + ch_id(r), f"conv_k1_chain<{'bf16' if r.bf else 'f32'}>", got, *ch_gate(r, c))


def run_k1r(ops, r, c):
    """the outputs of the row's descriptors, on the device"""
    dt, odt = tdt(r.bf), tdt(r.bf and not r.f32out)
    xs = [x.to(DEV, dt) for x in c["x"]]
    bn = [(g32(c["scale"][i]), g32(c["shift"][i])) if r.bn else (None, None) for i in range(len(xs))]
    couts = [s[1] for s in r.specs]
    if r.form == "single":
        buf = nan_buf((r.B, 3 + couts[0] + GUARD) + r.size, odt)
        ops.conv3d_k1_resample(xs[0], r.size, r.align, g32(c["w"][0]), bn[0][0], bn[0][1], r.relu, buf, 3)
        torch.cuda.synchronize()
        return taken(buf, [(3, couts[0])], kr_id(r))
    if r.form == "pair":
        spans = [(GUARD, couts[0]), (GUARD + couts[0] + 3, couts[1])]
        buf = nan_buf((r.B, spans[1][0] + couts[1] + GUARD) + r.size, odt)
        ops.conv3d_k1_resample_pair([(xs[i], g32(c["w"][i]), bn[i][0], bn[i][1], r.relu, spans[i][0]) for i in range(2)], r.size, buf)
        torch.cuda.synchronize()
        return taken(buf, spans, kr_id(r))
    bufs = [nan_buf((r.B, GUARD + i + co + GUARD) + r.size, odt) for i, co in enumerate(couts)]
    ops.conv3d_k1_resample_multi([(xs[i], g32(c["w"][i]), bn[i][0], bn[i][1], r.relu, bufs[i], GUARD + i) for i in range(len(xs))], r.size)
    torch.cuda.synchronize()
    return [taken(b, [(GUARD + i, co)], kr_id(r))[0] for i, (b, co) in enumerate(zip(bufs, couts))]


@pytest.mark.gpu
@pytest.mark.parametrize("r", KR_ROWS + KR_FAM, ids=kr_id)
def test_k1_resample(gops, r):
    c = kr_base_of(r)
    outs = run_k1r(gops, r, c)
    dev = DEV if prod(r.size) >= 1 << 16 else "cpu"
    for i, got in enumerate(outs):
        check(f"{kr_id(r)}:{i}", f"conv_k1_resample<{'bf16' if r.bf else 'f32'},{r.nco}>", got, *kr_gate(r, c, i, c["x"][i], dev))


@pytest.mark.gpu
@pytest.mark.parametrize("r", KR_BAD, ids=kr_id)
def test_k1_resample_non_finite(gops, r):
    c = kr_base_of(r)
    outs = run_k1r(gops, r, c)
    ci, co, s = r.specs[0]
    ind = torch.zeros((r.B, 1) + s, dtype=F64)
    ind[(1, 0) + r.bad[1]] = 1.0
    reach = tap_reach(ind, tables(s, r.size, True)).expand(r.B, co, *r.size)
    check_reach(kr_id(r), "conv_k1_resample", outs[0], reach, lambda: kr_gate(r, c, 0, c["xz"][0]), lambda: kr_gate(r, c, 0, c["x"][0]), r.bad[0], r.relu)
    for i in range(1, len(outs)):                                                    # the partner of a paired launch never sees it
        check(f"{kr_id(r)}:{i}", "conv_k1_resample", outs[i], *kr_gate(r, c, i, c["x"][i]))


def run_tri(ops, r, x):
    dt = tdt(r.bf)
    if r.plain:
        out = ops.trilinear3d(x.to(DEV, dt), r.size, r.align)
        torch.cuda.synchronize()
        return out
    ch0 = 3 if r.sl else GUARD
    buf = nan_buf((r.B, ch0 + r.C + GUARD) + r.size, dt)
    ops.trilinear3d_act(sliced(x, dt, r.sl), r.size, r.align, r.relu, buf, ch0)
    torch.cuda.synchronize()
    return taken(buf, [(ch0, r.C)], tr_id(r))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("r", TR_ROWS + TR_FAM, ids=tr_id)
def test_trilinear(gops, r):
    x, _ = tr_base(r.B, r.C, r.in_size, r.bf, r.fam, r.bad)
    check(tr_id(r), f"trilinear<{'bf16' if r.bf else 'f32'},{r.route}>", run_tri(gops, r, x), *tr_gate(r, x))


@pytest.mark.gpu
@pytest.mark.parametrize("r", TR_BAD, ids=tr_id)
def test_trilinear_non_finite(gops, r):
    x, xz = tr_base(r.B, r.C, r.in_size, r.bf, r.fam, r.bad)
    got = run_tri(gops, r, x)
    ind = torch.zeros((r.B, r.C) + r.in_size, dtype=F64)
    ind[(1, 1) + r.bad[1]] = 1.0
    reach = tap_reach(ind, tables(r.in_size, r.size, r.align))
    check_reach(tr_id(r), f"trilinear<{r.route}>", got, reach, lambda: tr_gate(r, xz), lambda: tr_gate(r, x), r.bad[0], r.relu)


@pytest.mark.gpu
@pytest.mark.parametrize("r", AD_ROWS, ids=lambda r: f"{r.tag}_b{r.B}c{r.C}v{r.V}_{'bf16' if r.bf else 'f32'}")
def test_add_is_exact(gops, r):
    dt, g = tdt(r.bf), gen("add", r.tag, r.V)
    a, b = torch.randn((r.B, r.ca, r.V), generator=g).to(dt), (torch.randn((r.B, r.cb, r.V), generator=g) * 3).to(dt)
    buf = nan_buf((r.B, r.cy, r.V), dt)
    ad = a.to(DEV)
    if r.tag == "scalar_misaligned_base":                                           # every size a multiple of four, the pointer one element off
        ad = torch.empty(a.numel() + 1, device=DEV, dtype=dt)[1:].view(a.shape).copy_(ad)
        assert ad.data_ptr() % (4 * ad.element_size()) != 0
    gops.add(ad, r.a0, b.to(DEV), r.b0, buf, r.y0, r.C)
    torch.cuda.synchronize()
    got = taken(buf, [(r.y0, r.C)], r.tag)[0].cpu()
    assert torch.equal(got, a[:, r.a0:r.a0 + r.C] + b[:, r.b0:r.b0 + r.C]), r.tag
    print(f"K1 case={r.tag} inst=add<{'bf16' if r.bf else 'f32'}> worst=0/0 = 0.000")


@pytest.mark.gpu
@pytest.mark.parametrize("r", CS_ROWS + CS_FAM, ids=cs_id)
def test_conv2d_k3_strided(gops, r):
    x, w, sc, sh = cs_base(r)
    got = gops.conv2d_k3_strided(x.to(DEV, tdt(r.bf)), g32(w), g32(sc) if r.bn else None, g32(sh) if r.bn else None, r.relu, r.stride)
    torch.cuda.synchronize()
    check("strided_" + cs_id(r), f"conv2d_k3_strided<{'bf16' if r.bf else 'f32'},12>", got, *cs_gate(r, x, w, sc, sh))


def run_cell2d(ops, r, c):
    ng = r.cout // 4
    gch = [8 * ((g + 1) % ng) for g in range(ng)] if r.perm else None             # every other group of the span stays unused
    span = 8 * ng - 4 if r.perm else r.cout
    buf = nan_buf((r.B, span + 2 * GUARD) + r.size, torch.float32)
    out = buf[:, GUARD:GUARD + span]
    dest = [GUARD + (gch[co // 4] if gch else 4 * (co // 4)) + co % 4 for co in range(r.cout)]
    pre = [(g32(c["w1"][s]), g32(c["bn1"][s][0]) if pbn else None, g32(c["bn1"][s][1]) if pbn else None, prelu) for s, (pbn, prelu) in enumerate((r.pre0, r.pre1))]
    pk = [ops.conv3d_k3_pack(g32(w)) for w in c["w3"]]
    bn3 = [(g32(c["bn3"][s][0]), g32(c["bn3"][s][1])) if on else (None, None) for s, on in enumerate((r.bnA, r.bnB))]
    with ops.conv_precision("f16x3"):
        ops.cell2d(c["x"][0].to(DEV), pre[0], c["x"][1].to(DEV), pre[1], r.C, pk[0], bn3[0][0], bn3[0][1], pk[1], bn3[1][0], bn3[1][1], r.cout, r.relu, out, gch)
    torch.cuda.synchronize()
    full = buf.cpu()
    rest = [ch for ch in range(full.shape[1]) if ch not in dest]
    assert bool(torch.isnan(full[:, rest]).all()), (ce_id(r), "a store left the destination groups")
    return full[:, dest]


@pytest.mark.gpu
@pytest.mark.parametrize("r", CE_ROWS + CE_FAM, ids=ce_id)
def test_cell2d(gops, r):
    c = ce_base_of(r)
    check(ce_id(r), f"cell2d_x3<{r.C // 4}>", run_cell2d(gops, r, c), *ce_gate(r, c, c["x"]))


@pytest.mark.gpu
@pytest.mark.parametrize("r", CE_BAD, ids=ce_id)
def test_cell2d_non_finite(gops, r):
    c = ce_base_of(r)
    got = run_cell2d(gops, r, c)
    ind = torch.zeros((r.B, 1, 1) + r.size0, dtype=F64)
    ind[(1, 0, 0) + r.bad[1]] = 1.0
    staged = tap_reach(ind, tables((1,) + r.size0, (1,) + r.size, True)).squeeze(2).double()
    reach = (F.conv2d(staged, torch.ones((1, 1, 3, 3), dtype=F64), padding=1) > 0).expand(r.B, r.cout, *r.size)
    assert reach.any() and not reach[0].any() and reach.sum() <= reach.numel() // 8
    xz = [c["xz"][0], c["x"][1]]
    check(ce_id(r), "cell2d_x3", torch.where(reach, torch.zeros_like(got), got), *ce_gate(r, c, xz), where=~reach)
    inside_v, fin = got[reach].double(), torch.isfinite(got[reach])
    ok = torch.zeros_like(fin)
    if r.bad[0] == 3e38:                                                             # finite: the float64 result WITH the element, inside its gate
        want, wb = ce_gate(r, c, c["x"])
        ok |= (inside_v - want[reach]).abs() <= wb[reach]
    if r.relu:                                                                       # set A's non-finite pre-activation stored as +0: act(u_B) alone
        other, ob = ce_gate(r, c, xz, sets=(1,))
        ok |= (inside_v - other[reach]).abs() <= ob[reach]
    assert bool(ok[fin].all()), (ce_id(r), "a finite wrong value inside the reach")
