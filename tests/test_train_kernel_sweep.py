"""Sweep of the training-step kernels without a forward twin (rag_amd/csrc/train.hip): train-mode BatchNorm statistics, the BN + ReLU
pass and its adjoint, the 3x3x3 / 1x1x1 / strided 2-D weight gradients and the adjoints of the trilinear resample and the cost
volume, against float64 on the CPU computed from the very fp32 tensors the kernel reads.  U = 2^-24 below.

Gates, per element, nothing excused (a bound of zero demands the exact value):
    reductions     |got - ref64| <= (L + 8) * U * Y,  Y = the float64 sum of the |terms|, L = the longest sequential fp32 chain:
        BN sums          L = 4 * ceil(DHW / (1024 * gx)) + 8   (a thread's quads, the 256-wide tree; the partials are added in double)
        3x3x3 wgrad      L = 32 * ceil(ntiles / gx) + 4 + ceil(gx / 64) + 6   (MFMA steps of a tile x trips, the lane shuffles, the
                         reduce kernel's stride over gx partials and its shuffles); gx read from the workspace query on the GPU, and
                         taken as ntiles (the shortest chain possible) by the CPU self-check.  One rounding per MFMA step sufficed.
        1x1x1 wgrad      L = ceil(DHW / (256 * gx)) + 6 + 2 + gx * B   (a thread's voxels, shuffles, the 4 waves, the atomics)
        strided wgrad    L = ceil(B * Ho * Wo / (256 * gx)) + 8 + gx;   strided dgrad  L = 9 * Cout
        trilinear adj.   L = the taps of an input voxel (product over the axes of <= 2 * ceil(out / in) + 2); plus, per axis,
                         2^-23 * (in - 1) times the adjoint of |dy| with that axis' two tap weights set to 1, for the
                         interpolation weight being formed in fp32 (an absolute error in lambda: see tri_case)
        cost volume adj. L = d
    elementwise    |got - ref64| <= 4 * U * (sum of the |terms| in float64)      (three roundings)
BatchNorm yardsticks are centred: they are built from x - mean64, so none loosens as |mean| / std grows (y excepted, see there).
    mean           4 U (|mean64| + E|x - mean64|)
    variance       Bvar = 3 (L + 8) U (var64 + (mean64 - K)^2), K = x[0, c, 0], the pivot bn_stats_kernel documents (q / n carries
                   (L + 8) U of its terms, (s / n)^2 twice that of |mean64 - K| E|x - K|); invstd, scale, running_var and shift take
                   the propagated bound + 4 U of their own terms.  Independently invstd, scale and running_var are within 1e-5
                   relative of float64 on EVERY BN row (eps term as reference; a constant channel gives invstd = eps^-1/2).
                   For running_var the 1e-5 is relative to the blended value (1 - m) old + m (var + eps): only the momentum = 1
                   rows hold the batch variance itself to 1e-5 (at m = 0.1 one rounding of an fp32 running_var near 1 is
                   already 6e-5 of a variance of 0.01); at lower momentum the derived gate is the check.
    y              against act(x * scale + shift) (+ res) evaluated in float64 from the fp32 (scale, shift) the call returned, to
                   4 U (|x scale| + |shift| + |res|): the forward's contract is that fma (the adjoint re-derives its mask from it),
                   and scale / shift themselves are held to the centred gates above.  A constant channel gives act(beta) to that gate.
                   y is ALSO held to the float64 batch norm itself (y_true_gate), to the same 4 U (|x scale64| + |shift64| + |res|)
                   plus what the statistics' centred bounds let through: |x - mean64| Bscale + |scale64| Bmean.
                   (A y gate centred on x - mean64 is out of reach of ANY fp32 shift: rounding shift = beta - mean scale once
                   moves y by 2^-25 |mean scale|, far above 4 U |x - mean| |scale| at |mean| / std = 1000.  ATen's fp32 forward
                   is the same x alpha + beta: test_bn_gates_hold_for_aten_fp32 shows it inside y_true_gate on every row and
                   outside the centred 4 U (|x - mean64| |scale64| + |beta|) on every conditioning row.)
                   ragmi_bn_act_fwd (eval path; scale and shift are its inputs) runs on every row from the returned statistics,
                   through the same views, to the same gate, and gives the fused launch's y bit for bit.
    adjoint        (dy, x, scale, shift, mean, invstd) are all fp32 INPUTS of ragmi_bn_act_bwd, so the float64 reference uses those
                   values: g = dy [x scale + shift > 0], dgamma = invstd sum g (x - mean), dbeta = sum g,
                   dx = g c1 + (x - mean) c2 + c3.  dgamma: Y = invstd sum |g| |x - mean|; dbeta: Y = sum |g|;
                   dx: 4 U (|g c1| + |x - mean| |c2| + |scale mean(g)|) + the two reduction bounds carried through c2 and c3
                   (|x - mean| |scale| invstd^2 Bsgx / n + |scale| Bsg / n): a masked element has g = 0 and nothing else to hide
                   the sums' error behind.  The split pair coeffs + apply is held to the same gate.
ReLU knife edge: an fp32 fma is exactly rounded, so its sign is the sign of the float64 value of the same fp32 operands and the
reference's mask is the kernel's.  The rows still keep every float64 pre-activation outside 8 U (|x scale| + |shift|) of zero
(test_no_relu_knife_edge): elements drawn inside the band are redrawn when the row is built — at |mean| / std = 1000 the band holds
about three of 4096 elements, so no seed is free of them.  The eval-path row with integer x, scale 1, shift -2 has exact zeros: y = 0
and zero gradient there.

Rows (module-level tables below): BN shapes from less than one quad to B > 256 (reduce_blocks = 1, more than 256 partials) and
(16, 256, 1, 1, 1028) and (258, 1, 1, 1, 3076), whose grids are capped at 1 so that threads go round the two-quads-per-trip loop:
one double trip and nothing after it, and a double trip followed by the single-quad tail (thread 0: two double trips); the
conditioning matrix (mean, std) in {(0.5, 2), (10, 1), (100, 1), (1000, 1), (-100, 0.1)} plus a constant channel, mixed over the
channels of one launch (the 5-channel shape runs two mixes, the second with the constant channel); channel-slice views,
y_ch0 / res_ch0 / dy_ch0 > 0, out=, a base pointer off by one float, guard channels bit-identical; momentum {0, 0.1, 1}, absent
running statistics, num_batches_tracked, accumulate.  3x3x3 wgrad: Cin x Cout matrix
(CG 1..4, gz > 1) on a vector and a scalar geometry, geometry matrix around the 2 x 8 x 32 tile, a Cin = Cout = 48 row whose
persistent workgroups take >= 3 trips with a ragged last one, `into` over 1, 2, 3, 8 destinations, planar2d, g_ch0, x slices.
1x1x1 wgrad: Cin x Cout x DHW x B, twice per row.  Strided stem: stride x (H, W) x channels x B.  Trilinear adjoint: the per-axis
pairs 1-1, 1-5, 5-1, 2-7, 7-2, 4-8, 8-4, 4-12, 12-4, 5-5 and 3 -> 200 / 200 -> 3 (more than four taps: the generic loop) and a
cpt > 1 row.  Cost volume adjoint: w < d, w = d, w = 1, hw around 256.

What the sweep found: bn_stats_kernel summed x and x^2 raw and bn_finalize* formed q / n - mean^2, which cancels like (mean / std)^2
(relative variance error up to 8e-2 in the conditioning matrix); the adjoint formed sum g x - mean sum g and x c2 + c3 with the same
cancellation one power lower.  The sums are taken about the pivot K and about the mean now, dx is g c1 + (x - mean) c2 + c3.

Every GPU row prints `TRAIN case=... worst=err/bound` (the 1x1x1 and strided matrices one line per parametrised case, with the
row that set it).  Measured on the MI355X, worst err / bound per family:
  BN statistics    mean 0.248 (16x256x1x1x1028), invstd 0.228, scale 0.389, shift 0.177 (2x5x3x7x9, the mix with the constant
                   channel); flat relative error of invstd on the 12-channel conditioning launch 2.2e-7 at most (gate 1e-5)
  BN forward       y 0.250, y + res 0.476 (258x1x1x1x3076), bn_act the same (bit-identical); views 0.248 / 0.436
  running stats    mean 0.235, var 0.300 (momentum 0.1)
  BN adjoint       dx 0.147 train (conditioning matrix) / 0.250 eval, dgamma 0.046, dbeta 0.050; accumulate 0.015; views dx 0.247
  3x3x3 wgrad      channel matrix 0.012 (i24 o16), geometry 0.032 (B1 i5 o5 5x3x2), into 0.013 (n = 8), planar 0.011,
                   persistent trips 0.001 (H = 16: gx = 7, 32 tiles)   1x1x1 wgrad  0.118 (i48 o24, DHW 1, B 3)
  strided stem     dgrad 0.084 (stride 1, 36x60), wgrad 0.108 (stride 3, 9x9)
  trilinear adj.   0.410 (200x5x4 -> 3x5x8, align_corners = False)    cost volume adj.  left 0.170, right 0.152
The library of the parent commit, run through the conditioning matrix by the entry points whose ABI it shares (statistics, fused
adjoint, running statistics): invstd off by 2.3e-4 .. 5.4e-4 relative at mean 100 / std 1, 5.6e-3 .. 1.7e-2 at 1000 / 1, up to 2.7e-2
at -100 / 0.1 and by 65 .. 90 % on the constant channel (its variance came out far from 0); dx at 2.4 .. 6.9 of its bound, dgamma of
the constant channel nonzero; test_bn_running_statistics failed on every conditioning row with momentum > 0.

Unmarked tests run without a GPU; the rest need the MI355X."""
import functools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import matching_oracle as O

DEV = "cuda:0"
U = 2.0 ** -24
EPS = 1e-5
SENT = -12345.678

def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def gen(*key):
    return torch.Generator().manual_seed(seed_of(*key))


def ceil_div(a, b):
    return -(-a // b)


def check(tag, got, ref, bound, quiet=False):
    """every element inside its bound (exact where the bound is zero); prints and returns the worst err / bound"""
    g64 = torch.as_tensor(got).detach().cpu().double().reshape(ref.shape)
    assert torch.isfinite(g64).all(), (tag, "non-finite output")
    err = (g64 - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    zero = bound == 0
    assert bool((err[zero] == 0).all()), (tag, "inexact where the bound is zero")
    ratio = torch.where(zero, torch.zeros_like(err), err / bound.clamp_min(1e-300)).reshape(-1)
    k = int(ratio.argmax()) if ratio.numel() else 0
    worst = float(ratio[k]) if ratio.numel() else 0.0
    if not quiet:
        print(f"TRAIN case={tag} worst={float(err.reshape(-1)[k]):.3e}/{float(bound.reshape(-1)[k]):.3e} = {worst:.3f}")
    assert worst <= 1.0, (tag, worst)
    return worst


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


# =========================================================================== BatchNorm rows
BN_SHAPES = ((1, 2, 1, 1, 5), (2, 3, 2, 2, 1), (2, 5, 3, 7, 9), (1, 12, 8, 16, 32), (2, 4, 4, 16, 36), (3, 4, 1, 5, 1027), (300, 2, 1, 2, 2),
             (16, 256, 1, 1, 1028),       # B * C = 4096 caps gx at 1: thread 0 takes one double trip of the two-quad loop, no tail
             (258, 1, 1, 1, 3076))        # B > 256 caps gx at 1: three quads per thread (double trip + tail), four for thread 0
COND_SHAPES = ((2, 5, 3, 7, 9), (1, 12, 8, 16, 32))
COND_SPECS = ((0.5, 2.0), (10.0, 1.0), (100.0, 1.0), (1000.0, 1.0), (-100.0, 0.1), (100.1, 0.0))     # std 0: the constant channel
PLAIN = ((0.5, 2.0),)
# "cond": channel c takes COND_SPECS[c % 6] (5 channels: the five (mean, std); 12: all six twice); "condk": the same from spec 3 on,
# which gives the 5-channel shape its constant channel
BN_ROWS = tuple((s, "plain") for s in BN_SHAPES) + tuple((s, "cond") for s in COND_SHAPES) + ((COND_SHAPES[0], "condk"),)
VIEW_SHAPES = ((2, 4, 4, 16, 36), (2, 5, 3, 7, 9))        # DHW % 4 == 0 and != 0


def bn_gx(B, C, dhw):
    """reduce_blocks of train.hip"""
    return max(1, min(ceil_div(4096, B * C), ceil_div(dhw, 1024), max(1, 256 // B)))


def bn_chain(B, C, dhw):
    return 4 * ceil_div(dhw, 1024 * bn_gx(B, C, dhw)) + 8


def channel_spec(kind, C, c):
    if kind == "plain":
        return PLAIN[0]
    return COND_SPECS[(c + (3 if kind == "condk" else 0)) % len(COND_SPECS)]


def stats64(x, gamma, beta):
    B, C = x.shape[:2]
    x64 = x.double().transpose(0, 1).reshape(C, -1)
    n = x64.shape[1]
    mean = x64.mean(dim=1)
    xc = x64 - mean[:, None]
    var = (xc * xc).mean(dim=1)
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma.double() * invstd
    return {"n": n, "mean": mean, "var": var, "invstd": invstd, "scale": scale, "shift": beta.double() - mean * scale,
            "mad": xc.abs().mean(dim=1), "K": x64[:, 0].clone(), "varu": var * (n / max(n - 1, 1))}


def v5(t):
    return t.reshape(1, -1, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def bn_case(shape, kind, relu):
    """Inputs of a BN row (fp32, shared, never modified) with their float64 statistics.  With relu, elements whose float64
    pre-activation falls inside the knife-edge band are redrawn from their channel's distribution until none is left."""
    B, C = shape[:2]
    g = gen("bn", shape, kind)
    x = torch.empty(shape)
    specs = [channel_spec(kind, C, c) for c in range(C)]
    for c, (m, s) in enumerate(specs):
        x[:, c] = m + s * torch.randn((B,) + shape[2:], generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    for c, (m, s) in enumerate(specs):
        if s == 0.0:
            beta[c] = 0.25 if c % 2 else -0.25          # a constant channel's y is act(beta): keep it off zero
    dy = torch.randn(shape, generator=g)
    res = torch.randn(shape, generator=g)
    redrawn = 0
    for _ in range(50):
        st = stats64(x, gamma, beta)
        if not relu:
            break
        hit = knife_edge(x, st)
        if not hit.any():
            break
        redrawn += int(hit.sum())
        for c, (m, s) in enumerate(specs):
            h = hit[:, c]
            if h.any():
                x[:, c][h] = m + s * torch.randn(int(h.sum()), generator=g)
    return {"shape": shape, "kind": kind, "x": x, "gamma": gamma, "beta": beta, "dy": dy, "res": res, "st": st, "specs": specs,
            "redrawn": redrawn}


def knife_edge(x, st):
    """elements whose float64 pre-activation lies within 8 U (|x scale| + |shift|) of zero"""
    xs = x.double() * v5(st["scale"])
    pre = xs + v5(st["shift"])
    return pre.abs() <= 8 * U * (xs.abs() + v5(st["shift"]).abs())


def fwd_stat_bounds(c):
    """centred bounds of (mean, invstd, scale, shift, var) of a row"""
    st = c["st"]
    B, C = c["shape"][:2]
    L = bn_chain(B, C, st["n"] // B)
    bmean = 4 * U * (st["mean"].abs() + st["mad"])
    bvar = 3 * (L + 8) * U * (st["var"] + (st["mean"] - st["K"]) ** 2)
    rel = 0.5 * bvar / (st["var"] + EPS)
    binv = st["invstd"] * (rel + 4 * U)
    bscale = st["scale"].abs() * (rel + 4 * U)
    bshift = 4 * U * (c["beta"].double().abs() + (st["mean"] * st["scale"]).abs()) + st["mean"].abs() * bscale
    return {"mean": bmean, "invstd": binv, "scale": bscale, "shift": bshift, "var": bvar}


def y_true_gate(c, relu, use_res):
    """(float64 batch norm (+ ReLU, + res), its bound, the centred bound no fp32 shift can meet) of a row's y"""
    st, b = c["st"], fwd_stat_bounds(c)
    x = c["x"].double()
    xs, xc = x * v5(st["scale"]), x - v5(st["mean"])
    pre = xs + v5(st["shift"])
    ref = F.relu(pre) if relu else pre
    bound = 4 * U * (xs.abs() + v5(st["shift"]).abs()) + xc.abs() * v5(b["scale"]) + v5(st["scale"].abs() * b["mean"])
    centred = 4 * U * (xc.abs() * v5(st["scale"]).abs() + v5(c["beta"].double()).abs())
    if use_res:
        r = c["res"].double()
        ref, bound, centred = ref + r, bound + 4 * U * r.abs(), centred + 4 * U * r.abs()
    return ref, bound, centred


def check_fwd_stats(tag, c, got, quiet=False):
    """got: [4, C] (mean, invstd, scale, shift).  The derived gates, then the flat 1e-5 on invstd and scale."""
    st, b = c["st"], fwd_stat_bounds(c)
    got = got.detach().cpu().double()
    w = 0.0
    for i, k in enumerate(("mean", "invstd", "scale", "shift")):
        w = max(w, check(f"{tag}.{k}", got[i], st[k], b[k], quiet))
    for i, k in ((1, "invstd"), (2, "scale")):
        rel = ((got[i] - st[k]).abs() / st[k].abs()).max()
        assert float(rel) <= 1e-5, (tag, k, float(rel))
    return w


def bwd_inputs(c):
    """the fp32 (scale, shift, mean, invstd) handed to the adjoint: float64 statistics rounded once"""
    st = c["st"]
    return tuple(st[k].float() for k in ("scale", "shift", "mean", "invstd"))


@functools.lru_cache(maxsize=None)
def bwd_ref(shape, kind, relu, training):
    c = bn_case(shape, kind, relu)
    B, C = shape[:2]
    sc, sh, mu, inv = (t.double() for t in bwd_inputs(c))
    x, dy = c["x"].double(), c["dy"].double()
    n = c["st"]["n"]
    g = torch.where(x * v5(sc) + v5(sh) > 0, dy, torch.zeros_like(dy)) if relu else dy
    xc = x - v5(mu)
    red = lambda t: t.transpose(0, 1).reshape(C, -1).sum(dim=1)      # noqa: E731
    sg, sgx = red(g), red(g * xc)
    L = bn_chain(B, C, n // B)
    bsg, bsgx = (L + 8) * U * red(g.abs()), (L + 8) * U * red(g.abs() * xc.abs())
    out = {"dgamma": inv * sgx, "dbeta": sg, "bdgamma": inv * bsgx, "bdbeta": bsg, "g": g}
    if training:
        c2 = -sc * inv * inv * sgx / n
        c3 = -sc * sg / n
        out["dx"] = g * v5(sc) + xc * v5(c2) + v5(c3)
        out["bdx"] = (4 * U * ((g * v5(sc)).abs() + xc.abs() * v5(c2).abs() + v5(c3).abs())
                      + xc.abs() * v5(sc.abs() * inv * inv * bsgx / n) + v5(sc.abs() * bsg / n))
    else:
        out["dx"] = g * v5(sc)
        out["bdx"] = 4 * U * out["dx"].abs()
    return out


# =========================================================================== weight-gradient rows
K3_CH_GEOMS = ((2, 3, 9, 20), (2, 3, 9, 33))
K3_CIN = (1, 3, 4, 5, 12, 24)
K3_COUT = (1, 3, 4, 5, 8, 12, 16, 20, 24)
K3_GEOMS = ((1, 1, 1), (1, 1, 4), (5, 3, 2), (2, 8, 32), (3, 9, 33), (2, 8, 36), (1, 17, 64), (4, 16, 64))
K3_GEOM_B3 = ((5, 3, 2), (3, 9, 33))
K3_PAIRS = ((4, 12), (5, 5))


def k3_rows():
    rows = [(B, Cin, Cout, D, H, W) for (B, D, H, W) in K3_CH_GEOMS for Cin in K3_CIN for Cout in K3_COUT]
    rows += [(B, Cin, Cout) + g for g in K3_GEOMS for (Cin, Cout) in K3_PAIRS for B in ((1, 3) if g in K3_GEOM_B3 else (2,))]
    return rows


def k3_plan(Cout):
    """(CG, gz) of wgrad_plan"""
    ng = ceil_div(Cout, 4)
    cg = next(c for c in (4, 3, 2, 1) if ng % c == 0)
    return cg, ng // cg


def k3_ntiles(B, D, H, W):
    return B * ceil_div(D, 2) * ceil_div(H, 8) * ceil_div(W, 32)


def k3_chain(ntiles, gx):
    return 32 * ceil_div(ntiles, gx) + 4 + ceil_div(gx, 64) + 6


def wgrad64(x64, g64, Cout, Cin, k, **kw):
    conv = F.conv3d if x64.dim() == 5 else F.conv2d
    w = torch.zeros((Cout, Cin) + (3,) * (x64.dim() - 2) if k == 3 else (Cout, Cin) + (1,) * (x64.dim() - 2), dtype=torch.float64,
                    requires_grad=True)
    (dw,) = torch.autograd.grad(conv(x64, w, **kw), w, g64)
    return dw


@functools.lru_cache(maxsize=None)
def k3_case(B, Cin, Cout, D, H, W):
    g = gen("k3", B, Cin, Cout, D, H, W)
    x, gy = torch.randn((B, Cin, D, H, W), generator=g) * 2 + 0.5, torch.randn((B, Cout, D, H, W), generator=g) * 0.01
    return {"x": x, "g": gy, "ref": wgrad64(x.double(), gy.double(), Cout, Cin, 3, padding=1),
            "Y": wgrad64(x.double().abs(), gy.double().abs(), Cout, Cin, 3, padding=1)}


K1_CIN, K1_COUT, K1_DHW, K1_B = (1, 11, 12, 13, 24, 48), (1, 3, 4, 5, 12, 24), (1, 255, 256, 257, 4099), (1, 3)


def k1_gx(B, Cin, Cout, dhw):
    return max(1, min(ceil_div(dhw, 256), ceil_div(512, ceil_div(Cin, 12) * ceil_div(Cout, 4) * B)))


def k1_chain(B, Cin, Cout, dhw):
    gx = k1_gx(B, Cin, Cout, dhw)
    return ceil_div(dhw, 256 * gx) + 6 + 2 + gx * B


@functools.lru_cache(maxsize=None)
def k1_case(B, dhw):
    """one (x, g) at the widest channel counts; the rows take leading channels"""
    g = gen("k1", B, dhw)
    return torch.randn((B, 48, 1, 1, dhw), generator=g) * 2 + 0.5, torch.randn((B, 24 + 2, 1, 1, dhw), generator=g) * 0.01


def k1_ref(x, gy):
    x64, g64 = x.double().flatten(2), gy.double().flatten(2)
    return torch.einsum("bov,biv->oi", g64, x64), torch.einsum("bov,biv->oi", g64.abs(), x64.abs())


S2_STRIDES, S2_HW, S2_CH, S2_B = (1, 2, 3, 4), ((1, 1), (2, 3), (9, 9), (17, 23), (36, 60)), ((3, 5), (6, 12)), (1, 2)


@functools.lru_cache(maxsize=None)
def s2_case(B, Cin, Cout, H, W, s):
    g = gen("s2", B, Cin, Cout, H, W, s)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x, gy = torch.randn((B, Cin, H, W), generator=g) * 2 + 0.5, torch.randn((B, Cout, Ho, Wo), generator=g) * 0.1
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * 0.2
    x64, g64, w64 = x.double(), gy.double(), w.double()

    def dgrad(g_, w_):
        xx = torch.zeros_like(x64, requires_grad=True)
        return torch.autograd.grad(F.conv2d(xx, w_, stride=s, padding=1), xx, g_)[0]
    gx = min(ceil_div(B * Ho * Wo, 1024), 64)
    return {"x": x, "g": gy, "w": w, "dx": dgrad(g64, w64), "Ydx": dgrad(g64.abs(), w64.abs()), "Ldx": 9 * Cout,
            "dw": wgrad64(x64, g64, Cout, Cin, 3, stride=s, padding=1), "Ydw": wgrad64(x64.abs(), g64.abs(), Cout, Cin, 3, stride=s, padding=1),
            "Ldw": ceil_div(B * Ho * Wo, 256 * gx) + 8 + gx}


# =========================================================================== adjoint rows
TRI_CASES = (                                        # (in size, out size): the per-axis pairs 1-1, 1-5, 5-1, 2-7, 7-2, 4-8, 8-4, 4-12, 12-4, 5-5
    ((1, 1, 5), (1, 5, 1)), ((2, 7, 4), (7, 2, 8)), ((8, 4, 12), (4, 12, 4)), ((5, 5, 5), (5, 5, 5)), ((4, 2, 1), (8, 7, 5)),
    ((12, 8, 7), (4, 4, 2)), ((5, 4, 4), (5, 8, 12)), ((1, 7, 8), (1, 2, 4)), ((4, 5, 2), (12, 1, 7)), ((2, 1, 4), (7, 1, 8)),
    ((3, 2, 4), (200, 7, 8)), ((4, 200, 2), (8, 3, 7)), ((2, 4, 3), (7, 12, 200)), ((200, 5, 4), (3, 5, 8)),      # generic loop
)
TRI_CPT = (1, 8, (32, 32, 64), (16, 16, 32))         # cpt = min(C, voxels * C / 256K) = 2


def tri_matrices(i, o, align):
    """float64 [out, in] matrix of one axis and its tap support (1 at i0 and i1 = min(i0 + 1, in - 1))"""
    M = F.interpolate(torch.eye(i, dtype=torch.float64)[None], size=o, mode="linear", align_corners=align)[0].t().contiguous()
    i0 = (M > 0).double().argmax(dim=1)
    S = torch.zeros_like(M)
    S[torch.arange(o), i0] = 1.0
    S[torch.arange(o), (i0 + 1).clamp_max(i - 1)] = 1.0
    return M, S


@functools.lru_cache(maxsize=None)
def tri_case(B, C, isz, osz, align):
    """bound = (L + 8) U Y + per axis 2^-23 (in - 1) * (the adjoint of |dy| with that axis' two tap weights set to 1): the source
    index scale * (o + 0.5) - 0.5 is formed in fp32, so lambda carries an ABSOLUTE error of two roundings of the index, and a tap
    weight much smaller than 1 takes it whole (ATen's own fp32 result missed a bound relative to Y by 2x at 200 -> 3)."""
    dy = torch.randn((B, C) + osz, generator=gen("tri", B, C, isz, osz, align))
    xx = torch.zeros((B, C) + isz, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(F.interpolate(xx, size=osz, mode="trilinear", align_corners=align), xx, dy.double())
    MS = [tri_matrices(i, o, align) for i, o in zip(isz, osz)]
    adj = lambda d, mz, my, mx: torch.einsum("bcdhw,dz,hy,wx->bczyx", d, mz, my, mx)      # noqa: E731
    assert float((adj(dy.double(), MS[0][0], MS[1][0], MS[2][0]) - ref).abs().max()) <= 1e-12
    a = dy.double().abs()
    L = math.prod(2 * ceil_div(o, i) + 2 for i, o in zip(isz, osz))
    bound = (L + 8) * U * adj(a, MS[0][0], MS[1][0], MS[2][0])
    for ax in range(3):
        if isz[ax] != osz[ax]:
            ms = [MS[k][1 if k == ax else 0] for k in range(3)]
            bound = bound + 2.0 ** -23 * (isz[ax] - 1) * adj(a, *ms)
    return {"dy": dy, "ref": ref, "bound": bound}


CV_ROWS = tuple((B, C, d, h, w) for (d, h, w) in ((5, 85, 3), (5, 51, 5), (16, 16, 16), (4, 255, 1), (4, 257, 1), (3, 15, 17), (20, 1, 257))
                for C in (1, 3, 12) for B in (1, 2))


@functools.lru_cache(maxsize=None)
def cv_case(B, C, d, h, w):
    dc = torch.randn((B, 2 * C, d, h, w), generator=gen("cv", B, C, d, h, w))

    def adj(t):
        Lf = torch.zeros((B, C, h, w), dtype=torch.float64, requires_grad=True)
        Rf = torch.zeros((B, C, h, w), dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(O.cost_volume(Lf, Rf, 3 * d), (Lf, Rf), t, allow_unused=True)
    ref, Y = adj(dc.double()), adj(dc.double().abs())
    z = torch.zeros((B, C, h, w), dtype=torch.float64)
    return {"dc": dc, "ref": [z if t is None else t for t in ref], "bound": [(d + 8) * U * (z if t is None else t) for t in Y]}


# =========================================================================== CPU: the gates and the rows themselves
def test_row_tables_cover_what_they_claim():
    assert {bn_gx(*s[:2], math.prod(s[2:])) for s in BN_SHAPES} >= {1, 3, 4, 6}
    assert {bn_chain(*s[:2], math.prod(s[2:])) for s in BN_SHAPES} == {12, 16, 24}             # one, two and four quads per thread
    B, C = 300, 2
    assert bn_gx(B, C, 4) == 1 and B > 256                                         # more than 256 partials per channel
    assert [math.prod(s[2:]) % 4 == 0 for s in VIEW_SHAPES] == [True, False]
    assert 2304 == 2 * 1024 + 256 == math.prod((4, 16, 36))
    mix = lambda kind, C: {channel_spec(kind, C, c) for c in range(C)}             # noqa: E731
    assert mix("cond", 5) == set(COND_SPECS[:5]) and mix("cond", 12) == set(COND_SPECS)
    assert mix("condk", 5) >= {COND_SPECS[5], COND_SPECS[3], COND_SPECS[4]}        # constant, 1000 / 1, -100 / 0.1 in one launch
    plans = {k3_plan(co) for co in K3_COUT}
    assert {p[0] for p in plans} == {1, 2, 3, 4} and any(p[1] > 1 for p in plans)
    assert k3_ntiles(1, 2, 8, 32) == 1 and k3_ntiles(1, 3, 9, 33) == 8
    assert {W % 4 == 0 for (_b, _d, _h, W) in K3_CH_GEOMS} == {True, False}
    assert {h * w for (_b, _c, _d, h, w) in CV_ROWS} >= {255, 256, 257} and {w for r in CV_ROWS for w in r[4:]} >= {1}
    assert any(w < d for (_b, _c, d, _h, w) in CV_ROWS) and any(w == d for (_b, _c, d, _h, w) in CV_ROWS)
    pairs = {(i, o) for isz, osz in TRI_CASES for i, o in zip(isz, osz)}
    assert pairs >= {(1, 1), (1, 5), (5, 1), (2, 7), (7, 2), (4, 8), (8, 4), (4, 12), (12, 4), (5, 5), (3, 200), (200, 3)}
    Bc, Cc, isz, _osz = TRI_CPT
    assert min(Cc, math.prod(isz) * Bc * Cc // (256 * 1024)) > 1


@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("shape,kind", BN_ROWS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_bn_gates_hold_for_aten_fp32(shape, kind, relu):
    """ATen's fp32 CPU batch norm through the same gates: statistics (momentum 1 exposes them as running statistics) and the
    adjoint from the same fp32 (mean, invstd).  The yardsticks are nonzero wherever the reference is."""
    c = bn_case(shape, kind, relu)
    st, b = c["st"], fwd_stat_bounds(c)
    C = shape[1]
    rm, rv = torch.zeros(C), torch.zeros(C)
    F.batch_norm(c["x"], rm, rv, c["gamma"], c["beta"], True, 1.0, EPS)
    check("aten.mean", rm, st["mean"], b["mean"], True)
    check("aten.var", rv, st["varu"], b["var"] * (st["n"] / max(st["n"] - 1, 1)) + 4 * U * st["varu"], True)
    assert float(((rv.double() - st["varu"]).abs() / (st["varu"] + EPS)).max()) <= 1e-5
    y32 = F.batch_norm(c["x"], None, None, c["gamma"], c["beta"], True, 0.0, EPS)
    yref, ybound, ycentred = y_true_gate(c, relu, False)
    check("aten.y", F.relu(y32) if relu else y32, yref, ybound, True)
    if kind != "plain":             # the yardstick's |shift| term is needed: ATen's x alpha + beta misses the centred bound
        assert float((((F.relu(y32) if relu else y32).double() - yref).abs() / ycentred.clamp_min(1e-300)).max()) > 1.0
    r = bwd_ref(shape, kind, relu, True)
    sc, sh, mu, inv = bwd_inputs(c)
    dx, dg, db = torch.ops.aten.native_batch_norm_backward(r["g"].float(), c["x"], c["gamma"], None, None, mu, inv, True, EPS, [True, True, True])
    # ATen's scale is gamma * invstd in fp32, ours the rounded float64 scale: carry the reference over to its scale
    k = (c["gamma"].double() * inv.double()) / sc.double()
    check("aten.dgamma", dg, r["dgamma"], r["bdgamma"] + 4 * U * r["dgamma"].abs(), True)
    check("aten.dbeta", db, r["dbeta"], r["bdbeta"] + 4 * U * r["dbeta"].abs(), True)
    check("aten.dx", dx, r["dx"] * v5(k), r["bdx"] * v5(k), True)
    for ref, bound in ((r["dx"], r["bdx"]), (r["dgamma"], r["bdgamma"]), (r["dbeta"], r["bdbeta"]), (st["mean"], b["mean"])):
        assert bool((bound.expand_as(ref)[ref != 0] > 0).all())
    live = st["var"] > 0
    assert bool((b["var"][live] > 0).all())


@pytest.mark.parametrize("shape,kind", BN_ROWS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_no_relu_knife_edge(shape, kind):
    c = bn_case(shape, kind, True)
    assert not knife_edge(c["x"], c["st"]).any()
    n_ch = math.prod(shape) // shape[1]
    assert c["redrawn"] <= max(4, n_ch * shape[1] // 200), c["redrawn"]         # a handful of redraws, not a reshaped distribution
    if kind == "plain":
        assert c["redrawn"] == 0


@pytest.mark.parametrize("row", k3_rows(), ids=lambda r: "B{}i{}o{}_{}x{}x{}".format(*r))
def test_k3_gate_holds_for_aten_fp32(row):
    B, Cin, Cout, D, H, W = row
    c = k3_case(*row)
    w = torch.zeros((Cout, Cin, 3, 3, 3), requires_grad=True)
    (dw,) = torch.autograd.grad(F.conv3d(c["x"], w, padding=1), w, c["g"])
    nt = k3_ntiles(B, D, H, W)
    check("aten.k3", dw, c["ref"], (k3_chain(nt, nt) + 8) * U * c["Y"], True)
    assert bool((c["Y"][c["ref"] != 0] > 0).all())


@pytest.mark.parametrize("B", K1_B)
@pytest.mark.parametrize("dhw", K1_DHW)
def test_k1_gate_holds_for_aten_fp32(dhw, B):
    x, gy = k1_case(B, dhw)
    for Cin in K1_CIN:
        for Cout in K1_COUT:
            xs, gs = x[:, :Cin], gy[:, :Cout]
            ref, Y = k1_ref(xs, gs)
            w = torch.zeros((Cout, Cin, 1, 1, 1), requires_grad=True)
            (dw,) = torch.autograd.grad(F.conv3d(xs, w), w, gs)
            check("aten.k1", dw, ref, (k1_chain(B, Cin, Cout, dhw) + 8) * U * Y, True)
            assert bool((Y[ref != 0] > 0).all())


@pytest.mark.parametrize("s", S2_STRIDES)
def test_strided_gates_hold_for_aten_fp32(s):
    for (H, W) in S2_HW:
        for (Cin, Cout) in S2_CH:
            for B in S2_B:
                c = s2_case(B, Cin, Cout, H, W, s)
                xx = c["x"].clone().requires_grad_(True)
                w = c["w"].clone().requires_grad_(True)
                dx, dw = torch.autograd.grad(F.conv2d(xx, w, stride=s, padding=1), (xx, w), c["g"])
                check("aten.s2.dx", dx, c["dx"], (c["Ldx"] + 8) * U * c["Ydx"], True)
                check("aten.s2.dw", dw, c["dw"], (c["Ldw"] + 8) * U * c["Ydw"], True)
                assert bool((c["Ydx"][c["dx"] != 0] > 0).all()) and bool((c["Ydw"][c["dw"] != 0] > 0).all())


def tri_rows():
    rows = [(1 + (k % 2), C, isz, osz, align) for k, (isz, osz) in enumerate(TRI_CASES) for align in (False, True) for C in (1, 3)]
    return rows + [TRI_CPT + (False,)]


@pytest.mark.parametrize("row", tri_rows(), ids=lambda r: "B{}C{}_{}_{}_{}".format(r[0], r[1], "x".join(map(str, r[2])), "x".join(map(str, r[3])), int(r[4])))
def test_trilinear_gate_holds_for_aten_fp32(row):
    B, C, isz, osz, align = row
    c = tri_case(*row)
    xx = torch.zeros((B, C) + isz, requires_grad=True)
    (dx,) = torch.autograd.grad(F.interpolate(xx, size=osz, mode="trilinear", align_corners=align), xx, c["dy"])
    check("aten.tri", dx, c["ref"], c["bound"], True)
    assert bool((c["bound"][c["ref"] != 0] > 0).all())


@pytest.mark.parametrize("row", CV_ROWS, ids=lambda r: "B{}C{}_{}x{}x{}".format(*r))
def test_costvol_gate_holds_for_the_oracle_fp32(row):
    B, C, d, h, w = row
    c = cv_case(*row)
    Lf, Rf = torch.zeros((B, C, h, w), requires_grad=True), torch.zeros((B, C, h, w), requires_grad=True)
    got = torch.autograd.grad(O.cost_volume(Lf, Rf, 3 * d), (Lf, Rf), c["dc"])
    for t, ref, bound in zip(got, c["ref"], c["bound"]):
        check("oracle.cv", t, ref, bound, True)
        assert bool((bound[ref != 0] > 0).all())


# =========================================================================== GPU
@pytest.fixture(scope="module")
def ra():
    import rag_amd
    rag_amd.load_library()
    return rag_amd


def gpu(x):
    return torch.as_tensor(x).to(DEV)


def run_bn_row(ra, tag, c, relu, x=None, with_res=False, y_into=None, res_in=None, dy_in=None, dx_into=None):
    """forward (stats, fused with and without res) and adjoint (fused and split, train and eval) of one row against its gates;
    x / y_into / res_in / dy_in / dx_into = (tensor or buffer, ch0) views to run through instead of fresh contiguous tensors"""
    ops = ra.ops
    shape, st = c["shape"], c["st"]
    B, C = shape[:2]
    xg = x if x is not None else gpu(c["x"])
    gm, bt = gpu(c["gamma"]), gpu(c["beta"])
    worst = check_fwd_stats(f"{tag}.stats", c, ops.bn_train_stats(xg, gm, bt, None, None, None, 0.1, EPS))
    for use_res in ((False, True) if with_res or res_in is not None else (False,)):
        rbuf, rch0 = (res_in if res_in is not None else (gpu(c["res"]), 0)) if use_res else (None, 0)
        ybuf, ych0 = y_into if y_into is not None else (None, 0)
        y, s4 = ops.bn_train_act(xg, gm, bt, None, None, None, 0.1, EPS, relu, res=rbuf, res_ch0=rch0, out=ybuf, out_ch0=ych0)
        worst = max(worst, check_fwd_stats(f"{tag}.act.stats", c, s4, quiet=True))
        s64 = s4.cpu().double()
        xs = c["x"].double() * v5(s64[2])
        pre = xs + v5(s64[3])
        ref = F.relu(pre) if relu else pre
        bound = 4 * U * (xs.abs() + v5(s64[3]).abs())
        if use_res:
            ref, bound = ref + c["res"].double(), bound + 4 * U * c["res"].double().abs()
        worst = max(worst, check(f"{tag}.y{'+res' if use_res else ''}", y[:, ych0:ych0 + C], ref, bound))
        tref, tbound, _centred = y_true_gate(c, relu, use_res)
        worst = max(worst, check(f"{tag}.y{'+res' if use_res else ''}.vs64", y[:, ych0:ych0 + C], tref, tbound, quiet=True))
        yb2 = torch.full_like(ybuf, SENT) if ybuf is not None else None
        y2 = ops.bn_act(xg, s4[2], s4[3], relu, out=yb2, out_ch0=ych0, res=rbuf, res_ch0=rch0)
        worst = max(worst, check(f"{tag}.bn_act{'+res' if use_res else ''}", y2[:, ych0:ych0 + C], ref, bound))
        assert torch.equal(bits(y2[:, ych0:ych0 + C]), bits(y[:, ych0:ych0 + C])), "bn_act and the fused launch differ"
        if yb2 is not None:
            other = [ch for ch in range(yb2.shape[1]) if not ych0 <= ch < ych0 + C]
            assert bool((yb2[:, other] == SENT).all()), "bn_act wrote outside its channel slice"
        for ch, (m, s) in enumerate(c["specs"]):
            if s == 0.0:                                  # constant channel: act(beta) (+ res)
                yb = F.relu(c["beta"][ch].double()) if relu else c["beta"][ch].double()
                want = yb + (c["res"][:, ch].double() if use_res else 0.0)
                check(f"{tag}.y.const", y[:, ych0 + ch], want + torch.zeros(c["x"][:, ch].shape, dtype=torch.float64), bound[:, ch], quiet=True)
                assert abs(float(s4[1, ch]) * math.sqrt(EPS) - 1.0) <= 1e-5
    sc, sh, mu, inv = (gpu(t) for t in bwd_inputs(c))
    dyb, dch0 = dy_in if dy_in is not None else (gpu(c["dy"]), 0)
    for training in (True, False):
        r = bwd_ref(shape, c["kind"], relu, training)
        dx, dg, db = ops.bn_act_bwd(dyb, xg, sc, sh, relu, mu, inv, training, out=dx_into, dy_ch0=dch0)
        t = f"{tag}.bwd{'T' if training else 'E'}"
        worst = max(worst, check(f"{t}.dx", dx, r["dx"], r["bdx"]), check(f"{t}.dgamma", dg, r["dgamma"], r["bdgamma"] + 4 * U * r["dgamma"].abs()),
                    check(f"{t}.dbeta", db, r["dbeta"], r["bdbeta"] + 4 * U * r["dbeta"].abs()))
        co = ops.bn_act_bwd_coeffs(dyb, dch0, xg, sc, sh, relu, mu, inv, training)
        dx2 = ops.bn_act_bwd_apply(dyb, dch0, xg, sc, sh, relu, co[0], co[1], co[2], co[3], out=dx_into)
        check(f"{t}.split.dx", dx2, r["dx"], r["bdx"], quiet=True)
        assert torch.equal(bits(co[4]), bits(dg)) and torch.equal(bits(co[5]), bits(db))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("shape,kind", BN_ROWS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_bn_rows(ra, shape, kind, relu):
    """every shape row and the conditioning matrix: statistics, fused forward with and without res, fused and split adjoint"""
    c = bn_case(shape, kind, relu)
    run_bn_row(ra, f"bn_{'x'.join(map(str, shape))}_{kind}_{'relu' if relu else 'lin'}", c, relu, with_res=True)


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("shape", VIEW_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_bn_views(ra, shape, relu):
    """x a channel slice (batch stride > C * DHW), y into y_ch0 > 0, res from res_ch0 > 0, dy from dy_ch0 > 0, dx into out=; the
    channels outside the slices keep their bits.  Then x and dy from a base pointer one float off (scalar path when DHW % 4 == 0)."""
    c = bn_case(shape, "plain", relu)
    B, C = shape[:2]
    vol = shape[2:]

    def wide(src, extra, ch0):
        buf = torch.full((B, C + extra) + vol, SENT, device=DEV)
        if src is not None:
            buf[:, ch0:ch0 + C] = gpu(src)
        return buf
    xw, yw, rw, dyw, dxw = wide(c["x"], 3, 1), wide(None, 4, 2), wide(c["res"], 2, 1), wide(c["dy"], 3, 3), wide(None, 2, 1)
    keep = [bits(t) for t in (xw, rw, dyw)]
    tag = f"bnview_{'x'.join(map(str, shape))}_{'relu' if relu else 'lin'}"
    run_bn_row(ra, tag, c, relu, x=xw[:, 1:1 + C], y_into=(yw, 2), res_in=(rw, 1), dy_in=(dyw, 3), dx_into=dxw[:, 1:1 + C])
    for t, k in zip((xw, rw, dyw), keep):
        assert torch.equal(bits(t), k)
    for buf, ch0 in ((yw, 2), (dxw, 1)):
        other = [ch for ch in range(buf.shape[1]) if not ch0 <= ch < ch0 + C]
        assert bool((buf[:, other] == SENT).all()), "wrote outside the channel slice"
    n = math.prod(shape)
    off = [torch.full((n + 1,), SENT, device=DEV) for _ in range(2)]
    off[0][1:] = gpu(c["x"]).reshape(-1)
    off[1][1:] = gpu(c["dy"]).reshape(-1)
    assert off[0][1:].data_ptr() % 16 == 4
    run_bn_row(ra, tag + "_off1", c, relu, x=off[0][1:].view(shape), dy_in=(off[1][1:].view(shape), 0))


@pytest.mark.gpu
def test_bn_train_act_rejects_y_over_x(ra):
    """the second launch re-reads the pivots x[0, c, 0] while other workgroups store y: ops refuses an `out` that overlaps x, and
    takes the neighbouring channels of the same buffer"""
    shape = (2, 4, 4, 16, 36)
    c = bn_case(shape, "plain", True)
    buf = torch.full((2, 9, 4, 16, 36), SENT, device=DEV)
    buf[:, 1:5] = gpu(c["x"])
    args = (gpu(c["gamma"]), gpu(c["beta"]), None, None, None, 0.1, EPS, True)
    for ch0 in (0, 1, 4):
        with pytest.raises(ValueError):
            ra.ops.bn_train_act(buf[:, 1:5], *args, out=buf, out_ch0=ch0)
    with pytest.raises(ValueError):
        ra.ops.bn_train_act(buf[:, 1:5], *args, out=buf[:, 1:5])
    y, s4 = ra.ops.bn_train_act(buf[:, 1:5], *args, out=buf, out_ch0=5)
    check_fwd_stats("bn_inplace_neighbour.stats", c, s4)
    tref, tbound, _centred = y_true_gate(c, True, False)
    check("bn_inplace_neighbour.y.vs64", y[:, 5:9], tref, tbound)
    assert bool((buf[:, 0] == SENT).all()) and torch.equal(bits(buf[:, 1:5]), bits(c["x"]))


@pytest.mark.gpu
@pytest.mark.parametrize("momentum", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("shape,kind", [((2, 5, 3, 7, 9), "cond"), ((2, 5, 3, 7, 9), "condk"), ((1, 12, 8, 16, 32), "cond"), ((2, 4, 4, 16, 36), "plain")],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_bn_running_statistics(ra, shape, kind, momentum):
    """momentum update of running_mean / running_var (unbiased) against float64, num_batches_tracked + 1 exactly once, from both
    entry points; running_var within 1e-5 of float64 relative to its own terms (+ eps)."""
    c = bn_case(shape, kind, False)
    st, b = c["st"], fwd_stat_bounds(c)
    C = shape[1]
    g = gen("run", shape, kind)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    m = float(torch.tensor(momentum, dtype=torch.float32))
    want_m = (1 - m) * rm0.double() + m * st["mean"]
    want_v = (1 - m) * rv0.double() + m * st["varu"]
    bm = m * b["mean"] + 4 * U * ((1 - m) * rm0.double().abs() + m * st["mean"].abs())
    bv = m * b["var"] * (st["n"] / max(st["n"] - 1, 1)) + 4 * U * ((1 - m) * rv0.double() + m * st["varu"])
    for fused in (False, True):
        rm, rv, nbt = gpu(rm0.clone()), gpu(rv0.clone()), torch.tensor(7, device=DEV, dtype=torch.int64)
        if fused:
            ra.ops.bn_train_act(gpu(c["x"]), gpu(c["gamma"]), gpu(c["beta"]), rm, rv, nbt, momentum, EPS, True)
        else:
            ra.ops.bn_train_stats(gpu(c["x"]), gpu(c["gamma"]), gpu(c["beta"]), rm, rv, nbt, momentum, EPS)
        tag = f"bnrun_{'x'.join(map(str, shape))}_m{momentum}_{'act' if fused else 'stats'}"
        check(f"{tag}.mean", rm, want_m, bm)
        check(f"{tag}.var", rv, want_v, bv)
        assert float(((rv.cpu().double() - want_v).abs() / ((1 - m) * rv0.double() + m * (st["varu"] + EPS))).max()) <= 1e-5
        assert int(nbt) == 8
        if momentum == 0.0:
            assert torch.equal(bits(rm), bits(rm0)) and torch.equal(bits(rv), bits(rv0))


@pytest.mark.gpu
def test_bn_accumulate_into(ra):
    """dgamma_into / dbeta_into add onto non-zero contents (fused and split entry points)"""
    shape, relu = (2, 5, 3, 7, 9), True
    c = bn_case(shape, "cond", relu)
    r = bwd_ref(shape, "cond", relu, True)
    sc, sh, mu, inv = (gpu(t) for t in bwd_inputs(c))
    g = gen("acc")
    g0, b0 = torch.randn(5, generator=g) * 3, torch.randn(5, generator=g) * 3
    for split in (False, True):
        dg, db = gpu(g0.clone()), gpu(b0.clone())
        if split:
            ra.ops.bn_act_bwd_coeffs(gpu(c["dy"]), 0, gpu(c["x"]), sc, sh, relu, mu, inv, True, dgamma_into=dg, dbeta_into=db)
        else:
            _dx, a_, b_ = ra.ops.bn_act_bwd(gpu(c["dy"]), gpu(c["x"]), sc, sh, relu, mu, inv, True, dgamma_into=dg, dbeta_into=db)
            assert a_ is None and b_ is None
        check(f"bnacc_{'split' if split else 'fused'}.dgamma", dg, g0.double() + r["dgamma"], r["bdgamma"] + 4 * U * (g0.double().abs() + r["dgamma"].abs()))
        check(f"bnacc_{'split' if split else 'fused'}.dbeta", db, b0.double() + r["dbeta"], r["bdbeta"] + 4 * U * (b0.double().abs() + r["dbeta"].abs()))


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
def test_bn_eval_exact_zero(ra, relu):
    """eval path, x small integers, scale 1, shift -2: the x == 2 elements are exact zeros -> y == 0 and zero gradient (torch.relu)"""
    shape = (2, 3, 2, 5, 8)
    g = gen("exact")
    x = torch.randint(-3, 7, shape, generator=g).float()
    dy = torch.randint(-4, 5, shape, generator=g).float()
    one, sh, zero = torch.ones(3, device=DEV), torch.full((3,), -2.0, device=DEV), torch.zeros(3, device=DEV)
    assert int((x == 2).sum()) > 10
    y = ra.ops.bn_act(gpu(x), one, sh, relu)
    pre = x - 2
    assert torch.equal(y.cpu(), F.relu(pre) if relu else pre)
    want = torch.where(pre > 0, dy, torch.zeros_like(dy)) if relu else dy
    co = ra.ops.bn_act_bwd_coeffs(gpu(dy), 0, gpu(x), one, sh, relu, zero, one, False)
    dx = ra.ops.bn_act_bwd_apply(gpu(dy), 0, gpu(x), one, sh, relu, co[0], co[1], co[2], co[3])
    assert torch.equal(dx.cpu(), want)
    assert torch.equal(co[5].cpu(), want.transpose(0, 1).reshape(3, -1).sum(dim=1))          # integers: exact in any order
    assert torch.equal(co[4].cpu(), (want * x).transpose(0, 1).reshape(3, -1).sum(dim=1))
    print(f"TRAIN case=bn_eval_exact_{'relu' if relu else 'lin'} worst=0/0 (bit-exact)")


def k3_gx(ra, B, Cin, Cout, D, H, W):
    cg, gz = k3_plan(Cout)
    n = ra.load_library().ragmi_conv3d_k3_wgrad_workspace_elems(B, Cin, Cout, D, H, W)
    per = (gz * cg * 4) * (ceil_div(Cin, 4) * 4) * 27
    assert n > 0 and n % per == 0
    return n // per


def k3_bound(ra, row, c):
    B, Cin, Cout, D, H, W = row
    gx = k3_gx(ra, *row)
    return (k3_chain(k3_ntiles(B, D, H, W), gx) + 8) * U * c["Y"]


@pytest.mark.gpu
@pytest.mark.parametrize("Cin", K3_CIN)
@pytest.mark.parametrize("geom", K3_CH_GEOMS, ids=lambda g: "B{}_{}x{}x{}".format(*g))
def test_k3_wgrad_channel_matrix(ra, geom, Cin):
    B, D, H, W = geom
    for Cout in K3_COUT:
        row = (B, Cin, Cout, D, H, W)
        c = k3_case(*row)
        dw = ra.ops.conv3d_k3_wgrad(gpu(c["x"]), gpu(c["g"]), Cout)
        check(f"k3ch_i{Cin}o{Cout}_{D}x{H}x{W}", dw, c["ref"], k3_bound(ra, row, c))


@pytest.mark.gpu
@pytest.mark.parametrize("geom", K3_GEOMS, ids=lambda g: "{}x{}x{}".format(*g))
def test_k3_wgrad_geometry_matrix(ra, geom):
    for row in [r for r in k3_rows() if r[3:] == geom and (r[1], r[2]) in K3_PAIRS and (r[0],) + geom not in K3_CH_GEOMS]:
        c = k3_case(*row)
        dw = ra.ops.conv3d_k3_wgrad(gpu(c["x"]), gpu(c["g"]), row[2])
        check("k3geo_B{}i{}o{}_{}x{}x{}".format(*row), dw, c["ref"], k3_bound(ra, row, c))


@pytest.mark.gpu
def test_k3_wgrad_persistent_trips(ra):
    """Cin = Cout = 48: 36 channel workgroups per tile slot, so gx is small; the smallest (2, 8, H, 64) with ntiles >= 3 gx and a
    ragged last trip runs the grid-stride loop, the pipelined prefetch and its clamped last prefetch."""
    Cin = Cout = 48
    for H in range(16, 257, 8):
        row = (2, Cin, Cout, 8, H, 64)
        gx, nt = k3_gx(ra, *row), k3_ntiles(2, 8, H, 64)
        if nt >= 3 * gx and nt % gx != 0:
            break
    assert nt >= 3 * gx and nt % gx != 0, (nt, gx)
    c = k3_case(*row)
    dw = ra.ops.conv3d_k3_wgrad(gpu(c["x"]), gpu(c["g"]), Cout)
    check(f"k3trips_H{H}_gx{gx}_nt{nt}", dw, c["ref"], k3_bound(ra, row, c))
    dw2 = ra.ops.conv3d_k3_wgrad(gpu(c["x"]), gpu(c["g"]), Cout)
    assert torch.equal(bits(dw), bits(dw2))


@pytest.mark.gpu
@pytest.mark.parametrize("W", [20, 33])
def test_k3_wgrad_destinations_and_views(ra, W):
    """`into` over n = 1, 2, 3, 8 destinations on non-zero contents, g at g_ch0 > 0 of a wider buffer, x a channel slice, the
    destinations carved from one guarded buffer; planar2d (D = 1) fresh and accumulated."""
    B, Cin, Cout, D, H = 2, 5, 24, 3, 9
    row = (B, Cin, Cout, D, H, W)
    c = k3_case(*row)
    bound = k3_bound(ra, row, c)
    xw = torch.full((B, Cin + 2, D, H, W), SENT, device=DEV)
    xw[:, 1:1 + Cin] = gpu(c["x"])
    gw = torch.full((B, Cout + 5, D, H, W), SENT, device=DEV)
    gw[:, 3:3 + Cout] = gpu(c["g"])
    g0 = torch.randn((Cout, Cin, 3, 3, 3), generator=gen("k3into", W))
    for n in (1, 2, 3, 8):
        per = Cout // n * Cin * 27
        buf = torch.full((n * (per + 16) + 16,), SENT, device=DEV)
        dsts = [buf[16 + k * (per + 16):16 + k * (per + 16) + per].view(Cout // n, Cin, 3, 3, 3) for k in range(n)]
        for k, d in enumerate(dsts):
            d.copy_(gpu(g0[k * (Cout // n):(k + 1) * (Cout // n)]))
        assert ra.ops.conv3d_k3_wgrad(xw[:, 1:1 + Cin], gw, Cout, g_ch0=3, into=dsts) is None
        check(f"k3into_n{n}_W{W}", torch.cat(dsts), g0.double() + c["ref"], bound + 4 * U * (g0.double().abs() + c["ref"].abs()))
        mask = torch.ones_like(buf, dtype=torch.bool)
        for k in range(n):
            mask[16 + k * (per + 16):16 + k * (per + 16) + per] = False
        assert bool((buf[mask] == SENT).all()), "wrote outside a destination"
    assert bool((xw[:, [0, Cin + 1]] == SENT).all()) and bool((gw[:, [0, 1, 2, Cout + 3, Cout + 4]] == SENT).all())
    rowp = (B, Cin, Cout, 1, H, W)
    cp = k3_case(*rowp)
    bp = k3_bound(ra, rowp, cp)[:, :, 1]
    dw = ra.ops.conv3d_k3_wgrad(gpu(cp["x"]), gpu(cp["g"]), Cout, planar2d=True)
    check(f"k3planar_W{W}", dw, cp["ref"][:, :, 1], bp)
    d0 = gpu(g0[:, :, 1].contiguous())
    ra.ops.conv3d_k3_wgrad(gpu(cp["x"]), gpu(cp["g"]), Cout, into=[d0], planar2d=True)
    check(f"k3planar_into_W{W}", d0, g0[:, :, 1].double() + cp["ref"][:, :, 1], bp + 4 * U * (g0[:, :, 1].double().abs() + cp["ref"][:, :, 1].abs()))


@pytest.mark.gpu
@pytest.mark.parametrize("B", K1_B)
@pytest.mark.parametrize("dhw", K1_DHW)
def test_k1_wgrad_matrix(ra, dhw, B):
    """every Cin x Cout, twice (the atomics change the order, not the bound), g at g_ch0 = 2 of the 26-channel buffer, and `into`
    on non-zero contents"""
    x, gy = k1_case(B, dhw)
    xg, gg = gpu(x), gpu(gy)
    worst = (0.0, "")
    for Cin in K1_CIN:
        for Cout in K1_COUT:
            for ch0 in ((0, 2) if (Cin, Cout) in ((13, 5), (48, 24), (1, 1), (12, 4)) else (0,)):
                ref, Y = k1_ref(x[:, :Cin], gy[:, ch0:ch0 + Cout])
                bound = (k1_chain(B, Cin, Cout, dhw) + 8) * U * Y
                for rep in range(2):
                    dw = ra.ops.conv3d_k1_wgrad(xg[:, :Cin], gg, Cout, g_ch0=ch0)
                    worst = max(worst, (check(f"k1_i{Cin}o{Cout}_v{dhw}B{B}_ch{ch0}_{rep}", dw, ref, bound, quiet=True), f"i{Cin}o{Cout}ch{ch0}"))
                if ch0:
                    d0 = torch.randn((Cout, Cin), generator=gen("k1into", Cin, Cout))
                    dst = gpu(d0.clone())
                    ra.ops.conv3d_k1_wgrad(xg[:, :Cin], gg, Cout, g_ch0=ch0, into=dst)
                    check(f"k1into_i{Cin}o{Cout}_v{dhw}B{B}", dst, d0.double() + ref, bound + (k1_gx(B, Cin, Cout, dhw) * B + 4) * U * (d0.double().abs() + Y), quiet=True)
    print(f"TRAIN case=k1_v{dhw}B{B} worst={worst[0]:.3f} ({worst[1]})")


@pytest.mark.gpu
@pytest.mark.parametrize("s", S2_STRIDES)
def test_strided_stem_grads(ra, s):
    worst = {"dx": (0.0, ""), "dw": (0.0, "")}
    for (H, W) in S2_HW:
        for (Cin, Cout) in S2_CH:
            for B in S2_B:
                c = s2_case(B, Cin, Cout, H, W, s)
                tag = f"s{s}_B{B}i{Cin}o{Cout}_{H}x{W}"
                dx = ra.ops.conv2d_k3_strided_dgrad(gpu(c["g"]), gpu(c["w"]), (H, W), s)
                worst["dx"] = max(worst["dx"], (check(f"s2dx_{tag}", dx, c["dx"], (c["Ldx"] + 8) * U * c["Ydx"], quiet=True), tag))
                dw = ra.ops.conv2d_k3_strided_wgrad(gpu(c["x"]), gpu(c["g"]), s)
                bound = (c["Ldw"] + 8) * U * c["Ydw"]
                worst["dw"] = max(worst["dw"], (check(f"s2dw_{tag}", dw, c["dw"], bound, quiet=True), tag))
                d0 = torch.randn((Cout, Cin, 3, 3), generator=gen("s2into", tag))
                dst = gpu(d0.clone())
                ra.ops.conv2d_k3_strided_wgrad(gpu(c["x"]), gpu(c["g"]), s, into=dst)
                check(f"s2into_{tag}", dst, d0.double() + c["dw"], bound + (c["Ldw"] + 8) * U * d0.double().abs(), quiet=True)
    for k, (wv, tag) in worst.items():
        print(f"TRAIN case=s2{k}_s{s} worst={wv:.3f} ({tag})")


@pytest.mark.gpu
@pytest.mark.parametrize("row", tri_rows(), ids=lambda r: "B{}C{}_{}_{}_{}".format(r[0], r[1], "x".join(map(str, r[2])), "x".join(map(str, r[3])), int(r[4])))
def test_trilinear_adjoint(ra, row):
    B, C, isz, osz, align = row
    c = tri_case(*row)
    dx = ra.ops.trilinear3d_bwd(gpu(c["dy"]), isz, align)
    check("tri_B{}C{}_{}_{}_a{}".format(B, C, "x".join(map(str, isz)), "x".join(map(str, osz)), int(align)), dx, c["ref"], c["bound"])


@pytest.mark.gpu
@pytest.mark.parametrize("row", CV_ROWS, ids=lambda r: "B{}C{}_{}x{}x{}".format(*r))
def test_costvol_adjoint(ra, row):
    c = cv_case(*row)
    dl, dr = ra.ops.costvol_bwd(gpu(c["dc"]))
    check("cvL_B{}C{}_{}x{}x{}".format(*row), dl, c["ref"][0], c["bound"][0])
    check("cvR_B{}C{}_{}x{}x{}".format(*row), dr, c["ref"][1], c["bound"][1])
