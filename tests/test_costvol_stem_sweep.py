"""Sweep of the cost volume + stem3d0 kernels (rag_amd/csrc/costvol_stem.hip: pre-summed weight variants, the VALU and matrix-core
planes kernels, the combine kernel with its G4 stores and fused tails) over channel counts, geometries, outputs, workspace
handling and non-finite inputs, against
    F.conv3d(O.cost_volume(L, R, maxdisp).double(), w.double(), padding=1)   then scale / shift / ReLU in float64
computed from the features the kernel reads (the bf16-rounded ones under bf16 storage).

Gate, per voxel, nothing excused; mag = F.conv3d(|cost|, |w|) in float64 (the yardstick of test_x3_error_bound_adversarial):
    fp32 FMAs             |out - ref| <= |scale| * 1e-6 * mag
    split operands        |out - ref| <= |scale| * ((2^-20 + 1e-6) * mag + 2^-33 * block)
                          block = Xmax * sum|w| + Wmax * sum|x| of include/rag_amd.h, Xmax tensor-wide
    bf16 storage          the bound of the arithmetic that ran + 2^-8 * |ref|   (round to nearest is 2^-9)
    a fused tail          |s_t| * (sum_co |w_t[k,co]| * bound_main[co] + 1e-6 * sum_co |w_t[k,co] * v_ref[co]|) (+ 2^-8 |ref| under bf16)
"The arithmetic that ran" is the split-operand matrix-core kernel for f16x3 / bf16 with C % 4 == 0, C <= 12 and Cout % 4 == 0,
fp32 FMAs for everything else (include/rag_amd.h) — a row is held to the tighter fp32 bound wherever the header routes it to the
FMAs.  Where mag == 0 (no admissible tap: planes i >= W + 2, ...) the output must be act(shift) bit for bit.  The CPU tests check
the yardstick itself on every row (ATen's float32 convolution stays within 5e-7 * mag; mag > 0 on >= 40 % of the voxels) and that
the geometry rows reach every reachable (cls, tc, xr) class of the kernel file's header.

Two rows answer the CPU tests rather than the plan this file was written to: "far inside the band" is (4,9,16) because (4,7,16)
has mag > 0 on 36.6 % of its voxels only (9 columns: 43 %), and (5,3,4) — W = D - 1 — is there because no other row reaches
(cls = 2, tc = -1, xr = 1).  ops.costvol_stem always has a main output, so
the y-less form (tails only) is not reachable from here and is not run.  The fused rows run at (h, w, D) = (171, 32, 48) and
(497, 33, 16): the candidates (16, 24, 48) and (32, 33, 16) are below what the fused path supports.

Ragged output channel counts (C % 4 == 0, Cout % 4 != 0, f16x3 or bf16): the matrix-core planes kernel stores a lane quarter's four
channels as one float4 at (y * width + xi) * Cout + 4 * kb for every 4 * kb < Cout; with Cout = 5 the kb = 1 quarter covered
channels 4..7 of a 5-float pixel, i.e. channels 0..2 of the next pixel (and 12 bytes past the workspace at its end).  stem_run sends
such Cout to the FMA kernel now; the channel matrix and the guarded-workspace rows below hold those shapes to the gate.

Non-finite inputs: the variant planes have tap columns without an admissible dz (a pre-summed weight that is a sum of nothing).
Multiplying a feature by that zero carried an Inf / NaN to voxels whose window holds a ZERO of the reference's cost volume there
(in the band, on the planes i = 0 and i = D - 1, in the column x = W - 1); both planes kernels leave those columns out now, and
test_non_finite_inputs_stay_local holds the reach to exactly the float64 convolution's.

Every GPU row prints `STEM case=... prec=... worst=err/bound`.  Measured on the MI355X, worst err / bound per family:
  channel matrix   FMAs: fp32 0.189 (C1 o5), f16x3 0.189 (C1 o5), bf16 0.993 (C3 o5)    matrix cores: f16x3 0.074 (C4 o12), bf16 0.991 (C8 o16)
  geometry matrix  FMAs: fp32 0.144 (7x129x2 C12 o12), f16x3 0.141 (3x80x70 C4 o5)     matrix cores: f16x3 0.077 (3x80x70 C12 o12)
  wider out        fp32 0.139, bf16 0.991        tails        fp32 0.207 (k4, C12 o5), bf16 0.979
  workspace rows   f16x3 0.131, bf16 0.992       non-finite   fp32 0.100, f16x3 0.044       fused stems (stem3d0) f16x3 0.070
The bf16 rows sit at 0.96..0.99 of their gate by construction, not for lack of precision: a bf16 value carries 8 significant bits,
so round to nearest moves a value just above a power of two by up to 2^-8 of itself — the storage term of the gate is that worst
case itself, and the arithmetic term on top of it is all the margin there is (the fp32 values underneath are the rows above).

Unmarked tests run without a GPU; the rest need the MI355X."""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import matching_oracle as O

DEV = "cuda:0"
PRECS = ("fp32", "f16x3", "bf16")          # "bf16": bf16 feature / output storage (the conv precision setting does not apply)

# --------------------------------------------------------------------------- rows
CH_GEOM = (2, 9, 21, 5)                    # (B, h, w, D) of the channel matrix
CH_PAIRS = tuple((C, Cout) for C in (1, 3, 4, 8, 12, 16) for Cout in (1, 4, 5, 8, 12, 13, 16))
GEOMS = (
    (1, 1, 1), (1, 1, 3), (2, 1, 4),                                        # W = 1: x = 0 is both borders
    (3, 2, 1), (3, 2, 2), (3, 2, 5),                                        # W = 2
    (5, 3, 3), (5, 4, 3), (5, 5, 3), (5, 3, 5), (5, 3, 6), (5, 3, 4),       # W = D, D+1, D+2, D-2, D-3 (u1_0 clamps at -2), D-1
    (4, 9, 16),                                                             # far inside the band
    (6, 20, 1), (6, 20, 2), (6, 20, 3), (6, 20, 4), (6, 20, 5), (6, 20, 8), (6, 20, 9),      # z classes, CB_NI = 4 remainders
    (8, 64, 3), (9, 65, 3), (17, 66, 4), (7, 129, 2), (1, 68, 3),           # CS_TX / CSM_TX = 64, the 68-column halo, CS_TY = 8, H*W over 256
    (3, 80, 70), (3, 70, 80),                                               # band planes wider than one tile
)
GEOM_B3 = ((9, 65, 3), (5, 3, 5))          # rows run with B = 3 (B = 2 elsewhere)
GEOM_PAIRS = ((12, 12), (4, 5))


def geom_batch(g):
    return 3 if g in GEOM_B3 else 2


def all_rows():
    """(B, C, Cout, h, w, D) of every row of the channel and geometry matrices"""
    B, h, w, D = CH_GEOM
    rows = [(B, C, Cout, h, w, D) for C, Cout in CH_PAIRS]
    rows += [(geom_batch(g), C, Cout) + g for g in GEOMS for C, Cout in GEOM_PAIRS]
    return rows


def gen(seed):
    return torch.Generator().manual_seed(seed)


def v5(t):
    return t.view(1, -1, 1, 1, 1)


def uses_matrix_cores(prec, C, Cout):
    """the routing include/rag_amd.h documents for ragmi_costvol_stem_fwd"""
    return prec in ("f16x3", "bf16") and C % 4 == 0 and C <= 12 and Cout % 4 == 0


@functools.lru_cache(maxsize=None)
def base(B, C, Cout, h, w, D, bf=False, bad=None):
    """Inputs of a row and its float64 pre-activation reference, computed once and shared (never modified).  bf: features rounded
    to bf16.  bad = (side, b, c, y, x, value): the reference is computed with that element zeroed (valid outside its reach) and
    `reach` marks where the float64 convolution of its cost-volume indicator with |w| is nonzero."""
    seed = zlib.crc32(repr((B, C, Cout, h, w, D)).encode()) & 0x7fffffff
    g1 = gen(seed)
    L, R = torch.randn((B, C, h, w), generator=g1), torch.randn((B, C, h, w), generator=g1)
    wt = torch.randn((Cout, 2 * C, 3, 3, 3), generator=g1) * 0.1
    scale, shift = torch.rand(Cout, generator=g1) + 0.5, torch.randn(Cout, generator=g1) * 0.1
    if bf:
        L, R = L.to(torch.bfloat16).float(), R.to(torch.bfloat16).float()
    out = {"L": L, "R": R, "wt": wt, "scale": scale, "shift": shift, "key": (B, C, Cout, h, w, D)}
    Lr, Rr = L, R
    if bad is not None:
        side, b, c, y, x, val = bad
        Li, Ri = torch.zeros_like(L), torch.zeros_like(R)
        (Li if side == "L" else Ri)[b, c, y, x] = 1.0
        out["reach"] = F.conv3d(O.cost_volume(Li, Ri, 3 * D).double(), wt.double().abs(), padding=1) > 0
        Lr, Rr = L.clone(), R.clone()
        (Lr if side == "L" else Rr)[b, c, y, x] = 0.0
        Lb, Rb = L.clone(), R.clone()
        (Lb if side == "L" else Rb)[b, c, y, x] = val
        out["L"], out["R"] = Lb, Rb
    cost = O.cost_volume(Lr, Rr, 3 * D).double()
    w64 = wt.double()
    out["pre"] = F.conv3d(cost, w64, padding=1)
    out["mag"] = F.conv3d(cost.abs(), w64.abs(), padding=1)
    sum_x = F.conv3d(cost.abs(), torch.ones((1, 2 * C, 3, 3, 3), dtype=torch.float64), padding=1)
    wmax, sum_w = v5(w64.abs().flatten(1).max(dim=1).values), v5(w64.abs().flatten(1).sum(dim=1))
    out["block"] = float(cost.abs().max()) * sum_w + wmax * sum_x
    out["cost32"] = cost.float()
    return out


def reference(c, bn, relu):
    ref = c["pre"] * v5(c["scale"].double()) + v5(c["shift"].double()) if bn else c["pre"]
    return F.relu(ref) if relu else ref


def arith_bound(c, prec, bn):
    """bound of the arithmetic that ran, without the storage term"""
    C, Cout = c["key"][1], c["key"][2]
    if uses_matrix_cores(prec, C, Cout):
        b = (2.0 ** -20 + 1e-6) * c["mag"] + 2.0 ** -33 * c["block"]
    else:
        b = 1e-6 * c["mag"]
    return b * v5(c["scale"].double().abs()) if bn else b


def gate(c, prec, bn, relu):
    """(ref, bound) of the main output"""
    ref = reference(c, bn, relu)
    b = arith_bound(c, prec, bn)
    return ref, (b + 2.0 ** -8 * ref.abs() if prec == "bf16" else b)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check(tag, prec, out, ref, bound, c=None, bn=False, relu=False, where=None):
    """every voxel (of `where`) inside the bound; with `c`: act(shift) bit for bit where mag == 0.  Returns the worst err / bound."""
    got = out.detach().cpu()
    g64 = got.double()
    sel = torch.ones_like(ref, dtype=torch.bool) if where is None else where.expand_as(ref)
    assert torch.isfinite(g64[sel]).all(), (tag, prec, "non-finite output")
    err = (g64 - ref).abs()
    if c is not None:
        zero = (c["mag"] == 0) & sel
        if zero.any():
            act0 = (c["shift"] if bn else torch.zeros_like(c["shift"]))
            act0 = v5(F.relu(act0) if relu else act0).to(got.dtype).expand_as(got)
            assert torch.equal(bits(got)[zero], bits(act0.contiguous())[zero]), (tag, prec, "voxels without a tap are not act(shift) exactly")
        sel = sel & ~zero
    if not sel.any():
        print(f"STEM case={tag} prec={prec} worst=0/0 (no voxel with a tap)")
        return 0.0
    ratio = err[sel] / bound[sel].clamp_min(1e-300)
    k = int(ratio.argmax())
    print(f"STEM case={tag} prec={prec} worst={float(err[sel][k]):.3e}/{float(bound[sel][k]):.3e} = {float(ratio[k]):.3f}")
    assert float(ratio[k]) <= 1.0, (tag, prec, float(ratio[k]))
    return float(ratio[k])


# --------------------------------------------------------------------------- CPU: the yardstick and the rows themselves
def voxel_classes(h, w, D):
    """{(cls, tc, xr)} of a volume, as rag_amd/csrc/costvol_stem.hip's header defines them"""
    return {((1 if i == 0 else 0) + (2 if i == D - 1 else 0), min(max(x - i, -3), 2), 1 if x == w - 1 else 0)
            for i in range(D) for x in range(w)}


def test_geometry_rows_reach_every_class():
    """cls 1 and 3 are the plane i = 0, where tc = min(x, 2) >= 0; everything else occurs"""
    reachable = {(cls, tc, xr) for cls in range(4) for tc in range(-3, 3) for xr in range(2) if tc >= 0 or not (cls & 1)}
    seen = set()
    for (h, w, D) in GEOMS:
        seen |= voxel_classes(h, w, D)
    assert seen <= reachable
    assert seen == reachable, sorted(reachable - seen)
    assert {c[0] for c in seen} == {0, 1, 2, 3} and {c[1] for c in seen} == set(range(-3, 3)) and {c[2] for c in seen} == {0, 1}


@pytest.mark.parametrize("row", all_rows(), ids=lambda r: "B{}C{}o{}_{}x{}x{}".format(*r))
def test_yardstick_is_sound_on_every_row(row):
    """ATen's own float32 convolution stays within 5e-7 * mag of float64 (the gates leave 2x over it), and mag > 0 on at least 40 %
    of the voxels: no row tests mostly zeros."""
    c = base(*row)
    y32 = F.conv3d(c["cost32"], c["wt"], padding=1).double()
    assert bool(((y32 - c["pre"]).abs() <= 5e-7 * c["mag"]).all())
    share = float((c["mag"] > 0).double().mean())
    assert share >= 0.40, share


def test_ragged_store_of_the_matrix_core_planes_leaves_its_pixel():
    """The store indexing of costvol_stem_planes_mfma_body on the host: lane quarter kb of pixel p writes floats
    [p * Cout + 4 kb, p * Cout + 4 kb + 4) for 4 kb < Cout.  With Cout % 4 == 0 that tiles every pixel exactly; with a ragged Cout it
    covers floats of pixel p + 1 and runs past the plane set — so the header's routing must keep ragged Cout off that kernel."""
    def stores(Cout, npix):
        return [(p, range(p * Cout + 4 * kb, p * Cout + 4 * kb + 4)) for p in range(npix) for kb in range(4) if 4 * kb < Cout]
    for Cout in range(1, 17):
        npix = 6
        outside = [(p, f) for p, r in stores(Cout, npix) for f in r if not p * Cout <= f < (p + 1) * Cout]
        assert (not outside) == (Cout % 4 == 0), Cout
        assert (max(f for _p, r in stores(Cout, npix) for f in r) >= npix * Cout) == (Cout % 4 != 0)      # past the workspace's end
        assert not uses_matrix_cores("f16x3", 12, Cout) or Cout % 4 == 0
    assert [f for p, r in stores(5, 2) if p == 0 for f in r if f >= 5] == [5, 6, 7]      # Cout = 5: channels 0..2 of pixel 1


# --------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ra():
    import rag_amd
    rag_amd.load_library()
    return rag_amd


def gpu(x):
    return torch.as_tensor(x).to(DEV)


def run_stem(ra, c, prec, bn, relu, **kw):
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    D, Cout = c["key"][5], c["key"][2]
    with ra.ops.conv_precision("f16x3" if prec == "bf16" else prec):
        var = ra.ops.costvol_stem_prepare(gpu(c["wt"]))
        out = ra.ops.costvol_stem(gpu(c["L"]).to(dt), gpu(c["R"]).to(dt), 3 * D, var, Cout, gpu(c["scale"]) if bn else None,
                                  gpu(c["shift"]) if bn else None, relu, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C,Cout", CH_PAIRS)
def test_channel_matrix(ra, C, Cout, prec):
    """every COUT4 / NCG / NC instantiation in both storage types, C = 16 falling back to the FMAs, ragged Cout off the matrix cores"""
    B, h, w, D = CH_GEOM
    c = base(B, C, Cout, h, w, D, prec == "bf16")
    out = run_stem(ra, c, prec, True, True)
    ref, bound = gate(c, prec, True, True)
    check(f"ch_C{C}o{Cout}", prec, out, ref, bound, c, True, True)


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [True, False], ids=["bnrelu", "plain"])
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("C,Cout", GEOM_PAIRS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "{}x{}x{}".format(*g))
def test_geometry_matrix(ra, geom, C, Cout, prec, bn):
    h, w, D = geom
    c = base(geom_batch(geom), C, Cout, h, w, D)
    out = run_stem(ra, c, prec, bn, bn)
    ref, bound = gate(c, prec, bn, bn)
    check(f"geo_{h}x{w}x{D}_C{C}o{Cout}_{'bnrelu' if bn else 'plain'}", prec, out, ref, bound, c, bn, bn)


SENT = -12345.678


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("C,Cout", [(12, 12), (12, 5), (4, 8)])
def test_outputs_and_tails(ra, C, Cout, prec):
    """A wider `out` keeps its other channels; the G4 store equals the plane store; two tails (1, 3 or 4 channels at a nonzero
    y_ch0 of a wider buffer, one of them G4) stay inside the tail bound and leave their neighbours alone."""
    B, h, w, D = 2, 6, 40, 8
    c = base(B, C, Cout, h, w, D, prec == "bf16")
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    ref, bound = gate(c, prec, True, True)
    wide = torch.full((B, Cout + 3, D, h, w), SENT, device=DEV, dtype=dt)
    keep = bits(wide[:, Cout:].cpu())
    run_stem(ra, c, prec, True, True, out=wide)
    assert torch.equal(bits(wide[:, Cout:].cpu()), keep)
    check(f"out_wide_C{C}o{Cout}", prec, wide[:, :Cout], ref, bound, c, True, True)
    if Cout % 4 == 0:
        g4 = run_stem(ra, c, prec, True, True, out_g4=True)
        assert torch.equal(bits(ra.ops.from_g4(g4).cpu()), bits(wide[:, :Cout].contiguous().cpu()))
    # tails: (cout, y_ch0, BN, ReLU, g4) into 8- and 12-channel sentinel buffers
    g1 = gen(977 + C * 17 + Cout)
    specs = [[(1, 5, True, True, False), (3, 2, False, False, False)], [(4, 4, True, False, True), (3, 1, True, True, False)]]
    v_ref, b_main = ref, arith_bound(c, prec, True)
    for si, pair in enumerate(specs):
        bufs, tails, exp = [], [], []
        for (k, ch0, tbn, trelu, tg4) in pair:
            if tg4 and prec == "bf16":
                tg4 = False                    # (ops.Tail's G4 destinations are fp32 tensors)
            tw = torch.randn((k, Cout), generator=g1) * 0.3
            ts, th = torch.rand(k, generator=g1) + 0.5, torch.randn(k, generator=g1) * 0.1
            buf = torch.full((B, 12 if tg4 else 8, D, h, w), SENT, device=DEV, dtype=dt)
            bufs.append(buf)
            tails.append(ra.ops.Tail(gpu(tw), gpu(ts) if tbn else None, gpu(th) if tbn else None, trelu, buf, ch0, g4=tg4))
            t64 = torch.einsum("kc,bcdhw->bkdhw", tw.double(), v_ref)
            tb = torch.einsum("kc,bcdhw->bkdhw", tw.double().abs(), b_main) + 1e-6 * torch.einsum("kc,bcdhw->bkdhw", tw.double().abs(), v_ref.abs())
            if tbn:
                t64, tb = t64 * v5(ts.double()) + v5(th.double()), tb * v5(ts.double().abs())
            t64 = F.relu(t64) if trelu else t64
            exp.append((t64, tb + 2.0 ** -8 * t64.abs() if prec == "bf16" else tb))
        main = run_stem(ra, c, prec, True, True, tails=tails)
        assert torch.equal(bits(main.cpu()), bits(wide[:, :Cout].contiguous().cpu()))
        for (k, ch0, _tbn, _trelu, tg4), buf, (t64, tb) in zip(pair, bufs, exp):
            planes = ra.ops.from_g4(buf) if (tg4 and prec != "bf16") else buf
            check(f"tail{si}_k{k}_C{C}o{Cout}", prec, planes[:, ch0:ch0 + k], t64, tb)
            other = [ch for ch in range(planes.shape[1]) if not ch0 <= ch < ch0 + k]
            assert bool((planes[:, other].float() == torch.tensor(SENT, dtype=dt).float()).all()), "a tail wrote outside its channels"


def guarded_workspace(ra, c):
    B, C, Cout, h, w, D = c["key"]
    n = ra.load_library().ragmi_costvol_stem_workspace_elems(B, C, Cout, D, h, w)
    big = torch.full((n + 128,), SENT, device=DEV)
    ws = big[64:64 + n]
    ws.fill_(float("nan"))
    return big, ws, n


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f16x3", "bf16"])
@pytest.mark.parametrize("B,C,Cout,h,w,D", [(2, 12, 5, 9, 21, 5), (2, 4, 13, 9, 21, 5), (3, 12, 12, 9, 65, 3), (2, 12, 12, 3, 80, 70)])
def test_workspace_contract_and_determinism(ra, B, C, Cout, h, w, D, prec):
    """The planes stay inside ragmi_costvol_stem_workspace_elems floats (64 guard floats on each side keep their bits: a ragged Cout on
    the matrix-core kernel ran 12 bytes over), no unwritten (NaN) plane element reaches an output, and a second call gives the same bits."""
    c = base(B, C, Cout, h, w, D, prec == "bf16")
    ref, bound = gate(c, prec, True, True)
    outs = []
    for _ in range(2):
        big, ws, n = guarded_workspace(ra, c)
        outs.append(run_stem(ra, c, prec, True, True, workspace=ws))
        guards = torch.cat([big[:64], big[64 + n:]]).cpu()
        assert bool((guards == torch.tensor(SENT)).all()), "the planes kernel wrote outside the workspace"
    check(f"ws_C{C}o{Cout}_{h}x{w}x{D}", prec, outs[0], ref, bound, c, True, True)
    assert torch.equal(bits(outs[0].cpu()), bits(outs[1].cpu()))


@pytest.mark.gpu
def test_workspace_argument_is_validated(ra):
    c = base(2, 12, 5, 9, 21, 5)
    _big, ws, n = guarded_workspace(ra, c)
    spare = torch.empty(n + 8, device=DEV)
    for bad in (ws[:n - 1], spare[1:], ws.double(), ws.cpu(), torch.empty(2 * n, device=DEV)[::2]):
        with pytest.raises(ValueError):
            run_stem(ra, c, "fp32", True, True, workspace=bad)
    out = run_stem(ra, c, "fp32", True, True, workspace=spare)      # larger than needed is fine
    assert torch.equal(out, run_stem(ra, c, "fp32", True, True))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("bad", [("L", 1, 5, 3, 2, float("inf")), ("R", 1, 7, 4, 3, float("nan"))], ids=["inf_in_L", "nan_in_R"])
def test_non_finite_inputs_stay_local(ra, bad, prec):
    """include/rag_amd.h: a non-finite feature makes non-finite exactly the outputs whose 3x3x3 window holds it in the reference's
    cost volume; every other voxel keeps the gate.  The bad pixel sits inside the diagonal band (x < D - 2), where variant planes have
    tap columns without an admissible dz (weight 0): multiplying those would carry the value to voxels the reference keeps finite."""
    B, C, Cout, h, w, D = 2, 12, 12, 8, 70, 6
    c = base(B, C, Cout, h, w, D, False, bad)
    out = run_stem(ra, c, prec, True, False)
    ref, bound = gate(c, prec, True, False)
    reach = c["reach"]
    assert reach.any() and not reach[0].any() and reach.sum() < reach.numel() // 50
    assert not torch.isfinite(out.cpu()[reach]).any(), "a non-finite input left a finite output inside its reach"
    check(f"nonfinite_{bad[0]}", prec, torch.where(gpu(reach), torch.zeros_like(out), out), ref, bound, c, True, False, where=~reach)


@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w,maxdisp", [(1, 171, 32, 144), (1, 497, 33, 48)])
def test_fused_stems_inside_the_band(ra, B, h, w, maxdisp):
    """test_costvol_stem_conv3d_fused_bitwise's contract at W <= D (every column inside the band) and W ~ 2 D: the fused stem3d0 +
    stem3d1 call equals the two calls bit for bit, and the two-call stem3d0 output is inside this file's gate.  The shapes are the
    nearest to (16, 24, D = 48) and (32, 33, D = 16) that ragmi_costvol_stem_conv3d_supported accepts — the z-marching kernel wants
    W >= 32 and D * H * W >= 2^18: the same W (32 at least) and D, the smallest such H."""
    C, cmid, cout, d = 12, 12, 12, maxdisp // 3
    c = base(B, C, cmid, h, w, d)
    g1 = gen(563)
    w1 = torch.randn((cout, cmid, 3, 3, 3), generator=g1) * 0.1
    s1, h1 = torch.rand(cout, generator=g1) + 0.5, torch.randn(cout, generator=g1) * 0.1
    tw0 = torch.randn((4, cmid), generator=g1) * 0.3
    tw1 = [torch.randn((4, cout), generator=g1) * 0.3 for _ in range(2)]
    L, R, s0, h0 = gpu(c["L"]), gpu(c["R"]), gpu(c["scale"]), gpu(c["shift"])
    with ra.ops.conv_precision("f16x3"):
        assert ra.ops.costvol_stem_conv3d_supported(C, cmid, cout, B, d, h, w, ntail=2)
        var = ra.ops.costvol_stem_prepare(gpu(c["wt"]))
        pk = ra.ops.conv3d_k3_pack(gpu(w1))
        outs = {}
        for fused in (False, True):
            pre0 = torch.full((B, 8, d, h, w), float("nan"), device=DEV)
            pre1 = torch.full((B, 8, d, h, w), float("nan"), device=DEV)
            t0 = [ra.ops.Tail(gpu(tw0), None, None, True, pre0, 0, g4=True)]
            t1 = [ra.ops.Tail(gpu(tw1[0]), None, None, True, pre0, 4, g4=True), ra.ops.Tail(gpu(tw1[1]), None, None, False, pre1, 0, g4=True)]
            y = torch.full((B, cout, d, h, w), float("nan"), device=DEV)
            if fused:
                ra.ops.costvol_stem_conv3d(L, R, maxdisp, var, cmid, s0, h0, True, t0, pk, cout, gpu(s1), gpu(h1), True, y, None, tails=t1,
                                           store_main=True)
            else:
                mid = ra.ops.costvol_stem(L, R, maxdisp, var, cmid, s0, h0, True, tails=t0, out_g4=True)
                ra.ops.conv3d_k3(mid, pk, cout, gpu(s1), gpu(h1), True, y, None, tails=t1, x_g4=True)
            torch.cuda.synchronize()
            outs[fused] = (y, ra.ops.from_g4(pre0), ra.ops.from_g4(pre1))
    for a_, b_ in zip(outs[True], outs[False]):
        assert torch.equal(torch.nan_to_num(a_, nan=-7.0), torch.nan_to_num(b_, nan=-7.0))
    assert not torch.isnan(outs[True][0]).any() and not torch.isnan(outs[True][1]).any() and torch.isnan(outs[True][2][:, 4:]).all()
    ref, bound = gate(c, "f16x3", True, True)
    check(f"fused_mid_{h}x{w}x{d}", "f16x3", ra.ops.from_g4(mid), ref, bound, c, True, True)
