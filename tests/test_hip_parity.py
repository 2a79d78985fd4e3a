"""GPU parity tests: the HIP path (through the C ABI) vs the CPU oracle and the
reference-generated golden fixtures.  Run with `pytest -m gpu` on the MI355X.

Tolerances: the cost volume is a pure copy -> bit exact.  Everything else is fp32
arithmetic in a different accumulation order than MKL-DNN -> 2e-4 abs/rel per tensor, and
the end-to-end gate of BASELINE.json: EPE <= 1e-3 px vs the CPU reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, split_sd
from oracle import matching_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=2e-4, atol=2e-4)
EPE_GATE = 1e-3


def gpu(x):
    return torch.as_tensor(x).to(DEV)


@pytest.fixture(scope="module")
def ra():
    import rag_amd
    rag_amd.load_library()
    return rag_amd


def gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------- cost volume
@pytest.mark.parametrize("tag", ["a", "b"])
def test_costvol_golden_bit_exact(ra, tag):
    g = load_golden(f"g1_costvol_{tag}")
    out = ra.ops.costvol(gpu(g["left_fea"]), gpu(g["right_fea"]), int(g["maxdisp"]))
    assert np.array_equal(out.cpu().numpy(), g["cost"])


@pytest.mark.parametrize("B,C,h,w,maxdisp", [(1, 12, 4, 8, 24), (2, 3, 5, 7, 30), (1, 12, 3, 5, 48),
                                             (2, 12, 16, 28, 48), (1, 1, 1, 1, 3), (1, 12, 9, 33, 27)])
def test_costvol_vs_oracle_ragged(ra, B, C, h, w, maxdisp):
    L, R = torch.randn((B, C, h, w), generator=gen(1)), torch.randn((B, C, h, w), generator=gen(2))
    ref = O.cost_volume(L, R, maxdisp)
    out = ra.ops.costvol(gpu(L), gpu(R), maxdisp)
    assert torch.equal(out.cpu(), ref)


def test_costvol_full_size_bit_exact(ra):
    """BASELINE config 2 size: [1,24,64,128,416]; the oracle copy loop takes < 1 s."""
    L, R = torch.randn((1, 12, 128, 416), generator=gen(3)), torch.randn((1, 12, 128, 416), generator=gen(4))
    out = ra.ops.costvol(gpu(L), gpu(R), 192).cpu()
    assert torch.equal(out, O.cost_volume(L, R, 192))


# --------------------------------------------------------------------------- disp head
def test_disp_golden(ra):
    g = load_golden("g2_disp")
    out = ra.Disp(int(g["maxdisp"]))(gpu(g["x"]))
    np.testing.assert_allclose(out.cpu().numpy(), g["out"], **TOL)
    out2 = ra.Disp(int(g["maxdisp2"]))(gpu(g["x2"]))
    np.testing.assert_allclose(out2.cpu().numpy(), g["out2"], **TOL)
    reg = ra.DisparityRegression(int(g["maxdisp"]))(gpu(g["prob"]))
    np.testing.assert_allclose(reg.cpu().numpy(), g["reg"], **TOL)


@pytest.mark.parametrize("B,d,h,w,maxdisp,scale", [(2, 16, 6, 10, 48, 1.0), (1, 64, 8, 12, 192, 5.0), (1, 7, 5, 3, 21, 20.0),
                                                   (1, 9, 4, 6, 20, 1.0),
                                                   # every maxdisp == 3 d row, the ones above included, runs the tiled kernel
                                                   # (disp.hip disp_softargmin_x3_kernel); d = 64, maxdisp = 192 runs its register
                                                   # form: costs of the trained net's magnitude, a peaky softmin, and the generic
                                                   # kernel on the same d for a ratio that is not 3
                                                   (1, 64, 20, 33, 192, 1000.0), (2, 64, 6, 9, 192, 1e4), (1, 64, 5, 7, 160, 5.0)])
def test_disp_vs_oracle(ra, B, d, h, w, maxdisp, scale):
    x = torch.randn((B, 1, d, h, w), generator=gen(5)) * scale   # large scale -> peaky softmin, exercises the online rescale
    ref = O.disp_head(x, maxdisp)
    out = ra.ops.disp_softargmin(gpu(x), maxdisp)
    if scale < 1000:
        np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=2e-4, atol=2e-4 * max(1.0, maxdisp / 48))
    else:
        # costs of 1e3-1e4 carry an fp32 rounding of 1e-4..1e-3 into the exponent (the lerp's last bit: fma here, mul + add in
        # ATen), i.e. ~1e-3 relative on the weights of a near-tie between two distant minima: bounded per pixel in proportion to
        # the cost magnitude, gated on average like every end-to-end comparison
        worst = float((out.cpu() - ref).abs().max())
        print(f"disp vs oracle at |cost| ~ {scale:g}: max |err| {worst:.3e} px = {worst / scale:.2e} x scale (bound 5e-6 x scale)")
        assert worst <= 5e-6 * scale              # measured 2.0e-6 x scale on 2 of 972 pixels at 1e4.  Loosened once (round 4); may not grow.
    assert O.epe(out.cpu(), ref) < EPE_GATE


def test_disp_monotone_cost_spike(ra):
    """A cost with one sharp minimum at coarse plane z0 regresses to the fine disparity 3*z0+1 (property test)."""
    d, h, w = 64, 8, 16
    x = torch.full((1, 1, d, h, w), 50.0)
    x[:, :, 20] = -50.0
    out = ra.ops.disp_softargmin(gpu(x), 192).cpu()
    assert torch.allclose(out, torch.full_like(out, 61.0), atol=1e-3)


# --------------------------------------------------------------------------- ConvBR_3d
@pytest.mark.parametrize("name", ["k3", "k3_wide", "k1", "k3_nobn"])
def test_convbr_golden(ra, name):
    g = load_golden("g3_convbr")
    cin, cout, k, pad, bn, relu = [int(v) for v in g[f"{name}::cfg"]]
    m = ra.ConvBR_3d(cin, cout, k, 1, pad, bn=bool(bn), relu=bool(relu))
    m.load_state_dict(split_sd(g, f"{name}::sd::"))
    m = m.to(DEV).eval()
    with torch.no_grad():
        y = m(gpu(g[f"{name}::x"]))
    np.testing.assert_allclose(y.cpu().numpy(), g[f"{name}::y_eval"], **TOL)


@pytest.mark.parametrize("cin,cout,shape", [(4, 4, (1, 4, 8, 32)), (4, 12, (2, 5, 9, 33)), (24, 12, (1, 6, 10, 40)),
                                            (12, 12, (1, 3, 17, 70)), (8, 8, (1, 8, 16, 13)), (16, 16, (2, 4, 8, 26)),
                                            (12, 1, (1, 5, 12, 20)), (3, 5, (1, 2, 3, 5)), (7, 9, (1, 9, 6, 11)),
                                            (4, 4, (1, 1, 1, 1)), (16, 48, (1, 4, 8, 26)), (4, 4, (1, 64, 20, 96))])
def test_conv3d_k3_vs_oracle(ra, cin, cout, shape):
    B, D, H, W = shape
    x = torch.randn((B, cin, D, H, W), generator=gen(6))
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen(7)) * (2.0 / (27 * cin)) ** 0.5
    scale, shift = torch.rand(cout, generator=gen(8)) + 0.5, torch.randn(cout, generator=gen(9)) * 0.1
    ref = F.relu(F.conv3d(x, w, padding=1) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1))
    ref2 = O.conv3d_explicit(x.numpy(), w.numpy(), 1) if x.numel() * cout < 2e6 else None
    packed = ra.ops.conv3d_k3_pack(gpu(w))
    out = torch.full((B, cout, D, H, W), float("nan"), device=DEV)
    ra.ops.conv3d_k3(gpu(x), packed, cout, gpu(scale), gpu(shift), True, out)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), **TOL)
    if ref2 is not None:  # raw conv, no BN/ReLU, against the explicit float64 restatement
        raw = torch.empty((B, cout, D, H, W), device=DEV)
        ra.ops.conv3d_k3(gpu(x), packed, cout, None, None, False, raw)
        np.testing.assert_allclose(raw.cpu().numpy(), ref2, **TOL)


def test_conv3d_k3_slices_residual_and_accumulate(ra):
    """Channel-slice input/output, per-group destination channels, residual from another buffer, and in-place accumulate."""
    B, D, H, W = 2, 5, 7, 19
    big_in = torch.randn((B, 10, D, H, W), generator=gen(10))
    w = torch.randn((8, 4, 3, 3, 3), generator=gen(11)) * 0.1
    res = torch.randn((B, 6, D, H, W), generator=gen(12))
    x = big_in[:, 3:7]
    conv = F.relu(F.conv3d(x, w, padding=1))
    out = torch.zeros((B, 16, D, H, W), device=DEV)
    packed = ra.ops.conv3d_k3_pack(gpu(w))
    xg = gpu(big_in)[:, 3:7]
    ra.ops.conv3d_k3(xg, packed, 8, None, None, True, out, [8, 0], gpu(res), [2, 0])
    exp = torch.zeros((B, 16, D, H, W))
    exp[:, 8:12] = conv[:, 0:4] + res[:, 2:6]
    exp[:, 0:4] = conv[:, 4:8] + res[:, 0:4]
    np.testing.assert_allclose(out.cpu().numpy(), exp.numpy(), **TOL)
    ra.ops.conv3d_k3(xg, packed, 8, None, None, True, out, [8, 0], out, [8, 0])   # accumulate in place
    exp[:, 8:12] += conv[:, 0:4]
    exp[:, 0:4] += conv[:, 4:8]
    np.testing.assert_allclose(out.cpu().numpy(), exp.numpy(), **TOL)


@pytest.mark.parametrize("ca,cb,cout,shape", [(4, 4, 12, (1, 5, 9, 33)), (8, 8, 24, (2, 4, 8, 20)), (16, 16, 48, (1, 4, 8, 13)),
                                              (4, 4, 4, (1, 3, 5, 7)), (4, 3, 8, (1, 6, 10, 40)), (4, 4, 12, (1, 64, 24, 96))])
def test_conv3d_k3_dual_vs_oracle(ra, ca, cb, cout, shape):
    """out = relu(bnA(convA(x[:, :ca]))) + relu(bnB(convB(x[:, ca:]))) + res, in one launch."""
    B, D, H, W = shape
    x = torch.randn((B, ca + cb, D, H, W), generator=gen(20))
    wa = torch.randn((cout, ca, 3, 3, 3), generator=gen(21)) * (2.0 / (27 * ca)) ** 0.5
    wb = torch.randn((cout, cb, 3, 3, 3), generator=gen(22)) * (2.0 / (27 * cb)) ** 0.5
    sa, ha = torch.rand(cout, generator=gen(23)) + 0.5, torch.randn(cout, generator=gen(24)) * 0.1
    sb, hb = torch.rand(cout, generator=gen(25)) + 0.5, torch.randn(cout, generator=gen(26)) * 0.1
    res = torch.randn((B, cout, D, H, W), generator=gen(27))
    v = lambda t: t.view(1, -1, 1, 1, 1)  # noqa: E731
    ref = F.relu(F.conv3d(x[:, :ca], wa, padding=1) * v(sa) + v(ha)) + F.relu(F.conv3d(x[:, ca:], wb, padding=1) * v(sb) + v(hb))
    out = torch.full((B, cout, D, H, W), float("nan"), device=DEV)
    pa, pb = ra.ops.conv3d_k3_pack(gpu(wa)), ra.ops.conv3d_k3_pack(gpu(wb))
    ra.ops.conv3d_k3_dual(gpu(x), ca, pa, gpu(sa), gpu(ha), pb, gpu(sb), gpu(hb), cout, True, out)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), **TOL)
    ra.ops.conv3d_k3_dual(gpu(x), ca, pa, gpu(sa), gpu(ha), pb, gpu(sb), gpu(hb), cout, True, out, None, gpu(res), None)
    np.testing.assert_allclose(out.cpu().numpy(), (ref + res).numpy(), **TOL)


@pytest.mark.parametrize("cin,cout,shape", [(12, 1, (1, 5, 12, 40)), (12, 1, (2, 3, 7, 9)), (4, 2, (1, 6, 10, 20)), (12, 1, (1, 64, 16, 96))])
def test_conv3d_k3_small_vs_oracle(ra, cin, cout, shape):
    """VALU form for Cout <= 2 (last_3_3d)."""
    B, D, H, W = shape
    x = torch.randn((B, cin, D, H, W), generator=gen(30))
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen(31)) * (2.0 / (27 * cin)) ** 0.5
    res = torch.randn((B, cout + 1, D, H, W), generator=gen(32))
    ref = F.conv3d(x, w, padding=1)
    out = torch.full((B, cout, D, H, W), float("nan"), device=DEV)
    ra.ops.conv3d_k3_small(gpu(x), gpu(w), None, None, False, out)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), **TOL)
    scale, shift = torch.rand(cout, generator=gen(33)) + 0.5, torch.randn(cout, generator=gen(34)) * 0.1
    ra.ops.conv3d_k3_small(gpu(x), gpu(w), gpu(scale), gpu(shift), True, out, 0, gpu(res), 1)
    exp = F.relu(ref * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)) + res[:, 1:1 + cout]
    np.testing.assert_allclose(out.cpu().numpy(), exp.numpy(), **TOL)


@pytest.mark.parametrize("cin,shape,dtype,bn", [
    (12, (1, 64, 128, 416), "f32", False),     # last_3_3d of the headline forward (rag_model.py:269, :361-365)
    (12, (2, 9, 140, 260), "f32", True),       # two pairs; partial tiles in y and x, a partial last depth segment, folded BN + ReLU
    (4, (1, 33, 129, 64), "f32", False),       # one row past a tile border
    (12, (1, 16, 64, 256), "bf16", False)])    # bf16 activation storage, fp32 output (the head's `mat` stays fp32)
def test_conv3d_c1_single_output_channel_form(ra, cin, shape, dtype, bn):
    """conv3d_c1_kernel (input-stationary z-marching VALU form, Cout = 1, volumes >= 2^18 voxels per sample, W % 4 == 0) behind
    ragmi_conv3d_k3_small_fwd_ex, against F.conv3d in float64; written into a channel slice of a wider buffer."""
    B, D, H, W = shape
    assert D * H * W >= 1 << 18 and W % 4 == 0
    bf = dtype == "bf16"
    x = torch.randn((B, cin, D, H, W), generator=gen(35))
    if bf:
        x = x.to(torch.bfloat16)
    w = torch.randn((1, cin, 3, 3, 3), generator=gen(36)) * (2.0 / (27 * cin)) ** 0.5
    ref = F.conv3d(x.double(), w.double(), padding=1)
    scale = shift = None
    if bn:
        scale, shift = torch.rand(1, generator=gen(37)) + 0.5, torch.randn(1, generator=gen(38)) * 0.1
        ref = F.relu(ref * scale.double() + shift.double())
    out = torch.full((B, 3, D, H, W), float("nan"), device=DEV)
    ra.ops.conv3d_k3_small(gpu(x), gpu(w), gpu(scale) if bn else None, gpu(shift) if bn else None, bn, out, 1)
    got = out.cpu()
    assert torch.isnan(got[:, 0]).all() and torch.isnan(got[:, 2]).all()         # the neighbouring channels are untouched
    np.testing.assert_allclose(got[:, 1:2].double().numpy(), ref.numpy(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("cin,shape,dtype,bn", [
    (12, (1, 32, 64, 208), "f32", False),      # the headline head: [1,12,32,64,208] -> mat [1,1,64,128,416] (rag_model.py:357-365)
    (12, (2, 5, 37, 50), "f32", True),         # two pairs; odd input sizes: partial tiles everywhere, partial depth segment; BN + ReLU
    (4, (1, 2, 2, 2), "f32", False),           # the smallest volume: every voxel is a border voxel
    (8, (1, 7, 33, 18), "f32", False),         # a tile border one row past 64 output rows
    (12, (1, 8, 40, 80), "bf16", False)])      # bf16 activation storage, fp32 output
def test_upconv3d_c1_fused_head_vs_oracle(ra, cin, shape, dtype, bn):
    """upconv3d_c1_kernel: conv3x3x3(Upsample(x2, trilinear, align_corners=True)(x)) with one output channel, the upsampled tensor
    never materialised — against ATen's fp32 F.interpolate + F.conv3d in float64, AND against this library's own two-kernel path (standalone
    upsample + conv3d_c1 / generic small-Cout kernel), which evaluates the same fp32 source indices."""
    B, Di, Hi, Wi = shape
    bf = dtype == "bf16"
    x = torch.randn((B, cin, Di, Hi, Wi), generator=gen(41))
    if bf:
        x = x.to(torch.bfloat16)
    w = torch.randn((1, cin, 3, 3, 3), generator=gen(42)) * (2.0 / (27 * cin)) ** 0.5
    # the reference's arithmetic: ATen's fp32 upsample (fp32 source indices: up to 4e-5 from an exact interpolation at an index of
    # ~400), then the convolution — summed in float64 here
    up = F.interpolate(x.float(), scale_factor=2, mode="trilinear", align_corners=True)
    ref = F.conv3d(up.double(), w.double(), padding=1)
    scale = shift = None
    if bn:
        scale, shift = torch.rand(1, generator=gen(43)) + 0.5, torch.randn(1, generator=gen(44)) * 0.1
        ref = F.relu(ref * scale.double() + shift.double())
    assert ra.ops.upconv3d_c1_supported(cin, Di, Hi, Wi)
    out = torch.full((B, 2, 2 * Di, 2 * Hi, 2 * Wi), float("nan"), device=DEV)
    ra.ops.upconv3d_c1(gpu(x), gpu(w), gpu(scale) if bn else None, gpu(shift) if bn else None, bn, out, 1)
    got = out.cpu()
    assert torch.isnan(got[:, 0]).all()
    np.testing.assert_allclose(got[:, 1:2].double().numpy(), ref.numpy(), rtol=3e-5, atol=3e-5)
    # the two-kernel path of this library (fp32 upsample written to HBM, then the convolution): same source indices, same products
    two = torch.empty((B, 1, 2 * Di, 2 * Hi, 2 * Wi), device=DEV)
    ra.ops.conv3d_k3_small(ra.ops.trilinear3d(gpu(x), (2 * Di, 2 * Hi, 2 * Wi), True), gpu(w), gpu(scale) if bn else None,
                           gpu(shift) if bn else None, bn, two)
    if not bf:           # (bf16 storage rounds the materialised upsample to bf16; the fused kernel keeps it in fp32)
        np.testing.assert_allclose(got[:, 1:2].numpy(), two.cpu().numpy(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("store_main", [True, False])
@pytest.mark.parametrize("shape", [(1, 5, 9, 33), (2, 4, 8, 20), (1, 64, 16, 64)])
def test_conv3d_k3_fused_tails_vs_oracle(ra, dual, store_main, shape):
    """Consumer 1x1x1 ConvBRs computed in the producing 3x3x3 kernel's epilogue; optionally without storing the producer."""
    B, D, H, W = shape
    cout = 12
    x = torch.randn((B, 8 if dual else 24, D, H, W), generator=gen(50))
    v = lambda t_: t_.view(1, -1, 1, 1, 1)  # noqa: E731
    sa, ha = torch.rand(cout, generator=gen(53)) + 0.5, torch.randn(cout, generator=gen(54)) * 0.1
    if dual:
        wa = torch.randn((cout, 4, 3, 3, 3), generator=gen(51)) * 0.1
        wb = torch.randn((cout, 4, 3, 3, 3), generator=gen(52)) * 0.1
        sb, hb = torch.rand(cout, generator=gen(55)) + 0.5, torch.randn(cout, generator=gen(56)) * 0.1
        main = F.relu(F.conv3d(x[:, :4], wa, padding=1) * v(sa) + v(ha)) + F.relu(F.conv3d(x[:, 4:], wb, padding=1) * v(sb) + v(hb))
    else:
        wa = torch.randn((cout, 24, 3, 3, 3), generator=gen(51)) * 0.05
        main = F.relu(F.conv3d(x, wa, padding=1) * v(sa) + v(ha))
    tw = [torch.randn((4, cout), generator=gen(57)) * 0.3, torch.randn((3, cout), generator=gen(58)) * 0.3]
    ts = [(torch.rand(4, generator=gen(59)) + 0.5, torch.randn(4, generator=gen(60)) * 0.1), (None, None)]
    exp0 = F.relu(F.conv3d(main, tw[0].view(4, cout, 1, 1, 1)) * v(ts[0][0]) + v(ts[0][1]))
    exp1 = F.conv3d(main, tw[1].view(3, cout, 1, 1, 1))
    out = torch.full((B, cout, D, H, W), -7.0, device=DEV)
    t0 = torch.zeros((B, 8, D, H, W), device=DEV)
    t1 = torch.zeros((B, 5, D, H, W), device=DEV)
    tails = [ra.ops.Tail(gpu(tw[0]), gpu(ts[0][0]), gpu(ts[0][1]), True, t0, 4), ra.ops.Tail(gpu(tw[1]), None, None, False, t1, 1)]
    if dual:
        ra.ops.conv3d_k3_dual(gpu(x), 4, ra.ops.conv3d_k3_pack(gpu(wa)), gpu(sa), gpu(ha), ra.ops.conv3d_k3_pack(gpu(wb)), gpu(sb),
                              gpu(hb), cout, True, out, tails=tails, store_main=store_main)
    else:
        ra.ops.conv3d_k3(gpu(x), ra.ops.conv3d_k3_pack(gpu(wa)), cout, gpu(sa), gpu(ha), True, out, tails=tails, store_main=store_main)
    if store_main:
        np.testing.assert_allclose(out.cpu().numpy(), main.numpy(), **TOL)
    else:
        assert float((out + 7.0).abs().max()) == 0.0            # untouched
    np.testing.assert_allclose(t0[:, 4:8].cpu().numpy(), exp0.numpy(), **TOL)
    np.testing.assert_allclose(t1[:, 1:4].cpu().numpy(), exp1.numpy(), **TOL)
    assert float(t0[:, :4].abs().max()) == 0.0 and float(t1[:, :1].abs().max()) == 0.0 and float(t1[:, 4:].abs().max()) == 0.0


def test_conv3d_linearity_full_size(ra):
    """Size-independent property at the headline level-3 shape: conv(a*x1 + x2) == a*conv(x1) + conv(x2)."""
    D, H, W = 64, 128, 416
    x1, x2 = torch.randn((1, 4, D, H, W), device=DEV), torch.randn((1, 4, D, H, W), device=DEV)
    packed = ra.ops.conv3d_k3_pack(torch.randn((12, 4, 3, 3, 3), device=DEV) * 0.1)
    outs = []
    for x in (x1, x2, 2.5 * x1 + x2):
        o = torch.empty((1, 12, D, H, W), device=DEV)
        ra.ops.conv3d_k3(x, packed, 12, None, None, False, o)
        outs.append(o)
    err = (outs[2] - (2.5 * outs[0] + outs[1])).abs().max().item()
    assert err < 3e-4, err      # level-3 volumes run on the f16x3 kernel: ~5e-6 relative per output (fp32 MFMA: ~6e-7)


@pytest.mark.parametrize("cin,cout,shape", [(12, 4, (2, 4, 6, 8)), (48, 24, (1, 4, 8, 26)), (24, 12, (1, 3, 5, 7)),
                                            (12, 16, (1, 2, 4, 6)), (5, 3, (1, 3, 3, 3)), (48, 8, (1, 8, 16, 52))])
def test_conv3d_k1_vs_oracle(ra, cin, cout, shape):
    B, D, H, W = shape
    x = torch.randn((B, cin, D, H, W), generator=gen(13))
    w = torch.randn((cout, cin, 1, 1, 1), generator=gen(14)) * (2.0 / cin) ** 0.5
    scale, shift = torch.rand(cout, generator=gen(15)) + 0.5, torch.randn(cout, generator=gen(16)) * 0.1
    ref = F.relu(F.conv3d(x, w) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1))
    out = torch.zeros((B, cout + 3, D, H, W), device=DEV)
    ra.ops.conv3d_k1(gpu(x), gpu(w.reshape(cout, cin)), gpu(scale), gpu(shift), True, out, 2)
    np.testing.assert_allclose(out[:, 2:2 + cout].cpu().numpy(), ref.numpy(), **TOL)
    assert float(out[:, :2].abs().max()) == 0.0 and float(out[:, 2 + cout:].abs().max()) == 0.0


# --------------------------------------------------------------------------- trilinear
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("shape,size", [((2, 3, 8, 12, 20), (4, 6, 10)), ((1, 2, 7, 9, 13), (4, 5, 7)),
                                        ((1, 2, 3, 4, 5), (6, 8, 10)), ((1, 12, 16, 32, 26), (32, 64, 52)),
                                        ((1, 4, 5, 5, 5), (5, 5, 5)), ((1, 2, 64, 32, 104), (32, 16, 52)),
                                        # the tiled up-sampling kernel (every scale <= 0.5): ragged tiles, ratios above two, two batches
                                        ((2, 3, 5, 7, 9), (13, 17, 40)), ((1, 5, 9, 6, 33), (18, 12, 67)),
                                        # degenerate extents (a single input plane / row) and one channel
                                        ((1, 2, 1, 3, 4), (2, 6, 8)), ((1, 1, 4, 1, 40), (8, 2, 80))])
def test_trilinear_vs_aten(ra, align, shape, size):
    x = torch.randn(shape, generator=gen(17))
    ref = F.interpolate(x, size, mode="trilinear", align_corners=align)
    out = ra.ops.trilinear3d(gpu(x), size, align)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape,couts,dtype", [((1, 12, 16, 128, 512), (8, 8), "f32"),     # cell 3's pair at a quarter of the headline depth
                                               ((2, 12, 8, 256, 520), (8, 4), "f32"),      # two samples, different output widths per conv
                                               ((1, 8, 16, 128, 512), (8, 8), "bf16")])
def test_k1_resample_pair_big_volume_down2(ra, shape, couts, dtype):
    """x0.5 down-sampling (align_corners=True) + 1x1x1 ConvBR pairs on volumes of >= 2^20 voxels (rag_model.py:146-155 for cell 3:
    the level 3 -> 6 pair, the HBM-bound launch) — against ATen's fp32 F.interpolate followed by the channel mix in float64.  The
    interpolation is ATen's bit for bit, so the tolerance is that of the 1x1x1 sum alone.  (Round 4 measured a 16-byte-per-lane
    "streaming" form of this kernel — two outputs per thread — against the shipped 8-byte pair loads, which are contiguous across
    lanes already: 88-93 us vs 68 us; not kept.)"""
    B, C, Di, Hi, Wi = shape
    assert Di * Hi * Wi >= 1 << 20
    size = (Di // 2, Hi // 2, Wi // 2)
    bf = dtype == "bf16"
    xs = [torch.randn(shape, generator=gen(61 + k)) for k in range(2)]
    if bf:
        xs = [x.to(torch.bfloat16) for x in xs]
    ws = [torch.randn((co, C), generator=gen(63 + k)) * 0.3 for k, co in enumerate(couts)]
    sc = [torch.rand(co, generator=gen(65 + k)) + 0.5 for k, co in enumerate(couts)]
    sh = [torch.randn(co, generator=gen(67 + k)) * 0.1 for k, co in enumerate(couts)]
    out = torch.full((B, sum(couts) + 1) + size, float("nan"), device=DEV, dtype=torch.bfloat16 if bf else torch.float32)
    specs = [(gpu(xs[0]), gpu(ws[0]), gpu(sc[0]), gpu(sh[0]), True, 0), (gpu(xs[1]), gpu(ws[1]), gpu(sc[1]), gpu(sh[1]), False, couts[0])]
    ra.ops.conv3d_k1_resample_pair(specs, size, out)
    got = out.float().cpu()
    ch0 = 0
    for k, co in enumerate(couts):
        up = F.interpolate(xs[k].float(), size, mode="trilinear", align_corners=True).double()
        ref = torch.einsum("oc,bcdhw->bodhw", ws[k].double(), up) * sc[k].double().view(1, -1, 1, 1, 1) + sh[k].double().view(1, -1, 1, 1, 1)
        ref = F.relu(ref) if k == 0 else ref
        tol = dict(rtol=1e-2, atol=3e-2) if bf else dict(rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(got[:, ch0:ch0 + co].double().numpy(), ref.numpy(), **tol)
        ch0 += co
    assert torch.isnan(got[:, ch0]).all()


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("shape,size", [((1, 3, 16, 32, 104), (32, 64, 208)),      # x2 up (the tiled LDS kernel when align)
                                        ((2, 4, 9, 21, 50), (5, 11, 25)),          # ~x0.5 down, odd sizes (scale_dimension's odd rule)
                                        ((1, 2, 8, 16, 200), (24, 48, 600)),       # x3 (Disp's factor), indices up to 600
                                        ((1, 2, 7, 5, 9), (7, 13, 9))])            # mixed: identity / up / identity
def test_trilinear_bit_identical_to_aten_cpu(ra, align, shape, size):
    """Round 4: lin_index and the interpolation blends reproduce ATen's CPU arithmetic bit for bit — the source index src = fl(scale
    * dst) rounded BEFORE its integer part and fraction are taken (align_corners) or fma(scale, dst + 0.5, -0.5) (not aligned), each
    blend fma(w0, a, fl(w1 * b)), x innermost, then y, then z (csrc/common.h).  The resample kernels therefore return the
    reference's own bits, not an approximation of them."""
    x = torch.randn(shape, generator=gen(21)) * 50.0
    ref = F.interpolate(x, size, mode="trilinear", align_corners=align)
    out = ra.ops.trilinear3d(gpu(x), size, align).cpu()
    same = int((out == ref).sum())
    assert same == ref.numel(), f"{ref.numel() - same} of {ref.numel()} voxels differ; max |diff| {float((out - ref).abs().max()):.3e}"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape,size", [((2, 5, 3, 4, 5), (6, 8, 10)), ((1, 8, 4, 8, 26), (8, 16, 52))])
def test_trilinear_act_into_slice(ra, shape, size, relu):
    """ragmi_trilinear3d_act_fwd: a channel SLICE of a wider tensor -> (ReLU of) its resample inside a wider output buffer."""
    wide = torch.randn((shape[0], shape[1] + 3) + shape[2:], generator=gen(18))
    x = wide[:, 2:2 + shape[1]]
    ref = F.interpolate(x, size, mode="trilinear", align_corners=True)
    ref = F.relu(ref) if relu else ref
    out = torch.full((shape[0], shape[1] + 4) + tuple(size), 7.0, device=DEV)
    ra.ops.trilinear3d_act(gpu(wide)[:, 2:2 + shape[1]], size, True, relu, out, 1)
    np.testing.assert_allclose(out[:, 1:1 + shape[1]].cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    assert float(out[:, 0].min()) == 7.0 and float(out[:, 1 + shape[1]:].min()) == 7.0          # neighbours untouched


def test_convbr_upsample_runs_conv_first(ra):
    """An up-sampling 1x1x1 ConvBR_3d (Cout <= Cin) mixes the channels on the small volume and interpolates afterwards
    (rag_amd.modules._ConvBR.forward): same function as the reference order conv(interpolate(x)) up to rounding."""
    torch.manual_seed(5)
    m = ra.ConvBR_3d(24, 8, 1, 1, 0).eval()
    with torch.no_grad():
        m.bn.running_mean.normal_(0, 0.2)
        m.bn.running_var.uniform_(0.5, 1.5)
        m.bn.weight.uniform_(0.5, 1.5)
        m.bn.bias.normal_(0, 0.2)
    x = torch.randn((2, 24, 4, 6, 13), generator=gen(19))
    size = (8, 12, 26)
    with torch.no_grad():
        ref = F.relu(m.bn(m.conv(F.interpolate(x, size, mode="trilinear", align_corners=True))))
        out = m.to(DEV)(gpu(x), resample_to=size)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("cin,cout,shape,size", [(12, 8, (2, 8, 12, 20), (4, 6, 10)), (24, 16, (1, 7, 9, 13), (4, 5, 7)),
                                                 (48, 8, (1, 3, 4, 5), (6, 8, 10)), (48, 24, (1, 4, 8, 26), (8, 16, 52)),
                                                 (12, 4, (1, 64, 32, 104), (32, 16, 52))])
def test_conv3d_k1_resample_vs_aten(ra, cin, cout, shape, size):
    """Fused trilinear(align_corners=True) + 1x1x1 ConvBR vs F.interpolate -> conv -> affine -> relu."""
    x = torch.randn((shape[0], cin) + shape[1:], generator=gen(40))
    w = torch.randn((cout, cin, 1, 1, 1), generator=gen(41)) * (2.0 / cin) ** 0.5
    scale, shift = torch.rand(cout, generator=gen(42)) + 0.5, torch.randn(cout, generator=gen(43)) * 0.1
    ref = F.relu(F.conv3d(F.interpolate(x, size, mode="trilinear", align_corners=True), w) * scale.view(1, -1, 1, 1, 1)
                 + shift.view(1, -1, 1, 1, 1))
    out = torch.zeros((shape[0], cout + 2) + tuple(size), device=DEV)
    ra.ops.conv3d_k1_resample(gpu(x), size, True, gpu(w.reshape(cout, cin)), gpu(scale), gpu(shift), True, out, 1)
    np.testing.assert_allclose(out[:, 1:1 + cout].cpu().numpy(), ref.numpy(), **TOL)
    assert float(out[:, :1].abs().max()) == 0.0 and float(out[:, 1 + cout:].abs().max()) == 0.0


@pytest.mark.parametrize("cins,cout,shapes,size", [((48, 24), 16, ((4, 8, 26), (8, 16, 52)), (4, 8, 26)),
                                                   ((24, 48), 16, ((7, 9, 13), (4, 5, 7)), (4, 5, 7)),
                                                   ((12, 12), 8, ((8, 12, 20), (8, 12, 20)), (4, 6, 10)),
                                                   ((50, 20), 8, ((3, 4, 5), (3, 4, 5)), (3, 4, 5))])
def test_conv3d_k1_resample_pair_vs_aten(ra, cins, cout, shapes, size):
    """The paired launch (a cell's pre_preprocess + preprocess): each input resampled or ALREADY at the output size (one load per
    channel instead of eight taps), written into adjacent channel slices of one buffer."""
    B = 2
    outs, specs = [], []
    out = torch.zeros((B, 2 * cout + 1) + tuple(size), device=DEV)
    for k, (cin, shp) in enumerate(zip(cins, shapes)):
        x = torch.randn((B, cin) + shp, generator=gen(44 + k))
        w = torch.randn((cout, cin, 1, 1, 1), generator=gen(46 + k)) * (2.0 / cin) ** 0.5
        scale, shift = torch.rand(cout, generator=gen(48 + k)) + 0.5, torch.randn(cout, generator=gen(50 + k)) * 0.1
        xi = x if tuple(shp) == tuple(size) else F.interpolate(x, size, mode="trilinear", align_corners=True)
        outs.append(F.relu(F.conv3d(xi, w) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)))
        specs.append((gpu(x), gpu(w.reshape(cout, cin)), gpu(scale), gpu(shift), True, k * cout))
    ra.ops.conv3d_k1_resample_pair(specs, size, out)
    np.testing.assert_allclose(out[:, :cout].cpu().numpy(), outs[0].numpy(), **TOL)
    np.testing.assert_allclose(out[:, cout:2 * cout].cpu().numpy(), outs[1].numpy(), **TOL)
    assert float(out[:, 2 * cout:].abs().max()) == 0.0


def test_conv3d_k1_transposed_weight(ra):
    """ragmi_conv3d_k1_fwd_ex with the weight transposed in memory ([Cin, Cout]) == the plain call on its transposed copy: the
    1x1x1 data gradient reads the forward weight in place."""
    x = torch.randn((2, 24, 3, 5, 7), generator=gen(60))
    w = torch.randn((10, 24), generator=gen(61)) * 0.2            # conv 24 -> 10
    ref = torch.empty((2, 10, 3, 5, 7), device=DEV)
    ra.ops.conv3d_k1(gpu(x), gpu(w), None, None, False, ref)
    out = torch.zeros((2, 12, 3, 5, 7), device=DEV)
    ra.ops.conv3d_k1(gpu(x), gpu(w.t().contiguous()), None, None, False, out, 1, transposed=True)
    np.testing.assert_array_equal(out[:, 1:11].cpu().numpy(), ref.cpu().numpy())
    assert float(out[:, 0].abs().max()) == 0.0 and float(out[:, 11].abs().max()) == 0.0


@pytest.mark.parametrize("cin,cout,H,W,stride", [(6, 12, 36, 60, 3), (3, 5, 17, 23, 2), (6, 12, 48, 96, 3), (4, 4, 9, 9, 4)])
def test_conv2d_k3_strided_vs_aten(ra, cin, cout, H, W, stride):
    """Feature-Net stem2d1 (3x3, pad 1, stride 3; rag_model.py:201)."""
    x = torch.randn((2, cin, H, W), generator=gen(90))
    w = torch.randn((cout, cin, 3, 3), generator=gen(91)) * 0.2
    scale, shift = torch.rand(cout, generator=gen(92)) + 0.5, torch.randn(cout, generator=gen(93)) * 0.1
    ref = F.relu(F.conv2d(x, w, stride=stride, padding=1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    out = ra.ops.conv2d_k3_strided(gpu(x), gpu(w), gpu(scale), gpu(shift), True, stride)
    assert out.shape == ref.shape
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), **TOL)


def test_convbr2d_and_cell2d_on_depth1_volumes(ra):
    """2-D ConvBR / Cell on the 3-D kernels (depth-1 volume) vs PyTorch's 2-D ops with the same parameters."""
    torch.manual_seed(7)
    m = ra.ConvBR_2d(3, 6, 3, 1, 1).to(DEV).eval()
    with torch.no_grad():
        m.bn.running_mean.normal_(0, 0.1); m.bn.running_var.uniform_(0.5, 1.5); m.bn.weight.uniform_(0.5, 1.5); m.bn.bias.normal_(0, 0.1)
        x = torch.randn((2, 3, 24, 36), device=DEV)
        ref = F.relu(F.batch_norm(F.conv2d(x, m.conv.weight, padding=1), m.bn.running_mean, m.bn.running_var, m.bn.weight, m.bn.bias))
        np.testing.assert_allclose(m(x).cpu().numpy(), ref.cpu().numpy(), **TOL)
        rows = np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]])
        cell = ra.Cell_2d(3, 3, 4, 4, ra.Genotype(rows, None, rows, None), 8, -1).to(DEV).eval()
        s0, s1 = torch.randn((1, 12, 24, 36), device=DEV), torch.randn((1, 12, 24, 36), device=DEV)
        prev, cat = cell(s0, s1)
        assert prev is s1 and tuple(cat.shape) == (1, 24, 12, 18)
        # reference semantics with torch ops on the same parameters
        def cbr(mod, z, k):
            y = F.conv2d(z, mod.conv.weight, padding=(k - 1) // 2)
            y = F.batch_norm(y, mod.bn.running_mean, mod.bn.running_var, mod.bn.weight, mod.bn.bias)
            return F.relu(y)
        t1 = F.interpolate(s1, (12, 18), mode="bilinear", align_corners=True)
        t0 = F.interpolate(s0, (12, 18), mode="bilinear", align_corners=True)
        st = [cbr(cell.pre_preprocess, t0, 1), cbr(cell.preprocess, t1, 1)]
        contribs = cell._contributions()
        for k in sorted(contribs):
            st.append(sum(cbr(op, st[j], 3) if isinstance(op, ra.ConvBR_2d) else st[j] for (j, op) in contribs[k]))
        np.testing.assert_allclose(cat.cpu().numpy(), torch.cat(st[-3:], 1).cpu().numpy(), **TOL)


def test_add(ra):
    a, b = torch.randn((2, 6, 3, 5, 7), generator=gen(18)), torch.randn((2, 9, 3, 5, 7), generator=gen(19))
    out = torch.zeros((2, 8, 3, 5, 7), device=DEV)
    ra.ops.add(gpu(a), 1, gpu(b), 4, out, 2, 4)
    assert torch.equal(out[:, 2:6].cpu(), a[:, 1:5] + b[:, 4:8])


# --------------------------------------------------------------------------- Cell_3d
@pytest.mark.parametrize("name", ["same_conv", "same_unsorted", "same_deep", "down_even", "down_odd", "up", "skip"])
def test_cell3d_golden(ra, name):
    g = load_golden("g4_cell3d")
    pp, p, fm, du = [int(v) for v in g[f"{name}::cfg"]]
    rows = g[f"{name}::rows"]
    cell = ra.Cell_3d(3, 3, pp, p, ra.Genotype(rows, None, rows, None), fm, du)
    cell.load_state_dict(split_sd(g, f"{name}::sd::"))
    cell = cell.to(DEV).eval()
    s1 = gpu(g[f"{name}::s1"])
    with torch.no_grad():
        prev, cat = cell(gpu(g[f"{name}::s0"]), s1)
    assert prev is s1
    np.testing.assert_allclose(cat.cpu().numpy(), g[f"{name}::out"], **TOL)


@pytest.mark.parametrize("rows", [O.ALL_CONV, np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]]), O.ALL_SKIP],
                         ids=["conv", "mixed", "skip"])
def test_cell3d_block_multiplier_below_steps(ra, rows):
    """block_multiplier 2 < steps 3: state 2 lives in a scratch buffer, only states 3 and 4 are concatenated, and a launch whose
    destinations span both buffers splits.  Against the torch composition over _contributions() on the same parameters (CPU, fp64)."""
    torch.manual_seed(17)
    cell = ra.Cell_3d(3, 2, 4, 4, ra.Genotype(rows, None, rows, None), 4, 0).eval()
    with torch.no_grad():
        for m in cell.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1)
        x0, x1 = torch.randn((1, 8, 4, 12, 20)), torch.randn((1, 8, 4, 12, 20))

        def cbr(mod, z, k):
            w, bn = mod.conv.weight.double(), mod.bn
            y = F.batch_norm(F.conv3d(z, w, padding=(k - 1) // 2), bn.running_mean.double(), bn.running_var.double(), bn.weight.double(),
                             bn.bias.double(), eps=bn.eps)
            return F.relu(y)
        st = [cbr(cell.pre_preprocess, x0.double(), 1), cbr(cell.preprocess, x1.double(), 1)]
        contribs = cell._contributions()
        for k in sorted(contribs):
            st.append(sum(cbr(op, st[j], 3) if isinstance(op, ra.ConvBR_3d) else st[j] for (j, op) in contribs[k]))
        want = torch.cat(st[-2:], 1)
        cell = cell.to(DEV)
        s1 = gpu(x1)
        prev, cat = cell(gpu(x0), s1)
    assert prev is s1 and tuple(cat.shape) == (1, 8, 4, 12, 20)
    np.testing.assert_allclose(cat.cpu().numpy(), want.numpy(), **TOL)


# --------------------------------------------------------------------------- MatchingNet end to end
def _net_from_golden(ra, g, maxdisp):
    rows = g["rows"]
    net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=maxdisp)
    sd = {k: v for k, v in split_sd(g).items()
          if k.split(".")[0] in ("stem3d0", "stem3d1", "cells_3d", "last_3_3d", "last_6_3d", "last_12_3d")}
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval()


# `mat` against the reference's: absolute tolerance as a fraction of the tensor's largest magnitude (|mat| reaches 1e4-1e5 with seeded
# random weights, fp32 cancellation).  Strict fp32 (RAGMI_F32): the reassociation class.  f16x3 (RAGMI_F32X3, the default): each
# of the ~20 convolutions adds <= 3 * 2^-16 of its sum |w x| (include/rag_amd.h) — the deep levels of these small goldens run the
# box-tile f16x3 form.  The gate that matters, EPE <= 1e-3 px, is the same for both.
MAT_ATOL = {"fp32": 2e-6, "f16x3": 1.5e-5}      # (f16x3: loosened to the measurement in round 4 — 7.5x the strict path's; may not grow)


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["conv_48x96_d48", "unsorted_36x60_d24", "skip_48x72_d24"])
def test_matchingnet_golden(ra, name, prec):
    g = load_golden("g5_forward_" + name)
    net = _net_from_golden(ra, g, int(g["maxdisp"]))
    with torch.no_grad(), ra.ops.conv_precision(prec):
        lf, rf = gpu(g["left_fea"]), gpu(g["right_fea"])
        cost = net.cost_volume(lf, rf)
        mat = net.matching(cost, net.arch_init)
        disp = net(lf, rf)
    mat_err = float(np.abs(mat.cpu().numpy() - g["mat"]).max()) / float(np.abs(g["mat"]).max())
    print(f"matchingnet golden {name} [{prec}]: max |mat err| / max |mat| = {mat_err:.2e}; EPE {O.epe(disp.cpu(), torch.from_numpy(g['disp'])):.2e}; "
          f"max |disp err| {float((disp.cpu() - torch.from_numpy(g['disp'])).abs().max()):.3f} px")
    np.testing.assert_allclose(mat.cpu().numpy(), g["mat"], rtol=1e-3, atol=MAT_ATOL[prec] * float(np.abs(g["mat"]).max()))
    epe = O.epe(disp.cpu(), torch.from_numpy(g["disp"]))
    assert epe <= EPE_GATE, epe
    # random weights drive |cost| to 1e4-1e5, so softmin is almost an argmin: a few near-tie pixels may move by a fraction of a
    # pixel — or by whole pixels — under ANY legal fp32 reassociation (round 3: a resample summation order moved one pixel of
    # conv_48x96_d48 by 0.165 px at EPE 2.6e-5).  The gate is EPE; the per-pixel check is two quantile bounds, no cap on the
    # single largest move (that was a test of luck, not of parity): < 0.5 % of the pixels off by more than 2e-3 px, < 0.05 %
    # by more than 0.05 px.
    err = (disp.cpu() - torch.from_numpy(g["disp"])).abs()
    share_small, share_large = float((err > 2e-3).float().mean()), float((err > 5e-2).float().mean())
    assert share_small < 5e-3 and share_large < 5e-4, (share_small, share_large, float(err.max()))


def test_matchingnet_plumbing_config_golden(ra):
    """BASELINE configs[0] (256x512 padded to 264x516, D=48) against the reference-generated fixture."""
    g = load_golden("g7_plumbing_264x516_d48")
    net = _net_from_golden(ra, g, int(g["maxdisp"]))
    with torch.no_grad():
        disp = net(gpu(g["left_fea"]), gpu(g["right_fea"])).cpu()
    y0, y1, x0, x1 = [int(v) for v in g["crop_box"]]
    assert O.epe(disp[:, y0:y1, x0:x1], torch.from_numpy(g["disp_crop"])) <= EPE_GATE
    np.testing.assert_allclose(disp.double().mean(dim=2).numpy()[0], g["disp_row_means"], rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("name", ["conv_48x96_d48", "unsorted_36x60_d24"])
def test_network_forward_from_images_golden(ra, name):
    """Full reference-layout Network from images vs the reference output: Feature Net and Matching
    Net both on the HIP kernels."""
    g = load_golden("g5_forward_" + name)
    rows = g["rows"]
    net = ra.Network(ra.Genotype(rows, None, rows, None), DEV, maxdisp=int(g["maxdisp"]))
    net.load_state_dict(split_sd(g), strict=True)
    net = net.to(DEV).eval()
    with torch.no_grad():
        disp = net(gpu(g["left"]), gpu(g["right"]), 0, net.arch_init)
        fea = net.feature(gpu(g["left"]), net.arch_init, None)
        sel = [0] * 18
        disp_search = net.search_forward(gpu(g["left"]), gpu(g["right"]), 0, sel)
    np.testing.assert_allclose(fea.cpu().numpy(), g["left_fea"], rtol=2e-4, atol=2e-4)
    ref = torch.from_numpy(g["disp"])
    assert O.epe(disp.cpu(), ref) <= EPE_GATE, O.epe(disp.cpu(), ref)
    assert torch.equal(disp, disp_search)      # search_forward with all-zero unit choices == forward(arch_init)


def test_matchingnet_batch_shard_equivalence(ra):
    """Multi-GPU sharding is a batch split with no collective: a B=3 forward equals three B=1 forwards bitwise."""
    rows = O.ALL_CONV
    net = ra.MatchingNet(ra.ALL_CONV_GENOTYPE, maxdisp=48)
    net.load_state_dict(O.random_matching_state_dict(rows, seed=3))
    net = net.to(DEV).eval()
    lf, rf = torch.randn((3, 12, 16, 28), device=DEV), torch.randn((3, 12, 16, 28), device=DEV)
    with torch.no_grad():
        full = net(lf, rf)
        parts = torch.cat([net(lf[i:i + 1], rf[i:i + 1]) for i in range(3)])
    assert torch.equal(full, parts)


def test_matchingnet_headline_config_epe(ra):
    """BASELINE config 2: B=1, 384x1248, D=192, fp32, all-conv genotype, seeded weights with randomised BN
    (SURVEY §8(d)).  The CPU oracle takes ~10-15 s here.  Gate: EPE <= 1e-3 px."""
    rows = O.ALL_CONV
    sd = O.random_matching_state_dict(rows, seed=0)
    g = gen(1234)
    lf, rf = torch.randn((1, 12, 128, 416), generator=g), torch.randn((1, 12, 128, 416), generator=g)
    torch.set_num_threads(min(32, torch.get_num_threads() if torch.get_num_threads() > 8 else 16))
    ref = O.matching_net_forward(lf, rf, sd, rows, 192)
    net = ra.MatchingNet(ra.ALL_CONV_GENOTYPE, maxdisp=192)
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    with torch.no_grad():
        out = net(gpu(lf), gpu(rf)).cpu()
    epe = O.epe(out, ref)
    print(f"headline EPE vs CPU oracle: {epe:.3e} px; max abs {float((out - ref).abs().max()):.3e}")
    assert epe <= EPE_GATE, epe


MIXED_UNSORTED = np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]])     # SURVEY 8 A6's probe rows


def test_x3_margin_over_seeds_and_genotypes_at_headline_size(ra):
    """The f16x3 margin as a spread, not a point: B=1, 384x1248, D=192 under the default precision (RAGMI_F32X3) over weight
    seeds {0, 1, 2} x genotypes {all-conv, all-skip, mixed unsorted rows}, plus the src_self eval shape 576x1248
    (src_self/dataloaders/stereo_dataset.py:111-112, the provenance of BASELINE's 1248).  Every case must sit inside HALF the
    EPE budget (5e-4 px) against the CPU oracle; the table is printed."""
    torch.set_num_threads(min(32, torch.get_num_threads() if torch.get_num_threads() > 8 else 16))
    cases = [(name, rows, seed, (128, 416)) for name, rows in (("all-conv", O.ALL_CONV), ("all-skip", O.ALL_SKIP), ("mixed", MIXED_UNSORTED))
             for seed in (0, 1, 2)]
    cases.append(("all-conv", O.ALL_CONV, 0, (192, 416)))                      # 576 x 1248
    table = []
    for name, rows, seed, (h, w) in cases:
        sd = O.random_matching_state_dict(rows, seed=seed)
        g = gen(1234 + seed)
        lf, rf = torch.randn((1, 12, h, w), generator=g), torch.randn((1, 12, h, w), generator=g)
        ref = O.matching_net_forward(lf, rf, sd, rows, 192)
        net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=192)
        net.load_state_dict(sd, strict=True)
        net = net.to(DEV).eval()
        outs = {}
        for prec in ("f16x3", "fp32"):
            with torch.no_grad(), ra.ops.conv_precision(prec):
                outs[prec] = net(gpu(lf), gpu(rf)).cpu()
        del net
        table.append((name, seed, 3 * h, 3 * w, O.epe(outs["f16x3"], ref), float((outs["f16x3"] - ref).abs().max()),
                      O.epe(outs["fp32"], ref), O.epe(outs["f16x3"], outs["fp32"])))
    print("EPE vs the CPU oracle at D=192, split-operand form (RAGMI_F32X3, gate here 5e-4 px, budget 1e-3) | strict fp32 (RAGMI_F32):")
    for name, seed, H_, W_, epe, worst, epe32, epe_x32 in table:
        print(f"  {name:9s} seed {seed}  {H_}x{W_}: x3 EPE {epe:.3e} px (max |err| {worst:.3e}) | fp32 EPE {epe32:.3e} | x3 vs fp32 on the GPU {epe_x32:.3e}")
    for name, seed, H_, W_, epe, worst, epe32, epe_x32 in table:
        assert epe32 <= 1e-3, ("fp32", name, seed, H_, W_, epe32)
        assert epe <= 5e-4, ("x3", name, seed, H_, W_, epe)


# --------------------------------------------------------------------------- bf16 storage / fp32 accumulate (BASELINE config 3)
BF = torch.bfloat16
BF_TOL = dict(rtol=1.6e-2, atol=1.6e-2)   # a couple of bf16 ulps (2^-8 relative) on O(1) data


def bf(x):
    return x.to(BF)


def test_bf16_costvol_bit_exact(ra):
    L, R = bf(torch.randn((2, 12, 9, 33), generator=gen(70))), bf(torch.randn((2, 12, 9, 33), generator=gen(71)))
    out = ra.ops.costvol(L.to(DEV), R.to(DEV), 27)
    assert out.dtype == BF and torch.equal(out.cpu(), O.cost_volume(L, R, 27))
    L, R = bf(torch.randn((1, 12, 128, 416), generator=gen(72))), bf(torch.randn((1, 12, 128, 416), generator=gen(73)))
    assert torch.equal(ra.ops.costvol(L.to(DEV), R.to(DEV), 192).cpu(), O.cost_volume(L, R, 192))


@pytest.mark.parametrize("cin,cout,shape", [(4, 12, (2, 5, 9, 33)), (24, 12, (1, 6, 10, 40)), (16, 48, (1, 4, 8, 26)), (4, 4, (1, 64, 20, 96))])
def test_bf16_conv3d_k3(ra, cin, cout, shape):
    """bf16 in/out, fp32 math: reference = fp32 conv on the SAME bf16-rounded inputs, rounded once at the end."""
    B, D, H, W = shape
    x = bf(torch.randn((B, cin, D, H, W), generator=gen(74)))
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen(75)) * (2.0 / (27 * cin)) ** 0.5
    scale, shift = torch.rand(cout, generator=gen(76)) + 0.5, torch.randn(cout, generator=gen(77)) * 0.1
    res = bf(torch.randn((B, cout, D, H, W), generator=gen(78)))
    ref = F.relu(F.conv3d(x.float(), w, padding=1) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)) + res.float()
    out = torch.zeros((B, cout, D, H, W), device=DEV, dtype=BF)
    ra.ops.conv3d_k3(x.to(DEV), ra.ops.conv3d_k3_pack(gpu(w)), cout, gpu(scale), gpu(shift), True, out, None, res.to(DEV))
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), **BF_TOL)
    assert float((out.float().cpu() - bf(ref).float()).abs().max()) <= 2 * 2.0 ** -8 * float(ref.abs().max())   # <= ~1 ulp of the largest value


def test_bf16_pointwise_resample_add_disp(ra):
    x = bf(torch.randn((2, 12, 8, 12, 20), generator=gen(79)))
    w = torch.randn((8, 12, 1, 1, 1), generator=gen(80)) * 0.4
    scale, shift = torch.rand(8, generator=gen(81)) + 0.5, torch.randn(8, generator=gen(82)) * 0.1
    v = lambda t_: t_.view(1, -1, 1, 1, 1)  # noqa: E731
    out = torch.zeros((2, 8, 8, 12, 20), device=DEV, dtype=BF)
    ra.ops.conv3d_k1(x.to(DEV), gpu(w.reshape(8, 12)), gpu(scale), gpu(shift), True, out)
    np.testing.assert_allclose(out.float().cpu().numpy(), F.relu(F.conv3d(x.float(), w) * v(scale) + v(shift)).numpy(), **BF_TOL)
    size = (4, 6, 10)
    out2 = torch.zeros((2, 8) + size, device=DEV, dtype=BF)
    ra.ops.conv3d_k1_resample(x.to(DEV), size, True, gpu(w.reshape(8, 12)), gpu(scale), gpu(shift), True, out2)
    ref2 = F.relu(F.conv3d(F.interpolate(x.float(), size, mode="trilinear", align_corners=True), w) * v(scale) + v(shift))
    np.testing.assert_allclose(out2.float().cpu().numpy(), ref2.numpy(), **BF_TOL)
    up = ra.ops.trilinear3d(x.to(DEV), (16, 24, 40), True)
    np.testing.assert_allclose(up.float().cpu().numpy(), F.interpolate(x.float(), (16, 24, 40), mode="trilinear", align_corners=True).numpy(), **BF_TOL)
    a_, b_ = bf(torch.randn((2, 6, 3, 5, 8), generator=gen(83))), bf(torch.randn((2, 9, 3, 5, 8), generator=gen(84)))
    o = torch.zeros((2, 8, 3, 5, 8), device=DEV, dtype=BF)
    ra.ops.add(a_.to(DEV), 1, b_.to(DEV), 4, o, 2, 4)
    assert torch.equal(o[:, 2:6].cpu(), bf(a_[:, 1:5].float() + b_[:, 4:8].float()))
    c = bf(torch.randn((2, 1, 16, 6, 10), generator=gen(85)) * 2)
    d_ = ra.ops.disp_softargmin(c.to(DEV), 48)
    assert d_.dtype == torch.float32
    np.testing.assert_allclose(d_.cpu().numpy(), O.disp_head(c.float(), 48).numpy(), rtol=2e-4, atol=2e-3)


def test_bf16_matchingnet_epe_report(ra):
    """Config-3 style run at a reduced size: bf16 activations vs the fp32 build and vs the CPU oracle.  With seeded random
    weights |cost| ~ 1e4-1e5 and softmin is nearly an argmin, so bf16 rounding (2^-8) flips near-ties: the tolerance is
    STATED FROM MEASUREMENT — see DESIGN.md; the assertion is a sanity bound."""
    rows = O.ALL_CONV
    sd = O.random_matching_state_dict(rows, seed=4)
    net = ra.MatchingNet(ra.ALL_CONV_GENOTYPE, maxdisp=96)
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    g = gen(86)
    lf, rf = torch.randn((2, 12, 32, 64), generator=g), torch.randn((2, 12, 32, 64), generator=g)
    with torch.no_grad():
        d32 = net(gpu(lf), gpu(rf)).cpu()
        d16 = net(gpu(lf).to(BF), gpu(rf).to(BF)).cpu()
    ref = O.matching_net_forward(lf, rf, sd, rows, 96)
    e32, e16, e16_32 = O.epe(d32, ref), O.epe(d16, ref), O.epe(d16, d32)
    print(f"EPE fp32 vs oracle {e32:.3e}; bf16 vs oracle {e16:.3e}; bf16 vs fp32 build {e16_32:.3e} px (maxdisp 96)")
    # bf16 storage at this reduced size: 0.219 / 0.221 px with every tensor bf16 (rounds 2-4); 0.039 px with the mixed storage of round 5
    # (full-resolution tensors bf16, deep levels and head fp32).  The stated tolerance of the bf16 configuration is enforced on the
    # full workload below (BF16_FULL_GATE).
    assert d16.dtype == torch.float32 and torch.isfinite(d16).all() and e32 <= EPE_GATE and e16 < 0.08


BF16_FULL_GATE = 0.05     # px — SURVEY's gate for configs[2].  Round 5 (mixed storage: bf16 for the full-resolution tensors, fp32 from the first
                          # cell below the cost volume's resolution on — ops.set_bf16_deep_fp32): measured 0.0249 px at the full configs[2]
                          # workload.  Rounds 2-4 stored every tensor bf16: 0.0993 / 0.0973 px under a gate of 0.12 (still checked below as
                          # BF16_ALL_GATE, which may not grow).  Where the error comes from: tests/analysis_bf16_stage_epe.py.
BF16_ALL_GATE = 0.12


def test_bf16_config3_full_workload_gate(ra):
    """BASELINE configs[2] at its full size: B=8, 384x1248, D=192, bf16 activation storage (fp32 accumulate, fp32 `mat`).
    Pair 0 against the fp32 CPU oracle with a STATED tolerance; pairs 0..7 against the same pairs computed alone (the batch split
    that the multi-GPU path relies on), bitwise.  The fp32 build on the same inputs must stay inside the fp32 gate."""
    rows = O.ALL_CONV
    sd = O.random_matching_state_dict(rows, seed=0)
    g = gen(1234)
    lf, rf = torch.randn((8, 12, 128, 416), generator=g), torch.randn((8, 12, 128, 416), generator=g)
    net = ra.MatchingNet(ra.ALL_CONV_GENOTYPE, maxdisp=192)
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    with torch.no_grad():
        d16 = net(gpu(lf).to(BF), gpu(rf).to(BF))
        for i in range(8):
            alone = net(gpu(lf[i:i + 1]).to(BF), gpu(rf[i:i + 1]).to(BF))
            assert torch.equal(alone, d16[i:i + 1]), i
        d32 = net(gpu(lf[:1]), gpu(rf[:1])).cpu()
    torch.set_num_threads(16)
    ref = O.matching_net_forward(lf[:1], rf[:1], sd, rows, 192)
    e32, e16, e16_32 = O.epe(d32, ref), O.epe(d16[:1].cpu(), ref), O.epe(d16[:1].cpu(), d32)
    print(f"configs[2] full size: EPE fp32 vs oracle {e32:.3e}; bf16 vs oracle {e16:.3e}; bf16 vs fp32 build {e16_32:.3e} px")
    assert d16.dtype == torch.float32 and torch.isfinite(d16).all()
    assert e32 <= EPE_GATE, e32
    assert e16 <= BF16_FULL_GATE, e16
    # every stored tensor bf16 (rounds 2-4; ops.set_bf16_deep_fp32(False)): the old form keeps its old gate
    ra.ops.set_bf16_deep_fp32(False)
    try:
        with torch.no_grad():
            dall = net(gpu(lf[:1]).to(BF), gpu(rf[:1]).to(BF)).cpu()
    finally:
        ra.ops.set_bf16_deep_fp32(True)
    eall = O.epe(dall, ref)
    print(f"configs[2] full size, every stored tensor bf16: EPE vs oracle {eall:.3e} px")
    assert e16 < eall <= BF16_ALL_GATE, (e16, eall)


def test_bf16_storage_epe_at_two_cost_scales(ra):
    """VERDICT r03 8(c), measured in round 4 — and the hypothesis it was meant to confirm is REFUTED.  Round 3 explained configs[2]'s
    0.09-0.10 px (bf16 activation storage vs the fp32 build, seeded random weights, |cost| ~ 1e4) by the conditioning of a nearly-argmin
    softmin.  The same network with last_3_3d's weight scaled by 1e-3 (|cost| ~ 10-100, the scale of a trained net's matching cost;
    `mat` scales by exactly that factor, nothing else changes) does NOT show the error collapse: the EPE GROWS (0.075 -> 0.29 px).
    What bf16 storage carries is a RELATIVE error of `mat` of ~3e-3 of its largest magnitude (8 significant bits per stored stage,
    ~20 stages); on a peaked softmin most pixels do not move at all and a few move far, on a smooth one every pixel's expectation
    shifts a little — the second costs more EPE.  So configs[2] is a throughput / accuracy trade, not an fp32-class result: its gate is
    stated from BOTH regimes (<= 0.12 px at the benchmark's own weights, <= 0.5 px at the trained-net cost scale) together with the
    relative error of `mat` that explains them."""
    rows = O.ALL_CONV
    g = gen(1234)
    lf, rf = torch.randn((1, 12, 128, 416), generator=g), torch.randn((1, 12, 128, 416), generator=g)
    out = {}
    for f in (1.0, 1e-3):
        sd = O.random_matching_state_dict(rows, seed=0)
        sd["last_3_3d.0.conv.weight"] = sd["last_3_3d.0.conv.weight"] * f
        net = ra.MatchingNet(ra.ALL_CONV_GENOTYPE, maxdisp=192)
        net.load_state_dict(sd)
        net = net.to(DEV).eval()
        with torch.no_grad():
            feats = (gpu(lf), gpu(rf))
            m32 = net.matching(None, net.arch_init, None, features=feats)
            m16 = net.matching(None, net.arch_init, None, features=(feats[0].to(BF), feats[1].to(BF)))
            d32, d16 = net.disp(m32).cpu(), net.disp(m16).cpu()
        rel = float((m16.float() - m32).abs().max() / m32.abs().max())
        out[f] = (float(m32.abs().max()), O.epe(d16, d32), float((d16 - d32).abs().max()), rel)
        print(f"last_3_3d weight x {f:g}: max |cost| {out[f][0]:.3g}; bf16 storage vs fp32 build: max |mat err| / max |mat| {rel:.2e}, "
              f"EPE {out[f][1]:.3e} px (max {out[f][2]:.3f} px)")
    assert out[1.0][0] > 1e3 and out[1e-3][0] < 1e3                    # the two regimes
    # the stated gates of configs[2] (<= 0.05 px at the benchmark's weights, <= 0.1 px at the trained-net cost scale).
    # Round 5, mixed storage: measured 0.0252 / 0.0730 px, relative error of `mat` 4.2e-3 (rounds 2-4, every tensor bf16: 0.075-0.097 /
    # 0.29 px, 1.1e-2)
    assert out[1.0][1] <= BF16_FULL_GATE and out[1e-3][1] <= 0.1
    assert max(out[1.0][3], out[1e-3][3]) <= 8e-3                       # the relative error of `mat` under bf16 storage


# --------------------------------------------------------------------------- grown model: checkpoint round trip + serving (N4)
def test_multitask_serving_after_checkpoint_round_trip(ra, tmp_path):
    from rag_amd import checkpoint as ck
    mixed = np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]])
    torch.manual_seed(5)
    net = ra.Network(ra.ALL_CONV_GENOTYPE, DEV, maxdisp=48).to(DEV)
    archis = [net.arch_init]
    net.expand(1, ra.Genotype(mixed, None, mixed, None), DEV)
    for k in (1, 5, 9, 12, 15):
        net.p[k][-1] = 0.9
    archis.append(net.select(1))
    net = net.eval()
    path = tmp_path / "checkpoint_task1.ckpt"
    ck.save_checkpoint(path, net, archis, task=1)
    net2, archis2 = ck.load_checkpoint(str(path), device=DEV)
    serve = ck.MultiTaskStereo(net2, archis2)
    left, right = gpu(torch.randn((1, 3, 48, 96), generator=gen(81))), gpu(torch.randn((1, 3, 48, 96), generator=gen(82)))
    with torch.no_grad():
        outs = [net(left, right, t, archis[t]) for t in (0, 1)]
        served = [serve(left, right, t) for t in (0, 1)]
    assert torch.equal(outs[0], served[0]) and torch.equal(outs[1], served[1])
    assert not torch.equal(outs[0], outs[1])           # the two tasks really run different units


def test_grown_model_against_reference_outputs(ra, tmp_path):
    """g10: the REFERENCE's numbers for a grown model (expand -> forced winners -> select, rag_model.py:391-522, 709-845) with
    unit indices != 0 and task heads t != 0.  (1) search_forward on the expanded supermodel with mixed unit choices
    (rag_model.py:663-706); (2) the selected model saved as a run.py:194-196 checkpoint, reloaded through
    checkpoint.load_checkpoint (ModuleLists rebuilt from key names) and served per task by MultiTaskStereo.  EPE <= 1e-3 px."""
    import json
    from rag_amd import checkpoint as ck
    g = load_golden("g10_grown_model")
    blob = json.loads(bytes(g["blob"]).decode())
    maxdisp = int(g["maxdisp"])
    geno0 = ra.Genotype(g["rows_unit0"], None, g["rows_unit0"], None)
    geno1 = ra.Genotype(g["rows_unit1"], None, g["rows_unit1"], None)
    left, right = gpu(g["left"]), gpu(g["right"])
    # (1) the expanded supermodel
    net = ra.Network(geno0, DEV, maxdisp=maxdisp)
    net.expand(1, geno1, "cpu")
    net.load_state_dict(split_sd(g, "search::"), strict=True)
    net = net.to(DEV).eval()
    with torch.no_grad():
        for tag, sel, t in (("a", g["sel_a"], 1), ("b", g["sel_b"], 1), ("c", g["sel_a"], 0)):
            sel = [int(v) for v in sel]
            fea = net.search_feature(left, sel)
            np.testing.assert_allclose(fea.cpu().numpy(), g[f"search_left_fea_{tag}"], rtol=2e-4, atol=2e-4)
            disp = net.search_forward(left, right, t, sel)
            e = O.epe(disp.cpu(), torch.from_numpy(g[f"search_disp_{tag}"]))
            assert e <= EPE_GATE, (tag, e)
    # (2) checkpoint of the selected model -> reload -> serve both tasks
    sel_sd = split_sd(g, "selected::")
    genotypes = {}
    for name, n in blob["length"].items():
        if name.startswith("cell_"):
            genotypes[name] = [{"normal": g["rows_unit0"].tolist(), "reduce": g["rows_unit0"].tolist()}] + \
                              [{"normal": g["rows_unit1"].tolist(), "reduce": g["rows_unit1"].tolist()}] * (n - 1)
    path = tmp_path / "checkpoint_task1.ckpt"
    torch.save({"task": 1, "model": sel_sd, "optimizer": None, "archis": [blob["arch_t0"], blob["arch_t1"]],
                "genotypes": genotypes, "maxdisp": maxdisp}, path)
    net2, archis = ck.load_checkpoint(str(path), device=DEV)
    serve = ck.MultiTaskStereo(net2, archis)
    with torch.no_grad():
        for t in (0, 1):
            disp = serve(left, right, t)
            e = O.epe(disp.cpu(), torch.from_numpy(g[f"disp_t{t}"]))
            assert e <= EPE_GATE, (t, e)
            fea = net2.feature(left, archis[t], None)
            np.testing.assert_allclose(fea.cpu().numpy(), g[f"left_fea_t{t}"], rtol=2e-4, atol=2e-4)
    # a reference checkpoint (no genotypes / archis inside) loads when the caller supplies them
    torch.save({"task": 1, "model": sel_sd, "optimizer": None, "maxdisp": maxdisp}, path)   # (the reference hard-codes 192)
    net3, archis3 = ck.load_checkpoint(str(path), device=DEV, genotypes=genotypes, archis=[blob["arch_t0"], blob["arch_t1"]])
    with torch.no_grad():
        assert torch.equal(ck.MultiTaskStereo(net3, archis3)(left, right, 1), serve(left, right, 1))


# --------------------------------------------------------------------------- BASELINE configs[3] shape (480x960, D=192)
def test_matchingnet_config4_shape_epe_and_shard_equivalence(ra):
    """DrivingStereo eval pad 480x960, D=192 (features 160x320, cost depth 64): EPE vs the CPU oracle
    on one pair, and a pair computed alone equals the same pair inside a batch (the multi-GPU split is a batch split)."""
    rows = O.ALL_CONV
    sd = O.random_matching_state_dict(rows, seed=9)
    net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=192)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    lf, rf = torch.randn((2, 12, 160, 320), generator=gen(91)), torch.randn((2, 12, 160, 320), generator=gen(92))
    with torch.no_grad():
        both = net(gpu(lf), gpu(rf))
        alone = net(gpu(lf[1:]), gpu(rf[1:]))
    assert torch.equal(both[1:], alone)
    torch.set_num_threads(16)
    ref = O.matching_net_forward(lf[:1], rf[:1], sd, rows, 192)
    assert O.epe(both[:1].cpu(), ref) <= EPE_GATE


# --------------------------------------------------------------------------- cost volume + stem3d0 without the cost volume
@pytest.mark.parametrize("B,C,cout,h,w,maxdisp,bn,relu", [
    (1, 12, 12, 8, 32, 24, True, True),        # D=8
    (2, 12, 12, 5, 9, 48, True, True),         # w < D: every column is inside the diagonal band
    (1, 12, 12, 6, 20, 3, True, True),         # D=1: one plane is both z borders
    (1, 12, 12, 6, 20, 6, True, False),        # D=2
    (2, 3, 5, 7, 13, 15, False, False),        # odd channel counts, no BN
    (1, 12, 12, 16, 70, 48, True, True),       # wider than one 64-column tile
    (1, 12, 12, 128, 416, 192, True, True),    # headline size
])
def test_costvol_stem_vs_oracle(ra, B, C, cout, h, w, maxdisp, bn, relu):
    L, R = torch.randn((B, C, h, w), generator=gen(101)), torch.randn((B, C, h, w), generator=gen(102))
    wt = torch.randn((cout, 2 * C, 3, 3, 3), generator=gen(103)) * 0.1
    sd = {"conv.weight": wt, "bn.weight": torch.rand(cout, generator=gen(104)) + 0.5, "bn.bias": torch.randn(cout, generator=gen(105)) * 0.1,
          "bn.running_mean": torch.randn(cout, generator=gen(106)) * 0.1, "bn.running_var": torch.rand(cout, generator=gen(107)) + 0.5}
    torch.set_num_threads(16)
    ref = O.conv_br_3d(O.cost_volume(L, R, maxdisp), sd, "", padding=1, bn=bn, relu=relu)
    scale = shift = None
    if bn:
        scale = sd["bn.weight"] * torch.rsqrt(sd["bn.running_var"] + 1e-5)
        shift = sd["bn.bias"] - sd["bn.running_mean"] * scale
    var = ra.ops.costvol_stem_prepare(gpu(wt))
    out = ra.ops.costvol_stem(gpu(L), gpu(R), maxdisp, var, cout, gpu(scale) if bn else None, gpu(shift) if bn else None, relu)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), **TOL)


def test_costvol_stem_tails_and_bf16(ra):
    B, C, h, w, maxdisp = 2, 12, 6, 40, 24
    L, R = torch.randn((B, C, h, w), generator=gen(111)), torch.randn((B, C, h, w), generator=gen(112))
    wt = torch.randn((12, 24, 3, 3, 3), generator=gen(113)) * 0.1
    w1, w2 = torch.randn((4, 12), generator=gen(114)) * 0.3, torch.randn((3, 12), generator=gen(115)) * 0.3
    s1, h1 = torch.rand(4, generator=gen(116)) + 0.5, torch.randn(4, generator=gen(117)) * 0.1
    ref = F.relu(F.conv3d(O.cost_volume(L, R, maxdisp), wt, padding=1))
    t1 = F.relu(torch.einsum("kc,bcdhw->bkdhw", w1, ref) * s1.view(1, -1, 1, 1, 1) + h1.view(1, -1, 1, 1, 1))
    t2 = torch.einsum("kc,bcdhw->bkdhw", w2, ref)
    var = ra.ops.costvol_stem_prepare(gpu(wt))
    pre = torch.zeros((B, 8, maxdisp // 3, h, w), device=DEV)
    tails = [ra.ops.Tail(gpu(w1), gpu(s1), gpu(h1), True, pre, 4), ra.ops.Tail(gpu(w2), None, None, False, pre, 0)]
    out = ra.ops.costvol_stem(gpu(L), gpu(R), maxdisp, var, 12, None, None, True, tails=tails)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), **TOL)
    np.testing.assert_allclose(pre[:, 4:8].cpu().numpy(), t1.numpy(), **TOL)
    np.testing.assert_allclose(pre[:, 0:3].cpu().numpy(), t2.numpy(), **TOL)
    # bf16 storage: features and output in bf16, planes and arithmetic in fp32
    Lb, Rb = L.to(torch.bfloat16), R.to(torch.bfloat16)
    refb = F.relu(F.conv3d(O.cost_volume(Lb.float(), Rb.float(), maxdisp), wt, padding=1))
    outb = ra.ops.costvol_stem(gpu(Lb), gpu(Rb), maxdisp, var, 12, None, None, True)
    assert outb.dtype == torch.bfloat16
    np.testing.assert_allclose(outb.float().cpu().numpy(), refb.numpy(), rtol=1e-2, atol=1e-2)


# --------------------------------------------------------------------------- f16x3 convolution (conv3d_x3.hip; ABI dtype RAGMI_F32X3)
@pytest.fixture
def x3_on(ra):
    old = ra.ops.set_conv_precision("f16x3")
    yield
    ra.ops.set_conv_precision(old)


@pytest.mark.parametrize("cin,cout,shape", [(12, 12, (1, 16, 128, 130)), (4, 12, (2, 9, 129, 257)), (24, 12, (1, 8, 140, 250)), (4, 8, (1, 9, 170, 175)),
                                            (8, 24, (1, 10, 24, 72)), (16, 48, (1, 8, 24, 96))])
def test_x3_conv_vs_oracle(ra, x3_on, cin, cout, shape):
    """fp32 accuracy from three bf16 MFMAs per product: same entry point, shapes big enough PER SAMPLE to take a f16x3 kernel (the
    z-marching form from 2^18 voxels, the deep form from 2^14 with 8 / 16 input channels; the batch size never enters the choice)."""
    B, D, H, W = shape
    x = torch.randn((B, cin, D, H, W), generator=gen(121))
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen(122)) * 0.1
    sc, sh = torch.rand(cout, generator=gen(123)) + 0.5, torch.randn(cout, generator=gen(124)) * 0.1
    assert ra.ops.conv3d_k3_uses_x3(cin, cout, B, D, H, W) and ra.ops.conv3d_k3_uses_x3(cin, cout, 7 * B, D, H, W)
    assert not ra.ops.conv3d_k3_uses_x3(cin, cout, 64, D // 4, H // 4, W)          # a big batch of small samples stays exact fp32
    out = torch.empty((B, cout, D, H, W), device=DEV)
    ra.ops.conv3d_k3(gpu(x), ra.ops.conv3d_k3_pack(gpu(w)), cout, gpu(sc), gpu(sh), True, out)
    torch.set_num_threads(16)
    ref = F.relu(F.conv3d(x, w, padding=1) * sc.view(1, -1, 1, 1, 1) + sh.view(1, -1, 1, 1, 1))
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("nset,cs,cout,shape", [
    (1, 12, 12, (2, 128, 416)),       # Feature Net stem1 at the headline shape (both images as one batch)
    (2, 8, 24, (2, 64, 208)),         # Cell_2d dual launch at half resolution: two output blocks
    (2, 4, 12, (2, 128, 416)),        # Cell_2d dual launch at full resolution
    (1, 16, 8, (1, 37, 50)),          # four channel groups, partial tiles
    (1, 4, 20, (3, 19, 33)),          # one group, a partial second output block, ragged
    (1, 8, 4, (1, 2, 16))])           # the smallest eligible plane
def test_x2d_depth1_split_operand_conv(ra, x3_on, nset, cs, cout, shape):
    """conv2d_x3_kernel (round 4): depth-1 volumes under f16x3 — the Feature Net's ConvBR_2d / Cell_2d launches — through the 3x3x3
    entry points with FULL 3x3x3 weights (the taps dz != 1 meet only zero padding, whatever their weights), against F.conv3d in
    float64; destination-channel permutation per group of four."""
    B, H, W = shape
    cin = nset * cs
    x = torch.randn((B, cin, 1, H, W), generator=gen(201)) * 3.0
    ws = [torch.randn((cout, cs, 3, 3, 3), generator=gen(202 + i)) * (2.0 / (9 * cs)) ** 0.5 for i in range(nset)]
    sc = [torch.rand(cout, generator=gen(205 + i)) + 0.5 for i in range(nset)]
    sh = [torch.randn(cout, generator=gen(208 + i)) * 0.1 for i in range(nset)]
    v = lambda t: t.view(1, -1, 1, 1, 1)  # noqa: E731
    ref = sum(F.relu(F.conv3d(x[:, i * cs:(i + 1) * cs].double(), ws[i].double(), padding=1) * v(sc[i].double()) + v(sh[i].double()))
              for i in range(nset))
    ng = cout // 4
    perm = [4 * ((g * 7 + 1) % ng) for g in range(ng)]
    out = torch.full((B, cout, 1, H, W), float("nan"), device=DEV)
    pk = [ra.ops.conv3d_k3_pack(gpu(w)) for w in ws]
    if nset == 2:
        ra.ops.conv3d_k3_dual(gpu(x), cs, pk[0], gpu(sc[0]), gpu(sh[0]), pk[1], gpu(sc[1]), gpu(sh[1]), cout, True, out, perm)
    else:
        ra.ops.conv3d_k3(gpu(x), pk[0], cout, gpu(sc[0]), gpu(sh[0]), True, out, perm)
    exp = torch.empty_like(ref)
    for g in range(ng):
        exp[:, perm[g]:perm[g] + 4] = ref[:, 4 * g:4 * g + 4]
    np.testing.assert_allclose(out.cpu().double().numpy(), exp.numpy(), rtol=2e-4, atol=2e-4)
    # and the same call under strict fp32 (the fp32 matrix-core kernel) agrees with it to the split form's error bound
    with ra.ops.conv_precision("fp32"):
        out32 = torch.empty_like(out)
        if nset == 2:
            ra.ops.conv3d_k3_dual(gpu(x), cs, pk[0], gpu(sc[0]), gpu(sh[0]), pk[1], gpu(sc[1]), gpu(sh[1]), cout, True, out32, perm)
        else:
            ra.ops.conv3d_k3(gpu(x), pk[0], cout, gpu(sc[0]), gpu(sh[0]), True, out32, perm)
    assert float((out - out32).abs().max()) <= 2e-5 * float(exp.abs().max()) + 1e-6


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_k1_resample_multi_equals_separate_launches(ra, dtype):
    """ragmi_conv3d_k1_resample_multi_fwd (round 4): a cell's two 1x1x1 convs and the next cell's pre_preprocess of the same tensor as
    ONE launch, each into its own buffer — bit for bit what three separate ragmi_conv3d_k1_resample_fwd launches write."""
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    g1 = gen(221)
    size = (5, 9, 26)
    a = torch.randn((2, 48) + size, generator=g1).to(td)                 # already at the output size
    b = torch.randn((2, 24, 10, 18, 52), generator=g1).to(td)            # x0.5
    ws = [torch.randn((16, c), generator=g1) * 0.3 for c in (48, 24, 24)]
    sc = [torch.rand(16, generator=g1) + 0.5 for _ in range(3)]
    sh = [torch.randn(16, generator=g1) * 0.1 for _ in range(3)]
    outs = [torch.full((2, 34) + size, float("nan"), device=DEV, dtype=td) for _ in range(2)]
    refs = [torch.full((2, 34) + size, float("nan"), device=DEV, dtype=td) for _ in range(2)]
    xa, xb = gpu(a), gpu(b)
    specs = [(xa, 0, 0, 1), (xb, 1, 0, 17), (xb, 2, 1, 2)]               # (input, weight set, destination buffer, first channel)
    ra.ops.conv3d_k1_resample_multi([(x, gpu(ws[k]), gpu(sc[k]), gpu(sh[k]), True, outs[d], ch) for (x, k, d, ch) in specs], size)
    for (x, k, d, ch) in specs:
        ra.ops.conv3d_k1_resample(x, size, True, gpu(ws[k]), gpu(sc[k]), gpu(sh[k]), True, refs[d], ch)
    for o, r in zip(outs, refs):
        on, rn = o.float().cpu().numpy(), r.float().cpu().numpy()
        assert np.array_equal(np.isnan(on), np.isnan(rn))
        assert np.array_equal(on[~np.isnan(on)], rn[~np.isnan(rn)])


@pytest.mark.parametrize("C,cin0,size0,cin1,size1,size,B", [
    (8, 12, (128, 416), 12, (128, 416), (64, 208), 2),     # Feature Net cell 0: both inputs down-sampled x0.5
    (4, 12, (128, 416), 24, (64, 208), (128, 416), 2),     # cell 1: s0 at the cell's size, s1 up-sampled x2
    (8, 24, (64, 208), 12, (128, 416), (64, 208), 2),      # cell 2: s0 as is, s1 down-sampled
    (4, 9, (21, 50), 17, (41, 99), (41, 99), 3),           # ragged: odd channel counts, odd sizes, partial tiles, up + identity
    (8, 48, (10, 17), 5, (37, 33), (19, 17), 1)])          # 48 input channels; non-integer resample ratios
def test_cell2d_fused_launch(ra, x3_on, C, cin0, size0, cin1, size1, size, B):
    """ragmi_cell2d_fwd (round 4): a Cell_2d of the all-conv genotype as ONE launch — pre_preprocess / preprocess (1x1 ConvBR_2d on the
    bilinear align_corners=True resample of each input, rag_model.py:146-155) computed in the staging of the dual 3x3 launch —
    against the reference's order of operations evaluated by ATen in float64 (interpolation in fp32: its index rule is fp32)."""
    g1 = gen(211)
    steps = 3
    cout = steps * C
    xs = [torch.randn((B, cin0) + size0, generator=g1) * 2.0, torch.randn((B, cin1) + size1, generator=g1) * 2.0]
    w1 = [torch.randn((C, cin0), generator=g1) * 0.4, torch.randn((C, cin1), generator=g1) * 0.4]
    s1 = [torch.rand(C, generator=g1) + 0.5 for _ in range(2)]
    h1 = [torch.randn(C, generator=g1) * 0.2 for _ in range(2)]
    w3 = [torch.randn((cout, C, 3, 3), generator=g1) * (2.0 / (9 * C)) ** 0.5 for _ in range(2)]
    s3 = [torch.rand(cout, generator=g1) + 0.5 for _ in range(2)]
    h3 = [torch.randn(cout, generator=g1) * 0.1 for _ in range(2)]
    v = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    ref = 0
    for i in range(2):
        xi = xs[i] if tuple(xs[i].shape[2:]) == size else F.interpolate(xs[i], size, mode="bilinear", align_corners=True)
        si = F.relu(torch.einsum("oc,bchw->bohw", w1[i].double(), xi.double()) * v(s1[i].double()) + v(h1[i].double()))
        ref = ref + F.relu(F.conv2d(si, w3[i].double(), padding=1) * v(s3[i].double()) + v(h3[i].double()))
    assert ra.ops.cell2d_supported(C, cin0, cin1, cout, *size)
    ng = cout // 4
    perm = [4 * ((g * 7 + 1) % ng) for g in range(ng)]
    out = torch.full((B, cout) + size, float("nan"), device=DEV)
    pk = [ra.ops.conv3d_k3_pack(gpu(w)) for w in w3]
    ra.ops.cell2d(gpu(xs[0]), (gpu(w1[0]), gpu(s1[0]), gpu(h1[0]), True), gpu(xs[1]), (gpu(w1[1]), gpu(s1[1]), gpu(h1[1]), True), C,
                  pk[0], gpu(s3[0]), gpu(h3[0]), pk[1], gpu(s3[1]), gpu(h3[1]), cout, True, out, perm)
    exp = torch.empty_like(ref)
    for g in range(ng):
        exp[:, perm[g]:perm[g] + 4] = ref[:, 4 * g:4 * g + 4]
    np.testing.assert_allclose(out.cpu().double().numpy(), exp.numpy(), rtol=3e-4, atol=3e-4)
    with ra.ops.conv_precision("fp32"):
        assert not ra.ops.cell2d_supported(C, cin0, cin1, cout, *size)       # strict fp32 keeps the separate launches


@pytest.mark.parametrize("nset,cs,cout,shape,dtype", [
    (2, 16, 48, (1, 16, 32, 104), "f32"),      # a level-12 cell launch of the headline forward
    (2, 8, 24, (2, 8, 40, 56), "f32"),         # level-6 shape class: two output blocks over blockIdx.y, two batches
    (1, 16, 20, (2, 5, 61, 57), "f32"),        # ragged everywhere: odd depth, partial boxes, a partial output block
    (1, 8, 8, (2, 33, 64, 8), "f32"),          # narrower than a box
    (2, 8, 40, (1, 4, 40, 104), "f32"),        # three output blocks
    (2, 16, 16, (2, 6, 44, 64), "bf16"),       # bf16 storage: the activations are exact operands (two MFMAs per product)
    (2, 8, 24, (2, 6, 44, 64), "bf16")])
def test_x3_deep_form_vs_oracle(ra, x3_on, nset, cs, cout, shape, dtype):
    """conv3d_x3d_kernel (8 / 16 input channels per set, box tiles, 8-channel operand records): ConvBR_3d / the dual Cell_3d form
    against F.conv3d on the CPU, with a destination-channel permutation per group of four (the fused torch.cat)."""
    B, D, H, W = shape
    cin = nset * cs
    bf = dtype == "bf16"
    x = torch.randn((B, cin, D, H, W), generator=gen(171))
    if bf:
        x = x.to(torch.bfloat16)
    ws = [torch.randn((cout, cs, 3, 3, 3), generator=gen(172 + i)) * (2.0 / (27 * cs)) ** 0.5 for i in range(nset)]
    sc = [torch.rand(cout, generator=gen(175 + i)) + 0.5 for i in range(nset)]
    sh = [torch.randn(cout, generator=gen(178 + i)) * 0.1 for i in range(nset)]
    v = lambda t: t.view(1, -1, 1, 1, 1)  # noqa: E731
    ref = sum(F.relu(F.conv3d(x[:, i * cs:(i + 1) * cs].float(), ws[i], padding=1) * v(sc[i]) + v(sh[i])) for i in range(nset))
    assert ra.ops.conv3d_k3_uses_x3(cin, cout, B, D, H, W, nset=nset, dtype=torch.bfloat16 if bf else torch.float32)
    ng = (cout + 3) // 4
    perm = [4 * ((g * 7 + 1) % ng) for g in range(ng)] if cout % 4 == 0 else None     # group g lands at channel perm[g]
    out = torch.full((B, cout, D, H, W), float("nan"), device=DEV, dtype=torch.bfloat16 if bf else torch.float32)
    pk = [ra.ops.conv3d_k3_pack(gpu(w)) for w in ws]
    if nset == 2:
        ra.ops.conv3d_k3_dual(gpu(x), cs, pk[0], gpu(sc[0]), gpu(sh[0]), pk[1], gpu(sc[1]), gpu(sh[1]), cout, True, out, perm)
    else:
        ra.ops.conv3d_k3(gpu(x), pk[0], cout, gpu(sc[0]), gpu(sh[0]), True, out, perm)
    exp = ref
    if perm is not None:
        exp = torch.empty_like(ref)
        for g in range(ng):
            exp[:, perm[g]:perm[g] + 4] = ref[:, 4 * g:4 * g + 4]
    tol = dict(rtol=1e-2, atol=2e-2) if bf else dict(rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(out.float().cpu().numpy(), exp.numpy(), **tol)


@pytest.mark.parametrize("shape,nreg,couts", [((1, 16, 128, 128), 1, (8,)),         # cell 1's launch: one full-resolution tail + a 12 -> 8 down pair
                                              ((2, 16, 132, 160), 0, (8,)),         # cell 2's launch: down tails only; two samples; partial tiles
                                              ((1, 32, 128, 64), 2, (4, 4)),        # two regular tails + two separate 4-channel down tails
                                              ((1, 14, 128, 160), 1, (8,)),         # D % 4 == 2: last depth segment of 6 planes, 20 pairs per group
                                              ((1, 26, 64, 192), 0, (4, 4))])       # eligible for the half-item split; last segment 2
def test_x3_down_sampling_tails(ra, x3_on, shape, nreg, couts):
    """Down-sampling tails of the z-marching split-operand kernel (round 4): the 1x1x1 ConvBR_3d of a consumer cell that works one
    level down — F.interpolate(x, half size, 'trilinear', align_corners=True) followed by pre_preprocess / preprocess
    (rag_model.py:146-155) — computed conv-first in the PRODUCER's epilogue, against the reference order (resample, then mix)
    evaluated by ATen in fp32 / float64.  The producer's own output and its full-resolution tails must be unchanged."""
    B, D, H, W = shape
    C, cout = 4, 12
    g1 = gen(191)
    x = torch.randn((B, 2 * C, D, H, W), generator=g1)
    wa, wb = (torch.randn((cout, C, 3, 3, 3), generator=g1) * 0.2 for _ in range(2))
    sa, sb = (torch.rand(cout, generator=g1) + 0.5 for _ in range(2))
    ha, hb = (torch.randn(cout, generator=g1) * 0.1 for _ in range(2))
    v = lambda t: t.view(1, -1, 1, 1, 1)  # noqa: E731
    main = sum(F.relu(F.conv3d(x[:, i * C:(i + 1) * C].double(), w.double(), padding=1) * v(s.double()) + v(h.double()))
               for i, (w, s, h) in enumerate(((wa, sa, ha), (wb, sb, hb))))
    assert ra.ops.down2_tail_supported(D, H, W)
    half = (D // 2, H // 2, W // 2)
    tails, checks = [], []
    for k in range(nreg):
        tw, ts, th = torch.randn((4, cout), generator=g1) * 0.3, torch.rand(4, generator=g1) + 0.5, torch.randn(4, generator=g1) * 0.1
        out = torch.full((B, 5, D, H, W), float("nan"), device=DEV)
        tails.append(ra.ops.Tail(gpu(tw), gpu(ts), gpu(th), True, out, 1))
        ref = F.relu(torch.einsum("oc,bcdhw->bodhw", tw.double(), main) * v(ts.double()) + v(th.double()))
        checks.append((out, 1, 4, ref))
    for k, co in enumerate(couts):
        tw, ts, th = torch.randn((co, cout), generator=g1) * 0.3, torch.rand(co, generator=g1) + 0.5, torch.randn(co, generator=g1) * 0.1
        out = torch.full((B, co + 2, ) + half, float("nan"), device=DEV)
        gw, gs, gh = gpu(tw), gpu(ts), gpu(th)
        for c0 in range(0, co, 4):
            tails.append(ra.ops.Tail(gw[c0:c0 + 4], gs[c0:c0 + 4], gh[c0:c0 + 4], k == 0, out, 1 + c0, down=True))
        low = F.interpolate(main.float(), half, mode="trilinear", align_corners=True).double()      # the reference order: resample first
        ref = torch.einsum("oc,bcdhw->bodhw", tw.double(), low) * v(ts.double()) + v(th.double())
        checks.append((out, 1, co, F.relu(ref) if k == 0 else ref))
    ones = lambda t: gpu(t)  # noqa: E731
    y = torch.full((B, cout, D, H, W), float("nan"), device=DEV)
    with ra.ops.conv_precision("f16x3"):
        assert ra.ops.conv3d_k3_uses_x3(2 * C, cout, B, D, H, W, nset=2, ntail=len(tails))
        ra.ops.conv3d_k3_dual(gpu(x), C, ra.ops.conv3d_k3_pack(gpu(wa)), ones(sa), ones(ha), ra.ops.conv3d_k3_pack(gpu(wb)), ones(sb), ones(hb),
                              cout, True, y, tails=tails)
    np.testing.assert_allclose(y.cpu().double().numpy(), main.numpy(), rtol=2e-4, atol=2e-4)
    for (out, ch0, co, ref) in checks:
        got = out.cpu().double()
        assert torch.isnan(got[:, 0]).all() and torch.isnan(got[:, ch0 + co:]).all()
        np.testing.assert_allclose(got[:, ch0:ch0 + co].numpy(), ref.numpy(), rtol=3e-4, atol=3e-4)


def test_x3_down_sampling_tails_bf16_storage(ra):
    """The same down-sampling tails under bf16 activation storage (BASELINE configs[2]): bf16 in and out, fp32 on chip — against the
    reference order evaluated in float64 from the SAME bf16 inputs, to the storage format's rounding (2^-8 relative per stored value)."""
    B, D, H, W = 1, 16, 128, 128
    C, cout = 4, 12
    g1 = gen(231)
    x = torch.randn((B, 2 * C, D, H, W), generator=g1).to(torch.bfloat16)
    wa, wb = (torch.randn((cout, C, 3, 3, 3), generator=g1) * 0.2 for _ in range(2))
    sa, sb = (torch.rand(cout, generator=g1) + 0.5 for _ in range(2))
    ha, hb = (torch.randn(cout, generator=g1) * 0.1 for _ in range(2))
    v = lambda t: t.view(1, -1, 1, 1, 1)  # noqa: E731
    main = sum(F.relu(F.conv3d(x[:, i * C:(i + 1) * C].double(), w.double(), padding=1) * v(s.double()) + v(h.double()))
               for i, (w, s, h) in enumerate(((wa, sa, ha), (wb, sb, hb))))
    half = (D // 2, H // 2, W // 2)
    tw, ts, th = torch.randn((8, cout), generator=g1) * 0.3, torch.rand(8, generator=g1) + 0.5, torch.randn(8, generator=g1) * 0.1
    out = torch.full((B, 10) + half, float("nan"), device=DEV, dtype=torch.bfloat16)
    gw, gs, gh = gpu(tw), gpu(ts), gpu(th)
    tails = [ra.ops.Tail(gw[c0:c0 + 4], gs[c0:c0 + 4], gh[c0:c0 + 4], True, out, 1 + c0, down=True) for c0 in (0, 4)]
    low = F.interpolate(main.float(), half, mode="trilinear", align_corners=True).double()
    ref = F.relu(torch.einsum("oc,bcdhw->bodhw", tw.double(), low) * v(ts.double()) + v(th.double()))
    y = torch.full((B, cout, D, H, W), float("nan"), device=DEV, dtype=torch.bfloat16)
    assert ra.ops.conv3d_k3_uses_x3(2 * C, cout, B, D, H, W, nset=2, ntail=len(tails), dtype=torch.bfloat16)
    ra.ops.conv3d_k3_dual(gpu(x), C, ra.ops.conv3d_k3_pack(gpu(wa)), gpu(sa), gpu(ha), ra.ops.conv3d_k3_pack(gpu(wb)), gpu(sb), gpu(hb),
                          cout, True, y, tails=tails)
    np.testing.assert_allclose(y.float().cpu().double().numpy(), main.numpy(), rtol=1e-2, atol=2e-2)
    got = out.float().cpu().double()
    assert torch.isnan(got[:, 0]).all() and torch.isnan(got[:, 9:]).all()
    np.testing.assert_allclose(got[:, 1:9].numpy(), ref.numpy(), rtol=1e-2, atol=2e-2)


def test_costvol_stem_conv3d_fused_bf16_storage(ra):
    """The fused stems under bf16 activation storage (BASELINE configs[2]): stem3d1's staging rounds the expanded values to bf16 exactly
    as the store of the two-launch path does, so stem3d1's output and its own tails have the two-launch path's bits; stem3d0's tail in
    the product's idle rows (RAGMI_TAIL_ROWS) is formed from the ROUNDED activations (the two-launch path forms it before the store),
    so it agrees to the storage format's rounding."""
    B, h, w, maxdisp = 2, 72, 132, 96
    C, cmid, cout = 12, 12, 12
    g1 = gen(571)
    L, R = torch.randn((B, C, h, w), generator=g1).to(BF), torch.randn((B, C, h, w), generator=g1).to(BF)
    w0 = torch.randn((cmid, 2 * C, 3, 3, 3), generator=g1) * 0.05
    w1 = torch.randn((cout, cmid, 3, 3, 3), generator=g1) * 0.1
    s0, h0 = torch.rand(cmid, generator=g1) + 0.5, torch.randn(cmid, generator=g1) * 0.1
    s1, h1 = torch.rand(cout, generator=g1) + 0.5, torch.randn(cout, generator=g1) * 0.1
    tw0 = torch.randn((4, cmid), generator=g1) * 0.3
    tw1 = [torch.randn((4, cout), generator=g1) * 0.3 for _ in range(2)]
    d = maxdisp // 3
    assert ra.ops.costvol_stem_conv3d_supported(C, cmid, cout, B, d, h, w, ntail=2, dtype=BF)
    var = ra.ops.costvol_stem_prepare(gpu(w0))
    pk = ra.ops.conv3d_k3_pack(gpu(w1))
    pk16 = ra.ops.conv3d_k3_pack(ra.ops.stem_tail_rows_weight(gpu(w1), gpu(tw0)))
    outs = {}
    for mode in ("two launches", "fused", "fused, tail in the rows", "again"):
        pre0 = torch.full((B, 8, d, h, w), float("nan"), device=DEV, dtype=BF)
        pre1 = torch.full((B, 8, d, h, w), float("nan"), device=DEV, dtype=BF)
        t0 = [ra.ops.Tail(gpu(tw0), None, None, True, pre0, 0)]
        t1 = [ra.ops.Tail(gpu(tw1[0]), None, None, True, pre0, 4), ra.ops.Tail(gpu(tw1[1]), None, None, False, pre1, 0)]
        y = torch.full((B, cout, d, h, w), float("nan"), device=DEV, dtype=BF)
        if mode == "two launches":
            mid = ra.ops.costvol_stem(gpu(L), gpu(R), maxdisp, var, cmid, gpu(s0), gpu(h0), True, tails=t0)
            ra.ops.conv3d_k3(mid, pk, cout, gpu(s1), gpu(h1), True, y, None, tails=t1)
        else:
            rows = mode != "fused"
            ra.ops.costvol_stem_conv3d(gpu(L), gpu(R), maxdisp, var, cmid, gpu(s0), gpu(h0), True, t0, pk16 if rows else pk, cout, gpu(s1), gpu(h1),
                                       True, y, None, tails=t1, store_main=True, tail0_rows=rows)
        outs[mode] = (y, pre0, pre1)
    eq = lambda a_, b_: torch.equal(torch.nan_to_num(a_.float(), nan=-7.0), torch.nan_to_num(b_.float(), nan=-7.0))  # noqa: E731
    ref = outs["two launches"]
    assert all(eq(a_, b_) for a_, b_ in zip(outs["fused"], ref))
    assert all(eq(a_, b_) for a_, b_ in zip(outs["fused, tail in the rows"], outs["again"]))
    rows = outs["fused, tail in the rows"]
    assert eq(rows[0], ref[0]) and eq(rows[2], ref[2]) and eq(rows[1][:, 4:], ref[1][:, 4:])
    np.testing.assert_allclose(rows[1][:, :4].float().cpu().numpy(), ref[1][:, :4].float().cpu().numpy(), rtol=2e-2, atol=3e-2)
    assert torch.isnan(rows[2][:, 4:]).all() and not torch.isnan(rows[1]).any()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_conv3d_k1_chain_bitwise(ra, dt):
    """Two 1x1x1 ConvBR_3d in a row as one launch (the head's last_12_3d -> last_6_3d's channel mix, rag_model.py:358-365) against the
    two conv3d_k1 launches: the same fmaf chains in the same order (bf16 storage: the intermediate rounded as its store would be) —
    the same bits; and against float64."""
    g1 = gen(621)
    x = torch.randn((2, 48, 9, 20, 31), generator=g1).to(dt)
    w1, w2 = torch.randn((24, 48), generator=g1) * 0.2, torch.randn((12, 24), generator=g1) * 0.3
    s1, h1 = torch.rand(24, generator=g1) + 0.5, torch.randn(24, generator=g1) * 0.1
    s2, h2 = torch.rand(12, generator=g1) + 0.5, torch.randn(12, generator=g1) * 0.1
    assert ra.ops.conv3d_k1_chain_supported(48, 24, 12) and not ra.ops.conv3d_k1_chain_supported(48, 16, 12)
    mid = torch.empty((2, 24, 9, 20, 31), device=DEV, dtype=dt)
    ra.ops.conv3d_k1(gpu(x), gpu(w1), gpu(s1), gpu(h1), True, mid)
    sep = torch.full((2, 14, 9, 20, 31), float("nan"), device=DEV, dtype=dt)
    ra.ops.conv3d_k1(mid, gpu(w2), gpu(s2), gpu(h2), False, sep, 1)
    one = torch.full((2, 14, 9, 20, 31), float("nan"), device=DEV, dtype=dt)
    ra.ops.conv3d_k1_chain(gpu(x), gpu(w1), gpu(s1), gpu(h1), True, gpu(w2), gpu(s2), gpu(h2), False, one, 1)
    assert torch.equal(torch.nan_to_num(one.float(), nan=-7.0), torch.nan_to_num(sep.float(), nan=-7.0))
    v = lambda t: t.view(1, -1, 1, 1, 1)  # noqa: E731
    hid = F.relu(torch.einsum("oc,bcdhw->bodhw", w1.double(), x.double()) * v(s1.double()) + v(h1.double()))
    ref = torch.einsum("oc,bcdhw->bodhw", w2.double(), hid) * v(s2.double()) + v(h2.double())
    tol = 2e-4 if dt == torch.float32 else 3e-2
    np.testing.assert_allclose(one[:, 1:13].float().cpu().double().numpy(), ref.numpy(), rtol=tol, atol=tol)


def test_mixed_storage_edges_round_to_the_bf16_results(ra):
    """The two launches that cross from bf16 storage into the fp32 levels (round 5, include/rag_amd.h "Mixed storage"): a
    down-sampling tail with an fp32 destination (RAGMI_TAIL_F32) and the resample + 1x1x1 launch with an fp32 output
    (RAGMI_BF16 | RAGMI_OUT_F32) do the arithmetic of their bf16-destination twins and skip the final rounding — so rounding their
    output to bf16 gives the twins' bits; nothing else of the launch changes."""
    B, D, H, W = 1, 16, 128, 128
    C, cout = 4, 12
    g1 = gen(233)
    x = torch.randn((B, 2 * C, D, H, W), generator=g1).to(torch.bfloat16)
    wa, wb = (torch.randn((cout, C, 3, 3, 3), generator=g1) * 0.2 for _ in range(2))
    sa, sb = (torch.rand(cout, generator=g1) + 0.5 for _ in range(2))
    ha, hb = (torch.randn(cout, generator=g1) * 0.1 for _ in range(2))
    half = (D // 2, H // 2, W // 2)
    tw, ts, th = torch.randn((8, cout), generator=g1) * 0.3, torch.rand(8, generator=g1) + 0.5, torch.randn(8, generator=g1) * 0.1
    gw, gs, gh = gpu(tw), gpu(ts), gpu(th)
    pa, pb = ra.ops.conv3d_k3_pack(gpu(wa)), ra.ops.conv3d_k3_pack(gpu(wb))
    res = {}
    for odt in (torch.bfloat16, torch.float32):
        out = torch.full((B, 10) + half, float("nan"), device=DEV, dtype=odt)
        tails = [ra.ops.Tail(gw[c0:c0 + 4], gs[c0:c0 + 4], gh[c0:c0 + 4], True, out, 1 + c0, down=True) for c0 in (0, 4)]
        y = torch.full((B, cout, D, H, W), float("nan"), device=DEV, dtype=torch.bfloat16)
        ra.ops.conv3d_k3_dual(gpu(x), C, pa, gpu(sa), gpu(ha), pb, gpu(sb), gpu(hb), cout, True, y, tails=tails)
        res[odt] = (y, out)
    assert torch.equal(res[torch.float32][0], res[torch.bfloat16][0])
    o32, o16 = res[torch.float32][1], res[torch.bfloat16][1]
    assert o32.dtype == torch.float32 and torch.isnan(o32[:, 0]).all() and torch.isnan(o32[:, 9:]).all()
    assert torch.equal(o32[:, 1:9].to(torch.bfloat16), o16[:, 1:9])
    assert not torch.equal(o32[:, 1:9], o16[:, 1:9].float())           # (the fp32 destination really keeps more bits)
    # a full-resolution tail cannot cross: loud failure, not a reinterpretation of the buffer
    bad = ra.ops.Tail(gw[:4], gs[:4], gh[:4], True, torch.empty((B, 4, D, H, W), device=DEV), 0)
    with pytest.raises(RuntimeError):
        ra.ops.conv3d_k3_dual(gpu(x), C, pa, gpu(sa), gpu(ha), pb, gpu(sb), gpu(hb), cout, True,
                              torch.empty((B, cout, D, H, W), device=DEV, dtype=torch.bfloat16), tails=[bad])
    # resample + 1x1x1: x0.25 (cell 4's pre_preprocess), x0.5, and an input already at the output size
    xin = torch.randn((2, 12, 16, 40, 48), generator=g1).to(torch.bfloat16)
    w2 = torch.randn((16, 12), generator=g1) * 0.3
    s2, h2 = torch.rand(16, generator=g1) + 0.5, torch.randn(16, generator=g1) * 0.1
    for size in ((4, 10, 12), (8, 20, 24), (16, 40, 48)):
        o16 = torch.full((2, 18) + size, float("nan"), device=DEV, dtype=torch.bfloat16)
        o32 = torch.full((2, 18) + size, float("nan"), device=DEV)
        ra.ops.conv3d_k1_resample(gpu(xin), size, True, gpu(w2), gpu(s2), gpu(h2), True, o16, 1)
        ra.ops.conv3d_k1_resample(gpu(xin), size, True, gpu(w2), gpu(s2), gpu(h2), True, o32, 1)
        assert torch.isnan(o32[:, 0]).all() and torch.isnan(o32[:, 17]).all()
        assert torch.equal(o32[:, 1:17].to(torch.bfloat16), o16[:, 1:17]), size
        low = F.interpolate(xin.float(), size, mode="trilinear", align_corners=True).double()
        ref = F.relu(torch.einsum("oc,bcdhw->bodhw", w2.double(), low) * s2.double().view(1, -1, 1, 1, 1) + h2.double().view(1, -1, 1, 1, 1))
        np.testing.assert_allclose(o32[:, 1:17].cpu().double().numpy(), ref.numpy(), rtol=2e-4, atol=2e-4)
    with pytest.raises(RuntimeError):       # fp32 -> bf16 is not a crossing the executor makes
        ra.ops.conv3d_k1_resample(gpu(xin).float(), (8, 20, 24), True, gpu(w2), gpu(s2), gpu(h2), True,
                                  torch.empty((2, 16, 8, 20, 24), device=DEV, dtype=torch.bfloat16), 0)


def test_matchingnet_mixed_storage_plan(ra):
    """What MatchingNet._run_chain stores in which type under bf16 inputs (ops.set_bf16_deep_fp32): the level-3 cells' buffers bf16,
    everything from the first cell below the cost volume's resolution on fp32; with the switch off every buffer bf16."""
    rows = O.ALL_CONV
    net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=48)
    net.load_state_dict(O.random_matching_state_dict(rows, seed=3), strict=True)
    net = net.to(DEV).eval()
    lf, rf = (torch.randn((1, 12, 48, 72), generator=gen(7 + k)) for k in range(2))
    seen = {}
    orig = ra.ops.conv3d_k3_dual

    def spy(x, *a, **kw):
        seen.setdefault(tuple(x.shape[2:]), set()).add(x.dtype)
        return orig(x, *a, **kw)

    ra.ops.conv3d_k3_dual = spy
    try:
        with torch.no_grad():
            d_mixed = net(gpu(lf).to(BF), gpu(rf).to(BF))
            mixed = {k: set(v) for k, v in seen.items()}
            seen.clear()
            ra.ops.set_bf16_deep_fp32(False)
            d_all = net(gpu(lf).to(BF), gpu(rf).to(BF))
            every = {k: set(v) for k, v in seen.items()}
            d32 = net(gpu(lf), gpu(rf))
    finally:
        ra.ops.conv3d_k3_dual = orig
        ra.ops.set_bf16_deep_fp32(True)
    full = (16, 48, 72)
    assert mixed[full] == {torch.bfloat16} and all(v == {torch.float32} for k, v in mixed.items() if k != full) and len(mixed) == 3
    assert all(v == {torch.bfloat16} for v in every.values()) and len(every) == 3
    e_mixed, e_all = O.epe(d_mixed.cpu(), d32.cpu()), O.epe(d_all.cpu(), d32.cpu())
    print(f"EPE vs the fp32 build: mixed storage {e_mixed:.3e} px, every tensor bf16 {e_all:.3e} px")
    assert e_mixed < e_all


def test_x3_dual_tails_and_headline_epe(ra, x3_on):
    """The level-3 launches of the headline forward (stem3d1 with fused tails and no main store, dual cells) on the f16x3
    kernel: EPE vs the CPU oracle stays within the gate (measured 1.2e-4 px; fp32-MFMA path 1.5e-5 px)."""
    rows = O.ALL_CONV
    sd = O.random_matching_state_dict(rows, seed=0)
    net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=192)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    lf, rf = torch.randn((1, 12, 128, 416), generator=gen(131)), torch.randn((1, 12, 128, 416), generator=gen(132))
    assert ra.ops.conv3d_k3_uses_x3(8, 12, 1, 64, 128, 416, nset=2, ntail=2)
    with torch.no_grad():
        disp = net(gpu(lf), gpu(rf)).cpu()
    torch.set_num_threads(16)
    ref = O.matching_net_forward(lf, rf, sd, rows, 192)
    epe = O.epe(disp, ref)
    assert epe <= EPE_GATE, epe


def test_x3_precision_is_an_abi_argument(ra):
    """The precision is chosen per call by the dtype argument (RAGMI_F32 vs RAGMI_F32X3), never by the environment: same entry
    point, fp32-MFMA kernel vs f16x3 kernel, results within the documented bound of each other; an environment variable set
    after import changes nothing."""
    import os
    x = torch.randn((1, 12, 64, 128, 130), generator=gen(141))
    w = torch.randn((12, 12, 3, 3, 3), generator=gen(142)) * 0.1
    pk, xg = ra.ops.conv3d_k3_pack(gpu(w)), gpu(x)
    outs = {}
    for prec in ("f16x3", "fp32"):
        with ra.ops.conv_precision(prec):
            assert ra.ops.conv3d_k3_uses_x3(12, 12, 1, 64, 128, 130) == (prec == "f16x3")
            outs[prec] = ra.ops.conv3d_k3(xg, pk, 12, None, None, False, torch.empty((1, 12, 64, 128, 130), device=DEV))
    assert not torch.equal(outs["fp32"], outs["f16x3"])
    np.testing.assert_allclose(outs["f16x3"].cpu().numpy(), outs["fp32"].cpu().numpy(), rtol=1e-4, atol=1e-4)
    old = os.environ.get("RAGMI_X3")
    try:
        os.environ["RAGMI_X3"] = "0"
        with ra.ops.conv_precision("f16x3"):
            again = ra.ops.conv3d_k3(xg, pk, 12, None, None, False, torch.empty((1, 12, 64, 128, 130), device=DEV))
        assert torch.equal(again, outs["f16x3"])
    finally:
        if old is None:
            os.environ.pop("RAGMI_X3", None)
        else:
            os.environ["RAGMI_X3"] = old
    # the raw ABI: dtype 0 (RAGMI_F32) never takes the f16x3 kernel, dtype 2 (RAGMI_F32X3) does on this shape
    lib = ra.load_library()
    assert lib.ragmi_conv3d_k3_uses_x3(12, 12, 1, 64, 128, 130, 1, 0, 0, 0) == 0
    assert lib.ragmi_conv3d_k3_uses_x3(12, 12, 1, 64, 128, 130, 1, 0, 0, 2) == 1


def test_x3_error_bound_adversarial(ra):
    """The bound include/rag_amd.h documents for RAGMI_F32X3 (scaled fp16 halves), per output
        |y - y_exact| <= 2^-20 * sum_k |w_k x_k|  +  2^-33 * (Xmax * sum_k |w_k| + Wrow * sum_k |x_k|)
    (Xmax: largest |x| of the workgroup's column segment, here bounded by the tensor's; Wrow: largest |w| of the output channel)
    against an fp64 convolution on inputs chosen to hurt: (a) activations with a large common offset (post-ReLU-like, 1000 + N(0,1))
    under zero-sum weights — the exact result is O(1) while every product is O(100), so the error is judged against sum |w x|, not
    |y|: the block term is negligible there and the plain relative bound 1e-6 must hold; (b) operands spanning 2^-20 .. 2^20 in
    magnitude ELEMENT BY ELEMENT, where a block-scaled format loses the small operands next to large ones: the second term.  The strict
    RAGMI_F32 path is held to 1e-6 * sum |w x| on the same data."""
    D, H, W, cin, cout = 16, 128, 130, 4, 12
    g1 = gen(161)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g1) * 0.1
    w = w - w.mean(dim=(1, 2, 3, 4), keepdim=True)                      # every output channel's weights sum to zero
    xa = 1000.0 + torch.randn((1, cin, D, H, W), generator=g1)
    e = torch.randint(-20, 21, (1, cin, D, H, W), generator=g1).float()
    xb = torch.randn((1, cin, D, H, W), generator=g1) * torch.exp2(e)
    wb = w * torch.exp2(torch.randint(-20, 21, w.shape, generator=g1).float())
    for name, x, wt in (("offset", xa, w), ("range", xb, wb)):
        # fp64 reference and sum |w x| on a z-slab (interior planes 1..6 of an 8-plane crop: the crop's own z borders are excluded)
        xs, sl = x[:, :, :8].double(), slice(1, 7)
        ref = F.conv3d(xs, wt.double(), padding=1)[:, :, sl]
        mag = F.conv3d(xs.abs(), wt.double().abs(), padding=1)[:, :, sl]
        wrow = wt.double().abs().flatten(1).max(dim=1).values.view(1, -1, 1, 1, 1)
        sum_w = wt.double().abs().flatten(1).sum(dim=1).view(1, -1, 1, 1, 1)
        sum_x = F.conv3d(xs.abs(), torch.ones((1, cin, 3, 3, 3), dtype=torch.float64), padding=1)[:, :, sl]
        block = float(x.abs().max()) * sum_w + wrow * sum_x
        pk = ra.ops.conv3d_k3_pack(gpu(wt))
        for prec in ("f16x3", "fp32"):
            with ra.ops.conv_precision(prec):
                assert ra.ops.conv3d_k3_uses_x3(cin, cout, 1, D, H, W) == (prec == "f16x3")
                out = ra.ops.conv3d_k3(gpu(x), pk, cout, None, None, False, torch.empty((1, cout, D, H, W), device=DEV))
            abs_err = (out[:, :, sl].cpu().double() - ref).abs()
            rel = float((abs_err / mag.clamp_min(1e-300)).max())
            if prec == "fp32" or name == "offset":
                print(f"x3 bound [{name}] {prec}: max |err| / sum|w x| = {rel:.3e} (bound 1e-06)")
                assert rel <= 1e-6, (name, prec, rel)
            else:
                bound = 2.0 ** -20 * mag + 2.0 ** -33 * block
                worst = float((abs_err / bound).max())
                print(f"x3 bound [{name}] {prec}: max |err| / sum|w x| = {rel:.3e}; max |err| / documented bound = {worst:.3f} (must be <= 1)")
                assert worst <= 1.0, (name, prec, worst, rel)


def test_x3_scale_restart_on_growing_planes(ra):
    """The fp16 operand scale of a column segment is chosen from its first plane; a later plane that does not fit makes the
    workgroup restart its ring with a larger scale (conv3d_x3.hip).  Planes that start at exactly zero (the scale clamp), grow by
    1e3 and again by 1e4 inside a segment, and shrink again force that path several times per column; the result must stay inside
    the documented bound against an fp64 convolution, for the single and the dual (two-set) launch."""
    D, H, W, cin, cout = 16, 128, 130, 4, 12
    g1 = gen(171)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g1) * 0.1
    w2 = torch.randn((cout, cin, 3, 3, 3), generator=g1) * 0.1
    zscale = torch.tensor([0, 0, 0, 1, 1e3, 1e3, 1e7, 1e3, 1e-3, 1, 1e4, 1e4, 1e4, 1e-2, 3e4, 0], dtype=torch.float32).view(1, 1, D, 1, 1)
    x = torch.randn((1, 2 * cin, D, H, W), generator=g1) * zscale
    ref_a = F.conv3d(x[:, :cin].double(), w.double(), padding=1)
    ref_b = F.conv3d(x[:, cin:].double(), w2.double(), padding=1)
    mag_a = F.conv3d(x[:, :cin].double().abs(), w.double().abs(), padding=1)
    mag_b = F.conv3d(x[:, cin:].double().abs(), w2.double().abs(), padding=1)

    def block(xs, wt):
        wrow = wt.double().abs().flatten(1).max(dim=1).values.view(1, -1, 1, 1, 1)
        sum_w = wt.double().abs().flatten(1).sum(dim=1).view(1, -1, 1, 1, 1)
        sum_x = F.conv3d(xs.double().abs(), torch.ones((1, cin, 3, 3, 3), dtype=torch.float64), padding=1)
        return float(xs.abs().max()) * sum_w + wrow * sum_x

    with ra.ops.conv_precision("f16x3"):
        assert ra.ops.conv3d_k3_uses_x3(cin, cout, 1, D, H, W) and ra.ops.conv3d_k3_uses_x3(2 * cin, cout, 1, D, H, W, 2)
        one = ra.ops.conv3d_k3(gpu(x[:, :cin].contiguous()), ra.ops.conv3d_k3_pack(gpu(w)), cout, None, None, False,
                               torch.empty((1, cout, D, H, W), device=DEV)).cpu().double()
        ones, zeros = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
        dual = ra.ops.conv3d_k3_dual(gpu(x), cin, ra.ops.conv3d_k3_pack(gpu(w)), ones, zeros, ra.ops.conv3d_k3_pack(gpu(w2)), ones, zeros,
                                     cout, False, torch.empty((1, cout, D, H, W), device=DEV)).cpu().double()
    assert torch.isfinite(one).all() and torch.isfinite(dual).all()
    b1 = 2.0 ** -20 * mag_a + 2.0 ** -33 * block(x[:, :cin], w)
    worst1 = float(((one - ref_a).abs() / b1.clamp_min(1e-300)).max())
    b2 = 2.0 ** -20 * (mag_a + mag_b) + 2.0 ** -33 * (block(x[:, :cin], w) + block(x[:, cin:], w2))
    worst2 = float(((dual - (ref_a + ref_b)).abs() / b2.clamp_min(1e-300)).max())
    rel1 = float(((one - ref_a).abs() / mag_a.clamp_min(1e-300))[:, :, 3:15].max())
    print(f"x3 with scale restarts: |err| / documented bound = {worst1:.3f} (single), {worst2:.3f} (dual); |err| / sum|w x| on the non-zero planes {rel1:.2e}")
    assert worst1 <= 1.0 and worst2 <= 1.0


def test_x3_non_finite_inputs_terminate(ra):
    """An Inf (or an operand too large to scale into fp16) can never fit the operand scale: the kernel must not keep restarting its
    ring for it.  Contract (include/rag_amd.h): non-finite inputs give non-finite outputs where they reach, finite outputs elsewhere
    stay finite; NaNs propagate without touching the scale."""
    D, H, W, cin, cout = 16, 128, 130, 4, 12
    g1 = gen(181)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g1) * 0.1
    x = torch.randn((1, cin, D, H, W), generator=g1)
    x[0, 1, 5, 40, 50] = float("inf")
    x[0, 2, 12, 100, 7] = float("nan")
    x[0, 0, 9, 64, 64] = 3e38
    with ra.ops.conv_precision("f16x3"):
        out = ra.ops.conv3d_k3(gpu(x), ra.ops.conv3d_k3_pack(gpu(w)), cout, None, None, False, torch.empty((1, cout, D, H, W), device=DEV))
    torch.cuda.synchronize()
    out = out.cpu()
    assert not torch.isfinite(out[0, :, 4:7, 39:42, 49:52]).all()                # the Inf's neighbourhood
    assert torch.isnan(out[0, :, 11:14, 99:102, 6:9]).all()                      # the NaN's neighbourhood, all 27 x cout outputs
    far = out[0, :, :3, :20, 80:]                                                 # a column no bad value reaches
    ref = F.conv3d(x[:, :, :4, :21, 79:].double(), w.double(), padding=1)[0, :, :3, :20, 1:]
    assert torch.isfinite(far).all()
    np.testing.assert_allclose(far.numpy(), ref.numpy(), rtol=2e-4, atol=2e-4)


def test_x3_non_finite_inputs_leave_their_tile_mates_alone(ra):
    """an Inf — or a finite outlier no power-of-two scale can bring into fp16 (3e38) — must not pick the tile's operand
    scale: with the scale pinned at its floor every ordinary activation of the 8 x 32 tile flushed to fp16 zero for the rest of the
    depth segment, finite but WRONG.  Such elements take no part in the running maximum now: outputs whose 3x3x3 window holds them
    are non-finite (as under RAGMI_F32 / the reference's fp32), every other voxel of the SAME tile and segment is right."""
    D, H, W, cin, cout = 16, 128, 130, 4, 12
    g1 = gen(183)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g1) * 0.1
    x = torch.randn((1, cin, D, H, W), generator=g1)
    x[0, 1, 2, 4, 5] = float("inf")            # tile (y 0..7, x 0..31), early in its depth segment
    x[0, 3, 3, 12, 40] = 3e38                  # tile (y 8..15, x 32..63)
    with ra.ops.conv_precision("f16x3"):
        assert ra.ops.conv3d_k3_uses_x3(cin, cout, 1, D, H, W)
        out = ra.ops.conv3d_k3(gpu(x), ra.ops.conv3d_k3_pack(gpu(w)), cout, None, None, False, torch.empty((1, cout, D, H, W), device=DEV))
    torch.cuda.synchronize()
    out = out.cpu()
    ref = F.conv3d(x.double().nan_to_num(posinf=0.0).clamp(max=1e30), w.double(), padding=1)[0]      # bad values zeroed: valid outside their reach
    reach = torch.zeros((D, H, W), dtype=torch.bool)
    reach[1:4, 3:6, 4:7] = True
    reach[2:5, 11:14, 39:42] = True
    assert not torch.isfinite(out[0][:, reach]).all()
    for (ys, xs) in ((slice(0, 8), slice(0, 32)), (slice(8, 16), slice(32, 64))):      # the two tiles, whole depth
        ok = ~reach[:, ys, xs]
        got, exp = out[0][:, :, ys, xs][:, ok], ref[:, :, ys, xs][:, ok]
        assert torch.isfinite(got).all()
        np.testing.assert_allclose(got.numpy(), exp.numpy(), rtol=2e-4, atol=2e-4)


def test_x3_deep_form_first_box_wave_skew_and_halo_inf(ra):
    """Two deep-form (conv3d_x3d_kernel) hazards.  (a) ADVICE r03: the three box-maximum slots are zeroed by one wave while the other
    waves may already atomicMax their part of the FIRST box — a lost maximum gave that box a scale from a partial maximum and fp16
    overflow when the lost wave's values were > 4x the rest; the slots are now zeroed behind a barrier.  Every workgroup's first box
    here holds one small sub-region 1e3 x larger than the rest.  (b) VERDICT r03 8(e): an Inf outside a voxel's 3x3x3 window must
    not reach it through a zero-weight K slot: voxels one past the Inf's reach stay finite and right."""
    B, cs, cout, D, H, W = 1, 16, 48, 16, 32, 104
    g1 = gen(185)
    x = torch.randn((B, 2 * cs, D, H, W), generator=g1)
    # a spike region per box (boxes are 2 x 8 x 16): the last rows of the box's second plane — staged by the workgroup's last waves
    x[:, :, 1::2, 6::8, :] *= 1e3
    ws = [torch.randn((cout, cs, 3, 3, 3), generator=g1) * (2.0 / (27 * cs)) ** 0.5 for _ in range(2)]
    ones, zeros = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    ref = sum(F.conv3d(x[:, i * cs:(i + 1) * cs].double(), ws[i].double(), padding=1) for i in range(2))
    mag = sum(F.conv3d(x[:, i * cs:(i + 1) * cs].double().abs(), ws[i].double().abs(), padding=1) for i in range(2))
    with ra.ops.conv_precision("f16x3"):
        assert ra.ops.conv3d_k3_uses_x3(2 * cs, cout, B, D, H, W, nset=2)
        pk = [ra.ops.conv3d_k3_pack(gpu(w)) for w in ws]
        for _ in range(3):       # the window is timing dependent: a few launches
            out = ra.ops.conv3d_k3_dual(gpu(x), cs, pk[0], ones, zeros, pk[1], ones, zeros, cout, False,
                                        torch.empty((B, cout, D, H, W), device=DEV)).cpu().double()
            assert torch.isfinite(out).all()
            assert float(((out - ref).abs() / mag.clamp_min(1e-30)).max()) <= 2e-5
        # (b) one Inf; the voxels at distance 2 along x (either side) have it outside their window
        xi = x.clone()
        xi[0, 3, 7, 13, 50] = float("inf")
        out = ra.ops.conv3d_k3_dual(gpu(xi), cs, pk[0], ones, zeros, pk[1], ones, zeros, cout, False,
                                    torch.empty((B, cout, D, H, W), device=DEV)).cpu().double()
    assert not torch.isfinite(out[0, :, 6:9, 12:15, 49:52]).all()
    ring = out[0, :, 5:10, 11:16, 47:54].clone()
    ring_ref = ref[0, :, 5:10, 11:16, 47:54]
    inner = torch.zeros(ring.shape[1:], dtype=torch.bool)
    inner[1:4, 1:4, 2:5] = True
    assert torch.isfinite(ring[:, ~inner]).all(), "an Inf leaked beyond its 3x3x3 reach"
    np.testing.assert_allclose(ring[:, ~inner].numpy(), ring_ref[:, ~inner].numpy(), rtol=2e-4, atol=2e-3)


def test_partial_pack_is_poisoned_for_other_contracts(ra):
    """conv3d_k3_pack(for_current_precision=True) under "fp32" fills only the fp32-MFMA section; consumed under the
    split contract it now returns NaN everywhere (poisoned fragments / multipliers) instead of products of uninitialised memory."""
    cin, cout, D, H, W = 12, 12, 64, 64, 128
    x = torch.randn((1, cin, D, H, W), generator=gen(187))
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen(188)) * 0.1
    with ra.ops.conv_precision("fp32"):
        pk = ra.ops.conv3d_k3_pack(gpu(w), for_current_precision=True)
        good = ra.ops.conv3d_k3(gpu(x), pk, cout, None, None, False, torch.empty((1, cout, D, H, W), device=DEV))
    assert torch.isfinite(good).all()
    with ra.ops.conv_precision("f16x3"):
        assert ra.ops.conv3d_k3_uses_x3(cin, cout, 1, D, H, W)
        bad = ra.ops.conv3d_k3(gpu(x), pk, cout, None, None, False, torch.empty((1, cout, D, H, W), device=DEV))
    assert torch.isnan(bad).all()


def test_x3_bf16_storage(ra):
    """bf16 activation storage on the f16x3 kernel: the activations are exact bf16 operands, only the weights are split (2 MFMAs)."""
    B, cin, cout, D, H, W = 2, 12, 12, 32, 128, 130
    x = torch.randn((B, cin, D, H, W), generator=gen(151)).to(torch.bfloat16)
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen(152)) * 0.1
    assert ra.ops.conv3d_k3_uses_x3(cin, cout, B, D, H, W, dtype=torch.bfloat16)
    out = torch.empty((B, cout, D, H, W), device=DEV, dtype=torch.bfloat16)
    ra.ops.conv3d_k3(gpu(x), ra.ops.conv3d_k3_pack(gpu(w)), cout, None, None, True, out)
    ref = F.relu(F.conv3d(x[:1, :, :8].float(), w, padding=1))
    got = out[:1, :, :8].float().cpu()
    # interior planes only (the reference slab has its own z border at plane 7)
    np.testing.assert_allclose(got[:, :, :7].numpy(), ref[:, :, :7].numpy(), rtol=1e-2, atol=1e-2)


# --------------------------------------------------------------------------- G4: channel-group-interleaved level-3 tensors (round 5)
@pytest.mark.parametrize("shape,ntail", [((1, 16, 128, 128), 2), ((2, 16, 136, 132), 1), ((1, 24, 128, 96), 0)])
def test_x3_dual_g4_input_and_tails_bitwise(ra, x3_on, shape, ntail):
    """The level-3 dual launch (conv3d_x3q.hip) reading a G4 input and writing G4 tails against the same launch on channel planes:
    the arithmetic is the same instruction stream (only the loads / stores differ), so every bit must agree — and the plane run is
    itself checked against float64 (rag_model.py:160-172 via operations_3d.py:31-47)."""
    B, D, H, W = shape
    C, cout = 4, 12
    g1 = gen(501)
    x = torch.randn((B, 2 * C, D, H, W), generator=g1)
    wa, wb = (torch.randn((cout, C, 3, 3, 3), generator=g1) * 0.2 for _ in range(2))
    sa, sb = (torch.rand(cout, generator=g1) + 0.5 for _ in range(2))
    ha, hb = (torch.randn(cout, generator=g1) * 0.1 for _ in range(2))
    tw = [torch.randn((4, cout), generator=g1) * 0.3 for _ in range(ntail)]
    ts = [torch.rand(4, generator=g1) + 0.5 for _ in range(ntail)]
    th = [torch.randn(4, generator=g1) * 0.1 for _ in range(ntail)]
    with ra.ops.conv_precision("f16x3"):
        caps = ra.ops.conv3d_k3_g4_caps(2 * C, cout, B, D, H, W, nset=2, ntail=ntail)
        assert caps == 3, caps
        pa, pb = ra.ops.conv3d_k3_pack(gpu(wa)), ra.ops.conv3d_k3_pack(gpu(wb))
        outs = {}
        for g4 in (False, True):
            xin = ra.ops.to_g4(gpu(x)) if g4 else gpu(x)
            pre = torch.full((B, 8, D, H, W), float("nan"), device=DEV)
            tails = [ra.ops.Tail(gpu(tw[k]), gpu(ts[k]), gpu(th[k]), k == 0, pre, 4 * k, g4=g4) for k in range(ntail)]
            y = torch.full((B, cout, D, H, W), float("nan"), device=DEV)
            ra.ops.conv3d_k3_dual(xin, C, pa, gpu(sa), gpu(ha), pb, gpu(sb), gpu(hb), cout, True, y, tails=tails or None, x_g4=g4)
            outs[g4] = (y, ra.ops.from_g4(pre) if g4 else pre)
    assert torch.equal(outs[True][0], outs[False][0])
    for k in range(ntail):
        assert torch.equal(outs[True][1][:, 4 * k:4 * k + 4], outs[False][1][:, 4 * k:4 * k + 4])
    v = lambda t: t.view(1, -1, 1, 1, 1)  # noqa: E731
    main = sum(F.relu(F.conv3d(x[:, i * C:(i + 1) * C].double(), w.double(), padding=1) * v(s.double()) + v(h.double()))
               for i, (w, s, h) in enumerate(((wa, sa, ha), (wb, sb, hb))))
    np.testing.assert_allclose(outs[True][0].cpu().double().numpy(), main.numpy(), rtol=2e-4, atol=2e-4)
    for k in range(ntail):
        ref = torch.einsum("oc,bcdhw->bodhw", tw[k].double(), main) * v(ts[k].double()) + v(th[k].double())
        ref = F.relu(ref) if k == 0 else ref
        np.testing.assert_allclose(outs[True][1][:, 4 * k:4 * k + 4].cpu().double().numpy(), ref.numpy(), rtol=3e-4, atol=3e-4)


def test_x3_stem1_g4_input_and_tails_bitwise(ra, x3_on):
    """stem3d1's launch shape (12 -> 12, two fused tails, no main store: rag_model.py:235,341-343) on a G4 input with G4 tails against
    the plane form: bit-identical."""
    B, D, H, W = 1, 16, 128, 160
    g1 = gen(511)
    x = torch.randn((B, 12, D, H, W), generator=g1)
    w = torch.randn((12, 12, 3, 3, 3), generator=g1) * 0.1
    sc, sh = torch.rand(12, generator=g1) + 0.5, torch.randn(12, generator=g1) * 0.1
    tw = [torch.randn((4, 12), generator=g1) * 0.3 for _ in range(2)]
    with ra.ops.conv_precision("f16x3"):
        assert ra.ops.conv3d_k3_g4_caps(12, 12, B, D, H, W, nset=1, ntail=2) == 3
        pk = ra.ops.conv3d_k3_pack(gpu(w))
        outs = {}
        for g4 in (False, True):
            xin = ra.ops.to_g4(gpu(x)) if g4 else gpu(x)
            pre = torch.full((B, 8, D, H, W), float("nan"), device=DEV)
            tails = [ra.ops.Tail(gpu(tw[k]), None, None, True, pre, 4 * k, g4=g4) for k in range(2)]
            y = torch.empty((B, 12, D, H, W), device=DEV)
            ra.ops.conv3d_k3(xin, pk, 12, gpu(sc), gpu(sh), True, y, None, tails=tails, store_main=False, x_g4=g4)
            outs[g4] = ra.ops.from_g4(pre) if g4 else pre
    assert torch.equal(outs[True], outs[False])
    v = lambda t: t.view(1, -1, 1, 1, 1)  # noqa: E731
    main = F.relu(F.conv3d(x.double(), w.double(), padding=1) * v(sc.double()) + v(sh.double()))
    for k in range(2):
        ref = F.relu(torch.einsum("oc,bcdhw->bodhw", tw[k].double(), main))
        np.testing.assert_allclose(outs[True][:, 4 * k:4 * k + 4].cpu().double().numpy(), ref.numpy(), rtol=3e-4, atol=3e-4)


def test_costvol_stem_g4_output_and_tail_bitwise(ra):
    """stem3d0 folded with the cost volume writing a G4 output and a G4 tail against the plane form (rag_model.py:375-383, 234, 341)."""
    B, C, h, w, maxdisp = 2, 12, 6, 40, 24
    L, R = torch.randn((B, C, h, w), generator=gen(521)), torch.randn((B, C, h, w), generator=gen(522))
    wt = torch.randn((12, 24, 3, 3, 3), generator=gen(523)) * 0.1
    w1 = torch.randn((4, 12), generator=gen(524)) * 0.3
    s1, h1 = torch.rand(4, generator=gen(525)) + 0.5, torch.randn(4, generator=gen(526)) * 0.1
    var = ra.ops.costvol_stem_prepare(gpu(wt))
    outs = {}
    for g4 in (False, True):
        pre = torch.full((B, 8, maxdisp // 3, h, w), float("nan"), device=DEV)
        tails = [ra.ops.Tail(gpu(w1), gpu(s1), gpu(h1), True, pre, 4, g4=g4)]
        out = ra.ops.costvol_stem(gpu(L), gpu(R), maxdisp, var, 12, None, None, True, tails=tails, out_g4=g4)
        outs[g4] = (ra.ops.from_g4(out), ra.ops.from_g4(pre)) if g4 else (out, pre)
    assert torch.equal(outs[True][0], outs[False][0])
    assert torch.equal(outs[True][1][:, 4:8], outs[False][1][:, 4:8])
    assert torch.isnan(outs[True][1][:, 0:4]).all()


def test_g4_is_refused_where_the_kernel_does_not_take_it(ra):
    """A call that lands on a kernel without the G4 forms fails loudly (RAGMI_EUNSUPPORTED), never reads planes as groups."""
    x = torch.randn((1, 8, 8, 16, 32), generator=gen(531))
    w = torch.randn((8, 8, 3, 3, 3), generator=gen(532)) * 0.1
    with ra.ops.conv_precision("fp32"):
        assert ra.ops.conv3d_k3_g4_caps(8, 8, 1, 8, 16, 32) == 0
        pk = ra.ops.conv3d_k3_pack(gpu(w))
        with pytest.raises(RuntimeError):
            ra.ops.conv3d_k3(gpu(x), pk, 8, None, None, True, torch.empty((1, 8, 8, 16, 32), device=DEV), x_g4=True)


@pytest.mark.parametrize("hwd", [(384, 1248, 192), (192, 384, 96)])
def test_matchingnet_g4_plan_and_bitwise(ra, x3_on, hwd):
    """The fused executor with its private level-3 tensors channel-group-interleaved (round 5) against the same forward on channel
    planes, and with stem3d0 + stem3d1 as one call that never writes stem3d0's output against the two separate launches: same kernels,
    same arithmetic, other loads and stores — the disparity maps agree bit for bit; and the plan really is G4 for stem3d0's output and
    the three level-3 cells, with the stems fused, at the headline shape (rag_model.py:341-351)."""
    H, W, D = hwd
    rows = O.ALL_CONV
    sd = O.random_matching_state_dict(rows, seed=0)
    net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=D)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    lf, rf = torch.randn((2, 12, H // 3, W // 3), generator=gen(541)), torch.randn((2, 12, H // 3, W // 3), generator=gen(542))
    outs = {}
    try:
        ra.ops.set_stem_tail_rows(False)
        for g4, fuse in ((True, True), (True, False), (False, False), (False, True)):
            ra.ops.set_g4(g4)
            ra.ops.set_stem_fusion(fuse)
            with torch.no_grad():
                outs[(g4, fuse)] = net(gpu(lf), gpu(rf))
            plan = net.last_g4_plan
            assert plan["stem0_out"] == g4 and [plan["pre"][j] for j in (0, 1, 2)] == [g4] * 3 and plan["stems_fused"] == fuse, plan
            assert not any(plan["pre"][j] for j in range(3, 8)) and not plan.get("stem_tail_rows", False)
        # the default: stems fused with cell 0's pre_preprocess in the idle rows of stem3d1's matrix product — split-operand products
        # instead of an exact fp32 chain for that one 1x1x1 conv: not the same bits, the same disparities to the RAGMI_F32X3 class
        ra.ops.set_g4(True)
        ra.ops.set_stem_fusion(True)
        ra.ops.set_stem_tail_rows(True)
        with torch.no_grad():
            d_rows = net(gpu(lf), gpu(rf))
            d_again = net(gpu(lf), gpu(rf))
        assert net.last_g4_plan["stems_fused"] and net.last_g4_plan["stem_tail_rows"]
    finally:
        ra.ops.set_g4(True)
        ra.ops.set_stem_fusion(True)
        ra.ops.set_stem_tail_rows(True)
    for k in outs:       # G4 or planes, stems fused or not: the same bits
        assert torch.equal(outs[k], outs[(False, False)]), k
    assert torch.equal(d_rows, d_again)
    e = O.epe(d_rows.cpu(), outs[(False, False)].cpu())
    print(f"stem tail in the matrix product's idle rows vs the exact chain: EPE {e:.3e} px")
    assert e <= EPE_GATE / 2, e


def test_matchingnet_g4_plan_bf16_storage_bitwise(ra):
    """The G4 layout of the private level-3 tensors under bf16 activation storage (round 5: four bf16 of a voxel and group = one 8-byte
    access; the level-3 dual cells on conv3d_x3_kernel<bf16, 2, 2, *, XSRC = 1>): the same bits as channel planes, with the stems fused
    and not, and the plan says G4 for stem3d0's output and the three level-3 cells (the deep cells are fp32 planes: mixed storage)."""
    rows = O.ALL_CONV
    sd = O.random_matching_state_dict(rows, seed=0)
    net = ra.MatchingNet(ra.Genotype(rows, None, rows, None), maxdisp=96)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    lf, rf = torch.randn((2, 12, 72, 132), generator=gen(581)).to(BF), torch.randn((2, 12, 72, 132), generator=gen(582)).to(BF)
    outs = {}
    try:
        ra.ops.set_stem_tail_rows(False)
        for g4, fuse in ((True, True), (True, False), (False, False), (False, True)):
            ra.ops.set_g4(g4)
            ra.ops.set_stem_fusion(fuse)
            with torch.no_grad():
                outs[(g4, fuse)] = net(gpu(lf), gpu(rf))
            plan = net.last_g4_plan
            assert [plan["pre"][j] for j in (0, 1, 2)] == [g4] * 3 and plan["stems_fused"] == fuse, plan
            assert not any(plan["pre"][j] for j in range(3, 8))
        ra.ops.set_g4(True)
        ra.ops.set_stem_fusion(True)
        ra.ops.set_stem_tail_rows(True)
        with torch.no_grad():
            d_rows = net(gpu(lf), gpu(rf))
            d32 = net(gpu(lf).float(), gpu(rf).float())
    finally:
        ra.ops.set_g4(True)
        ra.ops.set_stem_fusion(True)
        ra.ops.set_stem_tail_rows(True)
    for k in outs:
        assert torch.equal(outs[k], outs[(False, False)]), k
    e_rows, e_ref = O.epe(d_rows.cpu(), d32.cpu()), O.epe(outs[(False, False)].cpu(), d32.cpu())
    print(f"bf16 storage vs the fp32 build: EPE {e_ref:.3e} px; with stem3d0's tail in the product's idle rows {e_rows:.3e} px")
    assert e_rows <= 1.5 * e_ref + 1e-3


def test_x3_down_tail_clamped_pair_ignores_a_non_finite_even_source(ra, x3_on):
    """Where the last output of an axis clamps, the x0.5 trilinear resample (align_corners=True, rag_model.py:146-150) reads the ODD source
    for both taps: a non-finite value in the even source next to it must not reach that output (0 * Inf = NaN).  D = 16:
    output plane 7 reads source plane 15 twice; an Inf in input plane 13 makes the producer's planes 12..14 non-finite and leaves 15 alone."""
    B, D, H, W = 1, 16, 128, 128
    C, cout = 4, 12
    g1 = gen(551)
    x = torch.randn((B, 2 * C, D, H, W), generator=g1)
    x[0, 1, 13, 40, 50] = float("inf")
    wa, wb = (torch.randn((cout, C, 3, 3, 3), generator=g1) * 0.2 for _ in range(2))
    tw = torch.randn((8, cout), generator=g1) * 0.3
    out = torch.full((B, 8, D // 2, H // 2, W // 2), float("nan"), device=DEV)
    gw = gpu(tw)
    tails = [ra.ops.Tail(gw[c0:c0 + 4], None, None, False, out, c0, down=True) for c0 in (0, 4)]
    y = torch.empty((B, cout, D, H, W), device=DEV)
    with ra.ops.conv_precision("f16x3"):
        # (no ReLU: max(NaN, 0) = 0 would hide the non-finite planes the test needs)
        ra.ops.conv3d_k3_dual(gpu(x), C, ra.ops.conv3d_k3_pack(gpu(wa)), None, None, ra.ops.conv3d_k3_pack(gpu(wb)), None, None, cout, False, y, tails=tails)
    yc = y.cpu()
    assert not torch.isfinite(yc[0, :, 14, 40, 50]).all() and torch.isfinite(yc[0, :, 15]).all()
    got = out.cpu()
    assert torch.isfinite(got[:, :, 7]).all()                      # the clamped plane: odd source only
    assert not torch.isfinite(got[:, :, 6, 20, 25]).all()          # the plane below reads (12, 13): non-finite, as in the reference
    main = F.conv3d(x[:, :C], wa, padding=1) + F.conv3d(x[:, C:], wb, padding=1)
    ref = torch.einsum("oc,bcdhw->bodhw", tw, F.interpolate(main[:, :, 15:16], (1, H // 2, W // 2), mode="trilinear", align_corners=True))
    ref = torch.cat([torch.zeros_like(ref)] * 7 + [ref], dim=2)      # (plane 7 = source plane 15 alone; planes 0..6 are not compared)
    np.testing.assert_allclose(got[:, :, 7].numpy(), ref[:, :, 7].numpy(), rtol=3e-4, atol=3e-4)


@pytest.mark.parametrize("B,h,w,maxdisp", [(1, 128, 160, 48), (2, 72, 132, 96), (1, 131, 171, 51)])      # (the last: ragged tiles, D = 17)
def test_costvol_stem_conv3d_fused_bitwise(ra, x3_on, B, h, w, maxdisp):
    """stem3d0 + stem3d1 as one call that never writes stem3d0's output (ragmi_costvol_stem_conv3d_fwd; rag_model.py:234-235, 341-343,
    375-383) against the two separate calls (costvol_stem -> conv3d_k3 with the same tails): stem3d1's staging evaluates the combine
    kernel's arithmetic, so the fused tails AND stem3d1's own output agree bit for bit; the separate path is itself checked against
    ATen in float64."""
    C, cmid, cout = 12, 12, 12
    g1 = gen(561)
    L, R = torch.randn((B, C, h, w), generator=g1), torch.randn((B, C, h, w), generator=g1)
    w0 = torch.randn((cmid, 2 * C, 3, 3, 3), generator=g1) * 0.05
    w1 = torch.randn((cout, cmid, 3, 3, 3), generator=g1) * 0.1
    s0, h0 = torch.rand(cmid, generator=g1) + 0.5, torch.randn(cmid, generator=g1) * 0.1
    s1, h1 = torch.rand(cout, generator=g1) + 0.5, torch.randn(cout, generator=g1) * 0.1
    tw0 = torch.randn((4, cmid), generator=g1) * 0.3
    tw1 = [torch.randn((4, cout), generator=g1) * 0.3 for _ in range(2)]
    d = maxdisp // 3
    with ra.ops.conv_precision("f16x3"):
        assert ra.ops.costvol_stem_conv3d_supported(C, cmid, cout, B, d, h, w, ntail=2)
        var = ra.ops.costvol_stem_prepare(gpu(w0))
        pk = ra.ops.conv3d_k3_pack(gpu(w1))
        outs = {}
        for fused in (False, True, "again", "once more"):      # (repeats: the fused tail once differed from run to run, NOTES.md round 5)
            pre0 = torch.full((B, 8, d, h, w), float("nan"), device=DEV)
            pre1 = torch.full((B, 8, d, h, w), float("nan"), device=DEV)
            t0 = [ra.ops.Tail(gpu(tw0), None, None, True, pre0, 0, g4=True)]
            t1 = [ra.ops.Tail(gpu(tw1[0]), None, None, True, pre0, 4, g4=True), ra.ops.Tail(gpu(tw1[1]), None, None, False, pre1, 0, g4=True)]
            y = torch.full((B, cout, d, h, w), float("nan"), device=DEV)
            if fused:
                ra.ops.costvol_stem_conv3d(gpu(L), gpu(R), maxdisp, var, cmid, gpu(s0), gpu(h0), True, t0, pk, cout, gpu(s1), gpu(h1), True, y,
                                           None, tails=t1, store_main=True)
            else:
                mid = ra.ops.costvol_stem(gpu(L), gpu(R), maxdisp, var, cmid, gpu(s0), gpu(h0), True, tails=t0, out_g4=True)
                ra.ops.conv3d_k3(mid, pk, cout, gpu(s1), gpu(h1), True, y, None, tails=t1, x_g4=True)
            outs[fused] = (y, ra.ops.from_g4(pre0), ra.ops.from_g4(pre1))
    for run in (True, "again", "once more"):
        for a_, b_ in zip(outs[run], outs[False]):
            assert torch.equal(torch.nan_to_num(a_, nan=-7.0), torch.nan_to_num(b_, nan=-7.0))
    # RAGMI_TAIL_ROWS: stem3d0's tail in rows 12..15 of stem3d1's matrix product (stem3d1's weight packed as 16 channels): stem3d1's
    # output and its own tails keep their bits; that one tail is a split-operand product now (the RAGMI_F32X3 class), run to run the same
    with ra.ops.conv_precision("f16x3"):
        pk16 = ra.ops.conv3d_k3_pack(ra.ops.stem_tail_rows_weight(gpu(w1), gpu(tw0)))
        rows_runs = []
        for _ in range(2):
            pre0 = torch.full((B, 8, d, h, w), float("nan"), device=DEV)
            pre1 = torch.full((B, 8, d, h, w), float("nan"), device=DEV)
            t0 = [ra.ops.Tail(gpu(tw0), None, None, True, pre0, 0, g4=True)]
            t1 = [ra.ops.Tail(gpu(tw1[0]), None, None, True, pre0, 4, g4=True), ra.ops.Tail(gpu(tw1[1]), None, None, False, pre1, 0, g4=True)]
            y = torch.full((B, cout, d, h, w), float("nan"), device=DEV)
            ra.ops.costvol_stem_conv3d(gpu(L), gpu(R), maxdisp, var, cmid, gpu(s0), gpu(h0), True, t0, pk16, cout, gpu(s1), gpu(h1), True, y,
                                       None, tails=t1, store_main=True, tail0_rows=True)
            rows_runs.append((y, ra.ops.from_g4(pre0), ra.ops.from_g4(pre1)))
    for a_, b_ in zip(rows_runs[0], rows_runs[1]):
        assert torch.equal(torch.nan_to_num(a_, nan=-7.0), torch.nan_to_num(b_, nan=-7.0))
    assert torch.isnan(rows_runs[0][2][:, 4:]).all() and not torch.isnan(rows_runs[0][1]).any()
    assert torch.equal(rows_runs[0][0], outs[False][0]) and torch.equal(rows_runs[0][2][:, :4], outs[False][2][:, :4])
    assert torch.equal(rows_runs[0][1][:, 4:], outs[False][1][:, 4:])
    np.testing.assert_allclose(rows_runs[0][1][:, :4].cpu().numpy(), outs[False][1][:, :4].cpu().numpy(), rtol=2e-6, atol=5e-6)
    assert torch.isnan(outs[True][2][:, 4:]).all() and not torch.isnan(outs[True][1]).any()
    v = lambda t: t.view(1, -1, 1, 1, 1)  # noqa: E731
    torch.set_num_threads(16)
    mid = F.relu(F.conv3d(O.cost_volume(L, R, maxdisp).double(), w0.double(), padding=1) * v(s0.double()) + v(h0.double()))
    ref = F.relu(F.conv3d(mid, w1.double(), padding=1) * v(s1.double()) + v(h1.double()))
    np.testing.assert_allclose(outs[True][0].cpu().double().numpy(), ref.numpy(), rtol=3e-4, atol=3e-4)
    np.testing.assert_allclose(outs[True][1][:, 0:4].cpu().double().numpy(), F.relu(torch.einsum("oc,bcdhw->bodhw", tw0.double(), mid)).numpy(), rtol=3e-4, atol=3e-4)
