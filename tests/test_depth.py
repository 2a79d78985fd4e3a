"""The monocular-depth network of rag_depth (models/rag_model.py:201-800): the fused HIP depth head (rag_amd/csrc/depth_head.hip),
the fused loss + metrics (rag_amd/csrc/depth_metrics.hip), `rag_amd.depth.Network` on the shipped trained weights, the checkpoint
loader and the growth API, against the REFERENCE's own numbers (g14-g18; generator tests/golden/make_golden_depth.py) and the
plain-torch restatements (rag_amd.depth.depth_head_torch / depth_metrics_torch).

Unmarked tests run without a GPU; the rest need the MI355X."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

DEV = "cuda:0"
HEAD_CASES = (0, 1, 2, 3)
# unit counts of the shipped task-3 checkpoint
TASK3_COUNTS = {"stem_2d0": 3, "stem_2d1": 3, "stem_2d2": 3, "last_3_2d": 3, "stem_3d0": 2, "stem_3d1": 3,
                "last_3_3d": 4, "last_6_3d": 4, "last_12_3d": 4}


def _json(a):
    return json.loads(bytes(a).decode())


def _sd():
    return {k: torch.as_tensor(v) for k, v in load_golden("g14_depth_ckpt_task3").items()}


def _head_case(k):
    g = load_golden("g16_depth_head")
    return [torch.as_tensor(g[f"case{k}_{n}"]) for n in ("y", "w3", "w1", "b1")] + [tuple(int(v) for v in g[f"case{k}_hw"]),
                                                                                     torch.as_tensor(g[f"case{k}_out"]),
                                                                                     torch.as_tensor(g[f"case{k}_out64"])]


# --------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("k", HEAD_CASES)
def test_depth_head_torch_matches_reference(k):
    from rag_amd.depth import depth_head_torch
    y, w3, w1, b1, hw, ref, ref64 = _head_case(k)
    out = depth_head_torch(y, w3, w1, b1, hw, 3, 80.0)
    out64 = depth_head_torch(y.double(), w3.double(), w1.double(), b1.double(), hw, 3, 80.0)
    assert float((out64 - ref64.double()).abs().max()) <= 1e-5          # ref64 is stored rounded to fp32
    assert out.shape == ref.shape == (y.shape[0], 3 * hw[0], 3 * hw[1])
    assert float((out - ref).abs().max()) <= 1e-4


def test_depth_metrics_torch_matches_reference():
    from rag_amd.depth import depth_metrics_torch
    g = load_golden("g17_depth_metrics")
    out = depth_metrics_torch(torch.as_tensor(g["est"]), torch.as_tensor(g["gt"]))
    np.testing.assert_allclose(out.numpy(), g["out"], rtol=1e-5, atol=1e-6)


def test_load_depth_checkpoint_from_keys():
    from rag_amd.depth import Network, load_depth_checkpoint
    import rag_amd
    assert rag_amd.DepthNetwork is Network
    sd = _sd()
    net, archis = load_depth_checkpoint({"model": sd}, "cpu", "from_keys")
    assert not net.training and archis == [net.arch_init]
    for name, n in TASK3_COUNTS.items():
        assert len(net._units(name)) == n, name
    for name in [f"cell_2d{i}" for i in range(4)] + [f"cell_3d{i}" for i in range(8)]:
        assert 1 <= len(net._units(name)) <= 4
    assert set(net.state_dict().keys()) == set(sd.keys())
    assert net.max_depth == 80 and tuple(net.depth_head.conv1.weight.shape) == (1, 1, 3, 3)
    assert net.depth_head.conv1.bias is not None
    assert tuple(net.stem3d0[0].conv.weight.shape) == (12, 12, 3, 3)
    # the stand-in rows are the generator's
    rows = _json(load_golden("g15_depth_forward")["rows"])
    from rag_amd.depth import genotypes_from_keys
    got = genotypes_from_keys(sd.keys())
    assert {k: [r.tolist() for r in v] for k, v in got.items()} == rows


def test_load_depth_checkpoint_wrong_genotype_raises():
    from rag_amd.depth import load_depth_checkpoint
    from rag_amd.modules import ALL_CONV_ROWS
    sd = _sd()
    rows = _json(load_golden("g15_depth_forward")["rows"])
    rows["cell_3d2"][0] = ALL_CONV_ROWS.tolist()         # no unit in the checkpoint is all-conv
    with pytest.raises(ValueError):
        load_depth_checkpoint({"model": sd}, "cpu", rows)
    with pytest.raises(ValueError):
        load_depth_checkpoint({"model": sd}, "cpu", None)
    ok, _ = load_depth_checkpoint({"model": sd}, "cpu", _json(load_golden("g15_depth_forward")["rows"]))
    with pytest.raises(ValueError):
        load_depth_checkpoint({"model": sd}, "cpu", "from_keys", archis=[{"stem_3d0": [5]}])


def test_depth_growth_api_matches_reference():
    from rag_amd.depth import Network
    from rag_amd.modules import Genotype
    blob = _json(load_golden("g18_depth_growth_api")["blob"])
    geno = lambda r: Genotype(normal=np.array(r), normal_concat=None, reduce=np.array(r), reduce_concat=None)  # noqa: E731
    shapes = lambda m: [[k, list(v.shape)] for k, v in sorted(m.state_dict().items())]  # noqa: E731
    all_conv = [[0, 1], [1, 1], [2, 1], [3, 1], [5, 1], [6, 1]]
    mixed = [[0, 1], [1, 0], [2, 1], [3, 1], [5, 0], [6, 1]]
    net = Network(geno(all_conv), "cpu")
    assert shapes(net) == blob["shapes_initial"]
    assert {k: list(v) for k, v in net.arch_init.items()} == blob["arch_init"]
    net.expand(1, geno(mixed), "cpu")
    assert shapes(net) == blob["shapes_expanded"]
    assert [[round(float(x), 6) for x in p] for p in net.p] == [[round(x, 6) for x in p] for p in blob["p_after_expand"]]
    assert {k: [int(i) for i in v] for k, v in net.new_models.items()} == blob["new_models"]
    for k, p in enumerate(net.p):
        if k in blob["winners"]:
            p[-1] = 0.9
    best = net.select(1)
    assert {k: [int(i) for i in v] for k, v in best.items()} == blob["best_archi"]
    assert {k: [int(i) for i in v] for k, v in net.model_to_train.items()} == blob["model_to_train"]
    assert {k: int(v) for k, v in net.length.items()} == blob["length"]
    assert shapes(net) == blob["shapes_selected"]
    assert len(net.get_param(net.model_to_train)) > 0


def test_depth_abi_symbols_exported():
    from rag_amd import _lib
    lib = ctypes.CDLL(_lib.lib_path())
    for name in ("ragmi_depth_head_fwd", "ragmi_depth_head_supported", "ragmi_depth_metrics_fwd", "ragmi_depth_metrics_workspace_elems"):
        assert hasattr(lib, name), name
    L = _lib.load_library()
    assert L.ragmi_version() >= 520
    assert L.ragmi_depth_head_supported(12, 8, 16, 16, 32, 3, 0) == 1
    assert L.ragmi_depth_head_supported(12, 8, 16, 16, 32, 3, 1) == 0        # bf16
    assert L.ragmi_depth_head_supported(17, 8, 16, 16, 32, 3, 0) == 0        # Cin > 16
    assert L.ragmi_depth_head_supported(12, 32, 16, 16, 32, 3, 0) == 0       # downsampling
    assert L.ragmi_depth_metrics_workspace_elems(1000) > 0


def test_depth_abi_rejects_bad_arguments_before_launch():
    """Argument checks return a negative status without touching a device (null pointers, bad dtype)."""
    from rag_amd import _lib
    L = _lib.load_library()
    assert L.ragmi_depth_head_fwd(None, None, None, None, None, 1, 12, 8, 16, 16, 32, 3, 80.0, 0, None) < 0
    assert L.ragmi_depth_metrics_fwd(None, None, 10, 0.85, None, None, 0, None) < 0


def test_depth_network_refuses_autograd_on_cpu_side():
    """The depth network is inference only: grad mode with trainable parameters raises before any kernel."""
    from rag_amd.depth import Network
    from rag_amd.modules import ALL_CONV_GENOTYPE
    net = Network(ALL_CONV_GENOTYPE, "cpu").eval()
    with pytest.raises(RuntimeError, match="inference only"):
        net(torch.zeros((1, 3, 36, 48)), None, 0, net.arch_init)


# --------------------------------------------------------------------------- GPU
def gpu(x):
    return torch.as_tensor(x).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("k", HEAD_CASES)
def test_depth_head_kernel_matches_reference(k):
    from rag_amd import ops
    y, w3, w1, b1, hw, ref, ref64 = _head_case(k)
    out = ops.depth_head(gpu(y), gpu(w3), gpu(w1), gpu(b1), hw, 3, 80.0)
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    err = float((out.cpu() - ref).abs().max())        # the fp32 reference: same fp32 source-index arithmetic as the kernel
    print(f"depth head case {k}: max |d| {err:.2e} m vs fp32 reference, {float((out.cpu().double() - ref64.double()).abs().max()):.2e} "
          "vs fp64")
    assert err <= 1e-4, err


@pytest.mark.gpu
def test_depth_head_refuses_bad_arguments():
    from rag_amd import ops
    y, w3, w1, b1, hw, _ref, _ref64 = _head_case(1)
    with pytest.raises(RuntimeError):
        ops.depth_head(gpu(y).bfloat16(), gpu(w3).bfloat16(), gpu(w1).bfloat16(), gpu(b1).bfloat16(), hw, 3, 80.0)
    with pytest.raises(RuntimeError):
        ops.depth_head(gpu(y), gpu(w3), gpu(w1), gpu(b1), (hw[0] // 4, hw[1] // 4), 3, 80.0)     # downsampling: not built
    with pytest.raises(RuntimeError):
        ops.depth_metrics(gpu(torch.ones(8)).bfloat16(), gpu(torch.ones(8)).bfloat16())
    with pytest.raises(RuntimeError):
        ops.depth_head(y, w3, w1, b1, hw, 3, 80.0)                                              # CPU tensors


@pytest.mark.gpu
def test_depth_metrics_kernel_matches_reference_and_is_deterministic():
    from rag_amd.depth import depth_metrics
    g = load_golden("g17_depth_metrics")
    est, gt = gpu(g["est"]), gpu(g["gt"])
    a = depth_metrics(est, gt)
    b = depth_metrics(est, gt)
    np.testing.assert_allclose(a.tensor.cpu().numpy(), g["out"], rtol=1e-5, atol=1e-6)
    assert torch.equal(a.tensor, b.tensor)
    f = a.floats()
    assert set(f) == {"silog_loss", "silog", "abs_rel", "log10", "rms", "sq_rel", "log_rms", "d1", "d2", "d3"}


def _net():
    from rag_amd.depth import load_depth_checkpoint
    return load_depth_checkpoint({"model": _sd()}, DEV, "from_keys")[0]


def _check(out, ref):
    d = (out.detach().cpu().double() - torch.as_tensor(ref).double()).abs()
    assert out.shape == tuple(ref.shape)
    return float(d.mean()), float(d.max())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_depth_network_matches_reference_on_trained_weights(precision):
    """Every archi of g15 and both search_forward cases: mean |d| <= 1e-3 m, max |d| <= 2e-2 m (gates set before measuring)."""
    from rag_amd import ops
    g = load_golden("g15_depth_forward")
    net = _net()
    worst = [0.0, 0.0]
    with ops.conv_precision(precision), torch.no_grad():
        for t in range(4):
            archi = _json(g[f"archi{t}"])
            for i in range(2):
                out = net(gpu(g[f"img{i}"]), None, t, archi)
                mean, mx = _check(out, g[f"out{i}_{t}"])
                worst = [max(worst[0], mean), max(worst[1], mx)]
        for k in range(2):
            sops, t = [int(v) for v in g[f"sops{k}"]], int(g[f"st{k}"])
            for i in range(2):
                out = net.search_forward(gpu(g[f"img{i}"]), None, t, sops)
                mean, mx = _check(out, g[f"sout{k}_{i}"])
                worst = [max(worst[0], mean), max(worst[1], mx)]
    print(f"depth vs reference ({precision}): worst mean |d| {worst[0]:.3e} m, worst max |d| {worst[1]:.3e} m")
    assert worst[0] <= 1e-3 and worst[1] <= 2e-2, worst


@pytest.mark.gpu
def test_depth_matching_and_disphead_compose_to_forward():
    """matching() -> depth_head(., 3) -> x max_depth is forward() (the fused head against the two-step path)."""
    g = load_golden("g15_depth_forward")
    net = _net()
    archi = _json(g["archi2"])
    with torch.no_grad():
        left = gpu(g["img0"])
        mat = net.matching(net.feature(left, archi, None), archi)
        two = net.depth_head(mat, 3)[:, 0] * net.max_depth
        fused = net(left, None, 2, archi)
    assert float((two - fused).abs().max()) <= 1e-3


@pytest.mark.gpu
def test_depth_forward_deterministic_and_graph_capturable():
    from rag_amd.train import graph_census
    g = load_golden("g15_depth_forward")
    net = _net()
    archi = _json(g["archi3"])
    left = gpu(g["img0"])
    with torch.no_grad():
        a = net(left, None, 3, archi)
        b = net(left, None, 3, archi)
        assert torch.equal(a, b)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(left, None, 3, archi)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            out = net(left, None, 3, archi)
        census = graph_census(graph)
        graph.instantiate()
        graph.replay()
        torch.cuda.synchronize()
    assert census["memcpy"] == 0 and census["memset"] == 0, census
    assert census["kernel"] > 0
    assert torch.equal(out, a)


@pytest.mark.gpu
def test_depth_network_refuses_autograd_and_bf16():
    g = load_golden("g15_depth_forward")
    net = _net()
    left = gpu(g["img1"])
    with pytest.raises(RuntimeError, match="inference only"):
        net(left, None, 0, net.arch_init)                 # grad enabled, parameters require grad
    with torch.no_grad():
        net.stem3d0[0].train()
        with pytest.raises(RuntimeError, match="inference only"):
            net(left, None, 0, net.arch_init)             # a BatchNorm in train mode
        net.eval()
        with pytest.raises(RuntimeError, match="fp32 only"):
            net(left.bfloat16(), None, 0, net.arch_init)
