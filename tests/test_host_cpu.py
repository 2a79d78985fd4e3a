"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol the header
declares, the host mirror keeps the reference's interface / state_dict layout, and the
product path refuses to run without the GPU (no silent fallback)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, split_sd
from oracle import matching_oracle as O


@pytest.fixture(scope="session")
def built_lib():
    import rag_amd
    if not os.path.exists(rag_amd.lib_path()):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return rag_amd.load_library()


def test_library_exports_every_declared_symbol(built_lib):
    header = open(os.path.join(ROOT, "include", "rag_amd.h")).read()
    declared = set(re.findall(r"\b(ragmi_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 11
    from rag_amd._lib import SIGNATURES
    assert declared == set(SIGNATURES), declared ^ set(SIGNATURES)
    for name in declared:
        assert hasattr(built_lib, name), name
    assert built_lib.ragmi_version() >= 100
    # fp32-MFMA section (groups x chunks x 7 VGPRs x 64 lanes) + bf16x3 fragments (1 cog x 21 K-slices x hi/lo x 64 lanes x 4 words)
    # fp32-MFMA section | bf16 fragments | scaled fp16 fragments | per-output-channel multipliers (one 16-channel block)
    assert built_lib.ragmi_conv3d_k3_packed_elems(12, 24) == 3 * 6 * 7 * 64 + 2 * (1 * 21 * 2 * 64 * 4) + 16


def test_abi_rejects_bad_arguments_without_gpu(built_lib):
    # argument validation happens before any launch, so it is checkable on CPU
    assert built_lib.ragmi_costvol_fwd(None, None, None, 1, 12, 8, 4, 4, 0, None) == -1
    assert b"null" in built_lib.ragmi_last_error()
    assert built_lib.ragmi_conv3d_k3_pack(None, None, 4, 4, 0, None) == -1


def test_ops_refuse_cpu_tensors(built_lib):
    import rag_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rag_amd.ops.costvol(torch.zeros(1, 12, 4, 4), torch.zeros(1, 12, 4, 4), 24)
    net = rag_amd.MatchingNet(rag_amd.ALL_SKIP_GENOTYPE, 24).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 12, 8, 12), torch.zeros(1, 12, 8, 12))


def test_missing_library_fails_loudly(monkeypatch):
    import rag_amd._lib as L
    monkeypatch.setattr(L, "_LIB", None)
    monkeypatch.setenv("RAG_AMD_LIB", "/nonexistent/librag_amd.so")
    with pytest.raises(RuntimeError, match="HIP library not found"):
        L.load_library()


def test_product_path_never_imports_oracle():
    pkg = os.path.join(ROOT, "rag_amd")
    for dirpath, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("no oracle", ""), f"{f} mentions the oracle"


@pytest.mark.parametrize("fixture", ["g5_forward_conv_48x96_d48", "g5_forward_unsorted_36x60_d24", "g5_forward_skip_48x72_d24"])
def test_state_dict_layout_matches_reference(fixture):
    """Matching-Net keys and shapes of rag_amd.MatchingNet == the reference Network's (checkpoint drop-in)."""
    import rag_amd
    g = load_golden(fixture)
    rows = g["rows"]
    ref = {k: tuple(v.shape) for k, v in split_sd(g).items()
           if k.split(".")[0] in ("stem3d0", "stem3d1", "cells_3d", "last_3_3d", "last_6_3d", "last_12_3d")}
    net = rag_amd.MatchingNet(rag_amd.Genotype(rows, None, rows, None), maxdisp=int(g["maxdisp"]))
    mine = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert mine == ref
    net.load_state_dict({k: v for k, v in split_sd(g).items() if k in ref}, strict=True)


@pytest.mark.parametrize("rows", [O.ALL_CONV, O.ALL_SKIP, np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]]),
                                  np.array([[1, 1], [0, 0], [4, 1], [2, 0], [7, 1], [8, 1]])])
def test_cell_positional_op_pairing_matches_oracle(rows):
    import rag_amd
    cell = rag_amd.Cell_3d(3, 3, 4, 4, rag_amd.Genotype(rows, None, rows, None), 4, 0)
    plan = O.resolve_cell_ops(rows)
    contribs = cell._contributions()
    for step, lst in enumerate(plan):
        mine = contribs[2 + step]
        assert [j for (j, _k, _t) in lst] == [j for (j, _op) in mine]
        for (j, k, op_type), (_j, op) in zip(lst, mine):
            assert op is cell._ops[k]
            assert isinstance(op, rag_amd.ConvBR_3d) == (op_type == 1)


def test_reference_interface_names():
    import rag_amd
    net = rag_amd.MatchingNet(rag_amd.ALL_CONV_GENOTYPE)
    assert net.maxdisp == 192 and isinstance(net.disp, rag_amd.Disp)
    for attr in ("stem3d0", "stem3d1", "cells_3d", "last_3_3d", "last_6_3d", "last_12_3d", "matching", "search_matching"):
        assert hasattr(net, attr)
    assert set(net.arch_init) == {"stem_3d0", "stem_3d1", "last_3_3d", "last_6_3d", "last_12_3d"} | {f"cell_3d{i}" for i in range(8)}
    c = rag_amd.Cell_3d(3, 3, 4, 8, rag_amd.ALL_CONV_GENOTYPE, 16, -1)
    assert (c.C_in, c.C_out, c.C_prev, c.C_prev_prev, c.scale) == (48, 16, 24, 12, 0.5)
    assert c.scale_dimension(64, 0.5) == 32 and c.scale_dimension(7, 0.5) == 4 and c.scale_dimension(3, 2) == 5
    m = rag_amd.ConvBR_3d(12, 1, 3, 1, 1, bn=False, relu=False)
    assert "bn.weight" in m.state_dict()           # bn constructed even when unused (operations_3d.py:38)
    assert list(rag_amd.OPS_3d) == ["skip_connect_3d", "3d_conv_3x3"] == rag_amd.PRIMITIVES_3D


def test_training_mode_runs_on_hip_or_fails_loudly():
    """Train-mode BN / autograd route to the HIP autograd Functions; on a machine without a GPU they raise
    (no PyTorch emulation), and folded BN parameters are never handed out for a train-mode unit."""
    import rag_amd
    from rag_amd import autograd as ag
    m = rag_amd.ConvBR_3d(4, 4, 3, 1, 1)
    m.train()
    assert m.autograd_mode(torch.zeros(1))                      # batch statistics -> training composition
    with pytest.raises(RuntimeError):
        m.prepared()
    m.eval()
    x = torch.zeros(1, 4, 2, 2, 2, requires_grad=True)
    assert m.autograd_mode(x)
    with torch.no_grad():
        assert not m.autograd_mode(x)
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, OSError)):            # CPU tensor: "rag_amd ops run on the MI355X only"
            m(x)
    for fn in (ag.ConvBRFn, ag.StridedStemFn, ag.TrilinearFn, ag.CostVolFn, ag.DispFn, ag.DispRegFn, ag.AddFn):
        assert issubclass(fn, torch.autograd.Function)


# ------------------------------------------------------------------ Network (growth loop surface)
def _blob():
    import json
    return json.loads(bytes(load_golden("g8_growth_api")["blob"]).decode())


def test_network_state_dict_matches_reference_network():
    """Full-Network keys and shapes (Feature Net + Matching Net) == the reference Network's; strict load."""
    import rag_amd
    g = load_golden("g5_forward_unsorted_36x60_d24")
    rows = g["rows"]
    ref = split_sd(g)
    net = rag_amd.Network(rag_amd.Genotype(rows, None, rows, None), "cpu", maxdisp=int(g["maxdisp"]))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.items()}
    net.load_state_dict(ref, strict=True)
    assert sorted(net.state_dict().keys()) == sorted(ref.keys())


def test_network_growth_api_matches_reference_bookkeeping():
    """expand / get_new_model / select replayed against the reference's own run (tests/golden/make_golden.py G8)."""
    import rag_amd
    blob = _blob()
    mixed = np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]])
    geno = lambda r: rag_amd.Genotype(r, None, r, None)  # noqa: E731
    net = rag_amd.Network(geno(O.ALL_CONV), "cpu")
    assert sorted(net.state_dict().keys()) == blob["keys_initial"]
    assert {k: list(v) for k, v in net.arch_init.items()} == blob["arch_init"]
    net.expand(1, geno(mixed), "cpu")
    assert sorted(net.state_dict().keys()) == blob["keys_expanded"]
    assert [[round(float(x), 6) for x in p] for p in net.p] == [[round(x, 6) for x in p] for p in blob["p_after_expand"]]
    assert {k: [int(i) for i in v] for k, v in net.new_models.items()} == blob["new_models"]
    for k, p in enumerate(net.p):
        if k in blob["winners"]:
            p[-1] = 0.9
    best = net.select(1)
    as_int = lambda d: {k: [int(i) for i in v] for k, v in d.items()}  # noqa: E731
    assert as_int(best) == blob["best_archi"]
    assert as_int(net.model_to_train) == blob["model_to_train"]
    assert {k: int(v) for k, v in net.length.items()} == blob["length"]
    assert sorted(net.state_dict().keys()) == blob["keys_selected"]
    # get_param / modify_param address exactly the units to train
    net.modify_param({k: list(range(net.length[k])) for k in net.length if k in net.new_models}, False)
    net.modify_param(net.model_to_train, True)
    trainable = {n for n, p in net.named_parameters() if p.requires_grad}
    n_params = sum(len(list(g["params"])) for g in net.get_param(net.model_to_train))
    assert n_params == len(trainable) and any(n.startswith("stem2d1.1.") for n in trainable)
    assert all(not n.startswith("stem2d0.") for n in trainable) and any(n.startswith("last_3_3d.1.") for n in trainable)
    net.expand(2, geno(O.ALL_SKIP), "cpu")
    best2 = net.select(2)
    assert as_int(best2) == blob["best_archi_round2"]
    assert {k: int(v) for k, v in net.length.items()} == blob["length_round2"]
    assert sorted(net.state_dict().keys()) == blob["keys_round2"]


# ------------------------------------------------------------------ edge cases / argument validation
def test_abi_rejects_unbuilt_dtype_and_bad_sizes(built_lib):
    """Validation runs before any launch, so it is checkable without a GPU (pointers are never dereferenced)."""
    import ctypes
    fake = ctypes.c_void_p(0x1000)
    # unknown dtype code -> RAGMI_EUNSUPPORTED (-2)
    assert built_lib.ragmi_costvol_fwd(fake, fake, fake, 1, 12, 8, 4, 4, 7, None) == -2
    assert b"dtype" in built_lib.ragmi_last_error()
    assert built_lib.ragmi_trilinear3d_fwd(fake, fake, 1, 1, 2, 2, 2, 4, 4, 4, 1, 9, None) == -2
    # non-positive sizes -> RAGMI_EINVAL (-1)
    assert built_lib.ragmi_costvol_fwd(fake, fake, fake, 0, 12, 8, 4, 4, 0, None) == -1
    assert built_lib.ragmi_conv3d_k1_fwd(fake, 0, fake, None, None, 0, fake, 0, 0, 1, 0, 4, 8, 0, None) == -1
    # scale without shift
    assert built_lib.ragmi_conv3d_k1_fwd(fake, 0, fake, fake, None, 0, fake, 0, 0, 1, 4, 4, 8, 0, None) == -1
    # too many output channels for one call / dual needs CinA % 4 == 0
    assert built_lib.ragmi_conv3d_k3_fwd(fake, 0, fake, None, None, 0, fake, 0, None, None, 0, None, 1, 4, 68, 2, 2, 2, 0, None) == -2
    assert built_lib.ragmi_conv3d_k3_dual_fwd(fake, 0, 3, fake, None, None, 4, fake, None, None, 0, fake, 0, None, None, 0, None,
                                              1, 4, 2, 2, 2, 0, None) == -1
    # small-Cout form only for Cout <= 2
    assert built_lib.ragmi_conv3d_k3_small_fwd(fake, 0, fake, None, None, 0, fake, 0, 0, None, 0, 0, 1, 4, 3, 2, 2, 2, 0, None) == -2


def test_cost_volume_maxdisp_semantics_match_reference():
    """d = int(maxdisp / 3) like rag_model.py:376-377 (maxdisp need not be a multiple of 3); disparities past the width
    stay zero (the reference's slice assignment is empty there)."""
    L, R = torch.randn(1, 2, 3, 4), torch.randn(1, 2, 3, 4)
    assert O.cost_volume(L, R, 25).shape == (1, 4, 8, 3, 4)
    c = O.cost_volume(L, R, 24)
    assert float(c[:, :, 4:].abs().max()) == 0.0 and torch.equal(c[:, :2, 0], L) and torch.equal(c[:, 2:, 1, :, 1:], R[..., :-1])


def test_oracle_rejects_shapes_the_reference_crashes_on():
    rows = O.ALL_SKIP
    sd = O.random_matching_state_dict(rows)
    with pytest.raises(ValueError):     # h = 10 is not a multiple of 4 -> reference: UnboundLocalError at rag_model.py:360-366
        O.matching(torch.zeros(1, 24, 4, 10, 8), sd, rows)


# ------------------------------------------------------------------ checkpoint round trip
def _grown_network():
    import rag_amd
    from rag_amd.modules import Genotype
    mixed = np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]])
    torch.manual_seed(5)
    net = rag_amd.Network(rag_amd.ALL_CONV_GENOTYPE, "cpu", maxdisp=48)
    archis = [net.arch_init]
    net.expand(1, Genotype(mixed, None, mixed, None), "cpu")
    for k in (1, 5, 9, 12):                      # the candidate wins in four layers
        net.p[k][-1] = 0.9
    archis.append(net.select(1))
    return net, archis


def test_checkpoint_round_trip_rebuilds_grown_model(tmp_path):
    from rag_amd import checkpoint as ck
    net, archis = _grown_network()
    path = tmp_path / "checkpoint_task1.ckpt"
    ck.save_checkpoint(path, net, archis, task=1)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert {"task", "model", "optimizer"} <= set(raw)                      # the reference's keys (run.py:194) are intact
    net2, archis2 = ck.load_checkpoint(str(path), device="cpu")
    sd1, sd2 = net.state_dict(), net2.state_dict()
    assert list(sd1) == list(sd2)
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    assert archis2 == [{k: [int(v) for v in vs] for k, vs in a.items()} for a in archis]
    assert net2.length == net.length and not net2.training
    # grown cell units were rebuilt from THEIR genotype (identity ops at the same positions)
    for name in ("cell_3d1", "cell_2d2"):
        for u1, u2 in zip(net._units(name), net2._units(name)):
            assert [type(o).__name__ for o in u1._ops] == [type(o).__name__ for o in u2._ops]
    serve = ck.MultiTaskStereo(net2, archis2)
    assert serve.n_tasks == 2
    with pytest.raises(IndexError):
        serve(None, None, 2)


def test_reference_style_checkpoint_needs_genotypes_and_checks_them():
    import rag_amd
    from rag_amd import checkpoint as ck
    net, archis = _grown_network()
    ref_style = {"task": 1, "model": net.state_dict(), "optimizer": None}       # what run.py:194 writes
    with pytest.raises(ValueError, match="no genotypes"):
        ck.load_checkpoint(ref_style, device="cpu")
    with pytest.raises(ValueError, match="wrong genotype"):                      # all-conv for every unit: the mixed units disagree
        ck.load_checkpoint(ref_style, device="cpu", genotypes=rag_amd.ALL_CONV_GENOTYPE)
    net2, archis2 = ck.load_checkpoint(ref_style, device="cpu", genotypes=ck.unit_genotypes(net), archis=archis)
    assert list(net2.state_dict()) == list(net.state_dict()) and len(archis2) == 2
    bad = [dict(archis[0], stem_3d0=[7])]
    with pytest.raises(ValueError, match="archis"):
        ck.load_checkpoint(ref_style, device="cpu", genotypes=ck.unit_genotypes(net), archis=bad)


# ------------------------------------------------------------------ MdeNAS supernet
def test_supernet_state_dict_matches_reference_and_genotype_parse():
    import rag_amd
    g = load_golden("g9_supernet")
    sd = split_sd(g)
    net = rag_amd.BasicNetwork(device="cpu", maxdisp=48)
    assert sorted(net.state_dict().keys()) == sorted(sd.keys())
    net.load_state_dict(sd, strict=True)
    assert sum(1 for _ in net.parameters()) == int(g["n_params"])
    assert net.matching.cells[0]._ops[0] is None and net.matching.cells[0]._ops[1] is not None      # no s0 edge in the first cell
    assert (net.num_edges, net.num_ops) == (9, 2) and net.p["normal"].shape == (9, 2)
    # genotype(): per step the two edges with the largest non-identity probability, each with its argmax op
    net.p["reduce"] = torch.tensor([[0.9, 0.1], [0.2, 0.8], [0.5, 0.5], [0.1, 0.9], [0.3, 0.7], [0.6, 0.4], [0.4, 0.6], [0.45, 0.55],
                                    [0.2, 0.8]]).log()
    rows = net.genotype().reduce.tolist()
    assert rows == [[1, 1], [0, 0], [3, 1], [4, 1], [8, 1], [6, 1]]
    twin = net.new()                             # mdenas_basicmodel.py:70-74: fresh weights, copied probabilities
    assert torch.equal(twin.p["reduce"], net.p["reduce"]) and twin.p["reduce"] is not net.p["reduce"]


def test_conv_precision_names_and_aliases():
    """"f16x3" is the canonical name of the split form (scaled fp16 halves since round 3); "bf16x3" (round 2's name) and "split"
    are aliases of it; anything else is refused; the context manager restores the previous setting."""
    from rag_amd import ops
    old = ops.get_conv_precision()
    try:
        assert ops.set_conv_precision("fp32") == old
        ops.set_conv_precision("bf16x3")
        assert ops.get_conv_precision() == "f16x3"
        with ops.conv_precision("fp32"):
            assert ops.get_conv_precision() == "fp32"
            with ops.conv_precision("split"):
                assert ops.get_conv_precision() == "f16x3"
            assert ops.get_conv_precision() == "fp32"
        assert ops.get_conv_precision() == "f16x3"
        assert ops.set_conv_precision("f16x3") == "f16x3"
        with pytest.raises(ValueError):
            ops.set_conv_precision("fp16")
    finally:
        ops.set_conv_precision(old)


def test_training_defaults_to_strict_fp32():
    """rag.py:204-216 trains in fp32: forward_backward / train_step / GraphedTrainStep default to the strict contract, the split
    form is opt-in by argument."""
    import inspect
    from rag_amd import train
    assert train.TRAIN_PRECISION == "fp32"
    for fn in (train.forward_backward, train.train_step, train.GraphedTrainStep.__init__):
        assert inspect.signature(fn).parameters["precision"].default is None      # None -> TRAIN_PRECISION


def test_g4_layout_helpers_round_trip():
    import rag_amd
    t = torch.arange(2 * 8 * 3 * 4 * 5, dtype=torch.float32).view(2, 8, 3, 4, 5)
    g = rag_amd.ops.to_g4(t)
    assert g.shape == t.shape and torch.equal(rag_amd.ops.from_g4(g), t)
    # group 1, voxel (d, h, w) = (1, 2, 3): its four channels are contiguous in the buffer
    flat = g.reshape(2, -1)
    base = ((1 * 3 + 1) * 4 + 2) * 5 + 3
    assert torch.equal(flat[0, 4 * base:4 * base + 4], t[0, 4:8, 1, 2, 3])


# ---- the fused executor's plan (rag_amd.modules._plan_chain): decisions only, so it is checked without a GPU.  The expected values are
# the ones the GPU tests assert on the running executor (test_matchingnet_g4_plan_and_bitwise, ..._bf16_storage_bitwise,
# test_matchingnet_mixed_storage_plan).
MIXED_ROWS = np.array([[0, 1], [1, 0], [3, 0], [2, 1], [8, 1], [6, 0]])      # (SURVEY 8 A6's unsorted probe rows, tools/fuzz_fused.py)


def _chain_plan(rows, fea_shape, maxdisp, dtype=torch.float32, folded=True):
    import rag_amd
    from rag_amd.modules import _plan_chain
    net = rag_amd.MatchingNet(rag_amd.Genotype(rows, None, rows, None), maxdisp=maxdisp).eval()
    cells = [c[0] for c in net.cells_3d]
    B, C, h, w = fea_shape
    return cells, _plan_chain(net.stem3d0[0], net.stem3d1[0], cells, B, C if folded else 2 * C, (maxdisp // 3, h, w), dtype, folded)


def _switches(ops, g4=True, fuse=True, rows=True, deep=True):
    ops.set_g4(g4)
    ops.set_stem_fusion(fuse)
    ops.set_stem_tail_rows(rows)
    ops.set_bf16_deep_fp32(deep)


@pytest.mark.parametrize("fea,maxdisp", [((2, 12, 128, 416), 192), ((2, 12, 64, 128), 96)])
def test_chain_plan_g4_and_fused_stems_fp32(built_lib, fea, maxdisp):
    from rag_amd import ops
    try:
        with ops.conv_precision("f16x3"):
            for g4, fuse in ((True, True), (True, False), (False, False), (False, True)):
                _switches(ops, g4, fuse, rows=False)
                _cells, plan = _chain_plan(O.ALL_CONV, fea, maxdisp)
                assert plan.stem0_g4 == g4 and [cp.g4 for cp in plan.cells[:3]] == [g4] * 3, plan
                assert not any(cp.g4 for cp in plan.cells[3:])
                assert plan.stems_fused == fuse and not plan.stem_tail_rows
                assert plan.stored[-2] == (not fuse)
            _switches(ops)
            _cells, plan = _chain_plan(O.ALL_CONV, fea, maxdisp)
            assert plan.stems_fused and plan.stem_tail_rows and plan.stem0_g4
            # the headline's fusion: stem3d1 and cells 0, 1 live only in their consumers' tails; cells 1 / 2 feed cell 3 one level down
            assert [plan.stored[i] for i in range(-2, 3)] == [False, False, False, False, True]
            assert plan.consumers[-2] == ((0, 0, False),) and plan.consumers[-1] == ((0, 1, False), (1, 0, False))
            assert plan.consumers[1] == ((2, 1, False), (3, 0, True)) and plan.consumers[2] == ((3, 1, True),)
            assert set(plan.sizes) == set(plan.cdt) == set(range(-2, 8)) and plan.sizes[-2] == (maxdisp // 3,) + fea[2:]
            # stem3d0 on a materialised cost volume: its output feeds more than tails, nothing of the stems is fused or G4
            _cells, plan = _chain_plan(O.ALL_CONV, fea, maxdisp, folded=False)
            assert not plan.stems_fused and not plan.stem_tail_rows and not plan.stem0_g4 and plan.stored[-2]
    finally:
        _switches(ops)


def test_chain_plan_g4_bf16_storage(built_lib):
    from rag_amd import ops
    try:
        for g4, fuse in ((True, True), (True, False), (False, False), (False, True)):
            _switches(ops, g4, fuse, rows=False)
            _cells, plan = _chain_plan(O.ALL_CONV, (2, 12, 72, 132), 96, torch.bfloat16)
            assert [cp.g4 for cp in plan.cells[:3]] == [g4] * 3 and not any(cp.g4 for cp in plan.cells[3:]), plan
            assert plan.stems_fused == fuse
    finally:
        _switches(ops)


def test_chain_plan_mixed_storage(built_lib):
    """bf16 inputs: the three full-resolution cells bf16, every later cell fp32 (ops.set_bf16_deep_fp32); switched off: every cell bf16."""
    from rag_amd import ops
    bf, f32 = torch.bfloat16, torch.float32
    try:
        _switches(ops)
        _cells, plan = _chain_plan(O.ALL_CONV, (1, 12, 48, 72), 48, bf)
        assert [plan.cdt[i] for i in range(-2, 8)] == [bf] * 5 + [f32] * 5
        assert [cp.dtype for cp in plan.cells] == [bf] * 3 + [f32] * 5
        assert [plan.sizes[i] == (16, 48, 72) for i in range(8)] == [True] * 3 + [False] * 5
        _switches(ops, deep=False)
        _cells, plan = _chain_plan(O.ALL_CONV, (1, 12, 48, 72), 48, bf)
        assert all(plan.cdt[i] == bf for i in range(-2, 8))
        _cells, plan = _chain_plan(O.ALL_CONV, (1, 12, 48, 72), 48, f32)
        assert all(plan.cdt[i] == f32 for i in range(-2, 8))
    finally:
        _switches(ops)


def test_chain_plan_strict_fp32_precision_has_no_g4_and_no_fused_stems(built_lib):
    from rag_amd import ops
    try:
        _switches(ops)
        with ops.conv_precision("fp32"):
            _cells, plan = _chain_plan(O.ALL_CONV, (2, 12, 128, 416), 192)
        assert not plan.stem0_g4 and not any(cp.g4 for cp in plan.cells) and not plan.stems_fused and not plan.stem_tail_rows
    finally:
        _switches(ops)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,any_dual", [(O.ALL_CONV, True), (O.ALL_SKIP, False), (MIXED_ROWS, False)])
def test_chain_plan_dual_cells_by_genotype(built_lib, rows, any_dual, dtype):
    """A cell is one dual launch exactly when both inputs feed conv branches into every new state and nothing else does; only such a
    cell takes tails or a G4 buffer."""
    from rag_amd import ops
    from rag_amd.modules import _ConvBR
    try:
        _switches(ops)
        for fea, maxdisp in (((2, 12, 128, 416), 192), ((1, 12, 48, 72), 48)):
            cells, plan = _chain_plan(rows, fea, maxdisp, dtype)
            assert len(plan.cells) == 8
            for c, cp in zip(cells, plan.cells):
                contribs = c._contributions()
                expect = all([src for src, _op in lst] == [0, 1] and all(isinstance(op, _ConvBR) for _s, op in lst) for lst in contribs.values())
                assert cp.dual == expect == any_dual
                assert cp.dual or not (cp.g4 or cp.tails)
                assert cp.store_main or cp.tails      # a concat nobody stores went to tails
    finally:
        _switches(ops)


# ---- a cell's launches as data (rag_amd.modules._Cell._schedule) and the head's decisions (_plan_head): checked without a GPU.
UNSORTED_ROWS = np.array([[1, 1], [0, 0], [4, 1], [2, 0], [7, 1], [8, 1]])   # (the second unsorted set of the pairing test above)
NAMED_ROWS = {"conv": O.ALL_CONV, "skip": O.ALL_SKIP, "mixed": MIXED_ROWS, "unsorted": UNSORTED_ROWS}


def _cell(rows, steps=3, block_multiplier=3):
    import rag_amd
    return rag_amd.Cell_3d(steps, block_multiplier, 4, 4, rag_amd.Genotype(rows, None, rows, None), 4, 0)


def test_cell_schedule_named_genotypes():
    """The schedules of the four named row sets, written out by hand from the executor's loop (sources in ascending order; a conv takes
    its target's running sum, else an identity partner that is already complete, as its residual; identities left over are added when
    their target is first read and at the end)."""
    from rag_amd.modules import Add, Conv, Dual
    c = _cell(O.ALL_CONV)
    o = c._ops
    assert c._schedule(True) == (Dual((o[0], o[2], o[4]), (o[1], o[3], o[5]), (2, 3, 4)),)
    # s0 outside the s0|s1 buffer: no dual launch; the three convs of s0 stacked, then those of s1 onto their running sums
    assert c._schedule(False) == (Conv(0, (o[0], o[2], o[4]), (2, 3, 4), None), Conv(1, (o[1], o[3], o[5]), (2, 3, 4), (2, 3, 4)))
    c = _cell(O.ALL_SKIP)
    for s0_in_pre in (True, False):
        sched = c._schedule(s0_in_pre)
        assert sched == (Add(0, 1, 2), Add(0, 1, 3), Add(0, 1, 4))
        assert not any(isinstance(s, (Conv, Dual)) for s in sched)
    # MIXED_ROWS: state 2 = conv(s0) + s1, state 3 = s0 + conv(s1), state 4 = conv(s1) + state 3 (ops paired by position)
    c = _cell(MIXED_ROWS)
    o = c._ops
    for s0_in_pre in (True, False):
        assert c._schedule(s0_in_pre) == (Conv(0, (o[0],), (2,), None), Conv(1, (o[3],), (3,), (0,)), Conv(1, (o[4],), (4,), None),
                                          Add(2, 1, 2), Add(4, 3, 4))
    # UNSORTED_ROWS: state 2 = conv(s0) + s1, state 3 = conv(s0) + state 2, state 4 = conv(state 2) + conv(state 3)
    c = _cell(UNSORTED_ROWS)
    o = c._ops
    for s0_in_pre in (True, False):
        assert c._schedule(s0_in_pre) == (Conv(0, (o[0], o[2]), (2, 3), None), Add(2, 1, 2), Conv(2, (o[4],), (4,), None), Add(3, 2, 3),
                                          Conv(3, (o[5],), (4,), (4,)))


def _random_rows(rng, steps=3):
    """each step selects one or two of its incoming edges, each with a random primitive; the rows in random order"""
    rows, offset = [], 0
    for i in range(steps):
        for e in rng.choice(2 + i, size=rng.integers(1, 3), replace=False):
            rows.append([offset + int(e), int(rng.integers(0, 2))])
        offset += 2 + i
    return np.array(rows)[rng.permutation(len(rows))]


def _schedule_row_sets():
    rng = np.random.default_rng(20240611)
    return list(NAMED_ROWS.items()) + [(f"random{i}", _random_rows(rng)) for i in range(200)]


def _interpret_schedule(cell, s0_in_pre, s0, s1):
    """Run the schedule on fp64 CPU tensors, one per state, checking on the way that no state is read before its last writer and that
    one launch keeps to one destination buffer and one residual buffer.  Returns (states, the (source, op) pairs the steps applied)."""
    import torch.nn.functional as F
    from rag_amd.modules import Add, Conv, Copy, Dual
    sched, where = cell._schedule(s0_in_pre), cell._layout(s0_in_pre)
    assert len(set(where)) == len(where) and where[0] == (("pre", 0) if s0_in_pre else ("s0", 0)) and where[1] == ("pre", cell.C_out)

    def writes(step):
        return step.dst_states if isinstance(step, (Dual, Conv)) else (step.dst,)

    left = {k: sum(k in writes(s) for s in sched) for k in range(2 + cell._steps)}      # writers still to come
    states, applied = {0: s0, 1: s1}, []

    def cbr(m, x):
        return F.relu(F.batch_norm(F.conv3d(x, m.conv.weight, padding=1), m.bn.running_mean, m.bn.running_var, m.bn.weight, m.bn.bias))

    def read(k, step):
        assert left[k] == 0 or k in writes(step), f"state {k} read by {step} before its last writer"
        return states[k]

    for step in sched:
        if isinstance(step, Dual):
            new = {k: cbr(ma, read(0, step)) + cbr(mb, read(1, step)) for k, ma, mb in zip(step.dst_states, step.a_mods, step.b_mods)}
            applied += [(0, m) for m in step.a_mods] + [(1, m) for m in step.b_mods]
        elif isinstance(step, Conv):
            assert len({where[k][0] for k in step.dst_states}) == 1
            assert step.res_states is None or (len(step.res_states) == len(step.dst_states) and len({where[r][0] for r in step.res_states}) == 1)
            new = {}
            for i, (k, m) in enumerate(zip(step.dst_states, step.mods)):
                new[k] = cbr(m, read(step.src, step))
                applied.append((step.src, m))
                if step.res_states is not None:
                    r = step.res_states[i]
                    assert r == k or r not in step.dst_states
                    new[k] = new[k] + read(r, step)
                    applied += [] if r == k else [(r, "identity", k)]
        elif isinstance(step, Add):
            new = {step.dst: read(step.a, step) + read(step.b, step)}
            applied += [(j, "identity", step.dst) for j in (step.a, step.b) if j != step.dst]
        else:
            assert isinstance(step, Copy)
            new = {step.dst: read(step.src, step).clone()}
            applied.append((step.src, "identity", step.dst))
        states.update(new)
        for k in new:
            left[k] -= 1
    return states, applied


_SCHEDULE_SETS = _schedule_row_sets()


@pytest.mark.parametrize("steps,block_multiplier", [(3, 3), (3, 2), (3, 1)])
@pytest.mark.parametrize("s0_in_pre", [True, False])
def test_cell_schedule_interpreted_matches_contributions(steps, block_multiplier, s0_in_pre):
    """Every concat state the schedule produces == sum over _contributions()[k] of op(state_j) (fp64, 1e-12 relative), for the named row
    sets and 200 seeded random ones; every (source, op) of _contributions() is applied by exactly one step."""
    import torch.nn.functional as F
    from rag_amd.modules import _ConvBR
    gen = torch.Generator().manual_seed(11)
    for name, rows in _SCHEDULE_SETS:
        cell = _cell(rows, steps, block_multiplier).double().eval()
        for m in cell._ops:
            if isinstance(m, _ConvBR):
                m.bn.running_mean.copy_(torch.randn(4, generator=gen, dtype=torch.float64) * 0.1)
                m.bn.running_var.copy_(torch.rand(4, generator=gen, dtype=torch.float64) + 0.5)
        s0, s1 = (torch.randn((1, 4, 2, 3, 4), generator=gen, dtype=torch.float64) for _ in range(2))
        with torch.no_grad():
            got, applied = _interpret_schedule(cell, s0_in_pre, s0, s1)
            contribs = cell._contributions()
            want = {0: s0, 1: s1}
            for k in sorted(contribs):
                want[k] = sum(F.relu(F.batch_norm(F.conv3d(want[j], op.conv.weight, padding=1), op.bn.running_mean, op.bn.running_var,
                                                  op.bn.weight, op.bn.bias)) if isinstance(op, _ConvBR) else want[j] for (j, op) in contribs[k])
        expected = sorted((j, id(op)) if isinstance(op, _ConvBR) else (j, -1, k) for k, lst in contribs.items() for (j, op) in lst)
        assert sorted((a[0], id(a[1])) if len(a) == 2 else (a[0], -1, a[2]) for a in applied) == expected, (name, rows)
        for k in range(2 + steps - block_multiplier, 2 + steps):
            err = float((got[k] - want[k]).abs().max()) / float(want[k].abs().max())
            assert err <= 1e-12, (name, rows, k, err)


@pytest.mark.parametrize("rows,any_dual", [(O.ALL_CONV, True), (O.ALL_SKIP, False), (MIXED_ROWS, False)])
def test_cell_schedule_is_cached_and_dual_branches_reads_it(rows, any_dual):
    import rag_amd
    from rag_amd.modules import Dual, _ConvBR
    net = rag_amd.MatchingNet(rag_amd.Genotype(rows, None, rows, None), maxdisp=48).eval()
    keys = set(net.state_dict())
    for c in (u[0] for u in net.cells_3d):
        contribs = c._contributions()
        assert c._contributions() is contribs
        expect = all([src for src, _op in lst] == [0, 1] and all(isinstance(op, _ConvBR) for _s, op in lst) for lst in contribs.values())
        for s0_in_pre in (True, False):
            sched = c._schedule(s0_in_pre)
            assert c._schedule(s0_in_pre) is sched and isinstance(sched, tuple)
            a, b, whole = c.dual_branches(s0_in_pre)
            if isinstance(sched[0], Dual):
                assert a == list(zip(sched[0].dst_states, sched[0].a_mods)) and b == list(zip(sched[0].dst_states, sched[0].b_mods))
            else:
                assert (a, b, whole) == (None, None, False)
            assert not any(isinstance(s, Dual) for s in sched[1:])
            assert whole == (expect and s0_in_pre) and expect == any_dual
    assert set(net.state_dict()) == keys and not any("cache" in n for n, _m in net.named_modules())      # the caches stay out of the tree


def test_plan_head_levels_switches_and_training(built_lib):
    import rag_amd
    from rag_amd import ops
    from rag_amd.modules import _HeadPlan, _plan_head
    net = rag_amd.MatchingNet(rag_amd.ALL_CONV_GENOTYPE, maxdisp=48).eval()
    m3, m6, m12 = net.last_3_3d[0], net.last_6_3d[0], net.last_12_3d[0]
    vol, f32, bf16 = (16, 48, 72), torch.float32, torch.bfloat16
    sizes = {1: (16, 48, 72), 2: (8, 24, 36), 4: (4, 12, 18)}
    chain = bool(built_lib.ragmi_conv3d_k1_chain_supported(48, 24, 12))
    upconv = bool(built_lib.ragmi_upconv3d_c1_supported(12, 8, 24, 36))
    old = ops.chain_k1_enabled(), ops.bf16_head_fp32_enabled()

    def plan(level, dtype=f32, train=False, vol=vol):
        return _plan_head(vol, sizes[level], dtype, m3, m6, m12, train)

    try:
        ops.set_chain_k1(True)
        ops.set_bf16_head_fp32(True)
        with torch.no_grad():
            for dtype in (f32, bf16):
                assert plan(1, dtype) == _HeadPlan(1, False, False, False)
                assert plan(2, dtype) == _HeadPlan(2, False, False, upconv)
            assert plan(4) == _HeadPlan(4, False, chain, upconv)
            assert plan(4, bf16) == _HeadPlan(4, True, False, upconv)
            ops.set_bf16_head_fp32(False)
            assert plan(4, bf16) == _HeadPlan(4, False, chain, upconv)
            ops.set_chain_k1(False)
            assert plan(4) == plan(4, bf16) == _HeadPlan(4, False, False, upconv)
            ops.set_chain_k1(True)
            ops.set_bf16_head_fp32(True)
            # an odd d: the upsampling is no exact factor 2
            assert plan(4, vol=(17, 48, 72)) == _HeadPlan(4, False, chain, False)
            assert plan(2, vol=(17, 48, 72)) == _HeadPlan(2, False, False, False)
            # a unit in its autograd form takes none of the fused launches
            for level in (2, 4):
                p = plan(level, train=True)
                assert (p.level, p.chain, p.upconv) == (level, False, False)
            with pytest.raises(ValueError, match="feature height must be a multiple of 4"):
                _plan_head(vol, (5, 16, 24), f32, m3, m6, m12, False)
            # the depth network's call: 2-D units on a depth-1 volume, its own last_3_3d (no m3)
            n6, n12 = rag_amd.ConvBR_2d(24, 12, 1, 1, 0).eval(), rag_amd.ConvBR_2d(48, 24, 1, 1, 0).eval()
            assert _plan_head((1, 48, 72), (1, 12, 18), f32, None, n6, n12, False) == _HeadPlan(4, False, chain, False)
            ops.set_chain_k1(False)
            assert _plan_head((1, 48, 72), (1, 12, 18), f32, None, n6, n12, False) == _HeadPlan(4, False, False, False)
    finally:
        ops.set_chain_k1(old[0])
        ops.set_bf16_head_fp32(old[1])


# ---- which kernel a 3x3x3 call runs on is decided once in the library (k3_route, rag_amd/csrc/conv3d.hip); the four shape predicates
# the fused executor plans from all ask it, so their answers cannot contradict each other.
def _csrc_constant(name):
    for fn in ("conv3d_x3_common.h", "conv3d_x3.hip"):
        m = re.search(r"constexpr int64_t %s = 1 << (\d+);" % name, open(os.path.join(ROOT, "rag_amd", "csrc", fn)).read())
        if m:
            return 1 << int(m.group(1))
    raise AssertionError(name)


def _k3_shape_grid():
    """(D, H, W): depth 1 and 2, W on both sides of every kernel's minimum, D = 7 / 8 around the z-marching minimum, volumes one row
    below and exactly at the two voxel thresholds, and the two level-3 volumes of the chain-plan tests above."""
    shapes = [(1, 64, W) for W in (8, 16, 31, 32)]
    for thr in (_csrc_constant("XD_MIN_VOXELS"), _csrc_constant("X3_MIN_VOXELS")):
        for D in (2, 7, 8):
            for W in (8, 16, 31, 32):
                at = -(-thr // (D * W))
                shapes += [(D, at - 1, W), (D, at, W)]
    return shapes + [(32, 64, 128), (64, 128, 416)]


@pytest.mark.parametrize("shape", _k3_shape_grid(), ids=lambda s: "x".join(map(str, s)))
def test_k3_host_predicates_agree(built_lib, shape):
    from rag_amd import ops
    uses_x3, g4_caps = built_lib.ragmi_conv3d_k3_uses_x3, built_lib.ragmi_conv3d_k3_g4_caps
    quarter, stem = built_lib.ragmi_conv3d_k3_quarter_store_supported, built_lib.ragmi_costvol_stem_conv3d_supported
    B, (D, H, W) = 2, shape
    fired = set()
    for dt in (ops.F32, ops.BF16, ops.F32X3):
        for cps in (4, 8, 12, 16, 24):
            for nset in (1, 2):
                for cout in (12, 16, 20):
                    for ntail in range(3):
                        vol = (cps * nset, cout, B, D, H, W, nset)
                        u = uses_x3(*vol, 0, ntail, dt)
                        fired.update(["x3"] if u else [])
                        for ndown in range(3):
                            caps, q = g4_caps(*vol, ntail, ndown, dt), quarter(*vol, ntail, ndown, dt)
                            fired.update((["caps"] if caps else []) + (["quarter"] if q else []))
                            assert 0 <= caps <= 3 and q in (0, 1)
                            assert not q or caps == 3, (vol, ntail, ndown, dt)
                            assert not caps or u, (vol, ntail, ndown, dt)
                            assert dt != ops.F32 or not (u or caps or q), (vol, ntail, ndown, dt)
        for C in (4, 8, 12):
            for cout in (12, 16, 20):
                for ntail in range(3):
                    s = stem(C, 12, cout, B, D, H, W, ntail, dt)
                    fired.update(["stem"] if s else [])
                    assert not s or (dt != ops.F32 and uses_x3(12, cout, B, D, H, W, 1, 0, ntail, dt)), (C, cout, shape, ntail, dt)
    # the implications are not vacuous: the level-3 volumes take every form, the depth-1 and deep-level ones the split-operand kernels
    if shape in ((32, 64, 128), (64, 128, 416)):
        assert fired == {"x3", "caps", "quarter", "stem"}, fired
    if shape in ((1, 64, 16), (1, 64, 32), (2, 256, 32), (8, 64, 32)):
        assert fired == {"x3"}, fired
