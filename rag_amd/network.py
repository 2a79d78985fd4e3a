"""`Network` — the reference's grown stereo model (src/models/rag_model.py:181-845) with the Matching-Net
half running on the HIP kernels of ``rag_amd``.

What `approaches/rag.py` (Appr) drives is kept one-to-one: ``forward(left, right, t, task_arch, path)``,
``search_forward(left, right, t, selected_ops)``, ``feature`` / ``matching`` / ``search_*``, the growth API
``expand(t, genotype, device)`` / ``select(t)`` / ``get_new_model`` / ``get_param`` / ``modify_param`` and the
attributes ``p, length, arch_init, new_models, model_to_train`` plus every per-layer ``nn.ModuleList`` name,
hence the checkpoint layout of ``run.py:194-196``.

The 2-D Feature Net (`Cell_2d`, `ConvBR_2d`; ≈1 % of the FLOPs) runs on the same HIP
kernels as the Matching Net: a 2-D conv is the 3-D kernel over a depth-1 volume, the stride-3 stem has its own
kernel (`ragmi_conv2d_k3_strided_fwd`), bilinear resampling is the trilinear kernel with one plane.  So
`Network.forward(left, right)` is HIP end to end; PyTorch only allocates.
"""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.nn as nn

from .metrics import MODE_RADIUS, refuse_autograd
from .modules import Cell_2d, Cell_3d, ConvBR_2d, ConvBR_3d, MatchingNet, _ConvBR  # noqa: F401

# Feature-Net macro architecture, rag_model.py:207-219: (prev_prev_fm, prev_fm, filter_multiplier, downup)
_CELL2D_ARCH = ((4, 4, 8, -1), (4, 8, 4, 1), (8, 4, 8, -1), (4, 8, 4, 1))


class Network(MatchingNet):
    """src/models/rag_model.py:181-845.  Unit lists grow with `expand` and shrink with `select`;
    `task_arch[name][0]` picks the unit of each layer for a task."""

    def __init__(self, genotype, device, maxdisp: int = 192):
        nn.Module.__init__(self)
        self.device = device
        self._num_layers_2d = 4
        self._K_multiplier = 2
        self._genotype0 = genotype
        self.length: Dict[str, int] = {}
        self.arch_init: Dict[str, List[int]] = {}
        # feature net (HIP, depth-1 volumes)
        self.cells_2d = nn.ModuleList()
        self.stem2d0 = nn.ModuleList([self._new_unit("stem_2d0", genotype)])
        self.stem2d1 = nn.ModuleList([self._new_unit("stem_2d1", genotype)])
        self.stem2d2 = nn.ModuleList([self._new_unit("stem_2d2", genotype)])
        for name in ("stem_2d0", "stem_2d1", "stem_2d2", "last_3_2d"):
            self.length[name], self.arch_init[name] = 1, [0]
        for i in range(self._num_layers_2d):
            self.cells_2d.append(nn.ModuleList([self._new_unit(f"cell_2d{i}", genotype)]))
            self.length[f"cell_2d{i}"], self.arch_init[f"cell_2d{i}"] = 1, [0]
        self.last_3_2d = nn.ModuleList([self._new_unit("last_3_2d", genotype)])
        # matching net (HIP)
        self._init_matching(genotype, maxdisp)
        self.act_dtype = torch.float32   # torch.bfloat16: Matching-Net activations stored as bf16 (BASELINE config 3)
        self.p = None               # per-layer unit probabilities during search_t
        self.new_models = None
        self.model_to_train = None

    # ------------------------------------------------------------------ unit bookkeeping
    # order of self.p: 3 stems 2d, 4 cells 2d, last_3_2d, 2 stems 3d, 8 cells 3d   (rag_model.py:403-498)
    def _p_layers(self) -> List[str]:
        return (["stem_2d0", "stem_2d1", "stem_2d2"] + [f"cell_2d{i}" for i in range(self._num_layers_2d)] +
                ["last_3_2d", "stem_3d0", "stem_3d1"] + [f"cell_3d{i}" for i in range(self._num_layers_3d)])

    def _units(self, name: str) -> nn.ModuleList:
        if name.startswith("cell_2d"):
            return self.cells_2d[int(name[7:])]
        if name.startswith("cell_3d"):
            return self.cells_3d[int(name[7:])]
        return getattr(self, {"stem_2d0": "stem2d0", "stem_2d1": "stem2d1", "stem_2d2": "stem2d2", "stem_3d0": "stem3d0",
                              "stem_3d1": "stem3d1"}.get(name, name))

    def _new_unit(self, name: str, genotype) -> nn.Module:
        fm = 12  # initial_fm = _filter_multiplier * _block_multiplier (rag_model.py:194)
        if name == "stem_2d0":
            return ConvBR_2d(3, fm // 2, 3, stride=1, padding=1)
        if name == "stem_2d1":
            return ConvBR_2d(fm // 2, fm, 3, stride=3, padding=1)
        if name == "stem_2d2":
            return ConvBR_2d(fm, fm, 3, stride=1, padding=1)
        if name == "last_3_2d":
            return ConvBR_2d(fm, fm, 1, 1, 0, bn=False, relu=False)
        if name.startswith("cell_2d"):
            pp, p, f, du = _CELL2D_ARCH[int(name[7:])]
            return Cell_2d(3, 3, pp, p, genotype, f, du)
        if name == "stem_3d0":
            return ConvBR_3d(fm * 2, fm, 3, stride=1, padding=1)
        if name == "stem_3d1":
            return ConvBR_3d(fm, fm, 3, stride=1, padding=1)
        if name.startswith("cell_3d"):
            return self._new_cell_3d(int(name[7:]), genotype)
        if name == "last_3_3d":
            return ConvBR_3d(fm, 1, 3, 1, 1, bn=False, relu=False)
        if name == "last_6_3d":
            return ConvBR_3d(fm * 2, fm, 1, 1, 0)
        if name == "last_12_3d":
            return ConvBR_3d(fm * 4, fm * 2, 1, 1, 0)
        raise KeyError(name)

    # ------------------------------------------------------------------ forward paths
    def feature(self, x, task_arch, path):                      # rag_model.py:285-323
        def unit(name):
            return task_arch[name][0] if task_arch is not None else None

        stem0 = self.stem2d0[unit("stem_2d0")](x)
        stem1 = self.stem2d1[unit("stem_2d1")](stem0)
        stem2 = self.stem2d2[unit("stem_2d2")](stem1)
        out = (stem1, stem2)
        for i, cell in enumerate(self.cells_2d):
            arch_cell = task_arch[f"cell_2d{i}"][0] if task_arch is not None else (path[i + 1] if path is not None else None)
            out = cell[arch_cell](out[0], out[1])
        if out[-1].size()[2] != stem2.size()[2]:
            raise ValueError("Network.feature: H and W must be multiples of 12 (the reference prints 'this is a bug' here)")
        return self.last_3_2d[unit("last_3_2d")](out[-1])

    def search_feature(self, x, selected_ops):                  # rag_model.py:641-660
        stem0 = self.stem2d0[selected_ops[0]](x)
        stem1 = self.stem2d1[selected_ops[1]](stem0)
        stem2 = self.stem2d2[selected_ops[2]](stem1)
        out = (stem1, stem2)
        for i, cell in enumerate(self.cells_2d):
            out = cell[selected_ops[i + 3]](out[0], out[1])
        if out[-1].size()[2] != stem2.size()[2]:
            raise ValueError("Network.search_feature: H and W must be multiples of 12")
        return self.last_3_2d[selected_ops[7]](out[-1])

    def _training_graph(self, *inputs) -> bool:
        """True when the call must build the reference's autograd graph / use batch statistics (rag.py:155-219)."""
        units = [m for m in self.modules() if isinstance(m, _ConvBR)] if self.training or torch.is_grad_enabled() else None
        if torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or any(p.requires_grad for p in self.parameters())):
            return True
        if units is None:
            # eval() on the root puts every unit in eval; a unit switched back to train() by hand is still honoured below
            units = self.__dict__.get("_convbr_cache")
            if units is None or self.__dict__.get("_convbr_count") != sum(len(self._units(n)) for n in self._p_layers()):
                units = [m for m in self.modules() if isinstance(m, _ConvBR)]
                self.__dict__["_convbr_cache"] = units
                self.__dict__["_convbr_count"] = sum(len(self._units(n)) for n in self._p_layers())
        return any(m.use_bn and m.bn.training for m in units)

    def _features(self, left, right, feature):
        if self._training_graph(left, right):
            # two passes like the reference: train-mode BatchNorm statistics are per view (rag_model.py:371-372)
            return feature(left), feature(right)
        # inference: both views share the Feature-Net weights and results are batch-independent -> one batched pass
        B = left.shape[0]
        fea = feature(torch.cat([left, right])).to(self.act_dtype)
        return fea[:B].contiguous(), fea[B:].contiguous()

    def forward(self, left, right, t, task_arch=None, path=None):   # rag_model.py:369-387
        lf, rf = self._features(left, right, lambda x: self.feature(x, task_arch, path))
        cost = self.matching(None, task_arch, path, features=(lf, rf))     # cost volume folded into stem3d0
        return self.disp(cost)

    def search_forward(self, left, right, t, selected_ops):        # rag_model.py:688-706
        lf, rf = self._features(left, right, lambda x: self.search_feature(x, selected_ops))
        cost = self.search_matching(None, selected_ops, t, features=(lf, rf))
        return self.disp(cost)

    def forward_stats(self, left, right, t, task_arch=None, path=None, out=None, stats=None):
        """forward with the head's statistics launch in place of the plain one -> DispStats (.disp is forward's result bit for
        bit, .variance / .peak / .entropy describe the distribution it is the mean of); inference only."""
        refuse_autograd("Network.forward_stats", left, right)
        with torch.no_grad():
            lf, rf = self._features(left, right, lambda x: self.feature(x, task_arch, path))
            cost = self.matching(None, task_arch, path, features=(lf, rf))
            return self.disp.forward_stats(cost, out, stats)

    def forward_train_stats(self, left, right, t, task_arch=None, path=None):
        """forward under autograd (two feature passes in training mode, as forward) with the head's statistics launch and its
        adjoint in place of the plain pair -> DispStats whose .disp and .tensor carry the graph.  fp32 only."""
        if left.dtype != torch.float32 or right.dtype != torch.float32:
            raise RuntimeError(f"Network.forward_train_stats: fp32 only (got {left.dtype}, {right.dtype})")
        lf, rf = self._features(left, right, lambda x: self.feature(x, task_arch, path))
        cost = self.matching(None, task_arch, path, features=(lf, rf))
        return self.disp.forward_train_stats(cost)

    def search_forward_stats(self, left, right, t, selected_ops, out=None, stats=None):
        """search_forward with the head's statistics launch -> DispStats; inference only."""
        refuse_autograd("Network.search_forward_stats", left, right)
        with torch.no_grad():
            lf, rf = self._features(left, right, lambda x: self.search_feature(x, selected_ops))
            cost = self.search_matching(None, selected_ops, t, features=(lf, rf))
            return self.disp.forward_stats(cost, out, stats)

    def forward_mode(self, left, right, t, task_arch=None, path=None, radius=MODE_RADIUS, out=None, stats=None, mode=None):
        """forward with the head's mode launch in place of the plain one -> DispMode (a DispStats with .mode_index / .mode_disp /
        .mode_mass: the disparity regressed inside a window of `radius` fine px around the distribution's mode, and the probability
        that window holds); inference only."""
        refuse_autograd("Network.forward_mode", left, right)
        with torch.no_grad():
            lf, rf = self._features(left, right, lambda x: self.feature(x, task_arch, path))
            cost = self.matching(None, task_arch, path, features=(lf, rf))
            return self.disp.forward_mode(cost, radius, out, stats, mode)

    def search_forward_mode(self, left, right, t, selected_ops, radius=MODE_RADIUS, out=None, stats=None, mode=None):
        """search_forward with the head's mode launch -> DispMode; inference only."""
        refuse_autograd("Network.search_forward_mode", left, right)
        with torch.no_grad():
            lf, rf = self._features(left, right, lambda x: self.search_feature(x, selected_ops))
            cost = self.search_matching(None, selected_ops, t, features=(lf, rf))
            return self.disp.forward_mode(cost, radius, out, stats, mode)

    def forward_lr(self, left, right, t, task_arch=None, path=None, **check_kw):
        """Both views' disparities and their left-right consistency from ONE forward of the stacked 2B batch
        (rag_amd.metrics.lr_stack: sample i + B is the pair seen from the right camera, mirrored along x) and one check launch
        (lr_consistency(D, D, mirrored=True, partner_shift=B, **check_kw); check_kw: abs_tol, rel_tol, occluded_weight, want_error).
        -> (disp_left, disp_right, check_left, check_right): each disparity [B,H,W] and each LRCheck in its own camera's coordinates
        (the right one mirrored back), disparities positive in both; inference only."""
        from .metrics import LRCheck, lr_consistency, lr_stack
        refuse_autograd("Network.forward_lr", left, right)
        for k in check_kw:
            if k not in ("abs_tol", "rel_tol", "occluded_weight", "want_error"):
                raise TypeError(f"Network.forward_lr: unexpected keyword {k!r} (mirrored and partner_shift are set by the stacked form)")
        with torch.no_grad():
            B = left.shape[0]
            left2, right2 = lr_stack(left, right)
            disp = self.forward(left2, right2, t, task_arch, path)
            chk = lr_consistency(disp, disp, mirrored=True, partner_shift=B, **check_kw)

            def back(v):                                    # the right camera's half, mirrored back into its own coordinates
                return v[B:].flip(-1) if v is not None else None
            return (disp[:B], back(disp), LRCheck(chk.weight[:B], chk.error[:B] if chk.error is not None else None, chk.valid[:B]),
                    LRCheck(back(chk.weight), back(chk.error), chk.valid[B:]))

    def forward_dense(self, left, right, t, task_arch=None, path=None, median=0, fill_value=0.0, speckle=None, **check_kw):
        """forward_lr, then every pixel its check rejects filled on the device (rag_amd.metrics.fill_disparity: the smaller of the
        nearest consistent disparities on its row, rows without one along the columns, then an optional 3x3 / 5x5 median).
        -> (dense_left, dense_right, check_left, check_right): the checks are forward_lr's; each dense_* is the FilledDisp (.disp,
        .code, .counts, .density, .filled) of fill_disparity(that view's disparity, its check, median, fill_value), run per view in
        that camera's own coordinates, so left and right mean the same in both.  `speckle` = (max_size, max_diff): each view's
        disparity and check first go through rag_amd.metrics.filter_speckles, in the same coordinates; the fill takes its result in
        place of the check and carries it as dense_*.speckles (None without).  check_kw as forward_lr; inference only."""
        from .metrics import fill_disparity, filter_speckles
        refuse_autograd("Network.forward_dense", left, right)
        if speckle is not None and (not isinstance(speckle, (tuple, list)) or len(speckle) != 2):
            raise ValueError(f"Network.forward_dense: speckle must be None or (max_size, max_diff), got {speckle!r}")
        disp_l, disp_r, chk_l, chk_r = self.forward_lr(left, right, t, task_arch, path, **check_kw)
        if speckle is None:
            return (fill_disparity(disp_l, chk_l, median, fill_value), fill_disparity(disp_r, chk_r, median, fill_value), chk_l, chk_r)

        def dense(disp, chk):
            spk = filter_speckles(disp, chk, speckle[0], speckle[1])
            out = fill_disparity(disp, spk, median, fill_value)
            out.speckles = spk
            return out
        return dense(disp_l, chk_l), dense(disp_r, chk_r), chk_l, chk_r

    # ------------------------------------------------------------------ the unit search's step (Appr.search_epoch, rag.py:344-406)
    def search_mode(self):
        """The module modes of search_epoch (rag.py:345-368): train() on the root, then eval() on every unit of the stems,
        last_3_2d and the cells - reused and candidate alike, so the trunk's BatchNorms use and keep their running statistics
        while the candidates' weights train; only the head lists stay in training mode.  Returns self."""
        self.train()
        for name in self._p_layers():
            for unit in self._units(name):
                unit.eval()
        return self

    def check_selected(self, t, selected_ops) -> List[int]:
        """`selected_ops` as a list of ints after the checks of the unit-search step: one unit index per `p` layer, each inside
        its ModuleList, and `t` inside the three head lists.  ValueError otherwise."""
        names = self._p_layers()
        if selected_ops is None or len(selected_ops) != len(names):
            raise ValueError(f"selected_ops must name one unit for each of the {len(names)} layers of p (rag_model.py:403-498)")
        sel = [int(v) for v in selected_ops]
        for name, idx in zip(names, sel):
            if not 0 <= idx < len(self._units(name)):
                raise ValueError(f"selected_ops: unit {idx} of {name} does not exist ({len(self._units(name))} units)")
        if t is None or isinstance(t, bool) or int(t) != t or not 0 <= int(t) < min(len(self.last_3_3d), len(self.last_6_3d), len(self.last_12_3d)):
            raise ValueError(f"selected_ops: t = {t!r} is outside the head lists (last_3_3d / last_6_3d / last_12_3d)")
        return sel

    def active_parameters(self, t, selected_ops) -> list:
        """The parameters a backward of search_forward(.., t, selected_ops) gives a gradient, read off the wiring: of every layer of
        `p` the parameters unit selected_ops[k] reads in its forward, and of the head last_12_3d[t], last_6_3d[t] and
        last_3_3d[t].conv.weight - those that require grad (after freeze_model / modify_param(new_models), rag.py:89-90, a reused
        unit contributes nothing).  A bn=False unit constructs a BatchNorm it never calls: its affine is never included."""
        sel = self.check_selected(t, selected_ops)
        out = []
        for name, idx in zip(self._p_layers(), sel):
            out += self._units(name)[idx].forward_parameters()
        for units in (self.last_12_3d, self.last_6_3d, self.last_3_3d):
            out += units[int(t)].forward_parameters()
        return [p for p in out if p.requires_grad]

    # ------------------------------------------------------------------ growth API
    def expand(self, t, genotype, device="cuda"):               # rag_model.py:391-522
        """Add one candidate unit per layer (built from `genotype`) and one head triple for task t; reset `p` so
        that every existing unit is K times as likely as the new one."""
        self.p = []
        for name in self._p_layers():
            self._units(name).append(self._new_unit(name, genotype).to(device))
            n_old = self.length[name]
            temp = torch.full((n_old + 1,), 1 / (self._K_multiplier * n_old + 1))
            temp[:n_old] *= self._K_multiplier
            self.p.append(temp)
        for name in ("last_3_3d", "last_6_3d", "last_12_3d"):
            self._units(name).append(self._new_unit(name, genotype).to(device))
        self.get_new_model(t=t)

    def get_new_model(self, t):                                 # rag_model.py:525-551
        new_models = {name: [self.length[name]] for name in self._p_layers()}
        for name in ("last_3_3d", "last_6_3d", "last_12_3d"):
            new_models[name] = [t]
        self.new_models = new_models

    def _modules_of(self, models) -> List[nn.Module]:
        order = (["stem_2d0", "stem_2d1", "stem_2d2", "last_3_2d", "stem_3d0", "stem_3d1", "last_3_3d", "last_6_3d",
                  "last_12_3d"] + [f"cell_2d{i}" for i in range(self._num_layers_2d)] +
                 [f"cell_3d{i}" for i in range(self._num_layers_3d)])
        return [self._units(name)[idx] for name in order if name in models for idx in models[name]]

    def get_param(self, models):                                # rag_model.py:553-595
        return [{"params": m.parameters()} for m in self._modules_of(models)]

    def modify_param(self, models, requires_grad=True):         # rag_model.py:597-638
        for m in self._modules_of(models):
            for param in m.parameters():
                param.requires_grad = requires_grad

    def select(self, t):                                        # rag_model.py:709-845
        """Keep, per layer, the most probable unit: reuse an old one (drop the candidate) or keep the candidate
        (it becomes a unit to train).  Returns the task's architecture dict."""
        model_to_train: Dict[str, list] = {}
        best_archi: Dict[str, list] = {}
        for k, name in enumerate(self._p_layers()):
            _v, idx = torch.max(self.p[k], dim=0)
            c = self.length[name]
            model_to_train[name], best_archi[name] = [], []
            if idx == c:
                best_archi[name].append(c)
                model_to_train[name].append(c)
            else:
                best_archi[name].append(idx)
                del self._units(name)[c]
            self.length[name] = len(self._units(name))
        for name in ("last_3_3d", "last_6_3d", "last_12_3d"):
            model_to_train[name], best_archi[name] = [t], [t]
        self.model_to_train = model_to_train
        return best_archi
