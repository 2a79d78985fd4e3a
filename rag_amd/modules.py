"""Host-side mirror of the reference's Matching-Net modules, running on librag_amd.so.

Names, constructor signatures, attribute names and state_dict key layout follow
chzhang18/RAG (src/models/rag_model.py, src/automl/operations_3d.py,
src/automl/genotypes_{2d,3d}.py) so a reference checkpoint loads unchanged and the
approaches/automl growth loop can poke the same attributes.  The arithmetic is NOT
PyTorch: every forward below enqueues hand-written HIP kernels through ``rag_amd.ops``.

New seam (named by BASELINE.json north_star; the reference inlines it in Network.forward,
rag_model.py:375-386): ``MatchingNet.forward(left_fea, right_fea) -> disp[B, 3h, 3w]``.

Two execution modes, both on the HIP kernels, neither with a PyTorch fallback:
  * inference (``torch.no_grad()`` + eval-mode BatchNorm): the fused executor below (folded BN, concat-free cells,
    dual-input launches, cross-module tails);
  * training (autograd enabled and something requires grad, or a BatchNorm in train mode): the same modules compose
    the ``rag_amd.autograd`` Functions node by node like the reference's graph (approaches/rag.py:155-219).
"""
from __future__ import annotations

from collections import namedtuple
from types import MappingProxyType
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import torch
import torch.nn as nn

from . import autograd as ag
from . import ops
from .metrics import MODE_RADIUS, DispMode, DispStats, refuse_autograd

# src/automl/genotypes_2d.py:4-8 — the genotype handed to Network / Cell_3d; 3-D cells read `.reduce`
Genotype = namedtuple("Genotype_2D", "normal normal_concat reduce reduce_concat")
# src/automl/genotypes_3d.py:6-9
PRIMITIVES_3D = ["skip_connect_3d", "3d_conv_3x3"]

ALL_CONV_ROWS = np.array([[0, 1], [1, 1], [2, 1], [3, 1], [5, 1], [6, 1]])
ALL_SKIP_ROWS = np.array([[0, 0], [1, 0], [2, 0], [3, 0], [5, 0], [6, 0]])
ALL_CONV_GENOTYPE = Genotype(normal=ALL_CONV_ROWS, normal_concat=None, reduce=ALL_CONV_ROWS, reduce_concat=None)


def _volume(size) -> int:
    n = 1
    for v in size:
        n *= int(v)
    return n


ALL_SKIP_GENOTYPE = Genotype(normal=ALL_SKIP_ROWS, normal_concat=None, reduce=ALL_SKIP_ROWS, reduce_concat=None)


class Identity_3d(nn.Module):
    """src/automl/operations_3d.py:84-90."""

    def forward(self, x):
        return x


class _ConvBR(nn.Module):
    """Conv(bias=False) -> BatchNorm -> ReLU as ONE fused HIP kernel; shared by the 3-D (Matching Net) and 2-D (Feature
    Net, a depth-1 volume on the same kernels) flavours.  Sub-module names `conv` / `bn`, the always-constructed `bn`
    and the init follow the reference (operations_3d.py:31-55, operations_2d.py:31-55)."""

    NDIM = 3

    def __init__(self, C_in, C_out, kernel_size, stride, padding, bn=True, relu=True):
        super().__init__()
        self.relu = relu
        self.use_bn = bn
        if self.NDIM == 3:
            self.conv = nn.Conv3d(C_in, C_out, kernel_size, stride=stride, padding=padding, bias=False)
            self.bn = nn.BatchNorm3d(C_out)
        else:
            self.conv = nn.Conv2d(C_in, C_out, kernel_size, stride=stride, padding=padding, bias=False)
            self.bn = nn.BatchNorm2d(C_out)
        self._initialize_weights()
        self._cache = None

    def _initialize_weights(self):
        nn.init.kaiming_normal_(self.conv.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.bn.weight, 1)
        nn.init.constant_(self.bn.bias, 0)

    # -- HIP-side parameters: packed weights + folded eval-mode BN, cached on tensor versions
    def _geometry(self) -> int:
        """kernel size 1 or 3 (stride 1, 'same' padding), or -3 for the strided 2-D 3x3 stem (Feature Net)."""
        k, n = self.conv.kernel_size, self.NDIM
        same = self.conv.padding == tuple((ki - 1) // 2 for ki in k) and self.conv.dilation == (1,) * n and self.conv.groups == 1
        if same and k in ((1,) * n, (3,) * n) and self.conv.stride == (1,) * n:
            return k[0]
        if same and n == 2 and k == (3, 3) and self.conv.stride[0] == self.conv.stride[1] > 1:
            return -3
        raise NotImplementedError("rag_amd ConvBR: only 1x1(x1)/pad0 and 3x3(x3)/pad1 at stride 1 (plus the strided 2-D 3x3 "
                                  "stem) are built (everything the reference instantiates)")

    def _small(self) -> bool:
        """Cout <= 2 (last_3_3d): VALU form of the 3x3x3 kernel instead of the 4-row MFMA."""
        return (self.NDIM == 3 and self.conv.out_channels <= 2 and self.conv.in_channels % 4 == 0
                and self.conv.in_channels <= 128)

    def stamp(self) -> tuple:
        w, bn = self.conv.weight, self.bn
        return (w.data_ptr(), w._version, bn.weight._version, bn.bias._version, bn.running_mean._version,
                bn.running_var._version, bn.weight.data_ptr(), str(w.device), self.use_bn)

    def prepared(self) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
        """(weights in kernel layout, scale, shift); scale/shift None when bn=False."""
        if self.use_bn and self.bn.training:
            raise RuntimeError("rag_amd ConvBR: folded BatchNorm parameters requested in train mode (internal error: "
                               "train-mode units run through rag_amd.autograd)")
        stamp = self.stamp()
        if self._cache is None or self._cache[0] != stamp:
            k = self._geometry()
            w = self.conv.weight.detach()
            with torch.no_grad():
                if k == -3 or (k == 3 and self._small()):
                    wk = w.contiguous()                      # strided 2-D stem / VALU form read the raw weight
                elif k == 3:
                    wk = ops.conv3d_k3_pack(w)               # a 2-D 3x3 packs as the dz = 1 plane of a 3x3x3 (depth-1 volumes)
                else:
                    wk = w.reshape(w.shape[0], w.shape[1]).contiguous()
                if self.use_bn:
                    bn = self.bn
                    # same folding ATen's eval batch_norm uses: alpha = gamma * rsqrt(var + eps); beta = b - mean * alpha
                    scale = (bn.weight.detach() * torch.rsqrt(bn.running_var.detach() + bn.eps)).float().contiguous()
                    shift = (bn.bias.detach() - bn.running_mean.detach() * scale).float().contiguous()
                else:
                    scale = shift = None
            self._cache = (stamp, wk, scale, shift)
        return self._cache[1], self._cache[2], self._cache[3]

    def forward_parameters(self) -> list:
        """The parameters forward() reads: the weight, and the BatchNorm affine unless bn=False (that unit constructs a BatchNorm
        it never calls)."""
        return [self.conv.weight] + ([self.bn.weight, self.bn.bias] if self.use_bn else [])

    def autograd_mode(self, *inputs) -> bool:
        """Training composition needed: a gradient is wanted, or this unit's BatchNorm uses batch statistics."""
        return (ag.needs_grad(*inputs, self.conv.weight, self.bn.weight, self.bn.bias)
                or (self.use_bn and self.bn.training))

    def _forward_autograd(self, x: torch.Tensor, resample_to: Optional[Sequence[int]]) -> torch.Tensor:
        if x.dtype != torch.float32:
            raise NotImplementedError("rag_amd: the training path is fp32 (bf16 storage is inference only)")
        if self._geometry() == -3:
            return ag.StridedStemFn.apply(x if x.dim() == 4 else x.squeeze(2), self.conv.weight, self.bn.weight, self.bn.bias, self)
        squeeze = x.dim() == 4
        if squeeze:
            x = x.unsqueeze(2)
        if resample_to is not None:
            x = ag.resample(x, resample_to, True)
        y = ag.ConvBRFn.apply(x, self.conv.weight, self.bn.weight, self.bn.bias, self)
        return y.squeeze(2) if squeeze else y      # (a select's backward is zeros + copy_: a memcpy node when captured)

    def costvol_fusable(self, C_fea: int) -> bool:
        """This unit can consume (left_fea, right_fea) directly instead of the cost volume (ragmi_costvol_stem_fwd)."""
        return (self.NDIM == 3 and self._geometry() == 3 and self.conv.in_channels == 2 * C_fea and C_fea <= 16
                and self.conv.out_channels <= 16)

    def costvol_variants(self) -> torch.Tensor:
        """pre-summed weight variants of the fused cost-volume form, cached on the weight version."""
        w = self.conv.weight
        key = (w.data_ptr(), w._version, str(w.device))
        hit = getattr(self, "_cv_cache", None)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, ops.costvol_stem_prepare(w.detach()))
            self._cv_cache = hit
        return hit[1]

    def forward_costvol(self, left_fea, right_fea, maxdisp, tails=None, out_g4: bool = False) -> torch.Tensor:
        """act(bn(conv(cost_volume(left_fea, right_fea)))) without materialising the cost volume (inference)."""
        _wk, scale, shift = self.prepared()
        return ops.costvol_stem(left_fea, right_fea, maxdisp, self.costvol_variants(), self.conv.out_channels, scale, shift,
                                self.relu, tails=tails, out_g4=out_g4)

    def as_tail(self, out: torch.Tensor, out_ch0: int, g4: bool = False) -> "ops.Tail":
        """This 1x1(x1) ConvBR (<= 4 output channels) as a tail of the kernel that produces its input (g4: `out` is a
        channel-group-interleaved buffer, ops.Tail)."""
        if self._geometry() != 1 or self.conv.out_channels > 4:
            raise ValueError("only 1x1x1 ConvBR with <= 4 output channels can be fused as a tail")
        wk, scale, shift = self.prepared()
        return ops.Tail(wk, scale, shift, self.relu, out, out_ch0, g4=g4)

    def as_down_tails(self, out: torch.Tensor, out_ch0: int) -> List["ops.Tail"]:
        """This 1x1x1 ConvBR (<= 8 output channels) applied to the x0.5 trilinear down-sampling of the producer's output, as one or
        two down-sampling tails (4 output channels each) of the kernel that produces its input; `out` is at half resolution."""
        if self._geometry() != 1 or self.conv.out_channels > 8:
            raise ValueError("only 1x1x1 ConvBR with <= 8 output channels can be fused as down-sampling tails")
        wk, scale, shift = self.prepared()
        tails = []
        for c0 in range(0, self.conv.out_channels, 4):
            c1 = min(c0 + 4, self.conv.out_channels)
            tails.append(ops.Tail(wk[c0:c1], None if scale is None else scale[c0:c1], None if shift is None else shift[c0:c1],
                                  self.relu, out, out_ch0 + c0, down=True))
        return tails

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, out_ch0: int = 0,
                resample_to: Optional[Sequence[int]] = None, tails: Optional[Sequence["ops.Tail"]] = None,
                store_main: bool = True, out_dtype: Optional[torch.dtype] = None, x_g4: bool = False) -> torch.Tensor:
        """`out`/`out_ch0` write into a channel slice of a wider buffer.  `x_g4` (3x3x3 form of the fused executor only): x is a
        channel-group-interleaved buffer (ops.conv3d_k3).  `resample_to` (1x1x1 only) first resamples x
        trilinearly (align_corners=True) to that size inside the same kernel — the reference's
        `conv(F.interpolate(x, size, mode='trilinear', align_corners=True))`.  The 2-D flavour accepts [B,C,H,W] (or an
        already depth-1 5-D view) and returns the same rank.  `out_dtype=torch.float32` (Cout <= 2 form only) keeps the result
        in fp32 although x is bf16: the head's `mat`."""
        if self.autograd_mode(x):
            if out is not None or tails:
                raise RuntimeError("rag_amd ConvBR: fused destinations/tails belong to the inference executor")
            return self._forward_autograd(x, resample_to)
        k = self._geometry()
        wk, scale, shift = self.prepared()
        cout = self.conv.out_channels
        if x_g4 and (k != 3 or self._small() or resample_to is not None or x.dim() != 5):
            raise RuntimeError("rag_amd ConvBR: a G4 input is taken by the 3x3x3 form only")
        if k == -3:
            return ops.conv2d_k3_strided(x if x.dim() == 4 else x[:, :, 0], wk, scale, shift, self.relu, self.conv.stride[0])
        squeeze = x.dim() == 4
        if squeeze:
            x = x.unsqueeze(2)
        # mixed storage (MatchingNet._run_chain): a bf16 input into an fp32 buffer is taken by the resample + 1x1x1 launch only
        # (an input already at the output size is its identity case)
        mixed = out is not None and out.dtype != x.dtype
        if mixed:
            if k != 1 or x.dtype != torch.bfloat16 or out.dtype != torch.float32:
                raise RuntimeError("rag_amd ConvBR: only a 1x1x1 conv crosses from bf16 storage to an fp32 destination")
            resample_to = tuple(x.shape[2:]) if resample_to is None else resample_to
        elif resample_to is not None and tuple(resample_to) == tuple(x.shape[2:]):
            resample_to = None
        if resample_to is not None:
            if k != 1:
                raise NotImplementedError("ConvBR: fused resample is built for the 1x1x1 form only")
            if out is None:
                out = torch.empty((x.shape[0], cout) + tuple(int(v) for v in resample_to), device=x.device, dtype=x.dtype)
            if not mixed and _volume(resample_to) > _volume(x.shape[2:]) and cout <= x.shape[1]:
                # upsampling: mix the channels (and fold the BatchNorm) on the SMALL volume, then interpolate the Cout maps and
                # apply the ReLU — both steps are affine and the taps sum to one, so only the rounding order differs
                low = torch.empty((x.shape[0], cout) + tuple(x.shape[2:]), device=x.device, dtype=x.dtype)
                ops.conv3d_k1(x, wk, scale, shift, False, low)
                ops.trilinear3d_act(low, resample_to, True, self.relu, out, out_ch0)
            else:
                ops.conv3d_k1_resample(x, resample_to, True, wk, scale, shift, self.relu, out, out_ch0)
            return out[:, :, 0] if squeeze else out
        if out is None:
            odt = out_dtype if (out_dtype is not None and k == 3 and self._small()) else x.dtype
            out = torch.empty((x.shape[0], cout) + tuple(x.shape[2:]), device=x.device, dtype=odt)
        if k == 3 and self._small():
            ops.conv3d_k3_small(x, wk, scale, shift, self.relu, out, out_ch0)
        elif k == 3:
            groups = [out_ch0 + 4 * g for g in range(ops.packed_groups(cout))]
            ops.conv3d_k3(x, wk, cout, scale, shift, self.relu, out, groups, tails=tails, store_main=store_main, x_g4=x_g4)
        else:
            ops.conv3d_k1(x, wk, scale, shift, self.relu, out, out_ch0)
        return out[:, :, 0] if squeeze else out


class ConvBR_3d(_ConvBR):
    """src/automl/operations_3d.py:31-47 — same ctor `(C_in, C_out, kernel_size, stride, padding, bn=True, relu=True)`."""
    NDIM = 3


class ConvBR_2d(_ConvBR):
    """src/automl/operations_2d.py:31-47 (Feature Net) on the same kernels over a depth-1 volume."""
    NDIM = 2


class Identity_2d(nn.Module):
    """src/automl/operations_2d.py Identity_2d."""

    def forward(self, x):
        return x


# src/automl/operations_3d.py:5-8 (stride is always 1 on the hot path)
def _skip(C, stride):
    if stride != 1:
        raise NotImplementedError("skip_connect_3d with stride != 1 is dead code in the reference (FactorizedReduce typo)")
    return Identity_3d()


OPS_3d = {
    "skip_connect_3d": _skip,
    "3d_conv_3x3": lambda C, stride: ConvBR_3d(C, C, 3, stride, 1),
}


# src/automl/genotypes_2d.py:10-12, operations_2d.py:5-8
PRIMITIVES = ["skip_connect_2d", "conv_3x3"]


def _skip_2d(C, stride):
    if stride != 1:
        raise NotImplementedError("skip_connect_2d with stride != 1 is dead code in the reference")
    return Identity_2d()


OPS_2d = {"skip_connect_2d": _skip_2d, "conv_3x3": lambda C, stride: ConvBR_2d(C, C, 3, stride, 1)}


class DisparityRegression(nn.Module):
    """src/models/rag_model.py:18-29: out[b,y,x] = sum_d x[b,d,y,x] * d."""

    def __init__(self, maxdisp):
        super().__init__()
        self.maxdisp = maxdisp

    def forward(self, x):
        assert x.is_contiguous() is True
        if ag.needs_grad(x):
            return ag.DispRegFn.apply(x, self.maxdisp)
        return ops.disparity_regression(x, self.maxdisp)

    def forward_stats(self, x, out=None, stats=None):
        """forward with the statistics of x's disparity axis in the same launch -> DispStats; inference only."""
        assert x.is_contiguous() is True
        refuse_autograd("DisparityRegression.forward_stats", x)
        return DispStats(*ops.disparity_regression_stats(x, self.maxdisp, out, stats))

    def forward_mode(self, x, radius=MODE_RADIUS, out=None, stats=None, mode=None):
        """forward_stats with the first arg-max of x's disparity axis, the regression over |k - arg-max| <= radius and that window's
        mass in the same launch -> DispMode; inference only."""
        assert x.is_contiguous() is True
        refuse_autograd("DisparityRegression.forward_mode", x)
        return DispMode(*ops.disparity_regression_mode(x, self.maxdisp, radius, out, stats, mode), radius)


class Disp(nn.Module):
    """src/models/rag_model.py:32-44, fused: trilinear x3 (align_corners=False) -> Softmin -> regression."""

    def __init__(self, maxdisp=192):
        super().__init__()
        self.maxdisp = maxdisp
        self.softmax = nn.Softmin(dim=1)                            # kept for attribute parity; unused
        self.disparity = DisparityRegression(maxdisp=self.maxdisp)  # idem

    def forward(self, x):
        if ag.needs_grad(x):
            return ag.DispFn.apply(x, self.maxdisp)
        return ops.disp_softargmin(x, self.maxdisp)

    def forward_stats(self, x, out=None, stats=None):
        """forward with the per-pixel variance, peak and entropy of the softmin distribution in the same launch -> DispStats
        (.disp is forward's result bit for bit); inference only.  `out` / `stats`: caller-owned outputs (a captured graph's)."""
        refuse_autograd("Disp.forward_stats", x)
        return DispStats(*ops.disp_softargmin_stats(x, self.maxdisp, out, stats))

    def forward_mode(self, x, radius=MODE_RADIUS, out=None, stats=None, mode=None):
        """forward_stats with the mode-local disparity in the same launch -> DispMode: .mode_index is the fine index of the smallest
        upsampled cost, .mode_disp the regression over |k - index| <= radius (on one surface where .disp averages two at a depth
        edge), .mode_mass the probability of that window; .disp and .tensor are forward_stats' bits.  Inference only."""
        refuse_autograd("Disp.forward_mode", x)
        return DispMode(*ops.disp_softargmin_mode(x, self.maxdisp, radius, out, stats, mode), radius)

    def forward_train_stats(self, x):
        """forward_stats under autograd -> DispStats whose .disp and .tensor carry the graph (ag.DispStatsFn: the adjoint of the
        disparity, variance, peak and entropy in one launch).  .disp is forward's result bit for bit.  fp32 only."""
        if x.dtype != torch.float32:
            raise RuntimeError(f"Disp.forward_train_stats: fp32 only (got {x.dtype}): the statistics' adjoint is not built for bf16 costs")
        return DispStats(*ag.DispStatsFn.apply(x, self.maxdisp))


def _scale_dimension(dim, scale):
    """rag_model.py:140-141 (and build_model_3d.py's cell): the size of one axis after a x0.5 / x2 resample."""
    return int((float(dim) - 1.0) * scale + 1.0) if dim % 2 == 1 else int(float(dim) * scale)


# What one cell launches behind its two 1x1x1 preprocess convs, as data (_Cell._schedule): a tuple of these steps, issued in order by
# _Cell._run.  States are indices (0 = s0, 1 = s1, 2.. = the new states; _Cell._layout places each in a buffer), never tensors.
#   Dual: ONE dual-input launch, state k = relu(bn(conv_a(s0))) + relu(bn(conv_b(s1))) for every k of dst_states (a_mods / b_mods stacked).
#   Conv: one 3x3x3 launch on state `src` with the sibling convs `mods` stacked; unit i writes dst_states[i] (all in one buffer) and, where
#         res_states is not None, adds res_states[i] (the running sum of its target, or an identity partner that is already complete).
#   Add:  dst = a + b.      Copy: dst = src (a lone identity branch).
Dual = namedtuple("Dual", "a_mods b_mods dst_states")
Conv = namedtuple("Conv", "src mods dst_states res_states")
Add = namedtuple("Add", "a b dst")
Copy = namedtuple("Copy", "src dst")


class _Cell(nn.Module):
    """Shared executor of Cell_3d (rag_model.py:114-177) and Cell_2d (:47-111) on HIP kernels; tensors are 5-D
    (the 2-D cell runs on depth-1 volumes: scale_dimension(1, s) == 1, and trilinear with one plane is bilinear).

    forward(prev_prev_input, prev_input) -> (prev_input, concat).  The 1x1x1 preprocess convs
    write s0|s1 into one buffer, every selected op writes/accumulates straight into its
    channel slice of the concat buffer (no `sum`, no `torch.cat` passes), and sibling
    3x3x3 convs that read the same state run as one launch.  Op/branch pairing is
    positional like the reference (ops created in genotype-row order, consumed in
    ascending-branch visit order: SURVEY.md §8 A6).
    """

    def __init__(self, steps, block_multiplier, prev_prev_fmultiplier, prev_filter_multiplier, genotype,
                 filter_multiplier, downup_sample):
        super().__init__()
        self.genotype = genotype
        self.C_in = block_multiplier * filter_multiplier
        self.C_out = filter_multiplier
        self.C_prev = int(block_multiplier * prev_filter_multiplier)
        self.C_prev_prev = int(block_multiplier * prev_prev_fmultiplier)
        self.downup_sample = downup_sample
        self.pre_preprocess = self.CONV(self.C_prev_prev, self.C_out, 1, 1, 0)
        self.preprocess = self.CONV(self.C_prev, self.C_out, 1, 1, 0)
        self._steps = steps
        self.block_multiplier = block_multiplier
        self._ops = nn.ModuleList()
        if downup_sample == -1:
            self.scale = 0.5
        elif downup_sample == 1:
            self.scale = 2
        for x in self._rows():
            self._ops.append(self.OPS[self.PRIMS[x[1]]](self.C_out, stride=1))
        self._fused_cache: Dict[tuple, tuple] = {}

    def _rows(self):
        raise NotImplementedError

    def scale_dimension(self, dim, scale):
        return _scale_dimension(dim, scale)

    def _contributions(self) -> Dict[int, List[Tuple[int, nn.Module]]]:
        """new-state index -> [(source state j, op module)] in the reference's visit order (computed once: rows and _ops never
        change after construction; kept in __dict__, out of the module tree)."""
        contribs = self.__dict__.get("_contribs_cache")
        if contribs is None:
            selected = set(int(v) for v in np.asarray(self._rows())[:, 0])
            contribs = {}
            offset, n_states, ops_index = 0, 2, 0
            for _ in range(self._steps):
                lst = []
                for j in range(n_states):
                    if offset + j in selected:
                        lst.append((j, self._ops[ops_index]))
                        ops_index += 1
                contribs[n_states] = lst
                offset += n_states
                n_states += 1
            self.__dict__["_contribs_cache"] = contribs
        return contribs

    def _layout(self, s0_in_pre: bool) -> Tuple[Tuple[str, int], ...]:
        """(buffer, first channel) of every state: s0 in the cell's s0|s1 buffer "pre" (it went through pre_preprocess) or in its own
        tensor "s0", s1 in "pre", the last block_multiplier new states in the concat "cat", earlier ones in "scratch"."""
        C, first_cat = self.C_out, 2 + self._steps - self.block_multiplier
        return ((("pre", 0) if s0_in_pre else ("s0", 0)), ("pre", C)) + tuple(
            ("cat", (k - first_cat) * C) if k >= first_cat else ("scratch", (k - 2) * C) for k in range(2, 2 + self._steps))

    def _schedule(self, s0_in_pre: bool) -> tuple:
        """The cell's launches behind the preprocess stage as a tuple of Dual / Conv / Add / Copy steps: a property of the genotype
        rows, steps, block_multiplier and of whether s0 sits in the s0|s1 buffer; touches no tensor.  Cached per s0_in_pre."""
        cache = self.__dict__.setdefault("_schedule_cache", {})
        key = bool(s0_in_pre)
        if key not in cache:
            cache[key] = self._build_schedule(key)
        return cache[key]

    def _build_schedule(self, s0_in_pre: bool) -> tuple:
        contribs = self._contributions()
        where = self._layout(s0_in_pre)
        n_states = 2 + self._steps
        first_cat = n_states - self.block_multiplier             # first state that lands in the concat buffer
        steps: list = []
        written = {k: False for k in contribs}
        pending_id = {k: [j for (j, op) in lst if not isinstance(op, _ConvBR)] for k, lst in contribs.items()}
        for k, lst in contribs.items():
            if not lst:
                raise ValueError("Cell_3d: a step with no selected branch (the reference fails in torch.cat here too)")

        def finalize(k: int) -> None:
            ids = pending_id[k]
            while ids:
                if not written[k]:
                    if len(ids) >= 2:
                        steps.append(Add(ids[0], ids[1], k))
                        del ids[:2]
                    else:
                        steps.append(Copy(ids.pop(0), k))
                    written[k] = True
                else:
                    steps.append(Add(k, ids.pop(0), k))

        # Fast path: the conv branches from s0 and from s1 feed the same new states, nothing else does and they share a buffer
        # (e.g. the all-conv genotype): ONE dual-input launch computes relu(bn(conv(s0))) + relu(bn(conv(s1)))
        # for all of them, so the running sum never goes through HBM.
        done = set()
        a, b = ([(k, op) for k, lst in contribs.items() for (src, op) in lst if src == j and isinstance(op, _ConvBR)] for j in (0, 1))
        if (a and s0_in_pre and [k for k, _ in a] == [k for k, _ in b] and all(len(contribs[k]) == 2 for k, _ in a)
                and len({k >= first_cat for k, _ in a}) == 1):
            steps.append(Dual(tuple(op for _k, op in a), tuple(op for _k, op in b), tuple(k for k, _op in a)))
            for j, branches in enumerate((a, b)):
                for k, op in branches:
                    written[k] = True
                    done.add((j, id(op)))

        for j in range(n_states):
            if j >= 2:
                finalize(j)
            parts: Dict[Optional[str], list] = {}                        # residual buffer -> [(new state, op, residual state)]
            for k, lst in contribs.items():
                for (src, op) in lst:
                    if src != j or not isinstance(op, _ConvBR) or (j, id(op)) in done:
                        continue
                    if written[k]:
                        res = k                                          # running sum: accumulate in place
                    else:
                        ready = [i for i in pending_id[k] if i <= j]     # identity partner already complete
                        if ready:
                            pending_id[k].remove(ready[0])
                        res = ready[0] if ready else None
                    written[k] = True
                    parts.setdefault(None if res is None else where[res][0], []).append((k, op, res))
            for items in parts.values():
                # all destinations of one launch live in one buffer: a group that spans scratch and concat states splits
                by_buf: Dict[str, list] = {}
                for item in items:
                    by_buf.setdefault(where[item[0]][0], []).append(item)
                for sub in by_buf.values():
                    steps.append(Conv(j, tuple(op for (_k, op, _r) in sub), tuple(k for (k, _o, _r) in sub),
                                      None if sub[0][2] is None else tuple(r for (_k, _o, r) in sub)))
        for k in contribs:
            finalize(k)
        return tuple(steps)

    def _fused(self, mods: Sequence[ConvBR_3d]):
        """Concatenated packed weights / scale / shift of sibling convs (cached on their stamps)."""
        key = tuple(id(m) for m in mods)
        stamps = tuple(m.stamp() for m in mods)
        hit = self._fused_cache.get(key)
        if hit is None or hit[0] != stamps:
            prep = [m.prepared() for m in mods]
            if len(mods) == 1:
                fused = prep[0]
            else:
                # sibling convs as one stacked convolution: pack the concatenated raw weights (the packed layout has sections
                # that do not concatenate); BN scale / shift simply stack
                with torch.no_grad():
                    wk = ops.conv3d_k3_pack(torch.cat([m.conv.weight.detach() for m in mods]))
                fused = (wk, torch.cat([p[1] for p in prep]), torch.cat([p[2] for p in prep]))
            hit = (stamps, fused)
            self._fused_cache[key] = hit
        return hit[1]

    def _convbrs(self):
        """the ConvBR units of this cell (cached: the module tree of a cell never changes after construction)."""
        units = self.__dict__.get("_convbr_cache")
        if units is None:
            units = [m for m in self.modules() if isinstance(m, _ConvBR)]
            self.__dict__["_convbr_cache"] = units
        return units

    def forward_parameters(self) -> list:
        """The parameters forward() reads: preprocess, pre_preprocess unless prev_prev already has C_out channels (it is skipped
        then, rag_model.py:150-151), and the conv branches of the genotype (every new state is concatenated into the output)."""
        out = self.preprocess.forward_parameters()
        if self.C_prev_prev != self.C_out:
            out += self.pre_preprocess.forward_parameters()
        for lst in self._contributions().values():
            for _j, op in lst:
                if isinstance(op, _ConvBR):
                    out += op.forward_parameters()
        return out

    def autograd_mode(self, *inputs) -> bool:
        units = self._convbrs()
        if torch.is_grad_enabled():
            if any(t is not None and t.requires_grad for t in inputs):
                return True
            if any(m.conv.weight.requires_grad or m.bn.weight.requires_grad or m.bn.bias.requires_grad for m in units):
                return True
        return any(m.use_bn and m.bn.training for m in units)

    def forward(self, prev_prev_input, prev_input):
        run = self._run_autograd if self.autograd_mode(prev_prev_input, prev_input) else self._run
        if prev_input.dim() == 4:     # 2-D cell: run on depth-1 volumes
            return prev_input, run(prev_prev_input.unsqueeze(2), prev_input.unsqueeze(2)).squeeze(2)
        return prev_input, run(prev_prev_input, prev_input)

    def _run_autograd(self, prev_prev_input, prev_input):
        """The reference's forward node by node (rag_model.py:143-177) on the autograd Functions."""
        s0, s1 = prev_prev_input, prev_input
        if self.downup_sample != 0:
            s1 = ag.resample(s1, self.out_size(s1.shape[2:]), True)
        s0 = ag.resample(s0, s1.shape[2:], True)
        if s0.shape[1] != self.C_out:
            s0 = self.pre_preprocess(s0)
        s1 = self.preprocess(s1)
        states = [s0, s1]
        contribs = self._contributions()
        n_states = 2 + self._steps
        pending: Dict[int, list] = {k: [] for k in contribs}
        for k, lst in contribs.items():
            if not lst:
                raise ValueError("Cell_3d: a step with no selected branch (the reference fails in torch.cat here too)")
        # Sources in ascending order: state j is complete once every source < j has been applied (targets are always
        # later states).  The conv branches leaving one state run as ONE stacked convolution (ag.ConvBRGroupFn).
        for j in range(n_states):
            if j >= 2:
                acc = pending[j][0]
                for h in pending[j][1:]:
                    acc = ag.AddFn.apply(acc, h)
                states.append(acc)
            out_ops = [(k, op) for k, lst in contribs.items() for (src, op) in lst if src == j]
            convs = [(k, op) for (k, op) in out_ops if isinstance(op, _ConvBR)]
            grouped = (len(convs) > 1 and all(op._geometry() == 3 and op.use_bn and op.relu for _k, op in convs)
                       and states[j].dtype == torch.float32)
            if grouped:
                params = [p for _k, op in convs for p in (op.conv.weight, op.bn.weight, op.bn.bias)]
                # every target already holding exactly one contribution: hand it to the group as that unit's residual, the sum
                # then comes out of the BatchNorm + ReLU pass (no add launch, no extra tensor)
                fuse = all(len(pending[k]) == 1 and pending[k][0].dtype == torch.float32 for k, _op in convs)
                res = [pending[k][0] for k, _op in convs] if fuse else []
                outs = dict(zip([k for k, _op in convs],
                                ag.ConvBRGroupFn.apply(states[j], tuple(op for _k, op in convs), *params, *res)))
                if fuse:
                    for k, _op in convs:
                        pending[k].clear()
            for k, op in out_ops:
                pending[k].append(outs[k] if (grouped and isinstance(op, _ConvBR)) else op(states[j]))
        return torch.cat(states[-self.block_multiplier:], dim=1)

    def out_size(self, prev_size: Sequence[int]) -> Tuple[int, int, int]:
        """Spatial size this cell works at (and outputs) given the size of prev_input."""
        if self.downup_sample == 0:
            return tuple(int(v) for v in prev_size)
        return tuple(self.scale_dimension(int(v), self.scale) for v in prev_size)

    def dual_branches(self, s0_in_pre: bool):
        """(a, b, whole): the conv branches leaving s0 and s1 as [(new state k, op)] when they run as ONE dual launch — both feed
        the same new states, nothing else feeds those, and they share a buffer — else (None, None, False); `whole`: that launch produces
        every new state of the cell, so consumer tails can ride on it.  A property of the genotype and of whether s0 sits in the
        cell's s0|s1 buffer (it went through pre_preprocess, here or as its producer's tail)."""
        first = self._schedule(s0_in_pre)[0]      # (the schedule decides; a Dual step is always its first)
        if not isinstance(first, Dual):
            return None, None, False
        a, b = list(zip(first.dst_states, first.a_mods)), list(zip(first.dst_states, first.b_mods))
        return a, b, len(a) == self._steps and self.block_multiplier == self._steps

    def _one_launch_2d(self, s0, s1, size) -> bool:
        """A Cell_2d in which every new state is conv(s0) + conv(s1) (the all-conv genotype) can run as ONE launch — the two 1x1
        ConvBRs and their bilinear resamples in the staging of the dual 3x3 launch (ragmi_cell2d_fwd); s0 / s1 are never written.
        The shape / dtype / precision half of that condition (the caller knows whether the cell is one dual launch).  Both INPUTS must
        be depth-1 volumes too: the launch resamples in 2-D, and a Cell_3d that ends at depth 1 may read a deeper input (cell 5 of the
        Matching Net on a d = 4 cost volume reads T[3] at depth 2)."""
        C, (D, H, W) = self.C_out, size
        return (D == 1 and s0.shape[2] == 1 and s1.shape[2] == 1 and s0.shape[1] != C
                and s1.dtype == torch.float32 and s0.dtype == torch.float32
                and ops.get_conv_precision() == "f16x3" and ops.cell2d_supported(C, s0.shape[1], s1.shape[1], C * self._steps, H, W))

    def _run(self, prev_prev_input, prev_input, plan: Optional["_CellPlan"] = None, pre: Optional[torch.Tensor] = None,
             tails: Optional[Sequence["ops.Tail"]] = None):
        """forward() plus the cross-cell fusion of MatchingNet._run_chain: `plan` is this cell's slice of the chain plan (None: a
        stand-alone cell — nothing arrives fused, everything is stored), `pre` the [B, 2C, ...] buffer in which s0 (ch 0..C) and /
        or s1 (ch C..2C) have already been written as `plan.has` says, `tails` the consumer 1x1x1 convs the plan put on THIS
        cell's dual launch (`plan.tails`).  Returns the concat, or None when the plan does not store it."""
        C = self.C_out
        if C % 4 != 0 or self.block_multiplier > self._steps:
            raise NotImplementedError("rag_amd.Cell_3d: filter_multiplier must be a multiple of 4 and "
                                      "block_multiplier <= steps (true for every cell the reference builds)")
        s0, s1 = prev_prev_input, prev_input
        pre_has = plan.has if plan is not None else (False, False)
        s0_in_pre = pre_has[0] or s0.shape[1] != C
        a, b, whole = self.dual_branches(s0_in_pre)
        if plan is None:
            plan = _CellPlan(size=self.out_size(s1.shape[2:]), dtype=s1.dtype, has=pre_has, g4=False, dual=whole, store_main=True, tails=False,
                             shared_pre=False, quarter=False)
        # the trilinear resamples (rag_model.py:146-153) are fused into the 1x1x1 preprocess convs that consume them
        size = tuple(int(v) for v in plan.size)
        if not pre_has[0] and s0.shape[1] == C and tuple(s0.shape[2:]) != size:
            s0 = ops.trilinear3d(s0, size, True)     # no pre_preprocess to fuse into (never the case in Network)
        D, H, W = size
        if whole and pre is None and not tails and plan.store_main and self._one_launch_2d(s0, s1, size):
            cat = torch.empty((s1.shape[0], self.block_multiplier * C, D, H, W), device=s1.device, dtype=s1.dtype)
            pa, sa, ha = self._fused([op for _k, op in a])
            pb, sb, hb = self._fused([op for _k, op in b])
            groups = [(k - 2) * C + 4 * g for k, _op in a for g in range(C // 4)]
            ops.cell2d(s0, self.pre_preprocess.prepared() + (self.pre_preprocess.relu,), s1,
                       self.preprocess.prepared() + (self.preprocess.relu,), C, pa, sa, ha, pb, sb, hb, C * self._steps, True, cat, groups)
            return cat
        if pre is None:
            pre = torch.empty((s1.shape[0], 2 * C, D, H, W), device=s1.device, dtype=plan.dtype)
        B, dev, adt = pre.shape[0], pre.device, pre.dtype
        cat = (pre if not plan.store_main else   # placeholder pointer: nothing is stored when the output is only consumed by tails
               torch.empty((B, self.block_multiplier * C, D, H, W), device=dev, dtype=adt))
        scratch = (torch.empty((B, (self._steps - self.block_multiplier) * C, D, H, W), device=dev, dtype=adt)
                   if self.block_multiplier < self._steps else None)

        # an UP-sampled input runs conv-first through the ConvBR forward (channel mix on the small volume); everything else —
        # down-sampling or an input already at the cell's size — shares one paired launch (measured: splitting an
        # identity + down-sampling pair into two launches costs 43 us instead of 27)
        grows = any(s is not None and _volume(size) > _volume(s.shape[2:]) and C <= s.shape[1] for s in (s0, s1))
        if not pre_has[0] and not pre_has[1] and s0.shape[1] != C and not grows and s0.dtype == s1.dtype == adt:
            # both 1x1x1 convs (each with its own fused resample) as ONE launch
            w0, sc0, sh0 = self.pre_preprocess.prepared()
            w1, sc1, sh1 = self.preprocess.prepared()
            ops.conv3d_k1_resample_pair([(s0, w0, sc0, sh0, self.pre_preprocess.relu, 0),
                                         (s1, w1, sc1, sh1, self.preprocess.relu, C)], size, pre)
        else:
            if not s0_in_pre:
                s0 = s0.contiguous()
            elif not pre_has[0]:               # (else: already written by the producer of prev_prev_input, a fused tail)
                self.pre_preprocess(s0, out=pre, out_ch0=0, resample_to=size)
            if not pre_has[1]:
                self.preprocess(s1, out=pre, out_ch0=C, resample_to=size)
        self._issue(s0_in_pre, {"pre": pre, "s0": s0, "scratch": scratch, "cat": cat}, plan, tails)
        return cat if plan.store_main else None      # (not stored: the concat existed only inside the kernel, for its tails)

    def _issue(self, s0_in_pre: bool, buffers: Dict[str, Optional[torch.Tensor]], plan: "_CellPlan", tails) -> None:
        """Launch the schedule on the buffers of _layout: the only place of the cell that launches a 3x3x3 conv or an add (as
        attributes of `ops` at call time: the benchmark wraps them)."""
        C, pre = self.C_out, buffers["pre"]
        where = [(buffers[name], ch) for (name, ch) in self._layout(s0_in_pre)]
        for step in self._schedule(s0_in_pre):
            if isinstance(step, Dual):
                pa, sa, ha = self._fused(step.a_mods)
                pb, sb, hb = self._fused(step.b_mods)
                groups = [where[k][1] + 4 * g for k in step.dst_states for g in range(C // 4)]
                ops.conv3d_k3_dual(pre, C, pa, sa, ha, pb, sb, hb, C * len(step.dst_states), True, where[step.dst_states[0]][0], groups,
                                   tails=tails, store_main=plan.store_main, x_g4=plan.g4, quarter=plan.quarter)
            elif isinstance(step, Conv):
                xbuf, xch = where[step.src]
                packed, scale, shift = self._fused(step.mods)
                out_groups = [where[k][1] + 4 * g for k in step.dst_states for g in range(C // 4)]
                res_buf = res_groups = None
                if step.res_states is not None:
                    res_buf = where[step.res_states[0]][0]
                    res_groups = [where[r][1] + 4 * g for r in step.res_states for g in range(C // 4)]
                ops.conv3d_k3(xbuf[:, xch:xch + C], packed, C * len(step.mods), scale, shift, True, where[step.dst_states[0]][0], out_groups,
                              res_buf, res_groups)
            elif isinstance(step, Add):
                (ba, ca), (bb, cb), (buf, ch) = where[step.a], where[step.b], where[step.dst]
                ops.add(ba, ca, bb, cb, buf, ch, C)
            else:
                (bs, cs), (buf, ch) = where[step.src], where[step.dst]
                torch.mul(bs[:, cs:cs + C], 1, out=buf[:, ch:ch + C])   # lone identity: a copy KERNEL (no memcpy node when captured)


class Cell_3d(_Cell):
    """src/models/rag_model.py:114-177: forward(prev_prev_input, prev_input) -> (prev_input, concat); ops from genotype.reduce."""
    CONV, OPS, PRIMS = ConvBR_3d, OPS_3d, PRIMITIVES_3D

    def _rows(self):
        return self.genotype.reduce


class Cell_2d(_Cell):
    """src/models/rag_model.py:47-111 (Feature Net cell; ops from genotype.normal) on the same executor."""
    CONV, OPS, PRIMS = ConvBR_2d, OPS_2d, PRIMITIVES

    def _rows(self):
        return self.genotype.normal


# Matching-Net macro architecture, src/models/rag_model.py:238-261:
# (prev_prev_fmultiplier, prev_filter_multiplier, filter_multiplier, downup_sample)
_CELL3D_ARCH = ((4, 4, 4, 0), (4, 4, 4, 0), (4, 4, 4, 0), (4, 4, 8, -1),
                (4, 8, 16, -1), (8, 16, 8, 1), (16, 8, 16, -1), (8, 16, 16, 0))


# What the fused executor (MatchingNet._run_chain) does at one shape, as data.  Tensors: T[-2] = stem3d0's output, T[-1] = stem3d1's,
# T[i] = cell i's; cell i reads T[i-2] (prev_prev, role 0) and T[i-1] (prev, role 1).
#   _CellPlan: size / dtype of the cell's s0|s1 buffer and of its output; has = which halves of that buffer are written before the cell
#   runs (fused tails, shared_pre); g4 = the buffer is channel-group-interleaved; dual = one dual launch produces every new state
#   (_Cell.dual_branches); store_main = the concat is written; tails = its consumers ride on that launch (else they run as plain 1x1x1
#   launches behind it); shared_pre = its two 1x1x1 convs and cell i+1's pre_preprocess run as one launch in front of it; quarter = its
#   stored concat is read only by a x0.25 resample two cells on, and the launch skips the planes and rows that resample never reads.
#   _ChainPlan: sizes[i], cdt[i] (storage type), consumers[i] = ((cell j, role, down), ...) fused onto T[i]'s producer, stored[i] for
#   i = -2 .. n-1; cells = the _CellPlans; stem0_g4 = T[-2] is G4; stems_fused = both stems as one call (T[-2] never written);
#   stem_tail_rows = cell 0's pre_preprocess in the idle rows of stem3d1's matrix product.
#   _HeadPlan (_plan_head; rag_model.py:353-366): level = the last cell's output is at 1/1, 1/2 or 1/4 of the volume; at 1/4: cross_f32 =
#   last_12_3d is the bf16 -> fp32 crossing launch, chain = last_12_3d and last_6_3d's channel mix as one launch (then the resample + ReLU)
#   instead of the two units; upconv = upsample_6 + last_3_3d as one kernel.
_CellPlan = namedtuple("_CellPlan", "size dtype has g4 dual store_main tails shared_pre quarter")
_ChainPlan = namedtuple("_ChainPlan", "sizes cdt consumers stored cells stem0_g4 stems_fused stem_tail_rows")
_HeadPlan = namedtuple("_HeadPlan", "level cross_f32 chain upconv")


def _down_tail_ok(prod, cons, B, src, dst, src_dt, dst_dt) -> bool:
    """cell `cons`' 1x1x1 conv on the output of cell `prod` as DOWN-SAMPLING tails of `prod`: `cons` works at exactly half of that size, the
    source pairs of that x0.5 resampling are aligned, and the producer is a level-3 dual launch with 12 output channels on the z-marching
    split-operand kernel (fp32 storage under the default precision, or bf16 storage) — the only form that takes them.  A bf16 producer
    may write fp32 down-sampling tails (RAGMI_TAIL_F32); nothing else crosses storage types."""
    return ((src_dt != torch.float32 or ops.get_conv_precision() == "f16x3")
            and (dst_dt == src_dt or (src_dt == torch.bfloat16 and dst_dt == torch.float32))
            and tuple(2 * v for v in dst) == tuple(src) and ops.down2_tail_supported(*src)
            and cons.C_out <= 8 and cons.C_out % 4 == 0 and prod.downup_sample == 0 and prod.C_out == 4 and prod.C_out * prod._steps <= 16
            and ops.conv3d_k3_uses_x3(2 * prod.C_out, prod.C_out * prod._steps, B, *src, nset=2, ntail=1, dtype=src_dt))


def _plan_chain(stem0, stem1, cells, B: int, C_fea: int, vol, adt: torch.dtype, folded: bool) -> _ChainPlan:
    """Every decision of the fused executor for stem3d0 -> stem3d1 -> cells (rag_model.py:341-351) on a [B, ., *vol] cost volume stored as
    `adt` (`folded`: stem3d0 consumes the [B, C_fea, h, w] feature maps instead of the volume).  Reads module structure, the ops switches
    and the library's host predicates; touches no tensor and launches nothing."""
    n = len(cells)
    f32, bf16 = torch.float32, torch.bfloat16
    caps = ops.conv3d_k3_g4_caps
    x3 = (adt == f32 and ops.get_conv_precision() == "f16x3") or adt == bf16      # the split-operand kernels: what G4 and the fused stems need
    # Sizes, and the storage type per cell (mixed storage): under bf16 storage only the FULL-RESOLUTION tensors stay bf16 — a cell that
    # works below the cost volume's resolution (at most 1/ratio of its voxels), and every cell behind one, keeps fp32
    # (ops.set_bf16_deep_fp32: the level-12 cells and the head carry most of the bf16 error, the deep levels ~4 % of the bytes;
    # tests/analysis_bf16_stage_epe.py).  The edges that cross are bf16 -> fp32 only: down-sampling tails (RAGMI_TAIL_F32) and the
    # resample + 1x1x1 launch (RAGMI_OUT_F32).
    sizes, cdt = {-2: tuple(vol), -1: tuple(vol)}, {-2: adt, -1: adt}
    cout = {-2: stem0.conv.out_channels, -1: stem1.conv.out_channels}       # channels of T[i]
    for i, c in enumerate(cells):
        sizes[i] = c.out_size(sizes[i - 1])
        deep = adt == bf16 and ops.bf16_deep_fp32_enabled() and (
            _volume(sizes[i]) * ops.bf16_deep_fp32_ratio() <= _volume(vol) or f32 in (cdt[i - 1], cdt[i - 2]))
        cdt[i] = f32 if deep else adt
        cout[i] = c.block_multiplier * c.C_out

    # Consumers of T[i] that can ride on its producer: a 4-channel 1x1x1 conv at the producer's size and storage type as a full-resolution
    # tail, one a level down as down-sampling tails.  A prev_prev edge skips a module, which must keep the size (for cell 0 that is
    # stem3d1), and exists only where the consumer has a pre_preprocess to run.
    consumers = {}
    for i in range(-2, n):
        found = []
        for j, role in ((i + 1, 1), (i + 2, 0)):
            c = cells[j] if 0 <= j < n else None
            # (a prev_prev edge across a resampling cell is at another size than T[i] and never rides as a tail.  Where that size is
            # exactly a quarter — cell 4 on T[2] — the edge is served by the quarter store below instead: T[i] stays a stored tensor,
            # but only the planes and rows that x0.25 resample reads are written)
            if c is None or (role == 0 and (c.C_prev_prev == c.C_out or (j > 0 and cells[j - 1].downup_sample != 0))):
                continue
            if c.downup_sample == 0 and c.C_out == 4 and cdt[j] == cdt[i]:
                found.append((j, role, False))
            elif c.downup_sample == -1 and i >= 0 and _down_tail_ok(cells[i], c, B, sizes[i], sizes[j], cdt[i], cdt[j]):
                found.append((j, role, True))
        consumers[i] = tuple(found)
    nfull = {i: sum(not d for (_j, _r, d) in consumers[i]) for i in consumers}                                  # tails of T[i]'s producer launch
    ndown = {i: sum((cells[j].C_out + 3) // 4 for (j, _r, d) in consumers[i] if d) for i in consumers}
    # one dual launch per cell (s0 sits in the s0|s1 buffer when it arrives as a tail or goes through pre_preprocess), which then takes tails
    dual = [c.dual_branches((i, 0, False) in consumers[i - 2] or (i, 0, True) in consumers[i - 2] or cout[i - 2] != c.C_out)[2]
            for i, c in enumerate(cells)]
    tails = {i: bool(consumers[i]) and dual[i] and cout[i] <= 16 for i in range(n)}
    tails[-2] = tails[-1] = True      # (the stems always apply theirs)

    # G4: which of the private level-3 tensors are stored channel-group-interleaved ([B][C/4][D][H][W][4], include/rag_amd.h) instead of as
    # channel planes.  Cell j's s0|s1 buffer can be G4 when cell j runs as ONE dual launch on the kernel that reads G4 (caps bit 0) and BOTH
    # halves arrive as full-resolution tails from producers that can write G4 (bit 1; stem3d0 folded with the cost volume always can).
    # The full-resolution tails of one producer launch share a layout, so candidates are withdrawn until every producer is consistent.
    # T[-2] can be G4 when nothing but stem3d1 and fused tails reads it.  Everything else, and every module boundary, stays planes.
    g4_ok = x3 and ops.g4_enabled()
    writes = {i: bool(g4_ok and nfull[i] and tails[i]
                      and caps(2 * c.C_out, cout[i], B, *sizes[i], nset=2, ntail=nfull[i], ndown=ndown[i], dtype=cdt[i]) & 2)
              for i, c in enumerate(cells)}
    writes[-2] = bool(g4_ok and nfull[-2] and (folded or caps(stem0.conv.in_channels, cout[-2], B, *vol, nset=1, ntail=nfull[-2], dtype=adt) & 2))
    writes[-1] = bool(g4_ok and nfull[-1] and caps(cout[-2], cout[-1], B, *vol, nset=1, ntail=nfull[-1], dtype=adt) & 2)
    g4 = [bool((j, 1, False) in consumers[j - 1] and (j, 0, False) in consumers[j - 2] and writes[j - 1] and writes[j - 2] and dual[j]
               and caps(2 * c.C_out, cout[j], B, *sizes[j], nset=2, ntail=nfull[j] if tails[j] else 0, ndown=ndown[j] if tails[j] else 0,
                        dtype=cdt[j]) & 1) for j, c in enumerate(cells)]
    changed = True
    while changed:          # one layout per producer launch
        changed = False
        for i in range(-2, n):
            js = [j for (j, _r, d) in consumers[i] if not d]
            if len({g4[j] for j in js}) > 1:
                for j in js:
                    g4[j] = False
                changed = True
    # stem3d0's own output is read by stem3d1 (3x3x3) and by cell 0's pre_preprocess tail only
    alone = folded and (0, 0, False) in consumers[-2]
    stem0_g4 = bool(g4_ok and alone and caps(cout[-2], cout[-1], B, *vol, nset=1, ntail=nfull[-1], dtype=adt) & 1)
    stems_fused = bool(x3 and alone and ops.stem_fusion_enabled() and cout[-2] == 12 and stem1._geometry() == 3 and not stem1._small()
                       and ops.costvol_stem_conv3d_supported(C_fea, 12, cout[-1], B, *vol, ntail=nfull[-1], dtype=adt))
    # (that one tail has four output channels — a full-resolution consumer always has — so it fits rows 12..15 of a 12-channel stem3d1)
    stem_tail_rows = stems_fused and ops.stem_tail_rows_enabled() and cout[-1] == 12

    # a main output is stored unless every reader is a tail of its producer (the head reads the last one)
    stored = {i: i == n - 1 or not tails[i] or len(consumers[i]) < sum(0 <= j < n for j in (i + 1, i + 2)) for i in range(-1, n)}
    stored[-2] = not stems_fused
    # Quarter store: T[i] is stored for ONE reader, cell i+2's pre_preprocess behind a x0.25 trilinear resample (cell i+1, one level down,
    # rides on T[i]'s producer as down-sampling tails), and its producer is the launch that can skip what that resample never reads
    # (ops.quarter_store_supported: fp32 storage under f16x3, a 12-channel level-3 dual launch, aligned axes and work items)
    quarter = {i: bool(ops.quarter_store_enabled() and 0 <= i and i + 2 < n and stored[i] and tails[i] and dual[i]
                       and consumers[i] == ((i + 1, 1, True),) and cdt[i] == cdt[i + 2] == f32 and ops.get_conv_precision() == "f16x3"
                       and cells[i + 2].C_prev_prev != cells[i + 2].C_out
                       and tuple(4 * v for v in sizes[i + 2]) == tuple(sizes[i])
                       and ops.quarter_store_supported(2 * cells[i].C_out, cout[i], B, *sizes[i], nset=2, ntail=0, ndown=ndown[i], dtype=cdt[i]))
               for i in range(n)}
    has = [[False, False] for _ in cells]
    plans = []
    for i in range(-2, n):
        if i >= 0:
            # shared_pre: cells i and i+1 both resample T[i-1] to the SAME size and nothing of either buffer is there yet — one launch for
            # cell i's two 1x1x1 convs and cell i+1's pre_preprocess (not across storage types, and not for an up-sampling input, which
            # runs conv-first with its cell)
            j = i + 1
            shared = (j < n and not any(has[i]) and not has[j][0] and sizes[i] == sizes[j] != sizes[i - 1] and stored[i - 2] and stored[i - 1]
                      and cout[i - 2] != cells[i].C_out and cout[i - 1] != cells[j].C_out and len({cdt[i - 2], cdt[i - 1], cdt[i], cdt[j]}) == 1
                      and _volume(sizes[i]) <= min(_volume(sizes[i - 2]), _volume(sizes[i - 1])))
            if shared:
                has[i], has[j][0] = [True, True], True
            plans.append(_CellPlan(sizes[i], cdt[i], tuple(has[i]), g4[i], dual[i], stored[i], tails[i], shared, quarter[i]))
        for (j, role, _d) in consumers[i]:
            has[j][role] = True
    ro = MappingProxyType
    return _ChainPlan(ro(sizes), ro(cdt), ro(consumers), ro(stored), tuple(plans), stem0_g4, stems_fused, stem_tail_rows)


def _plan_head(vol, last_size, last_dtype, m3, m6, m12, train: bool) -> _HeadPlan:
    """Every decision of the head (rag_model.py:353-366) on a `vol` = (d, h, w) cost volume whose last cell's output has spatial size
    `last_size` and storage type `last_dtype`.  `train`: a head unit runs its autograd form, which takes none of the fused launches.
    `m3` None: the caller applies its own last_3_3d (the depth head), no upconv.  Pure, like _plan_chain: reads the units' geometry, the
    ops switches and the library's host predicates."""
    d, h, w = (int(v) for v in vol)
    half = (max(d // 2, 1), h // 2, w // 2)      # (a depth-1 volume, the 2-D networks', keeps its one plane)
    last_size = tuple(int(v) for v in last_size)
    if last_size[1] == h:
        return _HeadPlan(1, False, False, False)
    if last_size[1] == h // 2:
        level = 2
    elif last_size[1] == h // 4:
        level = 4
    else:
        # the reference reaches `return mat` with mat unbound here (UnboundLocalError)
        raise ValueError("MatchingNet: feature height must be a multiple of 4 (input H a multiple of 12)")
    # bf16 storage: the head keeps fp32 from its first 1x1x1 conv on (the crossing launch: RAGMI_BF16 | RAGMI_OUT_F32)
    cross = (level == 4 and last_dtype == torch.bfloat16 and ops.bf16_head_fp32_enabled() and not (train and m12.autograd_mode())
             and m12._geometry() == 1)
    # last_12_3d and the channel mix of last_6_3d (conv-first, as ConvBR.forward runs an up-sampling 1x1x1) as ONE launch
    chain = (level == 4 and not cross and not train and m12._geometry() == 1 and m6._geometry() == 1 and ops.chain_k1_enabled()
             and _volume(half) > _volume(last_size) and m6.conv.out_channels <= m6.conv.in_channels
             and ops.conv3d_k1_chain_supported(m12.conv.in_channels, m12.conv.out_channels, m6.conv.out_channels))
    # upsample_6 + last_3_3d as ONE kernel when the upsampling is an exact factor 2 (always, for the sizes the reference accepts)
    upconv = (m3 is not None and not train and m3._small() and m3.conv.out_channels == 1 and (level == 4 or last_size == half)
              and (d, h, w) == tuple(2 * v for v in half) and ops.upconv3d_c1_supported(m6.conv.out_channels, *half))
    return _HeadPlan(level, bool(cross), bool(chain), bool(upconv))


def _plan_head_taps(plan: _HeadPlan, vol, last_size, last_dtype, m3, m6) -> bool:
    """Whether the head takes last_3_3d's channel sum BEFORE upsample_6 (rag_model.py:269, 357-365): the 1/4-level step's resample
    launch mixes last_6_3d's channels into the 27 tap volumes (ops.trilinear3d_act_k1) and ops.uptaps3d sums their 27 shifted x2
    samples, instead of trilinear3d_act -> upconv3d_c1.  Only where `plan` ends the 1/4-level step in that resample launch (chain) and
    runs the fused head kernel (upconv: inference, one output channel, exact factor 2) on an fp32 `low`.  Pure, like _plan_head."""
    if not (ops.head_taps_enabled() and plan.level == 4 and plan.chain and plan.upconv and m3 is not None and m3.conv.out_channels == 1
            and last_dtype == torch.float32):
        return False
    d, h, w = (int(v) for v in vol)
    half = (d // 2, h // 2, w // 2)
    return bool(ops.trilinear3d_act_k1_supported(m6.conv.out_channels, 27, tuple(int(v) for v in last_size), half, True)
                and ops.uptaps3d_supported(*half))


def _plan_head_xblend(plan: _HeadPlan, vol, last_size, last_dtype, m3, m6) -> bool:
    """Whether the tap form of the head (_plan_head_taps) blends the taps along x in the resample launch: it writes the nine x-blended
    row volumes Q [B, 9, d/2, h/2, w] (ops.trilinear3d_act_k1(xblend=True)) and ops.uptaps3d(xblended=True) is left the y and z
    blends.  Only where the tap form runs and both launches take the shape.  Pure, like _plan_head."""
    if not (ops.head_xblend_enabled() and _plan_head_taps(plan, vol, last_size, last_dtype, m3, m6)):
        return False
    d, h, w = (int(v) for v in vol)
    half = (d // 2, h // 2, w // 2)
    return bool(ops.trilinear3d_act_k1_supported(m6.conv.out_channels, 27, tuple(int(v) for v in last_size), half, True, xblend=True)
                and ops.uptaps3d_supported(*half, xblended=True))


def _head_quarter(last5, m12, m6, half, plan: _HeadPlan, taps_weight=None, xblend: bool = False) -> torch.Tensor:
    """The head's 1/4-level step, last_6_3d(upsample_12(last_12_3d(last5))) at `half` (upsample_12 is fused into last_6_3d's 1x1x1
    kernel, conv-first), launched as `plan` says; shared by MatchingNet._head and depth.Network._trunk.  `taps_weight` (_plan_head_taps:
    last_3_3d's raw [1, C, 3, 3, 3] weight): the resample launch returns that convolution's 27 tap volumes instead, or with `xblend`
    (_plan_head_xblend) their nine x-blended row volumes."""
    B, dev = last5.shape[0], last5.device
    if plan.chain:
        w1, s1, h1 = m12.prepared()
        w2, s2, h2 = m6.prepared()
        low = torch.empty((B, m6.conv.out_channels) + tuple(last5.shape[2:]), device=dev, dtype=last5.dtype)
        ops.conv3d_k1_chain(last5, w1, s1, h1, m12.relu, w2, s2, h2, False, low)
        if taps_weight is not None:
            return ops.trilinear3d_act_k1(low, half, True, m6.relu, taps_weight, transposed=True, xblend=xblend)
        y = torch.empty((B, m6.conv.out_channels) + tuple(half), device=dev, dtype=last5.dtype)
        ops.trilinear3d_act(low, half, True, m6.relu, y, 0)
        return y
    if plan.cross_f32:
        y12 = m12(last5, out=torch.empty((B, m12.conv.out_channels) + tuple(last5.shape[2:]), device=dev, dtype=torch.float32))
    else:
        y12 = m12(last5)
    return m6(y12, resample_to=half)


class MatchingNet(nn.Module):
    """The Matching-Net half of the reference `Network` (src/models/rag_model.py:230-275, 325-387).

    forward(left_fea[B,C,h,w], right_fea[B,C,h,w], task_arch=None) -> disp[B,3h,3w] wraps the three
    hot pieces the reference runs inline: cost-volume loop (:375-383) -> matching() (:325-366) ->
    Disp (:32-44).  Sub-module names (stem3d0, stem3d1, cells_3d, last_3_3d, last_6_3d, last_12_3d,
    disp) and therefore state_dict keys are the reference's; units are nn.ModuleLists indexed by
    task_arch[name][0] exactly like Network.matching.  `maxdisp` is a ctor argument (the reference
    hard-codes 192, rag_model.py:274).
    """

    def __init__(self, genotype=ALL_CONV_GENOTYPE, maxdisp: int = 192):
        super().__init__()
        self._init_matching(genotype, maxdisp)

    def _init_matching(self, genotype, maxdisp):
        self._step = 3
        self._block_multiplier = 3
        self._filter_multiplier = 4
        self._num_layers_3d = 8
        initial_fm = self._filter_multiplier * self._block_multiplier
        if not hasattr(self, "length"):
            self.length, self.arch_init = {}, {}
        for name in ("stem_3d0", "stem_3d1", "last_3_3d", "last_6_3d", "last_12_3d"):
            self.length[name] = 1
            self.arch_init[name] = [0]
        self.cells_3d = nn.ModuleList()
        self.stem3d0 = nn.ModuleList([ConvBR_3d(initial_fm * 2, initial_fm, 3, stride=1, padding=1)])
        self.stem3d1 = nn.ModuleList([ConvBR_3d(initial_fm, initial_fm, 3, stride=1, padding=1)])
        for i in range(self._num_layers_3d):
            self.cells_3d.append(nn.ModuleList([self._new_cell_3d(i, genotype)]))
            self.arch_init["cell_3d" + str(i)] = [0]
            self.length["cell_3d" + str(i)] = 1
        self.last_3_3d = nn.ModuleList([ConvBR_3d(initial_fm, 1, 3, 1, 1, bn=False, relu=False)])
        self.last_6_3d = nn.ModuleList([ConvBR_3d(initial_fm * 2, initial_fm, 1, 1, 0)])
        self.last_12_3d = nn.ModuleList([ConvBR_3d(initial_fm * 4, initial_fm * 2, 1, 1, 0)])
        self.maxdisp = maxdisp
        self.disp = Disp(self.maxdisp)

    def _new_cell_3d(self, i: int, genotype) -> Cell_3d:
        pp, p, fm, du = _CELL3D_ARCH[i]
        return Cell_3d(self._step, self._block_multiplier, pp, p, genotype, fm, du)

    # -- rag_model.py:325-366
    def matching(self, x, task_arch, path=None, features=None):
        """`features=(left_fea, right_fea)` with x=None: the cost volume is not built; stem3d0 consumes the feature maps
        directly (ragmi_costvol_stem_fwd) — inference only, same result as matching(cost_volume(...))."""
        def unit(name):
            return task_arch[name][0] if task_arch is not None else None

        cells = []
        for i, cell in enumerate(self.cells_3d):
            arch_cell = None
            if task_arch is not None:
                arch_cell = task_arch["cell_3d" + str(i)][0]
            elif path is not None:
                arch_cell = path[i + 1]
            cells.append(cell[arch_cell])
        last = self._run_chain(x, self.stem3d0[unit("stem_3d0")], self.stem3d1[unit("stem_3d1")], cells, features)
        return self._head(self._vol_size(x, features), last, unit("last_3_3d"), unit("last_6_3d"), unit("last_12_3d"))

    # -- rag_model.py:663-685
    def search_matching(self, x, selected_ops, t, features=None):
        cells = [cell[selected_ops[i + 10]] for i, cell in enumerate(self.cells_3d)]
        last = self._run_chain(x, self.stem3d0[selected_ops[8]], self.stem3d1[selected_ops[9]], cells, features)
        return self._head(self._vol_size(x, features), last, t, t, t)

    def _vol_size(self, x, features):
        if x is not None:
            return tuple(x.shape[2:])
        return (int(self.maxdisp / 3),) + tuple(features[0].shape[2:])

    def _run_chain(self, x, stem0, stem1, cells, features=None):
        """stem3d0 -> stem3d1 -> cells (rag_model.py:341-351) with cross-module fusion: the 1x1x1 pre_preprocess /
        preprocess conv of a cell that needs no resampling is computed in the epilogue of the kernel that PRODUCES its
        input (a "tail"), and a tensor consumed only by tails is never written to HBM.  Tensors: T[-2] = stem0 output,
        T[-1] = stem1 output, T[i] = output of cell i; cell i reads T[i-2] (prev_prev) and T[i-1] (prev).  Inference: `_plan_chain`
        decides everything up front (per call: it reads the ops switches); the code below allocates and launches what the plan says."""
        train = (stem0.autograd_mode(*(features if x is None else (x,))) or stem1.autograd_mode()
                 or any(c.autograd_mode() for c in cells))
        if x is None and (train or not stem0.costvol_fusable(features[0].shape[1])):
            x = self.cost_volume(*features)
        if train:
            out = (stem0(x),)                     # training: the reference's graph node by node (rag_model.py:341-351)
            out = (out[0], stem1(out[0]))
            for c in cells:
                out = c(out[0], out[1])
            return out[-1]
        n = len(cells)
        ref = x if x is not None else features[0]
        B, dev = ref.shape[0], ref.device
        plan = _plan_chain(stem0, stem1, cells, B, ref.shape[1], self._vol_size(x, features), ref.dtype, x is None)
        sizes, keep1 = plan.sizes, plan.stored[-1]
        self.last_g4_plan = {"pre": {j: cp.g4 for j, cp in enumerate(plan.cells)}, "stem0_out": plan.stem0_g4,      # (tests and tools read it)
                             "stems_fused": plan.stems_fused, **({"stem_tail_rows": plan.stem_tail_rows} if plan.stems_fused else {}),
                             "quarter": {j: cp.quarter for j, cp in enumerate(plan.cells)}}
        pre: Dict[int, torch.Tensor] = {}

        def buf(j):
            """cell j's s0|s1 buffer"""
            if j not in pre:
                pre[j] = torch.empty((B, 2 * cells[j].C_out) + sizes[j], device=dev, dtype=plan.cdt[j])
            return pre[j]

        def unit(j, role):
            """(the 1x1x1 conv of cell j on its input `role` (0 prev_prev, 1 prev), cell j's s0|s1 buffer, the conv's first channel there)"""
            return cells[j].preprocess if role else cells[j].pre_preprocess, buf(j), cells[j].C_out * role

        def tails(i):
            """the planned consumers of T[i] as tails of its producer"""
            out = []
            for (j, role, down) in plan.consumers[i]:
                mod, dst, ch0 = unit(j, role)
                out += mod.as_down_tails(dst, ch0) if down else [mod.as_tail(dst, ch0, g4=plan.cells[j].g4)]
            return out or None

        T: Dict[int, Optional[torch.Tensor]] = {-2: None}
        t0, t1 = tails(-2), tails(-1)
        if plan.stems_fused:
            # stem3d0 and stem3d1 as ONE call whose second kernel expands stem3d0's output from the variant planes in its own staging
            # (ops.costvol_stem_conv3d): nothing but stem3d1 and fused tails reads T[-2], so that 164 MB tensor is never written
            _w0, scale0, shift0 = stem0.prepared()
            wk1, scale1, shift1 = stem1.prepared()
            cout1 = stem1.conv.out_channels
            if plan.stem_tail_rows:
                # cell 0's pre_preprocess (the one tail on stem3d0's output) in the four idle rows of stem3d1's 12-channel matrix product
                key = (stem1.stamp(), cells[0].pre_preprocess.stamp())
                hit = getattr(stem1, "_rows_cache", None)
                if hit is None or hit[0] != key:
                    with torch.no_grad():
                        hit = (key, ops.conv3d_k3_pack(ops.stem_tail_rows_weight(stem1.conv.weight.detach(), t0[0].weight2d)))
                    stem1._rows_cache = hit
                wk1 = hit[1]
            out1 = torch.empty((B, cout1) + sizes[-1], device=dev, dtype=ref.dtype) if keep1 else None
            ops.costvol_stem_conv3d(features[0], features[1], self.maxdisp, stem0.costvol_variants(), 12, scale0, shift0, stem0.relu, t0,
                                    wk1, cout1, scale1, shift1, stem1.relu, out1, [4 * g for g in range(ops.packed_groups(cout1))],
                                    tails=t1, store_main=keep1, tail0_rows=plan.stem_tail_rows)
        else:
            # stem3d0: its output also feeds stem3d1 (3x3x3), so it is materialised
            if x is None:
                T[-2] = stem0.forward_costvol(features[0], features[1], self.maxdisp, tails=t0, out_g4=plan.stem0_g4)
            else:
                T[-2] = stem0(x, tails=t0)
            out1 = stem1(T[-2], tails=t1, store_main=keep1, x_g4=plan.stem0_g4)
        T[-1] = out1 if keep1 else None
        for i, (c, cp) in enumerate(zip(cells, plan.cells)):
            if cp.shared_pre:
                # Cells i and i+1 both resample T[i-1] (the `prev` of one, the `prev_prev` of the other) to the SAME size: cell i's two
                # 1x1x1 convs and cell i+1's pre_preprocess as ONE launch — T[i-1] is gathered by both in the same launch (the second
                # gather hits the L2 the first one filled) and cell i+1 keeps a plain 1x1x1 launch for its other input
                cj = cells[i + 1]
                ops.conv3d_k1_resample_multi([(T[i - 2],) + c.pre_preprocess.prepared() + (c.pre_preprocess.relu, buf(i), 0),
                                              (T[i - 1],) + c.preprocess.prepared() + (c.preprocess.relu, buf(i), c.C_out),
                                              (T[i - 1],) + cj.pre_preprocess.prepared() + (cj.pre_preprocess.relu, buf(i + 1), 0)], sizes[i])
            T[i] = c._run(T[i - 2], T[i - 1], cp, pre.get(i), tails(i) if cp.tails else None)
            if not cp.tails:      # a producer that is not one dual launch: its would-be tails run as plain 1x1x1 launches
                for (j, role, down) in plan.consumers[i]:
                    mod, dst, ch0 = unit(j, role)
                    mod(T[i], out=dst, out_ch0=ch0, resample_to=sizes[j] if down else None)
            T.pop(i - 2, None)
        return T[n - 1]

    def _head(self, vol, last_output, i3, i6, i12):
        """last_12_3d / last_6_3d / last_3_3d and their upsamples (rag_model.py:353-366): `_plan_head` decides, this allocates and launches."""
        m3, m6, m12 = self.last_3_3d[i3], self.last_6_3d[i6], self.last_12_3d[i12]
        train = any(m.autograd_mode(last_output) for m in (m3, m6, m12))
        plan = _plan_head(vol, last_output.shape[2:], last_output.dtype, m3, m6, m12, train)
        # `mat` — the [B,1,d,h,w] cost the soft-argmin reads — is always stored in fp32, also under bf16 activation storage: with
        # |cost| ~ 1e4 a bf16 rounding of it alone moved the disparity by 0.04-0.09 px (tests/analysis_bf16_stage_epe.py), and the
        # tensor is 1/12 of one level-3 activation
        f32 = torch.float32
        if plan.level == 1:
            return m3(last_output, out_dtype=f32)
        d, h, w = vol
        if _plan_head_taps(plan, vol, last_output.shape[2:], last_output.dtype, m3, m6):
            wk, scale, shift = m3.prepared()             # the raw [1, C, 3, 3, 3] weight, read as the [C][27] channel mix
            xb = _plan_head_xblend(plan, vol, last_output.shape[2:], last_output.dtype, m3, m6)      # p6: the x-blended rows Q
            p6 = _head_quarter(last_output, m12, m6, (d // 2, h // 2, w // 2), plan, taps_weight=wk, xblend=xb)
            return ops.uptaps3d(p6, scale, shift, m3.relu, xblended=xb)
        y = m6(last_output) if plan.level == 2 else _head_quarter(last_output, m12, m6, (d // 2, h // 2, w // 2), plan)
        if plan.upconv:         # the 12-channel full-resolution tensor is never written
            wk, scale, shift = m3.prepared()             # the raw [1, C, 3, 3, 3] weight (VALU forms read it as is)
            return ops.upconv3d_c1(y, wk, scale, shift, m3.relu, out_dtype=f32)
        up = ag.resample if train else ops.trilinear3d
        return m3(up(y, (d, h, w), True), out_dtype=f32)

    def cost_volume(self, left_fea, right_fea):
        """The inline loop of rag_model.py:375-383 as one kernel."""
        if ag.needs_grad(left_fea, right_fea):
            return ag.CostVolFn.apply(left_fea, right_fea, self.maxdisp)
        return ops.costvol(left_fea, right_fea, self.maxdisp)

    def forward(self, left_fea, right_fea, task_arch=None):
        if task_arch is None:
            task_arch = self.arch_init
        if left_fea.shape != right_fea.shape or left_fea.dim() != 4:
            raise ValueError("MatchingNet: left/right features must both be [B, C, h, w]")
        # the cost volume (rag_model.py:375-383) is folded into stem3d0 (ragmi_costvol_stem_fwd); matching(cost_volume(..))
        # remains available and gives the same result
        cost = self.matching(None, task_arch, None, features=(left_fea, right_fea))
        return self.disp(cost)

    def forward_stats(self, left_fea, right_fea, task_arch=None, out=None, stats=None):
        """forward with the head's statistics launch in place of the plain one -> DispStats; inference only."""
        refuse_autograd("MatchingNet.forward_stats", left_fea, right_fea)
        if task_arch is None:
            task_arch = self.arch_init
        if left_fea.shape != right_fea.shape or left_fea.dim() != 4:
            raise ValueError("MatchingNet: left/right features must both be [B, C, h, w]")
        with torch.no_grad():
            cost = self.matching(None, task_arch, None, features=(left_fea, right_fea))
            return self.disp.forward_stats(cost, out, stats)

    def forward_mode(self, left_fea, right_fea, task_arch=None, radius=MODE_RADIUS, out=None, stats=None, mode=None):
        """forward with the head's mode launch in place of the plain one -> DispMode; inference only."""
        refuse_autograd("MatchingNet.forward_mode", left_fea, right_fea)
        if task_arch is None:
            task_arch = self.arch_init
        if left_fea.shape != right_fea.shape or left_fea.dim() != 4:
            raise ValueError("MatchingNet: left/right features must both be [B, C, h, w]")
        with torch.no_grad():
            cost = self.matching(None, task_arch, None, features=(left_fea, right_fea))
            return self.disp.forward_mode(cost, radius, out, stats, mode)

    def forward_train_stats(self, left_fea, right_fea, task_arch=None):
        """forward under autograd with the head's statistics launch and its adjoint (Disp.forward_train_stats) -> DispStats whose
        .disp and .tensor carry the graph.  fp32 only."""
        if task_arch is None:
            task_arch = self.arch_init
        if left_fea.shape != right_fea.shape or left_fea.dim() != 4:
            raise ValueError("MatchingNet: left/right features must both be [B, C, h, w]")
        if left_fea.dtype != torch.float32 or right_fea.dtype != torch.float32:
            raise RuntimeError(f"MatchingNet.forward_train_stats: fp32 only (got {left_fea.dtype}, {right_fea.dtype})")
        cost = self.matching(None, task_arch, None, features=(left_fea, right_fea))
        return self.disp.forward_train_stats(cost)
