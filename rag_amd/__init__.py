"""rag_amd — MI355X-native (gfx950) implementation of the stereo Matching-Net forward path
of chzhang18/RAG: cost-volume build -> 3-D conv aggregation -> soft-argmin disparity
regression (and its training step), behind the reference's own nn.Module interface (src/models/rag_model.py).

Host code is PyTorch-ROCm (device memory, streams, torch.distributed); all arithmetic on
the path runs in hand-written HIP kernels reached through the C ABI of
``rag_amd/lib/librag_amd.so`` (include/rag_amd.h).  There is no CPU or eager fallback: the
ops raise if the library is missing.
"""
from ._lib import lib_path, load_library  # noqa: F401
from . import ops  # noqa: F401
from . import autograd  # noqa: F401
from . import metrics  # noqa: F401
from . import train  # noqa: F401
from .metrics import CalibrationMeter, DispMode, DispStats, EpochMeter, Sparsification, sparsification, uncertainty_loss  # noqa: F401
from .metrics import LRCheck, lr_consistency, lr_consistency_torch, lr_stack, re_and_sm_loss, re_and_sm_loss_torch  # noqa: F401
from .metrics import FilledDisp, fill_disparity, fill_disparity_torch  # noqa: F401
from .metrics import Speckles, filter_speckles, filter_speckles_torch  # noqa: F401
from .train import search_eval_step  # noqa: F401
from .modules import (  # noqa: F401
    ALL_CONV_GENOTYPE, ALL_SKIP_GENOTYPE, Cell_3d, ConvBR_3d, Disp, DisparityRegression, Genotype,
    Identity_3d, MatchingNet, OPS_3d, PRIMITIVES_3D,
)

from .modules import Cell_2d, ConvBR_2d, OPS_2d, PRIMITIVES  # noqa: E402,F401
from .network import Network  # noqa: E402,F401
from . import checkpoint  # noqa: E402,F401
from . import supernet  # noqa: E402,F401
from .supernet import AutoFeature, AutoMatching, BasicNetwork, DepthAutoMatching, DepthBasicNetwork  # noqa: E402,F401
from . import depth  # noqa: E402,F401
depth.BasicNetwork = DepthBasicNetwork      # the depth tree's own name for its supernet (rag_depth/src/automl/mdenas_basicmodel.py)
from .depth import DepthEpochMeter, DepthNetwork, depth_metrics, load_depth_checkpoint, silog_metrics_loss  # noqa: E402,F401
from . import depth_search  # noqa: E402,F401
from .depth_search import DepthGraphedSearchStep, depth_search_eval_step, depth_search_step  # noqa: E402,F401
from . import data  # noqa: E402,F401
from .data import color_stats, lanczos_taps, prepare_batch, random_crop_origin, resize_lanczos, resize_lanczos_torch, transfer_color  # noqa: E402,F401

__all__ = [
    "EpochMeter", "search_eval_step", "DispStats", "DispMode", "uncertainty_loss",
    "sparsification", "Sparsification", "CalibrationMeter",
    "LRCheck", "lr_consistency", "lr_consistency_torch", "lr_stack", "re_and_sm_loss", "re_and_sm_loss_torch",
    "FilledDisp", "fill_disparity", "fill_disparity_torch",
    "Speckles", "filter_speckles", "filter_speckles_torch",
    "DepthEpochMeter", "depth_metrics", "silog_metrics_loss", "depth_search", "depth_search_step", "depth_search_eval_step",
    "DepthGraphedSearchStep",
    "Network", "Cell_2d", "ConvBR_2d", "DepthNetwork", "load_depth_checkpoint",
    "data", "prepare_batch", "random_crop_origin", "color_stats", "transfer_color", "lanczos_taps", "resize_lanczos", "resize_lanczos_torch",
    "ops", "load_library", "lib_path", "MatchingNet", "Cell_3d", "ConvBR_3d", "Identity_3d", "Disp",
    "DisparityRegression", "OPS_3d", "PRIMITIVES_3D", "Genotype", "ALL_CONV_GENOTYPE", "ALL_SKIP_GENOTYPE",
]
