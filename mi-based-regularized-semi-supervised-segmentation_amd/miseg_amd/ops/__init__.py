"""torch.autograd front-ends of the HIP kernels (thin: pointer/shape plumbing only), one module per kernel family of ``csrc/``.

Every function here requires CUDA(HIP) tensors and raises otherwise -- the product has no CPU or eager-PyTorch fallback.  PyTorch
supplies device memory, the current HIP stream and autograd bookkeeping; all arithmetic happens in ``csrc/*.hip`` behind
``include/miseg_hip.h``.  This namespace re-exports the families, the plumbing under them (``_rt``, ``stepio``) and ``unet_ops``' stem data
gradient.  Two of its names are read from HERE whenever a family runs (``_pkg``): ``call``, so that a launch spy on ``ops.call`` sees every
family's launches, and ``_MI_PLANES``.  State that is rebound lives in one module and is read through functions (``mi.mi_precision_code``).
"""
import os

from .._cabi import call, query  # noqa: F401
from .._rt import (_DT, _GradJoin, _need_gpu, _ptr, _stream, _ws, PinnedRing, arange_i32, as_nhwc, cached_const, empty_nhwc, fill_zero,  # noqa: F401
                   flip_masks, flips_to_tensor, wait_stream, windows_tensor, zeros_nhwc)
from ..stepio import scalar_out, zero_counter  # noqa: F401
from ..unet_ops import stem_dgrad, stem_dgrad_supported  # noqa: F401

# 1: the joint forward writes the backward's operand planes and the f16 + fp8 backward copies its source rows from them.  Built and
# measured: the backward gains less inside the step (-0.06 ms) than the by-product costs the forward (+0.07 ms).
_MI_PLANES = os.environ.get("MISEG_MI_PLANES", "0") == "1"

from .batch import AFFINE_MAX_REACH, affine_inverse, affine_reach, affine_warp, cat_flip, cat_flipped, cat_mixed, flip, noise_add, split_rows  # noqa: E402,F401
from .contrast import (_CD_MAX_C, _SUPCON_MAX_D, _SUPCON_MAX_N, avgpool_nhwc, bias_amaxpool, bias_amaxpool_supported, bias_lrelu,  # noqa: E402,F401
                       bias_lrelu_supported, conv3x3_bias, conv3x3_bias_supported, supcon, supcon_supported)
from .heads import global_head, global_head_var, local_head, local_head_var  # noqa: E402,F401
from .losses import (_LOSS_CLASS_COUNTS, softmax_dice, softmax_dice_supported, softmax_entropy, softmax_entropy_supported, softmax_kl,  # noqa: E402,F401
                     softmax_accum, softmax_cross_pseudo, softmax_kl_consistency, softmax_mix_kl_consistency, softmax_mix_mse, softmax_mse, softmax_umse)
from .metrics import argmax_dice, largest_component, surface_stats  # noqa: E402,F401
from .mi import (LOCAL_LOSS_SINGLE_BLOCK_MAX_K, MI_PRECISIONS, _local_loss, colour_windows, global_joint, global_mi, global_mi_pair,  # noqa: E402,F401
                 local_mi_heads, local_mi_losses, local_mi_raw_joint, mi_precision_code, mi_precision_name, output_local_mi,
                 output_local_mi_supported, resolve_mi_precision, set_mi_precision)
from .vat import l2_perturb, normal_fill, philox_words  # noqa: E402,F401
