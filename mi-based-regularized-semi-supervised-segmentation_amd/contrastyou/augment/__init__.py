"""``contrastyou.augment``: the differentiable geometric transform on tensors (ref contrastyou/augment/__init__.py:5).

The reference's package also holds its PIL presets (``ACDCTransforms``, ``ACDCStrongTransforms``); this repository's input pipeline
lives in ``semi_seg.augment`` and ``miseg_amd.slices``, and nothing here imports torchvision.
"""
from .tensor_affine_transform import AffineTensorTransform, inverse_transform_matrix

__all__ = ["AffineTensorTransform", "inverse_transform_matrix"]
