"""``AffineTensorTransform``: a random rotation / shear / scale of a batch that can be replayed and undone, differentiable with respect
to the image (ref contrastyou/augment/tensor_affine_transform.py:9-103).

The draws, the matrices and the call signature are the reference's.  GPU fp32 batches are warped by the HIP kernels behind
``miseg_amd.ops.affine_warp`` (no sampling grid, a bit-reproducible backward); everything else -- CPU tensors, other dtypes and
interpolation modes, a matrix that wants its own gradient, a matrix whose backward the kernels cannot cover -- goes through
``F.affine_grid`` + ``F.grid_sample`` as in the reference.
"""
import numpy as np
import torch
from torch import Tensor
from torch.nn import functional as F

from miseg_amd import ops

_KERNEL_MODES = ("bilinear", "nearest")


def inverse_transform_matrix(AffineMatrix: Tensor) -> Tensor:
    """[B, 2, 3] -> [B, 2, 3]: each matrix completed by the row (0, 0, 1), inverted, and cut back to its first two rows
    (ref tensor_affine_transform.py:9-30: one ``torch.inverse`` per matrix, in the matrix's dtype and on its device)."""
    bn, k, l = AffineMatrix.shape
    assert k == 2 and l == 3, AffineMatrix.shape
    last_row = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float32, device=AffineMatrix.device)
    return torch.stack([torch.inverse(torch.cat([m, last_row], dim=0))[:2, :] for m in AffineMatrix], dim=0)


class AffineTensorTransform:
    def __init__(self, min_rot: float = 0, max_rot: float = 180, min_shear: float = 0.0, max_shear: float = 0.5, min_scale: float = 0.9,
                 max_scale: float = 1.1, mode="bilinear"):
        self.min_rot = min_rot
        self.max_rot = max_rot
        self.min_shear = min_shear
        self.max_shear = max_shear
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.mode = mode

    def get_random_affinematrix(self) -> Tensor:
        """One [2, 3] fp32 matrix from three ``numpy.random.rand()`` draws, in the reference's order: rotation (degrees), shear
        (degrees, added to the angle of the second column), scale (ref tensor_affine_transform.py:52-66).  No translation."""
        rot = np.radians(np.random.rand() * (self.max_rot - self.min_rot) + self.min_rot)
        shear = np.radians(np.random.rand() * (self.max_shear - self.min_shear) + self.min_shear)
        scale = np.random.rand() * (self.max_scale - self.min_scale) + self.min_scale
        rows = [[np.cos(rot) * scale, -np.sin(rot + shear) * scale, 0.0],
                [np.sin(rot) * scale, np.cos(rot + shear) * scale, 0.0]]
        return torch.from_numpy(np.array(rows, dtype=np.float32)).float()

    def _kernel_reach(self, img: Tensor, affinematrix: Tensor):
        """The backward search radius for ``ops.affine_warp`` if the kernels take this call, else ``None`` (torch path)."""
        if not (img.is_cuda and img.dtype == torch.float32 and self.mode in _KERNEL_MODES) or affinematrix.requires_grad:
            return None
        n, c, h, w = img.shape
        if img.numel() == 0 or img.numel() >= 2 ** 31 or max(h, w) > 2048:
            return None
        if not (img.is_contiguous() or img.is_contiguous(memory_format=torch.channels_last)):
            return None
        reach = ops.affine_reach(affinematrix, h, w)
        if reach > ops.AFFINE_MAX_REACH:
            if img.requires_grad and torch.is_grad_enabled():
                return None
            reach = ops.AFFINE_MAX_REACH          # no backward will run
        return reach

    def _perform_affine_transform(self, single_img: Tensor, affinematrix: Tensor) -> Tensor:
        assert len(single_img.shape) == 4
        assert affinematrix.shape[1] == 2 and affinematrix.shape[2] == 3, affinematrix.shape
        reach = self._kernel_reach(single_img, affinematrix)
        if reach is not None:
            return ops.affine_warp(single_img, affinematrix.detach().cpu(), mode=self.mode, reach=reach)
        affinematrix = affinematrix.to(single_img.device)
        grid = F.affine_grid(affinematrix, single_img.shape, align_corners=True)
        return F.grid_sample(single_img, grid, mode=self.mode, padding_mode="zeros", align_corners=True)

    def __call__(self, img: Tensor, AffineMatrix: Tensor = None, independent=True, inverse=False):
        """``img`` [B, C, H, W], [C, H, W] (one sample) or [H, W] -> ``(img_tf, AffineMatrix)`` with ``img_tf`` of ``img``'s shape.
        Without a matrix one is drawn per sample (``independent``) or one for the batch; as in the reference a first matrix is drawn
        either way, and dropped when ``independent``.  ``inverse=True`` applies, and returns, the inverse matrices."""
        assert len(img.shape) in (4, 3, 2)
        shape = img.shape
        while img.dim() < 4:
            img = img.unsqueeze(0)
        bn = img.shape[0]
        if AffineMatrix is None:
            AffineMatrix = self.get_random_affinematrix()
            if independent:
                AffineMatrix = torch.stack([self.get_random_affinematrix() for _ in range(bn)], dim=0)
            else:
                AffineMatrix = torch.stack([AffineMatrix] * bn, dim=0)
        else:
            assert AffineMatrix.shape[0] == bn
        if inverse:
            AffineMatrix = inverse_transform_matrix(AffineMatrix)
        img_tf = self._perform_affine_transform(img, AffineMatrix)
        return img_tf.view(*shape), AffineMatrix
