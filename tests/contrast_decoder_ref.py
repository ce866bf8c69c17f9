"""Shared by tests/test_cpu_contrast_decoder.py and tests/test_gpu_contrast_decoder.py: the embedding-row layout of
``miseg_bias_amaxpool_fwd`` (include/miseg_hip.h) as tensor reshapes, the torch composition of the pool on the CPU, and the inputs of
tests/golden/contrast_decoder.npz rebuilt from their ``synth`` tags (tests/golden/make_golden_contrast_decoder.py)."""
import torch
import torch.nn.functional as F

import synth


def embed_rows(pooled, partition_num, views):
    """[N, C, OH, OW] -> [N * PH * PW, C * bh * bw]: the value of (n = v * B + b, c, ph * bh + dh, pw * bw + dw) at row
    v * PH * PW * B + (ph * PW + pw) * B + b, column c * bh * bw + dh * bw + dw."""
    n, c, oh, ow = pooled.shape
    (ph, pw), b = partition_num, n // views
    bh, bw = oh // ph, ow // pw
    t = pooled.reshape(views, b, c, ph, bh, pw, bw).permute(0, 3, 5, 1, 2, 4, 6)
    return t.reshape(views * ph * pw * b, c * bh * bw)


def pool_reference(raw_nhwc, bias, output_size, partition_num, views):
    """fp32 on the CPU from the stored values of ``raw_nhwc`` [N, H, W, C]: (rows, idx [N, OH, OW, C] int32, the leaf the rows hang on)."""
    x = raw_nhwc.detach().cpu().float().permute(0, 3, 1, 2).contiguous().requires_grad_()
    vals, idx = F.adaptive_max_pool2d(x, output_size, return_indices=True)
    if bias is not None:
        vals = vals + bias.detach().cpu().float().view(1, -1, 1, 1)
    return embed_rows(vals, partition_num, views), idx.permute(0, 2, 3, 1).contiguous().to(torch.int32), x


def same_bits(a, b):
    """Equal as bit patterns, except that any NaN matches any NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    if not torch.equal(nan_a, nan_b):
        return False
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(ints)[~nan_a], b.contiguous().view(ints)[~nan_b]))


# ---- the fixture's inputs (tests/golden/make_golden_contrast_decoder.py)
def golden_projector_state():
    """The mlp LocalProjectionHead(32)'s state: seeded normals at the scale of nn.Conv2d's default initialisation."""
    T = torch.from_numpy
    return {"_projector.0.weight": T(synth.normal("contrast_decoder/proj/w1", (64, 32, 3, 3), scale=1.0 / 17)),
            "_projector.0.bias": T(synth.normal("contrast_decoder/proj/b1", (64,), scale=1.0 / 17)),
            "_projector.2.weight": T(synth.normal("contrast_decoder/proj/w2", (32, 64, 3, 3), scale=1.0 / 24)),
            "_projector.2.bias": T(synth.normal("contrast_decoder/proj/b2", (32,), scale=1.0 / 24))}


def golden_views(i, b, h):
    return (torch.from_numpy(synth.uniform(f"contrast_decoder/img{i}", (b, 1, h, h))),
            torch.from_numpy(synth.uniform(f"contrast_decoder/ctf{i}", (b, 1, h, h))))


GROUPS = ("projector.2", "projector.0", "Up_conv3", "Up3-5")


def group_of(name: str) -> str:
    if name.startswith("_projector.2"):
        return "projector.2"
    if name.startswith("_projector.0"):
        return "projector.0"
    return "Up_conv3" if name.startswith("Up_conv3") else "Up3-5"
