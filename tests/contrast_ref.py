"""Shared by tests/test_cpu_contrast.py and tests/test_gpu_contrast.py: the float64 closed form of the supervised-contrastive loss on
raw embeddings (the expression of include/miseg_hip.h, ``miseg_supcon``), seeded embeddings, and the inputs of tests/golden/contrast.npz
rebuilt from their ``synth`` tags (tests/golden/make_golden_contrast.py)."""
import torch

import synth


def closed_form(e, labels, views, T=0.07, Tb=0.07):
    """(loss, d loss / d e) in float64 with autograd for raw embeddings e [views * B, D], view-major; labels None = SimCLR."""
    e = e.detach().double().requires_grad_()
    n = e.shape[0]
    b = n // views
    lab = torch.arange(b) if labels is None else torch.as_tensor(labels).long()
    lab = lab.repeat(views)
    z = e / e.norm(dim=1, keepdim=True).clamp_min(1e-12)
    s = z @ z.t() / T
    m = s.max(dim=1, keepdim=True).values.detach()
    off = ~torch.eye(n, dtype=torch.bool)
    Z = (torch.exp(s - m) * off).sum(1, keepdim=True) + 1e-16
    pos = (lab.view(-1, 1) == lab.view(1, -1)) & off
    logp = s - m - torch.log(Z)
    loss = (T / Tb) * (-(logp * pos).sum(1) / pos.sum(1)).mean()
    loss.backward()
    return float(loss.detach()), e.grad


def embeddings(b, d, views, seed, scale=1.0):
    """View 1 = seeded normals, every further view = view 1 + 0.3 x noise (positives lie close), all times ``scale``."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(b, d, generator=g)
    return torch.cat([base] + [base + 0.3 * torch.randn(b, d, generator=g) for _ in range(views - 1)]) * scale


def golden_projector_state(output_dim=256):
    T = torch.from_numpy
    return {"_header.2.weight": T(synth.normal("contrast/proj/w1", (256, 256), scale=1.0 / 16)),
            "_header.2.bias": T(synth.normal("contrast/proj/b1", (256,), scale=1.0 / 16)),
            "_header.4.weight": T(synth.normal("contrast/proj/w2", (output_dim, 256), scale=1.0 / 16)),
            "_header.4.bias": T(synth.normal("contrast/proj/b2", (output_dim,), scale=1.0 / 16))}


def golden_views(i, b, h):
    return torch.from_numpy(synth.uniform(f"contrast/img{i}", (b, 1, h, h))), torch.from_numpy(synth.uniform(f"contrast/tf{i}", (b, 1, h, h)))


def group_of(name: str) -> str:
    if name.startswith("_header"):
        return "projector"
    return "Conv5" if name.startswith("Conv5") else "Conv1-4"
