"""Float64 references, case tables and input generators for the pixel-loss kernels (csrc/losses.hip) and the batch-assembly kernels
(the cat/flip family there, the byte movers at the end of csrc/tape.hip).  Shared by test_cpu_pixel_ref.py, which checks the
references and that every case reaches the branch it names, and test_gpu_pixel_kernels.py, which runs the kernels against them.

References are the expression of each kernel's header comment evaluated in float64 with eps = 1e-16 as a mean over pixels (over
npix * C for the MSE); gradients are float64 autograd of that expression.  A reference is computed once per case (lru_cache) and
handed out as is: callers must not write into it.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import synth

F64 = torch.float64
EPS = 1e-16

# ---- the launchers' constants (csrc/pixel_loss.h: pixel_blocks, MISEG_DISPATCH_C; csrc/losses.hip: kLT, the grids of argmax_dice / cat_flip*; csrc/tape.hip: copy_blocks)
LOSS_THREADS = 256
LOSS_MAX_BLOCKS = 2048
CLASS_COUNTS = (2, 3, 4, 5, 6, 8, 10, 16)
REFUSED_CLASS_COUNTS = (1, 7, 9, 11, 17, 32)
DICE_THREADS, DICE_MAX_BLOCKS = 256, 64
CAT_THREADS, CAT_MAX_BLOCKS = 256, 8192
COPY_THREADS, COPY_MAX_BLOCKS = 256, 2048
SCALES = (2, 12, 30)

# ---- bounds (the project's own: test_gpu_losses.py asks 1e-5 relative of the loss and <= 1e-7 of a vanishing one)
LOSS_REL = 1e-5
LOSS_ABS_SMALL = 1e-7        # where |ref| < LOSS_SMALL
LOSS_SMALL = 1e-6
GRAD_REL_OF_MAX = 1e-5       # max|got - ref| <= GRAD_REL_OF_MAX * max|ref| over the tensor


def loss_blocks(npix: int) -> int:
    return min(-(-npix // LOSS_THREADS), LOSS_MAX_BLOCKS)


def loss_branch(n: int, h: int, w: int) -> str:
    """Which path of a loss kernel's pixel loop a shape takes."""
    npix = n * h * w
    if npix > LOSS_MAX_BLOCKS * LOSS_THREADS:
        return "grid_stride"
    if npix < LOSS_THREADS:
        return "short_single_block"
    if npix == LOSS_THREADS:
        return "one_full_block"
    return "full_blocks_and_tail" if npix % LOSS_THREADS else "full_blocks"


# name -> (N, H, W, C, logit scale)
LOSS_CASES = {f"c{c}_s{s}": (3, 19, 23, c, s) for c in CLASS_COUNTS for s in SCALES}
LOSS_CASES.update({
    "short_c4": (1, 5, 7, 4, 2),
    "short_c16": (1, 5, 7, 16, 2),
    "oneblock_c4": (1, 16, 16, 4, 2),
    "stride_c2": (2, 512, 513, 2, 2),
    "stride_c4": (2, 512, 513, 4, 2),
})
LOSS_CASE_BRANCH = {name: "full_blocks_and_tail" for name in LOSS_CASES if name[0] == "c"}
LOSS_CASE_BRANCH.update({"short_c4": "short_single_block", "short_c16": "short_single_block", "oneblock_c4": "one_full_block",
                         "stride_c2": "grid_stride", "stride_c4": "grid_stride"})
KERNELS = ("kl", "mse", "klcons", "entropy")

# flip replay (softmax_mse / softmax_klcons): name -> (N, H, W, C, masks or None); bit 0 flips H, bit 1 flips W
FLIP_CASES = {
    "flip_5x7": (4, 5, 7, 4, (0, 1, 2, 3)),
    "flip_19x23": (4, 19, 23, 3, (0, 1, 2, 3)),
    "flip_19x23_rev": (4, 19, 23, 4, (3, 2, 1, 0)),
    "noflip_5x7": (4, 5, 7, 4, None),
}

# argmax_dice: name -> (N, H, W, C)
DICE_CASES = {f"dice_c{c}": (3, 19, 23, c) for c in CLASS_COUNTS}
DICE_CASES["dice_inner_loop"] = (1, 129, 130, 4)

# cat_flip / cat_flipped: name -> (Na, Nb, C, H, W)
CAT_CASES = {"cat_2_3_1_5x7": (2, 3, 1, 5, 7), "cat_1_4_2_19x23": (1, 4, 2, 19, 23), "cat_grid_stride": (1, 2, 1, 648, 650)}
CAT_FLIPPED_GRID_STRIDE = (1, 4, 1, 648, 650)      # cat_flipped writes Na + Nb samples: "cat_grid_stride" stays below its loop, this one does not
CAT_CABI_CASE = (0, 2, 3, 4, 6)          # Na = 0: a null `a`, through the C ABI only
# (the last but one fills the largest grid exactly, one 16-byte vector per thread, plus a tail; the last makes the threads loop)
BYTE_COUNTS = (1, 15, 16, 17, 4099, 16 * COPY_MAX_BLOCKS * COPY_THREADS + 5, 16 * (COPY_MAX_BLOCKS * COPY_THREADS + 3) + 5)
ASSEMBLE_BIG = 4 * (COPY_MAX_BLOCKS * COPY_THREADS + 1028)      # floats: more than 2048 * 256 float4


def masks_to_decisions(masks):
    return [[bool(m & 1), bool(m & 2)] for m in masks]


# ----------------------------------------------------------------------------- inputs
def logits(tag: str, n: int, c: int, h: int, w: int, scale: float = 1.0) -> torch.Tensor:
    """fp32 NCHW logits, N(0, scale^2)."""
    return torch.from_numpy(synth.normal("pixel/" + tag, (n, c, h, w), scale=float(scale)))


def labels(tag: str, n: int, h: int, w: int, c: int) -> torch.Tensor:
    return torch.from_numpy(synth.integers("pixel/" + tag, (n, h, w), c))


def case_inputs(kernel: str, name: str):
    """(a, second) of a LOSS_CASES / FLIP_CASES entry: second = int64 labels (kl), the detached logits b (mse, klcons) or None."""
    n, h, w, c = (LOSS_CASES.get(name) or FLIP_CASES[name])[:4]
    scale = LOSS_CASES[name][4] if name in LOSS_CASES else 2
    a = logits(f"{name}/a", n, c, h, w, scale)
    if kernel == "kl":
        return a, labels(f"{name}/t", n, h, w, c)
    if kernel in ("mse", "klcons"):
        return a, logits(f"{name}/b", n, c, h, w, scale)
    return a, None


def tie_logits(tag: str, n: int, c: int, h: int, w: int) -> torch.Tensor:
    """Logits drawn from {-1, -0.0, 0.0, 1}: ties (and the two zeros, which compare equal) at most pixels."""
    table = np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32)
    return torch.from_numpy(table[synth.integers("pixel/" + tag, (n, c, h, w), 4)])


SPECIAL_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FA12345,      # quiet / negative / signalling NaNs with payloads
                0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x00400000,   # -0.0, +0.0, denormals
                0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00800000)      # infinities, the largest and the smallest normal


def bit_payload(tag: str, shape, dtype=torch.float32) -> torch.Tensor:
    """A 4-byte payload for the bit-exact movers: normal noise with SPECIAL_BITS written over a seeded tenth of the entries and over
    the first and last ones.  Returned as ``dtype`` (float32 or int32) -- the same bits either way."""
    x = synth.normal("pixel/" + tag, shape).view(np.uint32).reshape(-1).copy()
    rs = np.random.RandomState(synth._seed("pixel/special/" + tag))
    where = rs.choice(x.size, max(2, x.size // 10), replace=False)
    x[where] = np.array(SPECIAL_BITS, dtype=np.uint32)[rs.randint(0, len(SPECIAL_BITS), where.size)]
    x[0], x[-1] = SPECIAL_BITS[0], SPECIAL_BITS[4]
    t = torch.from_numpy(x.view(np.int32).reshape(tuple(shape)))
    return t if dtype == torch.int32 else t.view(torch.float32)


def bits(t: torch.Tensor) -> torch.Tensor:
    """The integer view of a tensor's elements (for bit-exact comparisons that NaNs and the sign of zero cannot fool)."""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# fp32 bit patterns for the 16-bit cast of cat_flip_pad: round-to-nearest-even against truncation, half overflow, half denormals
ROUNDING_BITS = (
    0x3F80C000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF80C000,          # bf16: above half / tie to even (down, up) / just above, just below a tie
    0x3F801000, 0x3F803000, 0x3F801001, 0x3F800FFF,                                # half: tie to even down (1 + 2^-11), up (1 + 3 2^-11), either side of a tie
    0x477FE000, 0x477FF000, 0x477FEFFF, 0x47C35000, 0xC77FF000, 0x7F7FFFFF,          # 65504, 65520 (-> inf in half), just below it, 1e5, -65520, the largest float (inf in both)
    0x33800000, 0x33000000, 0x33C00000, 0x33000001, 0x387FC000, 0x38000000, 0x00000001,   # 2^-24, 2^-25 (tie -> 0), 3 2^-25, just above the tie, the largest half denormal, 2^-15, an fp32 denormal
    0x7FC00000, 0x80000000, 0x7F800000, 0xFF800000,                                # NaN, -0.0, infinities
)


def rounding_image(tag: str, n: int, h: int, w: int) -> torch.Tensor:
    """One-channel fp32 images [n, 1, h, w]: noise with every ROUNDING_BITS pattern placed at seeded positions (each at least once)."""
    x = synth.normal("pixel/" + tag, (n, 1, h, w)).view(np.uint32).reshape(-1).copy()
    rs = np.random.RandomState(synth._seed("pixel/rounding/" + tag))
    reps = max(1, x.size // (4 * len(ROUNDING_BITS)))
    where = rs.choice(x.size, reps * len(ROUNDING_BITS), replace=False)
    x[where] = np.tile(np.array(ROUNDING_BITS, dtype=np.uint32), reps)
    return torch.from_numpy(x.view(np.float32).reshape(n, 1, h, w))


# ----------------------------------------------------------------------------- float64 references
def _softmax64(z: torch.Tensor) -> torch.Tensor:
    return z.to(F64).softmax(1)


def kl_expr(z64: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean_pix sum_c -t_c log((p_c + eps) / (t_c + eps)), t = one-hot of ``target``; a label outside [0, C) is an all-zero row: it
    adds nothing and the divisor stays the number of pixels (the kernel's contract for a bad label)."""
    c = z64.shape[1]
    onehot = torch.stack([target == k for k in range(c)], 1).to(F64)
    p = z64.softmax(1)
    return (-onehot * torch.log((p + EPS) / (onehot + EPS))).sum(1).mean()


def mse_expr(a64: torch.Tensor, b64: torch.Tensor) -> torch.Tensor:
    """mean over N*C*H*W of (softmax(a) - softmax(b))^2, b detached."""
    return ((a64.softmax(1) - b64.detach().softmax(1)) ** 2).mean()


def klcons_expr(a64: torch.Tensor, b64: torch.Tensor) -> torch.Tensor:
    """mean_pix sum_c -t_c log((p_c + eps) / (t_c + eps)), p = softmax(a), t = softmax(b) detached."""
    p, t = a64.softmax(1), b64.detach().softmax(1)
    return (-t * torch.log((p + EPS) / (t + EPS))).sum(1).mean()


def entropy_expr(z64: torch.Tensor) -> torch.Tensor:
    """mean_pix -sum_c p_c log(p_c + eps)."""
    p = z64.softmax(1)
    return (-p * torch.log(p + EPS)).sum(1).mean()


EXPR = {"kl": kl_expr, "mse": mse_expr, "klcons": klcons_expr, "entropy": entropy_expr}


def value_and_grad(kernel: str, a: torch.Tensor, second=None):
    """(loss, d loss / d a) of a kernel's expression in float64, by autograd; ``second`` as in ``case_inputs`` (b already flipped)."""
    a64 = a.detach().to(F64).clone().requires_grad_(True)
    if kernel == "entropy":
        loss = entropy_expr(a64)
    elif kernel == "kl":
        loss = kl_expr(a64, second)
    else:
        loss = EXPR[kernel](a64, second.detach().to(F64))
    loss.backward()
    return loss.detach(), a64.grad


def analytic_grad(kernel: str, a: torch.Tensor, second=None) -> torch.Tensor:
    """The gradient written out by hand in float64 (d/dz_c = p_c (g_c - <g, p>) / npix through the softmax Jacobian), an independent
    check of ``value_and_grad``: g = -t / (p + eps) (kl, klcons), 2 (p - t) / C (mse), -(log(p + eps) + p / (p + eps)) (entropy)."""
    p = _softmax64(a)
    n, c, h, w = p.shape
    if kernel == "kl":
        t = torch.stack([second == k for k in range(c)], 1).to(F64)
        g = -t / (p + EPS)
    elif kernel == "klcons":
        g = -_softmax64(second) / (p + EPS)
    elif kernel == "mse":
        g = 2.0 * (p - _softmax64(second)) / c
    else:
        g = -(torch.log(p + EPS) + p / (p + EPS))
    return p * (g - (g * p).sum(1, keepdim=True)) / (n * h * w)


@functools.lru_cache(maxsize=None)
def case_reference(kernel: str, name: str):
    """(loss, grad) float64 of a LOSS_CASES entry (no flips), or of a FLIP_CASES entry on the materialised flip of b."""
    from oracle import losses as OL
    a, second = case_inputs(kernel, name)
    if name in FLIP_CASES and FLIP_CASES[name][4] is not None and kernel in ("mse", "klcons"):
        second = OL.apply_flips(second, masks_to_decisions(FLIP_CASES[name][4]))
    return value_and_grad(kernel, a, second)


def fp32_composition(kernel: str, a: torch.Tensor, second=None):
    """The same expression composed of fp32 torch ops on the CPU: (loss, grad).  Its distance from the float64 reference is the error
    an fp32 evaluation makes on the input -- the yardstick the bounds above were taken from."""
    a32 = a.detach().float().clone().requires_grad_(True)
    if kernel == "entropy":
        loss = entropy_expr(a32)
    elif kernel == "kl":
        c = a32.shape[1]
        onehot = torch.stack([second == k for k in range(c)], 1).float()
        p = a32.softmax(1)
        loss = (-onehot * torch.log((p + EPS) / (onehot + EPS))).sum(1).mean()
    else:
        loss = EXPR[kernel](a32, second.detach().float())
    loss.backward()
    return loss.detach(), a32.grad


def loss_error(got: float, ref: float):
    """(error, bound) of a loss value under the project's rule."""
    ref = float(ref)
    return abs(float(got) - ref), (LOSS_ABS_SMALL if abs(ref) < LOSS_SMALL else LOSS_REL * abs(ref))


def grad_error(got: torch.Tensor, ref: torch.Tensor):
    """(max |got - ref|, bound) with the bound a fraction of the LARGEST reference entry (element-wise relative bounds are wrong for
    peaked logits, where most entries lie many orders below the largest)."""
    ref = ref.to(F64)
    return float((got.detach().cpu().to(F64) - ref).abs().max()), GRAD_REL_OF_MAX * float(ref.abs().max())


# ----------------------------------------------------------------------------- argmax + Dice counts
def first_argmax(z: torch.Tensor) -> torch.Tensor:
    """First maximum over the channel axis (numpy's argmax rule), int64 [N, H, W]."""
    return torch.from_numpy(np.argmax(z.numpy(), axis=1).astype(np.int64))


def dice_bincount(pred: torch.Tensor, target: torch.Tensor, c: int):
    """(intersection, union) int64 [N, C] by numpy.bincount: union = |pred == k| + |target == k|, the reference's `union`
    (general_dice_meter.py:141-172).  A target outside [0, C) adds to no class and to no intersection; the prediction of that pixel
    still counts (what the kernel does)."""
    n = pred.shape[0]
    inter, uni = np.zeros((n, c), np.int64), np.zeros((n, c), np.int64)
    for i in range(n):
        p, t = pred[i].reshape(-1).numpy(), target[i].reshape(-1).numpy()
        ok = (t >= 0) & (t < c)
        uni[i] = np.bincount(p, minlength=c) + np.bincount(t[ok], minlength=c)
        inter[i] = np.bincount(p[ok & (p == t)], minlength=c)
    return torch.from_numpy(inter), torch.from_numpy(uni)


# ----------------------------------------------------------------------------- batch assembly
def cat_flip_ref(a, b, masks):
    from oracle import losses as OL
    return torch.cat([a, b, OL.apply_flips(b, masks_to_decisions(masks))])


def cat_flipped_ref(a, b, masks):
    from oracle import losses as OL
    return torch.cat([a, OL.apply_flips(b, masks_to_decisions(masks))])


def assemble_ref(parts):
    """[(src fp32 1-D or None, scale float or None, numel)] -> the fp32 buffer: scale * src (IEEE fp32 product), zeros for a null source."""
    out = []
    for src, scale, numel in parts:
        if src is None:
            out.append(torch.zeros(numel))
        else:
            out.append(src * torch.tensor(1.0 if scale is None else scale, dtype=torch.float32))
    return torch.cat(out)


def split_losses_ref(x: torch.Tensor, sizes, target: torch.Tensor, masks, coeffs):
    """d/dx of  c0 * KL(softmax(x0), onehot(target)) + c1 * MSE(softmax(x2), softmax(flip(x1)).detach())  over the batch
    x = [x0 | x1 | x2] in float64, the graph built with torch.split: (loss, grad [N, C, H, W])."""
    from oracle import losses as OL
    x64 = x.detach().to(F64).clone().requires_grad_(True)
    x0, x1, x2 = torch.split(x64, list(sizes), 0)
    b = x1.detach() if masks is None else OL.apply_flips(x1.detach(), masks_to_decisions(masks))
    loss = coeffs[0] * kl_expr(x0, target) + coeffs[1] * mse_expr(x2, b)
    loss.backward()
    return loss.detach(), x64.grad
