"""Layout of ``miseg_amd`` on the CPU: the names ``miseg_amd.ops`` has to offer, the import order of the layers under it
(``_cabi`` < ``_rt`` < ``stepio`` < ``tape``, ``checks``, ``gradslot``, ``packcache``, ``lazy`` < ``unet_ops`` < the ``ops`` families), where an import may still
sit inside a function, the one home of the local-MI precision, and the independence of the family modules.  Every expected name and
every exception is a literal here."""
import ast
import os
import subprocess
import sys

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mi-based-regularized-semi-supervised-segmentation_amd")
MISEG = os.path.join(PKG, "miseg_amd")

# every ``ops.NAME`` / ``O.NAME`` / ``from miseg_amd.ops import NAME`` of the repository before ``ops`` became a package (bench.py,
# __graft_entry__.py, semi_seg, contrastyou, deepclustering2, oracle, profiles, tests, the package itself) -- but for ``_mi_precision``: it
# is rebound by ``set_mi_precision``, a re-exported copy would go stale, and its one reader (the tape key) calls ``mi_precision_code()`` now
OPS_NAMES = [
    "AFFINE_MAX_REACH", "LOCAL_LOSS_SINGLE_BLOCK_MAX_K", "MI_PRECISIONS", "PinnedRing", "_CD_MAX_C", "_DT", "_GradJoin", "_LOSS_CLASS_COUNTS",
    "_MI_PLANES", "_SUPCON_MAX_D", "_SUPCON_MAX_N", "_local_loss", "_need_gpu", "_ptr", "_stream", "_ws", "affine_inverse", "affine_reach",
    "affine_warp", "arange_i32", "argmax_dice", "as_nhwc", "avgpool_nhwc", "bias_amaxpool", "bias_amaxpool_supported", "bias_lrelu",
    "bias_lrelu_supported", "cached_const", "call", "cat_flip", "cat_flipped", "colour_windows", "conv3x3_bias", "conv3x3_bias_supported",
    "empty_nhwc", "fill_zero", "flip", "flip_masks", "flips_to_tensor", "global_head", "global_head_var", "global_joint", "global_mi",
    "global_mi_pair", "l2_perturb", "largest_component", "local_head", "local_head_var", "local_mi_heads", "local_mi_losses",
    "local_mi_raw_joint", "mi_precision_name", "normal_fill", "output_local_mi", "output_local_mi_supported", "philox_words", "query",
    "resolve_mi_precision", "set_mi_precision", "softmax_dice", "softmax_dice_supported", "softmax_entropy", "softmax_entropy_supported",
    "softmax_kl", "softmax_kl_consistency", "softmax_mse", "split_rows", "stem_dgrad", "stem_dgrad_supported", "supcon", "supcon_supported",
    "surface_stats", "wait_stream", "zero_counter",
]

FAMILIES = ["batch", "contrast", "heads", "losses", "metrics", "mi", "vat"]
# the one piece two families share: a loss kernel whose input is a part of a ``split_rows`` writes that part's rows of the batch gradient
SHARED = {("losses", "batch"): {"_scaled_grad", "_split_part_of"}, ("mi", "batch"): {"_split_part_of"}}

# (file, function, imported module) -> why the import is not at the top of the file
LAZY_IMPORTS = {
    ("tape.py", "_key", ".ops.mi"): "the tape key reads the local-MI precision; ops is the top layer",
}


def _sources():
    for folder in (MISEG, os.path.join(MISEG, "ops")):
        for name in sorted(os.listdir(folder)):
            if name.endswith(".py"):
                path = os.path.join(folder, name)
                with open(path) as f:
                    yield os.path.relpath(path, MISEG), ast.parse(f.read())


def _imported(node):
    """The modules an import statement names, relative ones with their dots (``from . import a, b`` names ``.a`` and ``.b``)."""
    if isinstance(node, ast.Import):
        return [a.name for a in node.names]
    dots = "." * node.level
    return [dots + node.module] if node.module else [dots + a.name for a in node.names]


def test_ops_offers_every_name_the_repository_uses():
    from miseg_amd import ops
    missing = [n for n in OPS_NAMES if not hasattr(ops, n)]
    assert not missing, missing
    assert not hasattr(ops, "_mi_precision")


def test_lower_layers_import_without_the_upper_ones():
    code = ("import sys\n"
            "import miseg_amd._rt, miseg_amd.stepio, miseg_amd.checks, miseg_amd.packcache, miseg_amd.tape\n"
            "assert 'miseg_amd.ops' not in sys.modules and 'miseg_amd.unet_ops' not in sys.modules, sorted(m for m in sys.modules if m.startswith('miseg_amd'))\n"
            "import miseg_amd.unet_ops\n"
            "assert 'miseg_amd.ops' not in sys.modules, sorted(m for m in sys.modules if m.startswith('miseg_amd'))\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=PKG, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]


def test_imports_inside_functions_are_the_listed_few():
    assert len(LAZY_IMPORTS) <= 8
    found = set()
    for rel, tree in _sources():
        for fn in ast.walk(tree):
            if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
                continue
            for node in ast.walk(fn):
                if isinstance(node, (ast.Import, ast.ImportFrom)):
                    assert fn.name not in ("forward", "backward"), (rel, fn.name, node.lineno)
                    found |= {(rel, fn.name, m) for m in _imported(node) if m.startswith(".") or m.split(".")[0] == "miseg_amd"}
    assert found == set(LAZY_IMPORTS), (sorted(found - set(LAZY_IMPORTS)), sorted(set(LAZY_IMPORTS) - found))


def test_the_tape_key_and_ops_read_one_precision():
    from miseg_amd import ops
    from miseg_amd.ops.mi import mi_precision_code          # what tape.StepTape._key calls
    try:
        ops.set_mi_precision("bf16x3")
        assert ops.mi_precision_name() == "bf16x3" and mi_precision_code() == ops.MI_PRECISIONS["bf16x3"] == 1
    finally:
        ops.set_mi_precision("fp32")
    assert ops.mi_precision_name() == "fp32" and mi_precision_code() == 0


def test_family_modules_are_independent_and_short():
    present = sorted(n[:-3] for n in os.listdir(os.path.join(MISEG, "ops")) if n.endswith(".py") and not n.startswith("_"))
    assert present == FAMILIES
    for rel, tree in _sources():
        folder, name = os.path.split(rel)
        if folder != "ops":
            continue
        with open(os.path.join(MISEG, rel)) as f:
            assert len(f.read().splitlines()) <= 450, rel
        if name[:-3] not in FAMILIES:
            continue
        for node in ast.walk(tree):
            if isinstance(node, (ast.Import, ast.ImportFrom)):
                for m in _imported(node):
                    other = m[1:].split(".")[0] if m.startswith(".") and not m.startswith("..") else \
                        (m.split(".")[2] if m.startswith("miseg_amd.ops.") else None)
                    if other in FAMILIES:
                        names = {a.name for a in node.names}
                        assert isinstance(node, ast.ImportFrom) and node.module == other and names <= SHARED.get((name[:-3], other), set()), \
                            (rel, m, sorted(names))
