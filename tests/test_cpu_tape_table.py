"""The launch tape's recording table, checked as text (csrc/tape.h, MISEG_TAPE).

``MISEG_TAPE(fn, a, b, ...)`` compiles just as well with two same-typed arguments swapped (H and W, gx and gy, two int64_t
sizes): the eager call is unaffected, only a replay goes wrong, and only where the swapped values differ.  So every
``extern "C"`` definition of csrc/*.hip is parsed here and its macro line is held against its own signature.  The parser
is also what tests/test_gpu_tape_entry_points.py measures its coverage against.
"""
import glob
import os
import re
from typing import Dict, List, NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd", "csrc")


class EntryPoint(NamedTuple):
    name: str
    file: str
    ret: str
    params: List[str]          # parameter names, in signature order
    types: List[str]           # their types, as written
    body: str                  # between the outer braces, comments stripped


_DEF = re.compile(r'extern\s+"C"\s+((?:const\s+)?\w+\s*\**)\s*(miseg_\w+)\s*\(([^()]*)\)\s*\{')
_LAUNCH = re.compile(r"\bhipLaunchKernelGGL\b|\blaunch_\w+\s*\(|\bhipMem\w*Async\b")

# Launching `int miseg_*(void* stream, ...)` entry points that do not record themselves, with the reason.
UNTAPED_ON_PURPOSE: Dict[str, str] = {}


def strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _split_args(s: str) -> List[str]:
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _matching(text: str, start: int, open_ch: str, close_ch: str) -> int:
    """Index of the bracket that closes the one at text[start]."""
    depth = 0
    for i in range(start, len(text)):
        if text[i] == open_ch:
            depth += 1
        elif text[i] == close_ch:
            depth -= 1
            if depth == 0:
                return i
    raise ValueError("unbalanced " + open_ch)


def parse_entry_points(csrc: str = CSRC) -> Dict[str, EntryPoint]:
    found: Dict[str, EntryPoint] = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        text = strip_comments(open(path).read())
        for m in _DEF.finditer(text):
            brace = m.end() - 1
            body = text[brace + 1:_matching(text, brace, "{", "}")]
            params, types = [], []
            args = m.group(3).strip()
            if args and args != "void":
                for a in _split_args(args):
                    pm = re.match(r"^(.*?)(\w+)\s*(\[\s*\d*\s*\])?$", a, flags=re.S)
                    assert pm, (path, m.group(2), a)
                    params.append(pm.group(2))
                    types.append(" ".join(pm.group(1).split()))
            name = m.group(2)
            assert name not in found, f"{name} is defined twice ({found[name].file}, {os.path.basename(path)})"
            found[name] = EntryPoint(name, os.path.basename(path), " ".join(m.group(1).split()), params, types, body)
    return found


def macro_args(ep: EntryPoint):
    """The arguments of the MISEG_TAPE(...) that opens the body, or None."""
    m = re.match(r"\s*MISEG_TAPE\s*\(", ep.body)
    if not m:
        return None
    open_at = m.end() - 1
    return _split_args(ep.body[open_at + 1:_matching(ep.body, open_at, "(", ")")])


def fn_op_recorders(eps: Dict[str, EntryPoint]) -> List[str]:
    return sorted(n for n, ep in eps.items() if "TapeFnOp" in ep.body)


def taped_entry_points(csrc: str = CSRC) -> List[str]:
    """Every entry point that puts itself on a recording tape: by the macro, or by a TapeFnOp of its own."""
    eps = parse_entry_points(csrc)
    return sorted({n for n, ep in eps.items() if macro_args(ep) is not None} | set(fn_op_recorders(eps)))


# ---------------------------------------------------------------------------------------------------------------------------
EPS = parse_entry_points()


def test_parser_sees_the_library():
    """Every prototype of the header that a .hip file defines is found, with the header's parameter count."""
    import sys
    sys.path.insert(0, os.path.dirname(CSRC))
    from miseg_amd import _cabi
    declared = _cabi.PROTOTYPES
    missing = sorted(set(declared) - set(EPS))
    assert not missing, f"declared in the header, definition not parsed: {missing}"
    for name, (_, argtypes) in declared.items():
        assert len(EPS[name].params) == len(argtypes), (name, EPS[name].params)
    assert len(taped_entry_points()) >= 100


def test_macro_names_its_own_function():
    bad = {n: macro_args(ep)[0] for n, ep in EPS.items() if macro_args(ep) is not None and macro_args(ep)[0] != n}
    assert not bad, f"MISEG_TAPE records another function than the one it stands in: {bad}"


def test_macro_arguments_are_the_parameters_in_order():
    bad = {}
    for n, ep in EPS.items():
        args = macro_args(ep)
        if args is not None and args[1:] != ep.params:
            bad[n] = {"macro": args[1:], "signature": ep.params}
    assert not bad, f"MISEG_TAPE arguments differ from the signature (a replay would pass them wrongly): {bad}"


def test_a_macro_is_the_first_statement_or_absent():
    """A MISEG_TAPE further down the body would record after a refusal had already returned, or twice."""
    late = sorted(n for n, ep in EPS.items() if "MISEG_TAPE" in ep.body and macro_args(ep) is None)
    assert not late, late
    twice = sorted(n for n, ep in EPS.items() if ep.body.count("MISEG_TAPE") > 1)
    assert not twice, twice


def test_taped_entry_points_take_the_stream_first():
    """tape_record stores its first argument as the op's stream (miseg_tape_op_stream, the timing events)."""
    bad = sorted(n for n in taped_entry_points() if not (EPS[n].ret == "int" and EPS[n].types[0].replace(" ", "") == "void*"))
    assert not bad, bad


def test_flip_is_the_only_hand_recorded_entry_point():
    assert fn_op_recorders(EPS) == ["miseg_flip"]
    ep = EPS["miseg_flip"]
    assert macro_args(ep) is None and 'op->name = "miseg_flip"' in ep.body and "op->stream = stream" in ep.body
    # its closure passes its own copy of every parameter, in signature order
    m = re.search(r"return\s+miseg_flip\s*\(", ep.body)
    open_at = m.end() - 1
    passed = [a.replace("call->", "") for a in _split_args(ep.body[open_at + 1:_matching(ep.body, open_at, "(", ")")])]
    short = {"N": "n", "C": "c", "H": "h", "W": "w", "elem_bytes": "eb"}
    assert passed == [short.get(p, p) for p in ep.params], passed
    init = re.search(r"Call\s*\{([^;]*)\}\s*\)\s*;", ep.body).group(1)
    want = ["stream", "in", "out", "N", "C", "H", "W", "{is[0], is[1], is[2], is[3]}", "{os[0], os[1], os[2], os[3]}", "elem_bytes", "flips"]
    assert _split_args(init) == want, _split_args(init)


def test_every_launching_entry_point_is_taped():
    taped = set(taped_entry_points())
    launching = sorted(n for n, ep in EPS.items()
                       if ep.ret == "int" and ep.types and ep.types[0].replace(" ", "") == "void*" and ep.params[0] == "stream" and _LAUNCH.search(ep.body))
    untaped = [n for n in launching if n not in taped]
    assert sorted(untaped) == sorted(UNTAPED_ON_PURPOSE), f"launch without recording themselves: {untaped}"
    assert all(len(r.split()) >= 3 for r in UNTAPED_ON_PURPOSE.values())
    stale = sorted(set(UNTAPED_ON_PURPOSE) & taped)
    assert not stale, stale


def test_every_taped_entry_point_has_a_replay_case():
    import test_gpu_tape_entry_points as T
    taped = set(taped_entry_points())
    named = set(T.CASES) | set(T.EXCLUDED)
    assert not taped - named, f"taped, but neither replayed by a case nor excluded: {sorted(taped - named)}"
    assert not named - taped, f"named by CASES / EXCLUDED, but not a taped entry point: {sorted(named - taped)}"
    assert not set(T.CASES) & set(T.EXCLUDED)
    assert len(T.EXCLUDED) <= 5 and all(len(r.split()) >= 3 for r in T.EXCLUDED.values())
