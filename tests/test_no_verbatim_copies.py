"""The Python mirror keeps the reference's NAMES and signatures, not its bodies.

Two checks against the same-named reference file, both on the abstract syntax tree so that whitespace, comments, line
breaks and docstrings cannot hide (or fake) a match (round-5 review: the raw-line version of this test let a transcribed
``conv_encode`` through because ``int(a/b)`` and ``int(a / b)`` are different lines):

* no run of more than three consecutive identical statements anywhere in a file (the one tolerated block is the legacy
  ``feedback`` DeprecationWarning of ``Trellis.__init__`` whose text is API);
* no same-named function of ten or more statements shares 30 % or more of its statements with the reference's.

The reference's side is read from tests/golden/reference_fingerprints.json (written by ``python tests/golden/make_golden.py
--only fingerprints`` where the reference checkout exists): for every file of PAIRS the sequence of its normalised
statements and, per function, the statements of its body, each stored as a truncated SHA-256 of the normalised text.
Both checks only ask whether two statements are equal, so comparing fingerprints asserts exactly what comparing the
statements did, and the suite needs no copy of the reference."""
import ast
import collections
import difflib
import hashlib
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINGERPRINTS = os.path.join(ROOT, "tests", "golden", "reference_fingerprints.json")
PAIRS = [("channelcoding/convcode.py",) * 2, ("channelcoding/turbo.py",) * 2, ("channelcoding/ldpc.py",) * 2,
         ("channelcoding/interleavers.py",) * 2, ("modulation.py",) * 2, ("utilities.py",) * 2, ("links.py",) * 2,
         ("channels.py",) * 2, ("wifi80211.py",) * 2]
_BODIES = ("body", "orelse", "finalbody", "handlers")


def _is_docstring(node):
    return isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant) and isinstance(node.value.value, str)


def _flatten(stmts, out):
    """Statements in source order, one normalised string each; a compound statement contributes its header only and is
    then descended into."""
    for node in stmts:
        if _is_docstring(node):
            continue
        compound = any(getattr(node, f, None) for f in _BODIES if isinstance(getattr(node, f, None), list))
        if compound:
            out.append(ast.unparse(node).split("\n")[0])
            for f in _BODIES:
                sub = getattr(node, f, None)
                if isinstance(sub, list):
                    for h in sub:
                        if isinstance(h, ast.ExceptHandler):
                            out.append("except %s:" % (ast.unparse(h.type) if h.type else ""))
                            _flatten(h.body, out)
                    _flatten([s for s in sub if isinstance(s, ast.stmt)], out)
        else:
            out.append(ast.unparse(node))
    return out


def fingerprint(stmt):
    return hashlib.sha256(stmt.encode()).hexdigest()[:16]


def _reference(theirs):
    with open(FINGERPRINTS) as f:
        return json.load(f)["files"][theirs]


def _statements(path):
    return _flatten(ast.parse(open(path).read()).body, [])


def _functions(path):
    """{qualified name: [normalised statements of the body]} for every def, methods as Class.name."""
    found = {}

    def visit(body, prefix):
        for node in body:
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                found[prefix + node.name] = _flatten(node.body, [])
                visit(node.body, prefix + node.name + ".")
            elif isinstance(node, ast.ClassDef):
                visit(node.body, prefix + node.name + ".")
    visit(ast.parse(open(path).read()).body, "")
    return found


@pytest.mark.parametrize("ours,theirs", PAIRS)
def test_no_run_of_identical_statements(ours, theirs):
    mine = _statements(os.path.join(ROOT, "commpy_amd", ours))
    a = [fingerprint(s) for s in mine]
    b = _reference(theirs)["statements"]
    m = difflib.SequenceMatcher(None, a, b, autojunk=False).find_longest_match(0, len(a), 0, len(b))
    run = mine[m.a:m.a + m.size]
    if any("DeprecationWarning" in s for s in run):         # the warning text of the legacy-feedback Trellis path is API
        run = [s for s in run if "warn" not in s and "DeprecationWarning" not in s]
    assert len(run) <= 3, run


@pytest.mark.parametrize("ours,theirs", PAIRS)
def test_same_named_functions_share_under_30_percent(ours, theirs):
    mine = _functions(os.path.join(ROOT, "commpy_amd", ours))
    ref = _reference(theirs)["functions"]
    report = []
    for name, stmts in mine.items():
        if name not in ref or len(stmts) < 10:
            continue
        pool = collections.Counter(ref[name])
        shared = 0
        for s in map(fingerprint, stmts):
            if pool[s] > 0:
                pool[s] -= 1
                shared += 1
        if shared / len(stmts) >= 0.30:
            report.append((name, shared, len(stmts)))
    assert not report, report


def test_the_normaliser_sees_through_spacing_and_comments(tmp_path):
    """The property the raw-line version lacked."""
    a = tmp_path / "a.py"
    b = tmp_path / "b.py"
    a.write_text("def f(x, y):\n    '''doc'''\n    n = int(x/y)   # comment\n    if n:\n        return (n +\n                1)\n    return 0\n")
    b.write_text("def f(x, y):\n    n = int(x / y)\n    if n:\n        return n + 1\n    return 0\n")
    assert _statements(str(a)) == _statements(str(b))
    assert _functions(str(a))["f"] == ["n = int(x / y)", "if n:", "return n + 1", "return 0"]
