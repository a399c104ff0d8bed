"""The kernel-path switches (csrc/runtime.hip): one table behind cpx_set_precision, cpx_get_precision and the cpx_*_set_path
setters, read from the environment on first use.  The setters touch no device, so all of this runs on a CPU-only host."""
import os
import re
import subprocess
import sys

import pytest

from commpy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every documented name of every setter (include/commpy_amd.h), aliases included
SETTERS = {
    "cpx_set_precision": ("fp64-parity", "fp32-fast", "fp64", "fp32"),
    "cpx_viterbi_set_path": ("auto", "wave", "cw", "cw!", "cw2", "cw2!", "general"),
    "cpx_ldpc_set_path": ("auto", "tiled", "resident", "resident-log"),
    "cpx_demod_set_path": ("auto", "plain", "libm"),
    "cpx_kbest_set_path": ("auto", "general"),
    "cpx_best_first_set_path": ("auto", "general"),
}
# rows of INTEGRATION.md's environment table that are not kernel-path switches
NON_SWITCH_ENV = {"CPX_LIB_PATH", "CPX_VITERBI_JIT", "CPX_JIT_CACHE", "HIPCC", "CPX_CACHE_DIR", "CPX_TRACE", "CPX_COMM_NONCE",
                  "CPX_EXPECT_GPUS", "CPX_REFERENCE_PATH"}


@pytest.fixture
def lib():
    lib = _lib.load()
    yield lib
    for setter in SETTERS:
        getattr(lib, setter)(None)


@pytest.mark.parametrize("setter", sorted(SETTERS))
def test_setters_accept_their_names_and_refuse_others(lib, setter):
    fn = getattr(lib, setter)
    for name in SETTERS[setter]:
        assert fn(name.encode()) == _lib.CPX_OK, (setter, name)
    for reset in ([None, b""] if setter == "cpx_set_precision" else [None, b"", b"auto"]):
        assert fn(reset) == _lib.CPX_OK, (setter, reset)
    for bad in ([b"bogus", b"wx", b"auto"] if setter == "cpx_set_precision" else [b"bogus", b"wx", b"c2", b"wave2", b"Auto"]):
        assert fn(bad) == _lib.CPX_EINVAL, (setter, bad)
        err = _lib.last_error()
        assert setter in err and bad.decode() in err, err
        assert all(name in err for name in SETTERS[setter]), err


def test_precision_round_trip(lib):
    _lib.set_precision("fp32-fast")
    assert _lib.get_precision() == "fp32-fast"
    _lib.set_precision(None)
    assert _lib.get_precision() == "fp64-parity"
    _lib.set_precision("fp32")
    assert _lib.get_precision() == "fp32-fast"
    _lib.set_precision("fp64")
    assert _lib.get_precision() == "fp64-parity"
    with pytest.raises(ValueError):
        _lib.set_precision("fp16")
    assert _lib.get_precision() == "fp64-parity"


def _precision_in_fresh_process(env_value, reset_first):
    code = ("from commpy_amd import _lib\n"
            + ("_lib.set_precision(None)\n" if reset_first else "")
            + "print(_lib.get_precision())\n")
    env = dict(os.environ, CPX_PRECISION=env_value)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.strip()


def test_environment_sets_the_initial_mode_and_a_setter_wins():
    assert _precision_in_fresh_process("fp32-fast", reset_first=False) == "fp32-fast"
    assert _precision_in_fresh_process("fp32-fast", reset_first=True) == "fp64-parity"
    assert _precision_in_fresh_process("bogus", reset_first=False) == "fp64-parity"     # unknown values leave the default


def _switch_table_env_vars():
    src = open(os.path.join(ROOT, "commpy_amd", "csrc", "runtime.hip")).read()
    table = re.search(r"kSwitches\[\] = \{(.*?)\n\};", src, flags=re.S)
    assert table, "switch table not found in runtime.hip"
    return set(re.findall(r'\{"(CPX_[A-Z_]+)"', table.group(1)))


def _documented_env_vars():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = re.search(r"^## Environment variables.*?$(.*?)(?=^## |\Z)", doc, flags=re.S | re.M)
    assert section, "no 'Environment variables' section in INTEGRATION.md"
    names = set()
    for row in re.findall(r"^\| *(`.*?) *\|", section.group(1), flags=re.M):
        names.update(re.findall(r"`([A-Z_]+)`", row))
    return names


def test_switch_table_matches_the_documented_environment_variables():
    switches = _switch_table_env_vars()
    assert len(switches) == 8, switches
    documented = _documented_env_vars()
    assert NON_SWITCH_ENV <= documented, NON_SWITCH_ENV - documented
    assert switches == documented - NON_SWITCH_ENV, (switches ^ (documented - NON_SWITCH_ENV))


def test_forced_path_resets_even_when_the_block_raises(lib, monkeypatch):
    calls = []
    real = _lib._set_mode

    def spy(setter, mode):
        calls.append((setter, mode))
        real(setter, mode)

    monkeypatch.setattr(_lib, "_set_mode", spy)
    for kind, mode in (("viterbi", "wave"), ("ldpc", "tiled"), ("demod", "plain"), ("kbest", "general"), ("best_first", "general")):
        calls.clear()
        with pytest.raises(KeyError):
            with _lib.forced_path(kind, mode):
                raise KeyError("inside the block")
        setter = "cpx_%s_set_path" % kind
        assert calls == [(setter, mode), (setter, None)], calls
    calls.clear()
    with pytest.raises(ValueError):
        with _lib.forced_path("viterbi", "wx"):                    # refused by the setter: nothing to reset
            pass
    with pytest.raises(ValueError):
        with _lib.forced_path("turbo", "wave"):
            pass
    assert calls == [("cpx_viterbi_set_path", "wx")], calls
