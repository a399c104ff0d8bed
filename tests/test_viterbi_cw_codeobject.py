"""CPU check of the fused Viterbi kernel's sources: hipcc cross-compiles csrc/viterbi_cw.hip for gfx950 as the code object of one
64-state generator pair (commpy_amd/jit.py -- the mirrored-ring flavour of the headline kernel, with the lean branch metrics and the
flush of the fused path) and the image holds exactly the six kernels cpx_trellis_attach_viterbi_code looks up by name: a change of
the kernel's template signature, or a source that no longer compiles for the device, fails here without a GPU."""
import os
import re
import shutil

import pytest


def test_k7_pair_code_object_holds_the_kernels_the_library_asks_for(tmp_path, monkeypatch):
    from commpy_amd import build, jit
    if shutil.which(build._hipcc()) is None and not os.path.exists(build._hipcc()):
        pytest.skip("no hipcc here")
    monkeypatch.setenv("CPX_JIT_CACHE", str(tmp_path))
    lg, g0, g1 = 6, 0o135, 0o147                                  # K = 7, a pair that is not built in
    image = jit.viterbi_code_object(lg, g0, g1)
    assert image is not None, jit.viterbi_code_object.last_error
    assert image[:4] == b"\x7fELF"
    for typ in range(3):
        for rt in (False, True):
            sym = jit.kernel_symbol(lg, g0, g1, typ, rt)
            assert sym.encode() in image, sym
            # the mangled name carries the template arguments the dispatcher's own instantiations use: 28 hops, float64, 32-slot mirrored ring
            assert re.fullmatch(r"_ZN12_GLOBAL__N_123viterbi_cw_fused_kernelILi6ELj%dELj%dELi%dELi28ELb%dEdLi32ELb1EEEvNS_8CwParamsE"
                                % (g0, g1, typ, int(rt)), sym), sym
    found = set(re.findall(rb"viterbi_cw_fused_kernelILi(\d+)ELj(\d+)ELj(\d+)ELi(\d)ELi28ELb([01])E", image))
    assert found == {(b"6", b"%d" % g0, b"%d" % g1, b"%d" % t, b"%d" % r) for t in range(3) for r in range(2)}, found
    assert b"viterbi_cw_acs_kernel" not in image and b"viterbi_cw_tb_kernel" not in image
