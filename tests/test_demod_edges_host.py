"""CPU half of the demodulation edge-case tests: the oracle the GPU tests compare against (oracle.demodulate) is pinned here to
the reference rule written as literal NumPy, on the edge inputs of tests/demod_edges.py, and the contract classifier of that
module is checked on hand-built cases.

The oracle builds each symbol as ``re + im * _Complex_I`` (oracle/cpx_oracle.c), which for an infinite imaginary part gives a NaN
real part; the distances, and so every decision and LLR, come out as the reference's all the same -- these tests keep it so."""
import numpy as np
import pytest

import oracle
from demod_edges import (BIG, EXACT, ROUND, TIE, edge_symbols, hard_contract, labels_of, same_soft, soft_literal)

NOISE_VARS = (0.5, 1e-295, 1e295, 0.0, -0.5, np.inf, np.nan, 5e-324)


def _qam(m):
    """QAMModem(m)'s table, restated (odd-integer grid, snake order, Gray re-indexed)."""
    side = int(np.sqrt(m))
    pam = np.arange(-side + 1, side, 2)
    c = pam.repeat(side) + 1j * np.tile(np.hstack((pam, pam[::-1])), side // 2)
    idx = np.arange(m)
    return c[(idx ^ (idx >> 1)).argsort()]


def _psk(m):
    c = np.exp(1j * np.arange(0, 2 * np.pi, 2 * np.pi / m))
    idx = np.arange(m)
    return c[(idx ^ (idx >> 1)).argsort()]


TABLES = {"qam4": lambda: _qam(4), "qam16": lambda: _qam(16), "qam64": lambda: _qam(64), "psk8": lambda: _psk(8),
          "random16": lambda: (lambda rs: rs.randn(16) + 1j * rs.randn(16))(np.random.RandomState(16))}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_oracle_hard_is_the_reference_rule_on_edges(name):
    """Exact and tied symbols: the oracle's label is the literal ``abs(y - c[:, None]).argmin(0)``.  Within the rounding band
    glibc's cabs and NumPy's complex abs may round differently, so there both must lie in the band -- the same contract the
    kernels are held to."""
    c = TABLES[name]()
    y, cls = edge_symbols(c, np.random.RandomState(1))
    nb = int(np.log2(c.size))
    kind, band, ref = hard_contract(c, y)
    with np.errstate(all="ignore"):
        literal = np.abs(y - c[:, None]).argmin(0)
    assert np.array_equal(literal, ref)
    got = labels_of(oracle.demodulate(c, y, "hard"), nb)
    pinned = kind != ROUND
    assert np.array_equal(got[pinned], ref[pinned])
    for i in np.nonzero(kind == TIE)[0]:
        assert got[i] == min(band[i])
    for i in np.nonzero(kind == ROUND)[0]:
        assert int(got[i]) in band[i] and int(ref[i]) in band[i], (y[i], got[i], ref[i], band[i])
    nonfin = ~(np.isfinite(y.real) & np.isfinite(y.imag)) | (cls == "overflow")
    assert np.all(got[nonfin] == 0) and np.all(kind[nonfin] == EXACT)
    assert np.any(kind[cls == "big"] == ROUND)                   # the large-magnitude class really reaches the band


@pytest.mark.parametrize("nv", NOISE_VARS)
@pytest.mark.parametrize("name", sorted(TABLES))
def test_oracle_soft_is_the_reference_rule_on_edges(name, nv):
    """The oracle's LLRs against the literal sums in constellation order: NaN / +inf / -inf exactly where the rule has them,
    finite values to the last few ulps (glibc's exp and NumPy's differ by an ulp here and there)."""
    c = TABLES[name]()
    y, _ = edge_symbols(c, np.random.RandomState(2))
    got = oracle.demodulate(c, y, "soft", nv)
    want = soft_literal(c, y, nv)
    assert same_soft(got, want, tol=0.0).size == np.sum(np.isfinite(want) & (got != want))     # only finite values differ
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-12 * np.maximum(1.0, np.abs(want[fin])))


def test_contract_classifier_hand_built():
    """EXACT / TIE / ROUND on cases worked out by hand for 16-QAM (levels -3, -1, 1, 3 on both axes)."""
    c = _qam(16)
    lab = {complex(p): m for m, p in enumerate(c)}
    y = np.array([
        1 + 1j,                                     # on a point: EXACT
        0.999 + 1.001j,                             # near a point: EXACT
        2 + 1j,                                     # midpoint between 1 and 3 on the real axis: TIE of two labels
        2 + 2j,                                     # midpoint on both axes: TIE of four
        0j,                                         # the origin: TIE of the four inner points
        complex(np.nextafter(2.0, 3.0), 1.0),       # one ulp past the boundary: EXACT (3 + 1j)
        complex(2.0 + 2.0 ** -30, 1e5),             # near the boundary under a huge imaginary part: ROUND
        complex(0.3, np.inf),                       # non-finite: EXACT, label 0
        complex(np.nan, 0.3),
        complex(1.3e308, 1.5e308),                  # hypot overflows for every point: EXACT, label 0
    ])
    kind, band, ref = hard_contract(c, y)
    assert list(kind) == [EXACT, EXACT, TIE, TIE, TIE, EXACT, ROUND, EXACT, EXACT, EXACT]
    assert ref[0] == lab[1 + 1j] and ref[1] == lab[1 + 1j] and ref[5] == lab[3 + 1j]
    assert sorted(band[2]) == sorted([lab[1 + 1j], lab[3 + 1j]]) and ref[2] == min(band[2])
    assert sorted(band[3]) == sorted(lab[complex(a, b)] for a in (1, 3) for b in (1, 3))
    assert sorted(band[4]) == sorted(lab[complex(a, b)] for a in (-1, 1) for b in (-1, 1))
    assert sorted(band[6]) == sorted([lab[1 + 3j], lab[3 + 3j]])        # the two points nearest 2 + 1e5j
    assert ref[7] == 0 and ref[8] == 0 and ref[9] == 0


def test_contract_band_edges():
    """The band is 2^-51 of the distance wide: two candidates 2^-52 apart at distance ~1 share it, 2^-51 apart they do not."""
    c = np.array([0.0 + 0j, 2.0 + 0j])
    # y = 1 + d: distances 1 + d and 1 - d, 2 |d| apart
    for d, want in ((0.0, TIE), (-2.0 ** -53, ROUND), (2.0 ** -52, EXACT)):
        kind, band, _ = hard_contract(c, np.array([1.0 + d + 1e-300j]))
        assert kind[0] == want, (d, kind[0])
    kind, _, ref = hard_contract(c, np.array([complex(np.inf, 0.0), complex(-np.inf, np.nan)]))
    assert list(kind) == [EXACT, EXACT] and list(ref) == [0, 0]


def test_edge_symbols_cover_every_class():
    c = _qam(64)
    y, cls = edge_symbols(c, np.random.RandomState(0))
    for name in ("point", "mid1", "mid2", "origin", "pairmid", "ulp", "big", "nonfinite", "overflow", "subnormal"):
        assert np.any(cls == name), name
    nonfin = y[cls == "nonfinite"]
    for re_kind in (np.isfinite, np.isposinf, np.isneginf, np.isnan):
        for im_kind in (np.isfinite, np.isposinf, np.isneginf, np.isnan):
            if re_kind is np.isfinite and im_kind is np.isfinite:
                continue
            assert np.any(re_kind(nonfin.real) & im_kind(nonfin.imag)), (re_kind.__name__, im_kind.__name__)
    for B in BIG:
        assert np.any(np.abs(y.imag[cls == "big"]) == B) and np.any(np.abs(y.real[cls == "big"]) == B)
    assert np.any(np.signbit(y.real) & (y.real == 0)) and np.any((np.abs(y.real) > 0) & (np.abs(y.real) < 2.3e-308))
