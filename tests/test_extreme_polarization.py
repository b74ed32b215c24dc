"""CPU: the spin polarization (mode 5) on the extreme cells of tests/extreme_cells.py, per bin -- the inputs and the metric of
tests/test_gpu_extreme_polarization.py before any device sees them.  The reference is the numpy restatement of
tests/test_gpu_polarization.py in long double, computed here (36 cells: milliseconds), no fixture.

Surfaces: fast-flow, far-eta, tau-extremes and isothermal-mix, both dimensions where the case has them; X.grid() (pT to 40 GeV); X.species()
plus a boson of the proton's mass (a fermion / boson pair of equal mass) and a Boltzmann copy of the pion; synth_vorticity(36); the
surface's single temperature T = 0.101, 0.151, 0.199.

Metric: every bin of St, Sx, Sy, Sn against max(|ref|, 1e-4 sum |summands|, 1e-280) -- the vorticity terms change sign from cell to cell --
and Snorm against max(|ref|, 1e-280).  The largest value of the array is not used.  The double restatement meets 1e-9 (half the device bound)."""
from functools import lru_cache

import numpy as np
import pytest

import extreme_cells as X
from is3d_amd import synth
from test_gpu_polarization import OUTS, restate

TOL_DOUBLE = 1e-9
FLOOR = 1e-280
SURFACES = [(c, d) for c in ("fast-flow", "far-eta", "tau-extremes", "isothermal-mix") for d in X.DIMS[c]]
TEMPERATURES = (0.101, 0.151, 0.199)
CASES = [(c, d, T) for c, d in SURFACES for T in TEMPERATURES]
IDS = ["%s-%d-T%.3f" % c for c in CASES]


@lru_cache(maxsize=None)
def species():
    sp = {k: np.asarray(X.species()[k], dtype=np.float64) for k in ("mass", "sign", "degeneracy", "baryon")}
    p, pi = X.species_ids().index(2212), X.species_ids().index(211)
    for src, sign in ((p, -1.0), (pi, 0.0)):
        for k in sp:
            sp[k] = np.append(sp[k], sp[k][src])
        sp["sign"][-1] = sign
    assert sp["sign"][p] == 1.0 and sp["sign"][pi] == -1.0 and len(sp["mass"]) == 7
    for v in sp.values():
        v.setflags(write=False)
    return sp


@lru_cache(maxsize=None)
def vorticity():
    return synth.synth_vorticity(X.N_CELLS)


@lru_cache(maxsize=None)
def reference(case, dim, T):
    """(outputs, scales) as doubles: the long-double restatement and what each bin's error is judged against"""
    assert np.finfo(np.longdouble).nmant >= 63
    ref, mag = restate(X.surface(case, dim), vorticity(), species(), X.grid(), T, dim, dtype=np.longdouble)
    out, scale = {}, {}
    for k in OUTS:
        out[k] = ref[k].astype(np.float64)
        s = np.abs(ref[k]) if k == "Snorm" else np.maximum(np.abs(ref[k]), 1e-4 * mag[k])
        scale[k] = np.maximum(s, FLOOR).astype(np.float64)
        out[k].setflags(write=False)
        scale[k].setflags(write=False)
    return out, scale


def errors(got, case, dim, T):
    """{output: worst error}; every value finite"""
    ref, scale = reference(case, dim, T)
    out = {}
    for k in OUTS:
        assert np.isfinite(got[k]).all(), k
        out[k] = float(np.max(np.abs(got[k] - ref[k]) / scale[k]))
    return out


@pytest.mark.parametrize("case,dim,T", CASES, ids=IDS)
def test_the_double_restatement_reproduces_the_long_double_one(case, dim, T):
    ref, _ = reference(case, dim, T)
    for k in OUTS:
        assert np.isfinite(ref[k]).all(), k
    assert np.count_nonzero(np.abs(ref["Snorm"]) > FLOOR) > 0.5 * ref["Snorm"].size
    err = errors(restate(X.surface(case, dim), vorticity(), species(), X.grid(), T, dim), case, dim, T)
    print("%s %d+1D T = %.3f: double against long double %s" % (case, dim, T, {k: "%.2e" % v for k, v in err.items()}))
    assert max(err.values()) < TOL_DOUBLE, err


def test_the_vorticity_terms_cancel_where_the_scale_says():
    """the 1e-4 sum |summands| term of the scale is in use: some bins of St .. Sn lie below it -- and Snorm has none such to hide"""
    n = 0
    for case, dim, T in CASES:
        ref, scale = reference(case, dim, T)
        n += sum(int(np.count_nonzero(scale[k] > np.maximum(np.abs(ref[k]), FLOOR))) for k in OUTS[:4])
        assert np.array_equal(scale["Snorm"], np.maximum(np.abs(ref["Snorm"]), FLOOR))
    assert n > 0
