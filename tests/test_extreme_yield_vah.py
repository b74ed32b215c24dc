"""CPU: the mean yield of an anisotropic-hydro surface on the extreme VAH cells of tests/extreme_cells.py (the committed cells of
tests/golden/golden_extreme.npz with their scipy coefficients; `anisotropy` covers the whole (alpha_L, Lambda) table) -- the reference and
the bound of tests/test_gpu_extreme_yield_vah.py before any device sees them.  The reference is tests/vah_yield_ref.py in long double; the
bound is the 1e-11 that tests/test_gpu_total_yield_vah.py already holds against that restatement, relative, per species.  The double
restatement meets half of it here, on every whole surface and on every single-cell slice (worst 2.7e-12, one cell of fast-flow 3+1D: the
local-rest-frame shear components at gamma = 20), so the plain relative error is used and no cancellation-aware scale is needed."""
from functools import lru_cache

import numpy as np
import pytest

import extreme_cells as X
import vah_yield_ref as ref
from is3d_amd import inputs

RTOL = 1.0e-11        # tests/test_gpu_total_yield_vah.py
Y_CUT = 0.8
SURFACES = [(c, d) for c in X.VAH_CASES for d in X.DIMS[c]]
IDS = ["%s-%d" % s for s in SURFACES]
LD = np.longdouble


@lru_cache(maxsize=None)
def gla():
    return inputs.feqmod_tables(0.15)


def cells_of(case, dim):
    return X.fixture_cells("%s_%dv" % (case, dim))


def one(v, c):
    return {k: a[c:c + 1] for k, a in v.items()}


@lru_cache(maxsize=None)
def reference(case, dim):
    """long double, rounded to double: (yield_by_species [S] of the whole surface, [36][S] of every single-cell slice, skipped cells)"""
    assert np.finfo(LD).nmant >= 63
    v, o = cells_of(case, dim), dict(dimension=dim)
    _, by, skipped = ref.total_yield_vah_ref(v, X.species(), gla(), o, y_cut=Y_CUT, dtype=LD)
    cells = np.stack([ref.total_yield_vah_ref(one(v, c), X.species(), gla(), o, y_cut=Y_CUT, dtype=LD)[1] for c in range(X.N_CELLS)])
    dead = np.flatnonzero(~X.live(v))
    assert skipped == len(dead) == len(X.expected_skipped(case)) and (cells[dead] == 0).all() and (np.delete(cells, dead, axis=0) != 0).all()
    return by.astype(np.float64), cells.astype(np.float64), dead


def rel(got, want):
    """worst relative error; an exact zero must be met exactly"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(got == 0.0, want == 0.0)
    return float(np.max(np.abs(got - want) / np.where(want == 0.0, 1.0, np.abs(want))))


@pytest.mark.parametrize("case,dim", SURFACES, ids=IDS)
def test_the_double_restatement_meets_half_the_device_bound(case, dim):
    v, o = cells_of(case, dim), dict(dimension=dim)
    want_by, want_cells, _ = reference(case, dim)
    assert np.isfinite(want_by).all() and np.isfinite(want_cells).all()
    _, by, _ = ref.total_yield_vah_ref(v, X.species(), gla(), o, y_cut=Y_CUT)
    cells = np.stack([ref.total_yield_vah_ref(one(v, c), X.species(), gla(), o, y_cut=Y_CUT)[1] for c in range(X.N_CELLS)])
    print("%s %d+1D: double against long double, whole surface %.2e, single cells %.2e" % (case, dim, rel(by, want_by), rel(cells, want_cells)))
    assert rel(by, want_by) <= 0.5 * RTOL and rel(cells, want_cells) <= 0.5 * RTOL


def test_the_long_double_form_leaves_the_double_form_alone():
    v = cells_of("anisotropy", 3)
    a = ref.total_yield_vah_ref(v, X.species(), gla(), dict(dimension=3), y_cut=Y_CUT)
    assert isinstance(a[0], float) and a[1].dtype == np.float64
    b = ref.total_yield_vah_ref(v, X.species(), gla(), dict(dimension=3), y_cut=Y_CUT, dtype=LD)
    assert b[1].dtype == LD and rel(a[1], b[1]) < 1e-14 and a[2] == b[2]
