"""GPU (-m gpu): is3d_total_yield_vah (cf_yield_vah.hip: three radial integrals per (cell, class)) on the extreme VAH cells of
tests/extreme_cells.py -- flow to gamma = 20, stresses x 25, |eta| to 7, tau = 0.05 / 50, and with `anisotropy` the whole (alpha_L, Lambda)
coefficient table, where it had only run with alpha_L in [0.7, 1.2] -- against the long-double restatement of
tests/test_extreme_yield_vah.py, per species: once on the whole surface and once per single-cell slice with first_cell set, with the cells'
own coefficients and with tab=.  RTOL = 1e-11 relative, the bound tests/test_gpu_total_yield_vah.py holds against the same restatement (the
double restatement meets half of it on these cells, tests/test_extreme_yield_vah.py); the skipped cells of isothermal-mix contribute
exactly 0.

Worst errors on an MI355X over the whole surface and the 36 single-cell slices, cells' coefficients and tables (also DESIGN.md, section 2,
"Extreme cells"): 3+1D 1.7e-12 (fast-flow), 2+1D 5.1e-14 (large-stress); anisotropy 3+1D / 2+1D below 1e-13.  No defect was found."""
from functools import lru_cache

import numpy as np
import pytest

import extreme_cells as X
from is3d_amd import api, inputs
from test_extreme_yield_vah import IDS, RTOL, SURFACES, Y_CUT, cells_of, gla, one, reference, rel

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def vah_tables():
    return inputs.vah_df_tables()


@pytest.mark.parametrize("case,dim", SURFACES, ids=IDS)
def test_yields_against_long_double(case, dim):
    v, o = cells_of(case, dim), dict(dimension=dim)
    want_by, want_cells, dead = reference(case, dim)
    for what, tab in (("cells", None), ("tables", vah_tables())):
        N, by, st = api.total_yield_vah(v, X.species(), gla(), o, tab=tab, y_cut=Y_CUT)
        assert st["n_cells_skipped"] == len(dead) and np.isfinite(by).all()
        err = rel(by, want_by)
        assert err <= RTOL and rel(N, np.cumsum(want_by)[-1]) <= RTOL, (case, dim, what, err)
        got = np.zeros_like(want_cells)
        for c in range(X.N_CELLS):
            _, got[c], st1 = api.total_yield_vah(one(v, c), X.species(), gla(), o, tab=tab, y_cut=Y_CUT, first_cell=1000 + c)
            assert st1["n_cells_skipped"] == int(c in dead)
        assert (got[dead] == 0.0).all()
        err1 = rel(got, want_cells)
        print("%s %d+1D %s: device against long double, whole surface %.2e, single cells %.2e" % (case, dim, what, err, err1))
        assert err1 <= RTOL, (case, dim, what, err1)
