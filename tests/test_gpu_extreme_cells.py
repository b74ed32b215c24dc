"""GPU (-m gpu): the three momentum-spectrum families on the extreme cells of tests/extreme_cells.py, held to the committed numpy long-double
spectra of tests/golden/golden_extreme.npz (tests/golden/make_golden_extreme.py) -- the one check of these kernels not written in C by the hand
that wrote them.  Flow to gamma = 20, T on the edges of the coefficient table, pi^{mu nu} times 25 with bulkPi = -0.9 P / +0.5 P, |eta| to 7,
tau = 0.05 / 50, the whole (alpha_L, Lambda) table and mu_B on its last node reach the factorised exponent pT D'_j - mT C'_k (two terms of order
1e3 .. 1e4 cancelling to order 10), the Dmax / Cmin bounds of the unit cull, the spline's first and last interval, the delta-f clamp on most
of the grid, and the modified-equilibrium matrix near singular, breakdown cells and narrow rows included.  tests/test_extreme_cells.py shows on
the CPU that the oracle meets 1e-9 on every case.

TOL = 2e-9, the 3+1D bound of tests/test_gpu_parity.py, on every bin against max(|ref|, 1e-280); the raw cases (outflow = 0,
regulate_deltaf = 0) against the cancellation-aware scale of tests/test_gpu_fuzz.py.  Why it should hold: in bins above 1e-280 the exponent's
summands stay below about 1e4 (pT u_perp / T at 40 GeV, gamma = 20, T = 0.14 is 5 800), so some 50 roundings x 1e4 x 2^-53 are near 1e-10.
Culls on, exact-only and off are bitwise equal; breakdown, narrow and skipped counts are the fixture's.

Worst errors on an MI355X are in DESIGN.md (section 2, "Extreme cells"): 3.1e-10 (anisotropic hydro, isothermal-mix, regulate_deltaf = 0), 1.4e-10
(modified equilibrium, fast-flow), 4.4e-11 (delta-f).  No case needed a conditioning factor and no defect was found.

Sensitivity, once, on a scratch build: with the tile's Dmax formed from 7 of its 8 phi (cf_prep, a bound that misses a term) the four 3+1D fast-flow
and the two raw 3+1D isothermal-mix cases of test_deltaf_spectra fail -- exp(pT (D'_j - Dmax)) overflows at gamma = 20 and the spectrum is not
finite -- with 36 cells; of the older files only runs of 1 300 cells and more notice (tests/test_gpu_rowgroup_cull.py, tests/test_gpu_parity.py,
the counts test of tests/test_gpu_pds_cull.py), as a cull that is no longer bitwise."""
from functools import lru_cache

import numpy as np
import pytest

import extreme_cells as X
import test_gpu_pds_cull as pc
from is3d_amd import api, inputs
from oracle import oracle
from test_extreme_cells import df_tables, error, fq_for

pytestmark = pytest.mark.gpu

TOL = 2e-9            # tests/test_gpu_parity.py, 3+1D


def cases(family):
    cs = X.fixture_cases(family)
    return pytest.mark.parametrize("case", cs, ids=[c["key"] for c in cs])


def held(got, case, what):
    assert np.isfinite(got).all(), (case["key"], what)
    err = error(got, case)
    assert err < TOL, (case["key"], what, err)
    return err


@pytest.mark.devlib
@cases("df")
def test_deltaf_spectra(case):
    """default kernel and the 8 x 7 tile without the E2 stream (the developer build adds its own variants), one and three cell chunks; the row
    culls on / exact-only / off give the same bits and the counts of tests/test_gpu_pds_cull.py::three_modes; three shards on one device"""
    cells, o, dim = X.fixture_cells(case["cells"]), case["opts"], case["dim"]
    sp, g, df = X.species(), X.grid(), df_tables(False)
    flags = {k: v for k, v in o.items() if k not in ("dimension", "df_mode")}
    worst = 0.0
    if dim == 3:
        for variant in pc.variants():
            for nch in (1, 3):
                got, (s0, _, _) = pc.three_modes(cells, sp, g, df, o["df_mode"], variant, cell_chunks=nch, **flags)
                assert s0["n_cells_skipped"] == case["n_skipped"] and s0["bad_cell"] == -1
                worst = max(worst, held(got, case, (variant, nch)))
    else:
        for nch in (1, 3):
            runs = [api.smooth_spectra(cells, sp, g, df, dict(o, cell_chunks=nch, zero_skip=zs)) for zs in (0, 1, 2)]
            assert np.array_equal(runs[0][0], runs[2][0]) and np.array_equal(runs[1][0], runs[2][0]), nch
            assert runs[0][1]["n_cells_skipped"] == case["n_skipped"] and runs[0][1]["bad_cell"] == -1
            worst = max(worst, held(runs[0][0], case, nch))
    multi, _, shards = api.smooth_spectra_multi(cells, sp, g, df, o, devices=[0] * 3)
    assert len(shards) == 3
    worst = max(worst, held(multi, case, "three shards"))
    print("%s: worst error against long double %.3e" % (case["key"], worst))


@cases("dfb")
def test_deltaf_spectra_with_baryon(case):
    cells, o = X.fixture_cells(case["cells"]), case["opts"]
    sp, g, df = X.species(), X.grid(), df_tables(True)
    worst = 0.0
    for nch in (1, 3):
        runs = [api.smooth_spectra(cells, sp, g, df, dict(o, cell_chunks=nch, zero_skip=zs)) for zs in (0, 1, 2)]
        assert np.array_equal(runs[0][0], runs[2][0]) and np.array_equal(runs[1][0], runs[2][0]), nch
        assert runs[0][1]["n_cells_skipped"] == case["n_skipped"] and runs[0][1]["bad_cell"] == -1
        worst = max(worst, held(runs[0][0], case, nch))
    multi, _, _ = api.smooth_spectra_multi(cells, sp, g, df, o, devices=[0] * 3)
    worst = max(worst, held(multi, case, "three shards"))
    print("%s: worst error against long double %.3e" % (case["key"], worst))


@cases("fq")
def test_modified_equilibrium_spectra(case):
    cells, o = X.fixture_cells(case["cells"]), case["opts"]
    fq = fq_for(cells)
    on, s0 = api.smooth_spectra(cells, X.species(), X.grid(), df_tables(False), o, fq=fq)
    off, s2 = api.smooth_spectra(cells, X.species(), X.grid(), df_tables(False), dict(o, zero_skip=2), fq=fq)
    assert np.array_equal(on, off)
    for st in (s0, s2):
        assert st["n_cells_breakdown"] == case["n_breakdown"] and st["n_cells_skipped"] == case["n_skipped"] and st["bad_cell"] == -1
        assert st["n_cells_narrow"] == case["n_narrow_cells"]
    print("%s: error against long double %.3e (breakdown %d, narrow cells %d, narrow rows %d)" % (
        case["key"], held(on, case, "feqmod"), case["n_breakdown"], case["n_narrow_cells"], case["n_narrow_rows"]))


@lru_cache(maxsize=None)
def vah_tables():
    return inputs.vah_df_tables()


@cases("vah")
def test_anisotropic_hydro_spectra(case):
    """with the cells' own coefficients (scipy's, as committed) and with the coefficients the device interpolates from the tables"""
    cells, o = X.fixture_cells(case["cells"]), case["opts"]
    worst = {}
    for name, tab in (("cells", None), ("tables", vah_tables())):
        on, s0 = api.smooth_spectra_vah(cells, X.species(), X.grid(), o, tab=tab)
        off, _ = api.smooth_spectra_vah(cells, X.species(), X.grid(), dict(o, zero_skip=2), tab=tab)
        assert np.array_equal(on, off) and s0["bad_cell"] == -1, name
        worst[name] = held(on, case, name)
    print("%s: error against long double %.3e with the cells' coefficients, %.3e from the tables" % (case["key"], worst["cells"], worst["tables"]))


def outcome(run):
    """('value', spectrum) or ('domain', text)"""
    try:
        return "value", run()
    except api.Is3dError as e:
        assert e.code == api.IS3D_EDOMAIN
        return "domain", str(e)
    except (RuntimeError, ValueError) as e:
        return "domain", str(e)


@pytest.mark.parametrize("df_mode", [1, 2, 3, 4])
@pytest.mark.parametrize("dim", [3, 2])
def test_a_cell_exactly_on_a_table_node_ends_as_the_oracle_says(dim, df_mode):
    """T exactly on the first and on the last node of the coefficient table, one cell each: a value where the oracle gives a value, and
    IS3D_EDOMAIN naming the cell where the oracle's spline refuses"""
    sp, g, df = X.species(), X.grid(), df_tables(False)
    o = dict(dimension=dim, df_mode=df_mode)
    for i in (0, 1):
        cells = {k: v[i:i + 1] for k, v in X.exact_nodes(dim).items()}
        fq = fq_for(X.exact_nodes(dim)) if df_mode >= 3 else None
        if fq:
            want = outcome(lambda: oracle.dN_pTdpTdphidy_feqmod(cells, sp, g, df, fq, o)[0])
        else:
            want = outcome(lambda: oracle.dN_pTdpTdphidy(cells, sp, g, df, o))
        got = outcome(lambda: api.smooth_spectra(cells, sp, g, df, o, fq=fq)[0])
        print("T = %r, %d+1D, df_mode %d: oracle %s, device %s" % (float(cells["T"][0]), dim, df_mode, want[0], got[0]))
        assert got[0] == want[0], (got, want)
        if want[0] == "value":
            err = float(np.max(np.abs(got[1] - want[1]) / np.maximum(np.abs(want[1]), 1e-280)))
            assert np.isfinite(got[1]).all() and err < TOL, err
        else:
            assert "cell 0:" in got[1]
