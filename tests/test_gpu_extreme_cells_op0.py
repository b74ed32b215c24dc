"""GPU (-m gpu): operation 0 -- cf_st_cells (cf_spacetime.hip), cf_spacetime_feqmod.hip, cf_spacetime_vah.hip -- on the extreme cells of
tests/extreme_cells.py, per cell and per pT node, held to the committed numpy long-double values of tests/golden/golden_extreme_op0.npz
(tests/golden/make_golden_extreme_op0.py).  These kernels share the physics of the spectrum kernels but have their own arithmetic: their own
factorisation of the exponent (E2_j = exp(pT D'_j - bmax), E1 = exp(bmax - mT C'_k), bmax the maximum over the phi of a tile), their own
wave-uniform row skip, one reciprocal of d.x in the Chapman-Enskog branch, the clamp and the outflow cut formed inline.  Before this file they
had only seen gamma <= 1.2 and T in [0.140, 0.160], and dN_dy_cell under the shipped Gauss weights, which the lowest pT nodes decide.

Seven pT weight vectors (tests/extreme_cells.py: all ones and the unit vectors e_0 .. e_5, pT = 0.05 .. 40 GeV) with a seeded positive phi_w:
under e_i, dN_dy_cell is the (phi, y | eta) sum of a cell at node i alone.  Every entry of dN_dy_cell within TOL = 2e-9 of the fixture in the
metric of tests/test_extreme_cells_op0.py (the bound of tests/test_gpu_extreme_cells.py; the same exponent: 50 roundings x 1e4 x 2^-53),
with opts.cell_chunks 1 and 3 (operation 0 sizes its chunks from the lane waves and does not read the option: the second run shows it
harmless); skipped, breakdown, renorm-skipped and bad-cell counts are the fixture's; zero_skip 0 / 2 the same bits; the tau / r / tau x r
histograms the left-to-right sums of the device's own dN_dy_cell (bins that leave tau-extremes cells outside on both sides); the 2+1D
dN_dydeta at the nodes 0, 60, 120, 180, 240; three shards on one device bitwise the single-device result but for the 2+1D dN_dydeta (TOL).
Anisotropic hydro runs with the cells' own coefficients and with tab= (it has no multi-device operation 0).  The 2+1D modified-equilibrium
cases carry the six nodes in a nine-node pT grid whose last three weights are zero (tests/extreme_cells.py, op0_grid: the kernel's 48 KiB of
eta rows refuse 6 pT x 241 eta, a documented limit), which changes no value asked here.

Worst errors on an MI355X over every weight vector, chunk count and the dN_dydeta nodes, 3+1D / 2+1D (also DESIGN.md, section 2, "Extreme cells"):
    delta-f               4.4e-11 (isothermal-mix, df_mode 2, raw) / 1.6e-10 (large-stress, df_mode 2, raw)
    include_baryon = 1    2.5e-12 / 9.0e-13
    modified equilibrium  8.7e-10 (large-stress, df_mode 4: the cells with det A ~ 1e-3, where the double restatement of
                          tests/dndx_feqmod_ref.py is 9.3e-10 from long double itself; the next case is 2.4e-10) / 9.7e-11 (fast-flow, df_mode 3)
    anisotropic hydro     2.4e-11 (tau-extremes, regulate_deltaf = 0, from the tables) / 1.9e-11 (fast-flow, regulate_deltaf = 1, from the tables)
No case needed a conditioning factor.

One defect was found and fixed (cf_spacetime_feqmod.hip, cf_st_fq_cells).  In 2+1D, operation 0 puts a cell's rows at eta_scale eta_k with
eta_scale = det A and no upper bound (smooth_kernels.cpp:1847-1849; the spectra routine scales only for det A < 1).  The exponent-range bound of
cf_prep_feqmod takes cosh(max |eta_k|) and so does not cover det A > 1: on fq_large-stress_2_mode4 (det A to 95: E_mod / T_mod ~ 1e124 on the
outer rows) and fq_isothermal-mix_2_mode3 the argument of exp_p9 left its |v| < 1.4e9 domain.  With the row cull on, those rows are dropped
before the exponential (the values were right); with zero_skip = 2 dN_dy and the histograms came out NaN, which the zero_skip 0 / 2 comparison
of this file showed.  The kernel now holds the argument at 1e9 in 2+1D, where e^-X is the same +0; every other bit is as before.

Sensitivity, once, on a scratch build: with bmax of cf_st_cells formed from 7 of a tile's 8 phi (a bound that misses a term), all 8 fast-flow
and all 8 isothermal-mix cases of test_deltaf fail, 36 cells each -- E2_j = exp(pT D'_j - bmax) overflows at gamma = 20: dN_dy_cell is not
finite already under the all-ones weight in 12 of them, and in the four 3+1D isothermal-mix cases it is finite and wrong by 100 % under
e_5 alone, the 40 GeV node that the all-ones sum hides -- while tests/test_gpu_spacetime.py, tests/test_gpu_spacetime_multi.py, tests/test_gpu_hostile_surfaces.py and
tests/test_gpu_offtile.py pass (364 tests): none of the older files notices."""
from functools import lru_cache

import numpy as np
import pytest

import extreme_cells as X
import extreme_cells_op0 as O
from is3d_amd import api, inputs
from test_gpu_spacetime import binned, bins_of

pytestmark = pytest.mark.gpu

TOL = 2e-9            # tests/test_gpu_extreme_cells.py
HISTS = ("dN_taudtaudy", "dN_twopirdrdy", "dN_twopitaurdtaudrdy")


def cases(family):
    cs = X.fixture_op0_cases(family)
    return pytest.mark.parametrize("case", cs, ids=[c["key"] for c in cs])


def cells_of(case):
    """the committed cells with the transverse positions of the table (no case moves them)"""
    tag = case["cells"]
    src = X.surface(case["case"], case["dim"], vah=tag.endswith("v"), baryon=tag.endswith("b"))
    return dict(X.fixture_cells(tag), x=src["x"], y=src["y"])


@lru_cache(maxsize=None)
def vah_tables():
    return inputs.vah_df_tables()


def grid_of(case, name):
    """X.op0_grid; the 2+1D modified-equilibrium cases with three zero-weight pT nodes behind the six (the kernel refuses 6 pT x 241 eta)"""
    return X.op0_grid(name, padded=case["family"] == "fq" and case["dim"] == 2)


def runner(case, cells, **kw):
    """run(name, **opts) -> the library result under the pT weight vector `name`"""
    bins, o = X.op0_bins(cells), case["opts"]
    if case["family"] == "vah":
        return lambda name, **extra: api.spacetime_distributions_vah(cells, X.species(), grid_of(case, name), bins, dict(o, **extra), per_cell=True, **kw)
    df = O.df_tables(case["family"] == "dfb")
    fq = O.fq_for(X.fixture_cells(case["cells"])) if case["family"] == "fq" else None
    return lambda name, **extra: api.spacetime_distributions(cells, X.species(), grid_of(case, name), df, bins, dict(o, **extra), per_cell=True, fq=fq)


def check_counts(res, case):
    st = res["stats"]
    assert st["n_cells_skipped"] == case["n_skipped"] and st["bad_cell"] == -1, st
    if case["family"] == "fq":
        fs = res["feqmod_stats"]
        assert (fs["n_cells_breakdown"], fs["n_renorm_skipped"]) == (case["n_breakdown"], case["n_renorm_skipped"]), fs


def check_sums(res, cells, bins):
    """the histograms and dN_dy are the left-to-right sums of the device's own dN_dy_cell"""
    pc = res["dN_dy_cell"]
    for name, want in zip(HISTS, binned(pc, cells, bins)):
        assert np.array_equal(res[name], want), name
    assert np.array_equal(res["dN_dy"], np.cumsum(pc, axis=1)[:, -1])


def same_bits(a, b, what, but=()):
    for k in api.SPACETIME_OUTPUTS:
        if k not in but:
            assert np.array_equal(a[k], b[k]), (what, k)


def on_the_extreme_cells(case, run, cells, what=""):
    """every weight vector, cell_chunks 1 and 3 -> worst error of dN_dy_cell (and of the 2+1D dN_dydeta)"""
    bins = X.op0_bins(cells)
    it, _ = bins_of(cells, bins)
    assert (it < 0).any() and (it >= bins["tau_bins"]).any()
    worst = 0.0
    for name in X.PT_W_NAMES:
        for nch in (1, 3):
            res = run(name, cell_chunks=nch)
            check_counts(res, case)
            err = O.held(res["dN_dy_cell"], case, name)
            print("%s %s %s cell_chunks %d: worst error against long double %.3e" % (case["key"], what, name, nch, err))
            assert err < TOL, (case["key"], what, name, nch, err)
            check_sums(res, cells, bins)
            worst = max(worst, err)
            if case["dim"] == 3:
                assert np.array_equal(res["dN_dydeta"][:, 0], res["dN_dy"])
            elif name == "ones":
                err = O.held_eta(res["dN_dydeta"], case)
                print("%s %s dN_dydeta: worst error against long double %.3e" % (case["key"], what, err))
                assert np.isfinite(res["dN_dydeta"]).all() and err < TOL, (case["key"], what, "dN_dydeta", err)
                worst = max(worst, err)
        if name in ("ones", "e5"):
            same_bits(run(name, zero_skip=2), run(name, zero_skip=0), (case["key"], what, name, "zero_skip"))
    return worst


def three_shards(case, cells):
    bins, o = X.op0_bins(cells), case["opts"]
    fq = O.fq_for(X.fixture_cells(case["cells"])) if case["family"] == "fq" else None
    args = (cells, X.species(), grid_of(case, "ones"), O.df_tables(case["family"] == "dfb"), bins, o)
    single = api.spacetime_distributions(*args, per_cell=True, fq=fq)
    multi = api.spacetime_distributions_multi(*args, devices=[0] * 3, per_cell=True, fq=fq)
    assert len(multi["shard_stats"]) == 3
    same_bits(multi, single, (case["key"], "three shards"), but=("dN_dydeta",) if case["dim"] == 2 else ())
    if case["dim"] == 2:
        err = O.held_eta(multi["dN_dydeta"], case)
        assert err < TOL, (case["key"], "three shards, dN_dydeta", err)


@cases("df")
def test_deltaf(case):
    cells = cells_of(case)
    worst = on_the_extreme_cells(case, runner(case, cells), cells)
    three_shards(case, cells)
    print("%s: worst error against long double %.3e" % (case["key"], worst))


@cases("dfb")
def test_deltaf_with_baryon(case):
    cells = cells_of(case)
    worst = on_the_extreme_cells(case, runner(case, cells), cells)
    three_shards(case, cells)
    print("%s: worst error against long double %.3e" % (case["key"], worst))


@cases("fq")
def test_modified_equilibrium(case):
    cells = cells_of(case)
    worst = on_the_extreme_cells(case, runner(case, cells), cells)
    three_shards(case, cells)
    print("%s: worst error against long double %.3e (breakdown %d)" % (case["key"], worst, case["n_breakdown"]))


@cases("vah")
def test_anisotropic_hydro(case):
    """with the cells' own coefficients (scipy's, as committed) and with the coefficients the device interpolates from the tables"""
    cells = cells_of(case)
    worst = {}
    for what, kw in (("cells", {}), ("tables", dict(tab=vah_tables()))):
        worst[what] = on_the_extreme_cells(case, runner(case, cells, **kw), cells, what)
    print("%s: worst error against long double %.3e with the cells' coefficients, %.3e from the tables" % (case["key"], worst["cells"], worst["tables"]))
