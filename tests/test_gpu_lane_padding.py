"""GPU (-m gpu): the slots that pad the lanes to whole waves are copies of the last real lane (is3d::lane_arrays, cf_plan_geometry.h) and so
never change a wave-wide cull vote.  Before, a padding slot was a boson of mT = 1, pT = 0 with pe = 0: alive in many more rows than the heavy
lanes it shares its wave with, it kept rows running that no real lane needs.

The smallest shape that shows it is one wave that is mostly padding: three species of 3 GeV and more on 5 pT x 8 phi x 7 y -- 15 real lanes, 49
padding slots, one 8 x 7 tile -- and cells at T = 0.10 GeV in two sets.  Set A sits |y - eta| = 4.05 .. 4.55 from every y of the grid: the tested
exponent pT Dmax - mT C'_k is below -760 for every real lane (exp == +0, the row is dead under the exact-zero rule) but above -600 for (mT, pT) =
(1, 0).  Set B sits within 0.7 of every y: live for everything.  The test states the exponents once more in numpy, asserts that none lies within 10
of the bound -- the expected count then hangs on no rounding -- and holds status.n_wave_rows_culled of a zero_skip = 1 run to the count of rows dead
for all REAL lanes of their wave.  With the old padding set A's rows stay alive and that count is 0.

The same count is held once each for cf_main_tile (33 pT: no E2 table stream), cf_main_feqmod (df_mode 4) and cf_main_vah3, each with its own bound
(E/T, E_a/Lambda > 745.25; inviscid cells, alpha_L = 1: the bounds are then closed forms of the flow), and a table of whole waves (4 species x 32 pT)
gives the counts and the bits it gave before.  Spectra: bitwise across zero_skip 0 / 1 / 2, and within the 2e-9 of the 3+1D parity tests of the oracle."""
import numpy as np
import pytest

from conftest import relerr
from is3d_amd import api, inputs, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 2e-9            # tests/test_gpu_parity.py, 3+1D
FLOOR = -745.2        # thr_floor of the delta-f kernels: exp(earg) == +0 below it
XCUT = 745.25         # cf_main_feqmod, cf_main_vah3: exp(-X) == +0 above it
MARGIN = 10.0
N_A, N_B = 12, 8
T0 = 0.10


def species(masses):
    n = len(masses)
    return dict(mc_id=np.arange(1, n + 1, dtype=np.int32) * 1000 + 1, mass=np.array(masses, dtype=np.float64), degeneracy=np.arange(1, n + 1, dtype=np.float64),
                baryon=np.array([float(i % 2) for i in range(n)]), sign=np.array([1.0 if i % 2 else -1.0 for i in range(n)]))


HEAVY3 = species([3.0, 3.5, 4.2])
HEAVY4 = species([3.0, 3.5, 4.2, 5.1])


def make_grid(fx, n_pT):
    rng = np.random.default_rng(26)
    return dict(pT=np.linspace(0.05, 2.0, n_pT), phi=np.sort(rng.random(8) * 2 * np.pi), y=np.linspace(-0.2, 0.2, 7), eta=fx["grid"]["eta"], eta_w=fx["grid"]["eta_w"])


def reshape_cells(c, inviscid):
    """cells of a seeded surface moved to T = 0.10 and to the two sets of eta, A and B interleaved; half the transverse flow"""
    n = len(c["tau"])
    assert n == N_A + N_B
    c = {k: np.array(v, dtype=np.float64, copy=True) for k, v in c.items()}
    rng = np.random.default_rng(2600)
    in_a = np.zeros(n, dtype=bool)
    in_a[rng.permutation(n)[:N_A]] = True
    side = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    c["eta"] = np.where(in_a, side * (4.3 + 0.05 * (2 * rng.random(n) - 1)), 0.5 * (2 * rng.random(n) - 1))
    c["un"] = 0.05 * np.tanh(c["eta"]) / c["tau"]
    c["ux"] *= 0.5
    c["uy"] *= 0.5
    scale = (T0 / c["T"]) ** 4          # P, E and with them the viscous terms follow T
    c["T"][:] = T0
    for f in c:
        if f in ("P", "E", "bulkPi") or f.startswith("pi") or f in ("Wx", "Wy"):
            c[f] = c[f] * (0.0 if inviscid and f not in ("P", "E") else scale)
    return c, in_a


@pytest.fixture(scope="module")
def surface():
    cells, in_a = reshape_cells(synth.synth_surface(N_A + N_B, 3, seed=2601), inviscid=False)
    return cells, in_a


def lane_waves(sp, pT):
    """(mT, pT) of the real lanes in the plan's order -- classes x pT sorted by mT, ties in natural order; every species here is a class -- and the wave of each"""
    mT = np.sqrt(sp["mass"][:, None] ** 2 + pT[None, :] ** 2).ravel()
    pTl = np.broadcast_to(pT[None, :], (len(sp["mass"]), len(pT))).ravel()
    order = np.argsort(mT, kind="stable")
    return mT[order], pTl[order], np.arange(len(order)) // 64


def flow_bounds(c, grid, scale):
    """C_k = (u^tau cosh(y_k - eta) - tau u^eta sinh(y_k - eta)) / scale [cell][k], D_j = (ux cos phi_j + uy sin phi_j) / scale [cell][j]: p.u / scale = mT C_k - pT D_j"""
    ut = np.sqrt(1.0 + c["ux"] ** 2 + c["uy"] ** 2 + c["tau"] ** 2 * c["un"] ** 2)
    dy = grid["y"][None, :] - c["eta"][:, None]
    C = (np.cosh(dy) * ut[:, None] - np.sinh(dy) * (c["tau"] * c["un"])[:, None]) / scale[:, None]
    D = (np.cos(grid["phi"])[None, :] * c["ux"][:, None] + np.sin(grid["phi"])[None, :] * c["uy"][:, None]) / scale[:, None]
    return C, D


def expected_culls(dead, wave):
    """dead [lane][cell][row] -> wave-rows dead for every real lane of their wave"""
    return int(sum(dead[wave == w].all(axis=0).sum() for w in np.unique(wave)))


def deltaf_expectation(c, in_a, sp, grid):
    """the exact-zero rule of cf_main_tile3e / cf_main_tile on an 8-phi tile: a row is dead for a lane when pT Dmax - mT C'_k < -745.2"""
    mT, pTl, wave = lane_waves(sp, grid["pT"])
    C, D = flow_bounds(c, grid, c["T"])
    earg = pTl[:, None, None] * D.max(axis=1)[None, :, None] - mT[:, None, None] * C[None, :, :]      # [lane][cell][row]
    assert np.all(np.abs(earg - FLOOR) > MARGIN)                                                      # the count hangs on no rounding
    assert np.all(earg[:, in_a, :] < -760.0) and np.all(earg[:, ~in_a, :] > FLOOR + MARGIN)           # set A dead, set B live, for every real lane
    assert np.all(-1.0 * C[in_a] > -600.0)                                                            # ... and set A alive for (mT, pT) = (1, 0)
    n_rows = (wave.max() + 1) * len(c["tau"]) * len(grid["y"])
    return expected_culls(earg < FLOOR, wave), n_rows, wave


def run(cells, sp, grid, df, **extra):
    return api.smooth_spectra(cells, sp, grid, df, dict(dimension=3, df_mode=2, **extra))


@pytest.fixture(scope="module")
def main_case(fx, surface):
    """the 15-lane wave under zero_skip 0 / 1 / 2, run once"""
    cells, in_a = surface
    grid = make_grid(fx, 5)
    want, n_rows, wave = deltaf_expectation(cells, in_a, HEAVY3, grid)
    assert wave.max() == 0 and len(wave) == 15 and want == N_A * 7
    runs = [run(cells, HEAVY3, grid, fx["df"], zero_skip=zs) for zs in (0, 1, 2)]
    for got, st in runs:
        assert st["kernel_variant"] == 6 and st["n_wave_rows"] == n_rows == 64 // 64 * (N_A + N_B) * 7
    print("15 lanes + 49 padding slots: culled %d / %d / %d of %d wave-rows (zero_skip 0 / 1 / 2), expected for zero_skip 1: %d" % (
        runs[0][1]["n_wave_rows_culled"], runs[1][1]["n_wave_rows_culled"], runs[2][1]["n_wave_rows_culled"], n_rows, want))
    return cells, grid, want, runs


def test_padding_casts_no_vote_of_its_own(main_case):
    """exact count: the rows dead for all real lanes -- on the table's own padding (1, 0, pe = 0) set A's rows stay alive and the count is 0"""
    _, _, want, runs = main_case
    assert runs[1][1]["n_wave_rows_culled"] == want
    assert runs[2][1]["n_wave_rows_culled"] == 0


def test_the_relative_rule_culls_no_less(main_case):
    _, _, _, runs = main_case
    assert runs[0][1]["n_wave_rows_culled"] >= runs[1][1]["n_wave_rows_culled"]


def test_culled_rows_change_no_bit(main_case):
    _, _, _, runs = main_case
    assert np.isfinite(runs[2][0]).all() and runs[2][0].max() > 0.0
    assert np.array_equal(runs[0][0], runs[2][0]) and np.array_equal(runs[1][0], runs[2][0])


def test_oracle_parity(fx, main_case):
    cells, grid, _, runs = main_case
    ref = oracle.dN_pTdpTdphidy(cells, HEAVY3, grid, fx["df"], dict(dimension=3, df_mode=2))
    err = relerr(runs[0][0], ref)
    print("max rel err vs oracle %.3e" % err)
    assert err < TOL


def test_tile_kernel_without_the_table_stream(fx, surface):
    """33 pT: cf_main_tile; 99 lanes, the second wave 35 of them and 29 padding slots"""
    cells, in_a = surface
    grid = make_grid(fx, 33)
    want, n_rows, wave = deltaf_expectation(cells, in_a, HEAVY3, grid)
    assert wave.max() == 1 and want == 2 * N_A * 7
    exact, st1 = run(cells, HEAVY3, grid, fx["df"], zero_skip=1)
    off, st2 = run(cells, HEAVY3, grid, fx["df"], zero_skip=2)
    assert st1["kernel_variant"] == 3 and st1["n_wave_rows"] == n_rows
    print("cf_main_tile, 99 lanes: culled %d of %d, expected %d" % (st1["n_wave_rows_culled"], n_rows, want))
    assert st1["n_wave_rows_culled"] == want and st2["n_wave_rows_culled"] == 0
    assert np.array_equal(exact, off)


def x_expectation(c, in_a, sp, grid, scale, feqmod):
    """the exact-zero rule of cf_main_feqmod / cf_main_vah3 on inviscid cells (alpha_L = 1), where E / T (E_a / Lambda) is p.u / scale: a row is dead for a
    lane when the kernel's lower bound of it over the phi tile exceeds 745.25.  cf_main_vah3: X >= max(mT C_k - pT Dmax, 0).  cf_main_feqmod bounds
    X^2 = mT^2 C_k^2 - 2 mT pT C_k D_j + pT^2 D_j^2 term by term: min_j of the mixed term and min_j of the last."""
    mT, pTl, wave = lane_waves(sp, grid["pT"])
    C, D = flow_bounds(c, grid, scale)
    m, p = mT[:, None, None], pTl[:, None, None]
    if feqmod:
        x2 = m * m * (C * C)[None] - 2.0 * m * p * (C * D.max(axis=1)[:, None])[None] + p * p * (D * D).min(axis=1)[None, :, None]
        X = np.sqrt(np.maximum(x2, 0.0))
    else:
        X = np.maximum(m * C[None] - p * D.max(axis=1)[None, :, None], 0.0)
    assert np.all(np.abs(X - XCUT) > MARGIN)
    assert np.all(X[:, in_a, :] > XCUT + MARGIN) and np.all(X[:, ~in_a, :] < XCUT - MARGIN)
    assert np.all(C[in_a] < XCUT - MARGIN)                                                            # (mT, pT) = (1, 0): X = C_k, alive on set A
    return expected_culls(X > XCUT, wave), (wave.max() + 1) * len(c["tau"]) * len(grid["y"])


def test_feqmod_kernel(fx):
    """cf_main_feqmod (df_mode 4) on the same wave of 15 lanes"""
    cells, in_a = reshape_cells(synth.synth_surface(N_A + N_B, 3, seed=2601), inviscid=True)
    grid = make_grid(fx, 5)
    want, n_rows = x_expectation(cells, in_a, HEAVY3, grid, cells["T"], feqmod=True)
    assert want == N_A * 7
    fq = inputs.feqmod_tables(inputs.surface_average_T(cells))
    res = [api.smooth_spectra(cells, HEAVY3, grid, fx["df"], dict(dimension=3, df_mode=4, zero_skip=zs), fq=fq) for zs in (1, 2)]
    (exact, st1), (off, st2) = res
    print("cf_main_feqmod: culled %d of %d, expected %d (breakdown cells %d)" % (st1["n_wave_rows_culled"], st1["n_wave_rows"], want, st1["n_cells_breakdown"]))
    assert st1["n_cells_breakdown"] == 0 and st1["n_cells_narrow"] == 0
    assert st1["n_wave_rows"] == n_rows and st1["n_wave_rows_culled"] == want and st2["n_wave_rows_culled"] == 0
    assert np.array_equal(exact, off) and off.max() > 0.0


def test_vah_kernel(fx):
    """cf_main_vah3 on the same wave of 15 lanes: Lambda = 0.10, alpha_L = 1 (xi_L = 0: E_a = p.u), pi_perp = W = bulk = 0"""
    cells, in_a = reshape_cells(synth.synth_vah_surface(N_A + N_B, 3, seed=2601), inviscid=True)
    cells["Lambda"] = np.full(N_A + N_B, T0)
    cells["aL"] = np.ones(N_A + N_B)
    grid = make_grid(fx, 5)
    want, n_rows = x_expectation(cells, in_a, HEAVY3, grid, cells["Lambda"], feqmod=False)
    assert want == N_A * 7
    (exact, st1), (off, st2) = [api.smooth_spectra_vah(cells, HEAVY3, grid, dict(dimension=3, zero_skip=zs)) for zs in (1, 2)]
    print("cf_main_vah3: culled %d of %d, expected %d" % (st1["n_wave_rows_culled"], st1["n_wave_rows"], want))
    assert st1["kernel_variant"] == 3
    assert st1["n_wave_rows"] == n_rows and st1["n_wave_rows_culled"] == want and st2["n_wave_rows_culled"] == 0
    assert np.array_equal(exact, off) and off.max() > 0.0


def test_whole_wave_table(fx, surface):
    """4 species x 32 pT = two whole waves: nothing is padded, the counts and the bits are what they were"""
    cells, in_a = surface
    grid = make_grid(fx, 32)
    want, n_rows, wave = deltaf_expectation(cells, in_a, HEAVY4, grid)
    assert len(wave) == 128 and want == 2 * N_A * 7
    on, st0 = run(cells, HEAVY4, grid, fx["df"])
    exact, st1 = run(cells, HEAVY4, grid, fx["df"], zero_skip=1)
    off, st2 = run(cells, HEAVY4, grid, fx["df"], zero_skip=2)
    assert st1["kernel_variant"] == 6 and st0["n_wave_rows"] == st1["n_wave_rows"] == st2["n_wave_rows"] == n_rows
    assert st0["n_wave_rows_culled"] >= st1["n_wave_rows_culled"] == want and st2["n_wave_rows_culled"] == 0
    assert np.array_equal(on, off) and np.array_equal(exact, off) and off.max() > 0.0
