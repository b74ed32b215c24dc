"""GPU (-m gpu): the accumulator-relative row cull with the UNIT'S OWN bound on the scaled p.dsigma in the exponent it tests (lambda_u, header
slot 11 of a 3+1D unit record without baryon slots: cf_prep, cull_refresh and kPdsBoundCull in cf_kernels.hip) -- variant 6
(the default 3+1D kernel), variant 3 and, in the developer build, variants 5, 10 and 12.

What can go wrong that could not before:
  * lambda_u from the wrong rows or phi of the record (an index slip in cf_prep's maxima, a padded row or phi read as a real one): a row whose terms
    still count is culled, and the spectrum with culling on differs from the one with culling off -- the assertion of every case here, bit for bit;
  * lambda_u reaching the exponent of the row EXPONENTIAL instead of only the tested one: every live row changes (same assertion, and the oracle);
  * the exact-zero floor taken relative: exp(earg) is +0 only below -745.2 whatever p.dsigma is, so lambda_u must not meet a threshold that is
    still the floor (a lane adds it only once all its group thresholds are relative bounds).  test_the_floor_is_held_against_earg_itself builds
    cells whose thresholds are still floors, whose lambda_u sits at the clamp, and which hold rows with a denormal, nonzero E1;
  * lambda_u entering an exact-only run (zero_skip = 1, no outflow clamp): their culled counts must stay those of the exact-zero rule;
  * exact zeros lost: the default must cull at least the rows the exact-zero rule culls, on every case.

Grids (phi x y x pT): 8 x 7 x 4 is one whole tile; 5 x 9 x 3 has a partial phi tile (three padded phi that repeat phi 4), a second row block of two
real rows and five padded ones, and 3 pT values: 9 lanes (pi/K/p) in a wave of 64, 915 (urqmd) in 15 waves, the last partly padded; 24 x 21 x 32
is the shipped grid.  Cells: 1, 6, 7 -- one 6-unit LDS batch and one cell more, i.e. just before / behind the first threshold refresh -- 64 and
1 300 (eight refreshes as one chunk); cell_chunks 1 and 3.

Tolerance against the oracle: the 2e-9 of tests/test_gpu_parity.py's 3+1D cases (TOL there and in tests/test_gpu_rowgroup_cull.py).  Everything
else is bitwise or a count."""
import numpy as np
import pytest

import hostile_surfaces as hs
import test_gpu_rowgroup_cull as rg
from conftest import relerr
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu

TOL = rg.TOL
LAMBDA_MAX = 40 * np.log(2.0)    # kPdsLambdaMax, cf_device.h
DS = hs.DS

GRIDS = {"8x7x4": (8, 7, 4), "5x9x3": (5, 9, 3), "24x21x32": None}


def make_grid(fx, shape):
    if GRIDS[shape] is None:
        return fx["grid"]
    J, K, n_pT = GRIDS[shape]
    rng = np.random.default_rng(1000 * J + 10 * K + n_pT)
    return dict(pT=np.linspace(0.05, 3.2, n_pT), phi=np.sort(rng.random(J) * 2 * np.pi), y=np.linspace(-4.5, 5.0, K), eta=fx["grid"]["eta"],
                eta_w=fx["grid"]["eta_w"])


def variants():
    return (0, 3) + ((5, 10, 12) if api.DEV_LIB else ())


def run(cells, sp, grid, df, df_mode, variant=0, **extra):
    got, st = api.smooth_spectra(cells, sp, grid, df, dict(dimension=3, df_mode=df_mode, kernel_variant=variant, **extra))
    assert st["kernel_variant"] == (variant or 6)
    return got, st


def three_modes(cells, sp, grid, df, df_mode, variant, **extra):
    """zero_skip 0 / 1 / 2: the same bits, the same wave-rows counted; returns the default's spectrum and the three status records"""
    on, s0 = run(cells, sp, grid, df, df_mode, variant, **extra)
    exact, s1 = run(cells, sp, grid, df, df_mode, variant, zero_skip=1, **extra)
    off, s2 = run(cells, sp, grid, df, df_mode, variant, zero_skip=2, **extra)
    assert np.isfinite(off).all(), (variant, extra)
    assert np.array_equal(on, off) and np.array_equal(exact, off), (variant, extra)
    assert s0["n_wave_rows"] == s1["n_wave_rows"] == s2["n_wave_rows"] > 0 == s2["n_wave_rows_culled"], (variant, extra)
    assert s0["n_wave_rows_culled"] >= s1["n_wave_rows_culled"], (variant, extra)   # no exact zero is lost to the unit bound
    return on, (s0, s1, s2)


def scaled(cells, s):
    """every dsigma component of cell c times 2^-s[c]"""
    c = {k: np.array(v, dtype=np.float64, copy=True) for k, v in cells.items()}
    for f in DS:
        c[f] = np.ldexp(c[f], -np.asarray(s, dtype=np.int64))
    return c


# the developer build (tests/test_gpu_devlib.py re-runs the cases marked devlib there) sees the two cell counts on either side of a refresh schedule
CELLS = [1, 6, pytest.param(7, marks=pytest.mark.devlib), 64, pytest.param(1300, marks=pytest.mark.devlib)]


# (the shipped grid runs with pi/K/p here; urqmd on it is tests/test_gpu_rowgroup_cull.py's and the counts test's below)
@pytest.mark.parametrize("df_mode", [2, 1])
@pytest.mark.parametrize("n", CELLS)
@pytest.mark.parametrize("shape,species", [("8x7x4", "pikp"), ("8x7x4", "urqmd"), ("5x9x3", "pikp"), ("5x9x3", "urqmd"), ("24x21x32", "pikp")])
def test_the_unit_bound_changes_no_bit(fx, shape, n, species, df_mode):
    grid, sp, df = make_grid(fx, shape), fx[species], fx["df"]
    cells = synth.synth_surface(n, 3, seed=4100 + n)
    first = None
    for variant in variants():
        for nch in (1, 3):
            on, (s0, s1, _) = three_modes(cells, sp, grid, df, df_mode, variant, cell_chunks=nch)
            assert s0["n_wave_rows_culled"] >= s1["n_wave_rows_culled"], (variant, nch)
            if first is None:
                first = on
                print("%s n=%d %s df_mode=%d: culled %d of %d wave-rows (exact zeros alone %d)" % (
                    shape, n, species, df_mode, s0["n_wave_rows_culled"], s0["n_wave_rows"], s1["n_wave_rows_culled"]))
            else:   # another kernel or another partition of the cells: to rounding (tests/test_gpu_rowgroup_cull.py: 5e-11 and 1e-12)
                assert relerr(on, first) < rg.TOL_KERNELS, (variant, nch)
    if species == "pikp":
        err = rg.oracle_error(first, cells, sp, grid, df, df_mode)
        print("  max rel err vs oracle %.3e" % err)
        assert err < TOL


def rule_surface(kind, n, seed):
    """synth_surface cells with all four dsigma components times 2^-s per cell.  'mixed': s drawn from {0, 10, 30, 60} (60 is past kPdsLambdaMax =
    40 ln 2: the clamp); 'one-sets-the-scale': one cell (the middle one) at s = 0, every other cell at s = 45"""
    cells = synth.synth_surface(n, 3, seed=seed)
    if kind == "mixed":
        s = np.random.default_rng(seed).choice([0, 10, 30, 60], n)
        s[0] = 0          # at least one of each, wherever the draw fell
        s[-1] = 60
    else:
        s = np.full(n, 45)
        s[n // 2] = 0
    return scaled(cells, s)


@pytest.mark.devlib
@pytest.mark.parametrize("df_mode", [2, 1])
@pytest.mark.parametrize("kind", ["mixed", "one-sets-the-scale"])
@pytest.mark.parametrize("shape,species,n", [("24x21x32", "pikp", 97), ("5x9x3", "urqmd", 97), ("8x7x4", "pikp", 1300)])
def test_surfaces_made_for_the_rule(fx, shape, species, n, kind, df_mode):
    grid, sp, df = make_grid(fx, shape), fx[species], fx["df"]
    cells = rule_surface(kind, n, 4300 + n)
    first = None
    for variant in variants():
        for nch in (1, 3):
            on, (s0, s1, _) = three_modes(cells, sp, grid, df, df_mode, variant, cell_chunks=nch)
            assert s0["n_wave_rows_culled"] >= s1["n_wave_rows_culled"], (variant, nch)
            if first is None:
                first = on
                print("%s %s n=%d %s df_mode=%d: culled %d of %d wave-rows (exact zeros alone %d)" % (
                    kind, shape, n, species, df_mode, s0["n_wave_rows_culled"], s0["n_wave_rows"], s1["n_wave_rows_culled"]))
            else:
                assert relerr(on, first) < rg.TOL_KERNELS, (variant, nch)
    if species == "pikp":
        err = rg.oracle_error(first, cells, sp, grid, df, df_mode)
        print("  max rel err vs oracle %.3e" % err)
        assert err < TOL


def floor_cells(n_far):
    """n_far cells at eta = -4 with dsigma times 2^-60, then ONE cell left as it is: it sets the surface's scale (so the others' lambda_u is at the
    clamp) and runs last -- the n_far <= 6 cells in front of it fill at most the first LDS batch, before any threshold has left its floor"""
    cells = synth.synth_surface(n_far + 1, 3, seed=4500 + n_far)
    s = np.full(n_far + 1, 60)
    s[-1] = 0
    c = scaled(cells, s)
    c["eta"][:n_far] = -4.0
    return c


def floor_case_numbers(cells, sp, grid, n_far):
    """numpy: lambda_u of the far cells' units (before the clamp) and the tested exponents earg = pT Dmax - mT C'_k of their (lane, tile, row)"""
    pT, phi, yv = grid["pT"], grid["phi"], grid["y"]
    mass = np.unique(np.asarray(sp["mass"], dtype=np.float64))
    mT = np.sqrt(mass[:, None] ** 2 + pT[None, :] ** 2).ravel()
    pTl = np.broadcast_to(pT[None, :], (len(mass), len(pT))).ravel()
    mTmax, pTmax = mT.max(), pT.max()
    tau, eta, T = cells["tau"], cells["eta"], cells["T"]
    ut = np.sqrt(1 + cells["ux"] ** 2 + cells["uy"] ** 2 + tau ** 2 * cells["un"] ** 2)
    dy = yv[None, :] - eta[:, None]
    ch, sh = np.cosh(dy), np.sinh(dy)
    Cp = (ch * ut[:, None] - sh * (tau * cells["un"])[:, None]) / T[:, None]                                   # [c][k]
    Ak = ch * cells["dat"][:, None] + sh * (cells["dan"] / tau)[:, None]
    Dp = (np.cos(phi)[None, :] * cells["ux"][:, None] + np.sin(phi)[None, :] * cells["uy"][:, None]) / T[:, None]   # [c][j]
    Bj = np.cos(phi)[None, :] * cells["dax"][:, None] + np.sin(phi)[None, :] * cells["day"][:, None]
    gmax = np.cosh(np.maximum(np.abs(yv.min() - eta), np.abs(yv.max() - eta)))
    bound = ((mTmax * (np.abs(cells["dat"]) + np.abs(cells["dan"] / tau)) + pTmax * (np.abs(cells["dax"]) + np.abs(cells["day"]))) * gmax).max()
    psc = 2.0 ** -int(np.frexp(bound)[1])
    # the largest lambda any unit of a far cell can have: all rows, all phi
    lam_far = np.log((mTmax * np.abs(Ak[:n_far]).max(axis=1) + pTmax * np.abs(Bj[:n_far]).max(axis=1)) * psc)
    JT = 8
    earg = []
    for j0 in range(0, len(phi), JT):
        Dmax = Dp[:n_far, j0:j0 + JT].max(axis=1)                                                               # [c]
        earg.append(pTl[:, None, None] * Dmax[None, :, None] - mT[:, None, None] * Cp[None, :n_far, :])       # [l][c][k]
    return lam_far, np.stack(earg)


@pytest.mark.devlib
@pytest.mark.parametrize("n_far", [1, 2, 3, 4, 5, 6])
def test_the_floor_is_held_against_earg_itself(fx, n_far):
    grid, sp, df = fx["grid"], fx["pikp"], fx["df"]
    cells = floor_cells(n_far)
    lam_far, earg = floor_case_numbers(cells, sp, grid, n_far)
    assert (lam_far < -LAMBDA_MAX - 1.0).all()                         # lambda_u = -kPdsLambdaMax in every unit of the far cells
    # E1 = exp(earg) is a nonzero denormal for earg in [-745.13, -708.4]; such a (lane, row) sits above the exact-zero floor -745.2 and, with
    # lambda_u = -kPdsLambdaMax added, below it: lambda_u must stay out of a test against the floor.  (Rows below -745.2 - kPdsLambdaMax exist too.)
    trap = (earg >= -745.0) & (earg <= -708.5)
    assert trap.any() and (earg < -745.2 - LAMBDA_MAX).any()
    print("n_far=%d: %d (lane, tile, row) with a denormal E1, lambda of the far cells <= %.1f" % (n_far, int(trap.sum()), lam_far.max()))
    for df_mode in (2, 1):
        for variant in variants():
            _, (s0, s1, _) = three_modes(cells, sp, grid, df, df_mode, variant, cell_chunks=1)
            assert s0["n_wave_rows_culled"] >= s1["n_wave_rows_culled"], (df_mode, variant)
            a, sa = run(cells, sp, grid, df, df_mode, variant, outflow=0, cell_chunks=1)
            b, sb = run(cells, sp, grid, df, df_mode, variant, outflow=0, zero_skip=2, cell_chunks=1)
            assert np.array_equal(a, b) and sb["n_wave_rows_culled"] == 0, (df_mode, variant)
            assert s1["n_wave_rows_culled"] == sa["n_wave_rows_culled"], (df_mode, variant)


@pytest.mark.parametrize("which", ["shipped", "offtile"])
@pytest.mark.parametrize("case", hs.CASES)
def test_the_unit_bound_on_hostile_surfaces(fx, case, which):
    grid, sp = hs.plain(hs.grid(which)), hs.species()
    cells = hs.surface(case, 3)
    for df_mode in (2, 1):
        for variant in (0, 3):
            for nch in (1, 3):
                three_modes(cells, sp, grid, fx["df"], df_mode, variant, cell_chunks=nch)


@pytest.mark.parametrize("variant", [0, 3])
def test_a_uniform_power_of_two_is_exact_with_the_unit_bound(fx, variant):
    """dsigma -> 2^k dsigma: lambda_u is formed from the SCALED A_k, B_j, so it is the same at every k and the same rows are dropped"""
    grid, sp, df = hs.exact_grid(3), hs.species(), fx["df"]
    cells = hs.exact_base(3)
    base, st = run(cells, sp, grid, df, 2, variant)
    assert np.isfinite(base).all() and np.abs(base[base != 0]).min() > 1e-150
    for k in hs.UNIFORM_K:
        got, sk = run(hs.uniform(cells, k), sp, grid, df, 2, variant)
        assert np.array_equal(got, np.ldexp(base, k)), k
        assert sk["n_wave_rows_culled"] == st["n_wave_rows_culled"] and sk["n_wave_rows"] == st["n_wave_rows"], k


@pytest.mark.devlib
def test_unit_bound_counts_across_variants(fx):
    """the surface tests/test_gpu_parity.py::test_row_culling_changes_no_bit pins its cross-variant counts on (2 000 cells, seed 80, urqmd, three
    chunks): variants 6 and 3 within its 3 %, variant 5 (developer build) within its 2 % of either; with the surface-relative floors (zero_skip = 3)
    at least the default's rows go"""
    cells = synth.synth_surface(2000, 3, seed=80)
    sp, grid, df = fx["urqmd"], fx["grid"], fx["df"]
    o = dict(cell_chunks=3)
    on, s6 = run(cells, sp, grid, df, 2, **o)
    v3, s3 = run(cells, sp, grid, df, 2, 3, **o)
    off, sf = run(cells, sp, grid, df, 2, zero_skip=2, **o)
    _, s6e = run(cells, sp, grid, df, 2, zero_skip=1, **o)
    print("2000 cells, seed 80, urqmd, 3 chunks: wave-rows %d, culled variant 6 %d (%.4f), variant 3 %d, exact zeros alone %d" % (
        s6["n_wave_rows"], s6["n_wave_rows_culled"], s6["n_wave_rows_culled"] / s6["n_wave_rows"], s3["n_wave_rows_culled"], s6e["n_wave_rows_culled"]))
    assert np.array_equal(on, off) and relerr(on, v3) < rg.TOL_KERNELS
    assert s6["n_wave_rows"] == s3["n_wave_rows"] == sf["n_wave_rows"] and sf["n_wave_rows_culled"] == 0
    assert s6["n_wave_rows_culled"] > s6e["n_wave_rows_culled"] > 0
    assert abs(s6["n_wave_rows_culled"] - s3["n_wave_rows_culled"]) <= 3e-2 * s3["n_wave_rows_culled"]
    # zero_skip = 3 needs enough chunks for its first eighth (cf_plan.cpp); the default partition gives them
    _, d0 = run(cells, sp, grid, df, 2)
    surf, d3 = run(cells, sp, grid, df, 2, zero_skip=3)
    print("default partition: culled %d, with surface-relative floors %d of %d" % (d0["n_wave_rows_culled"], d3["n_wave_rows_culled"], d0["n_wave_rows"]))
    assert d3["n_wave_rows"] == d0["n_wave_rows"] and d3["n_wave_rows_culled"] >= d0["n_wave_rows_culled"]
    assert np.isfinite(surf).all()
    if api.DEV_LIB:
        v5, s5 = run(cells, sp, grid, df, 2, 5, **o)
        v5f, _ = run(cells, sp, grid, df, 2, 5, zero_skip=2, **o)
        assert np.array_equal(v5, v5f) and relerr(on, v5) < rg.TOL_KERNELS
        assert abs(s6["n_wave_rows_culled"] - s5["n_wave_rows_culled"]) <= 2e-2 * s5["n_wave_rows_culled"]
        assert abs(s5["n_wave_rows_culled"] - s3["n_wave_rows_culled"]) <= 2e-2 * s3["n_wave_rows_culled"]
