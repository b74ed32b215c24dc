"""GPU (-m gpu): cf_main_tile3e with the header's D'_j and gamma_j in SGPRs and ONE shared reciprocal per row of 8 phi values (SH8,
cf_kernels.hip) on the grids, cell counts and species lists where the tile can go wrong.  The form is the default 3+1D kernel (variant 6); the
developer build keeps the round-5 form as `kernel_variant = 13`; the one test that compares the two exists there only (marked `devlib`:
tests/test_gpu_devlib.py runs it in its child process on that build).

Tolerances: every case against the oracle at the 2e-9 of tests/test_gpu_parity.py's 3+1D cases; culling on against off bitwise.  The urqmd
list on 1 300 cells costs the CPU oracle 3.6e8 (20 x 9 x 5), 7.1e8 (8 x 7 x 32) and 6.4e9 (24 x 21 x 32) evaluations; on the last grid the
oracle therefore sees a fixed sample of 12 of the 305 species (every 32nd of the list plus the lightest and the heaviest: 2.5e8 evaluations;
species are independent in the oracle, and the species index is the fastest of the flat spectrum), and all 305 are held besides to the E2-less 8 x 7 tile (kernel_variant = 3)
at the 5e-11 tests/test_gpu_parity.py::test_row_culling_changes_no_bit uses between the two kernels."""
import numpy as np
import pytest

from conftest import relerr
from is3d_amd import api, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 2e-9           # tests/test_gpu_parity.py, 3+1D
TOL_KERNELS = 5e-11  # variant 6 against variant 3 there: the rounding of the exponent's argument
VARIANT = 0

# (J, K, n_pT): aligned; a partial phi tile, a partial row block and padded lanes; a single tile
GRIDS = {"aligned": (24, 21, 32), "partial": (20, 9, 5), "single": (8, 7, 32)}


def make_grid(fx, J, K, n_pT):
    rng = np.random.default_rng(1000 * J + 10 * K + n_pT)
    return dict(pT=np.linspace(0.05, 3.2, n_pT), phi=np.sort(rng.random(J) * 2 * np.pi), y=np.linspace(-2.5, 2.5, K), eta=fx["grid"]["eta"],
                eta_w=fx["grid"]["eta_w"])


def run(cells, sp, grid, df, df_mode, **extra):
    got, st = api.smooth_spectra(cells, sp, grid, df, dict(dimension=3, df_mode=df_mode, kernel_variant=VARIANT, **extra))
    assert st["kernel_variant"] == (VARIANT or 6)
    return got, st


@pytest.mark.parametrize("df_mode", [2, 1])
@pytest.mark.parametrize("n", [7, 1300])
@pytest.mark.parametrize("shape", sorted(GRIDS))
def test_rcp8_pikp_against_the_oracle(fx, shape, n, df_mode):
    grid = make_grid(fx, *GRIDS[shape])
    cells = synth.synth_surface(n, 3, seed=1300 + n)
    on, st_on = run(cells, fx["pikp"], grid, fx["df"], df_mode)
    off, st_off = run(cells, fx["pikp"], grid, fx["df"], df_mode, zero_skip=2)
    assert np.isfinite(on).all()
    assert np.array_equal(on, off) and st_off["n_wave_rows_culled"] == 0
    ref = oracle.dN_pTdpTdphidy(cells, fx["pikp"], grid, fx["df"], dict(dimension=3, df_mode=df_mode))
    err = relerr(on, ref)
    print("pikp %s n=%d df_mode=%d: max rel err vs oracle %.3e" % (shape, n, df_mode, err))
    assert err < TOL


@pytest.mark.parametrize("df_mode", [2, 1])
@pytest.mark.parametrize("n", [7, 1300])
@pytest.mark.parametrize("shape", sorted(GRIDS))
def test_rcp8_urqmd_list(fx, shape, n, df_mode):
    grid = make_grid(fx, *GRIDS[shape])
    cells = synth.synth_surface(n, 3, seed=1300 + n)
    on, st_on = run(cells, fx["urqmd"], grid, fx["df"], df_mode)
    off, _ = run(cells, fx["urqmd"], grid, fx["df"], df_mode, zero_skip=2)
    assert st_on["n_classes"] == 75
    assert np.isfinite(on).all() and np.array_equal(on, off)
    o = dict(dimension=3, df_mode=df_mode)
    if n == 1300 and shape == "aligned":
        # the oracle on a sample of the species (docstring), every species against the E2-less tile
        sp = fx["urqmd"]
        ns = len(sp["mass"])
        order = np.argsort(sp["mass"], kind="stable")
        pick = np.unique(np.concatenate([np.arange(0, ns, 32), order[:1], order[-1:]]))
        sub = {k: (np.asarray(v)[pick] if np.ndim(v) >= 1 and np.shape(v)[0] == ns else v) for k, v in sp.items()}
        ref = oracle.dN_pTdpTdphidy(cells, sub, grid, fx["df"], o)
        got = on.reshape(-1, ns)[:, pick].reshape(ref.shape)
        err = relerr(got, ref)
        v3, s3 = api.smooth_spectra(cells, sp, grid, fx["df"], dict(o, kernel_variant=3))
        e3 = relerr(on, v3)
        print("urqmd %s n=%d df_mode=%d: max rel err vs oracle on %d species %.3e, vs variant 3 on all %.3e" % (shape, n, df_mode, len(pick), err, e3))
        assert s3["kernel_variant"] == 3 and e3 < TOL_KERNELS
    else:
        err = relerr(on, oracle.dN_pTdpTdphidy(cells, fx["urqmd"], grid, fx["df"], o))
        print("urqmd %s n=%d df_mode=%d: max rel err vs oracle %.3e" % (shape, n, df_mode, err))
    assert err < TOL


@pytest.mark.parametrize("df_mode", [2, 1])
def test_rcp8_skipped_cells(fx, df_mode):
    """u.dsigma <= 0 cells, one of them outside the coefficient table with garbage beside it: counted, exactly zero, nothing leaks into the batch."""
    grid = make_grid(fx, *GRIDS["partial"])
    cells = synth.synth_surface(40, 3, seed=12)
    for k in ("dat", "dax", "day", "dan"):
        cells[k][[3, 17, 39]] *= -1.0
    cells["T"][17] = 0.05
    cells["eta"][39] = np.nan
    got, st = run(cells, fx["pikp"], grid, fx["df"], df_mode)
    assert st["n_cells_skipped"] == 3 and st["bad_cell"] == -1
    assert np.isfinite(got).all()
    assert relerr(got, oracle.dN_pTdpTdphidy(cells, fx["pikp"], grid, fx["df"], dict(dimension=3, df_mode=df_mode))) < TOL


@pytest.mark.devlib
@pytest.mark.skipif(not api.DEV_LIB, reason="kernel_variant 13 exists in the developer build only")
def test_rcp8_against_the_round5_form(fx):
    """Developer build: the largest relative difference between the default (SH8) and the round-5 form (variant 13) on the aligned grid x 1 300 cells --
    printed for LABBOOK.md, and held to the rounding class of the change (a different reciprocal grouping and FMA contraction: a few 1e-13)."""
    grid = make_grid(fx, *GRIDS["aligned"])
    cells = synth.synth_surface(1300, 3, seed=2600)
    for sp in ("pikp", "urqmd"):
        new, _ = run(cells, fx[sp], grid, fx["df"], 2)
        old, so = api.smooth_spectra(cells, fx[sp], grid, fx["df"], dict(dimension=3, df_mode=2, kernel_variant=13))
        assert so["kernel_variant"] == 13
        d = relerr(new, old)
        print("SH8 (variant 6) against the round-5 form (variant 13), %s, 1300 cells, 24 x 21 x 32: max rel diff %.3e" % (sp, d))
        assert d < TOL_KERNELS
