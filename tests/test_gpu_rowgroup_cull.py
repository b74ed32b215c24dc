"""GPU (-m gpu): the accumulator-relative row cull with one threshold per ROW GROUP ({0,1} {2,3,4} {5,6} of the 8 x 7 tile: cull_refresh,
cf_kernels.hip) in the kernels that share the rule: variant 6 (the default 3+1D kernel), variant 3 (the tile without the E2
stream) and, in the developer build, variants 5, 10 and 12; variant 13 there keeps one threshold per (lane, tile).

What can go wrong that could not before: a row is weighed against its own group's accumulators, so a group threshold taken from the wrong rows (an
index slip between the row of the test and the row of the minimum) culls rows that still count -- the spectrum with culling on then differs from the
one with culling off, which is the assertion of every case here, bit for bit.  The real rows of a PARTIAL row block now cull relative to their
accumulators too (a group that holds a padded row k >= K keeps the floor, the other groups do not): the grids put the edge of the grid at every
position inside a group -- K = 1, 2, 3, 5, 8, 9 -- next to an aligned one and a padded phi tile.  A unit that passes the unit bound (held against the
smallest group threshold) with an empty row mask leaves behind its row tests: the counts n_wave_rows / n_wave_rows_culled must not notice.

Cell counts: the thresholds are refreshed after the 6-unit batches 0, 1, 3, 7, ... of a chunk: 1 and 7 cells end before / just behind the first
refresh; as one chunk (cell_chunks = 1) 97 and 1 300 run through five and eight of them, cut into 64 chunks they never reach the second.

Tolerances: every case against the oracle at the 2e-9 of tests/test_gpu_parity.py's 3+1D cases, as tests/test_gpu_tile3e_rcp8.py; where the urqmd
list would cost the CPU oracle more than 1e8 evaluations it sees that file's fixed sample of 12 of the 305 species (species are independent in the
oracle).  Everything else is bitwise."""
import numpy as np
import pytest

import hostile_surfaces as hs
from conftest import relerr
from is3d_amd import api, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 2e-9           # tests/test_gpu_parity.py, 3+1D
TOL_KERNELS = 5e-11  # variant 6 against variants 3 and 5 there: the rounding of the exponent's argument

# (J, K, n_pT).  aligned: the shipped 24 x 21 x 32 grid itself (|y| up to 5: the edge row blocks the groups were made for).  partial: the second row
# block holds rows {7, 8} and five padded ones -- one real group beside two that keep the floor.  k1 .. k8 (J = 8): a lone real row in a group, a whole group,
# a group partly padded, the last group missing, one real row in the second block.  j5: a padded phi tile.
GRIDS = {"aligned": None, "partial": (20, 9, 5), "k1": (8, 1, 5), "k2": (8, 2, 5), "k3": (8, 3, 5), "k5": (8, 5, 5), "k8": (8, 8, 5), "j5": (5, 7, 5)}
CELLS = (1, 7, 97, 1300)
ORACLE_BUDGET = 1e8  # evaluations (cells x species x bins) the CPU oracle is given per case


def make_grid(fx, shape):
    if GRIDS[shape] is None:
        return fx["grid"]
    J, K, n_pT = GRIDS[shape]
    rng = np.random.default_rng(1000 * J + 10 * K + n_pT)
    return dict(pT=np.linspace(0.05, 3.2, n_pT), phi=np.sort(rng.random(J) * 2 * np.pi), y=np.linspace(-4.5, 5.0, K), eta=fx["grid"]["eta"],
                eta_w=fx["grid"]["eta_w"])


def run(cells, sp, grid, df, df_mode, variant=0, **extra):
    got, st = api.smooth_spectra(cells, sp, grid, df, dict(dimension=3, df_mode=df_mode, kernel_variant=variant, **extra))
    assert st["kernel_variant"] == (variant or 6)
    return got, st


def oracle_error(got, cells, sp, grid, df, df_mode):
    """max rel err against the oracle; on a sample of the species where all of them would cost it more than ORACLE_BUDGET evaluations"""
    o = dict(dimension=3, df_mode=df_mode)
    ns = len(sp["mass"])
    if len(cells["tau"]) * ns * len(grid["pT"]) * len(grid["phi"]) * len(grid["y"]) <= ORACLE_BUDGET:
        return relerr(got, oracle.dN_pTdpTdphidy(cells, sp, grid, df, o))
    order = np.argsort(sp["mass"], kind="stable")
    pick = np.unique(np.concatenate([np.arange(0, ns, 32), order[:1], order[-1:]]))
    sub = {k: (np.asarray(v)[pick] if np.ndim(v) >= 1 and np.shape(v)[0] == ns else v) for k, v in sp.items()}
    ref = oracle.dN_pTdpTdphidy(cells, sub, grid, df, o)
    return relerr(got.reshape(-1, ns)[:, pick].reshape(ref.shape), ref)   # the species index is the fastest of the flat spectrum


@pytest.mark.parametrize("df_mode", [2, 1])
@pytest.mark.parametrize("species", ["pikp", "urqmd"])
@pytest.mark.parametrize("n", CELLS)
@pytest.mark.parametrize("shape", sorted(GRIDS))
def test_row_groups_change_no_bit(fx, shape, n, species, df_mode):
    grid, sp, df = make_grid(fx, shape), fx[species], fx["df"]
    cells = synth.synth_surface(n, 3, seed=2000 + n)
    on, st_on = run(cells, sp, grid, df, df_mode)
    exact, st_exact = run(cells, sp, grid, df, df_mode, zero_skip=1)
    off, st_off = run(cells, sp, grid, df, df_mode, zero_skip=2)
    assert np.isfinite(on).all()
    assert np.array_equal(on, off) and np.array_equal(exact, off)
    assert st_off["n_wave_rows_culled"] == 0 and st_on["n_wave_rows_culled"] >= st_exact["n_wave_rows_culled"]
    assert st_on["n_wave_rows"] == st_exact["n_wave_rows"] == st_off["n_wave_rows"] > 0
    err = oracle_error(on, cells, sp, grid, df, df_mode)
    print("%s n=%d %s df_mode=%d: culled %d of %d wave-rows (exact zeros alone %d), max rel err vs oracle %.3e" % (
        shape, n, species, df_mode, st_on["n_wave_rows_culled"], st_on["n_wave_rows"], st_exact["n_wave_rows_culled"], err))
    assert err < TOL
    # other workgroup shapes: other batch lengths, hence other refresh points -- the same bits
    for wpg in (1, 2, 4):
        got, st = run(cells, sp, grid, df, df_mode, waves_per_group=wpg)
        assert np.array_equal(got, on) and st["n_wave_rows"] == st_on["n_wave_rows"], wpg
    # other cell partitions: other accumulators, culling on against off bitwise on each.  Between partitions the sum is taken in another order: every
    # term is >= 0 (outflow clamp, regulated df), so at most 1 300 roundings of 1.1e-16 each -- 1.5e-13, held at 1e-12
    for nch in (1, 3, 64):
        a, sa = run(cells, sp, grid, df, df_mode, cell_chunks=nch)
        b, sb = run(cells, sp, grid, df, df_mode, cell_chunks=nch, zero_skip=2)
        assert np.array_equal(a, b) and sa["n_wave_rows"] == sb["n_wave_rows"] and sb["n_wave_rows_culled"] == 0, nch
        assert relerr(a, on) < 1e-12, nch


@pytest.mark.parametrize("shape", ["aligned", "partial"])
def test_row_groups_over_several_passes(fx, shape):
    """a workspace that holds a fraction of the cells: the accumulators of a pass start from zero again, the partial spectrum is carried in memory"""
    grid, sp, df = make_grid(fx, shape), fx["pikp"], fx["df"]
    cells = synth.synth_surface(1300, 3, seed=3300)
    small = dict(workspace_bytes=(4 << 20) if shape == "aligned" else (1 << 18))
    on, st_on = run(cells, sp, grid, df, 2, **small)
    off, st_off = run(cells, sp, grid, df, 2, zero_skip=2, **small)
    assert st_on["n_passes"] > 1 and st_off["n_passes"] == st_on["n_passes"]
    assert np.array_equal(on, off) and st_on["n_wave_rows"] == st_off["n_wave_rows"] and st_on["n_wave_rows_culled"] > 0 == st_off["n_wave_rows_culled"]
    assert oracle_error(on, cells, sp, grid, df, 2) < TOL


@pytest.mark.parametrize("which", ["shipped", "offtile"])
@pytest.mark.parametrize("case", hs.CASES)
def test_row_groups_on_hostile_surfaces(fx, case, which):
    """cells 80 binades apart, one cell 2^60 above the rest, space-like and eta-dominated normals, inflow: accumulators that jump by 60 binades
    inside a chunk, or stay zero for most of it, under thresholds that are refreshed at batches 0, 1, 3 only (36 cells)"""
    grid, sp = hs.plain(hs.grid(which)), hs.species()
    cells = hs.surface(case, 3)
    for df_mode in (2, 1):
        for variant in (0, 3):
            on, st_on = run(cells, sp, grid, fx["df"], df_mode, variant)
            exact, _ = run(cells, sp, grid, fx["df"], df_mode, variant, zero_skip=1)
            off, st_off = run(cells, sp, grid, fx["df"], df_mode, variant, zero_skip=2)
            assert np.isfinite(on).all() and np.array_equal(on, off) and np.array_equal(exact, off), (df_mode, variant)
            assert st_on["n_wave_rows"] == st_off["n_wave_rows"] and st_off["n_wave_rows_culled"] == 0, (df_mode, variant)


def counts_case(fx):
    return synth.synth_surface(1300, 3, seed=2600), fx["urqmd"], fx["grid"], fx["df"]


# The cross-variant count bounds are those of tests/test_gpu_parity.py::test_row_culling_changes_no_bit and hold under its partition, three cell
# chunks: the kernels refresh their thresholds per LDS batch, the batches are 6 units (variants 5, 6, 10, 12, 13) or 13 (variant 3), and a count
# compares rules only where a chunk is long against that schedule.  Under the default partition (64-cell chunks: 20 here) variant 3 gets its first
# thresholds at cells 13, 26, 52 of 65 against 6, 12, 24, 48 -- the one-threshold rule itself then differs by 3.9 % between variants 6 and 3
# (1 528 645 against 1 471 221 culled wave-rows of 3 112 200 on this surface, parent commit; 0.57 % with three chunks).
COUNTS_CHUNKS = 3


def test_row_group_counts(fx):
    """1 300 cells x urqmd x the aligned grid: the wave-rows counted are the same whichever way they are culled and however the cells are cut (75
    classes x 32 pT = 2 400 lanes = 38 waves, x cells x 3 x 3 tiles x 7 rows), and variants 6 and 3 cull the same rows to the 3 %
    tests/test_gpu_parity.py holds them to."""
    cells, sp, grid, df = counts_case(fx)
    _, sd = run(cells, sp, grid, df, 2)
    _, sd3 = run(cells, sp, grid, df, 2, 3)
    assert sd["n_wave_rows"] == sd3["n_wave_rows"] == 38 * 1300 * 3 * 3 * 7
    on, s6 = run(cells, sp, grid, df, 2, cell_chunks=COUNTS_CHUNKS)
    _, s6e = run(cells, sp, grid, df, 2, zero_skip=1, cell_chunks=COUNTS_CHUNKS)
    _, s6f = run(cells, sp, grid, df, 2, zero_skip=2, cell_chunks=COUNTS_CHUNKS)
    v3, s3 = run(cells, sp, grid, df, 2, 3, cell_chunks=COUNTS_CHUNKS)
    v3e, _ = run(cells, sp, grid, df, 2, 3, zero_skip=1, cell_chunks=COUNTS_CHUNKS)
    v3f, s3f = run(cells, sp, grid, df, 2, 3, zero_skip=2, cell_chunks=COUNTS_CHUNKS)
    print("1300 cells, urqmd, 24 x 21 x 32: wave-rows %d, culled variant 6 %d (exact zeros alone %d), variant 3 %d" % (
        s6["n_wave_rows"], s6["n_wave_rows_culled"], s6e["n_wave_rows_culled"], s3["n_wave_rows_culled"]))
    assert s6["n_classes"] == 75
    assert s6["n_wave_rows"] == s6e["n_wave_rows"] == s6f["n_wave_rows"] == s3["n_wave_rows"] == s3f["n_wave_rows"] == 38 * 1300 * 3 * 3 * 7
    assert np.array_equal(v3, v3f) and np.array_equal(v3e, v3f) and relerr(on, v3) < TOL_KERNELS
    assert s6["n_wave_rows_culled"] > s6e["n_wave_rows_culled"] > 0 == s6f["n_wave_rows_culled"] == s3f["n_wave_rows_culled"]
    assert abs(s6["n_wave_rows_culled"] - s3["n_wave_rows_culled"]) <= 3e-2 * s3["n_wave_rows_culled"]


@pytest.mark.devlib
@pytest.mark.skipif(not api.DEV_LIB, reason="kernel variants 5, 10, 12 and 13 exist in the developer build only")
def test_row_group_counts_against_the_tile_rule(fx):
    """Developer build: variant 13 keeps one threshold per (lane, tile) -- the groups cull at least its rows; variants 5, 10 and 12 take the groups with
    the default, held to it as tests/test_gpu_parity.py::test_row_culling_changes_no_bit holds them (and under its partition: COUNTS_CHUNKS).  The
    tile rule's count under the default partition is checked besides: there, too, the groups cull at least its rows."""
    cells, sp, grid, df = counts_case(fx)
    nch = dict(cell_chunks=COUNTS_CHUNKS)
    on, s6 = run(cells, sp, grid, df, 2, **nch)
    _, s13 = run(cells, sp, grid, df, 2, 13, **nch)
    v3, s3 = run(cells, sp, grid, df, 2, 3, **nch)
    print("culled wave-rows of %d: variant 6 %d, variant 13 (tile rule) %d, variant 3 %d" % (
        s6["n_wave_rows"], s6["n_wave_rows_culled"], s13["n_wave_rows_culled"], s3["n_wave_rows_culled"]))
    assert s13["n_wave_rows"] == s6["n_wave_rows"] and s6["n_wave_rows_culled"] >= s13["n_wave_rows_culled"] > 0
    _, d6 = run(cells, sp, grid, df, 2)
    _, d13 = run(cells, sp, grid, df, 2, 13)
    assert d13["n_wave_rows"] == d6["n_wave_rows"] and d6["n_wave_rows_culled"] >= d13["n_wave_rows_culled"] > 0
    v5, s5 = run(cells, sp, grid, df, 2, 5, **nch)
    v5e, _ = run(cells, sp, grid, df, 2, 5, zero_skip=1, **nch)
    v5f, s5f = run(cells, sp, grid, df, 2, 5, zero_skip=2, **nch)
    assert np.array_equal(v5, v5f) and np.array_equal(v5e, v5f) and s5f["n_wave_rows_culled"] == 0 and s5["n_wave_rows"] == s6["n_wave_rows"]
    assert relerr(on, v5) < TOL_KERNELS and relerr(v5, v3) < TOL_KERNELS
    assert abs(s6["n_wave_rows_culled"] - s5["n_wave_rows_culled"]) <= 2e-2 * s5["n_wave_rows_culled"]
    assert abs(s5["n_wave_rows_culled"] - s3["n_wave_rows_culled"]) <= 2e-2 * s3["n_wave_rows_culled"]
    for variant, wpg in ((10, 1), (12, 4)):
        for extra in (dict(), dict(waves_per_group=wpg), dict(zero_skip=1), dict(zero_skip=2)):
            got, st = run(cells, sp, grid, df, 2, variant, **nch, **extra)
            assert np.array_equal(got, on) and st["n_wave_rows"] == s6["n_wave_rows"], (variant, extra)
