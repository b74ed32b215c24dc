"""GPU (-m gpu): every path that takes a power-of-two scale out of p.dsigma -- or sits beside one -- on the surfaces of
tests/hostile_surfaces.py, against the oracle's plain `if (pds <= 0)` arithmetic.  The kernels form max(p.dsigma, 0) with the VOP3 clamp of
an add / fma on p.dsigma 2^-e; where the bound behind e misses a term, or e is stale, the clamp returns 1 and the spectrum is finite and
wrong.  These surfaces put cells 80 binades apart, one cell 2^60 above the rest, space-like and eta-dominated normals and inflow cells in
front of the three pieces of code that choose e (cf_pds_bound / pds_scale, cf_prep_feqmod phase 2e, the shards of cf_multi.hip).

Tolerances are the ones the subsystems' tests hold: 2e-9 for spectra (tests/test_gpu_parity.py, tests/test_gpu_fuzz.py; with outflow = 0
against the cancellation-aware scale of test_gpu_fuzz.py), 1e-10 / 1e-9 for operation 0 with df_mode 1, 2 / 3, 4 (tests/test_gpu_offtile.py;
with the outflow cut per cell, relative: a vs-max metric would pass with every small cell wrong), assert_close of
tests/test_gpu_polarization.py for mode 5, 1e-12 between a sharded and a single-device spectrum (tests/test_gpu_parity.py, shard additivity).
Under a uniform 2^k the spectrum is ldexp(base, k) bit for bit, culls on or off.

What these cases found: a live cell past the b < 1e300 cut of cf_pds_bound (and of phase 2e) took the scale of the OTHER cells, so its
clamped p.dsigma read 1: a finite spectrum that the oracle does not have.  cf_prep and cf_prep_feqmod now leave such a cell out and report it
(IS3D_EDOMAIN names it).  Nothing else: no bound misses a term, status[6] does not survive an execute, no cull threshold is absolute.

Worst errors on an MI355X (every case, grid, flag and cull setting of a path):
    delta-f spectra, outflow = 1     3+1D 2.6e-10 (regulate_deltaf = 0: bins where 1 + df changes sign)   2+1D 1.4e-12   baryon slots 2.1e-12
    delta-f spectra, outflow = 0     3+1D 2.6e-10   2+1D 1.5e-11   (against the cancellation-aware scale)
    modified equilibrium             df_mode 4 with the cut 1.1e-12 / 3.6e-14 (3+1D / 2+1D), without 8.9e-13 / 1.1e-14; df_mode 3 9.4e-13 / 1.5e-14
    anisotropic hydro                3+1D 1.4e-10   2+1D 1.8e-13
    operation 0, dN_dy_cell          df_mode 2: 3.0e-14 relative per cell, 1.5e-14 vs-max signed; df_mode 4: 1.7e-14, 1.0e-14
    mode 5                           7.3e-14 of the array maximum
    three shards                     4.2e-15 against one device, 5.8e-12 against the oracle
    uniform 2^k, k = -100, -7, 33, 100    bit for bit on all four paths, with zero_skip = 2 and with the default culls

Sensitivity, once, on scratch builds: without the pTmax (|dax| + |day|) term of cf_pds_bound the `spacelike` delta-f spectra fail (3+1D on the
off-tile grid, 2+1D on both grids, every df_mode / regulate_deltaf) and nothing else, old parity files included; with e_c - 1 in phase 2e
`spacelike` df_mode 4 fails in both dimensions and the uniform-2^k test in 3+1D, nothing in the old files.  Time-like cells hide both: the
lanes that exceed a bound that is one binade short sit at the largest |y - eta|, where the exponential has long taken the term away.
Operation 0 forms its cut with a max (cf_spacetime.hip), so only its un-scale is on trial here."""
from functools import lru_cache

import numpy as np
import pytest

import dndx_feqmod_ref
import hostile_surfaces as H
import offtile_cases as OC
from conftest import relerr
from is3d_amd import api, inputs, synth
from oracle import oracle
from test_gpu_offtile import rel_err
from test_gpu_polarization import assert_close, restate
from test_gpu_spacetime import err_vs_max, oracle_cells
from test_gpu_spacetime_feqmod import check_against_restatement

pytestmark = pytest.mark.gpu

TOL = 2e-9            # spectra: tests/test_gpu_parity.py, tests/test_gpu_fuzz.py
TOL_OP0 = {2: 1e-10, 4: 1e-9}   # tests/test_gpu_offtile.py
TOL_SHARDS = 1e-12    # tests/test_gpu_parity.py: a sharded against a single-device spectrum
SIGNED = dict(outflow=0, regulate_deltaf=0)
DIMS = {c: ((3,) if c == "eta_heavy" else (3, 2)) for c in H.CASES}


def spectra_grid(gname, dim):
    g = H.plain(H.grid(gname))
    if dim == 2 and gname == "shipped":
        g = dict(g, pT=g["pT"][::4], phi=g["phi"][::3])   # the 241-node eta sum multiplies the oracle's work (tests/test_hostile_surfaces.py runs the same)
    return g


def frozen(a):
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def df_tables(baryon):
    return inputs.df_tables_full() if baryon else inputs.df_tables()


@lru_cache(maxsize=None)
def df_reference(case, dim, gname, df_mode, regulate, outflow, baryon):
    """(oracle spectrum, the scale its bins are judged against): |ref|, and with outflow = 0 the cancellation-aware scale of
    tests/test_gpu_fuzz.py -- 1e-4 of what was added up, from two oracle runs with the cut (dsigma as it is and negated)"""
    cells, g, df = H.surface(case, dim, baryon=baryon), spectra_grid(gname, dim), df_tables(baryon)
    o = dict(dimension=dim, df_mode=df_mode, regulate_deltaf=regulate, outflow=outflow, include_baryon=int(baryon), include_baryondiff_deltaf=int(baryon))
    ref = oracle.dN_pTdpTdphidy(cells, H.species(), g, df, o)
    scale = np.abs(ref)
    if not outflow:
        pos = oracle.dN_pTdpTdphidy(cells, H.species(), g, df, dict(o, outflow=1, regulate_deltaf=1))
        neg = oracle.dN_pTdpTdphidy({k: (-v if k in H.DS else v) for k, v in cells.items()}, H.species(), g, df, dict(o, outflow=1, regulate_deltaf=1))
        scale = np.maximum(scale, 1e-4 * (pos + neg))
    return o, frozen(ref), frozen(scale)


DF_RUNS = [(c, d, 1) for c in H.CASES for d in DIMS[c]] + [(c, d, 0) for c in ("binades", "spacelike") for d in (3, 2)]


@pytest.mark.parametrize("gname", ["shipped", "offtile"])
@pytest.mark.parametrize("regulate", [1, 0])
@pytest.mark.parametrize("df_mode", [2, 1])
@pytest.mark.parametrize("case,dim,outflow", DF_RUNS, ids=["%s-%dd-outflow%d" % r for r in DF_RUNS])
def test_deltaf_spectra(case, dim, outflow, df_mode, regulate, gname):
    """the per-execute scale (cf_pds_bound, pds_scale, lane_pe, cf_finalize): default kernel and, in 3+1D, the 8 x 7 tile without the E2
    stream (kernel_variant 3); row culls on and off"""
    o, ref, scale = df_reference(case, dim, gname, df_mode, regulate, outflow, False)
    cells, g = H.surface(case, dim), spectra_grid(gname, dim)
    worst = 0.0
    for variant in ((0, 3) if dim == 3 else (0,)):
        for zs in (0, 2):
            got, st = api.smooth_spectra(cells, H.species(), g, df_tables(False), dict(o, kernel_variant=variant, zero_skip=zs))
            assert np.isfinite(got).all()
            assert st["n_cells_skipped"] == int((~H.live(cells)).sum()) and st["bad_cell"] == -1
            err = float(np.max(np.abs(got - ref) / np.maximum(scale, 1e-280)))
            worst = max(worst, err)
            assert err < TOL, (variant, zs, st["kernel_variant"], err)
    print("delta-f %s %d+1D outflow=%d df_mode=%d regulate=%d %s: worst error %.3e" % (case, dim, outflow, df_mode, regulate, gname, worst))


@pytest.mark.parametrize("df_mode", [2, 1])
def test_deltaf_spectra_with_baryon_slots(df_mode):
    o, ref, scale = df_reference("binades", 3, "shipped", df_mode, 1, 1, True)
    for zs in (0, 2):
        got, st = api.smooth_spectra(H.surface("binades", 3, baryon=True), H.species(), spectra_grid("shipped", 3), df_tables(True), dict(o, zero_skip=zs))
        err = relerr(got, ref)
        print("delta-f binades 3+1D include_baryon=1 df_mode=%d zero_skip=%d: %.3e" % (df_mode, zs, err))
        assert err < TOL


# ---- modified equilibrium ----
@lru_cache(maxsize=None)
def fq_reference(case, dim, gname, df_mode, outflow):
    cells, g = H.surface(case, dim), spectra_grid(gname, dim)
    fq = inputs.feqmod_tables(inputs.surface_average_T(cells))
    o = dict(dimension=dim, df_mode=df_mode, outflow=outflow)
    ref, _ = oracle.dN_pTdpTdphidy_feqmod(cells, H.species(), g, inputs.df_tables(), fq, o)
    return o, fq, frozen(ref)


FQ_RUNS = [(c, d, 4, 1) for c in ("binades",) + H.GIANTS + ("spacelike", "eta_heavy") for d in DIMS[c]] + \
          [("binades", d, 3, 1) for d in (3, 2)] + [("binades", d, 4, 0) for d in (3, 2)]


@pytest.mark.parametrize("gname", ["shipped", "offtile"])
@pytest.mark.parametrize("case,dim,df_mode,outflow", FQ_RUNS, ids=["%s-%dd-mode%d-outflow%d" % r for r in FQ_RUNS])
def test_modified_equilibrium_spectra(case, dim, df_mode, outflow, gname):
    """df_mode 4 with the outflow cut: the CLAMP instantiations of cf_main_feqmod and the per-cell e_c of phase 2e, which comes back through
    exp_p9_scaled; df_mode 3 and outflow = 0 run beside it without a scale"""
    o, fq, ref = fq_reference(case, dim, gname, df_mode, outflow)
    cells, g = H.surface(case, dim), spectra_grid(gname, dim)
    assert np.isfinite(ref).all()
    for zs in (0, 2):
        got, st = api.smooth_spectra(cells, H.species(), g, inputs.df_tables(), dict(o, zero_skip=zs), fq=fq)
        err = relerr(got, ref)
        print("feqmod %s %d+1D df_mode=%d outflow=%d %s zero_skip=%d: %.3e" % (case, dim, df_mode, outflow, gname, zs, err))
        assert np.isfinite(got).all() and st["bad_cell"] == -1
        assert err < TOL


# ---- anisotropic hydro (no outflow cut on this path) ----
@pytest.mark.parametrize("gname", ["shipped", "offtile"])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("case", ("binades",) + H.GIANTS)
def test_anisotropic_hydro_spectra(case, dim, gname):
    cells, g = H.surface(case, dim, vah=True), spectra_grid(gname, dim)
    ref = oracle.dN_pTdpTdphidy_vah(cells, H.species(), g, dict(dimension=dim))
    for zs in (0, 2):
        got, _ = api.smooth_spectra_vah(cells, H.species(), g, dict(dimension=dim, zero_skip=zs))
        err = relerr(got, ref, floor=1e-270)
        print("vah %s %d+1D %s zero_skip=%d: %.3e" % (case, dim, gname, zs, err))
        assert err < TOL


# ---- operation 0 ----
def op0_grid(dim):
    """the off-tile grid; in 2+1D every second eta node, weight doubled: 5 pT values x 241 eta nodes are past the LDS bound of the df_mode 3 / 4
    per-cell kernel (192 nodes; tests/offtile_cases.py: op0_lds_max_eta)"""
    g = H.grid("offtile")
    return g if dim == 3 else dict(g, eta=g["eta"][::2], eta_w=2.0 * g["eta_w"][::2])


@lru_cache(maxsize=None)
def op0_reference(case, dim, df_mode, outflow):
    cells, g = H.surface(case, dim), op0_grid(dim)
    o = dict(dimension=dim, df_mode=df_mode, **({} if outflow else SIGNED))
    if df_mode == 2:
        return o, None, frozen(oracle_cells(cells, range(H.N_CELLS), H.species(), g, inputs.df_tables(), o))
    fq = inputs.feqmod_tables(inputs.surface_average_T(cells))
    return o, fq, dndx_feqmod_ref.dndx(cells, H.species(), g, inputs.df_tables(), fq, o)


@pytest.mark.parametrize("outflow", [1, 0])
@pytest.mark.parametrize("df_mode", [2, 4])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("case", ["binades", "spacelike"])
def test_operation_0_per_cell(case, dim, df_mode, outflow):
    """st_unscale reads the bound of the delta-f records (df_mode 2); df_mode 4 runs on unscaled records.  With the outflow cut every cell's
    yield is held to its OWN size: the small cells of `binades` are the point."""
    o, fq, want = op0_reference(case, dim, df_mode, outflow)
    cells, g = H.surface(case, dim), op0_grid(dim)
    bins = OC.bins_for(cells)
    res = api.spacetime_distributions(cells, H.species(), g, inputs.df_tables(), bins, o, per_cell=True, fq=fq)
    pc = want if df_mode == 2 else want["per_cell"]
    tol = TOL_OP0[df_mode]
    err = rel_err(res["dN_dy_cell"], pc) if outflow else err_vs_max(res["dN_dy_cell"], pc)
    print("operation 0 %s %d+1D df_mode=%d outflow=%d: dN_dy_cell %s error %.3e" % (case, dim, df_mode, outflow, "relative" if outflow else "vs-max", err))
    assert err < tol
    if df_mode == 4:
        check_against_restatement(res, want, cells, bins, not outflow, dim)
    else:
        assert err_vs_max(res["dN_dy"], pc.sum(axis=1)) < tol


# ---- mode 5 ----
@pytest.mark.parametrize("dim", [3, 2])
def test_mode_5(dim):
    cells, g = H.surface("binades", dim), H.plain(H.grid("shipped" if dim == 3 else "offtile"))
    w = synth.synth_vorticity(H.N_CELLS, seed=77 + dim)
    T = 0.1503
    got = api.spin_polarization(cells, w, H.species(), g, T, dict(dimension=dim))
    ref = restate(cells, w, H.species(), g, T, dim)
    print("mode 5 binades %d+1D: worst error against the array maximum %.3e" % (
        dim, max(float(np.max(np.abs(got[k] - ref[k])) / np.max(np.abs(ref[k]))) for k in api.POLARIZATION_OUTPUTS)))
    assert_close(got, ref)


# ---- shards: a different shard takes the large e each time ----
@pytest.mark.parametrize("path", ["df-3d", "df-2d", "fq-3d"])
@pytest.mark.parametrize("case", H.GIANTS)
def test_three_shards_against_one_device(case, path):
    dim = 2 if path == "df-2d" else 3
    cells, g = H.surface(case, dim), spectra_grid("offtile", dim)
    if path.startswith("fq"):
        o, fq, ref = fq_reference(case, dim, "offtile", 4, 1)
    else:
        (o, ref, _), fq = df_reference(case, dim, "offtile", 2, 1, 1, False), None
    one, _ = api.smooth_spectra(cells, H.species(), g, inputs.df_tables(), o, fq=fq)
    multi, agg, shards = api.smooth_spectra_multi(cells, H.species(), g, inputs.df_tables(), o, devices=[0] * 3, fq=fq)
    assert len(shards) == 3
    d, e = relerr(multi, one), relerr(multi, ref)
    print("shards %s %s: against one device %.3e, against the oracle %.3e" % (case, path, d, e))
    assert d < TOL_SHARDS and e < TOL


# ---- plan reuse: no bound survives an execute ----
@pytest.mark.parametrize("path", ["df-3d", "df-2d", "fq-3d", "fq-2d"])
def test_plan_executes_giant_then_the_untouched_surface(path):
    import torch
    dim = int(path[3])
    g, sp, df = spectra_grid("offtile", dim), H.species(), inputs.df_tables()
    giant, plain_cells = H.surface("giant-middle", dim), H.base(dim)
    fq = inputs.feqmod_tables(inputs.surface_average_T(plain_cells)) if path.startswith("fq") else None
    o = dict(dimension=dim, df_mode=4 if fq else 2)
    dev = torch.device("cuda:0")

    def run(plan, cells):
        t = {k: torch.from_numpy(np.ascontiguousarray(cells[k])).to(dev) for k in synth.CELL_FIELDS}
        out = torch.zeros(plan.output_size, dtype=torch.float64, device=dev)
        plan.execute(H.N_CELLS, {k: v.data_ptr() for k, v in t.items()}, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    fresh = api.Plan(sp, g, df, o, max_cells=H.N_CELLS, fq=fq)
    reused = api.Plan(sp, g, df, o, max_cells=H.N_CELLS, fq=fq)
    try:
        want = run(fresh, plain_cells)
        big = run(reused, giant)
        again = run(reused, plain_cells)
    finally:
        fresh.close()
        reused.close()
    assert big.max() > 2.0 ** 50 * want.max()
    assert again.tobytes() == want.tobytes()


# ---- out of range ----
@pytest.mark.parametrize("path", ["df-3d", "df-2d", "fq-3d", "fq-2d"])
def test_a_cell_past_the_1e300_cut_is_refused_or_right(path):
    """dat = 1e301 on one live cell: past the b < 1e300 cut of cf_pds_bound and of phase 2e there is no scale.  Either the call names the cell
    (IS3D_EDOMAIN) or its spectrum is the oracle's; a finite spectrum that is not the oracle's is the silent clamp."""
    dim = int(path[3])
    cells, bad = H.out_of_range(dim)
    assert H.live(cells)[bad]
    g, sp, df = spectra_grid("offtile", dim), H.species(), inputs.df_tables()
    fq = inputs.feqmod_tables(inputs.surface_average_T(H.base(dim))) if path.startswith("fq") else None
    o = dict(dimension=dim, df_mode=4 if fq else 2)
    try:
        got, st = api.smooth_spectra(cells, sp, g, df, o, fq=fq)
    except api.Is3dError as e:
        print("%s: refused: %s" % (path, e))
        assert e.code == api.IS3D_EDOMAIN and ("cell %d:" % bad) in str(e) and "1e300" in str(e)
        return
    with np.errstate(over="ignore", invalid="ignore"):
        ref = oracle.dN_pTdpTdphidy_feqmod(cells, sp, g, df, fq, o)[0] if fq else oracle.dN_pTdpTdphidy(cells, sp, g, df, o)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    ok = np.isfinite(ref)
    assert relerr(got[ok], ref[ok]) < TOL


# ---- exactness under a uniform power of two ----
def exact_run(path, dim, cells, zs):
    g, sp = H.exact_grid(dim), H.species()
    if path == "vah":
        return api.smooth_spectra_vah(cells, sp, g, dict(dimension=dim, zero_skip=zs))[0]
    fq = inputs.feqmod_tables(inputs.surface_average_T(H.exact_base(dim))) if path == "fq" else None
    return api.smooth_spectra(cells, sp, g, inputs.df_tables(), dict(dimension=dim, df_mode=4 if fq else 2, zero_skip=zs), fq=fq)[0]


@pytest.mark.parametrize("zero_skip", [2, 0])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("path", ["df", "fq", "vah"])
def test_a_uniform_power_of_two_is_exact(path, dim, zero_skip):
    """dsigma -> 2^k dsigma gives ldexp(spectrum, k) bit for bit: every scale is a power of two and comes back as one, and the default culls
    compare against the accumulators (nothing absolute), so they drop the same rows at every k"""
    cells = H.exact_base(dim, vah=path == "vah")
    base = exact_run(path, dim, cells, zero_skip)
    assert np.isfinite(base).all() and np.abs(base[base != 0]).min() > 1e-150
    for k in H.UNIFORM_K:
        got = exact_run(path, dim, H.uniform(cells, k), zero_skip)
        same = np.array_equal(got, np.ldexp(base, k))
        print("uniform(%d) %s %d+1D zero_skip=%d: %s" % (k, path, dim, zero_skip, "bit for bit" if same else "max rel diff %.3e" % relerr(got, np.ldexp(base, k), floor=1e-300)))
        assert same, k
