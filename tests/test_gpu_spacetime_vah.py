"""GPU: operation 0 for anisotropic hydro (is3d_spacetime_distributions_vah, is3d_vah_plan_execute_spacetime; cf_spacetime_vah.hip).  The
reference has no such routine; the oracle pins it unmodified: dN_dy_cell of one cell is oracle.dN_pTdpTdphidy_vah of that cell alone,
contracted with w_pT w_phi and summed over y (in 2+1D the oracle's eta sum already carries w_k deta).

Worst errors of dN_dy_cell against that route, relative to the largest |value| of the array (the values change sign), measured on an
MI355X -- tolerance 2e-9, the VAH parity tolerance of tests/test_gpu_vah.py:
    3+1D shipped grid   {} 6.7e-15   regulate_deltaf=0 5.4e-15   include_bulk_deltaf=0 6.9e-15   include_shear_deltaf=0 6.1e-15
    2+1D shipped grid   {} 1.8e-15   regulate_deltaf=0 1.7e-15   include_bulk_deltaf=0 8.2e-16   include_shear_deltaf=0 2.5e-15
    off-tile grid (13 pT, 5 phi, 9 y | 40 eta)   3+1D 2.7e-15   2+1D 1.1e-15
2+1D dN_dydeta at the nodes 0, 60, 120, 180, 240: 5.3e-15 (off-tile grid, nodes 0, 13, 30, 39: 6.0e-15); the equilibrium link of 3+1D: 2.1e-15."""
import os
import subprocess

import numpy as np
import pytest

import refformat
from is3d_amd import api, inputs, synth
from oracle import oracle
from test_gpu_spacetime import CLI_BINS, binned, bins_of, contract, err_vs_max, read_dir, wgrid

pytestmark = pytest.mark.gpu
TOL = 2e-9   # tests/test_gpu_vah.py
SPECIES3 = [211, 321, 2212, -2212, 3122, 333]   # five classes: 2 1/2 waves at 32 pT, one wave half filled
COEF = ("c0", "c1", "c2", "c3", "c4")
SMALL_WS = 200000   # bytes: 23 cells of 3+1D records per pass, 2 cells of 2+1D records


def surface(dim):
    """the issue's surfaces: every cell inside the coefficient tables, and the cell with the largest tau -- outside the tau bins -- given
    u.dsigma < 0, which this path neither skips nor leaves out of its counters"""
    cells = synth.synth_vah_surface(70 if dim == 3 else 9, dim, seed=900 + dim)
    _, found = oracle.vah_coefficients(inputs.vah_df_tables(), cells["Lambda"], cells["aL"])
    assert found.all()
    cells["dat"][int(np.argmax(cells["tau"]))] *= -1.0
    return cells


def species(fx, dim):
    return inputs.species(SPECIES3) if dim == 3 else fx["pikp"]


def surface_bins(cells):
    r = np.sqrt(cells["x"] ** 2 + cells["y"] ** 2)
    return dict(tau_min=float(cells["tau"].min()) + 0.01, tau_max=0.9 * float(cells["tau"].max()), tau_bins=7, r_min=0.0,
                r_max=0.8 * float(r.max()), r_bins=5)


def grid_of(fx, name):
    g = wgrid(fx)
    if name == "shipped":
        return g
    # off the tiles: 13 pT (16 lane slots, 3 idle), 5 phi (one clamped tile), 9 y / 40 eta (2 row blocks, 5 / 22 padding rows); weights of the same rows
    return dict(pT=g["pT"][:13], pT_w=g["pT_w"][:13], phi=g["phi"][:5], phi_w=g["phi_w"][:5], y=g["y"][:9], eta=g["eta"][:40], eta_w=g["eta_w"][:40])


def uds(cells):
    ut = np.sqrt(1.0 + cells["ux"] ** 2 + cells["uy"] ** 2 + cells["tau"] ** 2 * cells["un"] ** 2)
    return ut * cells["dat"] + cells["ux"] * cells["dax"] + cells["uy"] * cells["day"] + cells["un"] * cells["dan"]


def oracle_cells_vah(cells, sp, g, o):
    """[S][n]: the oracle's dN_dy_cell, one cell at a time"""
    n = len(cells["tau"])
    out = np.zeros((len(sp["mass"]), n))
    for c in range(n):
        one = {k: v[c:c + 1] for k, v in cells.items()}
        out[:, c] = contract(oracle.dN_pTdpTdphidy_vah(one, sp, g, o), sp, g, o["dimension"])
    return out


_RUNS = {}


def run(fx, dim, grid="shipped", **flags):
    """library result (per_cell) of the issue's surface, computed once per case"""
    key = (dim, grid, tuple(sorted(flags.items())))
    if key not in _RUNS:
        cells = surface(dim)
        _RUNS[key] = (cells, api.spacetime_distributions_vah(cells, species(fx, dim), grid_of(fx, grid), surface_bins(cells),
                                                              dict(dimension=dim, **flags), per_cell=True))
    return _RUNS[key]


FLAGS = [dict(), dict(regulate_deltaf=0), dict(include_bulk_deltaf=0), dict(include_shear_deltaf=0)]


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("grid,flags", [("shipped", f) for f in FLAGS] + [("off-tile", {})],
                         ids=["shipped-" + ("-".join(f) or "default") for f in FLAGS] + ["off-tile"])
def test_parity_with_the_oracle(fx, dim, grid, flags):
    cells, res = run(fx, dim, grid, **flags)
    sp, g, o = species(fx, dim), grid_of(fx, grid), dict(dimension=dim, **flags)
    ref = oracle_cells_vah(cells, sp, g, o)
    assert np.isfinite(ref).all()
    neg = int(np.argmax(cells["tau"]))
    assert uds(cells)[neg] < 0
    if grid == "shipped" and not flags:   # not skipped: a negative value (an unregulated delta-f can flip it; the off-tile eta rows, all far backward, see little of the cell)
        assert (ref[:, neg] < 0).all() and (res["dN_dy_cell"][:, neg] < 0).all()
    # the per-cell values sum to the whole-surface contraction
    whole = contract(oracle.dN_pTdpTdphidy_vah(cells, sp, g, o), sp, g, dim)
    assert err_vs_max(ref.sum(axis=1), whole) < 1e-13
    err = err_vs_max(res["dN_dy_cell"], ref)
    print("dN_dy_cell dim=%d grid=%s flags=%s: worst error / max |value| = %.3e" % (dim, grid, flags, err))
    assert err < TOL
    bins = surface_bins(cells)
    t, r, tr = binned(ref, cells, bins)
    for name, want in (("dN_taudtaudy", t), ("dN_twopirdrdy", r), ("dN_twopitaurdtaudrdy", tr), ("dN_dy", ref.sum(axis=1))):
        assert err_vs_max(res[name], want) < TOL, name
    if dim == 3:
        assert res["dN_dydeta"].shape == (len(sp["mass"]), 1)
        assert np.array_equal(res["dN_dydeta"][:, 0], res["dN_dy"])
    assert res["stats"]["n_classes"] == (5 if dim == 3 else 3)


@pytest.mark.parametrize("dim", [3, 2])
def test_order_of_additions_and_counters(fx, dim):
    cells, res = run(fx, dim)
    bins = surface_bins(cells)
    pc = res["dN_dy_cell"]
    t, r, tr = binned(pc, cells, bins)
    assert np.array_equal(res["dN_taudtaudy"], t)
    assert np.array_equal(res["dN_twopirdrdy"], r)
    assert np.array_equal(res["dN_twopitaurdtaudrdy"], tr)
    assert np.array_equal(res["dN_dy"], np.cumsum(pc, axis=1)[:, -1])
    it, ir = bins_of(cells, bins)
    st = res["stats"]
    # ALL cells, whatever the sign of u.dsigma: 1 below and 9 / 2 above the tau bins, 15 / 4 outside the r bins; the negated cell is one of them
    out_t, out_r = (it < 0) | (it >= bins["tau_bins"]), (ir < 0) | (ir >= bins["r_bins"])
    assert (int(np.sum(it < 0)), int(np.sum(it >= bins["tau_bins"])), int(np.sum(out_r))) == ((1, 9, 15) if dim == 3 else (1, 2, 4))
    assert out_t[int(np.argmax(cells["tau"]))] and int(np.sum(out_t & (uds(cells) > 0))) == int(np.sum(out_t)) - 1
    assert st["n_tau_outside"] == int(np.sum(out_t)) and st["n_r_outside"] == int(np.sum(out_r))
    assert st["n_tau_negative"] == int(np.sum(it < 0)) and st["n_r_negative"] == int(np.sum(ir < 0))
    assert st["n_cells_skipped"] == 0


@pytest.mark.parametrize("dim", [3, 2])
def test_bitwise_invariances(fx, dim):
    cells, res = run(fx, dim)
    sp, g, bins = species(fx, dim), wgrid(fx), surface_bins(cells)
    # cell_chunks is not read on this path (the chunk count comes from the lane waves: is3d_vah_plan_execute_spacetime): that entry only proves
    # the option harmless.  Chunks of more than one cell run in tests/test_gpu_spacetime_vah_offtile.py.
    for extra in (dict(), dict(workspace_bytes=SMALL_WS), dict(cell_chunks=3), dict(zero_skip=2)):
        got = api.spacetime_distributions_vah(cells, sp, g, bins, dict(dimension=dim, **extra), per_cell=True)
        if "workspace_bytes" in extra:
            assert got["stats"]["n_passes"] > 1
        for k in api.SPACETIME_OUTPUTS:
            assert np.array_equal(got[k], res[k]), (extra, k)
    # D of a cell depends on that cell alone
    for c in (0, int(np.argmax(cells["tau"])), len(cells["tau"]) - 1):
        one = api.spacetime_distributions_vah({k: v[c:c + 1] for k, v in cells.items()}, sp, g, bins, dict(dimension=dim), per_cell=True)
        assert np.array_equal(one["dN_dy_cell"][:, 0], res["dN_dy_cell"][:, c]), c


@pytest.mark.parametrize("dim", [3, 2])
def test_tables_give_the_coefficients_of_the_cells(fx, dim):
    cells, _ = run(fx, dim)
    sp, g, bins, tab = species(fx, dim), wgrid(fx), surface_bins(cells), inputs.vah_df_tables()
    from_tab = api.spacetime_distributions_vah({k: v for k, v in cells.items() if k not in COEF}, sp, g, bins, dict(dimension=dim), per_cell=True, tab=tab)
    coef = api.vah_coefficients(tab, cells["Lambda"], cells["aL"])
    from_cells = api.spacetime_distributions_vah(dict(cells, **coef), sp, g, bins, dict(dimension=dim), per_cell=True)
    for k in api.SPACETIME_OUTPUTS:
        assert np.array_equal(from_tab[k], from_cells[k]), k
    assert np.isfinite(from_tab["dN_dy_cell"]).all() and (from_tab["dN_dy_cell"] != 0).all()


@pytest.mark.parametrize("grid", ["shipped", "off-tile"])
def test_dN_dydeta_2d(fx, grid):
    cells, res = run(fx, 2, grid)
    sp, g, o = fx["pikp"], grid_of(fx, grid), dict(dimension=2)
    deta = g["eta"][1] - g["eta"][0]
    K = len(g["eta"])

    def node(k):   # the oracle on the two-node grid [eta_k, eta_k + deta], weights [w_k, 0]: that node's term of the eta sum
        g2 = dict(g, eta=np.array([g["eta"][k], g["eta"][k] + deta]), eta_w=np.array([g["eta_w"][k], 0.0]))
        return contract(oracle.dN_pTdpTdphidy_vah(cells, sp, g2, o), sp, g2, 2)

    terms = np.stack([node(k) for k in range(K)], axis=1)   # [S][K]
    whole = contract(oracle.dN_pTdpTdphidy_vah(cells, sp, g, o), sp, g, 2)
    # the route is the oracle's own eta sum taken term by term: what remains is the rounding of K additions in another order (2e-15 measured, shipped grid)
    assert err_vs_max(terms.sum(axis=1), whole) < K * 2.0 ** -52
    assert res["dN_dydeta"].shape == (3, K)
    worst = 0.0
    for k in ([0, 60, 120, 180, 240] if grid == "shipped" else [0, 13, 30, 39]):
        err = err_vs_max(res["dN_dydeta"][:, k], terms[:, k] / (g["eta_w"][k] * deta))
        worst = max(worst, err)
        assert err < TOL, k
    print("dN_dydeta grid=%s: worst error / max |value| = %.3e" % (grid, worst))
    assert err_vs_max(res["dN_dydeta"] @ (g["eta_w"] * deta), res["dN_dy"]) < 1e-12


def test_equilibrium_link_3d(fx):
    """a_L = 1, Lambda = T and both corrections off: f_a is the equilibrium distribution, so the result is that of the viscous-hydro
    operation 0 with its delta-f corrections and its outflow cut off -- on the cells that path does not skip (u.dsigma > 0)."""
    cells = surface(3)
    eq = dict(cells, aL=np.ones_like(cells["aL"]), Lambda=cells["T"].copy())
    sp, g, bins = species(fx, 3), wgrid(fx), surface_bins(cells)
    off = dict(dimension=3, include_bulk_deltaf=0, include_shear_deltaf=0)
    got = api.spacetime_distributions_vah(eq, sp, g, bins, off, per_cell=True)
    vh = api.spacetime_distributions(eq, sp, g, fx["df"], bins, dict(off, df_mode=1, outflow=0), per_cell=True)
    lv = uds(cells) > 0
    assert int(np.sum(~lv)) == 1 and np.all(vh["dN_dy_cell"][:, ~lv] == 0.0) and np.all(got["dN_dy_cell"][:, ~lv] < 0.0)
    err = err_vs_max(got["dN_dy_cell"][:, lv], vh["dN_dy_cell"][:, lv])
    print("equilibrium link: worst error / max |value| = %.3e" % err)
    assert err < TOL


def test_domain_and_refusals(fx):
    cells = surface(3)
    sp, g, bins = fx["pikp"], wgrid(fx), surface_bins(cells)
    bad = dict(cells, Lambda=cells["Lambda"].copy())
    bad["Lambda"][11] = 1e-12
    for dim, tab in ((3, None), (2, None), (3, inputs.vah_df_tables())):
        with pytest.raises(api.Is3dError) as e:
            api.spacetime_distributions_vah(bad, sp, g, bins, dict(dimension=dim), tab=tab)
        assert e.value.code == api.IS3D_EDOMAIN and e.value.bad_cell == 11, (dim, tab is not None)
    hot = dict(cells, Lambda=2.5 * cells["Lambda"])   # beyond the last Lambda node of the tables
    with pytest.raises(api.Is3dError) as e:
        api.spacetime_distributions_vah(hot, sp, g, bins, dict(dimension=3), tab=inputs.vah_df_tables())
    assert e.value.code == api.IS3D_EDOMAIN and e.value.bad_cell == 0 and "beyond the last node" in str(e.value)
    before = api.resource_counters()
    for kw in (dict(cells={k: v for k, v in cells.items() if k != "x"}), dict(bins=dict(bins, tau_bins=0)), dict(bins=dict(bins, r_max=bins["r_min"])),
               dict(opts=dict(dimension=3, kernel_variant=2)), dict(grid=dict(g, pT=np.linspace(0.1, 3, 65), pT_w=np.full(65, 0.1)))):
        a = dict(dict(cells=cells, grid=g, bins=bins, opts=dict(dimension=3)), **kw)
        with pytest.raises(api.Is3dError) as e:
            api.spacetime_distributions_vah(a["cells"], sp, a["grid"], a["bins"], a["opts"])
        assert e.value.code == api.IS3D_EINVAL, kw.keys()
    assert api.resource_counters() == before


def test_device_plan_entry_matches_the_one_shot(fx):
    import torch
    cells, ref = run(fx, 2)
    sp, g, bins = fx["pikp"], wgrid(fx), surface_bins(cells)
    n = len(cells["tau"])
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items()}
    shapes = api.spacetime_shapes(len(sp["mass"]), n, bins, 2, len(g["eta"]))
    outs = {k: torch.zeros(v, dtype=torch.float64, device=dev) for k, v in shapes.items()}
    for tab in (None, inputs.vah_df_tables()):
        plan = api.VahPlan(sp, fx["grid"], dict(dimension=2), tab=tab, max_cells=n)
        try:
            stream = torch.cuda.current_stream().cuda_stream
            ptrs = {k: v.data_ptr() for k, v in t.items() if k in api.VAH_FIELDS and not (tab is not None and k in COEF)}
            for _ in range(2):
                st = plan.execute_spacetime(n, ptrs, t["x"].data_ptr(), t["y"].data_ptr(), g["pT_w"], g["phi_w"], bins,
                                            {k: v.data_ptr() for k, v in outs.items()}, stream)
                torch.cuda.synchronize()
                if tab is None:
                    for k in api.SPACETIME_OUTPUTS:
                        assert np.array_equal(outs[k].cpu().numpy(), ref[k]), k
            assert st["ms_cells"] > 0.0 and st["n_classes"] == 3 and np.isfinite(outs["dN_dy"].cpu().numpy()).all()
            # the spectra of the same plan still run beside it
            spec = torch.zeros(plan.output_size, dtype=torch.float64, device=dev)
            plan.execute(n, ptrs, spec.data_ptr(), stream)
            torch.cuda.synchronize()
            assert np.isfinite(spec.cpu().numpy()).all()
            with pytest.raises(api.Is3dError) as e:
                plan.execute_spacetime(n, ptrs, 0, t["y"].data_ptr(), g["pT_w"], g["phi_w"], bins, {k: v.data_ptr() for k, v in outs.items()}, stream)
            assert e.value.code == api.IS3D_EINVAL
        finally:
            plan.close()


# ---- the command line tool (is3d_run.cpp): mode = 2, operation = 0, df_mode = 4 ----

CLI_IDS = [211, 321, 2212]


@pytest.mark.parametrize("dim", [3, 2])
def test_cli_mode2_operation_0(tmp_path, fx, dim):
    cells = synth.synth_vah_surface(19 if dim == 3 else 5, dim, seed=60 + dim)
    vh = synth.synth_surface(3, dim)            # make_run_dir wants a mode-1 surface to write first; it is replaced below
    root = refformat.make_run_dir(str(tmp_path / "run"), vh, CLI_IDS, dict(dimension=dim, df_mode=4, mode=2, operation=0))
    surf = os.path.join(root, "input", "surface.dat")
    synth.write_surface_vah_dat(surf, cells)
    tab = inputs.vah_df_tables()
    refformat.write_vah_df_tables(os.path.join(root, "deltaf_coefficients", "vah"), tab)
    r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "vahydro" in r.stdout and "Total number of freezeout cells: %d" % len(cells["tau"]) in r.stdout
    st_dir = os.path.join(root, "results", "spacetime_distribution")
    n_eta = 1 if dim == 3 else 241
    want_names = sorted(n for i in CLI_IDS for n in ("dN_taudtaudy_%d.dat" % i, "dN_twopirdrdy_%d.dat" % i, "dN_twopitaurdtaudrdy_%d.dat" % i,
                                                       "dN_dydeta_%d_%dpt.dat" % (i, n_eta)))
    assert sorted(os.listdir(st_dir)) == want_names
    # no momentum-spectra file
    assert not [f for f in os.listdir(os.path.join(root, "results")) if f.startswith("dN_pTdpTdphidy")]
    assert not any(f.startswith("dN_dy_") for f in os.listdir(os.path.join(root, "results", "dN_dy")))
    # the library result for the surface read back from the file, through the library's writer: the same text (the 7 digits the files carry)
    parsed = api.surface_read_vah(surf, dim)
    sp = inputs.species(CLI_IDS)
    res = api.spacetime_distributions_vah(parsed, sp, wgrid(fx), CLI_BINS, dict(dimension=dim), tab=tab)
    os.makedirs(str(tmp_path / "mine"))
    api.write_spacetime(str(tmp_path / "mine"), CLI_BINS, CLI_IDS, [parsed["eta"][-1]] if dim == 3 else wgrid(fx)["eta"], res)
    assert read_dir(str(tmp_path / "mine")) == read_dir(st_dir)
    assert np.all(res["dN_dy"] != 0.0) and r.stdout.count("dN_dy = ") == len(CLI_IDS)
    for ip in range(len(CLI_IDS)):
        assert ("dN_dy = %f" % res["dN_dy"][ip]) in r.stdout
    # a device list changes nothing: the first device computes alone
    for f in os.listdir(st_dir):
        os.remove(os.path.join(st_dir, f))
    r2 = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600, env=dict(os.environ, IS3D_DEVICES="0,0"))
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert read_dir(str(tmp_path / "mine")) == read_dir(st_dir)
    # mode = 2 with operation = 2 stays refused
    root2 = refformat.make_run_dir(str(tmp_path / "bad"), vh, CLI_IDS, dict(dimension=dim, df_mode=4, mode=2, operation=2))
    r3 = subprocess.run([api.CLI_PATH], cwd=root2, capture_output=True, text=True, timeout=600)
    assert r3.returncode != 0 and "stub" in r3.stderr
