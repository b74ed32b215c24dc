"""GPU: operation 0 (is3d_spacetime_distributions, is3d_plan_execute_spacetime) -- the smooth spacetime distributions of calculate_dN_dX
(emissionfunction_smooth_kernels.cpp:1000-1446).  The oracle is used unmodified: dN_dy_cell of a set of cells is the oracle's spectrum of
those cells contracted with w_pT w_phi and summed over y (:1370)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refformat
from conftest import ROOT
from is3d_amd import api, inputs, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

SPECIES = [211, 321, 2212, -2212, 3122, -3122, 3312, 111]


def wgrid(fx):
    g = fx["grid_w"]
    return dict(fx["grid"], pT_w=g["pT_w"], phi_w=g["phi_w"])


def contract(spec, sp, g, dim):
    """[S] of sum_pT sum_phi sum_y w_pT w_phi spec (the 3+1D y sum without weights, quirk 1)."""
    S, npT, J = len(sp["mass"]), len(g["pT"]), len(g["phi"])
    ny = 1 if dim == 2 else len(g["y"])
    a = spec.reshape(ny, J, npT, S)
    return np.einsum("kjps,p,j->s", a, g["pT_w"], g["phi_w"])


def oracle_cells(cells, idx, sp, g, df, o):
    """[S][len(idx)]: the oracle's dN_dy_cell of every listed cell."""
    out = np.zeros((len(sp["mass"]), len(idx)))
    for i, c in enumerate(idx):
        one = {k: v[c:c + 1] for k, v in cells.items()}
        out[:, i] = contract(oracle.dN_pTdpTdphidy(one, sp, g, df, o), sp, g, o["dimension"])
    return out


def bins_of(cells, bins):
    tw = (bins["tau_max"] - bins["tau_min"]) / bins["tau_bins"]
    rw = (bins["r_max"] - bins["r_min"]) / bins["r_bins"]
    it = np.floor((cells["tau"] - bins["tau_min"]) / tw)
    ir = np.floor((np.sqrt(cells["x"] ** 2 + cells["y"] ** 2) - bins["r_min"]) / rw)
    return it, ir


def binned(per_cell, cells, bins):
    """the histograms as sums of per_cell [S][n] over each bin's cells in ascending order"""
    it, ir = bins_of(cells, bins)
    tb, rb = bins["tau_bins"], bins["r_bins"]
    S = per_cell.shape[0]
    t, r, tr = np.zeros((S, tb)), np.zeros((S, rb)), np.zeros((S, tb, rb))
    for b in range(tb):
        m = it == b
        if m.any():
            t[:, b] = np.cumsum(per_cell[:, m], axis=1)[:, -1]
    for b in range(rb):
        m = ir == b
        if m.any():
            r[:, b] = np.cumsum(per_cell[:, m], axis=1)[:, -1]
    for a in range(tb):
        for b in range(rb):
            m = (it == a) & (ir == b)
            if m.any():
                tr[:, a, b] = np.cumsum(per_cell[:, m], axis=1)[:, -1]
    return t, r, tr


def live(cells):
    """u.dsigma > 0: the cells the reference bins (:1160-1170; its skip test precedes the binning and the negative-index messages)"""
    ut = np.sqrt(1.0 + cells["ux"] * cells["ux"] + cells["uy"] * cells["uy"] + (cells["tau"] * cells["tau"]) * cells["un"] * cells["un"])
    return ut * cells["dat"] + cells["ux"] * cells["dax"] + cells["uy"] * cells["day"] + cells["un"] * cells["dan"] > 0.0


def err_vs_max(got, ref):
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


def surface_bins(cells):
    r = np.sqrt(cells["x"] ** 2 + cells["y"] ** 2)
    return dict(tau_min=float(cells["tau"].min()) - 0.01, tau_max=float(cells["tau"].max()) * 0.9, tau_bins=7, r_min=0.0,
                r_max=float(r.max()) * 0.8, r_bins=5)


CASES = [(3, 1, 0, {}), (3, 2, 0, {}), (2, 1, 0, {}), (2, 2, 0, {}), (3, 1, 1, {}), (3, 2, 1, {}), (2, 1, 1, {}), (2, 2, 1, {}),
         (3, 2, 0, dict(outflow=0, regulate_deltaf=0)), (2, 1, 0, dict(outflow=0, regulate_deltaf=0)),
         (3, 1, 1, dict(outflow=0, regulate_deltaf=0))]


@pytest.mark.parametrize("dim,df_mode,baryon,flags", CASES)
def test_parity_with_oracle(fx, dim, df_mode, baryon, flags):
    g = wgrid(fx)
    df = inputs.df_tables_full() if baryon else fx["df"]
    cells = synth.synth_surface(200 if dim == 3 else 50, dim, seed=300 + 10 * dim + df_mode, baryon=bool(baryon))
    sp = inputs.species(SPECIES)
    o = dict(dimension=dim, df_mode=df_mode, include_baryon=baryon, include_baryondiff_deltaf=baryon, **flags)
    bins = surface_bins(cells)
    res = api.spacetime_distributions(cells, sp, g, df, bins, o, per_cell=True)
    n = len(cells["tau"])
    ref_cell = oracle_cells(cells, range(n), sp, g, df, o)
    signed = flags.get("outflow", 1) == 0
    tol = 1e-10
    if signed:   # terms of both signs: the error against the largest value of the array
        assert err_vs_max(res["dN_dy_cell"], ref_cell) < tol
    else:
        rel = np.abs(res["dN_dy_cell"] - ref_cell) / np.maximum(np.abs(ref_cell), 1e-300)
        assert float(np.max(rel)) < tol
    t, r, tr = binned(ref_cell, cells, bins)
    for name, ref in (("dN_taudtaudy", t), ("dN_twopirdrdy", r), ("dN_twopitaurdtaudrdy", tr), ("dN_dy", ref_cell.sum(axis=1))):
        assert err_vs_max(res[name], ref) < tol, name
    if dim == 3:
        assert res["dN_dydeta"].shape == (len(SPECIES), 1)
        assert err_vs_max(res["dN_dydeta"][:, 0], ref_cell.sum(axis=1)) < tol
    else:
        # one-point eta grids [eta_k], [w_k]: the oracle's spectrum divided by w_k (:1365)
        ks = [0, 60, 120, 180, 240]
        for k in ks:
            g1 = dict(g, eta=g["eta"][k:k + 1], eta_w=g["eta_w"][k:k + 1])
            ref = contract(oracle.dN_pTdpTdphidy(cells, sp, g1, df, o), sp, g1, 2) / g["eta_w"][k]
            assert err_vs_max(res["dN_dydeta"][:, k], ref) < tol, k
        assert err_vs_max(res["dN_dydeta"] @ g["eta_w"], ref_cell.sum(axis=1)) < tol
    st = res["stats"]
    it, ir = bins_of(cells, bins)
    lv = live(cells)
    assert st["n_tau_outside"] == int(np.sum(lv & ((it < 0) | (it >= bins["tau_bins"]))))
    assert st["n_r_outside"] == int(np.sum(lv & ((ir < 0) | (ir >= bins["r_bins"]))))


@pytest.fixture(scope="module")
def big(fx):
    """1e5 cells x 305 species, 3+1D Chapman-Enskog, bins narrower than the surface"""
    cells = synth.synth_surface(100000, 3, seed=20260002)
    sp = inputs.species("urqmd")
    o = dict(dimension=3, df_mode=2)
    bins = dict(tau_min=0.5, tau_max=6.0, tau_bins=40, r_min=0.0, r_max=8.0, r_bins=32)
    res = api.spacetime_distributions(cells, sp, wgrid(fx), fx["df"], bins, o, per_cell=True)
    return cells, sp, o, bins, res


def test_full_size_binning_is_the_ordered_sum(fx, big):
    cells, sp, o, bins, res = big
    pc = res["dN_dy_cell"]
    t, r, tr = binned(pc, cells, bins)
    assert np.array_equal(res["dN_taudtaudy"], t)
    assert np.array_equal(res["dN_twopirdrdy"], r)
    assert np.array_equal(res["dN_twopitaurdtaudrdy"], tr)
    assert np.array_equal(res["dN_dy"], np.cumsum(pc, axis=1)[:, -1])
    it, ir = bins_of(cells, bins)
    st = res["stats"]
    lv = live(cells)
    assert st["n_tau_outside"] == int(np.sum(lv & ((it < 0) | (it >= bins["tau_bins"])))) > 0
    assert st["n_r_outside"] == int(np.sum(lv & ((ir < 0) | (ir >= bins["r_bins"]))))
    assert st["n_tau_negative"] == int(np.sum(lv & (it < 0))) and st["n_r_negative"] == int(np.sum(lv & (ir < 0)))
    again = api.spacetime_distributions(cells, sp, wgrid(fx), fx["df"], bins, o, per_cell=True)
    for k in api.SPACETIME_OUTPUTS:
        assert np.array_equal(again[k], res[k]), k
    # 300 stratified cells against the oracle
    idx = np.linspace(0, len(cells["tau"]) - 1, 300).astype(int)
    ref = oracle_cells(cells, idx, sp, wgrid(fx), fx["df"], o)
    rel = np.abs(pc[:, idx] - ref) / np.maximum(np.abs(ref), 1e-300)
    assert float(np.max(rel)) < 1e-10


def test_tie_to_the_spectra_path(fx, big):
    cells, sp, o, bins, res = big
    g = wgrid(fx)
    spec, _ = api.smooth_spectra(cells, sp, fx["grid"], fx["df"], o)
    ref = contract(spec, sp, g, 3)
    got = res["dN_dy_cell"].sum(axis=1)
    assert float(np.max(np.abs(got - ref) / np.abs(ref))) < 1e-12


def test_device_plan_entry_matches_the_one_shot(fx):
    import torch
    cells = synth.synth_surface(3000, 2, seed=77)
    sp = inputs.species("pikp")
    g = wgrid(fx)
    o = dict(dimension=2, df_mode=1)
    bins = surface_bins(cells)
    ref = api.spacetime_distributions(cells, sp, g, fx["df"], bins, o, per_cell=True)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items()}
    shapes = api.spacetime_shapes(len(sp["mass"]), len(cells["tau"]), bins, 2, len(g["eta"]))
    outs = {k: torch.zeros(v, dtype=torch.float64, device=dev) for k, v in shapes.items()}
    plan = api.Plan(sp, fx["grid"], fx["df"], o, max_cells=len(cells["tau"]))
    try:
        stream = torch.cuda.current_stream().cuda_stream
        for _ in range(2):
            st = plan.execute_spacetime(len(cells["tau"]), {k: v.data_ptr() for k, v in t.items()}, t["x"].data_ptr(), t["y"].data_ptr(),
                                        g["pT_w"], g["phi_w"], bins, {k: v.data_ptr() for k, v in outs.items()}, stream)
            torch.cuda.synchronize()
            for k in api.SPACETIME_OUTPUTS:
                assert np.array_equal(outs[k].cpu().numpy(), ref[k]), k
        assert st["ms_cells"] > 0.0 and st["n_classes"] == 3
        with pytest.raises(api.Is3dError) as e:
            plan.execute_spacetime(len(cells["tau"]), {k: v.data_ptr() for k, v in t.items()}, 0, t["y"].data_ptr(), g["pT_w"], g["phi_w"],
                                   bins, {k: v.data_ptr() for k, v in outs.items()}, stream)
        assert e.value.code == api.IS3D_EINVAL
    finally:
        plan.close()


def test_skipped_cells_and_table_edges(fx):
    g = wgrid(fx)
    sp = inputs.species("pikp")
    cells = synth.synth_surface(64, 3, seed=91)
    skip = [3, 17, 40]
    for c in skip:   # u.dsigma <= 0 (:1170)
        cells["dat"][c] = -abs(cells["dat"][c]) - 10.0
        cells["dax"][c] = cells["day"][c] = cells["dan"][c] = 0.0
    bins = surface_bins(cells)
    cells["tau"][skip] = 10.0 * bins["tau_max"]   # outside the tau bins: counted by no histogram count, as in the reference
    res = api.spacetime_distributions(cells, sp, g, fx["df"], bins, dict(dimension=3, df_mode=1), per_cell=True)
    ut = np.sqrt(1.0 + cells["ux"] ** 2 + cells["uy"] ** 2 + cells["tau"] ** 2 * cells["un"] ** 2)
    uds = ut * cells["dat"] + cells["ux"] * cells["dax"] + cells["uy"] * cells["day"] + cells["un"] * cells["dan"]
    assert res["stats"]["n_cells_skipped"] == int(np.sum(uds <= 0.0)) >= len(skip)
    it, ir = bins_of(cells, bins)
    out_t = (it < 0) | (it >= bins["tau_bins"])
    assert res["stats"]["n_tau_outside"] == int(np.sum(out_t & (uds > 0.0))) <= int(np.sum(out_t)) - len(skip)   # skipped cells are not counted
    assert np.all(res["dN_dy_cell"][:, uds <= 0.0] == 0.0)
    assert np.all(res["dN_dy_cell"][:, uds > 0.0] > 0.0)
    cells["T"][9] = 5.0   # outside the coefficient table
    with pytest.raises(api.Is3dError) as e:
        api.spacetime_distributions(cells, sp, g, fx["df"], bins, dict(dimension=3, df_mode=1))
    assert e.value.code == api.IS3D_EDOMAIN


# ---- the command line tool and the embedding entry (is3d_run.cpp, include/iS3D_amd.hpp) ----

CLI_BINS = dict(tau_min=0.0, tau_max=12.0, tau_bins=12, r_min=0.0, r_max=10.0, r_bins=10)   # refformat.PARAMS_TEMPLATE
CLI_IDS = [211, 321, 2212, -2212, 3122]


def read_dir(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("dim,df_mode,baryon", [(3, 1, 0), (3, 2, 1), (2, 1, 0), (2, 2, 1)])
def test_cli_operation_0(tmp_path, fx, dim, df_mode, baryon):
    cells = synth.synth_surface(60 if dim == 3 else 20, dim, seed=500 + 10 * dim + df_mode, baryon=bool(baryon))
    o = dict(dimension=dim, df_mode=df_mode, include_baryon=baryon, include_baryondiff_deltaf=baryon)
    root = refformat.make_run_dir(str(tmp_path / "run"), cells, CLI_IDS, dict(o, operation=0))
    r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    st_dir = os.path.join(root, "results", "spacetime_distribution")
    n_eta = 1 if dim == 3 else 241
    want_names = sorted(n for i in CLI_IDS for n in ("dN_taudtaudy_%d.dat" % i, "dN_twopirdrdy_%d.dat" % i, "dN_twopitaurdtaudrdy_%d.dat" % i,
                                                       "dN_dydeta_%d_%dpt.dat" % (i, n_eta)))
    assert sorted(os.listdir(st_dir)) == want_names
    # no momentum-spectra file (written for operation = 1 only, emissionfunction.cpp:1678)
    assert not os.path.exists(os.path.join(root, "results", "dN_pTdpTdphidy.dat"))
    assert not any(f.startswith("dN_dy_") for f in os.listdir(os.path.join(root, "results", "dN_dy")))
    assert os.path.exists(os.path.join(root, "average_thermodynamic_quantities.dat"))
    # the same doubles the tool saw: the library's own reader
    parsed, _, _ = api.surface_open(os.path.join(root, "input", "surface.dat"), 1, baryon, baryon, dim, cache=0)
    parsed = {k: v for k, v in parsed.items() if v is not None}
    df = inputs.df_tables_full() if baryon else fx["df"]
    sp = inputs.species(CLI_IDS)
    res = api.spacetime_distributions(parsed, sp, wgrid(fx), df, CLI_BINS, o, per_cell=True)
    eta_vals = [parsed["eta"][-1]] if dim == 3 else wgrid(fx)["eta"]
    os.makedirs(str(tmp_path / "mine"))
    api.write_spacetime(str(tmp_path / "mine"), CLI_BINS, CLI_IDS, eta_vals, res)
    assert read_dir(str(tmp_path / "mine")) == read_dir(st_dir)
    for ip, mc in enumerate(CLI_IDS):
        assert ("dN_dy = %f" % res["dN_dy"][ip]) in r.stdout
    # the printed values against the oracle (6 printed digits)
    ref_cell = oracle_cells(parsed, range(len(parsed["tau"])), sp, wgrid(fx), df, o)
    t, rr, tr = binned(ref_cell, parsed, CLI_BINS)
    tw = (CLI_BINS["tau_max"] - CLI_BINS["tau_min"]) / CLI_BINS["tau_bins"]
    rw = (CLI_BINS["r_max"] - CLI_BINS["r_min"]) / CLI_BINS["r_bins"]
    for ip, mc in enumerate(CLI_IDS):
        got = np.loadtxt(os.path.join(st_dir, "dN_taudtaudy_%d.dat" % mc))
        tau_mid = CLI_BINS["tau_min"] + tw * (np.arange(12) + 0.5)
        assert np.allclose(got[:, 1], t[ip] / (tau_mid * tw), rtol=2e-6, atol=1e-300)
        got = np.loadtxt(os.path.join(st_dir, "dN_twopirdrdy_%d.dat" % mc))
        r_mid = CLI_BINS["r_min"] + rw * (np.arange(10) + 0.5)
        assert np.allclose(got[:, 1], rr[ip] / (2 * np.pi * r_mid * rw), rtol=2e-6, atol=1e-300)
        got = np.loadtxt(os.path.join(st_dir, "dN_twopitaurdtaudrdy_%d.dat" % mc)).reshape(10, 12, 3)   # r outer, tau inner
        assert np.allclose(got[:, :, 2], tr[ip].T / (2 * np.pi * np.outer(r_mid, tau_mid) * tw * rw), rtol=2e-6, atol=1e-300)


@pytest.mark.parametrize("params", [dict(df_mode=3), dict(df_mode=4), dict(mode=2, df_mode=4), dict(mode=2, df_mode=1)])
def test_cli_operation_0_refusals(tmp_path, params):
    cells = synth.synth_surface(8, 3, seed=7)
    root = refformat.make_run_dir(str(tmp_path), cells, [211], dict(dict(operation=0, dimension=3), **params))
    r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "iS3D-amd:" in r.stderr
    if params.get("mode") != 2:
        assert "calculate_dN_dX_feqmod" in r.stderr
    assert os.listdir(os.path.join(root, "results", "spacetime_distribution")) == []


def test_embedding_operation_0(tmp_path, fx, monkeypatch):
    ids = [211, 321, 2212, -2212]
    n = 500
    cells = synth.synth_surface(n, 3, seed=96)
    root = refformat.make_run_dir(str(tmp_path / "run"), synth.synth_surface(2, 3, seed=1), ids, dict(operation=0, dimension=3, df_mode=2))
    os.remove(os.path.join(root, "input", "surface.dat"))          # the in-memory path must not need it
    exe = str(tmp_path / "embed_main")
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "embed_main.cpp"), "-o", exe,
                           "-L", os.path.dirname(api.LIB_PATH), "-lis3d_amd", "-Wl,-rpath," + os.path.dirname(api.LIB_PATH)])
    cols = ["tau", "x", "y", "eta", "dat", "dax", "day", "dan", "E", "T", "P", "ux", "uy", "un", "pixx", "pixy", "pixn", "piyy", "piyn", None, "bulkPi"]
    tab = np.stack([cells[c] if c else np.full(n, 7.0) for c in cols], axis=1)
    np.savetxt(str(tmp_path / "surf21.txt"), tab, fmt="%.17g")
    r = subprocess.run([exe, str(tmp_path / "surf21.txt")], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "Reading in freezeout surface from memory" in r.stdout and "EVENTS 0 SPECTRUM 0" in r.stdout
    res = api.spacetime_distributions(cells, inputs.species(ids), wgrid(fx), fx["df"], CLI_BINS, dict(dimension=3, df_mode=2))
    os.makedirs(str(tmp_path / "mine"))
    api.write_spacetime(str(tmp_path / "mine"), CLI_BINS, ids, [cells["eta"][-1]], res)
    st_dir = os.path.join(root, "results", "spacetime_distribution")
    assert read_dir(str(tmp_path / "mine")) == read_dir(st_dir) and len(os.listdir(st_dir)) == 16
    # NULL x / y on the embedding entry: IS3D_EINVAL before anything is written
    for f in os.listdir(st_dir):
        os.remove(os.path.join(st_dir, f))
    L = api.load()
    L.is3d_run_particlization.argtypes = [C.POINTER(api.Cells), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    cs = api.Cells()
    cs.n_cells = n
    held = {k: np.ascontiguousarray(cells[k]) for k in api.CELL_FIELDS if k in cells}
    for k, v in held.items():
        setattr(cs, k, v.ctypes.data)
    monkeypatch.chdir(root)
    for xp, yp in ((None, held["tau"].ctypes.data), (held["tau"].ctypes.data, None)):
        assert L.is3d_run_particlization(C.byref(cs), xp, yp, 0, None) == api.IS3D_EINVAL
    assert os.listdir(st_dir) == []
