"""GPU: operation 0 with the modified equilibrium (is3d_spacetime_distributions_feqmod, is3d_plan_execute_spacetime_feqmod) against the numpy
restatement of calculate_dN_dX_feqmod (tests/dndx_feqmod_ref.py), including the three places where that routine departs from the feqmod
spectra routine, and the bitwise contract of the binning."""
import numpy as np
import pytest

import dndx_feqmod_ref as ref
from is3d_amd import api, inputs, synth
from test_gpu_spacetime import binned, bins_of, contract, err_vs_max, live, surface_bins

pytestmark = pytest.mark.gpu

SPECIES = [211, 321, 2212, -2212, 3122, -3122, 3312, 111]


def wgrid(fx):
    g = fx["grid_w"]
    return dict(fx["grid"], pT_w=g["pT_w"], phi_w=g["phi_w"])


def fq_for(cells):
    return inputs.feqmod_tables(inputs.surface_average_T(cells))


def check_against_restatement(res, want, cells, bins, signed, dim, tol=1e-9):
    pc = want["per_cell"]
    if signed:
        assert err_vs_max(res["dN_dy_cell"], pc) < tol
    else:
        rel = np.abs(res["dN_dy_cell"] - pc) / np.maximum(np.abs(pc), 1e-300)
        assert float(np.max(rel)) < tol, float(np.max(rel))
    t, r, tr = binned(pc, cells, bins)
    for name, v in (("dN_taudtaudy", t), ("dN_twopirdrdy", r), ("dN_twopitaurdtaudrdy", tr), ("dN_dy", pc.sum(axis=1))):
        assert err_vs_max(res[name], v) < tol, name
    if dim == 3:
        assert err_vs_max(res["dN_dydeta"][:, 0], pc.sum(axis=1)) < tol
    else:
        assert err_vs_max(res["dN_dydeta"], want["eta"]) < tol
    st = res["stats"]
    it, ir = bins_of(cells, bins)
    lv = live(cells)
    assert st["n_tau_outside"] == int(np.sum(lv & ((it < 0) | (it >= bins["tau_bins"]))))
    assert st["n_r_outside"] == int(np.sum(lv & ((ir < 0) | (ir >= bins["r_bins"]))))
    assert st["n_tau_negative"] == int(np.sum(lv & (it < 0))) and st["n_r_negative"] == int(np.sum(lv & (ir < 0)))


CASES = [(3, 3, 0, {}), (3, 4, 0, {}), (2, 3, 0, {}), (2, 4, 0, {}),
         (3, 3, 0, dict(outflow=0, regulate_deltaf=0)), (3, 4, 0, dict(outflow=0, regulate_deltaf=0)),
         (2, 3, 0, dict(outflow=0, regulate_deltaf=0)), (2, 4, 0, dict(outflow=0, regulate_deltaf=0)),
         (3, 3, 1, {}), (2, 3, 1, {})]


@pytest.mark.parametrize("dim,df_mode,baryon,flags", CASES)
def test_parity_with_restatement(fx, dim, df_mode, baryon, flags):
    g = wgrid(fx)
    df = inputs.df_tables_full() if baryon else fx["df"]
    cells = synth.synth_surface(120 if dim == 3 else 30, dim, seed=700 + 10 * dim + df_mode + 100 * baryon, baryon=bool(baryon))
    cells = {k: (v.copy() if v is not None else None) for k, v in cells.items()}
    if df_mode == 3:
        cells["bulkPi"][::7] = -5.0 * cells["P"][::7]   # a few breakdown cells in every case
    sp = inputs.species(SPECIES)
    fq = fq_for(cells)
    o = dict(dimension=dim, df_mode=df_mode, include_baryon=baryon, include_baryondiff_deltaf=baryon, **flags)
    bins = surface_bins(cells)
    res = api.spacetime_distributions(cells, sp, g, df, bins, o, per_cell=True, fq=fq)
    want = ref.dndx(cells, sp, g, df, fq, o)
    check_against_restatement(res, want, cells, bins, flags.get("outflow", 1) == 0, dim)
    assert res["feqmod_stats"]["n_cells_breakdown"] == want["n_breakdown"]
    if df_mode == 3:
        assert want["n_breakdown"] > 0


def test_narrow_3d_cells_stay_on_feqmod(fx):
    """3+1D cells with detA < 0.01 (bulkPi -> -P, df_mode 4) among healthy ones: every row on feqmod (:1926-1934 commented out); the spectra
    path's contraction (narrow rows on the linear delta-f) is missed by far more than the tolerance."""
    g = wgrid(fx)
    cells = {k: (v.copy() if v is not None else None) for k, v in synth.synth_surface(40, 3, seed=321).items()}
    narrow = np.arange(0, 40, 4)
    for k in ("pixx", "pixy", "pixn", "piyy", "piyn"):
        cells[k][narrow] *= 0.05
    cells["bulkPi"][narrow] = -0.95 * cells["P"][narrow]
    y = fx["grid"]["y"]
    cells["eta"][narrow] = y[(np.arange(len(narrow)) * 2) % len(y)] + 1.0e-4
    sp = inputs.species("pikp")
    fq = fq_for(cells)
    o = dict(dimension=3, df_mode=4)
    bins = surface_bins(cells)
    res = api.spacetime_distributions(cells, sp, g, fx["df"], bins, o, per_cell=True, fq=fq)
    want = ref.dndx(cells, sp, g, fx["df"], fq, o)
    check_against_restatement(res, want, cells, bins, False, 3)
    spec, st = api.smooth_spectra({k: v[narrow] for k, v in cells.items() if v is not None}, sp, fx["grid"], fx["df"], o, fq=fq)
    assert st["n_cells_narrow"] > 0
    contracted = contract(spec, sp, g, 3)
    got = res["dN_dy_cell"][:, narrow].sum(axis=1)
    assert float(np.max(np.abs(got - contracted) / np.abs(contracted))) > 1e-6


def test_2d_eta_stretched_for_detA_above_one(fx):
    g = wgrid(fx)
    cells = {k: (v.copy() if v is not None else None) for k, v in synth.synth_surface(24, 2, seed=52).items()}
    big = np.arange(0, 24, 3)
    cells["bulkPi"][big] = np.abs(cells["bulkPi"][big]) + 0.05 * cells["P"][big]   # lambda > 0: detA > 1
    sp = inputs.species("pikp")
    fq = fq_for(cells)
    o = dict(dimension=2, df_mode=4)
    jon = ref.Jonah(fq)
    assert all(ref.cell_dndx(cells, c, sp, g, fx["df"], fq, o, jon)[4] >= 1.0 for c in big)
    bins = surface_bins(cells)
    res = api.spacetime_distributions(cells, sp, g, fx["df"], bins, o, per_cell=True, fq=fq)
    want = ref.dndx(cells, sp, g, fx["df"], fq, o)
    check_against_restatement(res, want, cells, bins, False, 2)
    spec, _ = api.smooth_spectra({k: v[big] for k, v in cells.items() if v is not None}, sp, fx["grid"], fx["df"], o, fq=fq)
    contracted = contract(spec, sp, g, 2)
    got = res["dN_dy_cell"][:, big].sum(axis=1)
    assert float(np.max(np.abs(got - contracted) / np.abs(contracted))) > 1e-6


@pytest.mark.parametrize("dim", [3, 2])
def test_breakdown_and_renorm_skip_cells(fx, dim):
    """df_mode 3: bulkPi = -5 P on every third cell (breakdown: the linearised delta-f), and two cells whose T_mod is ~2e-4 GeV: n_mod
    underflows, renorm / detA is inf for every class (:1881) -- they add 0, and every (cell, class) pair is counted."""
    g = wgrid(fx)
    cells = {k: (v.copy() if v is not None else None) for k, v in synth.synth_surface(60 if dim == 3 else 18, dim, seed=91 + dim).items()}
    cells["bulkPi"][::3] = -5.0 * cells["P"][::3]
    sk = [4, 11]
    from oracle import oracle
    for c in sk:
        co = oracle.df_coefficients(fx["df"], 2, float(cells["T"][c]))
        cells["bulkPi"][c] = -(cells["T"][c] - 1.9e-4) * co["betabulk"] / co["F"]   # m_pi0 / T_mod > 709.8: every exponential overflows
        if dim == 3:
            cells["eta"][c] = 0.0   # keeps E_mod / T_mod inside the kernel's exponent range (else IS3D_EDOMAIN, as on the spectra path)
    sp = inputs.species(SPECIES)
    fq = fq_for(cells)
    o = dict(dimension=dim, df_mode=3)
    bins = surface_bins(cells)
    res = api.spacetime_distributions(cells, sp, g, fx["df"], bins, o, per_cell=True, fq=fq)
    want = ref.dndx(cells, sp, g, fx["df"], fq, o)
    check_against_restatement(res, want, cells, bins, False, dim)
    fs = res["feqmod_stats"]
    assert fs["n_cells_breakdown"] == want["n_breakdown"] >= len(cells["tau"][::3])
    assert want["skipped"][sk].all() and not want["skipped"][np.setdiff1d(np.arange(len(cells["tau"])), sk)].any()
    assert fs["n_renorm_skipped"] == len(sk) * res["stats"]["n_classes"]
    assert np.all(res["dN_dy_cell"][:, sk] == 0.0)


def test_tie_to_the_spectra_path(fx):
    """No quirk cells: the sum over cells of dN_dy_cell is the contracted smooth_spectra(fq=) output."""
    g = wgrid(fx)
    for dim, dfm in ((3, 4), (3, 3), (2, 3)):
        cells = synth.synth_surface(300 if dim == 3 else 40, dim, seed=13 + dim + dfm)
        sp = inputs.species(SPECIES)
        fq = fq_for(cells)
        o = dict(dimension=dim, df_mode=dfm)
        jon = ref.Jonah(fq) if dfm == 4 else None
        keep = []
        for c in range(len(cells["tau"])):
            _, _, bd, skip, A = ref.cell_dndx(cells, c, inputs.species([211]), g, fx["df"], fq, o, jon)
            if not bd and not skip.any() and (A >= 0.01 if dim == 3 else A < 1.0):
                keep.append(c)
        assert len(keep) >= len(cells["tau"]) // 2
        cells = {k: v[keep] for k, v in cells.items() if v is not None}
        res = api.spacetime_distributions(cells, sp, g, fx["df"], surface_bins(cells), o, per_cell=True, fq=fq)
        spec, _ = api.smooth_spectra(cells, sp, fx["grid"], fx["df"], o, fq=fq)
        want = contract(spec, sp, g, dim)
        got = res["dN_dy_cell"].sum(axis=1)
        assert float(np.max(np.abs(got - want) / np.abs(want))) <= 1e-10, (dim, dfm)


@pytest.fixture(scope="module")
def big(fx):
    """1e5 cells x 305 species, 3+1D, df_mode 4, bins narrower than the surface"""
    cells = synth.synth_surface(100000, 3, seed=20260016)
    sp = inputs.species("urqmd")
    fq = fq_for(cells)
    o = dict(dimension=3, df_mode=4)
    bins = dict(tau_min=0.5, tau_max=6.0, tau_bins=40, r_min=0.0, r_max=8.0, r_bins=32)
    res = api.spacetime_distributions(cells, sp, wgrid(fx), fx["df"], bins, o, per_cell=True, fq=fq)
    return cells, sp, fq, o, bins, res


def test_full_size_binning_is_the_ordered_sum(fx, big):
    cells, sp, fq, o, bins, res = big
    pc = res["dN_dy_cell"]
    t, r, tr = binned(pc, cells, bins)
    assert np.array_equal(res["dN_taudtaudy"], t)
    assert np.array_equal(res["dN_twopirdrdy"], r)
    assert np.array_equal(res["dN_twopitaurdtaudrdy"], tr)
    assert np.array_equal(res["dN_dy"], np.cumsum(pc, axis=1)[:, -1])
    assert res["stats"]["n_tau_outside"] > 0
    again = api.spacetime_distributions(cells, sp, wgrid(fx), fx["df"], bins, o, per_cell=True, fq=fq)
    small = api.spacetime_distributions(cells, sp, wgrid(fx), fx["df"], bins, dict(o, workspace_bytes=96 << 20), per_cell=True, fq=fq)
    assert small["stats"]["n_passes"] > 1
    for k in api.SPACETIME_OUTPUTS:
        assert np.array_equal(again[k], res[k]), k
        assert np.array_equal(small[k], res[k]), k
    # about 50 stratified cells against the restatement
    idx = np.linspace(0, len(cells["tau"]) - 1, 50).astype(int)
    want = ref.dndx(cells, sp, wgrid(fx), fx["df"], fq, o, idx=idx)["per_cell"]
    rel = np.abs(pc[:, idx] - want) / np.maximum(np.abs(want), 1e-300)
    assert float(np.max(rel)) < 1e-9


def test_device_plan_entry_matches_the_one_shot(fx):
    import torch
    g = wgrid(fx)
    dev = torch.device("cuda:0")
    for dim, dfm in ((2, 4), (3, 3)):
        cells = {k: (v.copy() if v is not None else None) for k, v in synth.synth_surface(2000 if dim == 2 else 5000, dim, seed=77 + dim).items()}
        if dfm == 3:
            cells["bulkPi"][::5] = -5.0 * cells["P"][::5]
        cells = {k: v for k, v in cells.items() if v is not None}
        sp = inputs.species("pikp")
        fq = fq_for(cells)
        o = dict(dimension=dim, df_mode=dfm)
        bins = surface_bins(cells)
        ref1 = api.spacetime_distributions(cells, sp, g, fx["df"], bins, o, per_cell=True, fq=fq)
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items()}
        shapes = api.spacetime_shapes(len(sp["mass"]), len(cells["tau"]), bins, dim, len(g["eta"]))
        outs = {k: torch.zeros(v, dtype=torch.float64, device=dev) for k, v in shapes.items()}
        plan = api.Plan(sp, fx["grid"], fx["df"], o, max_cells=len(cells["tau"]), fq=fq)
        try:
            stream = torch.cuda.current_stream().cuda_stream
            for _ in range(2):
                st = plan.execute_spacetime(len(cells["tau"]), {k: v.data_ptr() for k, v in t.items()}, t["x"].data_ptr(), t["y"].data_ptr(),
                                            g["pT_w"], g["phi_w"], bins, {k: v.data_ptr() for k, v in outs.items()}, stream)
                torch.cuda.synchronize()
                for k in api.SPACETIME_OUTPUTS:
                    assert np.array_equal(outs[k].cpu().numpy(), ref1[k]), (dim, dfm, k)
            assert st["ms_cells"] > 0.0 and st["feqmod"]["n_cells_breakdown"] == ref1["feqmod_stats"]["n_cells_breakdown"]
        finally:
            plan.close()
