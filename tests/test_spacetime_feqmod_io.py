"""CPU: operation 0 with the modified equilibrium (is3d_spacetime_distributions_feqmod, calculate_dN_dX_feqmod) -- the argument checks, which
run before any device use, and the numpy restatement tests/dndx_feqmod_ref.py against the oracle's feqmod spectra where the two reference
routines coincide, and where they deliberately do not."""
import ctypes as C

import numpy as np
import pytest

import dndx_feqmod_ref as ref
from is3d_amd import api, inputs, synth
from oracle import oracle

BINS = dict(tau_min=0.5, tau_max=6.5, tau_bins=4, r_min=0.0, r_max=9.0, r_bins=3)


def wgrid(fx, **kw):
    return dict(fx["grid"], pT_w=fx["grid_w"]["pT_w"], phi_w=fx["grid_w"]["phi_w"], **kw)


def fq_for(cells):
    return inputs.feqmod_tables(inputs.surface_average_T(cells))


def contract(spec, sp, g, dim):
    S, npT, J = len(sp["mass"]), len(g["pT"]), len(g["phi"])
    ny = 1 if dim == 2 else len(g["y"])
    return np.einsum("kjps,p,j->s", spec.reshape(ny, J, npT, S), g["pT_w"], g["phi_w"])


def oracle_cell(cells, c, sp, g, df, fq, o):
    one = {k: (v[c:c + 1] if v is not None else None) for k, v in cells.items()}
    spec, _ = oracle.dN_pTdpTdphidy_feqmod(one, sp, g, df, fq, o)
    return contract(spec, sp, g, o["dimension"])


def test_argument_checks_precede_device_use(fx):
    """NULL fq, df_mode 1 / 2 on the feqmod entry, df_mode 4 with include_baryon, bad bins and NULL x or y are IS3D_EINVAL on a machine with
    or without a GPU."""
    cells = {k: v for k, v in synth.synth_surface(8, 3, seed=11).items() if k not in ("x", "y")}
    g = wgrid(fx)
    fq = fq_for(synth.synth_surface(8, 3, seed=11))
    xy = dict(x=np.linspace(0.0, 3.0, 8), y=np.zeros(8))
    cases = [(dict(df_mode=1), BINS, xy), (dict(df_mode=2), BINS, xy), (dict(df_mode=4, include_baryon=1), BINS, xy),
             (dict(df_mode=4), dict(BINS, tau_bins=0), xy), (dict(df_mode=3), dict(BINS, r_bins=0), xy),
             (dict(df_mode=4), dict(BINS, r_max=BINS["r_min"]), xy), (dict(df_mode=3), BINS, dict(x=None, y=xy["y"])),
             (dict(df_mode=4), BINS, dict(x=xy["x"], y=None))]
    sp = dict(fx["pikp"])
    for opts, bins, pos in cases:
        with pytest.raises(api.Is3dError) as e:
            api.spacetime_distributions(cells, sp, g, inputs.df_tables_full() if opts.get("include_baryon") else fx["df"], bins,
                                        dict(opts, dimension=3), x=pos["x"], y=pos["y"], fq=fq)
        assert e.value.code == api.IS3D_EINVAL, (opts, bins)
    with pytest.raises(api.Is3dError) as e:
        api.spacetime_distributions(cells, sp, g, fx["df"], BINS, dict(df_mode=4, include_baryon=1), fq=fq, **xy)
    assert "include_baryon" in str(e.value)
    # NULL feqmod tables
    L = api.load()
    rc = L.is3d_spacetime_distributions_feqmod(None, None, None, None, None, None, None, None, None, None, None, None, None, None)
    assert rc == api.IS3D_EINVAL and b"feqmod" in L.is3d_last_error()
    st, fst = api.SpacetimeStats(), api.SpacetimeFeqmodStats()
    rc = L.is3d_spacetime_distributions_feqmod(None, None, None, None, None, None, None, None, None, None, None, None, C.byref(st), C.byref(fst))
    assert rc == api.IS3D_EINVAL and st.code == api.IS3D_EINVAL and fst.first_cell_out_of_range == -1
    # the entry without fq still refuses df_mode 3 / 4 and names the routine and the new entry
    with pytest.raises(api.Is3dError) as e:
        api.spacetime_distributions(cells, sp, g, fx["df"], BINS, dict(df_mode=4), **xy)
    assert "calculate_dN_dX_feqmod" in str(e.value) and "is3d_spacetime_distributions_feqmod" in str(e.value)


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("df_mode", [3, 4])
@pytest.mark.parametrize("flags", [dict(), dict(outflow=0, regulate_deltaf=0)])
def test_restatement_matches_the_oracle_where_the_routines_coincide(fx, dim, df_mode, flags):
    """Healthy cells (no breakdown, 3+1D detA >= 0.01, 2+1D detA < 1): calculate_dN_dX_feqmod's dN_dy_cell is the spectra routine's output
    contracted with w_pT w_phi (and summed over y)."""
    cells = synth.synth_surface(12 if dim == 3 else 6, dim, seed=40 + dim + df_mode)
    sp = inputs.species([211, 321, 2212, -2212, 3122]) if dim == 3 else fx["pikp"]
    g = wgrid(fx)
    fq = fq_for(cells)
    o = dict(dimension=dim, df_mode=df_mode, **flags)
    jon = ref.Jonah(fq) if df_mode == 4 else None
    n_checked = 0
    for c in range(len(cells["tau"])):
        got, eta, bd, skip, A = ref.cell_dndx(cells, c, sp, g, fx["df"], fq, o, jon)
        if bd or skip.any() or (dim == 3 and A < 0.01) or (dim == 2 and A >= 1.0):
            continue
        want = oracle_cell(cells, c, sp, g, fx["df"], fq, o)
        scale = np.max(np.abs(want)) if flags else None
        err = np.abs(got - want) / (scale if scale else np.maximum(np.abs(want), 1e-300))
        assert float(np.max(err)) <= 1e-12, (c, float(np.max(err)))
        n_checked += 1
    assert n_checked >= 3


def test_restatement_differs_on_narrow_3d_cells(fx):
    """3+1D, detA < 0.01 (the recipe of test_gpu_feqmod.py::test_feqmod_narrow_rows): the spectra routine moves the rows |y - eta| < detA to
    the linearised delta-f, calculate_dN_dX_feqmod keeps every row on feqmod -- the restatement misses the oracle by far more than 1e-12."""
    cells = {k: (v.copy() if v is not None else None) for k, v in synth.synth_surface(4, 3, seed=321).items()}
    for k in ("pixx", "pixy", "pixn", "piyy", "piyn"):
        cells[k] *= 0.05
    cells["bulkPi"][:] = -0.95 * cells["P"]
    y = fx["grid"]["y"]
    cells["eta"][:] = y[(np.arange(4) * 2) % len(y)] + 1.0e-4
    sp, g = fx["pikp"], wgrid(fx)
    fq = fq_for(cells)
    o = dict(dimension=3, df_mode=4)
    jon = ref.Jonah(fq)
    for c in range(4):
        got, _, _, _, A = ref.cell_dndx(cells, c, sp, g, fx["df"], fq, o, jon)
        assert A < 0.01
        want = oracle_cell(cells, c, sp, g, fx["df"], fq, o)
        assert float(np.max(np.abs(got - want) / np.abs(want))) > 1e-6


def test_restatement_stretches_eta_for_detA_above_one_in_2d(fx):
    """2+1D, detA >= 1: calculate_dN_dX_feqmod scales the eta nodes by detA (:1847-1849), the spectra routine does not (:727-728); the
    restatement equals the oracle run on the eta nodes multiplied by detA, with the weights unchanged."""
    cells = {k: (v.copy() if v is not None else None) for k, v in synth.synth_surface(6, 2, seed=52).items()}
    cells["bulkPi"][:] = np.abs(cells["bulkPi"]) + 0.05 * cells["P"]      # lambda > 0: detA > 1
    sp, g = fx["pikp"], wgrid(fx)
    fq = fq_for(cells)
    o = dict(dimension=2, df_mode=4)
    jon = ref.Jonah(fq)
    for c in range(6):
        got, _, _, _, A = ref.cell_dndx(cells, c, sp, g, fx["df"], fq, o, jon)
        assert A >= 1.0
        plain = oracle_cell(cells, c, sp, g, fx["df"], fq, o)
        stretched = oracle_cell(cells, c, sp, dict(g, eta=g["eta"] * A), fx["df"], fq, o)
        assert float(np.max(np.abs(got - stretched) / np.abs(stretched))) <= 1e-12
        assert float(np.max(np.abs(got - plain) / np.abs(plain))) > 1e-6
