"""CPU: the hostile-surface table (tests/hostile_surfaces.py) -- that the oracle alone, on every case, gives references that
tests/test_gpu_hostile_surfaces.py's metrics can judge: enough live cells, spectra that are finite and non-zero nearly everywhere (a relative
error is asked of every bin), and, for the cases that are about the spread, per-cell yields that really are 2^60 apart.  The generator's
seeds were tuned here.  Nothing touches a GPU."""
import numpy as np
import pytest

import hostile_surfaces as H
from is3d_amd import inputs
from oracle import oracle
from test_gpu_spacetime import oracle_cells

DIMS = {c: ((3,) if c == "eta_heavy" else (3, 2)) for c in H.CASES}
CASE_DIMS = [(c, d) for c in H.CASES for d in DIMS[c]]


def test_the_table_is_what_the_docstring_says():
    assert 24 <= H.N_CELLS <= 64
    ids = H.species_ids()
    u = inputs.species("urqmd")
    assert ids[:4] == [211, 321, 2212, -2212] and H.species()["mass"][4] == u["mass"].max()
    g = H.grid("shipped")
    assert (len(g["pT"]), len(g["phi"]), len(g["y"])) == (32, 24, 21)
    g = H.grid("offtile")
    assert (len(g["phi"]), len(g["y"]), len(g["pT"])) == (20, 9, 5)
    for case, dim in CASE_DIMS:
        b, c = H.base(dim), H.surface(case, dim)
        for f in b:
            if f not in H.DS and not (f == "eta" and case == "spacelike" and dim == 3):   # (eta / 8 there: the module's docstring)
                assert np.array_equal(b[f], c[f]), (case, f)
    # powers of two: the mantissas of every component are the base surface's
    for case in ("binades",) + H.GIANTS:
        for dim in (3, 2):
            b, c = H.base(dim), H.surface(case, dim)
            for f in H.DS:
                assert np.array_equal(np.frexp(b[f])[0], np.frexp(c[f])[0]), (case, f)
            k = np.frexp(c["dat"])[1] - np.frexp(b["dat"])[1]
            if case == "binades":
                assert k.min() >= -H.BINADES and k.max() <= H.BINADES and k.max() - k.min() >= 60
            else:
                assert sorted(k)[-2:] == [0, H.GIANT_LOG2] and int(np.argmax(k)) == {"giant-first": 0, "giant-middle": H.N_CELLS // 2, "giant-last": H.N_CELLS - 1}[case]
    for k in H.UNIFORM_K:
        b = H.exact_base(3)
        c = H.uniform(b, k)
        assert np.array_equal(c["dat"], np.ldexp(b["dat"], k)) and np.array_equal(c["tau"], b["tau"])
    g3 = H.exact_grid(3)
    assert g3["pT"].max() <= 3.0 and np.abs(g3["y"]).max() + np.abs(H.exact_base(3)["eta"]).max() <= 3.0 and np.abs(H.exact_grid(2)["eta"]).max() <= 3.0


@pytest.mark.parametrize("case,dim", CASE_DIMS)
def test_enough_cells_are_live(case, dim):
    for vah in (False, True):
        lv = H.live(H.surface(case, dim, vah=vah))
        assert lv.mean() >= (0.25 if case == "inflow" else 0.5), (case, dim, lv.mean())
    if case == "inflow":
        c = H.surface(case, dim)
        lv = H.live(c)
        assert not lv[0::3].any() and lv[1::3].all() and lv[2::3].all()
        # the tilted third: p.dsigma < 0 over most of the grid (pions, the lightest and so the least one-sided species, at eta = y)
        g = H.grid("shipped")
        t = np.arange(1, H.N_CELLS, 3)
        mT = np.sqrt(0.13957 ** 2 + g["pT"] ** 2)
        pds = (mT[None, :, None] * c["dat"][t][:, None, None] + g["pT"][None, :, None] * (np.cos(g["phi"])[None, None, :] * c["dax"][t][:, None, None]
                                                                                          + np.sin(g["phi"])[None, None, :] * c["day"][t][:, None, None]))
        assert (pds < 0).mean() > 0.5


@pytest.mark.parametrize("gname", ["shipped", "offtile"])
@pytest.mark.parametrize("case,dim", CASE_DIMS)
def test_outflow_spectra_are_finite_and_non_zero(case, dim, gname):
    g = H.plain(H.grid(gname))
    if dim == 2 and gname == "shipped":
        g = dict(g, pT=g["pT"][::4], phi=g["phi"][::3])   # (the eta sum multiplies the oracle's work; the GPU test runs the same sub-grid)
    ref = oracle.dN_pTdpTdphidy(H.surface(case, dim), H.species(), g, inputs.df_tables(), dict(dimension=dim, df_mode=2))
    assert np.isfinite(ref).all()
    assert np.count_nonzero(ref) >= 0.9 * ref.size, (np.count_nonzero(ref), ref.size)


@pytest.mark.parametrize("case", ("binades",) + H.GIANTS)
@pytest.mark.parametrize("dim", [3, 2])
def test_per_cell_yields_span_2_to_the_60(case, dim):
    g = H.grid("offtile")
    c = H.surface(case, dim)
    pc = oracle_cells(c, range(H.N_CELLS), H.species(), g, inputs.df_tables(), dict(dimension=dim, df_mode=2))
    lv = H.live(c)
    assert (pc[:, lv] > 0).all() and not pc[:, ~lv].any()
    for s in range(pc.shape[0]):
        assert pc[s, lv].max() / pc[s, lv].min() >= 2.0 ** 60, (case, dim, s)
