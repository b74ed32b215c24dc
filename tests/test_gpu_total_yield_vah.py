"""GPU (-m gpu): is3d_total_yield_vah, the mean yield of an anisotropic-hydro surface, against its numpy restatement
(tests/vah_yield_ref.py, itself checked against the CPU oracle's smooth spectrum in tests/test_vah_yield_ref.py) on every path of the kernels
-- one thread, a part of a wave, more than a workgroup, several tiles per class, many classes, another node count -- and against what the
repository already holds: is3d_total_yield in the isotropic limit and the kept hadrons of is3d_sample_particles_vah, which it sizes.
Tolerances: 1e-11 relative against the restatement (the figure of test_total_yield_matches_the_oracle: two summation orders of <= 2e4 positive
terms and exp / sqrt / reciprocal at 1e-15), 1e-13 where only the order of a few additions differs."""
import numpy as np
import pytest

import vah_yield_ref as ref
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu
RTOL = 1.0e-11
COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]        # include_bulk_deltaf, include_shear_deltaf
Y_CUT = 0.8


@pytest.fixture(scope="module")
def sp():
    return inputs.species([211, 321, 2212, -2212])       # pi+, K+, p, pbar: 3 classes


@pytest.fixture(scope="module")
def gla():
    return inputs.feqmod_tables(0.15)


def surface(n, dim, seed):
    v = dict(synth.synth_vah_surface(n, dim, seed=seed))
    v["bulkPi"] = ref.BULK_SCALE * v["bulkPi"]           # so that the linear yields are positive
    return v


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def check(v, sp, gla, o, all_positive=True, **kw):
    want_N, want_by, want_skipped = ref.total_yield_vah_ref(v, sp, gla, o, y_cut=kw.get("y_cut", 0.5))
    N, by, st = api.total_yield_vah(v, sp, gla, o, **kw)
    print("n %d %s: yield %.15g restatement %.15g, by species %.3g, total %.3g relative" % (len(v["tau"]), o, N, want_N, rel(by, want_by), rel(N, want_N)))
    assert want_N > 0.0 and (np.all(want_by > 0.0) or not all_positive)
    assert rel(by, want_by) <= RTOL and rel(N, want_N) <= RTOL
    assert st["n_cells_skipped"] == want_skipped
    return N, by, st


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_matches_the_restatement(sp, gla, n, dim):
    v = surface(n, dim, 8100 + 10 * dim + n)
    for bulk, shear in COMBOS:
        _, _, st = check(v, sp, gla, dict(dimension=dim, include_bulk_deltaf=bulk, include_shear_deltaf=shear), y_cut=Y_CUT)
        assert st["n_classes"] == 3


@pytest.mark.parametrize("dim", [3, 2])
def test_the_full_species_list(fx, gla, dim):
    """305 species in 75 classes; species of one class with different degeneracies"""
    sp = fx["urqmd"]
    key = list(zip(sp["mass"], sp["sign"]))
    assert any(len({g for k, g in zip(key, sp["degeneracy"]) if k == k0}) > 1 for k0 in set(key))
    # (the linear yields of the resonances above ~1.5 GeV are negative even with bulkPi x 0.02 -- c0 m^2 Pi grows with m^2 -- and small: the
    # smallest magnitude is 1e-5 of the mean yield, no cancellation to the 1e-11 asked)
    _, by, st = check(surface(300, dim, 8200 + dim), sp, gla, dict(dimension=dim), all_positive=False, y_cut=Y_CUT)
    assert len(by) == 305 and st["n_classes"] == len(set(key)) == 75 and np.count_nonzero(by > 0.0) > 100


@pytest.mark.parametrize("dim", [3, 2])
def test_several_tiles_per_class_and_skipped_cells(sp, gla, dim):
    v = surface(20000, dim, 8300 + dim)
    v["dat"][::7] *= -1.0
    for bulk, shear in ((1, 1), (0, 0)):
        _, _, st = check(v, sp, gla, dict(dimension=dim, include_bulk_deltaf=bulk, include_shear_deltaf=shear), y_cut=Y_CUT)
        assert st["n_cells_skipped"] > 2000


def test_a_hand_made_five_node_rule(sp):
    rule = dict(root1=np.array([0.4, 1.3, 2.9, 5.5, 9.75]), weight1=np.array([0.31, 0.42, 0.2, 0.06, 0.004]))
    for dim in (3, 2):
        check(surface(257, dim, 8400 + dim), sp, rule, dict(dimension=dim), y_cut=Y_CUT)


def test_coefficients_from_the_tables(sp, gla):
    tab = inputs.vah_df_tables()
    v = surface(1000, 3, 8500)
    coef = api.vah_coefficients(tab, v["Lambda"], v["aL"])
    for bulk, shear in COMBOS:
        o = dict(dimension=3, include_bulk_deltaf=bulk, include_shear_deltaf=shear)
        N_tab, by_tab, _ = api.total_yield_vah(v, sp, gla, o, tab=tab)
        N_own, by_own, _ = api.total_yield_vah(dict(v, **{k: coef[k] for k in ("c0", "c1", "c2", "c3", "c4")}), sp, gla, o)
        assert rel(by_tab, by_own) <= 1.0e-13 and rel(N_tab, N_own) <= 1.0e-13
    want_N, want_by, _ = ref.total_yield_vah_ref(v, sp, gla, dict(dimension=3), coef=coef)
    assert rel(by_tab, want_by) <= RTOL and rel(N_tab, want_N) <= RTOL
    assert rel(by_tab, api.total_yield_vah(v, sp, gla, dict(dimension=3))[1]) > 1.0e-3      # the cells' own coefficients are others


@pytest.mark.parametrize("dim", [3, 2])
def test_isotropic_limit_is_the_viscous_yield(fx, sp, gla, dim):
    """alpha_L = 1, Lambda = T uniform, no residuals: is3d_total_yield with df_mode 1 and no bulk correction on the same geometry"""
    n = 1000
    v = dict(synth.synth_vah_surface(n, dim, seed=8600 + dim))
    v["dat"][::5] *= -1.0
    T = 0.152
    v.update(aL=np.ones(n), Lambda=np.full(n, T), T=np.full(n, T))
    for k in ("pitt", "pitx", "pity", "pitn", "pixx", "pixy", "pixn", "piyy", "piyn", "pinn", "Wx", "Wy", "bulkPi"):
        v[k] = np.zeros(n)
    z = np.zeros(n)
    c = {k: v[k] for k in ("tau", "eta", "ux", "uy", "un", "dat", "dax", "day", "dan", "T", "P", "E")}
    c.update(pixx=z, pixy=z, pixn=z, piyy=z, piyn=z, bulkPi=z)
    o = dict(dimension=dim, df_mode=1, include_bulk_deltaf=0)
    want, dens = api.total_yield(c, sp, fx["df"], inputs.feqmod_tables(T), (T, float(np.mean(v["E"])), float(np.mean(v["P"])), 0.0, 0.0), o, y_cut=Y_CUT)
    N, by, st = api.total_yield_vah(v, sp, gla, dict(dimension=dim), y_cut=Y_CUT)
    uds, _ = ref.lrf_dsigma(v)
    want_by = dens[0] * np.sum(uds[uds > 0.0]) * (2.0 * Y_CUT if dim == 2 else 1.0)
    print("yield %.15g viscous %.15g" % (N, want))
    assert want > 0.0 and st["n_cells_skipped"] == np.count_nonzero(uds <= 0.0) > 100
    assert rel(N, want) <= RTOL and rel(by, want_by) <= RTOL


def test_two_calls_give_the_same_bits_and_shards_add_up(sp, gla):
    tab = inputs.vah_df_tables()
    for dim in (3, 2):
        v = surface(20000, dim, 8700 + dim)
        o = dict(dimension=dim)
        N, by, _ = api.total_yield_vah(v, sp, gla, o, tab=tab, y_cut=Y_CUT)
        N2, by2, _ = api.total_yield_vah(v, sp, gla, o, tab=tab, y_cut=Y_CUT)
        assert N == N2 and np.array_equal(by, by2)
        cut = 9999
        a = api.total_yield_vah({k: x[:cut] for k, x in v.items()}, sp, gla, o, tab=tab, y_cut=Y_CUT)
        b = api.total_yield_vah({k: x[cut:] for k, x in v.items()}, sp, gla, o, tab=tab, y_cut=Y_CUT, first_cell=cut)
        assert rel(a[1] + b[1], by) <= 1.0e-13 and rel(a[0] + b[0], N) <= 1.0e-13


def test_bad_cells_are_named_and_the_others_summed(sp, gla):
    tab = inputs.vah_df_tables()
    n, first = 1500, 4000
    v = surface(n, 3, 8800)
    coef = api.vah_coefficients(tab, v["Lambda"], v["aL"])
    o = dict(dimension=3)

    def broken(changes):
        w = {k: x.copy() for k, x in v.items()}
        for field, cell, value in changes:
            w[field][cell] = value
        return w

    def rest(cells):
        keep = np.ones(n, dtype=bool)
        keep[list(cells)] = False
        sub = {k: x[keep] for k, x in v.items()}
        return ref.total_yield_vah_ref(sub, sp, gla, o, coef={k: coef[k][keep] for k in coef})

    cases = [([("Lambda", 40, 0.0)], True), ([("aL", 1217, np.nan)], True), ([("aL", 63, 2.5)], True),       # alpha_L beyond the last node (2.0)
             ([("Lambda", 1055, 0.0), ("aL", 12, np.nan)], True), ([("Lambda", 700, -0.1)], False), ([("aL", 1499, np.inf)], False)]
    for changes, with_tab in cases:
        cells = [c for _, c, _ in changes]
        with pytest.raises(api.Is3dError) as e:
            api.total_yield_vah(broken(changes), sp, gla, o, tab=tab if with_tab else None, first_cell=first)
        assert e.value.code == api.IS3D_EDOMAIN and e.value.bad_cell == first + min(cells), str(e.value)
        if with_tab:
            want_N, want_by, _ = rest(cells)
            assert rel(e.value.yield_by_species, want_by) <= RTOL and rel(e.value.mean_yield, want_N) <= RTOL
    # without the tables a cell off them is no bad cell
    w = broken([("aL", 63, 2.5)])
    check(w, sp, gla, o, first_cell=first)


@pytest.mark.parametrize("seed", [17, 20260018])
@pytest.mark.parametrize("dim", [3, 2])
def test_it_sizes_the_sampler(sp, gla, dim, seed):
    """On cells where p.dsigma > 0 for every momentum and with the residual corrections off, the sampler keeps a drawn hadron with probability
    w_visc <w_flux> = (1/2) u.dsigma / ds_max of a bound of 2 n_eq ds_max: the kept hadrons of a species are Poisson with mean EXACTLY n_events x
    yield_by_species (same nodes, same densities).  5 sigma at two seeds."""
    v = ref.outflow_free_cells(dim, 8900 + dim)
    o = dict(dimension=dim, include_bulk_deltaf=0, include_shear_deltaf=0)
    N, by, _ = api.total_yield_vah(v, sp, gla, o, y_cut=Y_CUT)
    n_events = int(np.ceil(5.0e4 / by.min()))
    assert n_events < 100000
    got, st = api.sample_particles_vah(v, sp, gla, o, n_events=n_events, seed=seed, y_cut=Y_CUT)
    assert st["n_cells_skipped"] == 0
    kept = np.bincount(got["species"], minlength=len(by))
    expected = n_events * by
    print("n_events %d kept %s expected %s deviation in sigma %s" % (n_events, kept, expected, (kept - expected) / np.sqrt(expected)))
    assert np.all(expected >= 5.0e4)
    assert np.all(np.abs(kept - expected) <= 5.0 * np.sqrt(expected))
