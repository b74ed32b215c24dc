"""GPU (-m gpu): the anisotropic-hydro sampler with its hadrons binned where they are sampled, in one pass and without a list
(is3d_sample_binned_vah, is3d_sample_binned_vah_multi; cf_sampler_fused with the anisotropic-hydro model).  The reference has no VAH sampler, so the yardstick is the
library's own list route: the histograms must be those of is3d_sampler_bin_list on the list is3d_sample_particles_vah returns for the same
arguments.  Every comparison is between integers; the one tolerance is the project's rule for vn_re / vn_im against a HOST-binned list (one
fixed-point unit per entry of the dN_pT bin: device and host libm differ).

Shapes: synth.synth_vah_surface with bulkPi * 0.02 (tests/test_gpu_sampler_vah.py: delta-f stays on for every species, the clamp is reached in
the tails only), the volumes scaled so that the closed-form bound sum_cells dn_tot (mean_drawn_per_event there, restated here) gives 2.5e4
drawn hadrons per call; every test asserts sum(yield) >= 2000 and that each of the five count arrays is non-zero."""
import numpy as np
import pytest

import sampler_bins_ref as R
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu
HBARC = synth.HBARC
COUNTS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r")
ALL = COUNTS + ("yield", "vn_re", "vn_im")
TALLIES = ("n_momentum_samples", "n_acceptances", "n_hadrons_drawn", "n_cells_skipped")
BULK_SCALE = 0.02
DRAWN = 2.5e4          # hadrons drawn per call by the closed-form bound (>= 2e4)
PIKP = [211, 321, 2212, -2212]           # pi+ K+ p pbar

# bins that leave hadrons OUTSIDE every range: the surfaces have tau in [1, 10], r in [0, 8], eta in [-4, 4] (3+1D)
BINS3 = dict(y_cut=2.1, y_bins=14, eta_cut=3.0, eta_bins=20, pT_lower_cut=0.1, pT_upper_cut=1.0, pT_bins=10, tau_min=2.5, tau_max=8.5, tau_bins=6,
             r_min=1.0, r_max=6.0, r_bins=5)
# 2+1D: the sampler draws |y| <= Y_CUT2 = 0.7, the bins end at 0.49; eta follows the sampled rapidity
BINS2 = dict(BINS3, y_cut=0.49, eta_cut=0.4)
# one cell: every hadron has the cell's tau and r, so those two ranges hold the whole surface and only the rapidity gate thins them
BINS2_ONE = dict(BINS2, tau_min=0.5, tau_max=10.5, r_min=0.0, r_max=9.0)
SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)             # iS3D_parameters.dat as shipped
Y_CUT2 = 0.7


# ---- the closed-form bound, restated from tests/test_gpu_sampler_vah.py ----
def neq_gauss_thermal(gla, mbar, sign):
    r, w = np.asarray(gla["root1"]), np.asarray(gla["weight1"])
    Ebar = np.sqrt(r[None, :] ** 2 + np.asarray(mbar)[:, None] ** 2)
    return np.sum(w[None, :] * r[None, :] * np.exp(r[None, :]) / (np.exp(Ebar) + sign), axis=1)


def lrf_dsigma(v):
    tau2 = v["tau"] ** 2
    ut = np.sqrt(1.0 + v["ux"] ** 2 + v["uy"] ** 2 + tau2 * v["un"] ** 2)
    uds = ut * v["dat"] + v["ux"] * v["dax"] + v["uy"] * v["day"] + v["un"] * v["dan"]
    ds2 = v["dat"] ** 2 - v["dax"] ** 2 - v["day"] ** 2 - v["dan"] ** 2 / tau2
    return uds, np.sqrt(np.maximum(uds * uds - ds2, 0.0))


def mean_drawn_per_event(v, sp, gla, y_max):
    """sum over the cells with u.dsigma > 0 of dn_tot = (sum_s dn_s) 2 y_max ds_max"""
    uds, dsp = lrf_dsigma(v)
    ds_max = np.abs(uds) + dsp
    dn = np.zeros_like(uds)
    for m, s, g in zip(sp["mass"], sp["sign"], sp["degeneracy"]):
        dn += 2.0 * v["aL"] * g * v["Lambda"] ** 3 / (2.0 * np.pi ** 2 * HBARC ** 3) * neq_gauss_thermal(gla, m / v["Lambda"], s)
    return float(np.sum(np.where(uds > 0.0, dn * 2.0 * y_max * ds_max, 0.0)))


def surface(n, dim, seed, sp, gla, n_events, backflow=False):
    """n synthetic VAH cells with bulkPi * 0.02, every 7th cell turned to u.dsigma <= 0 when asked, and the volumes scaled to DRAWN hadrons per
    call of n_events events by the closed-form bound"""
    v = {k: np.array(a, dtype=np.float64) for k, a in synth.synth_vah_surface(n, dim, seed=seed).items()}
    v["bulkPi"] = BULK_SCALE * v["bulkPi"]
    if backflow:
        for f in ("dat", "dax", "day", "dan"):
            v[f][3::7] = -v[f][3::7]
    y_max = Y_CUT2 if dim == 2 else 0.5
    scale = DRAWN / (n_events * mean_drawn_per_event(v, sp, gla, y_max))
    for f in ("dat", "dax", "day", "dan"):
        v[f] = scale * v[f]
    assert n_events * mean_drawn_per_event(v, sp, gla, y_max) >= 2.0e4
    return {k: np.ascontiguousarray(a) for k, a in v.items()}


def same(a, b, keys=ALL):
    return all(a[k].dtype == np.int64 and np.array_equal(a[k], b[k]) for k in keys)


def filled(h):
    """no empty comparison: at least 2000 hadrons, every count array non-zero"""
    return h["yield"].sum() >= 2000 and all(h[k].sum() > 0 for k in COUNTS)


@pytest.fixture(scope="module")
def gla():
    return inputs.feqmod_tables(0.15)


@pytest.fixture(scope="module")
def tab():
    return inputs.vah_df_tables()


@pytest.fixture(scope="module")
def species():
    return dict(pikp=inputs.species(PIKP), urqmd=inputs.species("urqmd"))


# ---- 1. equals the list route ----
# name: dimension, species, kernel_form, cells, events, coefficients from the tables, bins.  63 cells x 3 events: several events share a wave;
# 257 and 1000 cells: more than one workgroup, events change inside a wave, some cells with u.dsigma <= 0.
CASES = {
    "3d-pikp-global-63c-3e-tab": (3, "pikp", 1, 63, 3, True, BINS3),
    "3d-pikp-private-257c-8e-cells": (3, "pikp", 2, 257, 8, False, BINS3),
    "3d-pikp-global-1000c-1e-cells": (3, "pikp", 1, 1000, 1, False, BINS3),
    "3d-pikp-private-1000c-3e-tab": (3, "pikp", 2, 1000, 3, True, BINS3),
    "3d-urqmd-auto-257c-3e-tab": (3, "urqmd", 0, 257, 3, True, BINS3),              # 305 x 195 words: form 0 takes the global form
    "2d-pikp-private-1c-8e-tab": (2, "pikp", 2, 1, 8, True, BINS2_ONE),
    "2d-pikp-global-1c-1e-cells": (2, "pikp", 1, 1, 1, False, BINS2_ONE),
    "2d-pikp-global-63c-8e-cells": (2, "pikp", 1, 63, 8, False, BINS2),
    "2d-pikp-private-257c-1e-tab": (2, "pikp", 2, 257, 1, True, BINS2),
    "2d-pikp-global-1000c-3e-tab": (2, "pikp", 1, 1000, 3, True, BINS2),
    "2d-urqmd-auto-257c-3e-cells": (2, "urqmd", 0, 257, 3, False, BINS2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_binned_in_one_pass_equals_the_binned_list(species, gla, tab, case):
    dim, spname, form, n, n_events, from_tab, bins = CASES[case]
    sp = species[spname]
    S = len(sp["mass"])
    v = surface(n, dim, 9800 + n + dim, sp, gla, n_events, backflow=n >= 257)
    o = dict(dimension=dim)
    kw = dict(tab=tab if from_tab else None, n_events=n_events, seed=1000 + n, y_cut=Y_CUT2)
    plist, lst = api.sample_particles_vah(v, sp, gla, o, **kw)
    bins = dict(bins, kernel_form=form)
    got, st = api.sample_binned_vah(v, sp, gla, bins, o, **kw)
    total = int(got["yield"].sum())
    print(case, "hadrons", len(plist), "drawn", lst["n_hadrons_drawn"], {k: int(got[k].sum()) for k in COUNTS})
    assert filled(got)
    assert st["n_particles"] == len(plist) == total
    # hadrons fell outside every range
    assert all(got[k].sum() < total for k in COUNTS), {k: int(got[k].sum()) for k in COUNTS}
    # the one bin decision that goes through a transcendental is yp (device log against the C library's): no hadron of the fixture sits within
    # 1e-9 of a rapidity bin edge or of the gate.  A property of the fixture; every hadron is compared.
    yp = 0.5 * np.log((plist["E"] + plist["pz"]) / (plist["E"] - plist["pz"]))
    u = (yp + bins["y_cut"]) / (2.0 * bins["y_cut"] / bins["y_bins"])
    assert np.abs(u - np.rint(u)).min() > 1e-9 and np.abs(np.abs(yp) - bins["y_cut"]).min() > 1e-9
    want = api.sampler_bin_list(bins, n_events, S, plist)
    for k in COUNTS + ("yield",):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    for k in ("vn_re", "vn_im"):
        d = np.abs(got[k] - want[k])
        print(case, k, "against the host-binned list: max |delta|", int(d.max()), "max count", int(want["dN_pT"].max()))
        assert np.all(d <= want["dN_pT"][None]), k
    # the same list through the device kernel: the same arithmetic on the same particle bits
    dev, skipped = api.sampler_bin_list_device(bins, n_events, S, plist)
    assert skipped == 0
    for k in COUNTS + ("yield",):
        assert np.array_equal(got[k], dev[k]), k
    for k in ("vn_re", "vn_im"):
        print(case, k, "against the device-binned list: identical" if np.array_equal(got[k], dev[k]) else
              "against the device-binned list: max |delta| %d" % int(np.abs(got[k] - dev[k]).max()))
        assert np.all(np.abs(got[k] - dev[k]) <= dev["dN_pT"][None]), k
    for k in TALLIES:
        assert st[k] == lst[k], (k, st[k], lst[k])
    if n >= 257:
        assert st["n_cells_skipped"] > 0
    if spname == "urqmd":
        assert S == 305 and len(np.unique(plist["species"])) > 50


# ---- 2. the histograms do not depend on how the work is cut; 3. the stats convention ----
@pytest.fixture(scope="module")
def cut(species, gla, tab):
    """257 cells x 5 events, 3+1D, computed once and left unchanged"""
    sp = species["pikp"]
    v = surface(257, 3, 9901, sp, gla, 5, backflow=True)
    kw = dict(tab=tab, n_events=5, seed=77)
    whole, st = api.sample_binned_vah(v, sp, gla, BINS3, dict(dimension=3), **kw)
    assert filled(whole)
    return dict(v=v, sp=sp, kw=kw, whole=whole, stats=st)


def test_histograms_do_not_depend_on_how_the_work_is_cut(cut, gla):
    v, sp, kw, whole = cut["v"], cut["sp"], cut["kw"], cut["whole"]
    o = dict(dimension=3)
    for be in (0, 1, 2):
        h, _ = api.sample_binned_vah(v, sp, gla, BINS3, o, batch_events=be, **kw)
        assert same(h, whole), be
    forms = {}
    for form in (1, 2):                                    # global | workgroup-private
        forms[form], _ = api.sample_binned_vah(v, sp, gla, dict(BINS3, kernel_form=form), o, **kw)
        assert same(forms[form], whole), form
    assert same(forms[1], forms[2])
    again, _ = api.sample_binned_vah(v, sp, gla, BINS3, o, **kw)
    assert same(again, whole)
    for edges in ((0, 100, 257), (0, 64, 129, 257)):       # two and three cell shards through first_cell, added with numpy
        parts = []
        for lo, hi in zip(edges[:-1], edges[1:]):
            h, _ = api.sample_binned_vah({k: x[lo:hi] for k, x in v.items()}, sp, gla, BINS3, o, first_cell=lo, **kw)
            parts.append(h)
        assert same({k: sum(p[k] for p in parts) for k in ALL}, whole), edges
    multi, stm = api.sample_binned_vah_multi(v, sp, gla, BINS3, o, devices=(0, 0, 0), **kw)
    assert same(multi, whole) and stm["n_particles"] == cut["stats"]["n_particles"]
    assert all(stm[k] == cut["stats"][k] for k in TALLIES)
    other, _ = api.sample_binned_vah(v, sp, gla, BINS3, o, **dict(kw, seed=78))
    assert filled(other) and not same(other, whole)


def test_stats_convention(cut):
    st = cut["stats"]
    assert st["particle_workspace_bytes"] == 0 and st["ms_count"] == 0 and st["ms_fill"] == 0 and st["ms_bin"] > 0
    assert st["n_particles"] == cut["whole"]["yield"].sum() and st["n_hadrons_drawn"] >= st["n_particles"]


# ---- 3b. where the private form ends ----
# the bins of LDS_FIT in tests/test_gpu_sampler_bins_lists.py: one species, 15 * 500 + 200 + 200 + 146 + 146 = 8192 words
LDS_FIT = dict(R.BINS, pT_bins=500, y_bins=200, eta_bins=200, tau_bins=146, r_bins=146)


def test_the_private_form_ends_where_the_block_and_the_tally_words_fill_the_lds(gla, tab):
    """pi+ alone, 400 cells x 30 events.  The fused kernel keeps three tally words of static LDS beside the dynamic block, so tau_bins = 143
    (8189 words) is the largest block of the private form and tau_bins = 146 (8192 words, which the list kernel still holds) the first that
    form 0 must send to the global form.  Forms 0 and 1 at both sizes, and form 2 at 8189, give the histograms of the host-binned list of
    the same call; form 2 at 8192 is refused."""
    sp = inputs.species([211])
    v = surface(400, 3, 9941, sp, gla, 30)
    o = dict(dimension=3)
    kw = dict(tab=tab, n_events=30, seed=61)
    plist, lst = api.sample_particles_vah(v, sp, gla, o, **kw)
    assert len(plist) >= 2000
    for tau_bins, words, forms in ((143, 8189, (0, 1, 2)), (146, 8192, (0, 1))):
        bins = dict(LDS_FIT, tau_bins=tau_bins)
        assert R.layout_total(bins, 1) == words
        yp = 0.5 * np.log((plist["E"] + plist["pz"]) / (plist["E"] - plist["pz"]))
        u = (yp + bins["y_cut"]) / (2.0 * bins["y_cut"] / bins["y_bins"])
        assert np.abs(u - np.rint(u)).min() > 1e-9 and np.abs(np.abs(yp) - bins["y_cut"]).min() > 1e-9      # (a property of the fixture)
        want = api.sampler_bin_list(bins, 30, 1, plist)
        assert want["yield"].sum() == len(plist) and all(want[k].sum() > 0 for k in COUNTS)
        for form in forms:
            got, st = api.sample_binned_vah(v, sp, gla, dict(bins, kernel_form=form), o, **kw)
            for k in COUNTS + ("yield",):
                assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (words, form, k)
            for k in ("vn_re", "vn_im"):
                d = np.abs(got[k] - want[k])
                print(words, "words, form", form, k, "against the host-binned list: max |delta|", int(d.max()))
                assert np.all(d <= want["dN_pT"][None]), (words, form, k)
            assert st["n_particles"] == len(plist) and all(st[k] == lst[k] for k in TALLIES), (words, form)
    with pytest.raises(api.Is3dError) as e:
        api.sample_binned_vah(v, sp, gla, dict(LDS_FIT, kernel_form=2), o, **kw)
    assert e.value.code == api.IS3D_EINVAL and "kernel_form = 2" in str(e.value) and "8192" in str(e.value)


# ---- 4. nothing is allocated per event ----
def test_allocations_do_not_grow_with_events(species, gla, tab):
    sp = species["pikp"]
    o = dict(dimension=3)

    def allocations(n_events, batch_events):
        v = surface(63, 3, 9911, sp, gla, n_events)
        a0 = api.resource_counters()[1]
        h, st = api.sample_binned_vah(v, sp, gla, BINS3, o, tab=tab, n_events=n_events, seed=5, batch_events=batch_events)
        assert filled(h) and st["particle_workspace_bytes"] == 0
        return api.resource_counters()[1] - a0

    one, eight = allocations(1, 1), allocations(8, 0)
    print("device allocations: 1 event (batch_events = 1) %d, 8 events %d" % (one, eight))
    assert 0 < eight <= one


# ---- 5. bad cells ----
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_bad_cells_are_reported_and_the_others_binned(species, gla, tab, multi):
    """Lambda = NaN at cell 40 and alpha_L beyond the last table node (2.0) at cell 63: IS3D_EDOMAIN names the lower one by its global index,
    and the histograms are those of the surface with the two cells switched off through u.dsigma <= 0 -- the other cells keep their global
    indices, and with them their streams."""
    sp = species["pikp"]
    v = surface(90, 3, 9921, sp, gla, 9)
    o = dict(dimension=3)
    kw = dict(tab=tab, n_events=9, seed=41, first_cell=1000)
    if multi:
        kw["devices"] = [0, 0, 0]
    off = {k: x.copy() for k, x in v.items()}
    for f in ("dat", "dax", "day", "dan"):
        off[f][[40, 63]] = -off[f][[40, 63]]
    want, wst = api.sample_binned_vah(off, sp, gla, BINS3, o, **kw)
    assert filled(want) and wst["n_cells_skipped"] == 2
    bad = {k: x.copy() for k, x in v.items()}
    bad["Lambda"][40] = np.nan
    bad["aL"][63] = 2.5
    with pytest.raises(api.Is3dError) as e:
        api.sample_binned_vah(bad, sp, gla, BINS3, o, **kw)
    assert e.value.code == api.IS3D_EDOMAIN and e.value.bad_cell == 1040, str(e.value)
    assert same(e.value.hist, want)
    assert e.value.stats["n_particles"] == want["yield"].sum() and e.value.stats["n_hadrons_drawn"] == wst["n_hadrons_drawn"]
    whole, _ = api.sample_binned_vah(v, sp, gla, BINS3, o, **kw)
    assert not same(whole, want)                            # the two cells do emit


# ---- 6. refusals on the device machine ----
def test_refusals_leave_the_device_alone(species, gla, tab):
    sp = species["pikp"]
    v = surface(63, 3, 9931, sp, gla, 2)
    o = dict(dimension=3)
    before = api.resource_counters()
    for spx, bins, extra in ((species["urqmd"], dict(SHIPPED_BINS, kernel_form=2), {}), (sp, dict(BINS3, kernel_form=3), {}),
                             (sp, dict(BINS3, pT_upper_cut=BINS3["pT_lower_cut"]), {}), (sp, dict(BINS3, pT_upper_cut=0.05), {}),
                             (sp, BINS3, dict(fast=1))):
        for devices in (None, [0, 0]):
            with pytest.raises(api.Is3dError) as e:
                api.sample_binned_vah(v, spx, gla, bins, o, tab=tab, n_events=2, seed=3, devices=devices, **extra)
            assert e.value.code == api.IS3D_EINVAL, str(e.value)
    assert api.resource_counters() == before
