"""The C ABI of the anisotropic-hydro sampler binned on the device (is3d_sample_binned_vah, is3d_sample_binned_vah_multi) where no GPU is
needed: the symbols and their declarations, every refusal the header lists (IS3D_EINVAL with a message before any device use: the resource
counters stand still), their order (the sampler's refusals before the bins'), the no-CPU-path rule and the empty surface."""
import os

import numpy as np
import pytest

from conftest import ROOT
from is3d_amd import api, inputs, synth

NAMES = ("is3d_sample_binned_vah", "is3d_sample_binned_vah_multi")
BINS = dict(y_cut=2.0, y_bins=8, eta_cut=3.0, eta_bins=10, pT_lower_cut=0.1, pT_upper_cut=1.5, pT_bins=7, tau_min=1.0, tau_max=9.0, tau_bins=4,
            r_min=0.5, r_max=6.0, r_bins=3)
SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)
ARRAYS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "vn_re", "vn_im", "yield")


@pytest.fixture(scope="module")
def good():
    return dict(cells=synth.synth_vah_surface(5, 3, seed=21), sp=inputs.species([211, 321, 2212, -2212]), gla=inputs.feqmod_tables(0.15),
                tab=inputs.vah_df_tables())


def test_the_two_symbols_are_exported_and_declared():
    lib = api.load()
    header = open(os.path.join(ROOT, "include", "is3d_amd.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(lib, name), name
        assert "int %s(const is3d_vah_cells *cells" % name in header, name


def without(cells, *names):
    return {k: v for k, v in cells.items() if k not in names}


# what is3d_sample_particles_vah refuses (sampler_vah_check), then what is3d_sample_binned refuses of the bins
SAMPLER_REFUSALS = {
    "fast": lambda g: dict(fast=1),
    "feqmod": lambda g: dict(fq=g["gla"]),
    "n_events-0": lambda g: dict(n_events=0),
    "n_gla-0": lambda g: dict(gla=dict(root1=np.zeros(0), weight1=np.zeros(0))),
    "n_gla-257": lambda g: dict(gla=dict(root1=np.ones(257), weight1=np.ones(257))),
    "no-Lambda": lambda g: dict(cells=without(g["cells"], "Lambda")),
    "no-eta-3d": lambda g: dict(cells=without(g["cells"], "eta")),
    "no-c3-without-tables": lambda g: dict(cells=without(g["cells"], "c3")),
    "no-pitn-with-shear": lambda g: dict(cells=without(g["cells"], "pitn")),
    "dimension-4": lambda g: dict(opts=dict(dimension=4)),
}
BIN_REFUSALS = {
    "y_bins-0": dict(y_bins=0),
    "eta_bins-negative": dict(eta_bins=-3),
    "pT_bins-0": dict(pT_bins=0),
    "tau_bins-0": dict(tau_bins=0),
    "r_bins-negative": dict(r_bins=-1),
    "pT-range-empty": dict(pT_upper_cut=BINS["pT_lower_cut"]),
    "pT-range-inverted": dict(pT_upper_cut=0.05),
    "tau-range-empty": dict(tau_max=BINS["tau_min"]),
    "y_cut-0": dict(y_cut=0.0),
    "kernel_form-3": dict(kernel_form=3),
    "kernel_form-negative": dict(kernel_form=-1),
}


def refused(good, multi, bins=BINS, sp=None, **change):
    kw = dict(cells=good["cells"], gla=good["gla"], opts=dict(dimension=3), n_events=2, seed=3)
    kw.update(change)
    cells, gla, opts = kw.pop("cells"), kw.pop("gla"), kw.pop("opts")
    if multi:
        kw["devices"] = [0, 0]
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        api.sample_binned_vah(cells, sp or good["sp"], gla, bins, opts, **kw)
    assert e.value.code == api.IS3D_EINVAL, str(e.value)
    assert api.resource_counters() == before
    text = str(e.value).split(": ", 1)[1]
    assert len(text.strip()) > 8, str(e.value)        # a message, not only a code
    return text


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("case", sorted(SAMPLER_REFUSALS))
def test_the_samplers_refusals_come_before_any_device_use(good, case, multi):
    refused(good, multi, **SAMPLER_REFUSALS[case](good))


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("case", sorted(BIN_REFUSALS))
def test_the_bin_refusals_come_before_any_device_use(good, case, multi):
    refused(good, multi, bins=dict(BINS, **BIN_REFUSALS[case]))


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_private_form_is_refused_where_the_block_does_not_fit(good, multi):
    """305 species at the shipped bins: 305 * 1800 words against 8192 of 64 KiB; pi K p pbar at the same bins fit (7200) and are not refused for it"""
    urqmd = inputs.species("urqmd")
    assert len(urqmd["mass"]) == 305
    text = refused(good, multi, bins=dict(SHIPPED_BINS, kernel_form=2), sp=urqmd)
    assert "kernel_form = 2" in text and str(305 * 1800) in text
    with pytest.raises(api.Is3dError) as e:                     # ... a refusal of the sampler's comes first
        api.sample_binned_vah(good["cells"], urqmd, good["gla"], dict(SHIPPED_BINS, kernel_form=2), dict(dimension=3), fast=1,
                              **(dict(devices=[0, 0]) if multi else {}))
    assert e.value.code == api.IS3D_EINVAL and "fast" in str(e.value)


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_private_form_needs_room_for_the_tally_words_beside_the_block(good, multi):
    """pi K p pbar at the shipped bins with tau_bins = 128, r_bins = 300: 4 * (50 + 70 + 128 + 300 + 15 * 100) = 8192 words fill the 64 KiB of
    LDS, but the fused kernel keeps three tally words of static LDS beside the block: refused, as is3d_sample_fused refuses it.  r_bins = 298
    gives 8184 words, which fit with the three words (8189 is the largest block that does) and are not refused for it."""
    bins = dict(SHIPPED_BINS, tau_bins=128, r_bins=300, kernel_form=2)
    assert len(good["sp"]["mass"]) == 4
    text = refused(good, multi, bins=bins)
    assert "kernel_form = 2" in text and "8192" in text
    kw = dict(n_events=2, seed=3, **(dict(devices=[0, 0]) if multi else {}))
    fits = dict(bins, r_bins=298)
    if api.load().is3d_device_count() > 0:
        h, st = api.sample_binned_vah(good["cells"], good["sp"], good["gla"], fits, dict(dimension=3), **kw)
        assert h["dN_r"].shape == (4, 298) and h["dN_tau"].shape == (4, 128) and st["n_particles"] == h["yield"].sum()
        return
    with pytest.raises(api.Is3dError) as e:
        api.sample_binned_vah(good["cells"], good["sp"], good["gla"], fits, dict(dimension=3), **kw)
    assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)


def test_null_arguments_are_refused():
    lib = api.load()
    n = api.C.c_int64(7)
    for name, extra in ((NAMES[0], ()), (NAMES[1], (None, 0))):
        f = getattr(lib, name)
        f.argtypes = None
        f.restype = api.C.c_int
        assert f(None, None, None, None, None, *extra, None, None, api.C.byref(n), None) == api.IS3D_EINVAL
        assert n.value == 0 and lib.is3d_last_error().decode()
        assert f(None, None, None, None, None, *extra, None, None, None, None) == api.IS3D_EINVAL


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_a_good_call_has_no_cpu_path_and_an_empty_surface_gives_zero_histograms(good, multi):
    """With a device: histograms of the right shapes, and n_cells = 0 gives zeros.  Without one: IS3D_ENODEVICE for both (the plan comes first,
    as for is3d_sample_particles_vah)."""
    kw = dict(n_events=2, seed=3, **(dict(devices=[0, 0]) if multi else {}))
    none = {k: v[:0] for k, v in good["cells"].items()}
    if api.load().is3d_device_count() > 0:
        h, st = api.sample_binned_vah(good["cells"], good["sp"], good["gla"], BINS, dict(dimension=3), **kw)
        assert h["dN_pT"].shape == (4, 7) and h["vn_re"].shape == (7, 4, 7) and h["yield"].shape == (2,) and st["n_particles"] == h["yield"].sum()
        h, st = api.sample_binned_vah(none, good["sp"], good["gla"], BINS, dict(dimension=3), tab=good["tab"], **kw)
        assert st["n_particles"] == 0 and all(h[k].dtype == np.int64 and not h[k].any() for k in ARRAYS) and h["yield"].shape == (2,)
        return
    for cells in (good["cells"], none):
        with pytest.raises(api.Is3dError) as e:
            api.sample_binned_vah(cells, good["sp"], good["gla"], BINS, dict(dimension=3), **kw)
        assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
