"""The C ABI of the viscous sampler's fused sample-and-bin route (is3d_sampler_plan_execute_fused, is3d_sample_fused,
is3d_sample_fused_multi) where no GPU is needed: the symbols and their declarations, every refusal of the bins (IS3D_EINVAL with a message
before any device use: the resource counters stand still), their order (a NULL, n_events, the bins, kernel_form, the private form that does
not fit -- all before the plan's own checks and before the device is looked for), and the no-CPU-path rule."""
import os

import numpy as np
import pytest

from conftest import ROOT
from is3d_amd import api, inputs, synth

NAMES = ("is3d_sampler_plan_execute_fused", "is3d_sample_fused", "is3d_sample_fused_multi")
BINS = dict(y_cut=2.0, y_bins=8, eta_cut=3.0, eta_bins=10, pT_lower_cut=0.1, pT_upper_cut=1.5, pT_bins=7, tau_min=1.0, tau_max=9.0, tau_bins=4,
            r_min=0.5, r_max=6.0, r_bins=3)
SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)
ARRAYS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "vn_re", "vn_im", "yield")


@pytest.fixture(scope="module")
def good():
    return dict(cells=synth.synth_surface(5, 3, seed=21), sp=inputs.species("pikp"), df=inputs.df_tables(), gla=inputs.feqmod_tables(0.15))


def test_the_three_symbols_are_exported_and_declared():
    lib = api.load()
    header = open(os.path.join(ROOT, "include", "is3d_amd.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(lib, name), name
    assert "int is3d_sampler_plan_execute_fused(is3d_sampler_plan *plan, const is3d_cells *cells_dev" in header
    assert "int is3d_sample_fused(const is3d_cells *cells" in header and "int is3d_sample_fused_multi(const is3d_cells *cells" in header
    assert hasattr(api.SamplerPlan, "execute_fused") and callable(api.sample_fused) and callable(api.sample_fused_multi)


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


def refused(good, multi, bins=BINS, sp=None, opts=None, **change):
    kw = dict(n_events=2, seed=3)
    kw.update(change)
    if multi:
        kw["devices"] = [0, 0]
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        api.sample_fused(good["cells"], sp or good["sp"], good["df"], good["gla"], bins, opts or dict(dimension=3, df_mode=2), **kw)
    assert e.value.code == api.IS3D_EINVAL, str(e.value)
    assert api.resource_counters() == before
    text = str(e.value).split(": ", 1)[1]
    assert len(text.strip()) > 8, str(e.value)        # a message, not only a code
    return text


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("case", sorted(BIN_REFUSALS))
def test_the_bin_refusals_come_before_any_device_use(good, case, multi):
    refused(good, multi, bins=dict(BINS, **BIN_REFUSALS[case]))


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_the_order_of_the_refusals(good, multi):
    """n_events before the bins, the bins before kernel_form, kernel_form's range before the private form that does not fit; and all of them
    before the plan's own checks (a df_mode the sampler does not have)."""
    bad_opts = dict(dimension=3, df_mode=7)
    assert "n_events" in refused(good, multi, bins=dict(BINS, y_bins=0, kernel_form=3), n_events=0, opts=bad_opts)
    assert "bin count" in refused(good, multi, bins=dict(BINS, y_bins=0, kernel_form=3), opts=bad_opts)
    assert "kernel_form = 3" in refused(good, multi, bins=dict(BINS, kernel_form=3), opts=bad_opts)
    urqmd = inputs.species("urqmd")
    assert "kernel_form = 5" in refused(good, multi, bins=dict(SHIPPED_BINS, kernel_form=5), sp=urqmd, opts=bad_opts)
    # 305 species at the shipped bins: 305 * 1800 words against 8192 of 64 KiB
    text = refused(good, multi, bins=dict(SHIPPED_BINS, kernel_form=2), sp=urqmd, opts=bad_opts)
    assert "kernel_form = 2" in text and str(305 * 1800) in text


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_private_form_needs_room_for_the_tally_words_beside_the_block(good, multi):
    """One species at the shipped bins with r_bins = 6450: 50 + 70 + 120 + 6450 + 15 * 100 = 8190 words fit the 64 KiB of LDS alone but not with
    the three tally words of static LDS the fused kernel keeps beside the block: refused.  r_bins = 6449 gives 8189 words, the largest block
    that fits, and is not refused for it."""
    pion = inputs.species([211])
    text = refused(good, multi, bins=dict(SHIPPED_BINS, r_bins=6450, kernel_form=2), sp=pion)
    assert "kernel_form = 2" in text and "8190" in text
    kw = dict(n_events=2, seed=3, **(dict(devices=[0, 0]) if multi else {}))
    fits, o = dict(SHIPPED_BINS, r_bins=6449, kernel_form=2), dict(dimension=3, df_mode=2)
    if api.load().is3d_device_count() > 0:
        h, st = api.sample_fused(good["cells"], pion, good["df"], good["gla"], fits, o, **kw)
        assert h["dN_r"].shape == (1, 6449) and st["n_particles"] == h["yield"].sum()
        return
    with pytest.raises(api.Is3dError) as e:
        api.sample_fused(good["cells"], pion, good["df"], good["gla"], fits, o, **kw)
    assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)


def test_null_arguments_are_refused():
    lib = api.load()
    n = api.C.c_int64(7)
    for name, args in ((NAMES[1], 5), (NAMES[2], 7), (NAMES[0], 8)):
        f = getattr(lib, name)
        f.argtypes = None
        f.restype = api.C.c_int
        head = [None] * args if name != NAMES[0] else [None, None, None, None, api.C.c_int32(2), api.C.c_uint64(3), api.C.c_int64(0), api.C.c_int32(0)]
        assert f(*head, None, None, api.C.byref(n), None) == api.IS3D_EINVAL, name
        assert n.value in (0, 7) and lib.is3d_last_error().decode()
        assert f(*head, None, None, None, None) == api.IS3D_EINVAL, name


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_a_good_call_has_no_cpu_path(good, multi):
    """With a device: histograms of the right shapes, and n_cells = 0 gives zeros.  Without one: IS3D_ENODEVICE."""
    kw = dict(n_events=2, seed=3, **(dict(devices=[0, 0]) if multi else {}))
    o = dict(dimension=3, df_mode=2)
    none = {k: v[:0] for k, v in good["cells"].items()}
    if api.load().is3d_device_count() > 0:
        h, st = api.sample_fused(good["cells"], good["sp"], good["df"], good["gla"], BINS, o, **kw)
        assert h["dN_pT"].shape == (3, 7) and h["vn_re"].shape == (7, 3, 7) and h["yield"].shape == (2,) and st["n_particles"] == h["yield"].sum()
        h, st = api.sample_fused(none, good["sp"], good["df"], good["gla"], BINS, o, **kw)
        assert st["n_particles"] == 0 and all(h[k].dtype == np.int64 and not h[k].any() for k in ARRAYS) and h["yield"].shape == (2,)
        return
    for cells in (good["cells"], none):
        with pytest.raises(api.Is3dError) as e:
            api.sample_fused(cells, good["sp"], good["df"], good["gla"], BINS, o, **kw)
        assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
