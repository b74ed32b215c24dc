"""GPU (-m gpu): the sampler's test_sampler = 1 distributions binned on the device and list-free (is3d_sample_binned,
is3d_sampler_plan_execute_binned, is3d_sample_binned_multi) against the host yardstick on the sampler's own list
(is3d_sampler_bin_list(is3d_sample_particles)): parity, invariance under batching / sharding / devices, the memory bound, the refusals."""
import numpy as np
import pytest

from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu
COUNTS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield")
ALL = COUNTS + ("vn_re", "vn_im")

# bins that leave particles OUTSIDE every range: the surfaces have tau in [1, 10], r in [0, 8], eta in [-4, 4] (3+1D).
# The surfaces, modes and seeds are those of tests/test_gpu_sampler.py.  Its 25 events on the 600-cell surface hold 82 hadrons, too few to fill
# the histograms, and its 150 events on the 400-cell surface hold 510, so this file samples 400 and 450 events of them (the same surfaces, modes and
# seeds; more than 1000 hadrons are asserted below).
CASES = {
    "3d_ce": dict(n=600, dim=3, seed=811, df_mode=2, n_events=400, sseed=7, y_cut=0.5,
                  bins=dict(y_cut=2.1, y_bins=14, eta_cut=3.0, eta_bins=20, pT_lower_cut=0.1, pT_upper_cut=1.0, pT_bins=10, tau_min=2.5, tau_max=8.5,
                            tau_bins=6, r_min=1.0, r_max=6.0, r_bins=5)),
    "2d_14m": dict(n=400, dim=2, seed=802, df_mode=1, n_events=450, sseed=4242, y_cut=0.7,
                   bins=dict(y_cut=0.49, y_bins=14, eta_cut=0.4, eta_bins=20, pT_lower_cut=0.1, pT_upper_cut=1.0, pT_bins=10, tau_min=2.5, tau_max=8.5,
                             tau_bins=6, r_min=1.0, r_max=6.0, r_bins=5)),
}


def same(a, b, keys=ALL):
    return all(a[k].dtype == np.int64 and np.array_equal(a[k], b[k]) for k in keys)


@pytest.fixture(scope="module")
def runs(fx):
    """Per case, computed once and left unchanged: the list, its host histograms, and the device histograms of the same inputs."""
    out = {}
    for name, c in CASES.items():
        cells = synth.synth_surface(c["n"], c["dim"], seed=c["seed"])
        o = dict(dimension=c["dim"], df_mode=c["df_mode"])
        kw = dict(n_events=c["n_events"], seed=c["sseed"], y_cut=c["y_cut"])
        gla = inputs.feqmod_tables(0.15)
        plist, lst = api.sample_particles(cells, fx["pikp"], fx["df"], gla, o, **kw)
        want = api.sampler_bin_list(c["bins"], c["n_events"], 3, plist)
        got, st = api.sample_binned(cells, fx["pikp"], fx["df"], gla, c["bins"], o, **kw)
        out[name] = dict(c, cells=cells, o=o, kw=kw, gla=gla, list=plist, list_stats=lst, want=want, got=got, stats=st)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_binned_on_device_equals_the_binned_list(runs, case):
    r = runs[case]
    p, b = r["list"], r["bins"]
    assert len(p) > 1000
    # the one bin decision that goes through a transcendental is yp (device log vs the C library's): no particle of the fixture sits within
    # 1e-9 of a rapidity bin edge or of the gate.  A property of the fixture; every particle is compared.
    yp = 0.5 * np.log((p["E"] + p["pz"]) / (p["E"] - p["pz"]))
    u = (yp + b["y_cut"]) / (2.0 * b["y_cut"] / b["y_bins"])
    assert np.abs(u - np.rint(u)).min() > 1e-9 and np.abs(np.abs(yp) - b["y_cut"]).min() > 1e-9
    got, want, st = r["got"], r["want"], r["stats"]
    for k in COUNTS:
        print(case, k, int(got[k].sum()), int(want[k].sum()))
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    assert st["n_particles"] == len(p) == got["yield"].sum()
    # particles fell outside every range
    assert all(0 < want[k].sum() < len(p) for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r"))
    # one fixed-point step per particle: device and C library atan2 / sin / cos differ by a few ulp, far below a step of 2^-32
    for k in ("vn_re", "vn_im"):
        d = np.abs(got[k] - want[k])
        print(case, k, "max |delta|", int(d.max()), "max count", int(want["dN_pT"].max()))
        assert np.all(d <= want["dN_pT"][None]), k
    assert st["ms_bin"] > 0.0 and st["n_hadrons_drawn"] == r["list_stats"]["n_hadrons_drawn"]


def test_histograms_do_not_depend_on_geometry(runs, fx):
    """Integer sums: bit for bit under event batching, the kernel form, cell sharding, devices and repetition -- vn_* included."""
    r = runs["3d_ce"]
    args = (fx["pikp"], fx["df"], r["gla"], r["bins"], r["o"])
    whole = r["got"]
    for be in (1, 7):
        h, _ = api.sample_binned(r["cells"], *args, batch_events=be, **r["kw"])
        assert same(h, whole), be
    for form in (1, 2):                                      # global atomics | workgroup-private
        h, _ = api.sample_binned(r["cells"], fx["pikp"], fx["df"], r["gla"], dict(r["bins"], kernel_form=form), r["o"], **r["kw"])
        assert same(h, whole), form
    parts = []
    for lo, hi in ((0, 250), (250, 600)):
        sub = {k: v[lo:hi] for k, v in r["cells"].items()}
        h, _ = api.sample_binned(sub, *args, first_cell=lo, **r["kw"])
        parts.append(h)
    assert same({k: parts[0][k] + parts[1][k] for k in ALL}, whole)
    multi, stm = api.sample_binned_multi(r["cells"], *args, devices=[0, 0], **r["kw"])
    assert same(multi, whole) and stm["n_particles"] == r["stats"]["n_particles"]
    again, _ = api.sample_binned(r["cells"], *args, **r["kw"])
    assert same(again, whole)
    other, _ = api.sample_binned(r["cells"], *args, **dict(r["kw"], seed=8))
    assert not same(other, whole)
    # the second case through the other form too (2+1D: eta comes from the sampled rapidity)
    r2 = runs["2d_14m"]
    h, _ = api.sample_binned(r2["cells"], fx["pikp"], fx["df"], r2["gla"], dict(r2["bins"], kernel_form=1), r2["o"], batch_events=7, **r2["kw"])
    assert same(h, r2["got"])


def test_memory_is_one_batch_and_a_second_execute_allocates_nothing(runs, fx):
    import torch
    r = runs["3d_ce"]
    dev = torch.device("cuda:0")
    tens = {k: torch.from_numpy(np.ascontiguousarray(r["cells"][k])).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    plan = api.SamplerPlan(fx["pikp"], fx["df"], r["gla"], r["o"], max_cells=r["n"])
    xy = dict(x_ptr=ptrs["x"], y_ptr=ptrs["y"])
    h, st = plan.execute_binned(r["n"], ptrs, r["n_events"], r["sseed"], r["bins"], 3, batch_events=1, **xy)
    assert same(h, r["got"])
    assert 0 < st["particle_workspace_bytes"] <= 96 * int(h["yield"].max()) < 96 * st["n_particles"] // 5
    p0, a0 = api.resource_counters()
    h2, st2 = plan.execute_binned(r["n"], ptrs, r["n_events"], r["sseed"], r["bins"], 3, batch_events=1, **xy)
    assert api.resource_counters() == (p0, a0)
    assert same(h2, h) and st2["particle_workspace_bytes"] == st["particle_workspace_bytes"]
    plan.close()


def test_refusals_and_the_empty_surface(runs, fx):
    r = runs["3d_ce"]
    args = (fx["pikp"], fx["df"], r["gla"])
    p0, a0 = api.resource_counters()
    for bad in (dict(y_bins=0), dict(eta_bins=-3), dict(pT_bins=0), dict(tau_bins=0), dict(r_bins=-1), dict(pT_upper_cut=r["bins"]["pT_lower_cut"]),
                dict(pT_upper_cut=0.05), dict(kernel_form=3)):
        with pytest.raises(api.Is3dError) as e:
            api.sample_binned(r["cells"], *args, dict(r["bins"], **bad), r["o"], **r["kw"])
        assert e.value.code == -1, bad
    assert api.resource_counters() == (p0, a0)              # refused before any plan or launch
    empty, st = api.sample_binned({k: v[:0] for k, v in r["cells"].items()}, *args, r["bins"], r["o"], n_events=3, seed=7)
    assert st["n_particles"] == 0 and all(not empty[k].any() for k in ALL) and empty["yield"].shape == (3,)
