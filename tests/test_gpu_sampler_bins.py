"""GPU (-m gpu): the sampler's test_sampler = 1 distributions binned on the device and list-free (is3d_sample_binned,
is3d_sampler_plan_execute_binned, is3d_sample_binned_multi) against the host yardstick on the sampler's own list
(is3d_sampler_bin_list(is3d_sample_particles)): parity, invariance under batching / sharding / devices, the memory bound, the refusals; and
the same parity for the 305-species list (global atomics: the block does not fit the LDS), df_mode 3 / 4, fast = 1, include_baryon = 1, batches
without a particle, more shards than cells and a single event."""
import numpy as np
import pytest

from is3d_amd import api, inputs, synth
from sampler_bins_ref import layout_total

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


# ---- more of the sampler through the same parity: the inputs are those tests/test_gpu_sampler.py builds for these modes ----
SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)             # iS3D_parameters.dat as shipped


def parity(cells, sp, df, gla, bins, o, kw, at_least):
    """sample_binned against sampler_bin_list(sample_particles) of the same inputs: counts and yields exact, vn within one fixed-point step per
    particle; no sampled particle within 1e-9 of a rapidity edge or of the gate (a property of the seed, asserted).  Returns (list, got, stats)."""
    p, lst = api.sample_particles(cells, sp, df, gla, o, **kw)
    print("hadrons:", len(p))
    assert len(p) >= at_least
    yp = 0.5 * np.log((p["E"] + p["pz"]) / (p["E"] - p["pz"]))
    u = (yp + bins["y_cut"]) / (2.0 * bins["y_cut"] / bins["y_bins"])
    assert np.abs(u - np.rint(u)).min() > 1e-9 and np.abs(np.abs(yp) - bins["y_cut"]).min() > 1e-9
    want = api.sampler_bin_list(bins, kw["n_events"], len(sp["mass"]), p)
    got, st = api.sample_binned(cells, sp, df, gla, bins, o, **kw)
    for k in COUNTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    for k in ("vn_re", "vn_im"):
        assert np.all(np.abs(got[k] - want[k]) <= want["dN_pT"][None]), k
    assert st["n_particles"] == len(p) == got["yield"].sum() and st["n_hadrons_drawn"] == lst["n_hadrons_drawn"]
    return p, got, st


def test_305_species_take_the_global_form(fx):
    """The urqmd list at the shipped bin counts on the 3+1D surface: 305 * 1800 words do not fit the LDS, so form 0 must choose global atomics
    (the same bits as form 1) and form 2 is refused."""
    cells = synth.synth_surface(600, 3, seed=811)
    sp, gla, o = fx["urqmd"], inputs.feqmod_tables(0.15), dict(dimension=3, df_mode=2)
    assert len(sp["mass"]) == 305 and layout_total(SHIPPED_BINS, 305) == 305 * 1800 > 8192
    kw = dict(n_events=400, seed=7, y_cut=0.5)
    p, got, _ = parity(cells, sp, fx["df"], gla, SHIPPED_BINS, o, kw, 1001)
    assert len(np.unique(p["species"])) > 100
    h1, _ = api.sample_binned(cells, sp, fx["df"], gla, dict(SHIPPED_BINS, kernel_form=1), o, **kw)
    assert same(h1, got)
    with pytest.raises(api.Is3dError) as e:
        api.sample_binned(cells, sp, fx["df"], gla, dict(SHIPPED_BINS, kernel_form=2), o, **kw)
    assert e.value.code == api.IS3D_EINVAL and str(305 * 1800) in str(e.value)


@pytest.mark.parametrize("mode", ["3d_feqmod4", "2d_feqmod3_fast", "3d_ce_baryon"])
def test_other_modes_binned_on_device_equal_the_binned_list(fx, mode):
    """df_mode 4, df_mode 3 with fast = 1 (2+1D) and include_baryon = 1 (six species, p / pbar and Lambda / Lambdabar apart)."""
    if mode == "3d_ce_baryon":
        cells = synth.synth_surface(300, 3, seed=850 + 3 + 2, baryon=True)
        sp, df = inputs.species([211, 321, 2212, -2212, 3122, -3122]), inputs.df_tables_full()
        gla = inputs.feqmod_tables(inputs.surface_average_T(cells))
        o = dict(dimension=3, df_mode=2, include_baryon=1, include_baryondiff_deltaf=1)
        kw = dict(n_events=800, seed=90210, y_cut=0.8)
        bins = CASES["3d_ce"]["bins"]
    else:
        dim, df_mode, fast = (3, 4, 0) if mode == "3d_feqmod4" else (2, 3, 1)
        cells = synth.synth_surface(400, dim, seed=830 + dim + df_mode)
        cells = {k: v.copy() for k, v in cells.items()}
        cells["bulkPi"][::9] = -5.0 * cells["P"][::9]          # df_mode 3: breakdown; df_mode 4: clamped
        sp, df = fx["pikp"], fx["df"]
        gla = inputs.feqmod_tables(inputs.surface_average_T(cells))
        o = dict(dimension=dim, df_mode=df_mode)
        kw = dict(n_events=800, seed=31337, y_cut=0.9, fq=gla, fast=fast, T_avg=gla["T_avg"], T_avg_switch=0.151)
        bins = CASES["3d_ce" if dim == 3 else "2d_14m"]["bins"]
    assert 300 <= len(cells["T"]) <= 600
    p, got, st = parity(cells, sp, df, gla, bins, o, kw, 1001)
    assert (st["n_cells_breakdown"] > 0) == (mode == "2d_feqmod3_fast")
    assert all(0 < got[k].sum() < len(p) for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r"))


def test_batches_without_a_particle(runs, fx):
    """60 cells, 200 events, one event per batch: most batches hold no hadron (no fill, no bin launch for them) -- bit for bit the unbatched run."""
    r = runs["3d_ce"]
    cells = {k: v[:60] for k, v in r["cells"].items()}
    kw = dict(r["kw"], n_events=200)
    p, whole, _ = parity(cells, fx["pikp"], fx["df"], r["gla"], r["bins"], r["o"], kw, 20)
    assert (whole["yield"] == 0).any() and (whole["yield"] > 0).any()
    for form in (0, 1, 2):
        h, st = api.sample_binned(cells, fx["pikp"], fx["df"], r["gla"], dict(r["bins"], kernel_form=form), r["o"], batch_events=1, **kw)
        assert same(h, whole) and st["n_particles"] == len(p), form


def test_more_shards_than_cells_and_a_single_event(runs, fx):
    """Five shards of a 3-cell surface (two of them empty), and n_events = 1 over two shards: each equals the single-device result."""
    r = runs["3d_ce"]
    args = (fx["pikp"], fx["df"], r["gla"], r["bins"], r["o"])
    cells = {k: v[:3] for k, v in r["cells"].items()}
    kw = dict(r["kw"], n_events=3000)
    p, whole, _ = parity(cells, *args[:3], r["bins"], r["o"], kw, 5)
    multi, stm = api.sample_binned_multi(cells, *args, devices=[0] * 5, **kw)
    assert same(multi, whole) and stm["n_particles"] == len(p)
    kw1 = dict(r["kw"], n_events=1)
    p1, one, _ = parity(r["cells"], fx["urqmd"], fx["df"], r["gla"], r["bins"], r["o"], kw1, 1)
    assert one["yield"].shape == (1,) and one["yield"][0] == len(p1)
    multi1, st1 = api.sample_binned_multi(r["cells"], fx["urqmd"], fx["df"], r["gla"], r["bins"], r["o"], devices=[0, 0], **kw1)
    assert same(multi1, one) and st1["n_particles"] == len(p1)
    ref, _ = api.sample_binned(r["cells"], *args, **kw1)       # pi/K/p: the block fits, so the private form runs on a handful of hadrons too
    for form in (1, 2):
        h, _ = api.sample_binned(r["cells"], *args[:3], dict(r["bins"], kernel_form=form), r["o"], **kw1)
        assert same(h, ref), form
