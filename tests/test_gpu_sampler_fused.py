"""GPU (-m gpu): the viscous sampler with every hadron binned where it is sampled, in one pass and without a list (is3d_sample_fused,
is3d_sampler_plan_execute_fused, is3d_sample_fused_multi; cf_sampler_fused).  The definition is the list route: the histograms must be
those of is3d_sampler_bin_list on the list is3d_sample_particles returns for the same arguments -- counts and yields equal, vn_re / vn_im
within the project's rule against a HOST-binned list (one fixed-point unit per entry of the dN_pT bin: device and host libm differ); and
the tallies of the list route.  Against is3d_sample_binned (the list binned per batch on the device) counts and yields are equal too.
Every other comparison is bit for bit between integers.

Shapes, surfaces, modes, seeds and bins are those of tests/test_gpu_sampler_bins.py: the smallest that fill the histograms (> 1000 hadrons) and
leave hadrons outside every range."""
import numpy as np
import pytest

from is3d_amd import api, inputs, synth
from sampler_bins_ref import BINS as REF_BINS, layout_total

pytestmark = pytest.mark.gpu
COUNTS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield")
ALL = COUNTS + ("vn_re", "vn_im")
TALLIES = ("n_hadrons_drawn", "n_momentum_samples", "n_acceptances", "n_cells_skipped")

# bins that leave particles OUTSIDE every range: the surfaces have tau in [1, 10], r in [0, 8], eta in [-4, 4] (3+1D)
BINS3 = dict(y_cut=2.1, y_bins=14, eta_cut=3.0, eta_bins=20, pT_lower_cut=0.1, pT_upper_cut=1.0, pT_bins=10, tau_min=2.5, tau_max=8.5,
             tau_bins=6, r_min=1.0, r_max=6.0, r_bins=5)
BINS2 = dict(BINS3, y_cut=0.49, eta_cut=0.4)
SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)             # iS3D_parameters.dat as shipped
CASES = ("3d_ce", "2d_14m", "3d_urqmd", "3d_feqmod4", "2d_feqmod3_fast", "3d_ce_baryon")


def same(a, b, keys=ALL):
    return all(a[k].dtype == np.int64 and np.array_equal(a[k], b[k]) for k in keys)


def build_case(fx, name):
    """-> (cells, species, df, gla, bins, opts, kw)"""
    if name == "3d_ce":
        return (synth.synth_surface(600, 3, seed=811), fx["pikp"], fx["df"], inputs.feqmod_tables(0.15), BINS3, dict(dimension=3, df_mode=2),
                dict(n_events=400, seed=7, y_cut=0.5))
    if name == "2d_14m":
        return (synth.synth_surface(400, 2, seed=802), fx["pikp"], fx["df"], inputs.feqmod_tables(0.15), BINS2, dict(dimension=2, df_mode=1),
                dict(n_events=450, seed=4242, y_cut=0.7))
    if name == "3d_urqmd":
        return (synth.synth_surface(600, 3, seed=811), fx["urqmd"], fx["df"], inputs.feqmod_tables(0.15), SHIPPED_BINS, dict(dimension=3, df_mode=2),
                dict(n_events=400, seed=7, y_cut=0.5))
    if name == "3d_ce_baryon":
        cells = synth.synth_surface(300, 3, seed=850 + 3 + 2, baryon=True)
        return (cells, inputs.species([211, 321, 2212, -2212, 3122, -3122]), inputs.df_tables_full(), inputs.feqmod_tables(inputs.surface_average_T(cells)),
                BINS3, dict(dimension=3, df_mode=2, include_baryon=1, include_baryondiff_deltaf=1), dict(n_events=800, seed=90210, y_cut=0.8))
    dim, df_mode, fast = (3, 4, 0) if name == "3d_feqmod4" else (2, 3, 1)
    cells = {k: v.copy() for k, v in synth.synth_surface(400, dim, seed=830 + dim + df_mode).items()}
    cells["bulkPi"][::9] = -5.0 * cells["P"][::9]          # df_mode 3: breakdown; df_mode 4: clamped
    gla = inputs.feqmod_tables(inputs.surface_average_T(cells))
    return (cells, fx["pikp"], fx["df"], gla, BINS3 if dim == 3 else BINS2, dict(dimension=dim, df_mode=df_mode),
            dict(n_events=800, seed=31337, y_cut=0.9, fq=gla, fast=fast, T_avg=gla["T_avg"], T_avg_switch=0.151))


@pytest.fixture(scope="module")
def runs(fx):
    """Per case, computed once and left unchanged: the list with its host histograms, the list binned per batch on the device, the fused run."""
    out = {}
    for name in CASES:
        cells, sp, df, gla, bins, o, kw = build_case(fx, name)
        plist, lst = api.sample_particles(cells, sp, df, gla, o, **kw)
        want = api.sampler_bin_list(bins, kw["n_events"], len(sp["mass"]), plist)
        binned, bst = api.sample_binned(cells, sp, df, gla, bins, o, **kw)
        got, st = api.sample_fused(cells, sp, df, gla, bins, o, **kw)
        out[name] = dict(cells=cells, sp=sp, df=df, gla=gla, bins=bins, o=o, kw=kw, list=plist, list_stats=lst, want=want, binned=binned,
                         binned_stats=bst, got=got, stats=st)
    return out


@pytest.mark.parametrize("case", CASES)
def test_fused_equals_the_binned_list(runs, case):
    r = runs[case]
    p, b, got, want, st, lst = r["list"], r["bins"], r["got"], r["want"], r["stats"], r["list_stats"]
    print(case, "hadrons", len(p))
    assert len(p) > 1000
    # the one bin decision that goes through a transcendental is yp (device log vs the C library's): no particle of the fixture sits within
    # 1e-9 of a rapidity bin edge or of the gate.  A property of the fixture; every particle is compared.
    yp = 0.5 * np.log((p["E"] + p["pz"]) / (p["E"] - p["pz"]))
    u = (yp + b["y_cut"]) / (2.0 * b["y_cut"] / b["y_bins"])
    assert np.abs(u - np.rint(u)).min() > 1e-9 and np.abs(np.abs(yp) - b["y_cut"]).min() > 1e-9
    for k in COUNTS:
        print(case, k, int(got[k].sum()), int(want[k].sum()))
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    for k in ("vn_re", "vn_im"):
        d = np.abs(got[k] - want[k])
        print(case, k, "against the host-binned list: max |delta|", int(d.max()), "max count", int(want["dN_pT"].max()))
        assert np.all(d <= want["dN_pT"][None]), k
    assert st["n_particles"] == len(p) == got["yield"].sum()
    for k in TALLIES:
        assert st[k] == lst[k], (k, st[k], lst[k])
    assert st["particle_workspace_bytes"] == 0 and st["ms_count"] == 0 and st["ms_fill"] == 0 and st["ms_bin"] > 0
    if case != "3d_urqmd":                                   # (the shipped ranges hold the whole surface)
        assert all(0 < want[k].sum() < len(p) for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r"))
    assert (st["n_cells_breakdown"] > 0) == (case == "2d_feqmod3_fast")
    # the list binned per batch on the device: the same arithmetic on the same particle bits
    dev = r["binned"]
    for k in COUNTS:
        assert np.array_equal(got[k], dev[k]), k
    for k in ("vn_re", "vn_im"):
        print(case, k, "against sample_binned: identical" if np.array_equal(got[k], dev[k]) else
              "against sample_binned: max |delta| %d" % int(np.abs(got[k] - dev[k]).max()))
        assert np.all(np.abs(got[k] - dev[k]) <= dev["dN_pT"][None]), k
    assert st["n_particles"] == r["binned_stats"]["n_particles"]


def test_305_species_take_the_global_form(runs):
    """The urqmd list at the shipped bin counts: 305 * 1800 words do not fit the LDS, so form 0 must choose global atomics (the same bits as
    form 1) and form 2 is refused."""
    r = runs["3d_urqmd"]
    assert len(r["sp"]["mass"]) == 305 and layout_total(SHIPPED_BINS, 305) == 305 * 1800 > 8192
    assert len(np.unique(r["list"]["species"])) > 100
    args = (r["cells"], r["sp"], r["df"], r["gla"])
    h1, _ = api.sample_fused(*args, dict(SHIPPED_BINS, kernel_form=1), r["o"], **r["kw"])
    assert same(h1, r["got"])
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        api.sample_fused(*args, dict(SHIPPED_BINS, kernel_form=2), r["o"], **r["kw"])
    assert e.value.code == api.IS3D_EINVAL and str(305 * 1800) in str(e.value)
    assert api.resource_counters() == before


# the bins of LDS_FIT in tests/test_gpu_sampler_bins_lists.py: one species, 15 * 500 + 200 + 200 + 146 + 146 = 8192 words
LDS_FIT = dict(REF_BINS, pT_bins=500, y_bins=200, eta_bins=200, tau_bins=146, r_bins=146)


def test_the_private_form_ends_where_the_block_and_the_tally_words_fill_the_lds(fx):
    """pi+ alone, a 400-cell surface (its volumes times 50, for a few thousand hadrons) x 30 events.  The fused kernel keeps three tally words
    of static LDS beside the dynamic block, so tau_bins = 143 (8189 words) is the largest block of the private form and tau_bins = 146 (8192
    words, which the list kernel still holds) the first that form 0 must send to the global form.  Forms 0 and 1 at both sizes, and form 2 at
    8189, give the histograms of the host-binned list of the same call; form 2 at 8192 is refused."""
    sp, gla, o = inputs.species([211]), inputs.feqmod_tables(0.15), dict(dimension=3, df_mode=2)
    cells = {k: v.copy() for k, v in synth.synth_surface(400, 3, seed=861).items()}
    for f in ("dat", "dax", "day", "dan"):
        cells[f] *= 50.0
    kw = dict(n_events=30, seed=19, y_cut=0.5)
    plist, lst = api.sample_particles(cells, sp, fx["df"], gla, o, **kw)
    print("hadrons", len(plist))
    assert len(plist) >= 200
    for tau_bins, words, forms in ((143, 8189, (0, 1, 2)), (146, 8192, (0, 1))):
        bins = dict(LDS_FIT, tau_bins=tau_bins)
        assert layout_total(bins, 1) == words
        yp = 0.5 * np.log((plist["E"] + plist["pz"]) / (plist["E"] - plist["pz"]))
        u = (yp + bins["y_cut"]) / (2.0 * bins["y_cut"] / bins["y_bins"])
        assert np.abs(u - np.rint(u)).min() > 1e-9 and np.abs(np.abs(yp) - bins["y_cut"]).min() > 1e-9      # (a property of the fixture)
        want = api.sampler_bin_list(bins, 30, 1, plist)
        assert want["yield"].sum() == len(plist) and all(want[k].sum() > 0 for k in COUNTS)
        for form in forms:
            got, st = api.sample_fused(cells, sp, fx["df"], gla, dict(bins, kernel_form=form), o, **kw)
            for k in COUNTS:
                assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (words, form, k)
            for k in ("vn_re", "vn_im"):
                d = np.abs(got[k] - want[k])
                print(words, "words, form", form, k, "against the host-binned list: max |delta|", int(d.max()))
                assert np.all(d <= want["dN_pT"][None]), (words, form, k)
            assert st["n_particles"] == len(plist) and all(st[k] == lst[k] for k in TALLIES), (words, form)
    with pytest.raises(api.Is3dError) as e:
        api.sample_fused(cells, sp, fx["df"], gla, dict(LDS_FIT, kernel_form=2), o, **kw)
    assert e.value.code == api.IS3D_EINVAL and "kernel_form = 2" in str(e.value) and "8192" in str(e.value)


def test_histograms_do_not_depend_on_geometry(runs):
    """Integer sums: bit for bit under event batching, the kernel form, cell sharding, devices and repetition -- vn_* included."""
    r = runs["3d_ce"]
    args = (r["sp"], r["df"], r["gla"], r["bins"], r["o"])
    whole = r["got"]
    for be in (0, 1, 7):
        h, st = api.sample_fused(r["cells"], *args, batch_events=be, **r["kw"])
        assert same(h, whole) and all(st[k] == r["stats"][k] for k in TALLIES), be
    for form in (0, 1, 2):                                   # the measured choice | global atomics | workgroup-private
        h, _ = api.sample_fused(r["cells"], r["sp"], r["df"], r["gla"], dict(r["bins"], kernel_form=form), r["o"], **r["kw"])
        assert same(h, whole), form
    parts = []
    for lo, hi in ((0, 250), (250, 600)):
        sub = {k: v[lo:hi] for k, v in r["cells"].items()}
        h, _ = api.sample_fused(sub, *args, first_cell=lo, **r["kw"])
        parts.append(h)
    assert same({k: parts[0][k] + parts[1][k] for k in ALL}, whole)
    multi, stm = api.sample_fused_multi(r["cells"], *args, devices=[0, 0], **r["kw"])
    assert same(multi, whole) and stm["n_particles"] == r["stats"]["n_particles"]
    assert all(stm[k] == r["stats"][k] for k in TALLIES)
    again, _ = api.sample_fused(r["cells"], *args, **r["kw"])
    assert same(again, whole)
    other, _ = api.sample_fused(r["cells"], *args, **dict(r["kw"], seed=8))
    assert other["yield"].sum() > 1000 and not same(other, whole)
    # the 2+1D case through the other forms too (eta comes from the sampled rapidity)
    r2 = runs["2d_14m"]
    for form in (1, 2):
        h, _ = api.sample_fused(r2["cells"], r2["sp"], r2["df"], r2["gla"], dict(r2["bins"], kernel_form=form), r2["o"], batch_events=7, **r2["kw"])
        assert same(h, r2["got"]), form


def test_batches_without_a_particle(runs):
    """60 cells, 200 events, one event per batch: most batches hold no hadron (no launch for them) -- bit for bit the unbatched run."""
    r = runs["3d_ce"]
    cells = {k: v[:60] for k, v in r["cells"].items()}
    kw = dict(r["kw"], n_events=200)
    p, _ = api.sample_particles(cells, r["sp"], r["df"], r["gla"], r["o"], **kw)
    want = api.sampler_bin_list(r["bins"], 200, 3, p)
    assert len(p) >= 20 and (want["yield"] == 0).any() and (want["yield"] > 0).any()
    whole, st = api.sample_fused(cells, r["sp"], r["df"], r["gla"], r["bins"], r["o"], **kw)
    assert same(whole, want, COUNTS) and st["n_particles"] == len(p)
    for form in (0, 1, 2):
        h, st = api.sample_fused(cells, r["sp"], r["df"], r["gla"], dict(r["bins"], kernel_form=form), r["o"], batch_events=1, **kw)
        assert same(h, whole) and st["n_particles"] == len(p), form


def test_more_shards_than_cells_a_single_event_and_the_empty_surface(runs, fx):
    """Five shards of a 3-cell surface (two of them empty); n_events = 1 with the private form on a handful of hadrons; no cells at all."""
    r = runs["3d_ce"]
    args = (r["sp"], r["df"], r["gla"], r["bins"], r["o"])
    cells = {k: v[:3] for k, v in r["cells"].items()}
    kw = dict(r["kw"], n_events=3000)
    p, _ = api.sample_particles(cells, *args[:3], r["o"], **kw)
    want = api.sampler_bin_list(r["bins"], 3000, 3, p)
    assert len(p) >= 5
    whole, st = api.sample_fused(cells, *args, **kw)
    assert same(whole, want, COUNTS) and st["n_particles"] == len(p)
    multi, stm = api.sample_fused_multi(cells, *args, devices=[0] * 5, **kw)
    assert same(multi, whole) and stm["n_particles"] == len(p)
    kw1 = dict(r["kw"], n_events=1)
    p1, _ = api.sample_particles(r["cells"], *args[:3], r["o"], **kw1)
    want1 = api.sampler_bin_list(r["bins"], 1, 3, p1)
    assert 1 <= len(p1) < 100
    for form in (0, 1, 2):
        h, st1 = api.sample_fused(r["cells"], *args[:3], dict(r["bins"], kernel_form=form), r["o"], **kw1)
        assert same(h, want1, COUNTS) and h["yield"].shape == (1,) and h["yield"][0] == len(p1) == st1["n_particles"], form
        assert np.all(np.abs(h["vn_re"] - want1["vn_re"]) <= want1["dN_pT"][None]) and np.all(np.abs(h["vn_im"] - want1["vn_im"]) <= want1["dN_pT"][None])
    multi1, _ = api.sample_fused_multi(r["cells"], *args, devices=[0, 0], **kw1)
    assert same(multi1, h)
    empty, ste = api.sample_fused({k: v[:0] for k, v in r["cells"].items()}, *args, n_events=3, seed=7)
    assert ste["n_particles"] == 0 and all(not empty[k].any() for k in ALL) and empty["yield"].shape == (3,)


def test_memory_does_not_grow_with_hadrons_and_the_plan_serves_every_route(runs, fx):
    import torch
    r = runs["3d_ce"]
    n, ne, seed = 600, r["kw"]["n_events"], r["kw"]["seed"]
    dev = torch.device("cuda:0")
    tens = {k: torch.from_numpy(np.ascontiguousarray(r["cells"][k])).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    xy = dict(x_ptr=ptrs["x"], y_ptr=ptrs["y"])
    plan = api.SamplerPlan(r["sp"], r["df"], r["gla"], r["o"], max_cells=n)
    h, st = plan.execute_fused(n, ptrs, ne, seed, r["bins"], 3, batch_events=1, **xy)
    assert same(h, r["got"])
    assert st["particle_workspace_bytes"] == 0 and st["ms_count"] == 0 and st["ms_fill"] == 0 and 0 < st["ms_bin"]
    before = api.resource_counters()
    h2, st2 = plan.execute_fused(n, ptrs, ne, seed, r["bins"], 3, batch_events=1, **xy)
    assert api.resource_counters() == before
    assert same(h2, h) and st2["particle_workspace_bytes"] == 0
    # the same plan afterwards: the list binned per batch, the list itself, and the fused pass again
    hb, stb = plan.execute_binned(n, ptrs, ne, seed, r["bins"], 3, batch_events=1, **xy)
    assert same(hb, r["binned"]) and stb["particle_workspace_bytes"] > 0 and stb["n_particles"] == len(r["list"])
    buf = torch.zeros(len(r["list"]) * api.PARTICLE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    cnt, _ = plan.execute(n, ptrs, ne, seed, particles_ptr=buf.data_ptr(), capacity=len(r["list"]), **xy)
    assert cnt == len(r["list"])
    assert np.array_equal(np.frombuffer(buf.cpu().numpy().tobytes(), dtype=api.PARTICLE_DTYPE), r["list"])
    h3, st3 = plan.execute_fused(n, ptrs, ne, seed, r["bins"], 3, **xy)
    assert same(h3, h) and st3["particle_workspace_bytes"] == 0
    plan.close()

    def allocations(n_events):
        a0 = api.resource_counters()[1]
        fresh = api.SamplerPlan(r["sp"], r["df"], r["gla"], r["o"], max_cells=n)
        hh, s = fresh.execute_fused(n, ptrs, n_events, seed, r["bins"], 3, batch_events=1, **xy)
        assert s["particle_workspace_bytes"] == 0 and s["n_particles"] == hh["yield"].sum()
        fresh.close()
        return api.resource_counters()[1] - a0

    one, eight = allocations(1), allocations(8)
    print("device allocations of a fresh plan: 1 event %d, 8 events %d" % (one, eight))
    assert 0 < eight <= one


def test_refusals_leave_the_device_alone(runs):
    r = runs["3d_ce"]
    args = (r["cells"], r["sp"], r["df"], r["gla"])
    before = api.resource_counters()
    for bad in (dict(y_bins=0), dict(eta_bins=-3), dict(pT_bins=0), dict(tau_bins=0), dict(r_bins=-1), dict(pT_upper_cut=r["bins"]["pT_lower_cut"]),
                dict(pT_upper_cut=0.05), dict(kernel_form=3)):
        for devices in (None, [0, 0]):
            with pytest.raises(api.Is3dError) as e:
                api.sample_fused(*args, dict(r["bins"], **bad), r["o"], devices=devices, **r["kw"])
            assert e.value.code == api.IS3D_EINVAL, (bad, devices)
    assert api.resource_counters() == before              # refused before any plan or launch


def test_a_cell_off_the_coefficient_table_is_named(runs):
    r = runs["3d_ce"]
    cells = {k: v.copy() for k, v in r["cells"].items()}
    cells["T"][123] = 0.31
    msgs = []
    for fn in (api.sample_binned, api.sample_fused):
        with pytest.raises(api.Is3dError) as e:
            fn(cells, r["sp"], r["df"], r["gla"], r["bins"], r["o"], **r["kw"])
        assert e.value.code == api.IS3D_EDOMAIN and "cell 123" in str(e.value)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
