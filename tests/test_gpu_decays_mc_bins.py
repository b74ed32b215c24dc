"""GPU (-m gpu): the test_sampler distributions of sampled hadrons AFTER their Monte Carlo decays, binned on the device in one pass
(is3d_decay_particles_binned, is3d_sampler_plan_execute_decayed_binned, is3d_sample_decayed_binned, the driver's test_sampler_decayed).

The definition is the host route of tests/decays_mc_bins_cases.py: is3d_decay_particles, species -> slot[species] with slot -1 dropped,
is3d_sampler_bin_list.  Counts and yields must be equal exactly, vn_re / vn_im within one unit per entry of the dN_pT bin (device against host
libm), n_final, n_unbinned and every tally equal.  Every particle is compared; the condition on the fixtures -- no final particle within 1e-9
of a bin edge or of the rapidity gate, three orders above BOUND = 1.536e-12 -- is asserted on the host list in each test.

Lists: hand_list (257 primaries, 7 events; it needs the urqmd table's open 4-body channel, which the smash table has not) and every_unstable
on both tables, lifetime 0 and 1, as they are (every primary at one point: with lifetime 0 only the rapidity and pT histograms can see particles
outside their range) and with a position of its own per primary (`spread`: every histogram has entries and misses some)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import decays_mc_bins_cases as bc
import decays_mc_cases as cases
import decays_mc_ref as ref
import refformat
from is3d_amd import api, inputs, synth
from test_gpu_decays import RunResult
from test_gpu_sampler_bins import CASES

pytestmark = pytest.mark.gpu
URQMD, SMASH = "pdg-urqmd_v3.3+.dat", "pdg_smash.dat"
SEED = cases.SEED
SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)             # iS3D_parameters.dat as shipped: 1800 words per species
_cache = {}


@pytest.fixture(scope="module")
def tabs(reference):
    return cases.tables(api, reference)


def primaries(tabs, which):
    """which: hand | every-urqmd | every-smash, with -spread for a position of its own per primary -> (table, list, slot map, n_slots)"""
    if which not in _cache:
        kind = which.replace("-spread", "")
        t = tabs[SMASH if kind == "every-smash" else URQMD]
        q = cases.hand_list(api, t, ref.prepare(t)) if kind == "hand" else cases.every_unstable(api, t, 3)
        slot, ids = api.stable_slots(t)
        _cache[which] = (t, bc.spread(q) if which.endswith("-spread") else q, slot, len(ids))
    return _cache[which]


def host(tabs, which, lifetime, n=None):
    """the host route of the first n primaries of a list, computed once and never changed"""
    key = (which, lifetime, n)
    if key not in _cache:
        t, q, slot, S = primaries(tabs, which)
        _cache[key] = bc.host_route(api, t, t["mc_id"], q[:n], slot, S, bc.BINS, bc.N_EVENTS, lifetime, SEED)
    return _cache[key]


def device(tabs, which, lifetime=0, lo=0, hi=None, bins=bc.BINS, slot=None, n_slots=None):
    t, q, s, S = primaries(tabs, which)
    return api.decay_particles_binned(t, t["mc_id"], q[lo:hi], s if slot is None else slot, n_slots or S, bins, bc.N_EVENTS, seed=SEED,
                                      first_particle=lo, lifetime=lifetime)


# ---- 1. parity on the hand lists ----
@pytest.mark.parametrize("which", ["hand", "every-urqmd", "every-smash", "hand-spread", "every-urqmd-spread", "every-smash-spread"])
@pytest.mark.parametrize("lifetime", [0, 1])
def test_parity_with_the_host_route(tabs, which, lifetime):
    out, rel, want, st = host(tabs, which, lifetime)
    print(which, lifetime, "finals", len(out), "binned", len(rel), "edge distance %.3g" % bc.edge_distance(rel, bc.BINS))
    assert bc.edge_clear(rel, bc.BINS)
    assert len(rel) >= len(out) - 1 > 500                     # all stable entries have a slot: only the stuck 10333 of urqmd has none
    got, dst = device(tabs, which, lifetime)
    bc.assert_parity(got, dst, want, rel, out, st)
    assert dst["ms_bin"] > 0.0 and int(got["yield"].sum()) == len(rel) and (got["yield"] > 0).all()
    keys = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r") if (lifetime or which.endswith("-spread")) else ("dN_dy", "dN_pT")
    assert bc.inside_and_outside(got, len(rel), keys), {k: int(got[k].sum()) for k in keys}
    assert all(got[k].any() for k in bc.ALL)


# ---- 2. lengths off the wave and the workgroup ----
@pytest.mark.parametrize("n", cases.LENGTHS + (0,))
def test_lengths_off_the_wave_and_the_workgroup(tabs, n):
    out, rel, want, st = host(tabs, "hand-spread", 1, n)
    assert bc.edge_clear(rel, bc.BINS)
    for form in (0, 1):
        got, dst = device(tabs, "hand-spread", 1, 0, n, bins=dict(bc.BINS, kernel_form=form))
        bc.assert_parity(got, dst, want, rel, out, st)
    if n == 0:
        assert dst["n_final"] == 0 and dst["ms_bin"] == 0.0 and all(not got[k].any() for k in bc.ALL)


# ---- 3. no dependence on form or pieces ----
@pytest.mark.parametrize("which", ["hand-spread", "every-smash"])
def test_bits_do_not_depend_on_form_or_pieces(tabs, which):
    t, q, slot, S = primaries(tabs, which)
    pikp_slot, ids = api.stable_slots(t, [211, 321, 2212])           # three slots: every form runs
    kw = dict(slot=pikp_slot, n_slots=3)
    whole, st = device(tabs, which, 1, **kw)
    assert st["n_unbinned"] > 0 and whole["dN_pT"].sum() > 50
    for form in (1, 2):
        h, s2 = device(tabs, which, 1, bins=dict(bc.BINS, kernel_form=form), **kw)
        assert bc.same(h, whole) and s2["n_final"] == st["n_final"] and s2["n_unbinned"] == st["n_unbinned"], form
    n = len(q)
    for cuts in ((0, 100, n), (0, 63, 191, n)):
        parts = [device(tabs, which, 1, lo, hi, **kw) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert bc.same(bc.add([p[0] for p in parts]), whole), cuts
        for k in ("n_final", "n_unbinned", "n_decays", "n_stuck", "n_trials"):
            assert sum(p[1][k] for p in parts) == st[k], k
    again, _ = device(tabs, which, 1, **kw)
    assert bc.same(again, whole)
    # all stable entries: form 0 is the private form on the urqmd table (24 slots) and the global one on the smash table (147)
    full, _ = device(tabs, which, 1)
    full1, _ = device(tabs, which, 1, bins=dict(bc.BINS, kernel_form=1))
    assert bc.same(full, full1)


# ---- 4. the slot map ----
def test_slot_map(tabs):
    t, q, slot, S = primaries(tabs, "every-urqmd-spread")
    out, _, _ = api.decay_particles(t, t["mc_id"], q, seed=SEED, lifetime=1)
    pions, ids = api.stable_slots(t, [211, -211])
    assert list(ids) == [211, -211]
    rel = bc.relabel(out, pions)
    got, st = device(tabs, "every-urqmd-spread", 1, slot=pions, n_slots=2)
    assert st["n_final"] == len(out) and st["n_unbinned"] == len(out) - len(rel) == st["n_final"] - int(got["yield"].sum()) > 0
    assert bc.same(got, api.sampler_bin_list(bc.BINS, bc.N_EVENTS, 2, rel), bc.COUNTS)
    none = np.full(len(slot), -1, np.int32)
    got, st = device(tabs, "every-urqmd-spread", 1, slot=none, n_slots=1)
    assert st["n_unbinned"] == st["n_final"] == len(out) and all(not got[k].any() for k in bc.ALL)
    # the parent without an open channel is final as itself: in no slot unless it is given one
    e = int(np.nonzero(t["mc_id"] == 10333)[0][0])
    assert not t["stable"][e] and slot[e] == -1 and st["n_stuck"] == 1 == int((out["species"] == e).sum())
    own = none.copy()
    own[e] = 0
    got, st = device(tabs, "every-urqmd-spread", 1, slot=own, n_slots=1)
    assert int(got["yield"].sum()) == 1 and st["n_unbinned"] == st["n_final"] - 1
    base, st0 = device(tabs, "every-urqmd-spread", 1)
    assert st0["n_unbinned"] == 1


# ---- 5. form 2 refused where the block does not fit ----
def test_form_2_is_refused_where_the_block_does_not_fit(tabs):
    t, q, slot, S = primaries(tabs, "every-smash")
    assert S * 1800 > 8192 - 6
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        device(tabs, "every-smash", bins=dict(SHIPPED_BINS, kernel_form=2))
    assert e.value.code == api.IS3D_EINVAL and "do not fit" in str(e.value) and api.resource_counters() == before
    pikp_slot, _ = api.stable_slots(t, [211, 321, 2212])
    h2, _ = device(tabs, "every-smash", bins=dict(SHIPPED_BINS, kernel_form=2), slot=pikp_slot, n_slots=3)     # 5400 words
    h1, _ = device(tabs, "every-smash", bins=dict(SHIPPED_BINS, kernel_form=1), slot=pikp_slot, n_slots=3)
    assert bc.same(h2, h1) and h2["dN_pT"].sum() > 0


# ---- 6. the sampler route ----
SAMPLER = dict(CASES, **{"3d_feqmod4": dict(n=400, dim=3, seed=837, df_mode=4, n_events=300, sseed=31337, y_cut=0.9, bins=CASES["3d_ce"]["bins"])})


def sampler_run(fx, tabs, case):
    """Per case, computed once: cells, the thermal list, the host route's decayed histograms, and the plan with its device arrays."""
    import torch
    key = ("sampler", case)
    if key in _cache:
        return _cache[key]
    c = SAMPLER[case]
    cells = synth.synth_surface(c["n"], c["dim"], seed=c["seed"])
    t = tabs[URQMD]
    sp = fx["urqmd"]
    slot, ids = api.stable_slots(t, sp["mc_id"])
    S = len(ids)
    assert 3 < S <= 24
    o = dict(dimension=c["dim"], df_mode=c["df_mode"])
    gla = inputs.feqmod_tables(inputs.surface_average_T(cells) if c["df_mode"] == 4 else 0.15)
    skw = dict(fq=gla, T_avg=gla["T_avg"]) if c["df_mode"] == 4 else {}
    plist, _ = api.sample_particles(cells, sp, fx["df"], gla, o, n_events=c["n_events"], seed=c["sseed"], y_cut=c["y_cut"], **skw)
    out, rel, want, st = bc.host_route(api, t, sp["mc_id"], plist, slot, S, c["bins"], c["n_events"], 0, c["sseed"])
    dev = torch.device("cuda:0")
    tens = {k: torch.from_numpy(np.ascontiguousarray(cells[k])).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    plan = api.SamplerPlan(sp, fx["df"], gla, o, max_cells=c["n"], y_cut=c["y_cut"], **skw)
    table = api.DecayMcTable(t, sp["mc_id"], device=0)
    _cache[key] = dict(c, cells=cells, t=t, sp=sp, slot=slot, S=S, o=o, gla=gla, skw=skw, list=plist, out=out, rel=rel, want=want, st=st, tens=tens,
                       ptrs=ptrs, plan=plan, table=table)
    return _cache[key]


def execute(r, batch_events=0, n_events=None, n_cells=None, bins=None):
    return r["plan"].execute_decayed_binned(n_cells or r["n"], r["ptrs"], n_events or r["n_events"], r["sseed"], bins or r["bins"], len(r["sp"]["mass"]),
                                            r["table"], r["slot"], r["S"], x_ptr=r["ptrs"]["x"], y_ptr=r["ptrs"]["y"], batch_events=batch_events)


@pytest.mark.parametrize("case", list(SAMPLER))
def test_sampler_route_equals_the_host_route_for_every_batching(fx, tabs, case):
    r = sampler_run(fx, tabs, case)
    print(case, "hadrons", len(r["list"]), "finals", len(r["out"]), "binned", len(r["rel"]), "edge distance %.3g" % bc.edge_distance(r["rel"], r["bins"]))
    assert len(r["list"]) > 500 and len(r["out"]) > len(r["list"]) and bc.edge_clear(r["rel"], r["bins"])
    thermal, decayed, st, dst = execute(r)
    bc.assert_parity(decayed, dst, r["want"], r["rel"], r["out"], r["st"])
    assert st["n_particles"] == len(r["list"]) == dst["n_primaries"] and dst["ms_bin"] > 0.0
    assert bc.inside_and_outside(decayed, len(r["rel"]))
    only, st_only = r["plan"].execute_binned(r["n"], r["ptrs"], r["n_events"], r["sseed"], r["bins"], len(r["sp"]["mass"]), x_ptr=r["ptrs"]["x"],
                                             y_ptr=r["ptrs"]["y"])
    assert bc.same(thermal, only) and st_only["n_particles"] == st["n_particles"]
    for be in (1, 7):
        th, de, s2, d2 = execute(r, batch_events=be)
        assert bc.same(de, decayed) and bc.same(th, thermal), be
        for k in ("n_final", "n_unbinned", "n_decays", "n_stuck", "n_trials", "n_exhausted"):
            assert d2[k] == dst[k], k
    de1 = execute(r, bins=dict(r["bins"], kernel_form=1))[1]
    assert bc.same(de1, decayed)
    if case == "3d_ce":                                       # the host-pointer one-shot is the same run
        th, de, s3, d3 = api.sample_decayed_binned(r["cells"], r["sp"], fx["df"], r["gla"], r["bins"], r["t"], r["sp"]["mc_id"], r["slot"], r["S"], r["o"],
                                                   n_events=r["n_events"], seed=r["sseed"], y_cut=r["y_cut"])
        assert bc.same(de, decayed) and bc.same(th, thermal) and d3["n_final"] == dst["n_final"]


def test_sampler_route_with_empty_batches_and_a_single_event(fx, tabs):
    """60 cells and 200 events, one event per batch: most batches hold no hadron (no launch for them); then 3 cells with 1 event."""
    r = sampler_run(fx, tabs, "3d_ce")
    whole = execute(r, n_events=200, n_cells=60)
    assert (whole[0]["yield"] == 0).any() and (whole[0]["yield"] > 0).any() and whole[3]["n_final"] >= whole[2]["n_particles"] > 0
    each = execute(r, batch_events=1, n_events=200, n_cells=60)
    assert bc.same(each[0], whole[0]) and bc.same(each[1], whole[1]) and each[3]["n_final"] == whole[3]["n_final"]
    cells = {k: v[:60] for k, v in r["cells"].items()}
    plist, _ = api.sample_particles(cells, r["sp"], fx["df"], r["gla"], r["o"], n_events=200, seed=r["sseed"], y_cut=r["y_cut"])
    out, rel, want, st = bc.host_route(api, r["t"], r["sp"]["mc_id"], plist, r["slot"], r["S"], r["bins"], 200, 0, r["sseed"])
    assert bc.edge_clear(rel, r["bins"])
    bc.assert_parity(whole[1], whole[3], want, rel, out, st)
    one = execute(r, n_events=1, n_cells=3)
    cells = {k: v[:3] for k, v in r["cells"].items()}
    plist, _ = api.sample_particles(cells, r["sp"], fx["df"], r["gla"], r["o"], n_events=1, seed=r["sseed"], y_cut=r["y_cut"])
    out, rel, want, st = bc.host_route(api, r["t"], r["sp"]["mc_id"], plist, r["slot"], r["S"], r["bins"], 1, 0, r["sseed"])
    assert one[2]["n_particles"] == len(plist) and one[1]["yield"].shape == (1,) and bc.edge_clear(rel, r["bins"])
    if len(plist):
        bc.assert_parity(one[1], one[3], want, rel, out, st)
    else:
        assert one[3]["n_final"] == 0 and not one[1]["yield"].any()


# ---- 7. memory ----
def test_memory_is_one_batch_and_a_second_execute_allocates_nothing(fx, tabs):
    shared = sampler_run(fx, tabs, "3d_ce")
    # a plan of its own: the workspace of a plan keeps the size of the largest batch it has seen
    r = dict(shared, plan=api.SamplerPlan(shared["sp"], fx["df"], shared["gla"], shared["o"], max_cells=shared["n"], y_cut=shared["y_cut"]))
    th, de, st, dst = execute(r, batch_events=1)
    whole = execute(shared)
    assert bc.same(de, whole[1])
    assert 0 < st["particle_workspace_bytes"] <= 96 * int(th["yield"].max()) < 96 * st["n_particles"] // 5
    assert whole[2]["particle_workspace_bytes"] >= 96 * st["n_particles"] > 5 * st["particle_workspace_bytes"]
    p0, a0 = api.resource_counters()
    th2, de2, st2, dst2 = execute(r, batch_events=1)
    assert api.resource_counters() == (p0, a0)
    assert bc.same(de2, de) and bc.same(th2, th) and st2["particle_workspace_bytes"] == st["particle_workspace_bytes"]
    r["plan"].close()


def test_plan_entry_refusals_precede_device_use(fx, tabs):
    r = sampler_run(fx, tabs, "3d_ce")
    before = api.resource_counters()
    bad_slot = r["slot"].copy()
    bad_slot[0] = r["S"]
    other = api.DecayMcTable(r["t"], [211, 321], device=0)
    mid = api.resource_counters()
    plan, n_sp, ptrs = r["plan"], len(r["sp"]["mass"]), r["ptrs"]
    for kw in (dict(slot=bad_slot), dict(n_slots=0), dict(bins=dict(r["bins"], kernel_form=3)), dict(bins=dict(r["bins"], pT_bins=0)), dict(table=other)):
        with pytest.raises(api.Is3dError) as e:
            plan.execute_decayed_binned(r["n"], ptrs, r["n_events"], r["sseed"], kw.get("bins", r["bins"]), n_sp, kw.get("table", r["table"]),
                                        kw.get("slot", r["slot"]), kw.get("n_slots", r["S"]))
        assert e.value.code == api.IS3D_EINVAL, kw
    assert api.resource_counters() == mid and mid[0] == before[0]
    other.close()


# ---- 8. the driver ----
def test_driver_writes_the_decayed_distributions_beside_the_thermal_ones(tmp_path, reference, tabs):
    """a 2+1D toy run with test_sampler_on_device, with and without test_sampler_decayed: results/ is byte-identical, results/decayed/ holds the
    files of is3d_write_sampler_tests_binned on the host route's histograms for the chosen species that are stable, in chosen order"""
    ids = [211, 321, 2212, 113, 223, 2224, -2224, 221, -211]
    cells = synth.synth_surface(3000, 2, seed=92)
    t = tabs[URQMD]
    sub = ("dN_dy", "dN_deta", "momentum_distribution", "vn", "spacetime_distribution")
    files, stdout, roots = {}, {}, {}
    for key in (0, 1):
        root = refformat.make_run_dir(str(tmp_path / ("key%d" % key)), cells, ids, dict(operation=2, dimension=2, df_mode=2, sampler_seed=17, oversample=1,
                                                                                            min_num_hadrons=2000, test_sampler=1))
        shutil.copy(os.path.join(reference, "PDG", URQMD), os.path.join(root, "PDG", URQMD))     # the shipped list: the toy one has no decay data
        with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
            f.write("test_sampler_on_device\t= 1\n" + ("test_sampler_decayed\t= 1\n" if key else ""))
        for d in sub:
            os.makedirs(os.path.join(root, "results", d), exist_ok=True)
            if key:
                os.makedirs(os.path.join(root, "results", "decayed", d))
        r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        files[key] = {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), "rb").read()
                      for dp, _, fs in os.walk(os.path.join(root, "results")) for f in fs}
        stdout[key], roots[key] = r.stdout, root
    thermal = {k: v for k, v in files[1].items() if not k.startswith(os.path.join("results", "decayed"))}
    decayed = {os.path.relpath(k, os.path.join("results", "decayed")): v for k, v in files[1].items() if k not in thermal}
    assert thermal == files[0] and len(thermal) > 10 and len(decayed) > 10
    line = [ln for ln in stdout[1].split("\n") if ln.startswith("decayed and binned on the device:")]
    assert len(line) == 1 and all(w in line[0] for w in ("n_final", "n_unbinned", "n_decays", "n_stuck", "n_exhausted", "ms_bin")) and "decayed and binned" not in stdout[0]
    # the host route on the run's own list: the embedding entry of the same run directory with test_sampler = 0 returns it
    slot, slot_ids = api.stable_slots(t, ids)
    assert list(slot_ids) == [211, 321, 2212, -211]
    root2 = refformat.make_run_dir(str(tmp_path / "list"), cells, ids, dict(operation=2, dimension=2, df_mode=2, sampler_seed=17, oversample=1,
                                                                               min_num_hadrons=2000, test_sampler=0))
    shutil.copy(os.path.join(reference, "PDG", URQMD), os.path.join(root2, "PDG", URQMD))
    L = api.load()
    L.is3d_run_particlization.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RunResult)]
    res = RunResult()
    cwd = os.getcwd()
    os.chdir(root2)
    try:
        assert L.is3d_run_particlization(None, None, None, 0, C.byref(res)) == 0
    finally:
        os.chdir(cwd)
    n_events = int(res.n_events)
    plist = np.frombuffer(C.string_at(res.particles, res.n_particles * api.PARTICLE_DTYPE.itemsize), dtype=api.PARTICLE_DTYPE).copy()
    L.is3d_run_result_free(C.byref(res))
    par = os.path.join(roots[1], "iS3D_parameters.dat")
    bins = {k: api.param_get(par, k.lower()) for k in ("y_cut", "eta_cut", "pT_lower_cut", "pT_upper_cut", "tau_min", "tau_max", "r_min", "r_max")}
    bins.update({k: int(api.param_get(par, k)) for k in ("y_bins", "eta_bins", "pt_bins", "tau_bins", "r_bins")})
    bins["pT_bins"] = bins.pop("pt_bins")
    assert len(plist) > 1000 and n_events == len(files[1][os.path.join("results", "yield_list.dat")].split(b"\n")) - 2
    out, rel, want, st = bc.host_route(api, t, ids, plist, slot, len(slot_ids), bins, n_events, 0, 17)
    assert bc.edge_clear(rel, bins) and len(out) > len(plist)
    assert ("n_final %d, n_unbinned %d, n_decays %d, n_stuck %d" % (len(out), len(out) - len(rel), st["n_decays"], st["n_stuck"])) in line[0]
    mean_yield = float(files[1][os.path.join("results", "mean_yield.dat")])
    lib = tmp_path / "lib"
    for d in sub:
        os.makedirs(lib / d)
    api.write_sampler_tests_binned(str(lib), bins, n_events, slot_ids, want, mean_yield)
    written = {os.path.relpath(os.path.join(dp, f), str(lib)): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(str(lib)) for f in fs}
    assert sorted(written) == sorted(decayed)
    for k in written:
        if not k.startswith("vn"):                            # counts and yields are exact, so these files are equal byte for byte
            assert written[k] == decayed[k], k
    # vn/: the harmonic sums may differ by one fixed-point unit per entry (device against host libm), 2^-32 in v_n before the printed digits
    for k in (k for k in written if k.startswith("vn")):
        a, b = np.loadtxt(lib / k, ndmin=2), np.loadtxt(os.path.join(roots[1], "results", "decayed", k), ndmin=2)
        assert a.shape == b.shape and np.allclose(a, b, rtol=0.0, atol=2.0 ** -31 + 1e-6 * np.abs(a).max()), k
    # a missing directory is named
    shutil.rmtree(os.path.join(roots[1], "results", "decayed", "vn"))
    r = subprocess.run([api.CLI_PATH], cwd=roots[1], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "results/decayed/vn" in r.stderr and "test_sampler_decayed" in r.stderr, r.stderr
