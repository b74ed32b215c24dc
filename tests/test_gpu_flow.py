"""GPU (-m gpu): the per-event flow records on the device (cf_sampler_flow, every form) against the host route is3d_flow_list on lists made
by hand (tests/flow_cases.py).  M must be equal exactly, every Q word within M units of its record (device against host libm), and forms 0, 1
and 2 must give identical bits.

The lists: event sizes 1, 63, 64, 65, 0, 257 and a tail of 200 events of one or two particles (event boundaries at lane 0, at lane 63 and
mid-workgroup, an empty event, an event across the workgroups of the global form, more events in one slice than any window holds); the same
list shuffled; 9001 particles in 5 uneven events (three slices of the private form, crossed by events); particles out of range.  Slots: 1 and
3 with slot -1 present, 40 (a window of 4 events), and 161, the first count at which not even one event's records (161 x 51 = 8211 words) fit
the 8192 words of LDS: form 0 runs the global form there and form 2 is refused.

The decay sink (cf_decay_mc_flow) against its host route -- is3d_decay_particles, then is3d_flow_list on the decayed list with the slot map
over the table's entries -- on hand_list and every_unstable of tests/decays_mc_cases.py (7 events), lifetime 0 and 1, every form, and the list
in three pieces with first_particle; and against physics the restatement cannot vouch for: a rho0 at rest gives two pions back to back, so
c_n{2} of 50 such events is (-1)^n.

The sampler route (is3d_sampler_plan_execute_flow, is3d_sample_flow): 400 cells x 30 events, the shape of tests/test_gpu_sampler_fused.py, pi+
alone and pi+ with rho0 and omega (so that the decay pass has something to decay); the records must be those of the list the plan's execute
returns, at batch_events 1, 7 and 0, the decayed ones those of is3d_decay_particles_flow on that list, and the plan's older entries must return
afterwards what they returned before.  And the independence condition of tests/test_flow_host.py on the device sampler's own list.

The run driver: test_sampler_flow = 1 beside test_sampler_on_device = 1, and beside test_sampler_decayed = 1 too, writes the flow files and
leaves every other file byte for byte what the run without the key writes."""
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import decays_mc_cases as cases
import decays_mc_ref as ref
import flow_cases as F
import refformat
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2)
LISTS = dict(hand=F.hand_list, shuffled=F.shuffled_list, long=F.long_list)


@lru_cache(maxsize=None)
def host_records(name, n_slots):
    p, n_events = LISTS[name]()
    n_species = 162 if n_slots > F.N_SPECIES else F.N_SPECIES
    slot = F.slot_map(n_slots, n_species)
    want = api.flow_list(F.CUTS, n_events, n_slots, slot, p)
    assert np.array_equal(want["M"], F.numpy_M(F.CUTS, n_events, n_slots, slot, p))
    for v in want.values():
        v.setflags(write=False)
    return p, n_events, slot, want


@pytest.mark.parametrize("n_slots", (1, 3, 40))
@pytest.mark.parametrize("name", sorted(LISTS))
def test_flow_list_device_is_the_host_route_in_every_form(name, n_slots):
    p, n_events, slot, want = host_records(name, n_slots)
    assert (slot == -1).any() and want["M"][:, :, 1].sum() > 0 and want["M"][:, :, 2].sum() > 0 and (want["M"][:, :, 0] > want["M"][:, :, 1]).any()
    got = {}
    for form in FORMS:
        got[form], skipped = api.flow_list_device(dict(F.CUTS, kernel_form=form), n_events, n_slots, slot, p)
        assert skipped == 0
        F.assert_records(got[form], want, (name, n_slots, form))
    assert F.same_bits(got[0], got[1]) and F.same_bits(got[0], got[2]), (name, n_slots)


def test_records_that_fit_no_window_take_the_global_form():
    """161 slots: form 0 and form 1 agree bit for bit and with the host; form 2 is refused before any device use."""
    p, n_events, slot, want = host_records("hand", 161)
    g0, _ = api.flow_list_device(dict(F.CUTS, kernel_form=0), n_events, 161, slot, p)
    g1, _ = api.flow_list_device(dict(F.CUTS, kernel_form=1), n_events, 161, slot, p)
    F.assert_records(g0, want, "161 slots")
    assert F.same_bits(g0, g1)
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        api.flow_list_device(dict(F.CUTS, kernel_form=2), n_events, 161, slot, p)
    assert e.value.code == api.IS3D_EINVAL and "8211 words" in str(e.value)
    assert api.resource_counters() == before


def test_particles_out_of_range_add_nothing_and_are_counted():
    p, n_events, slot, want = host_records("hand", 3)
    q = np.concatenate([p[:100], p[:4], p[100:], p[:3]])
    q["species"][100:102] = (F.N_SPECIES, -1)
    q["event"][102:104] = (n_events, -1)
    q["event"][-3:] = (-5, n_events + 7, 2 ** 31 - 1)
    for form in FORMS:
        got, skipped = api.flow_list_device(dict(F.CUTS, kernel_form=form), n_events, 3, slot, q)
        assert skipped == 7
        F.assert_records(got, want, ("out of range", form))
    with pytest.raises(api.Is3dError) as e:
        api.flow_list(F.CUTS, n_events, 3, slot, q)
    assert e.value.code == api.IS3D_EINVAL


def test_pieces_of_a_list_add_to_the_whole_and_an_empty_list_is_zero():
    p, n_events, slot, _ = host_records("long", 3)
    whole, _ = api.flow_list_device(F.CUTS, n_events, 3, slot, p)
    parts = [api.flow_list_device(F.CUTS, n_events, 3, slot, p[a:b])[0] for a, b in ((0, 1), (1, 4500), (4500, len(p)))]
    assert all(np.array_equal(sum(q[k] for q in parts), whole[k]) for k in whole)
    empty, skipped = api.flow_list_device(F.CUTS, n_events, 3, slot, p[:0])
    assert skipped == 0 and all(not v.any() for v in empty.values())


# ---- the decay sink ----
URQMD = "pdg-urqmd_v3.3+.dat"
N_DECAY_EVENTS = 7            # hand_list: 257 // 40 + 1; every_unstable: 303 // 50 + 1
TALLIES = ("n_primaries", "n_decays", "n_final", "n_stuck", "n_trials", "n_exhausted", "max_stack", "max_depth", "n_closed_channels")
_cache = {}


@pytest.fixture(scope="module")
def table(reference):
    return cases.tables(api, reference)[URQMD]


def primaries(table, which):
    if which not in _cache:
        _cache[which] = cases.hand_list(api, table, ref.prepare(table)) if which == "hand" else cases.every_unstable(api, table, 3)
    return _cache[which]


def decay_host_route(table, which, lifetime, slot, n_slots):
    """(decayed list, its host records, the stats of is3d_decay_particles): computed once per case, never written to"""
    key = (which, lifetime, n_slots)
    if key not in _cache:
        out, _, st = api.decay_particles(table, table["mc_id"], primaries(table, which), seed=cases.SEED, lifetime=lifetime)
        assert F.edge_distance(F.CUTS, out) > 1e-9
        _cache[key] = (out, api.flow_list(F.CUTS, N_DECAY_EVENTS, n_slots, slot, out), st)
    return _cache[key]


def slots_of(table, kind):
    """every stable entry a slot of its own (24: a window of 6 of the 7 events) | pi+, K+, p (three slots: every event in the window)"""
    slot, ids = api.stable_slots(table) if kind == "stable" else api.stable_slots(table, [211, 321, 2212])
    return slot, len(ids)


@pytest.mark.parametrize("kind", ("stable", "pikp"))
@pytest.mark.parametrize("lifetime", (0, 1))
@pytest.mark.parametrize("which", ("hand", "every"))
def test_decay_particles_flow_is_the_host_route(table, which, lifetime, kind):
    slot, S = slots_of(table, kind)
    q = primaries(table, which)
    out, want, st = decay_host_route(table, which, lifetime, slot, S)
    kept = int(want["M"][:, :, 0].sum())
    assert 50 < kept < len(out) and want["M"][:, :, 1].sum() > 0 and want["M"][:, :, 2].sum() > 0
    got = {}
    for form in FORMS:
        got[form], dst = api.decay_particles_flow(table, table["mc_id"], q, slot, S, dict(F.CUTS, kernel_form=form), N_DECAY_EVENTS, seed=cases.SEED,
                                                  lifetime=lifetime)
        F.assert_records(got[form], want, (which, lifetime, kind, form))
        assert dst["n_final"] == len(out) and dst["n_unbinned"] == len(out) - kept
        assert all(dst[k] == st[k] for k in TALLIES), {k: (dst[k], st[k]) for k in TALLIES}
        assert dst["ms_bin"] > 0.0 and dst["ms_count"] == dst["ms_fill"] == 0.0
    assert F.same_bits(got[0], got[1]) and F.same_bits(got[0], got[2])
    # the list in three pieces with first_particle: the records and the tallies add
    n = len(q)
    parts = [api.decay_particles_flow(table, table["mc_id"], q[lo:hi], slot, S, F.CUTS, N_DECAY_EVENTS, seed=cases.SEED, lifetime=lifetime,
                                      first_particle=lo) for lo, hi in ((0, 63), (63, 191), (191, n))]
    assert all(np.array_equal(sum(r[k] for r, _ in parts), got[0][k]) for k in got[0])
    for k in ("n_final", "n_unbinned", "n_decays", "n_stuck", "n_trials"):
        assert sum(d[k] for _, d in parts) == dst[k], k


def test_decay_flow_refusals_and_the_empty_list(table):
    slot, S = slots_of(table, "pikp")
    q = primaries(table, "hand")
    before = api.resource_counters()
    bad_event = q.copy()
    bad_event["event"][5] = N_DECAY_EVENTS
    for kw in (dict(cuts=dict(F.CUTS, y_gap=2.0)), dict(cuts=dict(F.CUTS, kernel_form=3)), dict(n_slots=0), dict(n_slots=2), dict(n_events=0), dict(q=bad_event),
               dict(slot=np.minimum(np.arange(len(slot)), 160).astype(np.int32), n_slots=161, cuts=dict(F.CUTS, kernel_form=2))):
        a = dict(q=q, slot=slot, n_slots=S, cuts=F.CUTS, n_events=N_DECAY_EVENTS)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_flow(table, table["mc_id"], a["q"], a["slot"], a["n_slots"], a["cuts"], a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    assert api.resource_counters() == before
    r, st = api.decay_particles_flow(table, table["mc_id"], q[:0], slot, S, F.CUTS, N_DECAY_EVENTS)
    assert st["n_final"] == st["n_unbinned"] == 0 and all(not v.any() for v in r.values())


def test_a_rho0_at_rest_gives_two_pions_back_to_back():
    """Physics the restatement cannot vouch for: 50 events of one rho0 at rest, both pions in one slot -- M = 2 in every event and
    <2> = cos(n pi), so c_n{2} = (-1)^n within 1e-8 (a term is off by at most 2^-33 plus libm's ulps; the denominator is 2)."""
    t = cases.hand_table([cases.stable(211, 0.13957), cases.stable(-211, 0.13957), (113, 0.77526, 0.1491, 0, [(2, 1.0, [211, -211])])])
    q = ref.make_particles(api, t, t["mc_id"], [2] * 50, np.zeros((50, 3)), events=np.arange(50))
    wide = dict(y_cut=5.0, y_gap=0.5, pT_min=0.0, pT_max=100.0)
    for form in FORMS:
        r, st = api.decay_particles_flow(t, t["mc_id"], q, [0, 0, -1], 1, dict(wide, kernel_form=form), 50, seed=9)
        assert st["n_final"] == 100 and st["n_unbinned"] == 0 and np.all(r["M"][:, 0, 0] == 2)
        c = api.flow_cumulants(r)
        assert c["n_used_2"][0] == 50 and np.abs(c["c2"][0] - (-1.0) ** np.arange(1, 9)).max() < 1e-8, c["c2"][0]


# ---- the sampler route ----
SAMPLER_BINS = dict(y_cut=1.5, eta_cut=4.0, pT_lower_cut=0.25, pT_upper_cut=2.75, tau_min=1.0, tau_max=9.0, r_min=0.5, r_max=8.0,
                    y_bins=12, eta_bins=16, pT_bins=10, tau_bins=8, r_bins=15)
SPECIES = {"pi+": [211], "pi+ rho0 omega": [211, 113, 223]}


@pytest.fixture(scope="module")
def sampler_case(fx, table):
    import torch
    made = {}

    def make(name):
        if name not in made:
            sp, gla, o = inputs.species(SPECIES[name]), inputs.feqmod_tables(0.15), dict(dimension=3, df_mode=2)
            cells = {k: v.copy() for k, v in synth.synth_surface(400, 3, seed=861).items()}
            for f in ("dat", "dax", "day", "dan"):
                cells[f] *= 50.0
            kw = dict(n_events=30, seed=19, y_cut=0.5)
            plist, lst = api.sample_particles(cells, sp, fx["df"], gla, o, **kw)
            dev = torch.device("cuda:0")
            tens = {k: torch.from_numpy(np.ascontiguousarray(cells[k])).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
            ptrs = {k: v.data_ptr() for k, v in tens.items()}
            S = len(sp["mass"])
            slot = np.arange(S, dtype=np.int32)
            slot_d, ids = api.stable_slots(table, [211, -211, 111])
            made[name] = dict(sp=sp, gla=gla, o=o, cells=cells, kw=kw, list=plist, tens=tens, ptrs=ptrs, S=S, slot=slot, slot_d=slot_d, S_d=len(ids),
                              plan=api.SamplerPlan(sp, fx["df"], gla, o, max_cells=400, y_cut=0.5), dtable=api.DecayMcTable(table, sp["mc_id"], device=0),
                              want=api.flow_list(F.CUTS, 30, S, slot, plist))
        return made[name]

    yield make
    for r in made.values():
        r["plan"].close()


def run_flow(r, batch_events=0, decayed=True, cuts=F.CUTS, **over):
    a = dict(slot=r["slot"], n_slots=r["S"], slot_decayed=r["slot_d"], n_slots_decayed=r["S_d"], table=r["dtable"] if decayed else None)
    a.update(over)
    return r["plan"].execute_flow(400, r["ptrs"], 30, 19, cuts, a["slot"], a["n_slots"], table=a["table"], slot_decayed=a["slot_decayed"],
                                  n_slots_decayed=a["n_slots_decayed"], decay_seed=77, lifetime=1, x_ptr=r["ptrs"]["x"], y_ptr=r["ptrs"]["y"],
                                  batch_events=batch_events)


@pytest.mark.parametrize("name", list(SPECIES))
def test_execute_flow_is_flow_list_of_the_list_for_every_batching(table, sampler_case, name):
    r = sampler_case(name)
    assert len(r["list"]) >= 200 and r["want"]["M"][:, :, 0].sum() > 100
    want_d, dst_want = api.decay_particles_flow(table, r["sp"]["mc_id"], r["list"], r["slot_d"], r["S_d"], F.CUTS, 30, seed=77, lifetime=1, first_particle=0)
    if name != "pi+":
        assert dst_want["n_decays"] > 0 and dst_want["n_final"] > len(r["list"])
    first = None
    for batch_events in (1, 7, 0):
        rec, rec_d, st, dst = run_flow(r, batch_events)
        F.assert_records(rec, r["want"], (name, batch_events))
        assert st["n_particles"] == len(r["list"]) == dst["n_primaries"]
        assert F.same_bits(rec_d, want_d), (name, batch_events)
        assert all(dst[k] == dst_want[k] for k in ("n_final", "n_unbinned", "n_decays", "n_stuck", "n_trials", "n_exhausted")), (dst, dst_want)
        first = first or (rec, rec_d)
        assert F.same_bits(rec, first[0]) and F.same_bits(rec_d, first[1])
    for form in (1, 2):
        rec, rec_d, _, _ = run_flow(r, 7, cuts=dict(F.CUTS, kernel_form=form))
        assert F.same_bits(rec, first[0]) and F.same_bits(rec_d, first[1]), form
    only, st = run_flow(r, 0, decayed=False)
    assert F.same_bits(only, first[0]) and st["n_particles"] == len(r["list"])


def test_the_plans_older_entries_return_what_they_returned_before(table, sampler_case):
    import torch
    r = sampler_case("pi+ rho0 omega")
    plan, ptrs, S = r["plan"], r["ptrs"], r["S"]
    slot_b, ids = api.stable_slots(table, [211, -211, 111])

    def older():
        buf = torch.zeros(len(r["list"]) * api.PARTICLE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        n, _ = plan.execute(400, ptrs, 30, 19, particles_ptr=buf.data_ptr(), capacity=len(r["list"]), x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        lst = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=api.PARTICLE_DTYPE)[:n]
        binned, _ = plan.execute_binned(400, ptrs, 30, 19, SAMPLER_BINS, S, x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        th, de, _, dst = plan.execute_decayed_binned(400, ptrs, 30, 19, SAMPLER_BINS, S, r["dtable"], slot_b, len(ids), x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        return lst, binned, th, de, dst["n_final"]

    before = older()
    assert np.array_equal(before[0], r["list"])
    run_flow(r, 7)
    after = older()
    assert np.array_equal(before[0], after[0]) and before[4] == after[4]
    for a, b in zip(before[1:4], after[1:4]):
        assert all(np.array_equal(a[k], b[k]) for k in a)
    rec, rec_d, _, _ = run_flow(r, 0)
    F.assert_records(rec, r["want"], "after the older entries")


def test_execute_flow_refusals_leave_the_resource_counters_unmoved(table, sampler_case):
    r = sampler_case("pi+")
    run_flow(r, 0)
    other = api.DecayMcTable(table, [211, 321], device=0)
    before = api.resource_counters()
    bad_d = r["slot_d"].copy()
    bad_d[0] = r["S_d"]
    for kw in (dict(cuts=dict(F.CUTS, y_cut=0.0)), dict(cuts=dict(F.CUTS, kernel_form=3)), dict(slot=np.array([1], np.int32)), dict(n_slots=0),
               dict(slot_decayed=bad_d), dict(n_slots_decayed=0), dict(table=other), dict(n_slots=161, cuts=dict(F.CUTS, kernel_form=2))):
        with pytest.raises(api.Is3dError) as e:
            run_flow(r, 0, **kw)
        assert e.value.code == api.IS3D_EINVAL, kw
    assert api.resource_counters() == before


def test_sample_flow_is_execute_flow_and_the_device_samplers_hadrons_are_independent(fx, table, sampler_case):
    r = sampler_case("pi+ rho0 omega")
    rec, rec_d, st, dst = api.sample_flow(r["cells"], r["sp"], fx["df"], r["gla"], F.CUTS, r["slot"], r["S"], r["o"], table=table, chosen_mc_id=r["sp"]["mc_id"],
                                          slot_decayed=r["slot_d"], n_slots_decayed=r["S_d"], decay_seed=77, lifetime=1, batch_events=7, **r["kw"])
    want, want_d, _, dst_want = run_flow(r, 0)
    assert F.same_bits(rec, want) and F.same_bits(rec_d, want_d) and dst["n_final"] == dst_want["n_final"] and st["n_particles"] == len(r["list"])
    # the independence condition of tests/test_flow_host.py (same surface, events and seed) on the list the DEVICE sampler makes
    cells, sp, gla, o, kw = F.thermal_surface()
    thermal, st = api.sample_flow(cells, sp, fx["df"], gla, F.CUTS, [0], 1, o, **kw)
    pulls = F.independence_pulls(thermal)
    print("pulls of the device sampler's list", pulls)
    assert all(abs(v) <= 5.0 for v in pulls.values()), pulls


# ---- the run driver ----
def test_driver_writes_the_flow_files_and_leaves_every_other_file_as_it_was(tmp_path, reference):
    """A 2+1D toy run (the one of tests/test_gpu_decays_mc_bins.py) four times: with and without test_sampler_decayed, each with and without
    test_sampler_flow.  Without the flow files the results of a run with the key are those of the run without it, byte for byte; the flow
    files are cumulants_ and multiplicity_ of 211, 321, 2212, other and all; "all" is the sum of the slots; the thermal flow files do not
    depend on test_sampler_decayed; the decayed ones hold the stable chosen species only, with more pions than the thermal ones."""
    ids = [211, 321, 2212, 113, 223, 2224, -2224, 221, -211]
    cells = synth.synth_surface(3000, 2, seed=92)
    sub = ("dN_dy", "dN_deta", "momentum_distribution", "vn", "spacetime_distribution")
    files, stdout = {}, {}
    for decayed in (0, 1):
        for flow in (0, 1):
            root = refformat.make_run_dir(str(tmp_path / ("d%d_f%d" % (decayed, flow))), cells, ids,
                                          dict(operation=2, dimension=2, df_mode=2, sampler_seed=17, oversample=1, min_num_hadrons=2000, test_sampler=1))
            shutil.copy(os.path.join(reference, "PDG", URQMD), os.path.join(root, "PDG", URQMD))     # the shipped list: the toy one has no decay data
            with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
                f.write("test_sampler_on_device\t= 1\n" + ("test_sampler_decayed\t= 1\n" if decayed else "") +
                        ("test_sampler_flow\t= 1\nflow_y_cut = 0.4\nflow_y_gap = 0.2\nflow_pT_min = 0.1\n" if flow else ""))
            for d in sub + (("flow",) if flow else ()):
                os.makedirs(os.path.join(root, "results", d), exist_ok=True)
                if decayed:
                    os.makedirs(os.path.join(root, "results", "decayed", d))
            r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
            files[decayed, flow] = {os.path.relpath(os.path.join(dp, f), os.path.join(root, "results")): open(os.path.join(dp, f), "rb").read()
                                    for dp, _, fs in os.walk(os.path.join(root, "results")) for f in fs}
            stdout[decayed, flow] = r.stdout
    is_flow = lambda k: k.startswith("flow" + os.sep) or k.startswith(os.path.join("decayed", "flow") + os.sep)  # noqa: E731
    for decayed in (0, 1):
        rest = {k: v for k, v in files[decayed, 1].items() if not is_flow(k)}
        assert rest == files[decayed, 0] and len(rest) > 10
        assert "flow records on the device" in stdout[decayed, 1] and "flow records" not in stdout[decayed, 0]
    labels = ("211", "321", "2212", "other", "all")
    names = sorted(os.path.join("flow", "%s_%s.dat" % (k, l)) for k in ("cumulants", "multiplicity") for l in labels)
    assert sorted(k for k in files[0, 1] if is_flow(k)) == names
    thermal = {k: v for k, v in files[1, 1].items() if k.startswith("flow" + os.sep)}
    assert thermal == {k: files[0, 1][k] for k in names}
    stable = ("211", "321", "2212", "other", "all")                   # 211, 321, 2212 and -211 (other) are stable in the table
    assert sorted(k for k in files[1, 1] if k.startswith(os.path.join("decayed", "flow"))) == sorted(os.path.join("decayed", n) for n in names)
    assert stable == labels

    def mult(run, name):
        return np.loadtxt(tmp_path / run / "results" / name)

    for run, base_dir in (("d0_f1", "flow"), ("d1_f1", os.path.join("decayed", "flow"))):
        parts = [mult(run, os.path.join(base_dir, "multiplicity_%s.dat" % l)) for l in labels[:-1]]
        whole = mult(run, os.path.join(base_dir, "multiplicity_all.dat"))
        assert np.array_equal(sum(p[:, 1:] for p in parts), whole[:, 1:]) and whole[:, 1].sum() > 100 and whole[:, 2].sum() > 0 and whole[:, 3].sum() > 0
        c = np.loadtxt(tmp_path / run / "results" / base_dir / "cumulants_all.dat")
        assert c.shape == (8, 8) and np.all(np.isfinite(c)) and np.all(np.abs(c[:, 1]) < 1.0)
    pions_thermal = mult("d1_f1", os.path.join("flow", "multiplicity_211.dat"))[:, 1].sum()
    pions_decayed = mult("d1_f1", os.path.join("decayed", "flow", "multiplicity_211.dat"))[:, 1].sum()
    assert pions_decayed > pions_thermal > 0                            # the rho0, omega, Delta++ and eta feed the pi+
