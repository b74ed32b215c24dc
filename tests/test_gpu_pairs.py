"""GPU (-m gpu): the two-particle (delta y, delta phi) histograms on the device (cf_pair_cells, cf_pair_correlate: no loop over particle
pairs) against the host route is3d_pairs_list, the explicit double loop.  Every comparison of histograms and M is array_equal: the counts are
integers and the rule of csrc/cf_sampler_pairs.h reaches the same cell on both sides.

The lists (tests/pairs_cases.py): event sizes 0, 1, 2, 63, 64, 65, 257 and a tail of 200 one-particle events; the same list shuffled; 1, 3
and 10 slots (1, 6 and 55 classes) with slot -1 present; particles out of range; grids (n_y, n_phi) = (1, 4), (2, 12), (33, 20) and (64, 64),
the last with 127 x 64 bins (more than one bin per thread, the full 48 KiB of LDS); 1, 2 and 3 events for the cyclic partner of the mixed
pairs.  One event of 70 000 identical particles against the closed form: 70000 x 69999 > 2^32 in one bin.

The decay sink (cf_decay_mc_pairs) against its host route -- is3d_decay_particles, then is3d_pairs_list on the decayed list with the slot map
over the table's entries -- at lifetime 0 and 1 and in pieces with first_particle; and against physics no restatement vouches for: the two
pions of a rho0 at rest are back to back, so every (pi+, pi-) pair of one primary lands at delta phi = n_phi / 2.

The sampler route (is3d_sampler_plan_execute_pairs, is3d_sample_pairs) at batch_events 1, 7 and 0: equal to each other and to pairs_list of
the list the plan's execute returns; the plan's older entries unchanged afterwards; the independence condition of tests/test_pairs_host.py on
the device sampler's own list."""
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import decays_mc_cases as cases
import decays_mc_ref as ref
import flow_cases as F
import pairs_cases as P
import refformat
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu

LISTS = dict(hand=P.hand_list, shuffled=P.shuffled_list)


@lru_cache(maxsize=None)
def host_hist(n_slots, shape):
    """The host route on hand_list (the shuffled list has the same histograms), checked against the independent count; computed once."""
    p, n_events = P.hand_list()
    slot, bins = P.slot_map(n_slots), P.bins_of(shape)
    want = api.pairs_list(bins, n_events, n_slots, slot, p)
    assert P.same_hist(want, P.numpy_hist(bins, n_events, n_slots, slot, p))
    for v in want.values():
        v.setflags(write=False)
    return slot, bins, want


@pytest.mark.parametrize("shape", P.SHAPES)
@pytest.mark.parametrize("n_slots", (1, 3, 10))
@pytest.mark.parametrize("name", sorted(LISTS))
def test_pairs_list_device_is_the_host_route(name, n_slots, shape):
    p, n_events = LISTS[name]()
    slot, bins, want = host_hist(n_slots, shape)
    assert (slot == -1).any() and want["same"].sum() > 1000 and want["mixed"].sum() > 100 and 0 < want["M"].sum() < len(p)
    got, skipped = api.pairs_list_device(bins, n_events, n_slots, slot, p)
    assert skipped == 0
    for k in ("M", "same", "mixed"):
        assert np.array_equal(got[k], want[k]), (name, n_slots, shape, k)


@pytest.mark.parametrize("n_events", (1, 2, 3))
def test_one_two_and_three_events_mix_with_their_cyclic_partner(n_events):
    p, _ = P.few_events(n_events)
    slot, bins = P.slot_map(3), P.bins_of((33, 20))
    want = api.pairs_list(bins, n_events, 3, slot, p)
    assert want["mixed"].any() == (n_events >= 2)
    got, _ = api.pairs_list_device(bins, n_events, 3, slot, p)
    assert P.same_hist(got, want)


def test_particles_out_of_range_add_nothing_and_are_counted():
    p, n_events = P.hand_list()
    slot, bins, want = host_hist(3, (33, 20))
    q = np.concatenate([p[:100], p[:4], p[100:], p[:3]])
    q["species"][100:102] = (P.N_SPECIES, -1)
    q["event"][102:104] = (n_events, -1)
    q["event"][-3:] = (-5, n_events + 7, 2 ** 31 - 1)
    got, skipped = api.pairs_list_device(bins, n_events, 3, slot, q)
    assert skipped == 7 and P.same_hist(got, want)
    with pytest.raises(api.Is3dError) as e:
        api.pairs_list(bins, n_events, 3, slot, q)
    assert e.value.code == api.IS3D_EINVAL
    empty, skipped = api.pairs_list_device(bins, n_events, 3, slot, p[:0])
    assert skipped == 0 and all(not v.any() for v in empty.values())


def test_a_product_of_two_occupancies_beyond_32_bits():
    """Two events of 70 000 identical particles in one slot: same[n_y - 1][0] = 2 x 70000 x 69999 and mixed[n_y - 1][0] = 2 x 70000^2, each
    term above 2^32; every other bin zero.  (The host double loop is not run on this list.)"""
    N = 70000
    p = np.repeat(P.at(0.3, 1.0), 2 * N)
    p["event"][N:] = 1
    bins = P.bins_of((2, 12))
    got, _ = api.pairs_list_device(bins, 2, 1, [0], p)
    assert got["M"].tolist() == [[N], [N]]
    assert got["same"][0, 1, 0] == 2 * N * (N - 1) == got["same"].sum() and N * (N - 1) > 2 ** 32
    assert got["mixed"][0, 1, 0] == 2 * N * N == got["mixed"].sum()
    one, _ = api.pairs_list_device(bins, 1, 1, [0], p[:N])
    assert one["same"][0, 1, 0] == N * (N - 1) == 4899930000 and not one["mixed"].any()


# ---- the decay sink ----
URQMD = "pdg-urqmd_v3.3+.dat"
N_DECAY_EVENTS = 7
TALLIES = ("n_primaries", "n_decays", "n_final", "n_stuck", "n_trials", "n_exhausted", "max_stack", "max_depth", "n_closed_channels")
DECAY_BINS = P.bins_of((8, 12), y_cut=3.0, pT_min=0.0, pT_max=10.0)
_cache = {}


@pytest.fixture(scope="module")
def table(reference):
    return cases.tables(api, reference)[URQMD]


def primaries(table):
    if "hand" not in _cache:
        _cache["hand"] = cases.hand_list(api, table, ref.prepare(table))
    return _cache["hand"]


@pytest.mark.parametrize("lifetime", (0, 1))
def test_decay_particles_pairs_is_the_host_route(table, lifetime):
    slot, ids = api.stable_slots(table, [211, -211, 321])
    S, q = len(ids), primaries(table)
    out, _, st = api.decay_particles(table, table["mc_id"], q, seed=cases.SEED, lifetime=lifetime)
    assert P.edge_distance(DECAY_BINS, out) > 1e-9
    want = api.pairs_list(DECAY_BINS, N_DECAY_EVENTS, S, slot, out)
    kept = int(want["M"].sum())
    assert 50 < kept < len(out) and want["same"].sum() > 100 and want["mixed"].sum() > 100
    got, dst = api.decay_particles_pairs(table, table["mc_id"], q, slot, S, DECAY_BINS, N_DECAY_EVENTS, seed=cases.SEED, lifetime=lifetime)
    assert P.same_hist(got, want)
    assert dst["n_final"] == len(out) and dst["n_unbinned"] == len(out) - kept
    assert all(dst[k] == st[k] for k in TALLIES), {k: (dst[k], st[k]) for k in TALLIES}
    # pieces with first_particle: each piece is the host route on ITS decayed list, the multiplicities and tallies add, and so do the
    # same-event pairs when a piece ends where an event ends (the mixed pairs need both events in one call)
    n, cut = len(q), int(np.searchsorted(q["event"], 3))
    assert 0 < cut < n
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        part, d = api.decay_particles_pairs(table, table["mc_id"], q[lo:hi], slot, S, DECAY_BINS, N_DECAY_EVENTS, seed=cases.SEED, lifetime=lifetime,
                                            first_particle=lo)
        o, _, _ = api.decay_particles(table, table["mc_id"], q[lo:hi], seed=cases.SEED, lifetime=lifetime, first_particle=lo)
        assert P.same_hist(part, api.pairs_list(DECAY_BINS, N_DECAY_EVENTS, S, slot, o))
        parts.append((part, d))
    assert np.array_equal(sum(r["M"] for r, _ in parts), got["M"]) and np.array_equal(sum(r["same"] for r, _ in parts), got["same"])
    for k in ("n_final", "n_unbinned", "n_decays", "n_stuck", "n_trials"):
        assert sum(d[k] for _, d in parts) == dst[k], k


def test_decay_pairs_refusals_and_the_empty_list(table):
    slot, ids = api.stable_slots(table, [211, -211, 321])
    S, q = len(ids), primaries(table)
    before = api.resource_counters()
    bad_event = q.copy()
    bad_event["event"][5] = N_DECAY_EVENTS
    for kw in (dict(bins=dict(DECAY_BINS, n_phi=10)), dict(bins=dict(DECAY_BINS, y_cut=0.0)), dict(n_slots=0), dict(n_slots=2), dict(n_events=0),
               dict(q=bad_event)):
        a = dict(q=q, slot=slot, n_slots=S, bins=DECAY_BINS, n_events=N_DECAY_EVENTS)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_pairs(table, table["mc_id"], a["q"], a["slot"], a["n_slots"], a["bins"], a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    assert api.resource_counters() == before
    r, st = api.decay_particles_pairs(table, table["mc_id"], q[:0], slot, S, DECAY_BINS, N_DECAY_EVENTS)
    assert st["n_final"] == st["n_unbinned"] == 0 and all(not v.any() for v in r.values())


def test_the_pions_of_a_rho0_at_rest_are_back_to_back():
    """Physics the restatement cannot vouch for: 50 events of one rho0 at rest, pi+ in slot 0 and pi- in slot 1.  Class (0, 1) holds one pair
    per event (trigger pi+, associate pi-), all at delta phi = n_phi / 2; classes (0, 0) and (1, 1) hold none.  The pions' common polar
    angle is free, so delta y is summed over: y(pi-) = -y(pi+) puts the pair anywhere on the delta y axis."""
    t = cases.hand_table([cases.stable(211, 0.13957), cases.stable(-211, 0.13957), (113, 0.77526, 0.1491, 0, [(2, 1.0, [211, -211])])])
    q = ref.make_particles(api, t, t["mc_id"], [2] * 50, np.zeros((50, 3)), events=np.arange(50))
    bins = dict(y_cut=8.0, pT_min=0.0, pT_max=100.0, n_y=16, n_phi=20)
    out, _, _ = api.decay_particles(t, t["mc_id"], q, seed=9)
    assert P.edge_distance(bins, out) > 1e-9
    r, st = api.decay_particles_pairs(t, t["mc_id"], q, [0, 1, -1], 2, bins, 50, seed=9)
    assert st["n_final"] == 100 and st["n_unbinned"] == 0 and np.all(r["M"] == 1)
    per_dphi = r["same"].sum(axis=1)
    assert per_dphi[api.pair_class(0, 1, 2)].tolist() == [0] * 10 + [50] + [0] * 9
    assert not per_dphi[api.pair_class(0, 0, 2)].any() and not per_dphi[api.pair_class(1, 1, 2)].any()
    assert P.same_hist(r, api.pairs_list(bins, 50, 2, [0, 1, -1], out))


# ---- the sampler route ----
SAMPLER_BINS = dict(y_cut=1.5, eta_cut=4.0, pT_lower_cut=0.25, pT_upper_cut=2.75, tau_min=1.0, tau_max=9.0, r_min=0.5, r_max=8.0,
                    y_bins=12, eta_bins=16, pT_bins=10, tau_bins=8, r_bins=15)
PLAN_BINS = P.bins_of((12, 16))
N_EV = 30


@pytest.fixture(scope="module")
def sampler_case(fx, table):
    """400 cells x 30 events of pi+, rho0 and omega (the shape of tests/test_gpu_flow.py), so that the decay pass has something to decay."""
    import torch
    sp, gla, o = inputs.species([211, 113, 223]), inputs.feqmod_tables(0.15), dict(dimension=3, df_mode=2)
    cells = {k: v.copy() for k, v in synth.synth_surface(400, 3, seed=861).items()}
    for f in ("dat", "dax", "day", "dan"):
        cells[f] *= 50.0
    kw = dict(n_events=N_EV, seed=19, y_cut=0.5)
    plist, _ = api.sample_particles(cells, sp, fx["df"], gla, o, **kw)
    dev = torch.device("cuda:0")
    tens = {k: torch.from_numpy(np.ascontiguousarray(cells[k])).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    S = len(sp["mass"])
    slot_d, ids = api.stable_slots(table, [211, -211, 111])
    r = dict(sp=sp, gla=gla, o=o, cells=cells, kw=kw, list=plist, tens=tens, ptrs={k: v.data_ptr() for k, v in tens.items()}, S=S,
             slot=np.arange(S, dtype=np.int32), slot_d=slot_d, S_d=len(ids), plan=api.SamplerPlan(sp, fx["df"], gla, o, max_cells=400, y_cut=0.5),
             dtable=api.DecayMcTable(table, sp["mc_id"], device=0))
    r["want"] = api.pairs_list(PLAN_BINS, N_EV, S, r["slot"], plist)
    yield r
    r["plan"].close()


def run_pairs(r, batch_events=0, decayed=True, bins=PLAN_BINS, **over):
    a = dict(slot=r["slot"], n_slots=r["S"], slot_decayed=r["slot_d"], n_slots_decayed=r["S_d"], table=r["dtable"] if decayed else None)
    a.update(over)
    return r["plan"].execute_pairs(400, r["ptrs"], N_EV, 19, bins, a["slot"], a["n_slots"], table=a["table"], slot_decayed=a["slot_decayed"],
                                   n_slots_decayed=a["n_slots_decayed"], decay_seed=77, lifetime=1, x_ptr=r["ptrs"]["x"], y_ptr=r["ptrs"]["y"],
                                   batch_events=batch_events)


def test_execute_pairs_is_pairs_list_of_the_list_for_every_batching(table, sampler_case):
    r = sampler_case
    assert len(r["list"]) >= 200 and r["want"]["M"].sum() > 100 and r["want"]["mixed"].sum() > 1000
    out, _, dst_list = api.decay_particles(table, r["sp"]["mc_id"], r["list"], seed=77, lifetime=1)
    assert P.edge_distance(PLAN_BINS, out) > 1e-9 and dst_list["n_decays"] > 0
    want_d = api.pairs_list(PLAN_BINS, N_EV, r["S_d"], r["slot_d"], out)
    first = None
    for batch_events in (1, 7, 0):
        h, h_d, st, dst = run_pairs(r, batch_events)
        assert P.same_hist(h, r["want"]), batch_events
        assert P.same_hist(h_d, want_d), batch_events
        assert st["n_particles"] == len(r["list"]) == dst["n_primaries"]
        assert dst["n_final"] == len(out) and dst["n_unbinned"] == len(out) - int(want_d["M"].sum())
        first = first or (h, h_d)
        assert P.same_hist(h, first[0]) and P.same_hist(h_d, first[1])
    only, st = run_pairs(r, 0, decayed=False)
    assert P.same_hist(only, first[0]) and st["n_particles"] == len(r["list"])
    # other bins on the same plan: the blocks are sized again
    big = P.bins_of((33, 20))
    h, _ = run_pairs(r, 7, decayed=False, bins=big)
    assert P.same_hist(h, api.pairs_list(big, N_EV, r["S"], r["slot"], r["list"]))


def test_the_plans_older_entries_return_what_they_returned_before(table, sampler_case):
    import torch
    r = sampler_case
    plan, ptrs, S = r["plan"], r["ptrs"], r["S"]
    slot_b, ids = api.stable_slots(table, [211, -211, 111])

    def older():
        buf = torch.zeros(len(r["list"]) * api.PARTICLE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        n, _ = plan.execute(400, ptrs, N_EV, 19, particles_ptr=buf.data_ptr(), capacity=len(r["list"]), x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        lst = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=api.PARTICLE_DTYPE)[:n]
        binned, _ = plan.execute_binned(400, ptrs, N_EV, 19, SAMPLER_BINS, S, x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        flow, _ = plan.execute_flow(400, ptrs, N_EV, 19, F.CUTS, r["slot"], S, x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        th, de, _, dst = plan.execute_decayed_binned(400, ptrs, N_EV, 19, SAMPLER_BINS, S, r["dtable"], slot_b, len(ids), x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        return lst, binned, flow, th, de, dst["n_final"]

    before = older()
    assert np.array_equal(before[0], r["list"])
    run_pairs(r, 7)
    after = older()
    assert np.array_equal(before[0], after[0]) and before[5] == after[5]
    for a, b in zip(before[1:5], after[1:5]):
        assert all(np.array_equal(a[k], b[k]) for k in a)
    h, _, _, _ = run_pairs(r, 0)
    assert P.same_hist(h, r["want"])


def test_execute_pairs_refusals_leave_the_resource_counters_unmoved(table, sampler_case):
    r = sampler_case
    run_pairs(r, 0)
    other = api.DecayMcTable(table, [211, 321], device=0)
    before = api.resource_counters()
    bad_d = r["slot_d"].copy()
    bad_d[0] = r["S_d"]
    for kw in (dict(bins=dict(PLAN_BINS, y_cut=0.0)), dict(bins=dict(PLAN_BINS, n_phi=18)), dict(bins=dict(PLAN_BINS, n_y=65)),
               dict(slot=np.array([3, 0, 0], np.int32)), dict(n_slots=0), dict(slot_decayed=bad_d), dict(n_slots_decayed=0), dict(table=other)):
        with pytest.raises(api.Is3dError) as e:
            run_pairs(r, 0, **kw)
        assert e.value.code == api.IS3D_EINVAL, kw
    assert api.resource_counters() == before


def test_sample_pairs_is_execute_pairs_and_the_device_samplers_hadrons_are_independent(fx, table, sampler_case):
    r = sampler_case
    h, h_d, st, dst = api.sample_pairs(r["cells"], r["sp"], fx["df"], r["gla"], PLAN_BINS, r["slot"], r["S"], r["o"], table=table,
                                       chosen_mc_id=r["sp"]["mc_id"], slot_decayed=r["slot_d"], n_slots_decayed=r["S_d"], decay_seed=77, lifetime=1,
                                       batch_events=7, **r["kw"])
    want, want_d, _, dst_want = run_pairs(r, 0)
    assert P.same_hist(h, want) and P.same_hist(h_d, want_d) and dst["n_final"] == dst_want["n_final"] and st["n_particles"] == len(r["list"])
    # the independence condition of tests/test_pairs_host.py (same surface, events and seed) on the list the DEVICE sampler makes
    cells, sp, gla, o, kw = F.thermal_surface()
    plist, _ = api.sample_particles(cells, sp, fx["df"], gla, o, **kw)
    E, sigma = P.short_range_excess(P.BINS, kw["n_events"], plist)
    print("short-range excess of the device sampler's list: E = %.3e, sigma = %.3e, pull %.2f" % (E, sigma, E / sigma))
    assert abs(E) <= 5.0 * sigma, (E, sigma)
    # ... whose same and mixed totals are those of the device histograms of the same run
    hist, _ = api.sample_pairs(cells, sp, fx["df"], gla, P.BINS, [0], 1, o, **kw)
    assert P.same_hist(hist, api.pairs_list(P.BINS, kw["n_events"], 1, [0], plist))


# ---- the run driver ----
def test_driver_writes_the_pair_files_and_leaves_every_other_file_as_it_was(tmp_path, reference):
    """A 2+1D toy run (the one of tests/test_gpu_flow.py) four times: with and without test_sampler_decayed, each with and without
    test_sampler_pairs.  Without the pair files the results of a run with the key are those of the run without it, byte for byte; the pair
    files are one per class of 211, -211, 321, 2212 and other; the thermal ones do not depend on test_sampler_decayed; every class file's
    totals are the sums that the multiplicities give.  Those come from the flow files of the same runs (test_sampler_flow = 1 in all four, with
    the pair bins' acceptance: the two rules differ only for a hadron exactly on the upper rapidity edge)."""
    ids = [211, 321, 2212, 113, 223, 2224, -2224, 221, -211]
    cells = synth.synth_surface(3000, 2, seed=92)
    sub = ("dN_dy", "dN_deta", "momentum_distribution", "vn", "spacetime_distribution")
    files, stdout = {}, {}
    for decayed in (0, 1):
        for pairs in (0, 1):
            root = refformat.make_run_dir(str(tmp_path / ("d%d_p%d" % (decayed, pairs))), cells, ids,
                                          dict(operation=2, dimension=2, df_mode=2, sampler_seed=17, oversample=1, min_num_hadrons=2000, test_sampler=1))
            shutil.copy(os.path.join(reference, "PDG", URQMD), os.path.join(root, "PDG", URQMD))     # the shipped list: the toy one has no decay data
            with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
                f.write("test_sampler_on_device\t= 1\n" + ("test_sampler_decayed\t= 1\n" if decayed else "") +
                        "test_sampler_flow\t= 1\nflow_y_cut = 1.5\nflow_y_gap = 0.2\nflow_pT_min = 0.1\n" +
                        ("test_sampler_pairs\t= 1\npairs_y_cut = 1.5\npairs_pT_min = 0.1\npairs_y_bins = 6\npairs_phi_bins = 8\n" if pairs else ""))
            for d in sub + ("flow",) + (("pairs",) if pairs else ()):
                os.makedirs(os.path.join(root, "results", d), exist_ok=True)
                if decayed:
                    os.makedirs(os.path.join(root, "results", "decayed", d))
            r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
            files[decayed, pairs] = {os.path.relpath(os.path.join(dp, f), os.path.join(root, "results")): open(os.path.join(dp, f), "rb").read()
                                     for dp, _, fs in os.walk(os.path.join(root, "results")) for f in fs}
            stdout[decayed, pairs] = r.stdout
    is_pairs = lambda k: k.startswith("pairs" + os.sep) or k.startswith(os.path.join("decayed", "pairs") + os.sep)  # noqa: E731
    for decayed in (0, 1):
        rest = {k: v for k, v in files[decayed, 1].items() if not is_pairs(k)}
        assert rest == files[decayed, 0] and len(rest) > 10
        assert "pair correlations on the device" in stdout[decayed, 1] and "pair correlations" not in stdout[decayed, 0]
    labels = ("211", "321", "2212", "other", "-211")                    # slots in the order the chosen ids come: -211 is last
    names = sorted(os.path.join("pairs", "correlation_%s_%s.dat" % (labels[a], labels[b])) for a in range(5) for b in range(a, 5))
    assert sorted(k for k in files[0, 1] if is_pairs(k)) == names
    thermal = {k: v for k, v in files[1, 1].items() if k.startswith("pairs" + os.sep)}
    assert thermal == {k: files[0, 1][k] for k in names}
    stable = ("211", "321", "2212", "-211")                              # the chosen species that are stable in the table: no "other"
    names_d = sorted(os.path.join("decayed", "pairs", "correlation_%s_%s.dat" % (stable[a], stable[b])) for a in range(4) for b in range(a, 4))
    assert sorted(k for k in files[1, 1] if k.startswith(os.path.join("decayed", "pairs"))) == names_d

    def totals(run, name):
        path = tmp_path / run / "results" / name
        head = open(path).read().split("\n")[1]
        rows = np.loadtxt(path)
        n_same, n_mixed = (int(x.split(":")[1]) for x in head[2:].split(","))
        assert rows.shape == (11 * 8, 5) and rows[:, 2].sum() == n_same and rows[:, 3].sum() == n_mixed
        return n_same, n_mixed

    for run, base_dir, lab in (("d0_p1", "pairs", labels), ("d1_p1", os.path.join("decayed", "pairs"), stable)):
        n = {(a, b): totals(run, os.path.join(base_dir, "correlation_%s_%s.dat" % (lab[a], lab[b]))) for a in range(len(lab)) for b in range(a, len(lab))}
        assert n[0, 0][0] > 1000 and n[0, 0][1] > 1000
        flow_dir = os.path.join(os.path.dirname(base_dir), "flow")
        M = {l: np.loadtxt(tmp_path / run / "results" / flow_dir / ("multiplicity_%s.dat" % l))[:, 1].astype(np.int64) for l in ("211", "321", "2212")}
        for a in range(3):
            for b in range(a, 3):
                Ma, Mb = M[lab[a]], M[lab[b]]
                assert n[a, b] == (int((Ma * Mb).sum() - (Ma.sum() if a == b else 0)), int((Ma * np.roll(Mb, -1)).sum())), (run, a, b)
    pions_thermal = totals("d1_p1", os.path.join("pairs", "correlation_211_211.dat"))[0]
    pions_decayed = totals("d1_p1", os.path.join("decayed", "pairs", "correlation_211_211.dat"))[0]
    assert pions_decayed > pions_thermal > 0                             # the rho0, omega, Delta++ and eta feed the pi+
