"""GPU (-m gpu): the HBT histograms on the device (cf_hbt_select, cf_hbt_pairs: the loop over the ordered pairs of every (event, slot)
segment) against the host route is3d_hbt_list, the explicit double loop.  den and M are array_equal: the counts are integers and the rule
of csrc/cf_sampler_hbt.h reaches the same bin on both sides.  Each num word is within den units of the host's: one unit per pair is what the
two cos may differ by after llrint.  kernel_form 0, 1 and 2 give identical bits, num included.

The lists (tests/hbt_cases.py): segments of 0, 1, 2, 63, 64, 65 and 257 accepted particles, a tail of 200 events of 1-2 particles, one
event of 1000 (four tiles of i, and with the shuffled list any order inside a segment), slots 1 and 3 with -1 present, n_q even and odd, a
pair of identical momenta (q = 0), a back-to-back pair (KT = 0, rejected), particles out of range.  One event of 5000 particles runs over
two work items per tile of i (the split of the j loop) and is compared between the forms and with the closed form of its total.

The decay sink (cf_decay_mc_hbt, count and fill over one counter-based stream) against its host route -- is3d_decay_particles, then
is3d_hbt_list on the decayed list with the slot map over the table's entries -- at lifetime 0 and 1 in every form; a rho0 at rest with
lifetime 0 gives two pions at one point.  The sampler route at batch_events 1, 7 and 0 against is3d_hbt_list of the list execute returns."""
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import decays_mc_cases as cases
import decays_mc_ref as ref
import hbt_cases as H
import refformat
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu

LISTS = dict(hand=H.hand_list, shuffled=H.shuffled_list)
SHAPES = dict(even=H.BINS, odd=H.BINS_ODD, big=H.BINS_BIG)


@lru_cache(maxsize=None)
def host_hist(shape):
    """The host route on hand_list (the shuffled list has the same histograms), checked against the numpy restatement; computed once."""
    p, n_events = H.hand_list()
    want = api.hbt_list(SHAPES[shape], n_events, 4, H.SLOT4, p)
    assert H.same_counts(want, H.numpy_hist(SHAPES[shape], n_events, 4, H.SLOT4, p))
    for v in want.values():
        v.setflags(write=False)
    return want


def forms(bins):
    return (0, 1, 2) if bins["n_kT"] * bins["n_q"] ** 3 <= 3072 else (0, 1)   # BINS_BIG: form 0 against form 1, form 2 refused (below)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(LISTS))
def test_hbt_list_device_is_the_host_route_in_every_form(name, shape):
    p, n_events = LISTS[name]()
    bins, want = SHAPES[shape], host_hist(shape)
    per_slot = want["den"].sum(axis=(1, 2, 3, 4))
    assert per_slot[0] > 1000 and per_slot[1] > 100000 and per_slot[2] == 0 and per_slot[3] == 200 and 0 < want["M"].sum() < len(p)
    first = None
    for form in forms(bins):
        got, skipped = api.hbt_list_device(dict(bins, kernel_form=form), n_events, 4, H.SLOT4, p)
        assert skipped == 0
        assert H.same_counts(got, want), (name, shape, form)
        worst = int(np.max(np.abs(got["num"] - want["num"]) - want["den"]))
        print("%s %s form %d: max |num - host| %d, worst excess over den %d" % (name, shape, form, int(np.abs(got["num"] - want["num"]).max()), worst))
        assert H.num_within_one_unit_per_pair(want, got), (name, shape, form)
        first = first or got
        assert np.array_equal(got["num"], first["num"]), (name, shape, form)


def test_the_form_that_does_not_fit_is_refused_before_any_device_use():
    p, n_events = H.hand_list()
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        api.hbt_list_device(dict(H.BINS_BIG, kernel_form=2), n_events, 4, H.SLOT4, p)
    assert e.value.code == api.IS3D_EINVAL and "16000" in str(e.value)
    for kw in (dict(kernel_form=3), dict(kernel_form=-1), dict(n_q=1), dict(n_q=65), dict(n_kT=17), dict(q_max=0.0), dict(y_cut=float("nan"))):
        with pytest.raises(api.Is3dError) as e:
            api.hbt_list_device(dict(H.BINS, **kw), n_events, 4, H.SLOT4, p)
        assert e.value.code == api.IS3D_EINVAL, kw
    assert api.resource_counters() == before


def test_identical_momenta_and_the_back_to_back_pair():
    """The last event of hand_list alone: the two particles of equal momentum make the only two ordered pairs (q = 0: bin n_q / 2 in each
    direction for the even n_q), with cos(0) = 1 exactly although they sit at different points; the back-to-back pair has KT = 0."""
    p, n_events = H.hand_list()
    last = p[p["event"] == n_events - 1].copy()
    last["event"] = 0
    got, _ = api.hbt_list_device(H.BINS, 1, 4, H.SLOT4, last)
    assert got["M"].tolist() == [[4, 0, 0, 0]] and got["den"].sum() == 2
    assert got["den"][0, :, 4, 4, 4].sum() == 2 and got["num"].sum() == 2 * 2 ** 32
    assert H.same_counts(got, api.hbt_list(H.BINS, 1, 4, H.SLOT4, last))


def test_particles_out_of_range_add_nothing_and_are_counted():
    p, n_events = H.hand_list()
    want = host_hist("even")
    q = np.concatenate([p[:100], p[:4], p[100:], p[:3]])
    q["species"][100:102] = (H.N_SPECIES, -1)
    q["event"][102:104] = (n_events, -1)
    q["event"][-3:] = (-5, n_events + 7, 2 ** 31 - 1)
    got, skipped = api.hbt_list_device(H.BINS, n_events, 4, H.SLOT4, q)
    assert skipped == 7 and H.same_counts(got, want) and H.num_within_one_unit_per_pair(want, got)
    with pytest.raises(api.Is3dError) as e:
        api.hbt_list(H.BINS, n_events, 4, H.SLOT4, q)
    assert e.value.code == api.IS3D_EINVAL
    empty, skipped = api.hbt_list_device(H.BINS, n_events, 4, H.SLOT4, p[:0])
    assert skipped == 0 and all(not v.any() for v in empty.values())


def test_one_large_event_is_split_over_work_items_with_the_same_bits():
    """5000 particles in one segment: 20 tiles of i, each against two runs of j (16 + 4 tiles).  25 million ordered pairs: the forms
    against each other and the total against the closed form n (n - 1) with a q cube that holds every pair."""
    rng = np.random.default_rng(77)
    n = 5000
    p3, x4 = H.cluster(rng, n, spread=0.01)
    p = H.make(p3, x4, 0, 0)
    bins = dict(H.BINS, q_max=0.5, n_kT=1, kT_min=0.0, kT_max=5.0)
    a, _ = api.hbt_list_device(dict(bins, kernel_form=1), 1, 1, [0], p)
    b, _ = api.hbt_list_device(dict(bins, kernel_form=2), 1, 1, [0], p)
    assert a["M"].tolist() == [[n]] and a["den"].sum() == n * (n - 1)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # the first 300 of them against the host
    small, _ = api.hbt_list_device(bins, 1, 1, [0], p[:300])
    want = api.hbt_list(bins, 1, 1, [0], p[:300])
    assert H.same_counts(small, want) and H.num_within_one_unit_per_pair(want, small)


# ---- the decay sink ----
URQMD = "pdg-urqmd_v3.3+.dat"
N_DECAY_EVENTS = 7
TALLIES = ("n_primaries", "n_decays", "n_final", "n_stuck", "n_trials", "n_exhausted", "max_stack", "max_depth", "n_closed_channels")
DECAY_BINS = dict(y_cut=3.0, pT_min=0.0, pT_max=10.0, kT_min=0.0, kT_max=5.0, n_kT=2, q_max=1.5, n_q=6, kernel_form=0)
_cache = {}


@pytest.fixture(scope="module")
def table(reference):
    return cases.tables(api, reference)[URQMD]


def primaries(table):
    if "hand" not in _cache:
        a = cases.hand_list(api, table, ref.prepare(table))
        b = cases.every_unstable(api, table, 11)
        b["event"] %= N_DECAY_EVENTS
        _cache["hand"] = np.concatenate([a, b])
    return _cache["hand"]


@pytest.mark.parametrize("lifetime", (0, 1))
def test_decay_particles_hbt_is_the_host_route(table, lifetime):
    slot, ids = api.stable_slots(table, [211, -211, 321])
    S, q = len(ids), primaries(table)
    out, _, st = api.decay_particles(table, table["mc_id"], q, seed=cases.SEED, lifetime=lifetime)
    want = api.hbt_list(DECAY_BINS, N_DECAY_EVENTS, S, slot, out)
    kept = int(want["M"].sum())
    assert 50 < kept < len(out) and want["den"].sum() > 1000
    if lifetime:
        assert np.abs(out["t"]).max() > 0.0
    first = None
    for form in (0, 1, 2):
        got, dst = api.decay_particles_hbt(table, table["mc_id"], q, slot, S, dict(DECAY_BINS, kernel_form=form), N_DECAY_EVENTS, seed=cases.SEED,
                                           lifetime=lifetime)
        assert H.same_counts(got, want) and H.num_within_one_unit_per_pair(want, got), form
        assert dst["n_final"] == len(out) and dst["n_unbinned"] == len(out) - kept
        assert all(dst[k] == st[k] for k in TALLIES), {k: (dst[k], st[k]) for k in TALLIES}
        first = first or got
        assert np.array_equal(got["num"], first["num"])


def test_decay_hbt_refusals_and_the_empty_list(table):
    slot, ids = api.stable_slots(table, [211, -211, 321])
    S, q = len(ids), primaries(table)
    before = api.resource_counters()
    bad_event = q.copy()
    bad_event["event"][5] = N_DECAY_EVENTS
    for kw in (dict(bins=dict(DECAY_BINS, n_q=1)), dict(bins=dict(DECAY_BINS, y_cut=0.0)), dict(bins=dict(DECAY_BINS, n_q=20, kernel_form=2)),
               dict(n_slots=0), dict(n_slots=2), dict(n_events=0), dict(q=bad_event)):
        a = dict(q=q, slot=slot, n_slots=S, bins=DECAY_BINS, n_events=N_DECAY_EVENTS)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_hbt(table, table["mc_id"], a["q"], a["slot"], a["n_slots"], a["bins"], a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    assert api.resource_counters() == before
    r, st = api.decay_particles_hbt(table, table["mc_id"], q[:0], slot, S, DECAY_BINS, N_DECAY_EVENTS)
    assert st["n_final"] == st["n_unbinned"] == 0 and all(not v.any() for v in r.values())


def test_the_pions_of_rho0s_at_rest_are_born_at_one_point():
    """Physics the restatement cannot vouch for: events of three rho0 at rest at ONE point, lifetime 0, pi+ in slot 0 and pi- in slot 1: the
    three pions of a slot are born where the parents were, so every pair has dx = 0 and num = den 2^32 in every bin."""
    t = cases.hand_table([cases.stable(211, 0.13957), cases.stable(-211, 0.13957), (113, 0.77526, 0.1491, 0, [(2, 1.0, [211, -211])])])
    q = ref.make_particles(api, t, t["mc_id"], [2] * 60, np.zeros((60, 3)), events=np.arange(60) // 3)
    bins = dict(y_cut=8.0, pT_min=0.0, pT_max=100.0, kT_min=0.0, kT_max=5.0, n_kT=1, q_max=1.0, n_q=4, kernel_form=0)
    r, st = api.decay_particles_hbt(t, t["mc_id"], q, [0, 1, -1], 2, bins, 20, seed=9, lifetime=0)
    assert st["n_final"] == 120 and np.all(r["M"] == 3) and r["den"].sum() > 60
    assert np.array_equal(r["num"], r["den"] * 2 ** 32)
    out, _, _ = api.decay_particles(t, t["mc_id"], q, seed=9, lifetime=0)
    assert H.same_counts(r, api.hbt_list(bins, 20, 2, [0, 1, -1], out))


# ---- the sampler route ----
SAMPLER_BINS = dict(y_cut=1.5, eta_cut=4.0, pT_lower_cut=0.25, pT_upper_cut=2.75, tau_min=1.0, tau_max=9.0, r_min=0.5, r_max=8.0,
                    y_bins=12, eta_bins=16, pT_bins=10, tau_bins=8, r_bins=15)
PLAN_BINS = dict(y_cut=2.0, pT_min=0.0, pT_max=5.0, kT_min=0.0, kT_max=3.0, n_kT=2, q_max=1.2, n_q=6, kernel_form=0)
N_EV = 30


@pytest.fixture(scope="module")
def sampler_case(fx, table):
    """400 cells x 30 events of pi+, rho0 and omega (the shape of tests/test_gpu_sampler_fused.py), so that the decay pass has something to decay."""
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
    r["want"] = api.hbt_list(PLAN_BINS, N_EV, S, r["slot"], plist)
    yield r
    r["plan"].close()


def run_hbt(r, batch_events=0, decayed=True, bins=PLAN_BINS, **over):
    a = dict(slot=r["slot"], n_slots=r["S"], slot_decayed=r["slot_d"], n_slots_decayed=r["S_d"], table=r["dtable"] if decayed else None)
    a.update(over)
    return r["plan"].execute_hbt(400, r["ptrs"], N_EV, 19, bins, a["slot"], a["n_slots"], table=a["table"], slot_decayed=a["slot_decayed"],
                                 n_slots_decayed=a["n_slots_decayed"], decay_seed=77, lifetime=1, x_ptr=r["ptrs"]["x"], y_ptr=r["ptrs"]["y"],
                                 batch_events=batch_events)


def test_execute_hbt_is_hbt_list_of_the_list_for_every_batching(fx, table, sampler_case):
    r = sampler_case
    assert len(r["list"]) >= 200 and r["want"]["M"].sum() > 100 and r["want"]["den"].sum() > 100
    out, _, dst_list = api.decay_particles(table, r["sp"]["mc_id"], r["list"], seed=77, lifetime=1)
    assert dst_list["n_decays"] > 0
    want_d = api.hbt_list(PLAN_BINS, N_EV, r["S_d"], r["slot_d"], out)
    first = None
    for batch_events in (1, 7, 0):
        h, h_d, st, dst = run_hbt(r, batch_events)
        assert H.same_counts(h, r["want"]) and H.num_within_one_unit_per_pair(r["want"], h), batch_events
        assert H.same_counts(h_d, want_d) and H.num_within_one_unit_per_pair(want_d, h_d), batch_events
        assert st["n_particles"] == len(r["list"]) == dst["n_primaries"]
        assert dst["n_final"] == len(out) and dst["n_unbinned"] == len(out) - int(want_d["M"].sum())
        first = first or (h, h_d)
        assert all(np.array_equal(h[k], first[0][k]) and np.array_equal(h_d[k], first[1][k]) for k in h), batch_events
    only, st = run_hbt(r, 0, decayed=False)
    assert all(np.array_equal(only[k], first[0][k]) for k in only) and st["n_particles"] == len(r["list"])
    one, _ = run_hbt(r, 7, decayed=False, bins=dict(PLAN_BINS, kernel_form=1))
    assert all(np.array_equal(one[k], first[0][k]) for k in one)
    h, h_d, st, dst = api.sample_hbt(r["cells"], r["sp"], fx["df"], r["gla"], PLAN_BINS, r["slot"], r["S"], r["o"], table=table,
                                     chosen_mc_id=r["sp"]["mc_id"], slot_decayed=r["slot_d"], n_slots_decayed=r["S_d"], decay_seed=77, lifetime=1,
                                     batch_events=7, **r["kw"])
    assert all(np.array_equal(h[k], first[0][k]) and np.array_equal(h_d[k], first[1][k]) for k in h)


def test_the_plans_older_entries_return_what_they_returned_before(table, sampler_case):
    import torch
    import flow_cases as F
    import pairs_cases as P
    r = sampler_case
    plan, ptrs, S = r["plan"], r["ptrs"], r["S"]
    slot_b, ids = api.stable_slots(table, [211, -211, 111])

    def older():
        buf = torch.zeros(len(r["list"]) * api.PARTICLE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        n, _ = plan.execute(400, ptrs, N_EV, 19, particles_ptr=buf.data_ptr(), capacity=len(r["list"]), x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        lst = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=api.PARTICLE_DTYPE)[:n]
        binned, _ = plan.execute_binned(400, ptrs, N_EV, 19, SAMPLER_BINS, S, x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        flow, _ = plan.execute_flow(400, ptrs, N_EV, 19, F.CUTS, r["slot"], S, x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        pairs, _ = plan.execute_pairs(400, ptrs, N_EV, 19, P.bins_of((12, 16)), r["slot"], S, x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        th, de, _, dst = plan.execute_decayed_binned(400, ptrs, N_EV, 19, SAMPLER_BINS, S, r["dtable"], slot_b, len(ids), x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        return lst, binned, flow, pairs, th, de, dst["n_final"]

    before = older()
    assert np.array_equal(before[0], r["list"])
    run_hbt(r, 7)
    after = older()
    assert np.array_equal(before[0], after[0]) and before[6] == after[6]
    for a, b in zip(before[1:6], after[1:6]):
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_execute_hbt_refusals_leave_the_resource_counters_unmoved(table, sampler_case):
    r = sampler_case
    other = api.DecayMcTable(table, [211, 321], device=0)
    before = api.resource_counters()
    bad_d = r["slot_d"].copy()
    bad_d[0] = r["S_d"]
    for kw in (dict(bins=dict(PLAN_BINS, y_cut=0.0)), dict(bins=dict(PLAN_BINS, n_q=65)), dict(bins=dict(PLAN_BINS, n_q=16, kernel_form=2)),
               dict(slot=np.array([3, 0, 0], np.int32)), dict(n_slots=0), dict(slot_decayed=bad_d), dict(n_slots_decayed=0), dict(table=other)):
        with pytest.raises(api.Is3dError) as e:
            run_hbt(r, 0, **kw)
        assert e.value.code == api.IS3D_EINVAL, kw
    assert api.resource_counters() == before


# ---- the run driver ----
def test_driver_writes_the_hbt_files_and_leaves_every_other_file_as_it_was(tmp_path, reference):
    """A 2+1D toy run (the one of tests/test_gpu_pairs.py) four times: with and without test_sampler_decayed, each with and without
    test_sampler_hbt.  Without the HBT files the results of a run with the key are those of the run without it, byte for byte; the HBT files
    are one per (slot of 211, -211, 321, -321, kT bin) and a radii file per slot; the thermal ones do not depend on test_sampler_decayed;
    every correlation file's den column sums to its header's total, and C = 1 where den = 0."""
    ids = [211, 321, 2212, 113, 223, 2224, -2224, 221, -211, -321]
    cells = synth.synth_surface(3000, 2, seed=92)
    sub = ("dN_dy", "dN_deta", "momentum_distribution", "vn", "spacetime_distribution")
    files, stdout = {}, {}
    for decayed in (0, 1):
        for hbt in (0, 1):
            root = refformat.make_run_dir(str(tmp_path / ("d%d_h%d" % (decayed, hbt))), cells, ids,
                                          dict(operation=2, dimension=2, df_mode=2, sampler_seed=17, oversample=1, min_num_hadrons=2000, test_sampler=1))
            shutil.copy(os.path.join(reference, "PDG", URQMD), os.path.join(root, "PDG", URQMD))     # the shipped list: the toy one has no decay data
            with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
                f.write("test_sampler_on_device\t= 1\n" + ("test_sampler_decayed\t= 1\n" if decayed else "") +
                        ("test_sampler_hbt\t= 1\nhbt_y_cut = 1.5\nhbt_pT_min = 0.05\nhbt_kT_bins = 2\nhbt_q_max = 0.3\nhbt_q_bins = 6\n" if hbt else ""))
            for d in sub + (("hbt",) if hbt else ()):
                os.makedirs(os.path.join(root, "results", d), exist_ok=True)
                if decayed:
                    os.makedirs(os.path.join(root, "results", "decayed", d))
            r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
            files[decayed, hbt] = {os.path.relpath(os.path.join(dp, f), os.path.join(root, "results")): open(os.path.join(dp, f), "rb").read()
                                   for dp, _, fs in os.walk(os.path.join(root, "results")) for f in fs}
            stdout[decayed, hbt] = r.stdout
    is_hbt = lambda k: k.startswith("hbt" + os.sep) or k.startswith(os.path.join("decayed", "hbt") + os.sep)  # noqa: E731
    for decayed in (0, 1):
        rest = {k: v for k, v in files[decayed, 1].items() if not is_hbt(k)}
        assert rest == files[decayed, 0] and len(rest) > 10
        assert "HBT correlations on the device" in stdout[decayed, 1] and "HBT" not in stdout[decayed, 0]
    labels = ("211", "-211", "321", "-321")
    names = sorted([os.path.join("hbt", "correlation_%s_kT%d.dat" % (l, k)) for l in labels for k in (0, 1)] +
                   [os.path.join("hbt", "radii_%s.dat" % l) for l in labels])
    assert sorted(k for k in files[0, 1] if is_hbt(k)) == names
    assert {k: v for k, v in files[1, 1].items() if k.startswith("hbt" + os.sep)} == {k: files[0, 1][k] for k in names}
    assert sorted(k for k in files[1, 1] if k.startswith(os.path.join("decayed", "hbt"))) == sorted(os.path.join("decayed", n) for n in names)

    def total(run, name):
        path = tmp_path / run / "results" / name
        head = open(path).read().split("\n")[1]
        rows = np.loadtxt(path)
        assert rows.shape == (6 ** 3, 5) and rows[:, 3].sum() == int(head.split("pairs:")[1]) and np.all(rows[rows[:, 3] == 0, 4] == 1.0)
        assert np.all(np.abs(rows[:, 4] - 1.0) <= 1.0)
        return int(rows[:, 3].sum())

    thermal = total("d1_h1", os.path.join("hbt", "correlation_211_kT0.dat"))
    decayed = total("d1_h1", os.path.join("decayed", "hbt", "correlation_211_kT0.dat"))
    assert decayed > thermal > 100                                        # the rho0, omega, Delta++ and eta feed the pi+
    assert np.loadtxt(tmp_path / "d1_h1" / "results" / "hbt" / "radii_211.dat").shape == (2, 10)
