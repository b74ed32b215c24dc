"""GPU (-m gpu): the differential flow records on the device (cf_sampler_flow_diff, every form; the differential sink of cf_decay_mc_flow; the
sampler's batch loop; the run driver) against the host route is3d_flow_diff_list.  m must be equal exactly, every p word within m units of its
record (device against host libm), and forms 0, 1 and 2 must give identical bits.

The lists (tests/flow_diff_cases.py): one particle; 257 particles of one (event, slot, bin) -- a trip and a lane, every key equal; 64 particles
with 64 distinct keys; 700 particles over 5 events in random order, so that particles fall outside the window; 6 slots x 14 bins, where the
window (8126 words beside the staged edges) holds exactly 1 event of 3 (84 x 51 = 4284 words each), and 4 x 14, where it holds 2 of 5
(2856 words each); 4 x 40 bins, which fit no window; particles out of range; the empty list; a list in pieces."""
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import decays_mc_cases as cases
import decays_mc_ref as ref
import flow_cases as F
import flow_diff_cases as D
import refformat
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2)


def every_form(edges, n_events, n_slots, slot, p, what, forms=FORMS, skipped=0):
    """the device records in every form: against the host route, and against each other bit for bit"""
    cuts = D.cuts_for(edges)
    host = p[(p["species"] >= 0) & (p["species"] < len(slot)) & (p["event"] >= 0) & (p["event"] < n_events)] if skipped else p
    want = api.flow_diff_list(cuts, edges, n_events, n_slots, slot, host)
    assert np.array_equal(want["m"], D.numpy_m(cuts, edges, n_events, n_slots, slot, host))
    got = {}
    for form in forms:
        got[form], n_skipped = api.flow_diff_list_device(dict(cuts, kernel_form=form), edges, n_events, n_slots, slot, p)
        assert n_skipped == skipped, (what, form)
        D.assert_records(got[form], want, (what, form))
    assert all(D.same_bits(got[forms[0]], got[f]) for f in forms[1:]), what
    return got[forms[0]], want


def test_one_particle():
    p = D.particles_at([0.9], [1.0], [0.6], [1], [0])
    got, want = every_form(D.EDGES, 2, 1, [0], p, "one particle")
    assert got["m"].sum() == 2 and got["m"][1, 0, 3].tolist() == [1, 0, 1]          # bin 3 of [0.2, 3.0) / 14, sub-event B


def test_a_trip_and_a_lane_of_one_key():
    rng = np.random.default_rng(5)
    p = D.particles_at(rng.uniform(0.61, 0.79, 257), rng.uniform(-np.pi, np.pi, 257), rng.uniform(-0.2, 0.2, 257), 2, 1)
    got, want = every_form(D.EDGES, 3, 2, [-1, 1], p, "one key")
    assert got["m"][2, 1, 2, 0] == 257 == got["m"].sum()


def test_sixty_four_distinct_keys_in_one_wave():
    k = np.arange(64)
    edges = D.EDGES[:5]                                                    # 4 bins x 4 slots x 4 events
    pT = 0.5 * (edges[k % 4] + edges[k % 4 + 1])
    p = D.particles_at(pT, 0.1 * k, 0.0, k // 16, (k // 4) % 4)
    got, want = every_form(edges, 4, 4, [0, 1, 2, 3], p, "64 keys")
    assert np.all(got["m"][..., 0] == 1)


@lru_cache(maxsize=None)
def shuffled_700():
    rng = np.random.default_rng(20302)
    p = F.kinematic_list(rng, rng.integers(0, 5, 700))
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("n_slots,n_pT,n_events,window", ((3, 14, 5, 3), (6, 14, 3, 1), (4, 14, 5, 2), (4, 40, 5, 0)))
def test_lists_against_windows_of_every_size(n_slots, n_pT, n_events, window):
    assert min(n_events, (8192 - 66) // (n_slots * n_pT * 51)) == window
    edges = api.flow_diff_edges(0.2, 3.0, n_pT)
    p = shuffled_700()
    if n_events < 5:
        p = p[p["event"] < n_events]
    slot = F.slot_map(n_slots)
    forms = FORMS if window else (0, 1)
    for name, q in (("random order", p), ("by event", p[np.argsort(p["event"], kind="stable")])):
        got, want = every_form(edges, n_events, n_slots, slot, q, (name, n_slots, n_pT), forms)
        assert want["m"][..., 0].sum() > 150 and (want["m"][..., 0].sum(axis=(1, 2)) > 0).all()
    if not window:
        before = api.resource_counters()
        with pytest.raises(api.Is3dError) as e:
            api.flow_diff_list_device(D.cuts_for(edges, kernel_form=2), edges, n_events, n_slots, slot, p)
        assert e.value.code == api.IS3D_EINVAL and "8160 words" in str(e.value) and api.resource_counters() == before


def test_particles_out_of_range_are_counted_and_the_empty_list_is_zero():
    p = shuffled_700().copy()
    p["species"][100:102] = (F.N_SPECIES, -1)
    p["event"][102:104] = (5, -1)
    p["event"][-3:] = (-5, 12, 2 ** 31 - 1)
    every_form(D.EDGES, 5, 3, F.slot_map(3), p, "out of range", skipped=7)
    with pytest.raises(api.Is3dError) as e:
        api.flow_diff_list(D.CUTS, D.EDGES, 5, 3, F.slot_map(3), p)
    assert e.value.code == api.IS3D_EINVAL
    before = api.resource_counters()
    empty, skipped = api.flow_diff_list_device(D.CUTS, D.EDGES, 5, 3, F.slot_map(3), p[:0])
    assert skipped == 0 and all(not v.any() for v in empty.values()) and api.resource_counters() == before


def test_the_sum_over_bins_is_the_flow_kernels_record():
    p, slot = shuffled_700(), F.slot_map(3)
    for form in FORMS:
        diff, _ = api.flow_diff_list_device(dict(D.CUTS, kernel_form=form), D.EDGES, 5, 3, slot, p)
        flow, _ = api.flow_list_device(dict(D.CUTS, kernel_form=form), 5, 3, slot, p)
        assert F.same_bits(D.sum_over_bins(diff), flow), form


def test_pieces_of_a_list_add_to_the_whole():
    p, slot = shuffled_700(), F.slot_map(3)
    q = p[np.argsort(p["event"], kind="stable")]
    assert q["event"][299] == q["event"][300]                              # a cut inside an event
    for form in FORMS:
        cuts = dict(D.CUTS, kernel_form=form)
        whole, _ = api.flow_diff_list_device(cuts, D.EDGES, 5, 3, slot, q)
        parts = [api.flow_diff_list_device(cuts, D.EDGES, 5, 3, slot, q[a:b])[0] for a, b in ((0, 1), (1, 300), (300, 301), (301, 700))]
        assert all(np.array_equal(sum(r[k] for r in parts), whole[k]) for k in whole), form


# ---- the decay sink ----
SMASH = "pdg_smash.dat"
N_DECAY_EVENTS = 6
DECAY_EDGES = api.flow_diff_edges(0.2, 3.0, 7)


@pytest.fixture(scope="module")
def table(reference):
    return cases.tables(api, reference)[SMASH]


@pytest.fixture(scope="module")
def primaries(table):
    """300 primaries of the smash table, the chosen list being the table itself: rho0, Delta++ and omega in turn, 50 per event"""
    idx = ref.prepare(table)["index"]
    rng = np.random.default_rng(11)
    kinds = [idx[113], idx[2224], idx[223]]
    return ref.make_particles(api, table, table["mc_id"], [kinds[i % 3] for i in range(300)], rng.normal(size=(300, 3)) * 0.6, events=np.arange(300) // 50)


def test_decay_particles_flow_diff_is_the_host_route_on_the_decayed_list(table, primaries):
    slot, ids = api.stable_slots(table, [211, -211, 2212])
    S, cuts = len(ids), D.cuts_for(DECAY_EDGES)
    assert S == 3
    out, _, st = api.decay_particles(table, table["mc_id"], primaries, seed=cases.SEED, lifetime=0)
    pT = np.sqrt(out["px"] ** 2 + out["py"] ** 2)
    # the device builds the momenta itself (agreement with the host's to 1.5e-12): no particle within 1e-9 of a decision
    assert F.edge_distance(cuts, out) > 1e-9 and np.abs(pT[:, None] - DECAY_EDGES[None, :]).min() > 1e-9
    want = api.flow_diff_list(cuts, DECAY_EDGES, N_DECAY_EVENTS, S, slot, out)
    kept = int(want["m"][..., 0].sum())
    assert 200 < kept < len(out) and (want["m"][..., 0].sum(axis=(0, 1)) > 0).sum() >= 4 and st["n_decays"] >= 300
    got = {}
    for form in FORMS:
        got[form], dst = api.decay_particles_flow_diff(table, table["mc_id"], primaries, slot, S, dict(cuts, kernel_form=form), DECAY_EDGES, N_DECAY_EVENTS,
                                                       seed=cases.SEED)
        D.assert_records(got[form], want, ("decayed", form))
        assert dst["n_final"] == len(out) and dst["n_unbinned"] == len(out) - kept and dst["n_decays"] == st["n_decays"]
    assert D.same_bits(got[0], got[1]) and D.same_bits(got[0], got[2])
    # summed over the bins: the records of the plain sink
    flow, fst = api.decay_particles_flow(table, table["mc_id"], primaries, slot, S, cuts, N_DECAY_EVENTS, seed=cases.SEED)
    assert F.same_bits(D.sum_over_bins(got[0]), flow) and fst["n_unbinned"] == dst["n_unbinned"]
    # two pieces with first_particle, cut inside an event: the same bits
    parts = [api.decay_particles_flow_diff(table, table["mc_id"], primaries[lo:hi], slot, S, cuts, DECAY_EDGES, N_DECAY_EVENTS, seed=cases.SEED,
                                           first_particle=lo) for lo, hi in ((0, 131), (131, 300))]
    assert D.same_bits(D.add_records(parts[0][0], parts[1][0]), got[0])
    for k in ("n_final", "n_unbinned", "n_decays"):
        assert parts[0][1][k] + parts[1][1][k] == dst[k], k


# ---- the sampler route: 400 cells x 6 events, pi+ K+ p ----
SAMPLER_EDGES = api.flow_diff_edges(0.2, 3.0, 7)
SAMPLER_CUTS = D.cuts_for(SAMPLER_EDGES)


@pytest.fixture(scope="module")
def sampler_case(fx, table):
    import torch
    sp, gla, o = inputs.species([211, 321, 2212]), inputs.feqmod_tables(0.15), dict(dimension=3, df_mode=2)
    cells = {k: v.copy() for k, v in synth.synth_surface(400, 3, seed=861).items()}
    for f in ("dat", "dax", "day", "dan"):
        cells[f] *= 300.0
    kw = dict(n_events=6, seed=19, y_cut=0.5)
    plist, _ = api.sample_particles(cells, sp, fx["df"], gla, o, **kw)
    dev = torch.device("cuda:0")
    tens = {k: torch.from_numpy(np.ascontiguousarray(cells[k])).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    slot_d, ids = api.stable_slots(table, [211, 321, 2212])
    r = dict(sp=sp, gla=gla, o=o, df=fx["df"], cells=cells, kw=kw, list=plist, tens=tens, ptrs=ptrs, slot=np.arange(3, dtype=np.int32), slot_d=slot_d, S_d=len(ids),
             plan=api.SamplerPlan(sp, fx["df"], gla, o, max_cells=400, y_cut=0.5), dtable=api.DecayMcTable(table, sp["mc_id"], device=0))
    yield r
    r["plan"].close()


def run_diff(r, batch_events, decayed=True, cuts=SAMPLER_CUTS):
    return r["plan"].execute_flow_diff(400, r["ptrs"], 6, 19, cuts, SAMPLER_EDGES, r["slot"], 3, table=r["dtable"] if decayed else None,
                                       slot_decayed=r["slot_d"], n_slots_decayed=r["S_d"], decay_seed=77, lifetime=0, x_ptr=r["ptrs"]["x"],
                                       y_ptr=r["ptrs"]["y"], batch_events=batch_events)


def test_execute_flow_diff_is_the_list_route_for_every_batching(table, sampler_case):
    import torch
    r = sampler_case
    plan, ptrs, plist = r["plan"], r["ptrs"], r["list"]
    want = api.flow_diff_list(SAMPLER_CUTS, SAMPLER_EDGES, 6, 3, r["slot"], plist)
    assert len(plist) >= 100 and want["m"][..., 0].sum() > 50
    want_d, dst_want = api.decay_particles_flow_diff(table, r["sp"]["mc_id"], plist, r["slot_d"], r["S_d"], SAMPLER_CUTS, SAMPLER_EDGES, 6, seed=77)

    def older():
        buf = torch.zeros(len(plist) * api.PARTICLE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        n, _ = plan.execute(400, ptrs, 6, 19, particles_ptr=buf.data_ptr(), capacity=len(plist), x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        flow, _ = plan.execute_flow(400, ptrs, 6, 19, SAMPLER_CUTS, r["slot"], 3, x_ptr=ptrs["x"], y_ptr=ptrs["y"])
        return np.frombuffer(buf.cpu().numpy().tobytes(), dtype=api.PARTICLE_DTYPE)[:n], flow

    before = older()
    assert np.array_equal(before[0], plist)
    first = None
    for batch_events in (1, 4, 6):
        rec, rec_d, st, dst = run_diff(r, batch_events)
        D.assert_records(rec, want, batch_events)
        assert st["n_particles"] == len(plist) == dst["n_primaries"]
        assert D.same_bits(rec_d, want_d) and dst["n_final"] == dst_want["n_final"] and dst["n_unbinned"] == dst_want["n_unbinned"]
        first = first or (rec, rec_d)
        assert D.same_bits(rec, first[0]) and D.same_bits(rec_d, first[1]), batch_events
    for form in (1, 2):
        rec, rec_d, _, _ = run_diff(r, 4, cuts=dict(SAMPLER_CUTS, kernel_form=form))
        assert D.same_bits(rec, first[0]) and D.same_bits(rec_d, first[1]), form
    only, st = run_diff(r, 0, decayed=False)
    assert D.same_bits(only, first[0]) and st["n_particles"] == len(plist)
    # the plan then serves execute_flow and execute unchanged; the bins add up to execute_flow's records
    after = older()
    assert np.array_equal(before[0], after[0]) and F.same_bits(before[1], after[1]) and F.same_bits(D.sum_over_bins(first[0]), after[1])
    # ... and the one-shot entry is the plan's
    rec, rec_d, st, dst = api.sample_flow_diff(r["cells"], r["sp"], r["df"], r["gla"], SAMPLER_CUTS, SAMPLER_EDGES, r["slot"], 3, r["o"], table=table,
                                               chosen_mc_id=r["sp"]["mc_id"], slot_decayed=r["slot_d"], n_slots_decayed=r["S_d"], decay_seed=77,
                                               batch_events=4, **r["kw"])
    assert D.same_bits(rec, first[0]) and D.same_bits(rec_d, first[1]) and st["n_particles"] == len(plist)


# ---- the run driver ----
def test_driver_writes_the_differential_files_and_leaves_every_other_file_as_it_was(tmp_path, reference):
    """The 2+1D toy run of tests/test_gpu_flow.py with test_sampler_decayed = 1 and test_sampler_flow = 1, with and without
    test_sampler_flow_diff = 1: the run with the key writes differential_<label>.dat beside the flow files, for the thermal and the decayed
    hadrons; every other file is byte for byte what the run without the key writes."""
    ids = [211, 321, 2212, 113, 223, 2224, -2224, 221, -211]
    cells = synth.synth_surface(3000, 2, seed=92)
    sub = ("dN_dy", "dN_deta", "momentum_distribution", "vn", "spacetime_distribution", "flow")
    files, stdout = {}, {}
    for diff in (0, 1):
        root = refformat.make_run_dir(str(tmp_path / ("diff%d" % diff)), cells, ids,
                                      dict(operation=2, dimension=2, df_mode=2, sampler_seed=17, oversample=1, min_num_hadrons=2000, test_sampler=1))
        shutil.copy(os.path.join(reference, "PDG", "pdg-urqmd_v3.3+.dat"), os.path.join(root, "PDG", "pdg-urqmd_v3.3+.dat"))
        with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
            f.write("test_sampler_on_device\t= 1\ntest_sampler_decayed\t= 1\ntest_sampler_flow\t= 1\nflow_y_cut = 0.4\nflow_y_gap = 0.2\nflow_pT_min = 0.1\n" +
                    ("test_sampler_flow_diff = 1\nflow_diff_pt_bins = 6\nflow_diff_pt_max = 2.5\n" if diff else ""))
        for d in sub:
            os.makedirs(os.path.join(root, "results", d), exist_ok=True)
            os.makedirs(os.path.join(root, "results", "decayed", d))
        r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        files[diff] = {os.path.relpath(os.path.join(dp, f), os.path.join(root, "results")): open(os.path.join(dp, f), "rb").read()
                       for dp, _, fs in os.walk(os.path.join(root, "results")) for f in fs}
        stdout[diff] = r.stdout
    is_diff = lambda k: os.path.basename(k).startswith("differential_")  # noqa: E731
    assert not any(is_diff(k) for k in files[0]) and "differential flow" not in stdout[0] and "differential flow records on the device" in stdout[1]
    assert {k: v for k, v in files[1].items() if not is_diff(k)} == files[0] and len(files[0]) > 20
    labels = ("211", "321", "2212", "other", "all")
    want = sorted(os.path.join(d, "differential_%s.dat" % l) for d in ("flow", os.path.join("decayed", "flow")) for l in labels)
    assert sorted(k for k in files[1] if is_diff(k)) == want
    edges = api.flow_diff_edges(0.1, 2.5, 6)
    for base_dir in ("flow", os.path.join("decayed", "flow")):
        rows = {l: np.loadtxt(tmp_path / "diff1" / "results" / base_dir / ("differential_%s.dat" % l)) for l in labels}
        for l, t in rows.items():
            assert t.shape == (6 * 8, 12) and np.all(np.isfinite(t)), l
            assert np.array_equal(t[::8, 0], np.arange(6)) and np.allclose(t[::8, 1], edges[:-1], rtol=1e-8) and np.allclose(t[::8, 2], edges[1:], rtol=1e-8)
        # "all" is the sum of the slots, and its counts are those of the flow file of the same cuts below flow_diff_pt_max
        assert np.array_equal(sum(rows[l][:, 11] for l in labels[:-1]), rows["all"][:, 11]) and rows["all"][:, 11].sum() > 100
    pions_thermal = np.loadtxt(tmp_path / "diff1" / "results" / "flow" / "differential_211.dat")[::8, 11].sum()
    pions_decayed = np.loadtxt(tmp_path / "diff1" / "results" / "decayed" / "flow" / "differential_211.dat")[::8, 11].sum()
    assert pions_decayed > pions_thermal > 0                                # the rho0, omega, Delta++ and eta feed the pi+
