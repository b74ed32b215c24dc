"""GPU (-m gpu): is3d_decay_particles, the Monte Carlo decay of a sampled list to stable particles on the device.

Parity: the device's list against the scalar restatement (tests/decays_mc_ref.py, float64) on hand-made lists of 1, 63, 65 and 257 primaries
(rho0 -> pi pi, eta -> gamma gamma, omega -> pi0 gamma and 3 pi, a parent with a 4-body channel, a parent at rest, one at |p| = 20 GeV) and on
one primary of every unstable species of each shipped table: counts, species, origin, cell and event identical, no primary left out, momenta
and positions within BOUND = 64 x FLOOR = 64 x 2.4e-14 = 1.536e-12 (tests/decays_mc_cases.py: FLOOR is the restatement in float64 against
longdouble on these lists, measured 2.32e-14, relative to the primary's energy).  The same bound serves the conservation and mass-shell checks
on the device output alone.  Then the calling pattern, the bits (two runs; a list decayed in pieces), statistics with bounds from counting
statistics, the one parent without an open channel, and the run driver's decay_sampled_hadrons."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import decays_mc_cases as cases
import decays_mc_ref as ref
import refformat
from is3d_amd import api, synth
from oracle import oracle  # the checker's Philox stream, for the restatement

pytestmark = pytest.mark.gpu
URQMD, SMASH = "pdg-urqmd_v3.3+.dat", "pdg_smash.dat"
_cache = {}


@pytest.fixture(scope="module")
def tabs(reference):
    t = cases.tables(api, reference)
    return {k: (v, ref.prepare(v)) for k, v in t.items()}


def primaries(tabs, which):
    if which not in _cache:
        name = SMASH if which == "every-smash" else URQMD
        t, prep = tabs[name]
        _cache[which] = (t, prep, cases.hand_list(api, t, prep) if which == "hand" else cases.every_unstable(api, t, 3))
    return _cache[which]


def restated(tabs, which, lifetime):
    """the restatement of a whole list, computed once and never changed"""
    key = (which, lifetime)
    if key not in _cache:
        t, prep, q = primaries(tabs, which)
        _cache[key] = ref.decay_particles(t, t["mc_id"], q, oracle.rng_uniforms, cases.SEED, 0, lifetime, np.float64, prep)
    return _cache[key]


def device(t, q, lifetime=0, seed=cases.SEED, **kw):
    out, origin, st = api.decay_particles(t, t["mc_id"], q, seed=seed, lifetime=lifetime, **kw)
    assert st["n_exhausted"] == 0 and st["n_final"] == len(out) == len(origin) and st["n_primaries"] == len(q)
    return out, origin, st


def finals_of(r, i):
    return sorted(int(e) for e in r["species"][r["origin"] == i])


def test_hand_list_covers_its_cases(tabs):
    """the 257 hand-made primaries do hold what the parity test is meant to see (read off the restatement)"""
    t, prep, q = primaries(tabs, "hand")
    r = restated(tabs, "hand", 0)
    idx = prep["index"]
    per = {i: finals_of(r, i) for i in range(len(q))}
    of = lambda e: [per[i] for i in range(len(q)) if q["species"][i] == e]  # noqa: E731
    assert sorted([idx[211], idx[-211]]) in of(idx[113])
    assert [idx[22], idx[22]] in of(idx[221])
    assert sorted([idx[111], idx[22]]) in of(idx[223]) and sorted([idx[211], idx[-211], idx[111]]) in of(idx[223])
    four = cases.four_body_parent(t, prep)
    assert any(len(f) >= 4 for f in of(four)) and any(n == 4 for _, n, _ in prep["open"][four])
    assert q["px"][0] == q["py"][0] == q["pz"][0] == 0.0 and abs(np.sqrt(q["px"][1] ** 2 + q["py"][1] ** 2 + q["pz"][1] ** 2) - 20.0) < 0.1


@pytest.mark.parametrize("which,n,lifetime", [("hand", 1, 0), ("hand", 63, 0), ("hand", 65, 0), ("hand", 257, 0), ("hand", 257, 1),
                                              ("every-urqmd", 303, 0), ("every-urqmd", 303, 1), ("every-smash", 346, 0), ("every-smash", 346, 1)])
def test_parity_with_the_restatement(tabs, which, n, lifetime):
    t, prep, q = primaries(tabs, which)
    assert len(q) >= n and (which == "hand" or len(q) == n)
    r = restated(tabs, which, lifetime)
    keep = r["origin"] < n             # a primary's tree depends on its own index only: the first n primaries of the whole list
    out, origin, st = device(t, q[:n], lifetime)
    assert len(out) == int(keep.sum())
    assert np.array_equal(out["species"], r["species"][keep]) and np.array_equal(origin, r["origin"][keep])
    assert np.array_equal(out["cell"], r["cell"][keep]) and np.array_equal(out["event"], r["event"][keep])
    assert np.array_equal(np.unique(origin), np.arange(n))                  # no primary left out
    assert np.all(np.diff(origin) >= 0) and np.all(np.diff(out["event"]) >= 0)
    mom, pos = cases.device_arrays(out)
    d = cases.distance(mom, pos, r["mom"][keep], r["pos"][keep], origin, q)
    print("%s n = %d lifetime = %d: %d final particles, distance %.3g (bound %.3g)" % (which, n, lifetime, len(out), d, cases.BOUND))
    assert d <= cases.BOUND
    if n == len(q):
        for k in ("n_decays", "n_stuck", "n_trials", "n_exhausted", "max_stack", "max_depth", "n_closed_channels"):
            assert st[k] == r["stats"][k], k


@pytest.mark.parametrize("which,lifetime", [("hand", 0), ("hand", 1), ("every-urqmd", 0), ("every-smash", 1)])
def test_conservation_and_mass_shell_on_the_device_output_alone(tabs, which, lifetime):
    t, prep, q = primaries(tabs, which)
    out, origin, st = device(t, q, lifetime, seed=99)
    mom, _ = cases.device_arrays(out)
    tot = np.zeros((len(q), 4), np.longdouble)
    np.add.at(tot, origin, mom.astype(np.longdouble))
    P0 = np.stack([q[k] for k in ref.MOM], 1)
    cons = float(np.max(np.abs(tot - P0) / q["E"][:, None]))
    m, E = t["mass"][out["species"]], out["E"]
    shell = float(np.max(np.abs(E * E - out["px"] ** 2 - out["py"] ** 2 - out["pz"] ** 2 - m * m) / (E * E)))
    print("%s lifetime = %d: conservation %.3g, mass shell %.3g (bound %.3g)" % (which, lifetime, cons, shell, cases.BOUND))
    assert cons <= cases.BOUND and shell <= cases.BOUND
    unstable = out["species"][t["stable"][out["species"]] == 0]
    assert all(not prep["open"][e] for e in unstable) and len(unstable) == st["n_stuck"]


def test_calling_pattern(tabs):
    t, prep, q = primaries(tabs, "hand")
    full, origin, st = device(t, q)
    n = len(full)
    L = api.load()
    ts, ch, _, keep = api._decay_pack(t, t["mc_id"], dict(pT=[1.0], phi=[0.0], y=[0.0]))
    inp, cnt, stats = api.DecayMcInputs(cases.SEED, 0, 0, -1), ctypes.c_int64(0), api.DecayMcStats()
    L.is3d_decay_particles.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    head = [ctypes.addressof(ts), len(ch), ch.ctypes.data, ctypes.addressof(inp), len(q), q.ctypes.data]
    # the count call: no list, the full count
    assert L.is3d_decay_particles(*head, None, None, 0, ctypes.addressof(cnt), ctypes.addressof(stats)) == api.IS3D_OK
    assert cnt.value == n == stats.n_final and stats.ms_fill == 0.0
    # a list one short: IS3D_ENOMEM, the full count, nothing written
    buf = np.zeros(n, api.PARTICLE_DTYPE)
    buf["cell"], buf["E"] = -7, -1.0
    org = np.full(n, -9, np.int64)
    before, cnt.value = buf.copy(), 0
    assert L.is3d_decay_particles(*head, buf.ctypes.data, org.ctypes.data, n - 1, ctypes.addressof(cnt), None) == api.IS3D_ENOMEM
    assert cnt.value == n and buf.tobytes() == before.tobytes() and np.all(org == -9)
    # origin may be NULL
    assert L.is3d_decay_particles(*head, buf.ctypes.data, None, n, ctypes.addressof(cnt), None) == api.IS3D_OK
    assert cnt.value == n and buf.tobytes() == full.tobytes()
    # an empty list
    out, origin0, st0 = api.decay_particles(t, t["mc_id"], q[:0])
    assert len(out) == 0 and st0["n_final"] == 0 and st0["max_stack"] == 5
    # stable species come back unchanged but for the species, which indexes the table
    chosen = [211, -211, 321, 2212]
    s = ref.make_particles(api, t, chosen, [k % 4 for k in range(65)], np.random.default_rng(5).normal(size=(65, 3)))
    out, origin1, st1 = api.decay_particles(t, chosen, s, lifetime=1)
    assert len(out) == 65 and np.array_equal(origin1, np.arange(65)) and st1["n_decays"] == 0 and st1["n_trials"] == 0
    assert np.array_equal(t["mc_id"][out["species"]], np.array(chosen)[s["species"]])
    same = out.copy()
    same["species"] = s["species"]
    assert same.tobytes() == s.tobytes()


def test_bits(tabs):
    t, prep, q = primaries(tabs, "hand")
    for lifetime in (0, 1):
        a, ao, _ = device(t, q, lifetime)
        b, bo, _ = device(t, q, lifetime)
        assert a.tobytes() == b.tobytes() and np.array_equal(ao, bo)
        h, ho, _ = device(t, q[:100], lifetime)
        k, ko, _ = device(t, q[100:], lifetime, first_particle=100)
        assert np.concatenate([h, k]).tobytes() == a.tobytes() and np.array_equal(np.concatenate([ho, ko + 100]), ao)
        c, _, _ = device(t, q, lifetime, seed=cases.SEED + 1)
        assert c.tobytes() != a.tobytes()


N_STAT = 20000


def test_channel_frequencies(tabs):
    """20 000 eta of the urqmd table (at least 3 open channels, every daughter stable, so the final state names the channel): every channel
    within 5 multinomial sigma of its ratio renormalised over the open channels"""
    t, prep = tabs[URQMD]
    eta = prep["index"][221]
    chs = prep["open"][eta]
    states = [tuple(sorted(ds)) for _, _, ds in chs]
    assert len(chs) >= 3 and len(set(states)) == len(states) and all(t["stable"][d] for s in states for d in s)
    q = ref.make_particles(api, t, t["mc_id"], [eta] * N_STAT, np.random.default_rng(1).normal(size=(N_STAT, 3)) * 0.5)
    out, origin, st = device(t, q, seed=77)
    first = np.concatenate([np.nonzero(np.diff(origin, prepend=-1))[0], [len(out)]])
    seen = {}
    for i in range(N_STAT):
        s = tuple(sorted(int(e) for e in out["species"][first[i]:first[i + 1]]))
        seen[s] = seen.get(s, 0) + 1
    assert set(seen) <= set(states)
    cum = [float(c) for c, _, _ in chs]
    for j, s in enumerate(states):
        p = (cum[j] - (cum[j - 1] if j else 0.0)) / cum[-1]
        assert abs(seen.get(s, 0) - N_STAT * p) <= 5.0 * np.sqrt(N_STAT * p * (1.0 - p)), (s, seen.get(s, 0), N_STAT * p)


def test_two_body_angle_lifetime_and_width_zero(tabs):
    t, prep = tabs[URQMD]
    idx = prep["index"]
    rho, eta = idx[113], idx[221]
    # rho0 at rest: the first daughter's direction is isotropic
    q = ref.make_particles(api, t, t["mc_id"], [rho] * N_STAT, np.zeros((N_STAT, 3)))
    out, origin, st = device(t, q, seed=31)
    assert len(out) == 2 * N_STAT and st["n_trials"] == st["n_decays"] == N_STAT
    d0 = out[0::2]
    cos = d0["pz"] / np.sqrt(d0["px"] ** 2 + d0["py"] ** 2 + d0["pz"] ** 2)
    assert abs(cos.mean()) <= 5.0 / np.sqrt(3.0 * N_STAT)
    # moving rho0 with lifetime = 1: the proper time between the primary's position and its daughters' is exponential with mean hbarc / width
    q = ref.make_particles(api, t, t["mc_id"], [rho] * N_STAT, np.random.default_rng(2).normal(size=(N_STAT, 3)) * 0.6)
    out, origin, st = device(t, q, lifetime=1, seed=32)
    d0, d1 = out[0::2], out[1::2]
    assert all(np.array_equal(d0[k], d1[k]) for k in ("t", "x", "y", "z", "tau", "eta"))
    dt, dx, dy, dz = d0["t"] - q["t"], d0["x"] - q["x"], d0["y"] - q["y"], d0["z"] - q["z"]
    proper = np.sqrt(np.maximum(dt * dt - dx * dx - dy * dy - dz * dz, 0.0))
    tau0 = ref.HBARC / t["width"][rho]
    assert abs(proper.mean() - tau0) <= 5.0 * tau0 / np.sqrt(N_STAT)
    assert np.max(np.abs(d0["tau"] - np.sqrt(d0["t"] ** 2 - d0["z"] ** 2))) < 1e-9 and np.max(np.abs(np.tanh(d0["eta"]) - d0["z"] / d0["t"])) < 1e-9
    # eta has width 0 in this table: it decays where it is
    assert t["width"][eta] == 0.0 and not t["stable"][eta]
    q = ref.make_particles(api, t, t["mc_id"], [eta] * 257, np.random.default_rng(3).normal(size=(257, 3)) * 0.6)
    out, origin, st = device(t, q, lifetime=1, seed=33)
    assert st["n_decays"] >= 257
    for k in ref.POS:
        assert np.array_equal(out[k], q[k][origin]), k


def test_parent_without_an_open_channel_comes_back_as_itself(tabs):
    t, prep = tabs[URQMD]
    e = prep["index"][10333]
    assert not t["stable"][e] and not prep["open"][e]
    q = ref.make_particles(api, t, [10333], [0], [[0.3, -0.2, 0.5]])
    out, origin, st = api.decay_particles(t, [10333], q, lifetime=1)
    assert len(out) == 1 and st["n_stuck"] == 1 and st["n_decays"] == 0 and out["species"][0] == e
    same = out.copy()
    same["species"] = 0
    assert same.tobytes() == q.tobytes()


def _rows(path):
    lines = [ln for ln in open(path).read().split("\n") if ln and not ln.startswith("#")]
    return np.array([int(ln.split(" ")[0]) for ln in lines], np.int64)


def test_driver_writes_the_decayed_list_beside_the_thermal_one(tmp_path, reference, tabs):
    """a 2+1D toy surface run with and without decay_sampled_hadrons: the thermal file is byte-identical, the decayed file holds only ids that
    are stable in the table (or the one without an open channel) and at least as many rows"""
    ids = [211, 321, 2212, 113, 223, 2224, -2224, 221]
    cells = synth.synth_surface(3000, 2, seed=92)
    t, prep = tabs[URQMD]
    osc = {}
    for key in (0, 1):
        root = refformat.make_run_dir(str(tmp_path / ("key%d" % key)), cells, ids, dict(operation=2, dimension=2, df_mode=2, sampler_seed=17,
                                                                                            oversample=1, min_num_hadrons=2000))
        shutil.copy(os.path.join(reference, "PDG", URQMD), os.path.join(root, "PDG", URQMD))     # the shipped list: the toy one has no decay data
        if key:
            with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
                f.write("decay_sampled_hadrons\t= 1\n")
        r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        osc[key] = open(os.path.join(root, "results", "particle_list_osc.dat"), "rb").read()
        decayed = os.path.join(root, "results", "particle_list_osc_decayed.dat")
        assert os.path.exists(decayed) == bool(key)
        assert ("decays: " in r.stdout) == bool(key)
    assert osc[0] == osc[1]
    thermal, final = _rows(os.path.join(root, "results", "particle_list_osc.dat")), _rows(decayed)
    assert len(final) >= len(thermal) > 100 and set(thermal) - {211, 321, 2212} != set()
    stable = {int(i) for i, s in zip(t["mc_id"], t["stable"]) if s}
    assert set(int(i) for i in final) <= stable
    assert len(final) > len(thermal)
