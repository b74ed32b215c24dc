"""Shared cases of the flow-record tests (tests/test_flow_host.py, tests/test_gpu_flow.py): particle lists made by hand, a numpy restatement
of the per-particle region rule, and the comparison of device records with the host route's."""
from functools import lru_cache

import numpy as np

from is3d_amd import api

CUTS = dict(api.FLOW_CUTS)             # y_cut 1.0, y_gap 0.5, pT in [0.2, 3.0)
N_SPECIES = 41
HAND_SIZES = (1, 63, 64, 65, 0, 257)   # event boundaries at lane 0, at lane 63 and mid-workgroup; an empty event; one event across workgroups
HAND_TAIL = 200                        # ... and a tail of events of one or two particles: more events in one slice than any window holds


def kinematic_list(rng, events, n_species=N_SPECIES, mass=0.13957):
    """One particle per entry of `events`: rapidity in [-1.5, 1.5], pT in [0.05, 3.5], any azimuth -- on both sides of every cut."""
    n = len(events)
    p = np.zeros(n, dtype=api.PARTICLE_DTYPE)
    y, pT, phi = rng.uniform(-1.5, 1.5, n), rng.uniform(0.05, 3.5, n), rng.uniform(-np.pi, np.pi, n)
    mT = np.sqrt(mass * mass + pT * pT)
    p["E"], p["pz"], p["px"], p["py"] = mT * np.cosh(y), mT * np.sinh(y), pT * np.cos(phi), pT * np.sin(phi)
    p["event"] = events
    p["species"] = rng.integers(0, n_species, n)
    p["cell"] = np.arange(n)
    return p


@lru_cache(maxsize=None)
def hand_list():
    """(particles ordered by event, n_events): about 750 particles, the event sizes of HAND_SIZES, then HAND_TAIL events of 1 or 2."""
    rng = np.random.default_rng(20270)
    sizes = list(HAND_SIZES) + [1 + int(k) for k in rng.integers(0, 2, HAND_TAIL)]
    events = np.repeat(np.arange(len(sizes)), sizes)
    p = kinematic_list(rng, events)
    p.setflags(write=False)
    return p, len(sizes)


@lru_cache(maxsize=None)
def shuffled_list():
    p, n_events = hand_list()
    q = p[np.random.default_rng(7).permutation(len(p))]
    q.setflags(write=False)
    return q, n_events


@lru_cache(maxsize=None)
def long_list():
    """(particles, n_events): 9001 particles in 5 uneven events -- three workgroups of the private form, whose slices every event but the
    first crosses, and a ragged last trip."""
    rng = np.random.default_rng(20271)
    events = np.repeat(np.arange(5), (700, 3000, 1, 4000, 1300))
    p = kinematic_list(rng, events)
    p.setflags(write=False)
    return p, 5


def slot_map(n_slots, n_species=N_SPECIES):
    """species -> slot with slot -1 present: a few slots share out the species round robin; many slots take one species each."""
    s = np.arange(n_species)
    if n_slots < n_species:
        return (s % (n_slots + 1) - 1).astype(np.int32)
    return np.where(s < n_species - 1, s, -1).astype(np.int32)


def numpy_regions(cuts, p):
    """The region rule restated: -1 nothing, 0 full acceptance only, 1 sub-event A, 2 sub-event B (correctly rounded +, -, *, /, sqrt, as the
    library's rule; the four thresholds through numpy's exp)."""
    lo, hi, a, b = np.exp(-2.0 * cuts["y_cut"]), np.exp(2.0 * cuts["y_cut"]), np.exp(-cuts["y_gap"]), np.exp(cuts["y_gap"])
    den = p["E"] - p["pz"]
    with np.errstate(all="ignore"):
        ratio = (p["E"] + p["pz"]) / den
        pT = np.sqrt(p["px"] * p["px"] + p["py"] * p["py"])
    ok = (den > 0.0) & (ratio >= lo) & (ratio <= hi) & (pT >= cuts["pT_min"]) & (pT < cuts["pT_max"])
    return np.where(~ok, -1, np.where(ratio < a, 1, np.where(ratio > b, 2, 0)))


def numpy_M(cuts, n_events, n_slots, slot, p):
    """M [event][slot][3] by the restatement."""
    M = np.zeros((n_events, n_slots, 3), dtype=np.int64)
    reg, s = numpy_regions(cuts, p), np.asarray(slot)[p["species"]]
    keep = (reg >= 0) & (s >= 0)
    np.add.at(M, (p["event"][keep], s[keep], 0), 1)
    sub = keep & (reg > 0)
    np.add.at(M, (p["event"][sub], s[sub], reg[sub]), 1)
    return M


def thermal_surface():
    """(cells, species, gla, opts, kw) of the independence tests: pi+ alone, a 400-cell 3+1D surface (its volumes times 100, for about 190
    hadrons per event) x 60 events.  Chosen on the CPU so that every event has at least two hadrons in each sub-event of CUTS."""
    from is3d_amd import inputs, synth
    cells = {k: v.copy() for k, v in synth.synth_surface(400, 3, seed=861).items()}
    for f in ("dat", "dax", "day", "dan"):
        cells[f] *= 100.0
    return cells, inputs.species([211]), inputs.feqmod_tables(0.15), dict(dimension=3, df_mode=2), dict(n_events=60, seed=20270, y_cut=0.5)


def independence_pulls(records, harmonics=(2, 3)):
    """{n: (c_n{2,gap} - Re(qbar_A qbar_B*)) / sigma} of slot 0, qbar = sum Q / sum M over events, sigma the delete-one-event jackknife error
    of the difference.  Asserts that every event has M_A, M_B >= 2."""
    M = records["M"][:, 0, :].astype(np.float64)
    assert M[:, 1].min() >= 2 and M[:, 2].min() >= 2, (M[:, 1].min(), M[:, 2].min())
    N, scale = len(M), 2.0 ** 32
    c_lib = api.flow_cumulants(records)["c2_gap"][0]
    pulls = {}
    for n in harmonics:
        QA = (records["Q_re"][:, 0, 1, n - 1] + 1j * records["Q_im"][:, 0, 1, n - 1]) / scale
        QB = (records["Q_re"][:, 0, 2, n - 1] + 1j * records["Q_im"][:, 0, 2, n - 1]) / scale
        num, w = (QA * np.conj(QB)).real, M[:, 1] * M[:, 2]

        def diff(k):
            return num[k].sum() / w[k].sum() - ((QA[k].sum() / M[k, 1].sum()) * np.conj(QB[k].sum() / M[k, 2].sum())).real

        every = np.arange(N)
        assert abs(num.sum() / w.sum() - c_lib[n - 1]) < 1e-12
        jack = np.array([diff(np.delete(every, e)) for e in range(N)])
        sigma = np.sqrt((N - 1.0) / N * ((jack - jack.mean()) ** 2).sum())
        pulls[n] = float(diff(every) / sigma)
    return pulls


def edge_distance(cuts, p):
    """The smallest distance of a particle from a region decision: in rapidity from -y_cut, -y_gap / 2, y_gap / 2, y_cut, in pT from pT_min
    and pT_max.  Lists whose momenta the device computes itself (decays) agree with the host's to 1.5e-12: with every particle further than
    1e-9 from a decision, host and device reach the same regions."""
    if len(p) == 0:
        return np.inf
    with np.errstate(all="ignore"):
        y = 0.5 * np.log((p["E"] + p["pz"]) / (p["E"] - p["pz"]))
    pT = np.sqrt(p["px"] ** 2 + p["py"] ** 2)
    edges = (-cuts["y_cut"], -0.5 * cuts["y_gap"], 0.5 * cuts["y_gap"], cuts["y_cut"])
    d = [np.nanmin(np.abs(y - e)) for e in edges] + [np.abs(pT - cuts["pT_min"]).min(), np.abs(pT - cuts["pT_max"]).min()]
    return float(min(d))


def assert_records(got, want, what):
    """M bit for bit; every Q word within M units of its record (device and host libm differ by ulps, far below a step of 2^-32, so one
    rounding of term * 2^32 moves a term by at most one step)."""
    assert np.array_equal(got["M"], want["M"]), (what, "M")
    for k in ("Q_re", "Q_im"):
        d = np.abs(got[k] - want[k])
        assert np.all(d <= want["M"][..., None]), (what, k, int(d.max()))


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("M", "Q_re", "Q_im"))
