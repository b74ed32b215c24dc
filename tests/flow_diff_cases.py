"""Shared cases of the differential-flow tests (tests/test_flow_diff_host.py, tests/test_flow_diff_abi.py, tests/test_gpu_flow_diff.py): edge
tables, hand-made lists, a brute-force restatement of the differential correlators over distinct pairs and 4-tuples, and the comparison of
device records with the host route's."""
from functools import lru_cache

import numpy as np

import flow_cases as F
from is3d_amd import api

N_SPECIES = F.N_SPECIES
EDGES = api.flow_diff_edges(0.2, 3.0, 14)                  # the run driver's default table
CUTS = dict(F.CUTS, pT_min=float(EDGES[0]), pT_max=float(EDGES[-1]))
# non-uniform, over several binades, no edge a round multiple of the others
WIDE_EDGES = np.array([2.0 ** -6, 0.03, 0.11, 0.125, 0.7, 1.0, 1.0000000000000002, 2.5, 37.0], dtype=np.float64)
SCALE = 2.0 ** 32


def cuts_for(edges, **kw):
    return dict(F.CUTS, pT_min=float(edges[0]), pT_max=float(edges[-1]), **kw)


def particles_at(pT, phi, y, events, species, mass=0.13957):
    """Particles with px = pT cos(phi), py = pT sin(phi) as numpy rounds them."""
    pT, phi, y = np.broadcast_arrays(np.asarray(pT, np.float64), np.asarray(phi, np.float64), np.asarray(y, np.float64))
    p = np.zeros(len(pT), dtype=api.PARTICLE_DTYPE)
    mT = np.sqrt(mass * mass + pT * pT)
    p["E"], p["pz"], p["px"], p["py"] = mT * np.cosh(y), mT * np.sinh(y), pT * np.cos(phi), pT * np.sin(phi)
    p["event"], p["species"], p["cell"] = events, species, np.arange(len(pT))
    return p


def on_axis(pT, axis, y, events, species, mass=0.13957):
    """Particles whose transverse momentum lies on an axis (0: +x, 1: +y, 2: -x, 3: -y): sqrt(px^2 + py^2) is pT bit for bit, and the
    fixed-point terms of every harmonic are exact (0 or +-2^32)."""
    pT, axis, y = np.broadcast_arrays(np.asarray(pT, np.float64), np.asarray(axis), np.asarray(y, np.float64))
    p = np.zeros(len(pT), dtype=api.PARTICLE_DTYPE)
    mT = np.sqrt(mass * mass + pT * pT)
    p["E"], p["pz"] = mT * np.cosh(y), mT * np.sinh(y)
    p["px"] = np.where(axis == 0, pT, np.where(axis == 2, -pT, 0.0))
    p["py"] = np.where(axis == 1, pT, np.where(axis == 3, -pT, 0.0))
    p["event"], p["species"], p["cell"] = events, species, np.arange(len(pT))
    return p


def numpy_bins(edges, p):
    """The bin rule restated: the b with edges[b] <= pT < edges[b + 1], or -1; pT with correctly rounded *, + and sqrt as the library's."""
    with np.errstate(all="ignore"):
        pT = np.sqrt(p["px"] * p["px"] + p["py"] * p["py"])
    b = np.searchsorted(edges, pT, side="right") - 1
    return np.where((pT >= edges[0]) & (pT < edges[-1]), b, -1)


def numpy_m(cuts, edges, n_events, n_slots, slot, p):
    """m [event][slot][bin][3] by the restatements of the region and the bin."""
    m = np.zeros((n_events, n_slots, len(edges) - 1, 3), dtype=np.int64)
    reg, b, s = F.numpy_regions(cuts, p), numpy_bins(edges, p), np.asarray(slot)[p["species"]]
    keep = (reg >= 0) & (s >= 0)
    assert np.all(b[keep] >= 0)
    np.add.at(m, (p["event"][keep], s[keep], b[keep], 0), 1)
    sub = keep & (reg > 0)
    np.add.at(m, (p["event"][sub], s[sub], b[sub], reg[sub]), 1)
    return m


def sum_over_bins(rec):
    """Differential records -> the flow records they must add up to."""
    return dict(M=rec["m"].sum(axis=2), Q_re=rec["p_re"].sum(axis=2), Q_im=rec["p_im"].sum(axis=2))


def assert_records(got, want, what):
    """m bit for bit; every p word within m units of its record (the contract of the flow records)."""
    assert np.array_equal(got["m"], want["m"]), (what, "m")
    for k in ("p_re", "p_im"):
        d = np.abs(got[k] - want[k])
        assert np.all(d <= want["m"][..., None]), (what, k, int(d.max()))


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("m", "p_re", "p_im"))


def add_records(a, b):
    return {k: a[k] + b[k] for k in ("m", "p_re", "p_im")}


@lru_cache(maxsize=None)
def random_list(seed=20300, n_events=3, n=200, n_species=N_SPECIES):
    """About n particles over n_events events, on both sides of every cut of CUTS / EDGES."""
    rng = np.random.default_rng(seed)
    p = F.kinematic_list(rng, np.sort(rng.integers(0, n_events, n)), n_species)
    p.setflags(write=False)
    return p


# ---- the brute force: differential correlators of ONE event from the particles' angles, over distinct pairs and 4-tuples ----
QUARTER_COS = np.array([1.0, 0.0, -1.0, 0.0])


def quarter_cos(x):
    """cos(x pi / 2) of an integer array x, exactly."""
    return QUARTER_COS[np.asarray(x) % 4]


def brute_event(phi, poi, ref, n, cos=np.cos):
    """(<2'> numerator, weight, <4'> numerator, weight) of harmonic n for one event: phi the angles, poi / ref boolean masks.  Explicit sums
    over ordered tuples of DISTINCT particles, the first a particle of interest, the others reference particles.  cos: np.cos for angles in
    radians, quarter_cos for integer quarter turns (exact)."""
    phi = np.asarray(phi)
    P, R = np.nonzero(poi)[0], np.nonzero(ref)[0]
    if len(P) == 0 or len(R) == 0:
        return 0.0, 0.0, 0.0, 0.0
    i, j = P[:, None], R[None, :]
    d = i != j
    n2, w2 = float(cos(n * (phi[i] - phi[j]))[d].sum()), float(d.sum())
    i, j, k, l = P[:, None, None, None], R[None, :, None, None], R[None, None, :, None], R[None, None, None, :]
    d = (i != j) & (i != k) & (i != l) & (j != k) & (j != l) & (k != l)
    n4, w4 = float(cos(n * (phi[i] + phi[j] - phi[k] - phi[l]))[d].sum()), float(d.sum())
    return n2, w2, n4, w4


def brute_gap(phi, poi, ref, sub, n, cos=np.cos):
    """(<2'>_gap numerator, weight): pairs of a particle of interest in one sub-event with a reference particle in the other (sub: 1 A, 2 B,
    0 neither)."""
    phi, sub = np.asarray(phi), np.asarray(sub)
    num = w = 0.0
    for a, b in ((1, 2), (2, 1)):
        i, j = np.nonzero(poi & (sub == a))[0][:, None], np.nonzero(ref & (sub == b))[0][None, :]
        if i.size and j.size:
            num += float(cos(n * (phi[i] - phi[j])).sum())
            w += float(i.size * j.size)
    return num, w
