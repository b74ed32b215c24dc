"""Shared cases of the HBT tests (tests/test_hbt_host.py, tests/test_hbt_abi.py, tests/test_gpu_hbt.py): particle lists made by hand, the
rule of csrc/cf_sampler_hbt.h restated in numpy (every ordered pair of a segment at once: the same IEEE operations in the same order, no
contraction), and the Gaussian sources whose radii are known in closed form."""
from functools import lru_cache

import numpy as np

from is3d_amd import api

HBARC = 0.197327053
M_PI = 0.13957
N_SPECIES = 7
SLOT4 = np.array([0, 1, -1, 2, 3, -1, 1], dtype=np.int32)   # 4 slots, slots 1 and 3 in use, -1 present, two species share slot 1
BINS = dict(y_cut=1.0, pT_min=0.05, pT_max=2.0, kT_min=0.1, kT_max=1.0, n_kT=3, q_max=0.12, n_q=8, kernel_form=0)   # 1536 bins per slot: form 2 fits
BINS_ODD = dict(BINS, n_q=7, n_kT=1, kT_min=0.0)
BINS_BIG = dict(BINS, n_q=20, n_kT=2)                       # 16000 bins per slot: form 2 does not fit
HAND_SIZES = (0, 1, 2, 63, 64, 65, 257)                     # accepted particles of slot 0 in the first events
HAND_TAIL = 200                                             # ... then a tail of events of 1-2 particles
HAND_BIG = 1000                                             # ... then one event of about 1000: several i and j tiles, several work items


def derived(bins):
    return dict(lo=np.exp(-2.0 * bins["y_cut"]), hi=np.exp(2.0 * bins["y_cut"]), dkT=(bins["kT_max"] - bins["kT_min"]) / float(bins["n_kT"]),
                dq=2.0 * bins["q_max"] / float(bins["n_q"]))


def make(p3, x4, species, event, mass=M_PI):
    """A particle list from momenta [n][3], positions (t, x, y, z) [n][4], species and events."""
    p3, x4 = np.atleast_2d(np.asarray(p3, float)), np.atleast_2d(np.asarray(x4, float))
    n = len(p3)
    p = np.zeros(n, dtype=api.PARTICLE_DTYPE)
    p["px"], p["py"], p["pz"] = p3[:, 0], p3[:, 1], p3[:, 2]
    p["E"] = np.sqrt(mass * mass + (p3 * p3).sum(axis=1))
    p["t"], p["x"], p["y"], p["z"] = x4[:, 0], x4[:, 1], x4[:, 2], x4[:, 3]
    p["tau"] = np.sqrt(np.maximum(x4[:, 0] ** 2 - x4[:, 3] ** 2, 0.0))
    p["species"], p["event"] = species, event
    return p


def accepted(bins, p):
    d = derived(bins)
    E, px, py, pz = (np.asarray(p[k], np.float64) for k in ("E", "px", "py", "pz"))
    den = E - pz
    with np.errstate(all="ignore"):
        ratio = (E + pz) / den
        pT = np.sqrt(px * px + py * py)
    return (den > 0.0) & (ratio >= d["lo"]) & (ratio <= d["hi"]) & (pT >= bins["pT_min"]) & (pT < bins["pT_max"])


def pair_bins(bins, r):
    """All ordered pairs (i, j) of the records r (a structured array of accepted particles of one segment): (bin [n][n] or -1, phase [n][n])."""
    d = derived(bins)
    nq = bins["n_q"]
    g = lambda k: (np.asarray(r[k], np.float64)[:, None], np.asarray(r[k], np.float64)[None, :])  # noqa: E731
    (Ei, Ej), (xi, xj), (yi, yj), (zi, zj) = g("E"), g("px"), g("py"), g("pz")
    with np.errstate(all="ignore"):
        Kx, Ky, K0, Kz = (xi + xj) * 0.5, (yi + yj) * 0.5, (Ei + Ej) * 0.5, (zi + zj) * 0.5
        qx, qy, q0, qz = xi - xj, yi - yj, Ei - Ej, zi - zj
        KT = np.sqrt(Kx * Kx + Ky * Ky)
        ok = (KT > 0.0) & (KT >= bins["kT_min"]) & (KT < bins["kT_max"])
        uo = ((qx * Kx + qy * Ky) / KT + bins["q_max"]) / d["dq"]
        us = ((qx * Ky - qy * Kx) / KT + bins["q_max"]) / d["dq"]
        beta = Kz / K0
        g2 = 1.0 - beta * beta
        ul = ((qz - beta * q0) / np.sqrt(g2) + bins["q_max"]) / d["dq"]
        ok &= (g2 > 0.0)
        for u in (uo, us, ul):
            ok &= (u >= 0.0) & (u < float(nq))
        ikT = np.minimum(((KT - bins["kT_min"]) / d["dkT"]), 1e9)
    ok &= ~np.eye(len(r), dtype=bool)
    safe = lambda u: np.where(ok, u, 0.0).astype(np.int64)  # noqa: E731
    k = ((np.minimum(safe(ikT), bins["n_kT"] - 1) * nq + safe(uo)) * nq + safe(us)) * nq + safe(ul)
    (ti, tj), (ai, aj), (bi, bj), (ci, cj) = g("t"), g("x"), g("y"), g("z")
    phase = (((q0 * (ti - tj) - qx * (ai - aj)) - qy * (bi - bj)) - qz * (ci - cj)) / HBARC
    return np.where(ok, k, -1), phase


def numpy_hist(bins, n_events, n_slots, slot, p):
    """den and M by the restatement, exactly; num from numpy's cos (within one unit per pair of the library's)."""
    block = bins["n_kT"] * bins["n_q"] ** 3
    den = np.zeros((n_slots, block), dtype=np.int64)
    num = np.zeros((n_slots, block), dtype=np.int64)
    M = np.zeros((n_events, n_slots), dtype=np.int64)
    s = np.asarray(slot)[p["species"]]
    keep = accepted(bins, p) & (s >= 0)
    q, s = p[keep], s[keep]
    np.add.at(M, (q["event"], s), 1)
    order = np.lexsort((s, q["event"]))
    q, s = q[order], s[order]
    key = q["event"].astype(np.int64) * n_slots + s
    cuts = np.flatnonzero(np.diff(key)) + 1
    for r, sl in zip(np.split(q, cuts), np.split(s, cuts)):
        if len(r) < 2:
            continue
        k, phase = pair_bins(bins, r)
        hit = k >= 0
        np.add.at(den[sl[0]], k[hit], 1)
        np.add.at(num[sl[0]], k[hit], np.rint(np.cos(phase[hit]) * 4294967296.0).astype(np.int64))
    shape = (n_slots, bins["n_kT"]) + (bins["n_q"],) * 3
    return dict(num=num.reshape(shape), den=den.reshape(shape), M=M)


def cluster(rng, n, centre=(0.35, 0.1, 0.05), spread=0.04, size=3.0):
    """n momenta around `centre` (pairs land inside the q cube) and positions N(0, size) fm in t, x, y, z."""
    return np.asarray(centre) + spread * rng.standard_normal((n, 3)), size * rng.standard_normal((n, 4))


@lru_cache(maxsize=None)
def hand_list():
    """(particles, n_events).  Event e < 7 holds HAND_SIZES[e] accepted particles of species 0 (slot 0), as many of species 6 (slot 1), a few
    of species 2 (slot -1), one outside the rapidity cut and one below pT_min; then HAND_TAIL events of 1-2 particles of species 4 (slot 3);
    then one event of HAND_BIG particles of species 1 (slot 1); the last event holds a pair of identical momenta at two points (q = 0: the
    centre of the q cube for an even n_q, a bin edge for an odd one) and a back-to-back pair (KT = 0: rejected)."""
    rng = np.random.default_rng(20261)
    parts = []
    for e, n in enumerate(HAND_SIZES):
        for sp, m in ((0, n), (6, n), (2, 3)):
            p3, x4 = cluster(rng, m)
            parts.append(make(p3, x4, sp, e))
        parts.append(make([[0.1, 0.1, 5.0], [0.01, 0.01, 0.0]], np.zeros((2, 4)), 0, e))
    e = len(HAND_SIZES)
    for k in range(HAND_TAIL):
        p3, x4 = cluster(rng, 1 + k % 2, spread=0.01)
        parts.append(make(p3, x4, 4, e + k))
    e += HAND_TAIL
    p3, x4 = cluster(rng, HAND_BIG)
    parts.append(make(p3, x4, 1, e))
    e += 1
    same = np.array([[0.3, 0.2, 0.1], [0.3, 0.2, 0.1], [0.4, -0.1, 0.02], [-0.4, 0.1, 0.02]])
    parts.append(make(same, np.array([[0, 0, 0, 0], [1.0, 2.0, -1.0, 0.5], [0, 0, 0, 0], [0.5, 0.5, 0.5, 0.5]]), 0, e))
    p = np.concatenate(parts)
    p.setflags(write=False)
    return p, e + 1


@lru_cache(maxsize=None)
def shuffled_list():
    p, n_events = hand_list()
    q = p[np.random.default_rng(5).permutation(len(p))]
    q.setflags(write=False)
    return q, n_events


def same_counts(a, b):
    return np.array_equal(a["den"], b["den"]) and np.array_equal(a["M"], b["M"])


def num_within_one_unit_per_pair(a, b):
    return bool(np.all(np.abs(a["num"] - b["num"]) <= a["den"]))


# ---- Gaussian sources: physics the restatement cannot vouch for ----
PHYS_EVENTS, PHYS_PER_EVENT = 40, 400
SIGMA_T, SIGMA_Z = 1.5, 2.5
PHYS_T = dict(y_cut=1.0, pT_min=0.0, pT_max=3.0, kT_min=0.0, kT_max=3.0, n_kT=1, q_max=0.1, n_q=11, kernel_form=0)
PHYS_Z = dict(PHYS_T, y_cut=0.05, q_max=0.06, n_q=15)
PHYS_MIN_PAIRS, PHYS_C_MIN = 50, 0.2
PHYS_SEEDS = tuple(range(100, 108))
# the standard deviation of (lambda, R_o^2, R_s^2, R_l^2, R_os^2, R_ol^2, R_sl^2) of the HOST route over PHYS_SEEDS (ddof = 1), measured
PHYS_STD_T = (0.0009, 0.0365, 0.0253, 0.0107, 0.0066, 0.0036, 0.0075)
PHYS_STD_Z = (0.0006, 0.0054, 0.0101, 0.1022, 0.0059, 0.0239, 0.0156)


def _source(seed, centre, spread, sigma_T, sigma_z):
    rng = np.random.default_rng(seed)
    n = PHYS_EVENTS * PHYS_PER_EVENT
    p3 = np.asarray(centre) + rng.standard_normal((n, 3)) * spread
    x4 = np.zeros((n, 4))
    x4[:, 1:3] = sigma_T * rng.standard_normal((n, 2))
    x4[:, 3] = sigma_z * rng.standard_normal(n)
    return make(p3, x4, 0, np.repeat(np.arange(PHYS_EVENTS), PHYS_PER_EVENT))


def transverse_source(seed):
    """PHYS_EVENTS x PHYS_PER_EVENT pi+ with thermal-like momenta (Gaussian components of 0.12 GeV) emitted at t = z = 0 from N(0, SIGMA_T)
    in x and y, independent of the momenta: c = exp(-(q_o^2 + q_s^2) SIGMA_T^2 / hbarc^2)."""
    return _source(seed, (0.0, 0.0, 0.0), 0.12, SIGMA_T, 0.0)


def longitudinal_source(seed):
    """The same number of pi+ around p = (0.8, 0, 0) GeV (components N(0, 0.04): mT is large enough for pairs inside |y| < 0.05 to reach
    q_l = 0.06 GeV) emitted at t = x = y = 0 from N(0, SIGMA_Z) in z: c = exp(-q_z^2 SIGMA_Z^2 / hbarc^2), q_z between q_l and q_l cosh(y)."""
    return _source(seed, (0.8, 0.0, 0.0), 0.04, 0.0, SIGMA_Z)


def fit(bins, hist):
    r = api.hbt_radii(bins, hist, PHYS_MIN_PAIRS, PHYS_C_MIN)
    assert not r["singular"].any()
    return r["lambda"][0, 0], r["R2"][0, 0]


def core_bins_filled(bins, hist, sigma):
    """The fraction of the bins with |q| < hbarc / sigma in all three directions whose den passes PHYS_MIN_PAIRS."""
    nq, dq = bins["n_q"], 2.0 * bins["q_max"] / bins["n_q"]
    c = -bins["q_max"] + (np.arange(nq) + 0.5) * dq
    core = np.abs(c) < HBARC / sigma
    sel = hist["den"][0, 0][np.ix_(core, core, core)]
    return float((sel >= PHYS_MIN_PAIRS).mean())
