"""Shared cases of the pair-correlation tests (tests/test_pairs_host.py, tests/test_pairs_abi.py, tests/test_gpu_pairs.py): particle lists
made by hand, the per-particle cell rule of csrc/cf_sampler_pairs.h restated in Python (scalar) and numpy (lists), an independent count of the
pair histograms from per-event occupancy grids, and the short-range excess of the independence condition."""
import math
from functools import lru_cache

import numpy as np

from is3d_amd import api

BINS = dict(api.PAIR_BINS)                 # y_cut 2.0, pT in [0.2, 3.0), 32 x 32
SHAPES = ((1, 4), (2, 12), (33, 20), (64, 64))   # (n_y, n_phi): the smallest grid, odd sizes, 127 x 64 bins (more than one bin per thread, full LDS)
N_SPECIES = 23
HAND_SIZES = (0, 1, 2, 63, 64, 65, 257)    # an empty event, the single, the pair, around one wave, one event across workgroups
HAND_TAIL = 200                            # ... and a tail of one-particle events


def bins_of(shape, **over):
    return dict(BINS, n_y=shape[0], n_phi=shape[1], **over)


def tables(bins):
    """(edge[n_y + 1], dx[n_phi], dy[n_phi]): the rule's tables through Python's exp, cos and sin, the axis directions exact."""
    n_y, n_phi, y_cut = bins["n_y"], bins["n_phi"], bins["y_cut"]
    w = 2.0 * y_cut / float(n_y)
    edge = [math.exp(2.0 * (-y_cut + float(k) * w)) for k in range(n_y + 1)]
    dx = [math.cos(2.0 * math.pi * float(k) / float(n_phi)) for k in range(n_phi)]
    dy = [math.sin(2.0 * math.pi * float(k) / float(n_phi)) for k in range(n_phi)]
    q = n_phi // 4
    for k, (x, y) in zip((0, q, 2 * q, 3 * q), ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))):
        dx[k], dy[k] = x, y
    return np.array(edge), np.array(dx), np.array(dy)


def cell_of(bins, t, E, px, py, pz):
    """The rule for one momentum in Python floats (IEEE doubles, no contraction): (iy, iphi) or None."""
    edge, dx, dy = t
    n_y, n_phi = bins["n_y"], bins["n_phi"]
    num, den = E + pz, E - pz
    if not den > 0.0:
        return None
    ratio = num / den
    if not (ratio >= edge[0] and ratio < edge[n_y]):
        return None
    pT = math.sqrt(px * px + py * py)
    if not (pT >= bins["pT_min"] and pT < bins["pT_max"] and pT > 0.0):
        return None
    lo, hi = 0, n_y
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if edge[mid] <= ratio:
            lo = mid
        else:
            hi = mid
    iy = lo
    q = n_phi >> 2
    quad = 0 if (px > 0.0 and py >= 0.0) else 1 if (px <= 0.0 and py > 0.0) else 2 if (px < 0.0 and py <= 0.0) else 3
    lo, hi = quad * q, quad * q + q
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if float(dx[mid]) * py - float(dy[mid]) * px >= 0.0:
            lo = mid
        else:
            hi = mid
    return iy, lo


def numpy_cells(bins, p):
    """(iy, iphi) per particle of a list, iy = -1 where the rule accepts nothing: the same bisections on arrays."""
    edge, dx, dy = tables(bins)
    n_y, n_phi = bins["n_y"], bins["n_phi"]
    E, px, py, pz = (np.asarray(p[k], dtype=np.float64) for k in ("E", "px", "py", "pz"))
    den = E - pz
    with np.errstate(all="ignore"):
        ratio = (E + pz) / den
        pT = np.sqrt(px * px + py * py)
    ok = (den > 0.0) & (ratio >= edge[0]) & (ratio < edge[n_y]) & (pT >= bins["pT_min"]) & (pT < bins["pT_max"]) & (pT > 0.0)
    lo, hi = np.zeros(len(E), np.int64), np.full(len(E), n_y, np.int64)
    while np.any(hi - lo > 1):
        act = hi - lo > 1
        mid = (lo + hi) >> 1
        up = act & (edge[np.minimum(mid, n_y)] <= ratio)
        lo = np.where(up, mid, lo)
        hi = np.where(act & ~up, mid, hi)
    iy = lo
    q = n_phi >> 2
    quad = np.where((px > 0.0) & (py >= 0.0), 0, np.where((px <= 0.0) & (py > 0.0), 1, np.where((px < 0.0) & (py <= 0.0), 2, 3)))
    lo, hi = quad * q, quad * q + q
    while np.any(hi - lo > 1):
        act = hi - lo > 1
        mid = (lo + hi) >> 1
        up = act & (dx[mid % n_phi] * py - dy[mid % n_phi] * px >= 0.0)
        lo = np.where(up, mid, lo)
        hi = np.where(act & ~up, mid, hi)
    return np.where(ok, iy, -1), np.where(ok, lo, -1)


def occupancies(bins, n_events, n_slots, slot, p):
    """occ [event][slot][iy][iphi] by the numpy restatement of the rule."""
    occ = np.zeros((n_events, n_slots, bins["n_y"], bins["n_phi"]), dtype=np.int64)
    iy, iphi = numpy_cells(bins, p)
    s = np.asarray(slot)[p["species"]]
    keep = (iy >= 0) & (s >= 0)
    np.add.at(occ, (p["event"][keep], s[keep], iy[keep], iphi[keep]), 1)
    return occ


def correlate(bins, A, B):
    """[2 n_y - 1][n_phi]: sum over occupied cells a of A and b of B of A[a] B[b] at (iy_b - iy_a + n_y - 1, (iphi_b - iphi_a) mod n_phi)."""
    n_y, n_phi = bins["n_y"], bins["n_phi"]
    out = np.zeros((2 * n_y - 1, n_phi), dtype=np.int64)
    ya, pa = np.nonzero(A)
    yb, pb = np.nonzero(B)
    if len(ya) and len(yb):
        w = A[ya, pa][:, None] * B[yb, pb][None, :]
        np.add.at(out, ((yb[None, :] - ya[:, None] + n_y - 1).ravel(), ((pb[None, :] - pa[:, None]) % n_phi).ravel()), w.ravel())
    return out


def numpy_hist(bins, n_events, n_slots, slot, p):
    """The pair histograms counted a second way, without a loop over particle pairs: per-event occupancy grids, correlated cell by cell."""
    occ = occupancies(bins, n_events, n_slots, slot, p)
    n_classes = api.pair_classes(n_slots)
    same = np.zeros((n_classes, 2 * bins["n_y"] - 1, bins["n_phi"]), dtype=np.int64)
    mixed = np.zeros_like(same)
    M = occ.sum(axis=(2, 3))
    for e in range(n_events):
        for a in range(n_slots):
            if not M[e, a]:
                continue
            for b in range(a, n_slots):
                c = api.pair_class(a, b, n_slots)
                same[c] += correlate(bins, occ[e, a], occ[e, b])
                if a == b:
                    same[c, bins["n_y"] - 1, 0] -= M[e, a]
                if n_events >= 2:
                    mixed[c] += correlate(bins, occ[e, a], occ[(e + 1) % n_events, b])
    return dict(same=same, mixed=mixed, M=M)


def same_hist(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("same", "mixed", "M"))


def at(y, phi, pT=1.0, event=0, species=0, mass=0.13957):
    """Particles at rapidity y and azimuth phi."""
    y, phi, pT = np.broadcast_arrays(np.atleast_1d(np.asarray(y, np.float64)), np.asarray(phi, np.float64), np.asarray(pT, np.float64))
    p = np.zeros(len(y), dtype=api.PARTICLE_DTYPE)
    mT = np.sqrt(mass * mass + pT * pT)
    p["E"], p["pz"], p["px"], p["py"] = mT * np.cosh(y), mT * np.sinh(y), pT * np.cos(phi), pT * np.sin(phi)
    p["event"], p["species"] = event, species
    return p


def kinematic_list(rng, events, n_species=N_SPECIES, mass=0.13957):
    """One particle per entry of `events`: rapidity in [-2.4, 2.4], pT in [0.05, 3.5], any azimuth -- on both sides of every cut of BINS."""
    n = len(events)
    p = at(rng.uniform(-2.4, 2.4, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(0.05, 3.5, n), mass=mass)
    p["event"] = events
    p["species"] = rng.integers(0, n_species, n)
    p["cell"] = np.arange(n)
    return p


@lru_cache(maxsize=None)
def hand_list():
    """(particles ordered by event, n_events): 652 particles, the event sizes of HAND_SIZES, then HAND_TAIL events of one."""
    sizes = list(HAND_SIZES) + [1] * HAND_TAIL
    p = kinematic_list(np.random.default_rng(20280), np.repeat(np.arange(len(sizes)), sizes))
    p.setflags(write=False)
    return p, len(sizes)


@lru_cache(maxsize=None)
def shuffled_list():
    p, n_events = hand_list()
    q = p[np.random.default_rng(8).permutation(len(p))]
    q.setflags(write=False)
    return q, n_events


@lru_cache(maxsize=None)
def few_events(n_events):
    """(particles, n_events) for 1, 2 or 3 events of 40, 25, 31 particles: the cyclic partner of the mixed pairs."""
    sizes = (40, 25, 31)[:n_events]
    p = kinematic_list(np.random.default_rng(20281 + n_events), np.repeat(np.arange(n_events), sizes))
    p.setflags(write=False)
    return p, n_events


def slot_map(n_slots, n_species=N_SPECIES):
    """species -> slot with slot -1 present: the species are shared out round robin over n_slots + 1 values, the first of which is -1."""
    return (np.arange(n_species) % (n_slots + 1) - 1).astype(np.int32)


def edge_distance(bins, p):
    """The smallest distance of a particle from a cell decision, in rapidity from the edges, in azimuth from the bin directions, in pT from
    its two cuts.  Lists whose momenta the device computes itself (decays) agree with the host's to 1.5e-12: with every particle further than
    1e-9 from a decision, host and device reach the same cells."""
    if len(p) == 0:
        return np.inf
    with np.errstate(all="ignore"):
        y = 0.5 * np.log((p["E"] + p["pz"]) / (p["E"] - p["pz"]))
    pT = np.sqrt(p["px"] ** 2 + p["py"] ** 2)
    phi = np.arctan2(p["py"], p["px"]) % (2.0 * np.pi)
    ye = -bins["y_cut"] + np.arange(bins["n_y"] + 1) * (2.0 * bins["y_cut"] / bins["n_y"])
    pe = np.arange(bins["n_phi"] + 1) * (2.0 * np.pi / bins["n_phi"])
    d = [np.nanmin(np.abs(y[:, None] - ye[None, :])), np.abs(phi[:, None] - pe[None, :]).min(), np.abs(pT - bins["pT_min"]).min(),
         np.abs(pT - bins["pT_max"]).min()]
    return float(min(d))


def short_range_excess(bins, n_events, p):
    """(E, sigma): E = [same over the 3 x 3 bins around (delta y, delta phi) = (0, 0)] / n_same - [the same for mixed] / n_mixed of one slot
    holding every particle, and sigma from the delete-one-event jackknife: without event e its same-event pairs and its two mixed
    partnerships go, and its neighbours e - 1 and e + 1 become partners."""
    occ = occupancies(bins, n_events, 1, np.zeros(int(p["species"].max()) + 1, np.int32), p)[:, 0]
    n_y, n_phi = bins["n_y"], bins["n_phi"]
    M = occ.sum(axis=(1, 2))

    def near(A, B):
        h = correlate(bins, A, B)
        return int(h[n_y - 2:n_y + 1][:, (n_phi - 1, 0, 1)].sum()) if n_y >= 2 else int(h[:, (n_phi - 1, 0, 1)].sum())

    s3 = np.array([near(occ[e], occ[e]) - M[e] for e in range(n_events)], dtype=np.float64)
    S = (M * (M - 1)).astype(np.float64)
    nxt = (np.arange(n_events) + 1) % n_events
    m3 = np.array([near(occ[e], occ[nxt[e]]) for e in range(n_events)], dtype=np.float64)
    X = (M * M[nxt]).astype(np.float64)
    whole = s3.sum() / S.sum() - m3.sum() / X.sum()
    jack = np.zeros(n_events)
    for e in range(n_events):
        prev, after = (e - 1) % n_events, nxt[e]
        keep = np.arange(n_events) != e
        mk = keep & (np.arange(n_events) != prev)
        jack[e] = s3[keep].sum() / S[keep].sum() - (m3[mk].sum() + near(occ[prev], occ[after])) / (X[mk].sum() + M[prev] * M[after])
    sigma = math.sqrt((n_events - 1.0) / n_events * ((jack - jack.mean()) ** 2).sum())
    return float(whole), float(sigma)


def numpy_correlation(bins, hist, gap_bins=0):
    """is3d_pairs_correlation restated."""
    n_y, n_phi = bins["n_y"], bins["n_phi"]
    same, mixed = hist["same"].astype(np.float64), hist["mixed"].astype(np.float64)
    ns, nm = hist["same"].sum(axis=(1, 2)), hist["mixed"].sum(axis=(1, 2))
    C = np.zeros_like(same)
    C_phi = np.zeros((len(same), n_phi))
    V = np.zeros((len(same), 4))
    rows = np.abs(np.arange(2 * n_y - 1) - (n_y - 1)) >= gap_bins
    for c in range(len(same)):
        if ns[c] > 0:
            ok = mixed[c] > 0
            C[c][ok] = (same[c][ok] / float(ns[c])) / (mixed[c][ok] / float(nm[c]))
            s, m = hist["same"][c][rows].sum(axis=0), hist["mixed"][c][rows].sum(axis=0)
            ok = m > 0
            C_phi[c][ok] = (s[ok] / float(ns[c])) / (m[ok] / float(nm[c]))
        tot = C_phi[c].sum()
        if tot != 0.0:
            V[c] = [(C_phi[c] * np.cos(2.0 * np.pi * n * np.arange(n_phi) / n_phi)).sum() / tot for n in (1, 2, 3, 4)]
    return dict(C=C, C_phi=C_phi, V=V, n_same=ns, n_mixed=nm)
