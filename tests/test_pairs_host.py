"""CPU: the host side of the two-particle (delta y, delta phi) correlations -- is3d_pairs_list (the definition, an explicit double loop) and
is3d_pairs_correlation -- against the cell rule restated in Python on particles placed at its edges, closed forms, sum rules, an independent
count from per-event occupancy grids, and the one property no one-particle histogram and no sub-event cumulant can vouch for: that hadrons
of one event which are close in rapidity and azimuth are no more frequent than such hadrons of neighbouring events."""
import math

import numpy as np
import pytest

import flow_cases as F
import pairs_cases as P
from is3d_amd import api

OPEN = dict(y_cut=4.0, pT_min=0.0, pT_max=100.0, n_y=8, n_phi=12)      # every particle below is inside


def library_cells(bins, p):
    """The cell of every particle through the library: particle i of the list and a partner known to sit in cell (0, 0) form event i; the one
    pair of class (0, 1) of that event lands at (iy, iphi).  All events in one call would sum the histograms, so the list goes in chunks
    whose pairs cannot collide: one call per particle is the plain way and the lists here are short."""
    edge, _, _ = P.tables(bins)
    y0 = 0.25 * math.log(edge[0] * edge[1])
    partner = P.at(y0, 1e-3, pT=0.5 * (bins["pT_min"] + min(bins["pT_max"], 10.0)), species=0)
    assert P.cell_of(bins, P.tables(bins), *(float(partner[k][0]) for k in ("E", "px", "py", "pz"))) == (0, 0)
    out = []
    for i in range(len(p)):
        q = p[i:i + 1].copy()
        q["event"], q["species"] = 0, 1
        h = api.pairs_list(bins, 1, 2, [0, 1], np.concatenate([partner, q]))
        if h["M"][0, 1] == 0:
            out.append(None)
            continue
        dy, dphi = np.argwhere(h["same"][api.pair_class(0, 1, 2)])[0]
        out.append((int(dy) - (bins["n_y"] - 1), int(dphi)))
    return out


def restated_cells(bins, p):
    t = P.tables(bins)
    return [P.cell_of(bins, t, float(p["E"][i]), float(p["px"][i]), float(p["py"][i]), float(p["pz"][i])) for i in range(len(p))]


def precise_cells(bins, p, margin=1e-12):
    """(cells, far): the cell from long-double rapidity and azimuth, and whether both are further than `margin` from every edge."""
    L = np.longdouble
    E, px, py, pz = (p[k].astype(L) for k in ("E", "px", "py", "pz"))
    y = L(0.5) * np.log((E + pz) / (E - pz))
    phi = np.arctan2(py, px)
    two_pi = L(2) * np.arctan2(L(0), L(-1))
    phi = np.where(phi < 0, phi + two_pi, phi)
    wy, wp = L(2) * L(bins["y_cut"]) / bins["n_y"], two_pi / bins["n_phi"]
    fy, fp = (y + L(bins["y_cut"])) / wy, phi / wp
    iy, ip = np.floor(fy).astype(np.int64), np.floor(fp).astype(np.int64) % bins["n_phi"]
    far = (np.abs(fy - np.rint(fy)) * wy > margin) & (np.abs(fp - np.rint(fp)) * wp > margin)
    inside = (iy >= 0) & (iy < bins["n_y"])
    return [((int(a), int(b)) if ok else None) for a, b, ok in zip(iy, ip, inside)], far


@pytest.mark.parametrize("n_y", (1, 2, 33, 64))
def test_rapidity_index_at_every_edge(n_y):
    """Particles 1e-9 below and above every rapidity edge: the library, the Python restatement and long-double rapidity agree."""
    bins = dict(P.BINS, n_y=n_y, n_phi=4)
    edges = -bins["y_cut"] + np.arange(n_y + 1) * (2.0 * bins["y_cut"] / n_y)
    y = np.array([e + s * 1e-9 for e in edges for s in (-1.0, 1.0)])
    p = P.at(y, 0.3)
    want = [None] + [(k, 0) for k in range(n_y) for _ in (0, 1)] + [None]
    assert restated_cells(bins, p) == want
    assert library_cells(bins, p) == want
    precise, far = precise_cells(bins, p)
    assert far.all() and precise == want


@pytest.mark.parametrize("n_phi", (4, 12, 64))
def test_azimuth_index_at_every_direction(n_phi):
    """Particles exactly on every bin direction (the four axes among them), and one ulp of py (or of px where |dy| > |dx|) on either side."""
    bins = dict(P.BINS, n_y=1, n_phi=n_phi)
    _, dx, dy = P.tables(bins)
    q = n_phi // 4
    assert [(dx[k], dy[k]) for k in (0, q, 2 * q, 3 * q)] == [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
    rows = []
    for k in range(n_phi):
        rows.append((dx[k], dy[k]))
        if abs(dx[k]) >= abs(dy[k]):
            rows += [(dx[k], np.nextafter(dy[k], -np.inf)), (dx[k], np.nextafter(dy[k], np.inf))]
        else:
            rows += [(np.nextafter(dx[k], -np.inf), dy[k]), (np.nextafter(dx[k], np.inf), dy[k])]
    p = P.at(np.zeros(len(rows)), 0.0)
    p["px"], p["py"] = np.array(rows).T
    want = restated_cells(bins, p)
    assert all(c is not None for c in want)
    assert library_cells(bins, p) == want
    on = want[0::3]
    assert on == [(0, k) for k in range(n_phi)]                 # a particle on a direction belongs to the bin that starts there
    for k in (0, q, 2 * q, 3 * q):                              # exactly on an axis; the denormal step off it is decided by the signs alone
        below, above = want[3 * k + 1], want[3 * k + 2]
        assert {below, above} == {(0, (k - 1) % n_phi), (0, k)}
    precise, far = precise_cells(bins, p)
    assert all(a == b for a, b, f in zip(want, precise, far) if f)
    # away from the directions the long-double angle decides alone
    rng = np.random.default_rng(5)
    r = P.at(np.zeros(4000), rng.uniform(-np.pi, np.pi, 4000))
    precise, far = precise_cells(bins, r)
    got = restated_cells(bins, r)
    assert far.sum() > 3900 and all(a == b for a, b, f in zip(got, precise, far) if f)
    iy, iphi = P.numpy_cells(bins, r)
    assert [(int(a), int(b)) for a, b in zip(iy, iphi)] == got


def test_what_the_rule_rejects():
    bins = dict(P.BINS, n_y=2, n_phi=12)
    p = P.at(np.zeros(6), 0.0)
    p["px"][0], p["py"][0] = 0.0, 0.0                            # pT = 0
    p["px"][1] = bins["pT_min"]                                  # pT = pT_min is in (sqrt(fl(x * x)) = x)
    p["px"][2] = bins["pT_max"]                                  # pT = pT_max is out
    p["pz"][3] = p["E"][3]                                       # E - pz = 0
    p["pz"][4] = 2.0 * p["E"][4]                                 # E - pz < 0
    p["E"][5] = np.nan
    want = [None, (1, 0), None, None, None, None]
    assert restated_cells(bins, p) == want and library_cells(bins, p) == want
    zero = dict(bins, pT_min=0.0)                                # pT_min = 0 still rejects pT = 0
    assert library_cells(zero, p[:1]) == [None] and restated_cells(zero, p[:1]) == [None]


def test_the_restatement_and_the_library_agree_on_a_list():
    p, n_events = P.hand_list()
    for shape in P.SHAPES:
        bins = P.bins_of(shape)
        occ = P.occupancies(bins, n_events, 1, np.zeros(P.N_SPECIES, np.int32), p)
        M = api.pairs_list(bins, n_events, 1, np.zeros(P.N_SPECIES, np.int32), p)["M"]
        assert np.array_equal(M[:, 0], occ.sum(axis=(1, 2, 3))) and 0 < M.sum() < len(p)


# ---- closed forms ----
def hist_of(p, n_events=1, bins=OPEN, n_slots=1, slot=(0,)):
    return api.pairs_list(bins, n_events, n_slots, list(slot), p)


def test_one_particle_gives_nothing():
    h = hist_of(P.at(0.3, 1.0))
    assert h["M"].tolist() == [[1]] and not h["same"].any() and not h["mixed"].any()


def test_two_particles_in_one_cell():
    h = hist_of(P.at([0.3, 0.31], [1.0, 1.01]))
    assert h["same"][0, OPEN["n_y"] - 1, 0] == 2 == h["same"].sum() and not h["mixed"].any()


def test_a_back_to_back_pair():
    h = hist_of(P.at([0.3, 0.3], [0.7, 0.7 + np.pi]))
    assert h["same"][0, OPEN["n_y"] - 1, OPEN["n_phi"] // 2] == 2 == h["same"].sum()
    h = hist_of(P.at([0.3, -1.3], [0.7, 0.7 + np.pi]))           # 1.6 apart: two rapidity bins of width 1, once each way
    assert h["same"][0, OPEN["n_y"] - 1 + 2, 6] == 1 == h["same"][0, OPEN["n_y"] - 1 - 2, 6] and h["same"].sum() == 2


def test_a_regular_pentagon():
    """Five particles 72 degrees apart with n_phi = 20: each of the 20 ordered pairs is k x 4 bins away, k = 1..4, five pairs each."""
    bins = dict(OPEN, n_phi=20)
    h = hist_of(P.at(np.zeros(5), 0.1 + 2.0 * np.pi * np.arange(5) / 5.0), bins=bins)
    want = np.zeros(20, dtype=np.int64)
    want[[4, 8, 12, 16]] = 5
    assert h["same"][0, bins["n_y"] - 1].tolist() == want.tolist() and h["same"].sum() == 20


def test_two_slots_count_only_trigger_0_associate_1():
    p = P.at([0.3, 1.4, 1.4], [0.2, 0.2 + np.pi / 2, 0.2 + np.pi / 2], species=[0, 1, 1])
    h = hist_of(p, n_slots=2, slot=(0, 1))
    c01, n_y = api.pair_class(0, 1, 2), OPEN["n_y"]
    assert (api.pair_class(0, 0, 2), c01, api.pair_class(1, 1, 2)) == (0, 1, 2)
    assert h["same"][c01, n_y - 1 + 1, 3] == 2 == h["same"][c01].sum()       # from the slot-0 particle to each slot-1 particle, never back
    assert h["same"][2, n_y - 1, 0] == 2 == h["same"][2].sum() and not h["same"][0].any()
    assert h["M"].tolist() == [[1, 2]]


def test_one_event_has_no_mixed_pairs_and_two_mix_both_ways():
    a, b = P.at([0.3, 0.3], [0.1, 0.1]), P.at([1.4], [0.1 + np.pi], event=1)
    assert not hist_of(a)["mixed"].any()
    h = hist_of(np.concatenate([a, b]), n_events=2)
    n_y = OPEN["n_y"]
    assert h["mixed"][0, n_y - 1 + 1, 6] == 2 and h["mixed"][0, n_y - 1 - 1, 6] == 2 and h["mixed"].sum() == 4
    assert h["same"][0, n_y - 1, 0] == 2 == h["same"].sum()
    three = hist_of(np.concatenate([a, b, P.at([0.3], [0.1], event=2)]), n_events=3)     # 0 -> 1, 1 -> 2, 2 -> 0: each partnership once
    assert three["mixed"].sum() == 2 * 1 + 1 * 1 + 1 * 2 and three["mixed"][0, n_y - 1, 0] == 2


# ---- sums and the independent count ----
@pytest.mark.parametrize("n_slots", (1, 3, 10))
def test_sum_rules_and_the_independent_count(n_slots):
    p, n_events = P.hand_list()
    slot = P.slot_map(n_slots)
    for shape in P.SHAPES:
        bins = P.bins_of(shape)
        h = api.pairs_list(bins, n_events, n_slots, slot, p)
        M = h["M"]
        for a in range(n_slots):
            for b in range(a, n_slots):
                c = api.pair_class(a, b, n_slots)
                assert h["same"][c].sum() == (M[:, a] * M[:, b]).sum() - (M[:, a].sum() if a == b else 0)
                assert h["mixed"][c].sum() == (M[:, a] * np.roll(M[:, b], -1)).sum()
        assert P.same_hist(h, P.numpy_hist(bins, n_events, n_slots, slot, p)), (n_slots, shape)
    q, _ = P.shuffled_list()
    assert P.same_hist(api.pairs_list(bins, n_events, n_slots, slot, q), h)


@pytest.mark.parametrize("n_events", (1, 2, 3))
def test_few_events(n_events):
    p, _ = P.few_events(n_events)
    bins, slot = P.bins_of((33, 20)), P.slot_map(3)
    assert P.same_hist(api.pairs_list(bins, n_events, 3, slot, p), P.numpy_hist(bins, n_events, 3, slot, p))


# ---- the correlation function ----
@pytest.mark.parametrize("gap_bins", (0, 1, 5))
def test_pairs_correlation_is_its_restatement(gap_bins):
    """A handful of double operations on exact integers on either side: 1e-12 relative."""
    p, n_events = P.hand_list()
    bins = P.bins_of((6, 8))
    h = api.pairs_list(bins, n_events, 3, P.slot_map(3), p)
    got, want = api.pairs_correlation(bins, h, gap_bins), P.numpy_correlation(bins, h, gap_bins)
    assert np.array_equal(got["n_same"], want["n_same"]) and np.array_equal(got["n_mixed"], want["n_mixed"]) and got["n_mixed"].min() > 0
    for k in ("C", "C_phi"):
        assert np.all(np.abs(got[k] - want[k]) <= 1e-12 * np.abs(want[k])), k
    # V_n is a mean of cosines with the weights C_phi / sum C_phi: a sum whose terms cancel (some V_n vanish by symmetry), so the bound is
    # relative to the sum of the terms' magnitudes, sum |w cos|, not to the result
    w = want["C_phi"] / want["C_phi"].sum(axis=1, keepdims=True)
    for n in (1, 2, 3, 4):
        scale = (w * np.abs(np.cos(2.0 * np.pi * n * np.arange(bins["n_phi"]) / bins["n_phi"]))).sum(axis=1)
        assert np.all(np.abs(got["V"][:, n - 1] - want["V"][:, n - 1]) <= 1e-12 * scale), n
    assert (got["C"] > 0).any() and (got["C_phi"] > 0).all() and np.abs(got["V"]).max() < 1.0
    empty = {k: np.zeros_like(v) for k, v in h.items()}
    zero = api.pairs_correlation(bins, empty)
    assert not zero["C"].any() and not zero["C_phi"].any() and not zero["V"].any() and not zero["n_same"].any()


# ---- the independence condition ----
def thermal_list(fx):
    from oracle import oracle
    cells, sp, gla, o, kw = F.thermal_surface()
    d, _ = oracle.sample_particles(cells, sp, fx["df"], gla, o, **kw)
    p = np.zeros(len(d["E"]), dtype=api.PARTICLE_DTYPE)
    for k in p.dtype.names:
        p[k] = d[k]
    return p, kw["n_events"]


def test_close_hadrons_of_one_event_are_no_more_frequent_than_of_two(fx):
    """pi+ from the CPU restatement of the sampler (tests/flow_cases.py: thermal_surface, 60 events, seed 20270) in the driver's default bins.
    E = [same over the 3 x 3 bins around (0, 0)] / n_same - [the same for mixed] / n_mixed must vanish within 5 sigma of the delete-one-event
    jackknife.  Observed on this list: E = -7.55e-4, sigma = 3.28e-4, a pull of -2.31.  The case it must catch: the same list with every hadron of an
    event listed twice -- a sampler whose neighbouring hadrons share random numbers -- which passes every one-particle test (observed: E =
    6.41e-3, sigma = 3.57e-4, 18 sigma)."""
    p, n_events = thermal_list(fx)
    E, sigma = P.short_range_excess(P.BINS, n_events, p)
    print("short-range excess: E = %.3e, sigma = %.3e, pull %.2f" % (E, sigma, E / sigma))
    assert abs(E) <= 5.0 * sigma, (E, sigma)
    # the statistic is that of the library's histograms
    h = api.pairs_list(P.BINS, n_events, 1, [0], p)
    n_y, n_phi = P.BINS["n_y"], P.BINS["n_phi"]
    near = lambda a: a[0, n_y - 2:n_y + 1][:, (n_phi - 1, 0, 1)].sum()  # noqa: E731
    assert abs(near(h["same"]) / h["same"].sum() - near(h["mixed"]) / h["mixed"].sum() - E) < 1e-15
    twice = np.concatenate([p, p])
    E2, sigma2 = P.short_range_excess(P.BINS, n_events, twice)
    print("every hadron twice: E = %.3e, sigma = %.3e, pull %.2f" % (E2, sigma2, E2 / sigma2))
    assert E2 > 5.0 * sigma2, (E2, sigma2)
