"""CPU: the host side of the differential flow records -- is3d_flow_diff_list against is3d_flow_list (the sum rule) and
a numpy restatement of the bin rule, the bin edges bit for bit, and the differential Q-cumulants against explicit sums over distinct pairs
and 4-tuples."""
import numpy as np
import pytest

import flow_cases as F
import flow_diff_cases as D
from is3d_amd import api

# The largest deviation of is3d_flow_diff_cumulants from the brute-force sums over the general-angle cases below, measured on the CPU
# (DESIGN.md section 3u): 5.87e-10, a few times the 2^-33 = 1.2e-10 by which one fixed-point term is off (a correlator of one particle of
# interest against four reference particles carries the errors of p and of Q undiminished); the brute force sums doubles.
GENERAL_MEASURED = 5.9e-10
GENERAL_ALLOWED = 16 * GENERAL_MEASURED
# The standard deviation of v_2{2}(pT) in each of the four bins over 8 seeds (20310..20317) of the constructed sample below (DESIGN.md
# section 3u); the means over those seeds were 0.0998, 0.1022, 0.1005, 0.1009
V2_SIGMA = np.array([8.0e-3, 7.2e-3, 4.1e-3, 4.1e-3])


# ---- 1. the sum rule ----
@pytest.mark.parametrize("edges", (D.EDGES, D.WIDE_EDGES, np.array([0.2, 3.0])), ids=("uniform14", "wide8", "one-bin"))
def test_records_summed_over_bins_are_the_flow_records(edges):
    p, cuts, slot = D.random_list(), D.cuts_for(edges), F.slot_map(3)
    rec = api.flow_diff_list(cuts, edges, 3, 3, slot, p)
    flow = api.flow_list(cuts, 3, 3, slot, p)
    assert rec["m"].shape == (3, 3, len(edges) - 1, 3) and rec["m"][..., 0].sum() > 50
    assert F.same_bits(D.sum_over_bins(rec), flow)
    assert np.array_equal(rec["m"], D.numpy_m(cuts, edges, 3, 3, slot, p))
    if len(edges) > 2:
        assert (rec["m"][..., 0].sum(axis=(0, 1)) > 0).sum() >= 3             # several bins hold particles
    ref = api.flow_diff_reference(rec)
    assert F.same_bits(ref, api.flow_merge(flow, [0, 0, 0], 1))


def test_reference_takes_the_named_slots_and_bins():
    p, slot = D.random_list(), F.slot_map(3)
    rec = api.flow_diff_list(D.CUTS, D.EDGES, 3, 3, slot, p)
    ref = api.flow_diff_reference(rec, ref_slot=[1, 0, 1], ref_bins=(2, 9))
    for k, src in (("M", "m"), ("Q_re", "p_re"), ("Q_im", "p_im")):
        assert np.array_equal(ref[k][:, 0], rec[src][:, [0, 2], 2:9].sum(axis=(1, 2))), k


# ---- 2. bin edges ----
@pytest.mark.parametrize("edges", (D.EDGES, D.WIDE_EDGES), ids=("uniform14", "wide8"))
def test_a_pT_on_an_edge_goes_to_the_lower_inclusive_bin(edges):
    n = len(edges) - 1
    below = np.nextafter(edges, -np.inf)
    pT = np.concatenate([edges, below])                      # every edge, and the next double below it
    axis = np.arange(len(pT)) % 4
    p = D.on_axis(pT, axis, 0.1, 0, 0)
    with np.errstate(all="ignore"):
        assert np.array_equal(np.sqrt(p["px"] * p["px"] + p["py"] * p["py"]), pT)
    rec = api.flow_diff_list(D.cuts_for(edges), edges, 1, 1, [0], p)
    # edge k is the first value of bin k (k < n); the last edge and the double below the first add nothing; the double below edge k > 0
    # is the last value of bin k - 1
    assert np.array_equal(rec["m"][0, 0, :, 0], np.full(n, 2, dtype=np.int64))
    one = api.flow_diff_list(D.cuts_for(edges), edges, 1, 1, [0], p[:len(edges)])
    assert np.array_equal(one["m"][0, 0, :, 0], np.ones(n, dtype=np.int64))


def test_particles_that_add_nothing():
    edges = D.EDGES
    good = D.on_axis([1.0], [0], 0.1, 0, 0)
    last = D.on_axis([edges[-1]], [1], 0.1, 0, 0)
    first_below = D.on_axis([np.nextafter(edges[0], 0.0)], [2], 0.1, 0, 0)
    zero = D.on_axis([0.0], [0], 0.1, 0, 0)
    nan = good.copy()
    nan["px"] = np.nan
    nan_E = good.copy()
    nan_E["E"] = np.nan
    for q in (last, first_below, zero, nan, nan_E):
        rec = api.flow_diff_list(D.CUTS, edges, 1, 1, [0], q)
        assert not any(v.any() for v in rec.values())
    # ... and px = py = 0 adds nothing even to a table that starts at 0: pT = 0 is accepted there, in bin 0
    from_zero = np.array([0.0, 0.5, 1.0])
    rec = api.flow_diff_list(D.cuts_for(from_zero), from_zero, 1, 1, [0], zero)
    assert rec["m"][0, 0, :, 0].tolist() == [1, 0]
    assert api.flow_diff_list(D.CUTS, edges, 1, 1, [0], good)["m"].sum() == 1


def test_one_bin_is_the_flow_record():
    p, slot = D.random_list(), F.slot_map(4)
    edges = np.array([F.CUTS["pT_min"], F.CUTS["pT_max"]])
    rec = api.flow_diff_list(F.CUTS, edges, 3, 4, slot, p)
    flow = api.flow_list(F.CUTS, 3, 4, slot, p)
    assert np.array_equal(rec["m"][:, :, 0], flow["M"]) and np.array_equal(rec["p_re"][:, :, 0], flow["Q_re"])
    assert np.array_equal(rec["p_im"][:, :, 0], flow["Q_im"])


# ---- 3. / 4. the algebra against explicit sums ----
ALG_EDGES = np.array([0.2, 0.5, 1.0, 2.0])
ALG_CUTS = D.cuts_for(ALG_EDGES)
ALG_Y = np.array([-0.8, -0.1, 0.1, 0.8])                  # A, neither, neither, B at y_gap = 0.5
# (ref_slot, ref_bins): slot 0 in bins 0-1 is the reference (bins inside it, bin 2 and slot 1 outside); slot 0's bin 1 is the whole reference
REFERENCES = (([1, 0], (0, 2)), ([1, 0], (1, 2)), ([1, 1], (0, 3)))


def algebra_events(exact, seed=31):
    """6 events of 6-12 particles in 2 slots x 3 bins, at least 4 of each event in slot 0's bins 0 and 1 (the reference holds >= 4 when it is
    bin 1 alone).  -> (particles, angle per particle: integer quarter turns if exact, radians otherwise)."""
    rng = np.random.default_rng(seed)
    sizes = [6, 7, 9, 10, 12, 12]
    ev, pT, sp, ang, y = [], [], [], [], []
    for e, n in enumerate(sizes):
        s = rng.integers(0, 2, n)
        b = rng.integers(0, 3, n)
        s[:4], b[:4] = 0, 1
        s[4], b[4] = 0, 0
        s[5], b[5] = 1, rng.integers(0, 3)
        ev += [e] * n
        sp += s.tolist()
        pT += rng.uniform(ALG_EDGES[b] * 1.01, ALG_EDGES[b + 1] * 0.99).tolist()
        y += ALG_Y[rng.integers(0, 4, n)].tolist()
        ang += (rng.integers(0, 4, n) if exact else rng.uniform(-np.pi, np.pi, n)).tolist()
    if exact:
        return D.on_axis(pT, np.array(ang), y, ev, sp), np.array(ang, dtype=np.int64)
    p = D.particles_at(pT, ang, y, ev, sp)
    return p, np.arctan2(p["py"], p["px"])


def per_event_check(exact, tol):
    p, ang = algebra_events(exact)
    cos = D.quarter_cos if exact else np.cos
    n_events = int(p["event"].max()) + 1
    rec = api.flow_diff_list(ALG_CUTS, ALG_EDGES, n_events, 2, [0, 1], p)
    assert rec["m"][..., 0].sum() == len(p)
    bins, sub = D.numpy_bins(ALG_EDGES, p), F.numpy_regions(ALG_CUTS, p)
    worst = 0.0

    def close(got, want):
        nonlocal worst
        scale = abs(want) if (exact and want != 0.0) else 1.0
        worst = max(worst, abs(got - want) / scale)
        assert abs(got - want) <= tol * scale, (got, want)

    for ref_slot, (lo, hi) in REFERENCES:
        in_ref = (np.asarray(ref_slot)[p["species"]] == 1) & (bins >= lo) & (bins < hi)
        sums = {}                                            # (s, b, kind, n) -> [numerator, weight] over the events
        for e in range(n_events):
            one = {k: v[e:e + 1] for k, v in rec.items()}
            c = api.flow_diff_cumulants(one, ref_slot, (lo, hi))
            here = p["event"] == e
            assert in_ref[here].sum() >= 4
            for s in range(2):
                for b in range(3):
                    poi = here & (p["species"] == s) & (bins == b)
                    for n in range(1, 9):
                        n2, w2, n4, w4 = D.brute_event(ang, poi, here & in_ref, n, cos)
                        ng, wg = D.brute_gap(ang, poi, here & in_ref, sub, n, cos)
                        rows = [("2", n2, w2, c["d2"][s, b, n - 1], c["n_used_2"][s, b]), ("g", ng, wg, c["d2_gap"][s, b, n - 1], c["n_used_gap"][s, b])]
                        if n <= 4:
                            rows.append(("4", n4, w4, c["avg4"][s, b, n - 1], c["n_used_4"][s, b]))
                        for kind, num, w, got, used in rows:
                            assert used == (1 if w > 0 else 0), (kind, s, b, n, w)
                            close(got, num / w if w > 0 else 0.0)
                            acc = sums.setdefault((s, b, kind, n), [0.0, 0.0])
                            acc[0] += num
                            acc[1] += w
        # the event averages are the weighted means
        c = api.flow_diff_cumulants(rec, ref_slot, (lo, hi))
        ref_c = api.flow_cumulants(api.flow_diff_reference(rec, ref_slot, (lo, hi)))
        for (s, b, kind, n), (num, w) in sums.items():
            want = num / w if w > 0 else 0.0
            close(c[dict([("2", "d2"), ("g", "d2_gap"), ("4", "avg4")])[kind]][s, b, n - 1], want)
        for s in range(2):
            for b in range(3):
                for n in range(1, 5):
                    d4 = c["avg4"][s, b, n - 1] - 2.0 * c["d2"][s, b, n - 1] * ref_c["c2"][0, n - 1]
                    assert abs(c["d4"][s, b, n - 1] - (d4 if c["n_used_4"][s, b] else 0.0)) <= 1e-15
    return worst


def test_algebra_is_exact_on_quarter_turn_events():
    per_event_check(True, 1e-12)


def test_algebra_on_random_angles_is_within_the_fixed_point():
    worst = per_event_check(False, GENERAL_ALLOWED)
    print("largest deviation from the brute force: %.3e (measured %.1e, allowed %.1e)" % (worst, GENERAL_MEASURED, GENERAL_ALLOWED))


# ---- 5. zero weights, wrong-sign references, a constructed sample ----
def test_zero_weight_events_are_left_out():
    # event 0: the particle of interest IS the whole reference (m_p M - m_q = 0); event 1: three reference particles (M < 4);
    # event 2: six reference particles
    ev = [0] + [1] * 3 + [2] * 6
    p = D.on_axis(0.3, np.arange(len(ev)) % 4, [-0.8, 0.8] * 5, ev, 0)
    rec = api.flow_diff_list(ALG_CUTS, ALG_EDGES, 3, 1, [0], p)
    assert rec["m"][:, 0, 0, 0].tolist() == [1, 3, 6]
    c = api.flow_diff_cumulants(rec)
    assert c["n_used_2"][0, 0] == 2 and c["n_used_4"][0, 0] == 1 and c["n_used_gap"][0, 0] == 2 and c["n_events"][0, 0] == 3
    assert c["n_used_2"][0, 1] == c["n_used_4"][0, 1] == c["n_used_gap"][0, 1] == 0 and not c["d2"][0, 1].any() and c["sum_m"][0, 1] == 0
    assert c["sum_m"][0, 0] == 10 and c["mean_m"][0, 0] == 10 / 3
    # a particle of interest outside a reference of three: <2'> has a weight, the four-particle quantity is left out (M < 4)
    q = D.on_axis([0.3, 0.3, 0.3, 0.7], [0, 1, 2, 3], 0.1, 0, 0)
    c = api.flow_diff_cumulants(api.flow_diff_list(ALG_CUTS, ALG_EDGES, 1, 1, [0], q), ref_bins=(0, 1))
    assert c["n_used_2"][0, 1] == 1 and c["n_used_4"][0, 1] == 0 and c["n_used_4"][0, 0] == 0 and c["n_used_gap"][0, 1] == 0


def test_wrong_sign_reference_cumulants_give_zero_not_nan():
    # all particles of an event at the same angle: <2> = <4> = 1, c4 = 1 - 2 = -1 < 0, fine; opposite pairs: <2>_2 = -1/(M-1) < 0 for n = 1
    ev = np.repeat(np.arange(4), 6)
    p = D.on_axis(0.3, np.tile([0, 2], 12), np.tile([-0.8, 0.8], 12), ev, 0)
    rec = api.flow_diff_list(ALG_CUTS, ALG_EDGES, 4, 1, [0], p)
    c = api.flow_diff_cumulants(rec)
    r = api.flow_cumulants(api.flow_diff_reference(rec))
    assert r["c2"][0, 0] < 0 and r["c2_gap"][0, 0] < 0 and r["c4"][0, 1] < 0 < r["c2"][0, 1]
    assert c["v2"][0, 0, 0] == 0.0 and c["v2_gap"][0, 0, 0] == 0.0 and c["d2"][0, 0, 0] < 0
    assert c["v2"][0, 0, 1] == pytest.approx(1.0, abs=1e-12) and c["v4"][0, 0, 1] == pytest.approx(1.0, abs=1e-12)
    # c4 >= 0: two back-to-back pairs at right angles have <4>_2 = 1 and <2>_2 = -1/3 ... the sign is what is asserted
    assert all(np.isfinite(v).all() for v in c.values())
    for n in range(4):
        if r["c4"][0, n] >= 0:
            assert c["v4"][0, 0, n] == 0.0
    assert (r["c4"][0] >= 0).any()


def v2_sample(seed, n_events=2000, mult=60, v2=0.1):
    rng = np.random.default_rng(seed)
    n = n_events * mult
    phi = np.empty(0)
    while len(phi) < n:                                      # phi from 1 + 2 v2 cos(2 phi), by rejection
        x = rng.uniform(-np.pi, np.pi, n)
        phi = np.concatenate([phi, x[rng.uniform(0, 1 + 2 * v2, n) < 1 + 2 * v2 * np.cos(2 * x)]])
    edges = np.array([0.2, 0.6, 1.0, 1.6, 3.0])
    p = D.particles_at(rng.uniform(0.2, 3.0, n), phi[:n], rng.uniform(-0.9, 0.9, n), np.repeat(np.arange(n_events), mult), 0)
    rec = api.flow_diff_list(D.cuts_for(edges), edges, n_events, 1, [0], p)
    return api.flow_diff_cumulants(rec)


def test_a_constructed_v2_is_recovered_within_its_statistical_error():
    c = v2_sample(20301)
    v2 = c["v2"][0, :, 1]
    print("v_2{2}(pT) of the constructed sample:", v2, " v_2{2,gap}:", c["v2_gap"][0, :, 1], " v_2{4}:", c["v4"][0, :, 1])
    assert np.all(np.abs(v2 - 0.1) < 5 * V2_SIGMA), v2
    assert np.all(c["n_used_2"] >= 1990) and np.all(c["n_used_4"] >= 1990)      # an event with an empty bin is left out of that bin


def measure():
    """prints the two measured figures of this module"""
    print("general angles: largest deviation %.3e" % per_event_check(False, 1.0))
    v = np.array([v2_sample(s)["v2"][0, :, 1] for s in range(20310, 20318)])
    print("v2 over 8 seeds: mean", v.mean(axis=0), "std", v.std(axis=0, ddof=1))


if __name__ == "__main__":
    measure()
