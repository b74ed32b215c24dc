"""CPU: the host side of the per-event flow records -- is3d_flow_list (the definition), is3d_flow_merge and is3d_flow_cumulants -- against
closed forms, explicit sums over distinct pairs and quadruplets, the region rule restated in numpy on particles placed at its thresholds, and
the one property no one-particle histogram can vouch for: that the hadrons of a sampled list are independent of each other."""
import itertools

import numpy as np
import pytest

import flow_cases as F
from is3d_amd import api

OPEN = dict(y_cut=5.0, y_gap=0.0, pT_min=0.0, pT_max=100.0)      # every particle below is inside


def at_angles(phi, event=0, pT=1.0, y=0.0, mass=0.13957):
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    p = np.zeros(len(phi), dtype=api.PARTICLE_DTYPE)
    mT = np.sqrt(mass * mass + pT * pT)
    p["E"], p["pz"], p["px"], p["py"], p["event"] = mT * np.cosh(y), mT * np.sinh(y), pT * np.cos(phi), pT * np.sin(phi), event
    return p


def cumulants_of(p, n_events=1, cuts=OPEN):
    return api.flow_cumulants(api.flow_list(cuts, n_events, 1, [0], p))


# A term is off by at most 2^-33 (llrint) plus libm's ulps; |Q| <= M <= 8, so |Q|^2 moves by less than 2 M^2 2^-33 and |Q|^4 by less than
# 4 M^4 2^-33, against denominators M (M - 1) >= 12 and M (M - 1)(M - 2)(M - 3) >= 24: <2> and <4> move by less than 2^-30 < 1e-8.
TOL = 1e-8


@pytest.mark.parametrize("M", (2, 4, 5, 9))
def test_particles_at_one_angle(M):
    c = cumulants_of(at_angles(np.full(M, 0.3)))
    assert c["n_used_2"][0] == 1 and c["n_used_4"][0] == (1 if M >= 4 else 0) and c["mean_M"][0] == M and c["var_M"][0] == 0.0
    assert np.abs(c["c2"][0] - 1.0).max() < TOL and np.abs(c["v2"][0] - 1.0).max() < TOL
    if M >= 4:
        assert np.abs(c["avg4"][0] - 1.0).max() < TOL and np.abs(c["c4"][0] + 1.0).max() < 4 * TOL and np.abs(c["v4"][0] - 1.0).max() < 4 * TOL
    assert np.abs(c["v_rp"][0] - np.cos(np.arange(1, 9) * 0.3)).max() < TOL


def test_a_regular_pentagon():
    c = cumulants_of(at_angles(2.0 * np.pi * np.arange(5) / 5.0))
    want = np.where(np.arange(1, 9) % 5 == 0, 1.0, -0.25)
    assert np.abs(c["c2"][0] - want).max() < TOL
    assert np.abs(c["v2"][0] - np.sign(want) * np.sqrt(np.abs(want))).max() < TOL


def test_one_back_to_back_pair():
    c = cumulants_of(at_angles([0.7, 0.7 + np.pi]))
    assert np.abs(c["c2"][0] - (-1.0) ** np.arange(1, 9)).max() < TOL and c["n_used_4"][0] == 0 and not c["c4"][0].any()


def test_brute_force_pairs_and_quadruplets():
    rng = np.random.default_rng(44)
    for M in (4, 5, 6, 7, 8):
        phi = rng.uniform(-np.pi, np.pi, M)
        c = cumulants_of(at_angles(phi))
        pairs = np.array(list(itertools.permutations(range(M), 2)))
        quads = np.array(list(itertools.permutations(range(M), 4)))
        for n in range(1, 9):
            two = np.cos(n * (phi[pairs[:, 0]] - phi[pairs[:, 1]])).mean()
            assert abs(c["c2"][0][n - 1] - two) < TOL, (M, n)
            if n <= 4:
                four = np.cos(n * (phi[quads[:, 0]] + phi[quads[:, 1]] - phi[quads[:, 2]] - phi[quads[:, 3]])).mean()
                assert abs(c["avg4"][0][n - 1] - four) < TOL, (M, n)
                assert abs(c["c4"][0][n - 1] - (four - 2.0 * two * two)) < 4 * TOL, (M, n)


def test_event_weights_and_events_left_out():
    """Events of 1, 2, 3 and 6 particles: <<2>> weighs by M (M - 1) and leaves the single out, <<4>> takes the last alone; mean and population
    variance of M over all four."""
    rng = np.random.default_rng(45)
    sizes = (1, 2, 3, 6)
    phis = [rng.uniform(-np.pi, np.pi, M) for M in sizes]
    p = np.concatenate([at_angles(phi, event=e) for e, phi in enumerate(phis)])
    c = cumulants_of(p, n_events=4)
    assert (c["n_used_2"][0], c["n_used_4"][0], c["n_used_gap"][0], c["n_events"][0]) == (3, 1, 0, 4)
    assert c["mean_M"][0] == 3.0 and abs(c["var_M"][0] - np.var(sizes)) < 1e-12
    num = sum(np.cos(2 * (phi[:, None] - phi[None, :])).sum() - len(phi) for phi in phis[1:])
    assert abs(c["c2"][0][1] - num / sum(M * (M - 1) for M in sizes[1:])) < TOL
    assert abs(c["avg4"][0][1] - cumulants_of(at_angles(phis[3]))["avg4"][0][1]) < 1e-12
    assert not c["c2_gap"][0].any()


def test_sub_event_correlator():
    """<2>_gap = Re(Q_A Q_B*) / (M_A M_B) against the explicit sum over pairs with one particle on each side of the gap."""
    rng = np.random.default_rng(46)
    y = np.array([-0.9, -0.5, -0.3, -0.1, 0.0, 0.2, 0.4, 0.8, 0.95])
    phi = rng.uniform(-np.pi, np.pi, len(y))
    r = api.flow_list(F.CUTS, 1, 1, [0], at_angles(phi, y=y))
    assert r["M"][0, 0].tolist() == [9, 3, 3]
    A, B = phi[y < -0.25], phi[y > 0.25]
    c = api.flow_cumulants(r)
    for n in range(1, 9):
        assert abs(c["c2_gap"][0][n - 1] - np.cos(n * (A[:, None] - B[None, :])).mean()) < TOL
    assert c["n_used_gap"][0] == 1


def test_the_region_rule_at_its_thresholds():
    eps = 1e-9
    cuts = F.CUTS
    edges = (-cuts["y_cut"], -0.5 * cuts["y_gap"], 0.5 * cuts["y_gap"], cuts["y_cut"])
    y = np.array([e + s * eps for e in edges for s in (-1.0, 1.0)])
    want = np.array([-1, 1, 1, 0, 0, 2, 2, -1])
    p = at_angles(np.linspace(0.1, 3.0, len(y)), y=y)
    assert np.array_equal(F.numpy_regions(cuts, p), want)
    # pT = pT_min is in, pT = pT_max is out (sqrt(fl(x * x)) = x), E = pz adds nothing, a photon along -z has ratio 0
    q = at_angles([0.0, 0.0, 0.0, 0.0], y=0.0)
    q["px"][:2], q["py"][:2] = (cuts["pT_min"], cuts["pT_max"]), 0.0
    q["pz"][2] = q["E"][2]
    q["pz"][3] = -q["E"][3]
    assert np.array_equal(F.numpy_regions(cuts, q), [0, -1, -1, -1])
    # ratio = 1 exactly with y_gap = 0: in the full acceptance, in neither sub-event
    z = at_angles([0.3, 0.4], y=0.0)
    flat = dict(cuts, y_gap=0.0)
    assert np.all(z["pz"] == 0.0) and np.array_equal(F.numpy_regions(flat, z), [0, 0])
    both = np.concatenate([p, q, z])
    both["event"] = np.arange(len(both))
    for c, reg in ((cuts, F.numpy_regions(cuts, both)), (flat, F.numpy_regions(flat, both))):
        M = api.flow_list(c, len(both), 1, [0], both)["M"][:, 0, :]
        assert np.array_equal(M[:, 0], reg >= 0) and np.array_equal(M[:, 1], reg == 1) and np.array_equal(M[:, 2], reg == 2)
    assert np.array_equal(F.numpy_regions(flat, both)[-2:], [0, 0])


def test_records_of_the_hand_list_are_the_restatement():
    """M by the numpy restatement of the rule, Q by numpy's atan2, cos and sin: within M units per record."""
    p, n_events = F.hand_list()
    slot = F.slot_map(3)
    r = api.flow_list(F.CUTS, n_events, 3, slot, p)
    assert np.array_equal(r["M"], F.numpy_M(F.CUTS, n_events, 3, slot, p))
    reg, s = F.numpy_regions(F.CUTS, p), slot[p["species"]]
    keep = (reg >= 0) & (s >= 0)
    phi = np.arctan2(p["py"], p["px"])
    for n in (1, 8):
        want = np.zeros((n_events, 3), dtype=np.int64)
        np.add.at(want, (p["event"][keep], s[keep]), np.rint(np.cos(n * phi[keep]) * 2.0 ** 32).astype(np.int64))
        assert np.all(np.abs(r["Q_re"][:, :, 0, n - 1] - want) <= r["M"][:, :, 0])


def test_merge_and_additivity():
    p, n_events = F.hand_list()
    slot = F.slot_map(3)
    r = api.flow_list(F.CUTS, n_events, 3, slot, p)
    one = api.flow_list(F.CUTS, n_events, 1, np.where(slot >= 0, 0, -1), p)
    assert F.same_bits(api.flow_merge(r, [0, 0, 0], 1), one)
    two = api.flow_merge(r, [1, -1, 0], 2)
    assert all(np.array_equal(two[k][:, 1], r[k][:, 0]) and np.array_equal(two[k][:, 0], r[k][:, 2]) for k in r)
    parts = [api.flow_list(F.CUTS, n_events, 3, slot, p[a:b]) for a, b in ((0, 100), (100, 101), (101, len(p)))]
    assert all(np.array_equal(sum(q[k] for q in parts), r[k]) for k in r)
    q, _ = F.shuffled_list()
    assert F.same_bits(api.flow_list(F.CUTS, n_events, 3, slot, q), r)


def test_hadrons_of_a_thermal_list_are_independent(fx):
    """pi+ from the CPU restatement of the sampler (tests/flow_cases.py: thermal_surface, 60 events, seed 20270; every event has M_A >= 5 and
    M_B >= 4).  For independent emission E[Q_A Q_B* | M_A, M_B] = M_A M_B q_A q_B*, so c_n{2,gap} must equal Re(qbar_A qbar_B*),
    qbar = sum Q / sum M over events, within the delete-one-event jackknife error: 5 sigma is the condition.  Observed pulls of this list:
    n = 2: -0.97, n = 3: +1.36.  A sampler whose hadrons share random numbers (two stream roles on one counter, a batch that replays a
    stream) fails here and passes every one-particle histogram."""
    from oracle import oracle
    cells, sp, gla, o, kw = F.thermal_surface()
    d, _ = oracle.sample_particles(cells, sp, fx["df"], gla, o, **kw)
    p = np.zeros(len(d["E"]), dtype=api.PARTICLE_DTYPE)
    for k in p.dtype.names:
        p[k] = d[k]
    r = api.flow_list(F.CUTS, kw["n_events"], 1, [0], p)
    pulls = F.independence_pulls(r)
    print("pulls", pulls)
    assert all(abs(v) <= 5.0 for v in pulls.values()), pulls


def test_the_independence_condition_catches_a_replayed_stream():
    """The same statistic on a list whose sub-event B repeats the azimuths of sub-event A: far outside 5 sigma."""
    rng = np.random.default_rng(47)
    n_events, M = 60, 8
    phi = rng.uniform(-np.pi, np.pi, (n_events, M))
    ev = np.repeat(np.arange(n_events), M)
    p = np.concatenate([at_angles(phi.ravel(), event=ev, y=-0.6), at_angles(phi.ravel(), event=ev, y=0.6)])
    pulls = F.independence_pulls(api.flow_list(F.CUTS, n_events, 1, [0], p))
    assert all(v > 5.0 for v in pulls.values()), pulls
