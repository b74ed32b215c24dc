"""GPU (-m gpu): the two decay kernels against physics neither of their restatements can vouch for (tests/decays_physics_ref.py; the
references are checked on their own in tests/test_decays_physics.py).  Every table is hand-made (tests/decays_mc_cases.py).

Part A: is3d_decay_particles (cf_decay_mc) against exact flat n-body phase space, n = 3, 4 (one product massless), 5 and 5 at 20 MeV above
threshold: 2e5 primaries, half at rest and half moving, so the invariants are formed from boosted momenta.  The mass of all products but
one in 20 equal-probability bins (chi-square at 1e-6), the proposals per decay against the exact acceptance of the rejection, the
isotropy of every product in its parent's rest frame, and the proper times of a second-generation decay.

Part B: the feed-down (cf_decay_feed, quadrature) and the Monte Carlo entry (event generation) compute the same physical quantity: the
spectrum of the daughters of thermal boost-invariant parents at mid-rapidity.  Yield, <pT> and <pT^2> of every daughter species agree
within 5 standard errors of the sample plus 5e-4, the feed-down's quadrature allowance (test_gpu_decays.py::test_two_body_conserves_yield).

Every bound is a significance level, a multiple of a standard error computed from the sample, or a figure the project already holds."""
import numpy as np
import pytest

import decays_mc_cases as cases
import decays_mc_ref as ref
import decays_physics_ref as P
import decays_restated as R
from is3d_amd import api, inputs

pytestmark = pytest.mark.gpu

G = inputs.grid()
PT, PHI = G["pT"], G["phi"]
GRID = dict(pT=PT, phi=PHI, y=G["y"])
NAMES = ["P3", "P4", "P5", "P5t"]
N = 200000
BINS = 20
_runs = {}


# ---------------------------------------------------------------- part A ----------------------------------------------------------------
def primaries(t, n_primaries, seed):
    """the first half at rest, the second with N(0, 1.5 GeV) per component"""
    p3 = np.random.default_rng(seed).normal(size=(n_primaries, 3)) * 1.5
    p3[:n_primaries // 2] = 0.0
    return ref.make_particles(api, t, [cases.PARENT_ID], np.zeros(n_primaries, np.int64), p3, events=np.zeros(n_primaries, np.int64))


def decayed(t, q, n, seed):
    """the device's momenta [N n, 4] in product order (asserted through origin and species), the parents' [N, 4], the stats"""
    out, origin, st = api.decay_particles(t, [cases.PARENT_ID], q, seed=seed, capacity=n * len(q))
    assert st["n_exhausted"] == 0 and st["n_decays"] == len(q) and st["n_final"] == len(out) == n * len(q)
    assert np.array_equal(origin, np.repeat(np.arange(len(q)), n)) and np.array_equal(out["species"], np.tile(np.arange(n), len(q)))
    mom = np.stack([out[k] for k in ref.MOM], axis=1)
    P0 = np.stack([q[k] for k in ref.MOM], axis=1)
    cons = float(np.max(np.abs(mom.reshape(len(q), n, 4).sum(axis=1) - P0) / P0[:, :1]))
    assert cons <= cases.BOUND, cons
    return mom, P0, st


def run(name):
    if name not in _runs:
        t = cases.phase_space_table(name)
        _runs[name] = decayed(t, primaries(t, N, 41), len(cases.PHASE_SPACE[name][1]), seed=42)
    return _runs[name]


def masses_but(mom, P0, n, j):
    rest = P0 - mom[j::n]
    return np.sqrt(np.maximum(rest[:, 0] ** 2 - (rest[:, 1:] ** 2).sum(1), 0.0))


@pytest.mark.parametrize("name", NAMES)
def test_cluster_masses_follow_exact_phase_space(name):
    """the mass of all products but the last (the cluster the mass generation draws directly) and of all but the first (reached through every
    split and boost), 20 equal-probability bins of the exact distribution, Pearson's chi-square at 1e-6 with 19 degrees of freedom (63.7), for
    all primaries, those at rest and those moving.  Measured on the MI355X (all / rest / moving):
    P3 last 19.9 / 30.9 / 10.2, first 23.9 / 19.9 / 24.0; P4 last 23.2 / 17.9 / 22.0, first 19.4 / 18.4 / 23.7;
    P5 last 11.5 / 10.2 / 13.0, first 12.7 / 15.4 / 16.1; P5t last 18.7 / 17.4 / 14.3, first 18.6 / 15.5 / 15.0.
    With the weight dropped the same statistic stands at 2e4 to 9e4 (tests/test_decays_physics.py)."""
    M, m = cases.PHASE_SPACE[name]
    n = len(m)
    mom, P0, _ = run(name)
    for j in (n - 1, 0):
        edges = P.ClusterMass(M, m, j).equal_probability_edges(BINS)
        x = masses_but(mom, P0, n, j)
        chi = [P.chi_square(v, edges, np.full(BINS, 1.0 / BINS)) for v in (x, x[:N // 2], x[N // 2:])]
        print("%s all but product %d: chi-square %.1f (all) %.1f (at rest) %.1f (moving), bound %.1f" % (name, j, *chi, P.chi_square_bound(BINS)))
        assert max(chi) <= P.chi_square_bound(BINS)


@pytest.mark.parametrize("name", NAMES)
def test_proposals_per_decay_are_the_exact_acceptance(name):
    """n_trials / n_decays is geometric with the exact acceptance a = phase-space volume / (wmax T^(n-2) / (n-2)!): within 5 standard errors
    sqrt((1 - a) / (a^2 N)) of 1 / a.  Measured on the MI355X: P3 2.9231 (1 / a 2.9163, +1.29 s.e.), P4 15.5165 (15.5170, -0.01),
    P5 54.1567 (54.2746, -0.98), P5t 33.5338 (33.5733, -0.53)"""
    M, m = cases.PHASE_SPACE[name]
    _, _, st = run(name)
    a = P.acceptance(M, m)
    z = (st["n_trials"] / st["n_decays"] - 1.0 / a) / np.sqrt((1.0 - a) / (a * a * N))
    print("%s: %.4f proposals per decay, 1 / acceptance %.4f, %+.2f standard errors" % (name, st["n_trials"] / st["n_decays"], 1.0 / a, z))
    assert abs(z) <= 5.0


def rest_frame(p, Pp):
    """p [K, 4] in the rest frame of Pp [K, 4], by components along and across the flight direction: returns (cosine to the flight direction,
    azimuth about it)"""
    Mp = np.sqrt(Pp[:, 0] ** 2 - (Pp[:, 1:] ** 2).sum(1))
    Pabs = np.sqrt((Pp[:, 1:] ** 2).sum(1))
    nhat = Pp[:, 1:] / Pabs[:, None]
    along = (p[:, 1:] * nhat).sum(1)
    across = p[:, 1:] - along[:, None] * nhat
    along_rest = (Pp[:, 0] * along - Pabs * p[:, 0]) / Mp               # gamma (p_par - beta E)
    # a right-handed frame about the flight direction: e1 = z x n / |z x n|, e2 = n x e1
    e1 = np.stack([-nhat[:, 1], nhat[:, 0], np.zeros(len(nhat))], axis=1)
    e1 /= np.sqrt((e1 ** 2).sum(1))[:, None]
    e2 = np.cross(nhat, e1)
    cos = along_rest / np.sqrt(along_rest ** 2 + (across ** 2).sum(1))
    return cos, np.arctan2((across * e2).sum(1), (across * e1).sum(1))


@pytest.mark.parametrize("name", NAMES)
def test_every_product_is_isotropic_in_the_parents_rest_frame(name):
    """the moving half: each product taken back to its parent's rest frame by components along and across the flight direction (not the
    (gamma - 1) b.q / b^2 form of the kernel and its restatement).  cos(theta) to the flight direction has mean 0 +- 5 / sqrt(3 K) and mean
    square 1/3 +- 5 sqrt(4 / (45 K)); the azimuth about it has <cos>, <sin> = 0 +- 5 / sqrt(2 K).  Largest of the four over the products, in
    standard errors, measured on the MI355X: P3 2.4, P4 2.5, P5 2.0, P5t 3.1.  The half at rest (no boost at the first split) has no flight
    direction: the same four moments about the z axis, measured P3 1.2, P4 2.1, P5 2.4, P5t 1.9"""
    n = len(cases.PHASE_SPACE[name][1])
    mom, P0, _ = run(name)
    K = N - N // 2
    worst = 0.0
    for j in range(n):
        p = mom[j::n]
        at_rest = p[:N // 2]
        assert len(at_rest) == K
        moving = rest_frame(p[N // 2:], P0[N // 2:])
        resting = (at_rest[:, 3] / np.sqrt((at_rest[:, 1:] ** 2).sum(1)), np.arctan2(at_rest[:, 2], at_rest[:, 1]))
        for what, (cos, az) in (("moving", moving), ("at rest", resting)):
            z = [cos.mean() * np.sqrt(3.0 * K), ((cos * cos).mean() - 1.0 / 3.0) / np.sqrt(4.0 / (45.0 * K)),
                 np.cos(az).mean() * np.sqrt(2.0 * K), np.sin(az).mean() * np.sqrt(2.0 * K)]
            print("%s product %d %s: <cos> %+.2f, <cos^2> %+.2f, azimuth <cos> %+.2f <sin> %+.2f standard errors" % (name, j, what, *z))
            worst = max(worst, np.max(np.abs(z)))
    assert worst <= 5.0


@pytest.mark.parametrize("count", [63, 65])
@pytest.mark.parametrize("name", NAMES)
def test_short_lists_conserve_and_never_run_out_of_proposals(name, count):
    """off the wave size: decayed() asserts n_exhausted == 0, the output order and four-momentum conservation to BOUND"""
    t = cases.phase_space_table(name)
    decayed(t, primaries(t, count, 43), len(cases.PHASE_SPACE[name][1]), seed=44)


def test_second_generation_lifetime():
    """lifetime = 1 on X(1.5, width 0.1) -> R(0.77, width 0.15) pi0, R -> pi+ pi-: the proper time from X's vertex (where its pi0 is born) to
    R's vertex (where R's pions are born, both at one point) has mean hbarc / width_R, X's own flight hbarc / width_X, each within
    5 / sqrt(K) of it.  Measured on the MI355X: R 1.3119 fm (1.3155, -0.39 standard errors), X 1.9764 fm (1.9733, +0.22)"""
    K = 20000
    t = cases.CHAIN
    q = ref.make_particles(api, t, [9900], np.zeros(K, np.int64), np.random.default_rng(45).normal(size=(K, 3)) * 0.8)
    out, origin, st = api.decay_particles(t, [9900], q, seed=46, lifetime=1, capacity=3 * K)
    assert st["n_decays"] == 2 * K and len(out) == 3 * K and np.array_equal(origin, np.repeat(np.arange(K), 3))
    ids = t["mc_id"][out["species"]]
    assert np.array_equal(ids, np.tile([211, -211, 111], K))
    a, b, c = out[0::3], out[1::3], out[2::3]
    assert all(np.array_equal(a[k], b[k]) for k in ref.POS)

    def proper(u, v):
        d = [u[k] - v[k] for k in ("t", "x", "y", "z")]
        return np.sqrt(np.maximum(d[0] ** 2 - d[1] ** 2 - d[2] ** 2 - d[3] ** 2, 0.0))

    for what, tau, width in (("R", proper(a, c), 0.15), ("X", proper(c, q), 0.1)):
        tau0 = ref.HBARC / width
        z = (tau.mean() - tau0) / (tau0 / np.sqrt(K))
        print("%s: mean proper time %.4f fm, hbarc / width %.4f, %+.2f standard errors" % (what, tau.mean(), tau0, z))
        assert abs(z) <= 5.0
    assert np.all(a["t"] > c["t"]) and np.all(c["t"] > q["t"])


# ---------------------------------------------------------------- part B ----------------------------------------------------------------
N_MC = 2000000
BATCH = 250000
Y_W = 2.5
TEMPS = [0.15, 0.3]
FEEDS = ["F2", "F3", "F3m", "Fbr"]
_mc, _fed = {}, {}


def masses_of(t, ids_wanted):
    ids = [int(i) for i in t["mc_id"]]
    return [float(t["mass"][ids.index(int(c))]) for c in ids_wanted]


def thermal_row(ms, T):
    """[phi][pT][S]: the last species exp(-m_T / T), flat in phi; the others 0"""
    d = np.zeros((len(PHI), len(PT), len(ms)))
    d[:, :, -1] = np.exp(-np.sqrt(PT * PT + ms[-1] ** 2) / T)[None, :]
    return d.reshape(-1)


def feed_err(got, want, base, S):
    """worst |feed-down difference| relative to the largest feed-down of the same daughter (as tests/test_gpu_decays.py)"""
    dg, dr = (got - base).reshape(-1, S), (want - base).reshape(-1, S)
    scale = np.max(np.abs(dr), axis=0)
    live = scale > 0
    return float(np.max(np.abs(dg - dr)[:, live] / scale[live]))


def moments_of(fed, dN, chosen, T, ms):
    """per daughter: (yield per unit parent dN/dy, <pT>, <pT^2>) of its gain"""
    gain = (fed - dN).reshape(len(PHI), len(PT), len(chosen))
    out = {}
    for k, c in enumerate(chosen[:-1]):
        m = P.feed_moments(G, gain[:, :, k])
        out[int(c)] = (m[0] / P.thermal_dNdy(ms[-1], T), m[1] / m[0], m[2] / m[0])
    return out


def fed_down(name, T):
    if (name, T) not in _fed:
        t, chosen = cases.FEED[name]
        ms = masses_of(t, chosen)
        dN = thermal_row(ms, T)
        got, _ = api.resonance_decays(t, chosen, GRID, dN, dimension=2)
        _fed[name, T] = (got, dN, moments_of(got, dN, chosen, T, ms))
    return _fed[name, T]


def max_rapidity_shift(t, chosen):
    """the largest asinh(p* / m) over the products of the parent's channels: p* is largest when the other products move together"""
    ids = [int(i) for i in t["mc_id"]]
    e = ids.index(int(chosen[-1]))
    first = int(np.sum(t["n_channels"][:e]))
    M, worst = float(t["mass"][e]), 0.0
    for c in range(first, first + int(t["n_channels"][e])):
        ms = masses_of(t, t["daughters"][c][:abs(int(t["npart"][c]))])
        for k, mk in enumerate(ms):
            worst = max(worst, float(np.arcsinh(P.pstar(M, mk, sum(ms) - mk) / mk)))
    return worst


def monte_carlo(name, T):
    """per daughter id: [(value, standard error)] of the yield per unit parent dN/dy, <pT> and <pT^2> among the daughters with |y| <= 0.5 of
    N_MC thermal parents flat in |y| <= Y_W, decayed in batches through first_particle.  The standard errors come from the per-parent
    sums (count c, sum of pT^k a): N var(c) for the yield, sum (a - R c)^2 / C^2 for the ratio R = A / C."""
    if (name, T) in _mc:
        return _mc[name, T]
    t, chosen = cases.FEED[name]
    assert Y_W >= 0.5 + max_rapidity_shift(t, chosen)
    ids = [int(i) for i in t["mc_id"]]
    rng = np.random.default_rng(1000 + 7 * FEEDS.index(name) + int(100 * T))
    nbody = int(np.max(np.abs(t["npart"])))
    acc = {int(c): np.zeros(8) for c in chosen[:-1]}                  # C, sum c^2, A1, sum a1^2, sum a1 c, A2, sum a2^2, sum a2 c
    for first in range(0, N_MC, BATCH):
        q = P.thermal_parents(api, t, [chosen[-1]], 0, T, Y_W, BATCH, rng)
        out, origin, st = api.decay_particles(t, [chosen[-1]], q, seed=77, first_particle=first, capacity=nbody * BATCH)
        assert st["n_exhausted"] == 0 and st["n_decays"] == BATCH and st["n_stuck"] == 0
        keep = np.abs(np.arctanh(out["pz"] / out["E"])) <= 0.5
        pT2 = out["px"] ** 2 + out["py"] ** 2
        for c in acc:
            sel = keep & (out["species"] == ids.index(c))
            o, v2 = origin[sel], pT2[sel]
            cnt = np.bincount(o, minlength=BATCH).astype(np.float64)
            a1, a2 = np.bincount(o, np.sqrt(v2), minlength=BATCH), np.bincount(o, v2, minlength=BATCH)
            acc[c] += [cnt.sum(), (cnt * cnt).sum(), a1.sum(), (a1 * a1).sum(), (a1 * cnt).sum(), a2.sum(), (a2 * a2).sum(), (a2 * cnt).sum()]
    res = {}
    for c, (C, cc, A1, a11, a1c, A2, a22, a2c) in acc.items():
        scale = Y_W / (0.5 * N_MC)
        r = [(C * scale, np.sqrt(N_MC * (cc / N_MC - (C / N_MC) ** 2)) * scale)]
        for A, aa, ac in ((A1, a11, a1c), (A2, a22, a2c)):
            Rk = A / C
            r.append((Rk, np.sqrt(aa - 2.0 * Rk * ac + Rk * Rk * cc) / C))
        res[c] = r
    _mc[name, T] = res
    return res


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("name", FEEDS)
def test_feed_down_equals_its_restatement_on_the_hand_tables(name, T):
    """the existing 1e-10 of tests/test_gpu_decays.py on these tables; measured on the MI355X: 8.0e-14 (F2) to 1.7e-13 (F3m)"""
    t, chosen = cases.FEED[name]
    got, dN, _ = fed_down(name, T)
    want = R.feed_down(dN, t, chosen, PT, PHI)
    err = feed_err(got, want, dN, len(chosen))
    print("%s T = %.2f: worst feed-down error against the restatement %.2e" % (name, T, err))
    assert np.isfinite(got).all() and err < 1e-10


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("name", FEEDS)
def test_feed_down_and_monte_carlo_agree(name, T):
    """yield per unit parent dN/dy (the 3-body s rule's own defect taken out of the feed-down's), <pT> and <pT^2> of every daughter species:
    |feed-down - Monte Carlo| <= 5 standard errors of the sample + 5e-4 of the value.  The parent is log-linear in M_T and flat in phi, so the
    feed-down's interpolation and fit are exact and only its 12-point rules remain; 5e-4 is what the project allows those.
    Measured on the MI355X, 2e6 parents per case (0.6 s each, so N stays at 2e6): of the 60 differences the largest is 2.96 standard errors (the pi-
    yield of F3 at T = 0.15: 0.99582 +- 0.00141 against 1.00000); the standard errors are 1.4e-3 of a yield and 0.8e-3 to 2.6e-3 of a moment."""
    t, chosen = cases.FEED[name]
    _, _, fd = fed_down(name, T)
    mc = monte_carlo(name, T)
    plain = cases.expected_yields(t, chosen)
    with_defect = cases.expected_yields(t, chosen, lambda *a: P.s_rule_defect(api, *a))
    bad = []
    for c in plain:
        want = (fd[c][0] - (with_defect[c] - plain[c]), fd[c][1], fd[c][2])
        for what, w, (v, se) in zip(("yield", "<pT>", "<pT^2>"), want, mc[c]):
            z = (v - w) / se
            print("%s T = %.2f daughter %5d %-7s feed-down %.6f Monte Carlo %.6f +- %.6f (%+.2f standard errors)" % (name, T, c, what, w, v, se, z))
            if abs(v - w) > 5.0 * se + 5e-4 * abs(w):
                bad.append((c, what, w, v, se))
    assert not bad, bad


@pytest.mark.parametrize("T", TEMPS)
def test_power_monte_carlo_rejects_the_reference_recoil_mass(T):
    """the comparison has teeth: the restatement with the reference's recoil mass (divergence 3) gives the pion of
    K* -> K pi a <pT> that the same Monte Carlo sample rejects by more than 20 standard errors.  Measured on the MI355X: 0.4337 against
    0.3017 +- 0.0003 (519 standard errors) at T = 0.15, 0.5464 against 0.3831 +- 0.0004 (408) at T = 0.3"""
    t, chosen = cases.FEED["F2"]
    ms = masses_of(t, chosen)
    dN = thermal_row(ms, T)
    wrong = moments_of(R.feed_down(dN, t, chosen, PT, PHI, recoil="particle_2"), dN, chosen, T, ms)[-211]
    v, se = monte_carlo("F2", T)[-211][1]
    print("T = %.2f: pi- <pT> Monte Carlo %.4f +- %.4f, particle_2 recoil %.4f: %.0f standard errors" % (T, v, se, wrong[1], abs(v - wrong[1]) / se))
    assert abs(v - wrong[1]) > 20.0 * se
    assert abs(wrong[0] - 1.0) <= 5e-4          # ... while its yield is as good as the right one's
