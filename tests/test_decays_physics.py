"""CPU: the physics of the two decay paths as far as it can be fixed without a device.  tests/decays_physics_ref.py holds references that
restate neither path (exact flat n-body phase space from a recursion of two-body momenta, thermal parents, the 3-body s rule's own defect,
moments over the shipped grid); here they are checked on their own -- against the closed Dalitz weight, against finer rules, against
weighted events, against analytic moments -- and then the two restatements the device is held to elsewhere (tests/decays_mc_ref.py,
tests/decays_restated.py) are held to them.  tests/test_gpu_decays_physics.py does the same with the device.

Every bound is a significance level (chi-square at 1e-6), a multiple of a standard error computed from the sample, or a figure the project
already holds (5e-4: the feed-down's quadrature allowance of tests/test_gpu_decays.py::test_two_body_conserves_yield)."""
import numpy as np
import pytest
from scipy.integrate import quad

import decays_mc_cases as cases
import decays_mc_ref as ref
import decays_physics_ref as P
import decays_restated as R
from is3d_amd import api, inputs
from oracle import oracle

G = inputs.grid()
PT, PHI = G["pT"], G["phi"]
NAMES = ["P3", "P4", "P5", "P5t"]


def test_three_body_reference_is_the_dalitz_weight():
    """n = 3 of the recursion against the closed form test_decays_mc.py::test_three_body_phase_space_is_flat uses: m12^2 is weighted with the
    length of the m23^2 interval, sqrt(lambda(s, m1^2, m2^2) lambda(M^2, s, m3^2)) / s"""
    M, (m1, m2, m3) = cases.PHASE_SPACE["P3"]
    lam = lambda a, b, c: a * a + b * b + c * c - 2.0 * (a * b + b * c + c * a)  # noqa: E731
    w = lambda s: np.sqrt(max(lam(s, m1 * m1, m2 * m2) * lam(M * M, s, m3 * m3), 0.0)) / s  # noqa: E731
    c = P.ClusterMass(M, (m1, m2, m3), 2)
    assert c.lo == m1 + m2 and c.hi == M - m3
    edges = np.linspace(c.lo, c.hi, 9)
    closed = np.array([quad(w, a * a, b * b, epsrel=1e-13, epsabs=0.0)[0] for a, b in zip(edges[:-1], edges[1:])])
    closed /= closed.sum()
    d = np.max(np.abs(c.bin_probabilities(edges) / closed - 1.0))
    print("n = 3, 8 equal-width bins: recursion / Dalitz - 1 = %.2e" % d)
    assert d <= 1e-6
    e = c.equal_probability_edges(8)
    got = np.array([quad(w, a * a, b * b, epsrel=1e-13, epsabs=0.0)[0] for a, b in zip(e[:-1], e[1:])])
    assert np.max(np.abs(got / got.sum() * 8.0 - 1.0)) <= 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_reference_converged_and_agrees_with_weighted_events(name):
    """the rules of the reference against finer ones (1e-6 relative is what it promises), then against 4e5 weighted proposals of the mass
    generation: the directly generated cluster's 20 equal-probability bins, and the mean weight over the bound.  The bound is one:
    no weight reaches it.  Measured (seed 11): chi-square 11.9 / 14.0 / 14.2 / 15.4 (bound 63.7), acceptance 0.34290 / 0.064446 /
    0.018425 / 0.029786, events off by -0.20 / -1.30 / -0.99 / -0.96 standard errors, largest weight 0.445 / 0.123 / 0.039 / 0.060 of the bound"""
    M, m = cases.PHASE_SPACE[name]
    n = len(m)
    a, fine = P.acceptance(M, m), P.acceptance(M, m, ng=64)
    assert abs(a / fine - 1.0) <= 1e-6
    c, cf = P.ClusterMass(M, m, n - 1), P.ClusterMass(M, m, n - 1, ng=64, deg=200)
    edges = cf.equal_probability_edges(20)
    assert np.max(np.abs(c.bin_probabilities(edges) * 20.0 - 1.0)) <= 1e-6
    assert np.max(np.abs(c.equal_probability_edges(20) - edges)) <= 1e-6 * (c.hi - c.lo)
    mu, w = P.mass_generation(M, m, 400000, np.random.default_rng(11))
    chi = P.chi_square(mu[:, n - 2], edges, np.full(20, 0.05), w)
    wm = P.wmax(M, m)
    z = (w.mean() / wm - a) / (w.std(ddof=1) / wm / np.sqrt(len(w)))
    print("%s: weighted chi-square %.1f (bound %.1f), acceptance %.5g, events %+.2f standard errors, largest weight %.3f of the bound"
          % (name, chi, P.chi_square_bound(20), a, z, w.max() / wm))
    print("    standard error of the events' acceptance %.2g" % (w.std(ddof=1) / wm / np.sqrt(len(w))))
    assert chi <= P.chi_square_bound(20)
    assert abs(z) <= 5.0
    assert w.max() < wm


def test_acceptances_are_the_recorded_ones():
    """0.0645 and 0.0184 were first measured with 4e5 weighted events, whose standard errors are 5.5e-5 and 1.5e-5 (the test above prints
    them): 5 of those plus the rounding of the third digit"""
    assert abs(P.acceptance(*cases.PHASE_SPACE["P4"]) - 0.0645) <= 5 * 5.5e-5 + 5e-5
    assert abs(P.acceptance(*cases.PHASE_SPACE["P5"]) - 0.0184) <= 5 * 1.5e-5 + 5e-5


@pytest.mark.parametrize("name", NAMES)
def test_power_unweighted_masses_fail_the_chi_square(name):
    """with the weight dropped (every proposal accepted) the chi-square of the device test, at its N = 2e5, is far past its threshold.
    Measured (seed 12): 2.52e4 / 8.70e4 / 2.31e4 / 2.09e4 against 63.7"""
    M, m = cases.PHASE_SPACE[name]
    n = len(m)
    mu, _ = P.mass_generation(M, m, 200000, np.random.default_rng(12))
    edges = P.ClusterMass(M, m, n - 1).equal_probability_edges(20)
    chi = P.chi_square(mu[:, n - 2], edges, np.full(20, 0.05))
    print("%s: chi-square of unweighted masses %.3g (bound %.1f)" % (name, chi, P.chi_square_bound(20)))
    assert chi > 10.0 * P.chi_square_bound(20)


@pytest.mark.parametrize("M,T", [(0.8961, 0.15), (0.78265, 0.3), (1.0, 0.15)])
def test_thermal_parents_have_their_analytic_moments(M, T):
    N, Yw = 400000, 2.5
    pT, phi, y = P.thermal_momenta(M, T, Yw, N, np.random.default_rng(13))
    for k in (1, 2):
        v = pT ** k
        z = (v.mean() - P.thermal_pT_moment(M, T, k)) / (v.std(ddof=1) / np.sqrt(N))
        print("M = %g T = %g: <pT^%d> = %.6g, sample %+.2f standard errors" % (M, T, k, P.thermal_pT_moment(M, T, k), z))
        assert abs(z) <= 5.0
    assert abs(y.mean()) <= 5.0 * Yw / np.sqrt(3.0 * N) and abs((y * y).mean() - Yw * Yw / 3.0) <= 5.0 * Yw * Yw * np.sqrt(4.0 / 45.0 / N)
    assert abs(np.cos(phi).mean()) <= 5.0 / np.sqrt(2.0 * N) and abs(np.sin(phi).mean()) <= 5.0 / np.sqrt(2.0 * N)
    # the same moments and the yield by quadrature, and by the shipped grid's nodes (pT to 40 GeV): what the grid itself adds to a moment
    # has to be negligible against the 5e-4 the feed-down tests allow, so a hundredth of it (measured: 4.2e-9 at most)
    dens = lambda p, k: p ** (k + 1) * np.exp(-(np.sqrt(p * p + M * M) - M) / T)  # noqa: E731
    row = np.exp(-np.sqrt(PT * PT + M * M) / T)[None, :] * np.ones((len(PHI), 1))
    mom = P.feed_moments(G, row)
    assert abs(mom[0] / P.thermal_dNdy(M, T) - 1.0) <= 5e-6
    for k in (1, 2):
        exact = quad(dens, 0.0, np.inf, args=(k,), epsrel=1e-12)[0] / quad(dens, 0.0, np.inf, args=(0,), epsrel=1e-12)[0]
        assert abs(P.thermal_pT_moment(M, T, k) / exact - 1.0) <= 1e-10
        assert abs(mom[k] / mom[0] / exact - 1.0) <= 5e-6
    # packed on the table's mass shell
    t, chosen = cases.FEED["F2"]
    q = P.thermal_parents(api, t, [313], 0, T, Yw, 1000, np.random.default_rng(14))
    assert np.max(np.abs(q["E"] ** 2 - q["px"] ** 2 - q["py"] ** 2 - q["pz"] ** 2 - 0.8961 ** 2)) <= 1e-12 * np.max(q["E"]) ** 2
    assert np.all(np.abs(np.arctanh(q["pz"] / q["E"])) <= Yw * (1.0 + 1e-12)) and np.all(q["species"] == 0)


def masses_but(mom, P0, n, j):
    """the invariant mass of all products but product j of every primary: mom [N n, 4] in product order, P0 [N, 4]"""
    rest = P0 - mom[j::n]
    return np.sqrt(np.maximum(rest[:, 0] ** 2 - (rest[:, 1:] ** 2).sum(1), 0.0))


N_RESTATED = 3000


@pytest.mark.parametrize("name", ["P4", "P5", "P5t"])
def test_restatement_has_the_exact_mass_distributions(name):
    """tests/decays_mc_ref.py on the 4- and 5-body tables, 3000 primaries, half of them moving: the mass of all products but the last (the
    directly generated cluster) and of all but the first (the most indirect one) in 8 equal-probability bins, chi-square at 1e-6 (7 degrees
    of freedom: 40.5), the proposals per decay within 5 standard errors of 1 / acceptance, and no primary out of proposals.
    Measured: chi-square (last, first) P4 11.3, 5.5; P5 6.3, 13.4; P5t 9.7, 5.8; proposals per decay off by -0.17 / -0.28 / +0.13 standard errors"""
    M, m = cases.PHASE_SPACE[name]
    n = len(m)
    t = cases.phase_space_table(name)
    p3 = np.random.default_rng(15).normal(size=(N_RESTATED, 3)) * 1.5
    p3[::2] = 0.0
    q = ref.make_particles(api, t, [cases.PARENT_ID], [0] * N_RESTATED, p3)
    r = ref.decay_particles(t, [cases.PARENT_ID], q, oracle.rng_uniforms, seed=16)
    assert r["stats"]["n_exhausted"] == 0 and r["stats"]["n_decays"] == N_RESTATED
    assert np.array_equal(r["origin"], np.repeat(np.arange(N_RESTATED), n)) and np.array_equal(r["species"], np.tile(np.arange(n), N_RESTATED))
    P0 = np.stack([q[k] for k in ref.MOM], 1)
    for j in (n - 1, 0):
        chi = P.chi_square(masses_but(r["mom"], P0, n, j), P.ClusterMass(M, m, j).equal_probability_edges(8), np.full(8, 0.125))
        print("%s: all but product %d: chi-square %.1f (bound %.1f)" % (name, j, chi, P.chi_square_bound(8)))
        assert chi <= P.chi_square_bound(8)
    a = P.acceptance(M, m)
    z = (r["stats"]["n_trials"] / N_RESTATED - 1.0 / a) / np.sqrt((1.0 - a) / (a * a * N_RESTATED))
    print("%s: %.2f proposals per decay, 1 / acceptance %.2f, %+.2f standard errors" % (name, r["stats"]["n_trials"] / N_RESTATED, 1.0 / a, z))
    assert abs(z) <= 5.0


def thermal_row(chosen_masses, T):
    """[phi][pT][S], the last species exp(-m_T / T) flat in phi, the others 0"""
    d = np.zeros((len(PHI), len(PT), len(chosen_masses)))
    d[:, :, -1] = np.exp(-np.sqrt(PT * PT + chosen_masses[-1] ** 2) / T)[None, :]
    return d.reshape(-1)


def chosen_masses(t, chosen):
    ids = [int(i) for i in t["mc_id"]]
    return [float(t["mass"][ids.index(c)]) for c in chosen]


def test_s_rule_defect_of_omega():
    """the 12-point s rule of omega -> 3 pi integrates 2.98e-4 more than the 24-point normalisation it is divided by"""
    d = P.s_rule_defect(api, 0.78265, 0.13957, 0.13957, 0.13498)
    print("omega -> 3 pi, the pi+ group: defect %.4e" % d)
    assert abs(d - 2.98e-4) <= 0.01e-4


@pytest.mark.parametrize("T", [0.15, 0.3])
@pytest.mark.parametrize("name", ["F2", "F3", "F3m", "Fbr"])
def test_feed_down_restatement_conserves_every_yield(name, T):
    """tests/decays_restated.py on the hand tables: each daughter's added dN/dy over the parent's analytic dN/dy is sum mult x BR, the 3-body
    groups corrected by the s rule's own defect, to 5e-4.  Residuals measured, (T = 0.15, T = 0.3):
    F2 K+ (-2.8e-9, -4.3e-10), pi- (-1.0e-5, -3.8e-6); F3 pi+ and pi- (-4.2e-6, -1.0e-6), pi0 (-3.7e-6, -1.1e-6);
    F3m pi+ and pi- (+9.1e-5, +8.4e-6); Fbr pi+ and pi- (+1.6e-4, +2.2e-5), pi0 (+3.0e-5, +6.4e-7).
    Without the defect the 3-body groups stand at +2.9e-4 / +3.0e-4 (F3), +4.5e-4 / +3.6e-4 (F3m) and +3.6e-4 / +3.3e-4 (Fbr pi0)."""
    t, chosen = cases.FEED[name]
    ms = chosen_masses(t, chosen)
    dN = thermal_row(ms, T)
    fed = R.feed_down(dN, t, chosen, PT, PHI)
    gain = (fed - dN).reshape(len(PHI), len(PT), len(chosen))
    assert np.all(gain[:, :, -1] == 0.0)
    want = cases.expected_yields(t, chosen, lambda *a: P.s_rule_defect(api, *a))
    plain = cases.expected_yields(t, chosen)
    parent = P.thermal_dNdy(ms[-1], T)
    for k, c in enumerate(chosen[:-1]):
        y = P.feed_moments(G, gain[:, :, k])[0] / parent
        print("%s T = %.2f daughter %d: yield %.6f, sum mult BR %.2f, residual %+.2e (without the s-rule defect %+.2e)"
              % (name, T, c, y, plain[c], y / want[c] - 1.0, y / plain[c] - 1.0))
        assert abs(y / want[c] - 1.0) <= 5e-4


def test_expected_yields_of_the_hand_tables():
    assert cases.expected_yields(*cases.FEED["F2"]) == {321: 1.0, -211: 1.0}
    assert cases.expected_yields(*cases.FEED["F3"]) == {211: 1.0, -211: 1.0, 111: 1.0}
    assert cases.expected_yields(*cases.FEED["F3m"]) == {211: 2.0, -211: 1.0}
    assert cases.expected_yields(*cases.FEED["Fbr"]) == {211: 1.0, -211: 1.0, 111: 0.4}


def test_power_recoil_mass_moves_the_pion_spectrum():
    """divergence 3 of DESIGN.md section 3h is invisible to a yield and plain in a shape: with the reference's recoil mass (particle_2, the pion
    itself) K* -> K pi keeps the pion's yield to 2.5e-4 and moves its <pT> from 0.3016 to 0.4337 (T = 0.15)"""
    t, chosen = cases.FEED["F2"]
    dN = thermal_row(chosen_masses(t, chosen), 0.15)
    mom = {}
    for recoil in ("partner", "particle_2"):
        gain = (R.feed_down(dN, t, chosen, PT, PHI, recoil=recoil) - dN).reshape(len(PHI), len(PT), 3)
        mom[recoil] = P.feed_moments(G, gain[:, :, 1])
    a, b = mom["partner"], mom["particle_2"]
    print("pi- of K*: yield ratio - 1 = %.2e, <pT> %.4f (partner) %.4f (particle_2)" % (b[0] / a[0] - 1.0, a[1] / a[0], b[1] / b[0]))
    assert abs(b[0] / a[0] - 1.0) <= 5e-4
    assert abs((b[1] / b[0]) / (a[1] / a[0]) - 1.0) > 0.10
