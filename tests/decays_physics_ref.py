"""Test helper: references for the two decay paths that restate neither of them (numpy and scipy only).

(a) Flat n-body phase space, exactly.  With p*(a; b, c) the momentum of b and c in the rest frame of a and S_k = m_0 + ... + m_k,
        G_2(mu) = p*(mu; m_0, m_1),     G_k(mu) = int_{S_{k-2}}^{mu - m_{k-1}} dmu' G_{k-1}(mu') p*(mu; mu', m_{k-1}),
    the invariant mass mu of all products but the last has density ~ G_{n-1}(mu) p*(M; mu, m_{n-1}) on [S_{n-2}, M - m_{n-1}], and G_n(M) is
    the phase-space volume in the cluster masses.  Phase space is symmetric under relabelling, so the same formula with product j moved to
    the end is the mass of all products but j.  Every integral is a fixed Gauss-Legendre rule in t, mu' = lo + (hi - lo) sin^2(pi t / 2),
    which turns the square-root end points of p* and of G_{k-1} into analytic factors; the distribution function is the integral of a
    Chebyshev interpolant in the same variable.  tests/test_decays_physics.py checks n = 3 against the closed Dalitz weight, the rules
    against finer ones (1e-6 relative is the aim) and all of it against weighted events.
(b) Thermal boost-invariant parents dN / (dy pT dpT dphi) = A exp(-m_T / T), flat in y on [-Y_w, Y_w], with their analytic <pT^k>.
(c) The defect of the feed-down's 12-point s rule against its own 24-point normalisation for a 3-body group.
(d) Moments of a feed-down gain over the pT and phi nodes of the shipped grid."""
import math

import numpy as np
from numpy.polynomial.chebyshev import Chebyshev
from scipy import optimize, special, stats

import decays_mc_ref as mc_ref

NG = 40          # Gauss-Legendre points of every nested integral
DEG = 128        # degree of the Chebyshev interpolant of the mass density in t
_rules = {}


def pstar(a, b, c):
    v = (a - b - c) * (a + b + c) * (a + b - c) * (a - b + c)
    return np.sqrt(np.maximum(v, 0.0)) / (2.0 * a)


def _rule(ng):
    if ng not in _rules:
        x, w = np.polynomial.legendre.leggauss(ng)
        t = 0.5 * (x + 1.0)
        _rules[ng] = (np.sin(0.5 * np.pi * t), np.cos(0.5 * np.pi * t), 0.5 * w)
    return _rules[ng]


def G(masses, mu, ng=NG):
    """G_k(mu), k = len(masses), at every mu of an array"""
    m = [float(x) for x in masses]
    mu = np.asarray(mu, np.float64)
    if len(m) == 2:
        return pstar(mu, m[0], m[1])
    lo = math.fsum(m[:-1])
    L = np.maximum(mu - m[-1] - lo, 0.0)[..., None]
    s, c, w = _rule(ng)
    x = lo + L * (s * s)
    return np.sum(w * (np.pi * s * c) * L * G(m[:-1], x, ng) * pstar(mu[..., None], x, m[-1]), axis=-1)


def wmax(M, masses):
    """the bound the mass generation accepts against: prod_k p*(T + S_k; S_{k-1}, m_k)"""
    S = np.cumsum(masses)
    T = M - S[-1]
    return float(np.prod([pstar(T + S[k], S[k - 1], masses[k]) for k in range(1, len(masses))]))


def acceptance(M, masses, ng=NG):
    """E[w] / wmax of the mass generation: the sorted uniforms fill a simplex of volume T^(n-2) / (n-2)! in the cluster masses"""
    n = len(masses)
    if n == 2:
        return 1.0
    T = M - math.fsum(masses)
    return float(G(masses, np.float64(M), ng)) / (wmax(M, masses) * T ** (n - 2) / math.factorial(n - 2))


class ClusterMass:
    """the invariant mass of all products but product j of M -> masses in flat phase space"""

    def __init__(self, M, masses, j=-1, ng=NG, deg=DEG):
        m = [float(x) for x in masses]
        last = m.pop(j)
        assert len(m) >= 2
        self.lo, self.hi = math.fsum(m), float(M) - last
        L = self.hi - self.lo

        def h(t):
            s, c = np.sin(0.5 * np.pi * t), np.cos(0.5 * np.pi * t)
            mu = self.lo + L * s * s
            return G(m, mu, ng) * pstar(float(M), mu, last) * (np.pi * L) * s * c

        self._F = Chebyshev.interpolate(h, deg, domain=[0.0, 1.0]).integ(lbnd=0.0)
        self._norm = float(self._F(1.0))

    def _t(self, mu):
        return (2.0 / np.pi) * np.arcsin(np.sqrt(np.clip((np.asarray(mu, np.float64) - self.lo) / (self.hi - self.lo), 0.0, 1.0)))

    def cdf(self, mu):
        return self._F(self._t(mu)) / self._norm

    def bin_probabilities(self, edges):
        return np.diff(self.cdf(edges))

    def equal_probability_edges(self, bins):
        t = [0.0] + [optimize.brentq(lambda t, q=q: self._F(t) / self._norm - q, 0.0, 1.0, xtol=1e-15, rtol=1e-15)
                     for q in np.arange(1, bins) / bins] + [1.0]
        return self.lo + (self.hi - self.lo) * np.sin(0.5 * np.pi * np.array(t)) ** 2


def chi_square(x, edges, prob, weights=None):
    """Pearson's chi-square of the values x in the bins `edges` (values past an end by rounding fall into the end bins) against the bin
    probabilities `prob`; with weights, the weighted counts against the variance the sample itself gives them"""
    k = np.searchsorted(edges[1:-1], x, side="right")
    if weights is None:
        obs = np.bincount(k, minlength=len(prob)).astype(np.float64)
        exp = len(x) * np.asarray(prob)
        return float(np.sum((obs - exp) ** 2 / exp))
    W, p = float(np.sum(weights)), np.asarray(prob)
    sw = np.bincount(k, weights=weights, minlength=len(prob))
    # per event z_i = w_i (1[bin] - p): the bin's weighted count minus p W is sum z_i with variance ~ sum z_i^2
    sw2 = np.bincount(k, weights=weights * weights, minlength=len(prob))
    # (N p (1 - p) for unit weights: divided by 1 - p it is Pearson's denominator)
    var = sw2 * (1.0 - 2.0 * p) + p * p * float(np.sum(weights * weights))
    return float(np.sum((sw - p * W) ** 2 * (1.0 - p) / var))


def chi_square_bound(bins, level=1e-6):
    return float(stats.chi2.isf(level, bins - 1))


def mass_generation(M, masses, N, rng):
    """N proposals of the mass generation, vectorised: the cluster masses mu [N, n] (mu[:, k] is the mass of products 0..k) and the weight
    prod_k p*(mu_k; mu_{k-1}, m_k) of each.  Flat phase space is these proposals WITH their weights."""
    m = np.asarray(masses, np.float64)
    n = len(m)
    S = np.cumsum(m)
    T = M - S[-1]
    r = np.sort(rng.random((N, n - 2)), axis=1)
    mu = np.concatenate([np.full((N, 1), m[0]), S[1:n - 1] + r * T, np.full((N, 1), float(M))], axis=1)
    w = np.ones(N)
    for k in range(1, n):
        w = w * pstar(mu[:, k], mu[:, k - 1], m[k])
    return mu, w


# ---- (b) thermal parents ----
def thermal_pT_moment(M, T, k):
    """<pT^k> of dN / (pT dpT) ~ exp(-m_T / T), k = 0, 1, 2"""
    if k == 0:
        return 1.0
    if k == 1:
        return M * M * special.kve(2, M / T) / (M + T)       # M^2 T K_2(M / T) over T (M + T) exp(-M / T)
    if k == 2:
        return (6.0 * T ** 3 + 6.0 * M * T * T + 2.0 * M * M * T) / (M + T)
    raise ValueError(k)


def thermal_dNdy(M, T, A=1.0):
    """int pT dpT dphi A exp(-m_T / T)"""
    return 2.0 * np.pi * A * T * (M + T) * np.exp(-M / T)


def thermal_momenta(M, T, Yw, N, rng):
    """(pT, phi, y) of N parents: m_T - M is Exp(T) with probability M / (M + T), else Gamma(2, T) -- the two terms of (x + M) exp(-x / T)"""
    x = np.where(rng.random(N) < M / (M + T), rng.exponential(T, N), rng.gamma(2.0, T, N))
    mT = M + x
    return np.sqrt(mT * mT - M * M), rng.uniform(0.0, 2.0 * np.pi, N), rng.uniform(-Yw, Yw, N)


def thermal_parents(api, table, chosen_mc_id, species, T, Yw, N, rng):
    """N thermal primaries of chosen_mc_id[species] on the table's mass shell, packed as the Monte Carlo entry reads them"""
    ids = [int(i) for i in table["mc_id"]]
    M = float(table["mass"][ids.index(int(chosen_mc_id[species]))])
    pT, phi, y = thermal_momenta(M, T, Yw, N, rng)
    p3 = np.stack([pT * np.cos(phi), pT * np.sin(phi), np.sqrt(pT * pT + M * M) * np.sinh(y)], axis=1)
    return mc_ref.make_particles(api, table, chosen_mc_id, np.full(N, species), p3, events=np.zeros(N, np.int64))


# ---- (c) the 3-body s rule ----
def s_rule_defect(api, M, m1, m2, m3):
    """(12-point Gauss-Legendre of sqrt|(a - s)(b - s)(s - c)(s - d)| / s over [c, b]) / is3d_decay_q_factor - 1 for the group of m1: the
    yield of a 3-body group over mult x BR, minus 1, as far as the s rule goes"""
    a, b, c, d = (M + m1) ** 2, (M - m1) ** 2, (m2 + m3) ** 2, (m2 - m3) ** 2
    x, w = np.polynomial.legendre.leggauss(12)
    s = c + (b - c) * (1.0 + x) / 2.0
    return float(np.sum(w * (b - c) / 2.0 * np.sqrt(np.abs((a - s) * (b - s) * (s - c) * (s - d))) / s)) / api.decay_q_factor(M, m1, m2, m3) - 1.0


# ---- (d) moments of a feed-down result ----
def feed_moments(grid, gain, kmax=2):
    """[sum phi_w pT_w pT^k gain for k = 0..kmax]; gain is [n_phi][n_pT] (pT_w carries the pT of pT dpT)"""
    g = np.asarray(gain, np.float64).reshape(len(grid["phi"]), len(grid["pT"]))
    return np.array([float(np.einsum("j,i,ji->", grid["phi_w"], grid["pT_w"] * grid["pT"] ** k, g)) for k in range(kmax + 1)])
