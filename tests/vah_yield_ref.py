"""The mean yield of an anisotropic-hydro surface (is3d_total_yield_vah, include/is3d_amd.h) restated in numpy: the same alpha = 1
Gauss-Laguerre nodes, the same closed form, float64 -- and the cell helpers of tests/test_gpu_sampler_vah.py that the yield tests share
(copied: a test module is not imported from another).

Per cell with u.dsigma > 0 and species (m, sign, g), mbar = m / Lambda, Ebar_k = sqrt(r_k^2 + mbar^2) on the nodes (r_k, w_k):
    N0 = sum_k w_k r_k   e^{r_k}          / (e^{Ebar_k} + sign)
    A0 = sum_k w_k r_k   e^{r_k + Ebar_k} / (e^{Ebar_k} + sign)^2
    A2 = sum_k w_k r_k^3 e^{r_k + Ebar_k} / (e^{Ebar_k} + sign)^2
    K_m = [bulk] Pi (c0 + c2)
    K_p = ([bulk] Pi (c1 aL^2 + c2 (2 + aL^2)) + [shear] c4 (pi_XX + pi_YY + aL^2 pi_ZZ)) / 3
    N   = u.dsigma aL g Lambda^3 / (2 pi^2 hbarc^3) (N0 + K_m m^2 A0 + K_p Lambda^2 A2)
summed over the cells, times 2 y_cut in 2+1D."""
import numpy as np

from is3d_amd import synth

HBARC = synth.HBARC
VOLUME_SCALE = 1000.0
BULK_SCALE = 0.02
PI_FIELDS = ["pitt", "pitx", "pity", "pitn", "pixx", "pixy", "pixn", "piyy", "piyn", "pinn"]


def lrf_dsigma(v):
    """(u.dsigma, |dsigma_space| in the local rest frame): dsigma_mu is covariant, dsigma.dsigma = dat^2 - dax^2 - day^2 - dan^2 / tau^2"""
    tau2 = v["tau"] ** 2
    ut = np.sqrt(1.0 + v["ux"] ** 2 + v["uy"] ** 2 + tau2 * v["un"] ** 2)
    uds = ut * v["dat"] + v["ux"] * v["dax"] + v["uy"] * v["day"] + v["un"] * v["dan"]
    ds2 = v["dat"] ** 2 - v["dax"] ** 2 - v["day"] ** 2 - v["dan"] ** 2 / tau2
    return uds, np.sqrt(np.maximum(uds * uds - ds2, 0.0))


def outflow_free_cells(dim, seed, n=64):
    """n synthetic VAH cells (volumes x 1000, bulkPi x 0.02), dsigma_mu += k u_mu so that u.dsigma >= 2 |dsigma_space|: p.dsigma > 0 for every
    momentum (the shift adds nothing to the local-rest-frame spatial part)."""
    v = dict(synth.synth_vah_surface(n, dim, seed=seed))
    for f in ("dat", "dax", "day", "dan"):
        v[f] = VOLUME_SCALE * v[f]
    v["bulkPi"] = BULK_SCALE * v["bulkPi"]
    uds, dsp = lrf_dsigma(v)
    k = np.maximum(0.0, 2.0 * dsp * (1.0 + 1e-9) - uds)
    tau2 = v["tau"] ** 2
    ut = np.sqrt(1.0 + v["ux"] ** 2 + v["uy"] ** 2 + tau2 * v["un"] ** 2)
    v["dat"] = v["dat"] + k * ut
    v["dax"] = v["dax"] - k * v["ux"]
    v["day"] = v["day"] - k * v["uy"]
    v["dan"] = v["dan"] - k * tau2 * v["un"]
    uds2, dsp2 = lrf_dsigma(v)
    assert np.all(uds2 >= 2.0 * dsp2) and np.all(uds2 > 0.0)
    assert np.allclose(dsp2, dsp, rtol=1e-6, atol=1e-12)
    return {f: np.ascontiguousarray(a) for f, a in v.items()}


def shear_lrf_diagonal(v):
    """(pi_XX, pi_YY, pi_ZZ): pi_AB = A_mu B_nu pi_perp^{mu nu} on the Milne basis (X, Y, Z) of the sampler, covariant components with the
    metric (+, -, -, -tau^2)"""
    tau, ux, uy, un = v["tau"], v["ux"], v["uy"], v["un"]
    tau2 = tau * tau
    ut = np.sqrt(1.0 + ux * ux + uy * uy + tau2 * un * un)
    uperp, utperp = np.sqrt(ux * ux + uy * uy), np.sqrt(1.0 + ux * ux + uy * uy)
    sinhL, coshL = tau * un / utperp, ut / utperp
    moving = uperp > 1.0e-5
    safe = np.where(moving, uperp, 1.0)
    one, zero = np.ones_like(tau), np.zeros_like(tau)
    X = [uperp * coshL, np.where(moving, utperp * ux / safe, one), np.where(moving, utperp * uy / safe, zero), uperp * sinhL / tau]
    Y = [zero, np.where(moving, -uy / safe, zero), np.where(moving, ux / safe, one), zero]
    Z = [sinhL, zero, zero, coshL / tau]
    pi = {(0, 0): v["pitt"], (0, 1): v["pitx"], (0, 2): v["pity"], (0, 3): v["pitn"], (1, 1): v["pixx"], (1, 2): v["pixy"], (1, 3): v["pixn"],
          (2, 2): v["piyy"], (2, 3): v["piyn"], (3, 3): v["pinn"]}
    g = [one, -one, -one, -tau2]

    def quad(A):
        a = [g[m] * A[m] for m in range(4)]
        s = zero.copy()
        for m in range(4):
            for n in range(4):
                s = s + pi[(min(m, n), max(m, n))] * a[m] * a[n]
        return s

    return quad(X), quad(Y), quad(Z)


def radial_sums(root, weight, mbar, sign, dtype=np.float64):
    """(N0, A0, A2) for an array of mbar"""
    r, w = np.asarray(root, dtype=dtype)[None, :], np.asarray(weight, dtype=dtype)[None, :]
    with np.errstate(over="ignore"):
        e = np.minimum(np.exp(np.sqrt(r * r + np.asarray(mbar, dtype=dtype)[:, None] ** 2)), 1.0e300)   # held there, as the kernel holds it
    q = 1.0 / (e + sign)
    eq2 = e * q * q
    base = w * r * np.exp(r)
    return np.sum(base * q, axis=1), np.sum(base * eq2, axis=1), np.sum(base * r * r * eq2, axis=1)


def total_yield_vah_ref(v, sp, gla, opts, y_cut=0.5, coef=None, dtype=np.float64):
    """-> (mean_yield, yield_by_species, n_cells_skipped).  v: dict of VAH cell arrays; coef: dict c0..c4 in place of the cells' own; opts:
    dimension, include_bulk_deltaf, include_shear_deltaf (default 1).  dtype = np.longdouble: the same text in 80-bit arithmetic, yields
    returned in that type."""
    bulk, shear = int(opts.get("include_bulk_deltaf", 1)), int(opts.get("include_shear_deltaf", 1))
    if np.dtype(dtype) != np.float64:
        v = {k: np.asarray(a).astype(dtype) for k, a in v.items()}
        coef = None if coef is None else {k: np.asarray(a).astype(dtype) for k, a in coef.items()}
        sp = {k: np.asarray(sp[k]).astype(dtype) for k in ("mass", "sign", "degeneracy")}
    c = coef if coef is not None else v
    uds, _ = lrf_dsigma(v)
    live = uds > 0.0
    L, aL = v["Lambda"], v["aL"]
    K_m, K_p = np.zeros_like(uds), np.zeros_like(uds)
    if bulk:
        K_m = v["bulkPi"] * (c["c0"] + c["c2"])
        K_p = K_p + v["bulkPi"] * (c["c1"] * aL ** 2 + c["c2"] * (2.0 + aL ** 2))
    if shear:
        pXX, pYY, pZZ = shear_lrf_diagonal(v)
        K_p = K_p + c["c4"] * (pXX + pYY + aL ** 2 * pZZ)
    K_p = K_p / 3.0
    w = np.where(live, uds * aL * L ** 3, 0.0)
    by = np.zeros(len(sp["mass"]), dtype)
    for s, (m, sign, g) in enumerate(zip(sp["mass"], sp["sign"], sp["degeneracy"])):
        N0, A0, A2 = radial_sums(gla["root1"], gla["weight1"], m / L, sign, dtype)
        by[s] = g / dtype(2.0 * np.pi ** 2 * HBARC ** 3) * np.sum(w * (N0 + K_m * m * m * A0 + K_p * L * L * A2))
    if int(opts.get("dimension", 3)) == 2:
        by = by * (2.0 * y_cut)
    total = dtype(0.0)
    for x in by:
        total += x
    return (float(total) if np.dtype(dtype) == np.float64 else total), by, int(np.count_nonzero(~live))
