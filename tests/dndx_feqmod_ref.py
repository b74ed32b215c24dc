"""A numpy restatement of EmissionFunctionArray::calculate_dN_dX_feqmod (emissionfunction_smooth_kernels.cpp:1449-2135), per cell: dN_dy_cell
and the 2+1D dN/dy deta partials of operation 0 with the modified equilibrium (df_mode 3, 4).  The coefficients come from the oracle's
exported helpers (df_coefficients, df_coefficients_bilinear, jonah_tables, cspline_*); the rest is written out here.

Where it follows calculate_dN_dX_feqmod and not the spectra routine calculate_dN_ptdptdphidy_feqmod:
  - no narrow-row fallback in 3+1D (:1926-1934 is commented out);
  - 2+1D: eta_scale = detA whenever detA > deta_min (:1847-1849), no upper bound;
  - the nan / inf test is on renorm / detA in both dimensions (:1881), before the breakdown branch;
  - bulkPi regulation with <= / >= (:1708-1712); p.dsigma = w_eta (pt dat + px dax + py day + pn dan) in both branches (:1943, :2010).

dtype = np.longdouble (include_baryon = 0) restates the same text in 80-bit arithmetic for tests/golden/make_golden_extreme_op0.py: the
coefficients then come from scipy's natural splines (make_golden.coefficients_scipy) and the long-double lambda / z tables
(make_golden.jonah_tables_ld), the matrix inverse from a Newton-Schulz polish of the double one; the exponent, the matrix, p.dsigma and the
sums stay the lines below.  The double form (the default) is what it was, operation for operation.
"""
import numpy as np

from oracle import oracle

HBARC = 0.197327053


def _gt(kind, r, w, mbar, sign, chem=0.0, ft=float):
    """GaussThermal integrands neq_int, J10_int, J20_int; mbar, sign, chem: [S] (or scalars)"""
    mb = np.atleast_1d(np.asarray(mbar, dtype=ft))[:, None]
    sg = np.broadcast_to(np.atleast_1d(np.asarray(sign, dtype=ft)), mb.shape[:1])[:, None]
    ch = np.broadcast_to(np.atleast_1d(np.asarray(chem, dtype=ft)), mb.shape[:1])[:, None]
    Eb = np.sqrt(r[None, :] ** 2 + mb ** 2)
    q = np.exp(Eb - ch) + sg
    if kind == "neq":
        v = r[None, :] * np.exp(r[None, :]) / q
    elif kind == "J10":
        v = r[None, :] * np.exp(r[None, :] + Eb - ch) / (q * q)
    else:
        v = Eb * np.exp(r[None, :] + Eb - ch) / (q * q)
    return np.sum(w[None, :] * v, axis=1)


class Jonah:
    def __init__(self, fq):
        l2, z, bp, self.bp_max = oracle.jonah_tables(fq)
        self.bp, self.l2, self.z = bp, l2, z
        self.cl, self.cz = oracle.cspline_init(bp, l2), oracle.cspline_init(bp, z)

    def __call__(self, r):
        return oracle.cspline_eval(self.bp, self.l2, self.cl, r), oracle.cspline_eval(self.bp, self.z, self.cz, r)


def _golden():
    import os
    import sys
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if here not in sys.path:
        sys.path.insert(0, here)
    import make_golden
    return make_golden


class JonahLD:
    """Jonah for dtype = np.longdouble: the long-double tables, scipy's natural splines"""

    def __init__(self, fq):
        from scipy.interpolate import CubicSpline
        l2, z, bp = _golden().jonah_tables_ld(fq)
        self.bp_max = float(np.max(bp))
        self.sl, self.sz = CubicSpline(bp, l2, bc_type="natural"), CubicSpline(bp, z, bc_type="natural")

    def __call__(self, r):
        return np.longdouble(float(self.sl(float(r)))), np.longdouble(float(self.sz(float(r))))


def _inverse(A, ft):
    if ft is float:
        return np.linalg.inv(A)
    Ai = np.linalg.inv(A.astype(np.float64)).astype(ft)
    for _ in range(3):                  # Newton-Schulz polish, as make_golden.highprec_feqmod
        Ai = Ai @ (2 * np.eye(3, dtype=ft) - A @ Ai)
    return Ai


def cell_dndx(cells, c, sp, grid, df, fq, opts, jonah=None, dtype=np.float64, per_node=False):
    """-> (dN_dy_cell [S], eta partials [S][n_eta] (2+1D, already / w_eta; None in 3+1D), breakdown (bool), skipped [S] (bool: the renorm test),
    detA (nan for a skipped cell)).  per_node: pT_w is not read and the first two carry a pT axis, [S][n_pT] and [S][n_pT][n_eta]."""
    ft = float if np.dtype(dtype) == np.float64 else np.longdouble
    dim, dfm = int(opts["dimension"]), int(opts["df_mode"])
    outflow = opts.get("outflow", 1)
    regulate = opts.get("regulate_deltaf", 1)
    inc_bulk, inc_shear = opts.get("include_bulk_deltaf", 1), opts.get("include_shear_deltaf", 1)
    baryon_on = opts.get("include_baryon", 0)
    diff_on = baryon_on and opts.get("include_baryondiff_deltaf", 0)
    mass, sign, gdeg = (np.asarray(sp[k], dtype=ft) for k in ("mass", "sign", "degeneracy"))
    bnum = np.asarray(sp["baryon"], dtype=ft) if baryon_on else np.zeros_like(mass)
    S = len(mass)
    pT, phi = np.asarray(grid["pT"], ft), np.asarray(grid["phi"], float)      # the reference forms cos / sin in double
    pT_w, phi_w = (None if per_node else np.asarray(grid["pT_w"], ft)), np.asarray(grid["phi_w"], ft)
    prefactor = ft(2.0 * np.pi * HBARC) ** -3
    two_pi2_hbarC3 = ft(2.0 * np.pi ** 2 * HBARC ** 3)
    f = {k: ft(cells[k][c]) for k in cells if cells[k] is not None and k not in ("x", "y")}
    tau, tau2 = f["tau"], f["tau"] ** 2
    ux, uy, un = f["ux"], f["uy"], f["un"]
    ut = np.sqrt(1.0 + ux * ux + uy * uy + tau2 * un * un)
    dat, dax, day, dan = f["dat"], f["dax"], f["day"], f["dan"]
    neta = 1 if dim == 3 else len(grid["eta"])
    head = (S, len(pT)) if per_node else (S,)
    zero = (np.zeros(head, ft), None if dim == 3 else np.zeros(head + (neta,), ft), False, np.zeros(S, bool), float("nan"))
    if not (ut * dat + ux * dax + uy * day + un * dan > 0.0):
        return zero
    uperp, utperp = np.sqrt(ux * ux + uy * uy), np.sqrt(1.0 + ux * ux + uy * uy)
    T, P, E = f["T"], f["P"], f["E"]
    pitt = pitx = pity = pitn = pixx = pixy = pixn = piyy = piyn = pinn = 0.0
    if inc_shear:
        pixx, pixy, pixn, piyy, piyn = f["pixx"], f["pixy"], f["pixn"], f["piyy"], f["piyn"]
        pinn = (pixx * (ux * ux - ut * ut) + piyy * (uy * uy - ut * ut) + 2.0 * (pixy * ux * uy + tau2 * un * (pixn * ux + piyn * uy))) / (tau2 * utperp * utperp)
        pitn = (pixn * ux + piyn * uy + tau2 * pinn * un) / ut
        pity = (pixy * ux + piyy * uy + tau2 * piyn * un) / ut
        pitx = (pixx * ux + pixy * uy + tau2 * pixn * un) / ut
        pitt = (pitx * ux + pity * uy + tau2 * pitn * un) / ut
    bulkPi = f["bulkPi"] if inc_bulk else 0.0
    muB = nB = Vx = Vy = Vn = Vt = alphaB = ber = 0.0
    if diff_on:
        muB, nB, Vx, Vy, Vn = f["muB"], f["nB"], f["Vx"], f["Vy"], f["Vn"]
        Vt = (Vx * ux + Vy * uy + tau2 * Vn * un) / ut
        alphaB = muB / T
        ber = nB / (E + P)
    lam = z = 0.0
    if dfm == 4:
        jonah = jonah or (Jonah(fq) if ft is float else JonahLD(fq))
        if bulkPi <= -P:
            bulkPi = -(1.0 - 1.e-5) * P
        elif bulkPi / P >= jonah.bp_max:
            bulkPi = P * (jonah.bp_max - 1.e-5)
        l2, z = jonah(bulkPi / P)
        lam = -np.sqrt(l2) if bulkPi < 0 else (np.sqrt(l2) if bulkPi > 0 else 0.0)
    if baryon_on:
        co = oracle.df_coefficients_bilinear(df, 2, T, muB)
        F, G, betabulk, betaV, betapi = co["F"], co["G"], co["betabulk"], co["betaV"], co["betapi"]
    elif ft is float:
        co = oracle.df_coefficients(df, 2, T)
        F, G, betabulk, betaV, betapi = co["F"], 0.0, co["betabulk"], 1.0, co["betapi"]
    else:
        co = _golden().coefficients_scipy(df, 2, float(T))
        F, G, betabulk, betaV, betapi = ft(co["F"]), 0.0, ft(co["betabulk"]), 1.0, ft(co["betapi"])
    delta_lambda = bulkPi / (5.0 * betapi - 3.0 * P * (E + P) / E)
    delta_z = -3.0 * delta_lambda * P / E
    # Milne_Basis, boost_pimunu_to_lrf (viscous_correction.cpp)
    sinhL, coshL = tau * un / utperp, ut / utperp
    Xt, Zt, Xn, Zn = uperp * coshL, sinhL, uperp * sinhL / tau, coshL / tau
    Xx, Yx, Xy, Yy = 1.0, 0.0, 0.0, 1.0
    if uperp > 1.e-5:
        Xx, Yx, Xy, Yy = utperp * ux / uperp, -uy / uperp, utperp * uy / uperp, ux / uperp
    pixx_L = pitt * Xt * Xt + pixx * Xx * Xx + piyy * Xy * Xy + tau2 * tau2 * pinn * Xn * Xn \
        + 2.0 * (-Xt * (pitx * Xx + pity * Xy) + pixy * Xx * Xy + tau2 * Xn * (pixn * Xx + piyn * Xy - pitn * Xt))
    pixy_L = Yx * (-pitx * Xt + pixx * Xx + pixy * Xy + tau2 * pixn * Xn) + Yy * (-pity * Xt + pixy * Xx + piyy * Xy + tau2 * piyn * Xn)
    pixz_L = Zt * (pitt * Xt - pitx * Xx - pity * Xy - tau2 * pitn * Xn) - tau2 * Zn * (pitn * Xt - pixn * Xx - piyn * Xy - tau2 * pinn * Xn)
    piyy_L = pixx * Yx * Yx + 2.0 * pixy * Yx * Yy + piyy * Yy * Yy
    piyz_L = -Zt * (pitx * Yx + pity * Yy) + tau2 * Zn * (pixn * Yx + piyn * Yy)
    pizz_L = -(pixx_L + piyy_L)
    T_mod, alphaB_mod = T, alphaB
    if dfm == 3:
        T_mod = T + bulkPi * F / betabulk
        alphaB_mod = alphaB + bulkPi * G / betabulk
    shear_mod = 0.5 / betapi
    bulk_mod = lam if dfm == 4 else bulkPi / (3.0 * betabulk)
    A = np.array([[1.0 + pixx_L * shear_mod + bulk_mod, pixy_L * shear_mod, pixz_L * shear_mod],
                  [pixy_L * shear_mod, 1.0 + piyy_L * shear_mod + bulk_mod, piyz_L * shear_mod],
                  [pixz_L * shear_mod, piyz_L * shear_mod, 1.0 + pizz_L * shear_mod + bulk_mod]])
    detA = A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] ** 2) - A[0, 1] * (A[0, 1] * A[2, 2] - A[1, 2] * A[0, 2]) + A[0, 2] * (A[0, 1] * A[1, 2] - A[1, 1] * A[0, 2])
    r1, w1, r2, w2 = (np.asarray(fq[k], ft) for k in ("root1", "weight1", "root2", "weight2"))
    neq_fact = T ** 3 / two_pi2_hbarC3
    breakdown = False
    if dfm == 3:   # does_feqmod_breakdown (emissionfunction.cpp:109-150)
        mbp = fq["mass_pion0"] / T
        neq0 = neq_fact * _gt("neq", r1, w1, mbp, -1.0, ft=ft)[0]
        J200 = T * neq_fact * _gt("J20", r2, w2, mbp, -1.0, ft=ft)[0]
        dn0 = bulkPi * (neq0 + J200 * F / T / T) / betabulk
        breakdown = bool(detA <= fq["deta_min"] or (neq0 + dn0) < 0.0)
    eta_scale = detA if (detA > fq["deta_min"] and dim == 2) else 1.0
    renorm = np.ones(S, ft)
    if inc_bulk:
        if dfm == 3:
            mbar, mbm = mass / T, mass / T_mod
            neq = neq_fact * _gt("neq", r1, w1, mbar, sign, bnum * alphaB, ft=ft)
            N10 = bnum * neq_fact * _gt("J10", r1, w1, mbar, sign, bnum * alphaB, ft=ft)
            J20 = T * neq_fact * _gt("J20", r2, w2, mbar, sign, bnum * alphaB, ft=ft)
            n_lin = neq + (bulkPi / betabulk) * (neq + N10 * G + J20 * F / T / T)
            with np.errstate(all="ignore"):
                n_mod = (T_mod ** 3 / two_pi2_hbarC3) * _gt("neq", r1, w1, mbm, sign, bnum * alphaB_mod, ft=ft)
                renorm = n_lin / n_mod
        else:
            renorm = np.full(S, z, ft)
    with np.errstate(all="ignore"):
        q = renorm / detA
    skipped = ~np.isfinite(q.astype(np.float64))          # (the reference's test is on a double)
    if dim == 3:
        renorm = q
    # momentum grid: axes (k: y | eta, j: phi, p: pT, s)
    if dim == 3:
        ys, etas, ws = np.asarray(grid["y"], ft), np.array([f["eta"]]), np.array([1.0], ft)
        dlt = ys - etas[0]
    else:
        etas, ws = np.asarray(grid["eta"], ft), np.asarray(grid["eta_w"], ft)
        dlt = 0.0 - (etas if breakdown else eta_scale * etas)
    mT = np.sqrt(mass[None, :] ** 2 + pT[:, None] ** 2)                      # [p][s]
    ch, sh = np.cosh(dlt)[:, None, None, None], np.sinh(dlt)[:, None, None, None]
    w = (ws if dim == 2 else np.ones(len(dlt), ft))[:, None, None, None]
    pt, pn = mT[None, None] * ch, (mT[None, None] / tau) * sh
    t2pn = tau2 * pn
    px = (pT[None, :] * np.cos(phi)[:, None])[None, :, :, None]
    py = (pT[None, :] * np.sin(phi)[:, None])[None, :, :, None]
    pds = w * (pt * dat + px * dax + py * day + pn * dan)
    m2 = (mass ** 2)[None, None, None, :]
    with np.errstate(all="ignore"):
        if breakdown:
            pdotu = pt * ut - px * ux - py * uy - t2pn * un
            pimunu = pitt * pt * pt + pixx * px * px + piyy * py * py + pinn * t2pn * t2pn \
                + 2.0 * (-(pitx * px + pity * py) * pt + pixy * px * py + t2pn * (pixn * px + piyn * py - pitn * pt))
            feq = 1.0 / (np.exp(pdotu / T - bnum * alphaB) + sign)
            feqbar = 1.0 - sign * feq
            Vp = Vt * pt - Vx * px - Vy * py - Vn * t2pn
            df_shear = (0.5 / (betapi * T)) * pimunu / pdotu
            df_bulk = ((F / (T * T * betabulk)) * pdotu + (G / betabulk) * bnum + (1.0 / (3.0 * T * betabulk)) * (pdotu - m2 / pdotu)) * bulkPi
            df_diff = (ber - bnum / pdotu) * Vp / betaV
            dfv = feqbar * (df_shear + df_bulk + df_diff)
            if regulate:
                dfv = np.clip(dfv, -1.0, 1.0)
            fv = feq * (1.0 + dfv)
        else:
            pL = [-Xt * pt + Xx * px + Xy * py + Xn * t2pn, Yx * px + Yy * py + 0.0 * pt, -Zt * pt + Zn * t2pn]
            Ai = _inverse(A, ft)
            pm = [Ai[i, 0] * pL[0] + Ai[i, 1] * pL[1] + Ai[i, 2] * pL[2] for i in range(3)]
            Emod = np.sqrt(m2 + pm[0] ** 2 + pm[1] ** 2 + pm[2] ** 2)
            fv = np.abs(renorm)[None, None, None, :] / (np.exp(Emod / T_mod - bnum * alphaB_mod) + sign)
        term = pds * fv
    if outflow:
        term = np.where(pds <= 0.0, 0.0, term)
    term = np.where(skipped[None, None, None, :], 0.0, term)
    if per_node:
        red = np.einsum("kjps,j->kps", term, phi_w)                              # [k][p][s]
        cell = prefactor * gdeg[:, None] * red.sum(axis=0).T
        eta = None if dim == 3 else (prefactor * gdeg[:, None, None] * red.transpose(2, 1, 0) / ws[None, None, :])
        return cell, eta, breakdown, skipped, float(detA)
    red = np.einsum("kjps,p,j->ks", term, pT_w, phi_w)                           # [k][s]
    cell = prefactor * gdeg * red.sum(axis=0)
    eta = None if dim == 3 else (prefactor * gdeg[:, None] * red.T / ws[None, :])
    return cell, eta, breakdown, skipped, float(detA)


def dndx(cells, sp, grid, df, fq, opts, idx=None):
    """-> dict per_cell [S][n], eta [S][n_eta] (2+1D sums over the cells), n_breakdown, skipped [n][S]"""
    n = len(cells["tau"])
    idx = range(n) if idx is None else idx
    jonah = Jonah(fq) if int(opts["df_mode"]) == 4 else None
    S = len(sp["mass"])
    per, skip, nb = np.zeros((S, len(idx))), np.zeros((len(idx), S), bool), 0
    eta = None if int(opts["dimension"]) == 3 else np.zeros((S, len(grid["eta"])))
    for i, c in enumerate(idx):
        v, e, b, s, _ = cell_dndx(cells, c, sp, grid, df, fq, opts, jonah)
        per[:, i], skip[i], nb = v, s, nb + int(b)
        if eta is not None:
            eta += e
    return dict(per_cell=per, eta=eta, n_breakdown=nb, skipped=skip)
