"""Test helper: a numpy restatement of EmissionFunctionArray::do_resonance_decays (emissionfunction_resonance_decays.cpp:124-2158) as that
loop reads -- parents from the last chosen species down to index 1, channel by channel, group by group, each group's integral added to the
daughter's spectrum at once -- with the divergences of DESIGN.md section 3h (switch point, partner recoil mass unless recoil="particle_2",
clamped acos).  Gauss-Legendre nodes come from numpy, not from the reference's tables, and the M_T fit from numpy's least squares: an
evaluation independent of the library's, which agrees with it to rounding and to the 14th digit of the tabulated nodes.
Spectrum layout: flat, species fastest, [n_y_eff][n_phi][n_pT][S] (n_y_eff = 1 in 2+1D)."""
import numpy as np

X12, W12 = np.polynomial.legendre.leggauss(12)
X24, W24 = np.polynomial.legendre.leggauss(24)
TWO_PI = 2.0 * np.pi


class FitError(ValueError):
    pass


def q_factor(M, m1, m2, m3):
    a, b, c, d = (M + m1) ** 2, (M - m1) ** 2, (m2 + m3) ** 2, (m2 - m3) ** 2
    s = c + (b - c) * (1.0 + X24) / 2.0
    return float(np.sum(W24 * (b - c) * np.sqrt(np.abs((a - s) * (b - s) * (s - c) * (s - d))) / (2.0 * s)))


def _entries(table):
    off = np.concatenate([[0], np.cumsum(table["n_channels"])])
    return off


def _bracket(grid, x):
    """left / right node indices of x as the reference's `while (x > grid[iR]) iR++` from iR = 1 finds them"""
    iR = np.clip(np.searchsorted(grid, x, side="left"), 1, len(grid) - 1)
    return iR - 1, iR


def _log_parent(P, MT, Phi, Y, iYL, iYR, YL, YR):
    """log dN of the parent at (MT, Phi[, Y]): dN_dYMTdMTdPhi_(non_)boost_invariant"""
    phi = P["phi"]
    inr = (Phi >= phi[0]) & (Phi <= phi[-1])
    iL, iR = _bracket(phi, np.where(inr, Phi, phi[0]))
    PL = np.where(inr, phi[iL], phi[-1] - TWO_PI)
    PR = np.where(inr, phi[iR], phi[0])
    iL = np.where(inr, iL, len(phi) - 1)
    iR = np.where(inr, iR, 0)
    Phi = np.where(inr, Phi, Phi - np.floor(Phi / np.pi) * TWO_PI)
    MTv, L, fit = P["MTv"], P["L"], P["fit"]
    below = MT <= P["MTsw"]
    iML, iMR = _bracket(MTv, np.where(below, MT, MTv[0]))
    MTL, MTR = MTv[iML], MTv[iMR]
    wPL, wPR = (PR - Phi), (Phi - PL)
    if Y is None:
        lin = ((L[0, iL, iML] * wPL + L[0, iR, iML] * wPR) * (MTR - MT) + (L[0, iL, iMR] * wPL + L[0, iR, iMR] * wPR) * (MT - MTL)) / ((PR - PL) * (MTR - MTL))
        fl = lambda i: fit[0, i, 0] + fit[0, i, 1] * MT  # noqa: E731
        ext = (fl(iL) * wPL + fl(iR) * wPR) / (PR - PL)
    else:
        wYL, wYR = (YR - Y), (Y - YL)
        Lm = lambda iM: (L[iYL, iL, iM] * wYL + L[iYR, iL, iM] * wYR) * wPL + (L[iYL, iR, iM] * wYL + L[iYR, iR, iM] * wYR) * wPR  # noqa: E731
        lin = ((MTR - MT) * Lm(iML) + (MT - MTL) * Lm(iMR)) / ((YR - YL) * (PR - PL) * (MTR - MTL))
        fl = lambda iy, i: fit[iy, i, 0] + fit[iy, i, 1] * MT  # noqa: E731
        ext = ((fl(iYL, iL) * wYL + fl(iYR, iL) * wYR) * wPL + (fl(iYL, iR) * wYL + fl(iYR, iR) * wYR) * wPR) / ((YR - YL) * (PR - PL))
    return np.where(below, lin, ext)


def _parent_state(dN4, ip, M, pT, phi, mc_id):
    """log table, M_T nodes, per-row fits and the switch M_T of parent ip with (possibly adjusted) mass M"""
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.log(dN4[:, :, :, ip])                       # [y][phi][pT]
    MTv = np.sqrt(np.abs(pT * pT + M * M))
    ny, nphi, npT = L.shape
    fit = np.zeros((ny, nphi, 2))
    kmin = npT
    for iy in range(ny):
        for j in range(nphi):
            fin = np.isfinite(L[iy, j])
            stop = npT if fin.all() else int(np.argmin(fin))
            kmin = min(kmin, stop)
            sel = np.arange(stop)
            sel = sel[MTv[sel] > np.sqrt(2.73) * M]
            if len(sel) < 2:
                raise FitError("parent %d row iy=%d iphi=%d: %d points" % (mc_id, iy, j, len(sel)))
            A = np.stack([np.ones(len(sel)), MTv[sel]], axis=1)
            fit[iy, j] = np.linalg.lstsq(A, L[iy, j, sel], rcond=None)[0]
    return dict(L=L, MTv=MTv, fit=fit, MTsw=MTv[kmin - 1], phi=phi)


def _group_integral(P, M, m1, Es, ps, sw, pT, phi, y, dim3, clamps):
    """the decay integral of one group for every (y, phi, pT) bin: [ny][nphi][npT].  Axes of the point arrays: [pT][phi][s][v][zeta]."""
    ny = len(y) if dim3 else 1
    out = np.zeros((ny, len(phi), len(pT)))
    cz = np.cos((np.pi / 2.0) * (1.0 + X12))[None, None, None, None, :]
    Ymax = abs(y[-1]) if dim3 else 0.0
    pt = pT[:, None, None, None, None]
    pT2 = pt * pt
    mT2 = pT2 + m1 * m1
    mT = np.sqrt(mT2)
    Es_, ps_ = np.asarray(Es)[None, None, :, None, None], np.asarray(ps)[None, None, :, None, None]
    DY = np.log((ps_ + np.sqrt(Es_ * Es_ + pT2)) / mT)
    v = X12[None, None, None, :, None]
    ch = np.cosh(v * DY)
    den = mT2 * ch * ch - pT2
    MTbar = Es_ * M * mT * ch / den
    DMT = M * pt * np.sqrt(np.abs(Es_ * Es_ + pT2 - mT2 * ch * ch)) / den
    vw = DY * W12[None, None, None, :, None] / np.sqrt(np.abs(den))
    MT = MTbar + DMT * cz
    PT = np.sqrt(MT * MT - M * M)
    c = (MT * (mT * ch / pt) - Es_ * M / pt) / PT
    if not dim3:   # the library counts a clamp once per (bin, point)
        clamps[0] += int(np.sum((c > 1.0) | (c < -1.0))) * len(phi)
    Pt = np.arccos(np.clip(c, -1.0, 1.0))
    w = np.asarray(sw)[None, None, :, None, None] * vw * W12[None, None, None, None, :]
    ph = phi[None, :, None, None, None]
    P1 = np.fmod(Pt + ph, TWO_PI)
    P2 = np.fmod(-Pt + ph, TWO_PI)
    P1 = np.where(P1 < 0, P1 + TWO_PI, P1)
    P2 = np.where(P2 < 0, P2 + TWO_PI, P2)
    MTb = MT + 0.0 * P1
    for iy in range(ny):
        if dim3:
            Y = y[iy] + v * DY + 0.0 * MTb
            inY = np.abs(Y) <= Ymax
            iYL, iYR = _bracket(y, np.where(inY, Y, y[0]))
            args = (np.where(inY, Y, 0.0), iYL, iYR, y[iYL], y[iYR])
        else:
            inY, args = True, (None, 0, 0, 0.0, 0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.exp(_log_parent(P, MTb, P1, *args)) + np.exp(_log_parent(P, MTb, P2, *args))
            val = np.where(inY, w * MT * f, 0.0)
        out[iy] = np.sum(val, axis=(2, 3, 4)).T
    return out


def feed_down(dN, table, chosen, pT, phi, y=None, dim3=False, recoil="partner", stats=None):
    """the fed-down copy of the flat spectrum dN (see module doc); stats (dict) receives n_parents, n_channels, n_adjusted, n_clamps"""
    S = len(chosen)
    ny = len(y) if dim3 else 1
    dN4 = np.array(dN, dtype=np.float64).reshape(ny, len(phi), len(pT), S).copy()
    ids = list(np.asarray(table["mc_id"]))
    off = _entries(table)
    entry = [ids.index(c) for c in chosen]
    st = dict(n_parents=0, n_channels=0, n_adjusted=0, n_clamps=0)
    clamps = [0]
    for ip in range(S - 1, 0, -1):
        e = entry[ip]
        if table["stable"][e]:
            continue
        st["n_parents"] += 1
        base = None
        for j in range(table["n_channels"][e]):
            c = off[e] + j
            n = abs(int(table["npart"][c]))
            prod = [ids.index(int(d)) for d in table["daughters"][c][:n]]
            if n in (1, 4):
                continue
            br = float(table["branch_ratio"][c])
            M = float(table["mass"][e])
            m = [float(table["mass"][k]) for k in prod]
            adjusted = False
            if n == 2:
                while m[0] + m[1] > M:
                    adjusted = True
                    M += 0.25 * table["width"][e]
                    m[0] -= 0.5 * table["width"][prod[0]]
                    m[1] -= 0.5 * table["width"][prod[1]]
            sel = [k for k in prod if k in entry]
            if not sel:
                continue
            st["n_channels"] += 1
            st["n_adjusted"] += adjusted
            groups = []
            for k in sel:
                for g in groups:
                    if g[0] == k:
                        g[1] += 1
                        break
                else:
                    groups.append([k, 1])
            if base is None:
                base = dN4.copy()
            P = _parent_state(base, ip, M, pT, phi, int(table["mc_id"][e]))
            for k, mult in groups:
                rest = list(prod)
                i1 = rest.index(k)
                del rest[i1]
                if n == 2:
                    m1 = m[i1]
                    m2 = float(table["mass"][prod[1]]) if recoil == "particle_2" else m[1 - i1]
                    Es = (M * M + m1 * m1 - m2 * m2) / (2.0 * M)
                    ps = np.sqrt(Es * Es - m1 * m1)
                    pref = mult * M * br / (8.0 * ps)
                    I = _group_integral(P, M, m1, [Es], [ps], [1.0], pT, phi, y, dim3, clamps)
                else:
                    m1 = m[i1]
                    m2, m3 = [float(table["mass"][r]) for r in rest]
                    sp, sm, d = (M - m1) ** 2, (m2 + m3) ** 2, (m2 - m3) ** 2
                    s = sm + (sp - sm) * (1.0 + X12) / 2.0
                    Es = (M * M + m1 * m1 - s) / (2.0 * M)
                    ps = np.sqrt(Es * Es - m1 * m1)
                    sw = W12 * np.sqrt(np.abs((s - sm) * (s - d))) / s
                    pref = mult * M * M * (sp - sm) * br / (8.0 * q_factor(M, m1, m2, m3))
                    I = _group_integral(P, M, m1, Es, ps, sw, pT, phi, y, dim3, clamps)
                dN4[:, :, :, entry.index(k)] += pref * I
    st["n_clamps"] = clamps[0]
    if stats is not None:
        stats.update(st)
    return dN4.reshape(-1)
