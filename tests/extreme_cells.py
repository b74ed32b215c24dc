"""Extreme freezeout cells for the three momentum-spectrum families (delta-f: cf_kernels.hip; modified equilibrium: cf_feqmod.hip; anisotropic
hydro: cf_vah.hip): a seeded table of transformations of the NON-dsigma fields of synth.synth_surface / synth_vah_surface -- flow, temperature,
viscous stress, rapidity, proper time, the anisotropy variables, mu_B -- that take them out of the box every synthetic draw sits in (gamma <= 1.2,
T in [0.140, 0.160], pi ~ 2 % of E + P, |eta| <= 4, tau in [1, 10], alpha_L in [0.7, 1.2]).  tests/hostile_surfaces.py does the same for dsigma.
Pure numpy; tests/golden/make_golden_extreme.py evaluates the long-double restatements on every case and commits cells and spectra
(tests/golden/golden_extreme.npz, .json), tests/test_extreme_cells.py checks table and fixture on the CPU, tests/test_gpu_extreme_cells.py runs
the device against the fixture.  Operation 0 runs on the same committed cells (op0_weights, op0_grid, op0_bins, fixture_op0 below;
tests/extreme_cells_op0.py), and so do mode 5 (tests/test_extreme_polarization.py) and the VAH mean yield (tests/test_extreme_yield_vah.py).

Case            transformation (u = a uniform draw in [0.05, 1), one per cell; dsigma is never touched but where stated)
fast-flow       transverse rapidity uniform in [1.0, 3.7] (gamma to 20), azimuth uniform and independent of the cell's position; 3+1D:
                un = sinh(D) sqrt(1 + ux^2 + uy^2) / tau with D uniform in [-2, 2]
table-edge-T    T = T_first + 1e-3 u (even cells), T_last - 1e-3 u (odd cells); E, P and the stresses keep the size they had at T ~ 0.15, so
                the cold cells carry stresses far beyond their coefficients: breakdown cells of df_mode 3
large-stress    pixx, pixy, pixn, piyy, piyn times 25; bulkPi = -0.9 P (even cells), +0.5 P (odd cells); VAH: also Wx, Wy times 8
far-eta         (3+1D) |eta| uniform in [4, 7], random sign; un is the synthetic one for the new eta
tau-extremes    tau = 0.05 (1 + 0.1 u) (even cells), 50 (1 + 0.1 u) (odd cells); un, dan, pixn, piyn keep their values, so tau un and
                tau pixn leave their range as well
isothermal-mix  T = 0.151 but for three corona cells (CORONA) at 0.101 / 0.199 / 0.101; every fifth cell (0, 5, ..) has all four dsigma components
                negated (u.dsigma <= 0: skipped); 3+1D: eta from a plateau |eta| < 2.5 (70 %) plus Gaussian tails 2.5 + 1.3 |N(0,1)| cut at 6;
                cells 1, 4, 7, .. fly as in fast-flow; the five pi components and bulkPi times a log-uniform factor in [1, 25] (VAH: Wx, Wy
                times min(factor, 8))
anisotropy      (VAH) alpha_L uniform in [0.2, 2.0], Lambda / hbarc uniform in [0.6, 1.25] fm^-1: the whole df_vah table; cells 0, 1 within
                1e-3 of the lower end of both axes, cells 2, 3 within 1e-3 of the upper end
muB-edge        (include_baryon = 1) mu_B = 0 (even cells), mu_B,last - 1e-3 u (odd cells); nB, Vx, Vy, Vn times 10

NARROW (3+1D, table-edge-T and large-stress): two cells, one per prep batch, take the recipe of tests/test_gpu_feqmod.py::test_feqmod_narrow_rows
after the case's transformation -- the five pi components back to 0.05 of the synthetic ones, bulkPi = -0.95 P, eta = a y node + 1e-4 -- so that
df_mode 4 has 0 < detA < 0.01 and a row with |y - eta| < detA: the narrow-row window of smooth_kernels.cpp:811-819.  No seed would put a
random eta within 0.01 of a y node.

After every change of flow or stress the dependent components of a VAH cell (pitt, pitx, pity, pitn, pinn) are recomputed the way
synth.synth_vah_surface does it.  exact_nodes(): two cells with T exactly ON the first and the last node of the coefficient table.

One grid: 9 phi (one 8-wide tile and one more; seeded as hostile_surfaces.grid("offtile")), 8 y on [-5, 5] (one 7-row block and one more row),
6 pT log-spaced from 0.05 to 40 GeV, the shipped eta nodes for 2+1D.  Species: hostile_surfaces.species()."""
from functools import lru_cache

import numpy as np

import hostile_surfaces as H
from is3d_amd import inputs, synth

N_CELLS = 36          # as tests/hostile_surfaces.py: two 3+1D prep batches of 16 and a tail, past the first threshold refresh at 7 cells
CASES = ("fast-flow", "table-edge-T", "large-stress", "far-eta", "tau-extremes", "isothermal-mix", "anisotropy", "muB-edge")
VISCOUS_CASES = ("fast-flow", "table-edge-T", "large-stress", "far-eta", "tau-extremes", "isothermal-mix")     # delta-f and modified equilibrium
VAH_CASES = ("fast-flow", "large-stress", "far-eta", "tau-extremes", "isothermal-mix", "anisotropy")          # (T does not enter the VAH kernel)
BARYON_CASES = ("muB-edge",)
DIMS = {c: ((3,) if c == "far-eta" else (3, 2)) for c in CASES}
# tuned on the CPU (tests/test_extreme_cells.py) until the oracle alone meets the conditions of that file
SEEDS = {"fast-flow": 6101, "table-edge-T": 6102, "large-stress": 6103, "far-eta": 6104, "tau-extremes": 6105, "isothermal-mix": 6130,
         "anisotropy": 6107, "muB-edge": 6108}
PI5 = ("pixx", "pixy", "pixn", "piyy", "piyn")
STRESS, STRESS_W = 25.0, 8.0
CORONA = {4: 0.101, 17: 0.199, 30: 0.101}
T_ISO = 0.151
NARROW = (11, 29)
NARROW_CASES = ("table-edge-T", "large-stress")
HBARC = synth.HBARC

species = H.species
species_ids = H.species_ids
live = H.live


@lru_cache(maxsize=None)
def grid():
    g = inputs.grid()
    J, K, n_pT = 9, 8, 6
    rng = np.random.default_rng(1000 * J + 10 * K + n_pT)
    out = dict(pT=np.geomspace(0.05, 40.0, n_pT), phi=np.sort(rng.random(J) * 2 * np.pi), y=np.linspace(-5.0, 5.0, K), eta=g["eta"], eta_w=g["eta_w"])
    for v in out.values():
        v.setflags(write=False)
    return out


def table_T():
    T = inputs.df_tables()["T"]
    return float(T[0]), float(T[-1])


def _dependents(c):
    """pinn, pitn, pity, pitx, pitt of a VAH cell from the five independent components and the flow (synth.synth_vah_surface)"""
    if "pitt" not in c:
        return
    tau, ux, uy, un = c["tau"], c["ux"], c["uy"], c["un"]
    tau2 = tau * tau
    ut = np.sqrt(1.0 + ux * ux + uy * uy + tau2 * un * un)
    utperp2 = 1.0 + ux * ux + uy * uy
    pixx, pixy, pixn, piyy, piyn = (c[k] for k in PI5)
    pinn = (pixx * (ux * ux - ut * ut) + piyy * (uy * uy - ut * ut) + 2.0 * (pixy * ux * uy + tau2 * un * (pixn * ux + piyn * uy))) / (tau2 * utperp2)
    pitn = (pixn * ux + piyn * uy + tau2 * pinn * un) / ut
    pity = (pixy * ux + piyy * uy + tau2 * piyn * un) / ut
    pitx = (pixx * ux + pixy * uy + tau2 * pixn * un) / ut
    pitt = (pitx * ux + pity * uy + tau2 * pitn * un) / ut
    c.update(pinn=pinn, pitn=pitn, pity=pity, pitx=pitx, pitt=pitt)


def _fly(c, idx, rng, dim):
    n = len(idx)
    rho, az = rng.uniform(1.0, 3.7, n), rng.uniform(0.0, 2.0 * np.pi, n)
    c["ux"][idx] = np.sinh(rho) * np.cos(az)
    c["uy"][idx] = np.sinh(rho) * np.sin(az)
    if dim == 3:
        d = rng.uniform(-2.0, 2.0, n)
        c["un"][idx] = np.sinh(d) * np.sqrt(1.0 + c["ux"][idx] ** 2 + c["uy"][idx] ** 2) / c["tau"][idx]


def transform(cells, case, dim, seed):
    """a copy of `cells` (a synthetic surface) with the case's transformation applied"""
    c = {k: np.array(v, dtype=np.float64, copy=True) for k, v in cells.items()}
    n = len(c["tau"])
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.05, 1.0, n)
    even, odd = np.arange(0, n, 2), np.arange(1, n, 2)
    if case == "fast-flow":
        _fly(c, np.arange(n), rng, dim)
    elif case == "table-edge-T":
        T0, T1 = table_T()
        c["T"][even] = T0 + 1e-3 * u[even]
        c["T"][odd] = T1 - 1e-3 * u[odd]
    elif case == "large-stress":
        for k in PI5:
            c[k] = STRESS * c[k]
        c["bulkPi"][even] = -0.9 * c["P"][even]
        c["bulkPi"][odd] = 0.5 * c["P"][odd]
        if "Wx" in c:
            c["Wx"], c["Wy"] = STRESS_W * c["Wx"], STRESS_W * c["Wy"]
    elif case == "far-eta":
        if dim != 3:
            raise ValueError("far-eta is a 3+1D case")
        c["eta"] = rng.choice([-1.0, 1.0], n) * rng.uniform(4.0, 7.0, n)
        c["un"] = 0.05 * np.tanh(c["eta"]) / c["tau"]
    elif case == "tau-extremes":
        c["tau"][even] = 0.05 * (1.0 + 0.1 * u[even])
        c["tau"][odd] = 50.0 * (1.0 + 0.1 * u[odd])
    elif case == "isothermal-mix":
        c["T"][:] = T_ISO
        for i, t in CORONA.items():
            c["T"][i] = t
        for f in H.DS:
            c[f][0::5] = -c[f][0::5]
        if dim == 3:
            plateau = rng.random(n) < 0.7
            tails = rng.choice([-1.0, 1.0], n) * np.minimum(2.5 + 1.3 * np.abs(rng.standard_normal(n)), 6.0)
            c["eta"] = np.where(plateau, rng.uniform(-2.5, 2.5, n), tails)
            c["un"] = 0.05 * np.tanh(c["eta"]) / c["tau"]
        _fly(c, np.arange(1, n, 3), rng, dim)
        f = np.exp(rng.uniform(0.0, np.log(STRESS), n))
        for k in PI5 + ("bulkPi",):
            c[k] = f * c[k]
        if "Wx" in c:
            c["Wx"], c["Wy"] = np.minimum(f, STRESS_W) * c["Wx"], np.minimum(f, STRESS_W) * c["Wy"]
    elif case == "anisotropy":
        if "aL" not in c:
            raise ValueError("anisotropy is a VAH case")
        tab = inputs.vah_df_tables()
        a0, a1, l0, l1 = float(tab["aL"][0]), float(tab["aL"][-1]), float(tab["L"][0]), float(tab["L"][-1])
        aL, L = rng.uniform(a0, a1, n), rng.uniform(l0, l1, n)
        aL[:2], L[:2] = a0 + 1e-3 * u[:2], l0 + 1e-3 * u[:2]
        aL[2:4], L[2:4] = a1 - 1e-3 * u[2:4], l1 - 1e-3 * u[2:4]
        c["aL"], c["Lambda"] = aL, L * HBARC
    elif case == "muB-edge":
        if "muB" not in c:
            raise ValueError("muB-edge is an include_baryon = 1 case")
        last = float(inputs.df_tables_full()["muB"][-1])
        c["muB"][even] = 0.0
        c["muB"][odd] = last - 1e-3 * u[odd]
        for k in ("nB", "Vx", "Vy", "Vn"):
            c[k] = 10.0 * c[k]
    else:
        raise ValueError(case)
    if dim == 3 and case in NARROW_CASES and "aL" not in c:
        y = grid()["y"]
        for j, i in enumerate(NARROW):
            for k in PI5:
                c[k][i] = 0.05 * cells[k][i]
            c["bulkPi"][i] = -0.95 * c["P"][i]
            c["eta"][i] = y[(3 + 2 * j) % len(y)] + 1.0e-4
    _dependents(c)
    return c


@lru_cache(maxsize=None)
def _surface(case, dim, vah, baryon):
    c = transform(H.base(dim, vah, baryon, seed=6100), case, dim, SEEDS[case] + 10 * dim)
    for v in c.values():
        v.setflags(write=False)
    return c


def surface(case, dim, vah=False, baryon=False):
    """the case's surface (read-only arrays, shared)"""
    return _surface(case, dim, bool(vah), bool(baryon))


def expected_skipped(case):
    """the cells the construction turns against the flow"""
    return list(range(0, N_CELLS, 5)) if case == "isothermal-mix" else []


def exact_nodes(dim):
    """two cells with T exactly on the first and on the last node of the coefficient table"""
    c = {k: np.array(v[:2], copy=True) for k, v in H.base(dim, seed=6100).items()}
    c["T"][:] = table_T()
    return c


# ---- the committed fixtures (tests/golden/make_golden_extreme.py, make_golden_extreme_op0.py) ----
def _load(stem):
    """(arrays of tests/golden/<stem>.npz, read-only; the dict of <stem>.json)"""
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with np.load(os.path.join(here, stem + ".npz")) as z:
        arrays = {k: z[k] for k in z.files}
    for v in arrays.values():
        v.setflags(write=False)
    with open(os.path.join(here, stem + ".json")) as f:
        return arrays, json.load(f)


@lru_cache(maxsize=None)
def fixture():
    """(arrays of golden_extreme.npz, read-only; the dict of golden_extreme.json)"""
    return _load("golden_extreme")


def fixture_cases(family=None):
    return [c for c in fixture()[1]["cases"] if family is None or c["family"] == family]


# ---- operation 0 on the same cells (tests/golden/make_golden_extreme_op0.py) ----
ETA_NODES = (0, 60, 120, 180, 240)        # the 2+1D dN/dy deta partials that are committed
PT_W_NAMES = ("ones",) + tuple("e%d" % i for i in range(6))


@lru_cache(maxsize=None)
def op0_weights():
    """(phi_w [9], a seeded positive vector; {name: pT_w [6]}: all ones and the six unit vectors -- with e_i, dN_dy_cell is the (phi, y | eta) sum
    of a cell at pT node i alone, so that a high node cannot hide behind the low ones; a zero weight is an ordinary input)"""
    phi_w = np.random.default_rng(6200).uniform(0.5, 1.5, len(grid()["phi"]))
    pT_w = {"ones": np.ones(6)}
    pT_w.update({"e%d" % i: np.eye(6)[i] for i in range(6)})
    for v in (phi_w,) + tuple(pT_w.values()):
        v.setflags(write=False)
    return phi_w, pT_w


PT_PAD = (0.5, 1.0, 2.0)


def op0_grid(name, padded=False):
    """the grid with the reduction weights of the pT weight vector `name`.  padded: three more pT nodes (PT_PAD) of weight zero behind the six,
    which leave every dN_dy_cell and dN_dydeta what it is: the 2+1D modified-equilibrium kernel keeps 48 KiB of LDS for its eta rows, [4 waves]
    [64 / npTp classes][241] doubles, and refuses 6 pT x 241 eta (npTp = 8: 61 KiB; tests/test_spacetime_checks_shared.py pins that refusal),
    while 9 pT values (npTp = 16: 31 KiB) fit"""
    g = dict(grid(), phi_w=op0_weights()[0], pT_w=op0_weights()[1][name])
    if padded:
        g.update(pT=np.append(g["pT"], PT_PAD), pT_w=np.append(g["pT_w"], np.zeros(len(PT_PAD))))
    return g


def op0_bins(cells_xy):
    """tau bins that leave the cells of tau-extremes (0.05 / 50) outside on both sides, and the slowest and the fastest of every other case; r
    bins that end inside the surface"""
    r = np.sqrt(cells_xy["x"] ** 2 + cells_xy["y"] ** 2)
    return dict(tau_min=1.5, tau_max=8.0, tau_bins=5, r_min=0.0, r_max=0.8 * float(r.max()), r_bins=4)


@lru_cache(maxsize=None)
def fixture_op0():
    """(arrays of golden_extreme_op0.npz: per case key D [S][6][36], per 2+1D key also <key>_eta [S][5]; the dict of golden_extreme_op0.json)"""
    return _load("golden_extreme_op0")


def fixture_op0_cases(family=None):
    return [c for c in fixture_op0()[1]["cases"] if family is None or c["family"] == family]


def fixture_cells(tag):
    """the committed cells of a case entry's `cells` tag as a dict of arrays"""
    fields = synth.VAH_FIELDS if tag.endswith("v") else synth.CELL_FIELDS + (synth.BARYON_FIELDS if tag.endswith("b") else [])
    a = fixture()[0]["cells_" + tag]
    assert a.shape == (len(fields), N_CELLS)
    return {k: a[i] for i, k in enumerate(fields)}
