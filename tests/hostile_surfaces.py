"""Hostile freezeout surfaces for the p.dsigma power-of-two scales (cf_pds_bound / pds_scale, cf_prep_feqmod phase 2e, the shard bound of
cf_multi.hip): a seeded table of transformations of synth.synth_surface / synth_vah_surface that take dsigma where the synthetic surfaces
never go -- cells 80 binades apart, one cell 2^60 above the rest, space-like and eta-dominated normals, inflow -- so that a bound that misses
a term, or a scale that is stale, lets the VOP3 clamp of the kernels' p.dsigma saturate at 1 and shows against the oracle's plain
`if (pds <= 0)` arithmetic.  Pure numpy; tests/test_hostile_surfaces.py checks the table on the CPU, tests/test_gpu_hostile_surfaces.py runs
it on the GPU.

Case            transformation of (dat, dax, day, dan); every factor an exact power of two but the stated uniform draws
binades         cell c times 2^k_c, k_c integer uniform in [-40, 40]
giant-first     cell 0 times 2^60, the rest untouched
giant-middle    cell n/2 times 2^60
giant-last      cell n-1 times 2^60
spacelike       dax = +-f dat, day = +-g dat, f and g uniform in [5, 40], independent random signs; in 3+1D also eta -> eta / 8: the time-like
                term of cf_pds_bound carries cosh(max_k |y_k - eta|), and with one scale per execute a single cell at |eta| = 4 hid a
                dropped pTmax (|dax| + |day|) term from every 3+1D run -- with |eta| <= 1/2 the off-tile grid's run fails without it
eta_heavy       (3+1D) dan = +-f dat tau, f uniform in [2, 20]: |dan| / tau, the term next to dat in p.dsigma, is up to 20 |dat|
inflow          cells 0, 3, 6, .. negated (u.dsigma <= 0: skipped); cells 1, 4, 7, .. turned space-like along the flow, dat = -d and
                (dax, day) = g u_perp / |u_perp| with d / g = 0.9 v_perp: u.dsigma > 0, and p.dsigma < 0 wherever
                cos(phi - phi_u) < 0.9 v_perp mT cosh(y - eta) / pT, which is most of the grid (all of it for slow or heavy hadrons)
uniform(k)      the whole surface times 2^k, k in UNIFORM_K: the spectrum must be ldexp(base, k)

Grids: the shipped 32 x 24 x 21 | 241 grid and the off-tile (J, K, n_pT) = (20, 9, 5) grid of tests/test_gpu_tile3e_rcp8.py.  Species: pi+,
K+, p, pbar and the heaviest species of the urqmd list (mTmax enters both bounds)."""
from functools import lru_cache

import numpy as np

from is3d_amd import inputs, synth

DS = ("dat", "dax", "day", "dan")
CASES = ("binades", "giant-first", "giant-middle", "giant-last", "spacelike", "eta_heavy", "inflow")
GIANTS = ("giant-first", "giant-middle", "giant-last")
UNIFORM_K = (-100, -7, 33, 100)
N_CELLS = 36          # 24 .. 64: two 3+1D prep batches of 16 and a tail, nine 2+1D batches
GIANT_LOG2 = 60
BINADES = 40
# tuned on the CPU (tests/test_hostile_surfaces.py) until the oracle alone meets the three conditions of that file
SEEDS = {"binades": 5101, "giant-first": 5102, "giant-middle": 5103, "giant-last": 5104, "spacelike": 5140, "eta_heavy": 5106, "inflow": 5107}


def species_ids():
    u = inputs.species("urqmd")
    return [211, 321, 2212, -2212, int(u["mc_id"][int(np.argmax(u["mass"]))])]


@lru_cache(maxsize=None)
def species():
    return inputs.species(species_ids())


@lru_cache(maxsize=None)
def grid(which):
    """'shipped' | 'offtile', with the reduction weights pT_w, phi_w of operation 0 (offtile: all ones)"""
    g = inputs.grid()
    if which == "shipped":
        return {k: g[k] for k in ("pT", "phi", "y", "eta", "eta_w", "pT_w", "phi_w")}
    J, K, n_pT = 20, 9, 5
    rng = np.random.default_rng(1000 * J + 10 * K + n_pT)
    return dict(pT=np.linspace(0.05, 3.2, n_pT), phi=np.sort(rng.random(J) * 2 * np.pi), y=np.linspace(-2.5, 2.5, K), eta=g["eta"], eta_w=g["eta_w"],
                pT_w=np.ones(n_pT), phi_w=np.ones(J))


def plain(g):
    return {k: g[k] for k in ("pT", "phi", "y", "eta", "eta_w")}


def exact_grid(dim):
    """part 3 (uniform(k)): pT <= 3 GeV and |y - eta| <= 3, so that no base value comes near the denormal range"""
    g = grid("shipped")
    keep = np.abs(g["eta"]) <= 3.0
    return dict(pT=g["pT"][g["pT"] <= 3.0], phi=g["phi"], y=np.linspace(-2.0, 2.0, 9), eta=g["eta"][keep], eta_w=g["eta_w"][keep])


def live(cells):
    ut = np.sqrt(1.0 + cells["ux"] ** 2 + cells["uy"] ** 2 + cells["tau"] ** 2 * cells["un"] ** 2)
    return ut * cells["dat"] + cells["ux"] * cells["dax"] + cells["uy"] * cells["day"] + cells["un"] * cells["dan"] > 0.0


def transform(cells, case, dim, seed):
    """a copy of `cells` with the case's transformation applied to its normal vectors"""
    c = {k: np.array(v, dtype=np.float64, copy=True) for k, v in cells.items()}
    n = len(c["tau"])
    rng = np.random.default_rng(seed)
    if case == "binades":
        k = rng.integers(-BINADES, BINADES + 1, n)
        for f in DS:
            c[f] = np.ldexp(c[f], k)
    elif case in GIANTS:
        i = {"giant-first": 0, "giant-middle": n // 2, "giant-last": n - 1}[case]
        for f in DS:
            c[f][i] = np.ldexp(c[f][i], GIANT_LOG2)
    elif case == "spacelike":
        c["dax"] = rng.choice([-1.0, 1.0], n) * rng.uniform(5.0, 40.0, n) * c["dat"]
        c["day"] = rng.choice([-1.0, 1.0], n) * rng.uniform(5.0, 40.0, n) * c["dat"]
        if dim == 3:
            c["eta"] = 0.125 * c["eta"]
    elif case == "eta_heavy":
        if dim != 3:
            raise ValueError("eta_heavy is a 3+1D case")
        c["dan"] = rng.choice([-1.0, 1.0], n) * rng.uniform(2.0, 20.0, n) * c["dat"] * c["tau"]
    elif case == "inflow":
        neg = np.arange(0, n, 3)
        for f in DS:
            c[f][neg] = -c[f][neg]
        t = np.arange(1, n, 3)
        up = np.hypot(c["ux"][t], c["uy"][t])
        ut = np.sqrt(1.0 + up * up + (c["tau"][t] * c["un"][t]) ** 2)
        d = np.abs(c["dat"][t])
        g = d * ut / (0.9 * up)
        c["dat"][t] = -d
        c["dax"][t] = g * c["ux"][t] / up
        c["day"][t] = g * c["uy"][t] / up
        c["dan"][t] = 0.0
    else:
        raise ValueError(case)
    return c


def uniform(cells, k):
    return {f: (np.ldexp(v, k) if f in DS else v) for f, v in cells.items()}


def base(dim, vah=False, baryon=False, n=N_CELLS, seed=5100):
    c = synth.synth_vah_surface(n, dim, seed=seed + dim) if vah else synth.synth_surface(n, dim, seed=seed + dim, baryon=baryon)
    return {k: np.array(v, copy=True) for k, v in c.items()}


@lru_cache(maxsize=None)
def _surface(case, dim, vah, baryon):
    c = transform(base(dim, vah, baryon), case, dim, SEEDS[case] + 10 * dim)
    for v in c.values():
        v.setflags(write=False)
    return c


def surface(case, dim, vah=False, baryon=False):
    """the case's surface (read-only arrays, shared)"""
    return _surface(case, dim, bool(vah), bool(baryon))


def exact_base(dim, vah=False):
    """part 3: cells with |eta| <= 1 under exact_grid's |y| <= 2"""
    c = base(dim, vah)
    if dim == 3:
        c["eta"] = 0.25 * c["eta"]
    return c


def out_of_range(dim):
    """one live cell (the middle one) with dat = 1e301: past the b < 1e300 cut of cf_pds_bound and of phase 2e"""
    c = base(dim)
    i = len(c["tau"]) // 2
    c["dat"][i] = 1.0e301
    return c, i
