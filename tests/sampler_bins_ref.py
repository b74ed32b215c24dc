"""The one reference of the test_sampler = 1 bin rule that the CPU test (tests/test_sampler_bins_io.py) and the device tests
(tests/test_gpu_sampler_bins_lists.py) share: the hand-made particle list with particles on and beside every kind of edge (make_list), synthetic
lists of interior particles with explicit event arrays (interior_list), and the numpy restatement of sample_dN_dy ... sample_dN_dX
(sampling_kernels.cpp:31-152) -- numpy_hist, which is NOT the library's header csrc/cf_sampler_bins.h."""
import math

import numpy as np

from is3d_amd import api

BINS = dict(y_cut=1.5, eta_cut=4.0, pT_lower_cut=0.25, pT_upper_cut=2.75, tau_min=1.0, tau_max=9.0, r_min=0.5, r_max=8.0,
            y_bins=12, eta_bins=16, pT_bins=10, tau_bins=8, r_bins=15)
MASS = np.array([0.138, 0.494, 0.938])
IDS = [211, 321, 2212]
N_EVENTS = 5            # event 3 stays empty
COUNTS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield")
GATED = ("dN_pT", "dN_tau", "dN_r", "vn_re", "vn_im")       # what only particles inside |yp| <= y_cut add to
ALL = COUNTS + ("vn_re", "vn_im")
NAN_FIELDS = ("E", "px", "tau", "x", "eta")                 # one particle of make_list each
LOG_DECIDED = 1e-12     # a rapidity decision closer to an edge than this belongs to log's last bits, not to the bin rule

# kinds of the rows of make_list: a random row, a hand-made row whose rapidity is placed on or beside a rapidity edge, another hand-made row,
# and K_NAN + i for the row that gets NaN in NAN_FIELDS[i]
K_RANDOM, K_Y, K_EDGE, K_NAN = 0, 1, 2, 10


def _edge_particles():
    """(y, pT, phi, eta, tau, r) by hand: on the edge, one step of the last bit to either side, and well inside; and the kind of each row."""
    b = BINS
    rows, kinds = [], []

    def beside(v):
        return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]

    for y in beside(b["y_cut"]) + beside(-b["y_cut"]) + beside(0.0) + [b["y_cut"] + 1e-12, -b["y_cut"] - 1e-12, 2 * b["y_cut"]]:
        rows.append((y, 1.0, 0.3, 0.1, 4.0, 3.0))
        kinds.append(K_Y)
    pw = (b["pT_upper_cut"] - b["pT_lower_cut"]) / b["pT_bins"]
    for pT in beside(b["pT_lower_cut"]) + beside(b["pT_upper_cut"]) + beside(b["pT_lower_cut"] + 3 * pw) + [0.0, 1e-300, 10.0]:
        for phi in (0.0, -0.4, 2.5, -3.0, math.pi, -math.pi, -1e-17):     # phi < 0 is wrapped into [0, 2 pi)
            rows.append((0.2, pT, phi, -0.7, 4.0, 3.0))
            kinds.append(K_EDGE)
    for tau in beside(b["tau_min"]) + beside(b["tau_max"]) + [0.5 * b["tau_min"], 2.0 * b["tau_max"], b["tau_min"] + 3.0]:
        rows.append((-0.3, 0.8, 1.0, 0.0, tau, 3.0))
        kinds.append(K_EDGE)
    for r in beside(b["r_min"]) + beside(b["r_max"]) + [0.0, 0.5 * b["r_min"], 3.0 * b["r_max"]]:
        rows.append((0.4, 0.8, -2.0, 0.0, 4.0, r))
        kinds.append(K_EDGE)
    for eta in beside(b["eta_cut"]) + beside(-b["eta_cut"]) + [0.0, 9.0, -9.0]:
        rows.append((0.0, 0.9, 0.7, eta, 4.0, 3.0))          # y = 0 by hand: E + pz == E - pz, ON the edge between the two middle rapidity bins
        kinds.append(K_Y)
    for i in range(len(NAN_FIELDS)):                          # well inside every range; make_list puts the NaN in
        rows.append((0.3, 0.9, 0.5, 0.6, 4.5, 2.5))
        kinds.append(K_NAN + i)
    return np.array(rows), np.array(kinds)


def make_list(with_kinds=False):
    rng = np.random.default_rng(11)
    edge, edge_kinds = _edge_particles()
    n_rand = 2000 - len(edge)
    rand = np.stack([rng.normal(0, 1.2, n_rand), rng.gamma(2.0, 0.4, n_rand), rng.uniform(-math.pi, math.pi, n_rand), rng.normal(0, 2.5, n_rand),
                     rng.uniform(0.2, 11.0, n_rand), np.abs(rng.normal(0, 4.0, n_rand))], axis=1)
    rows = np.concatenate([edge, rand])
    kinds = np.concatenate([edge_kinds, np.full(n_rand, K_RANDOM)])
    perm = rng.permutation(len(rows))
    rows, kinds = rows[perm], kinds[perm]
    n = len(rows)
    p = np.zeros(n, dtype=api.PARTICLE_DTYPE)
    p["event"] = np.sort(rng.choice([0, 1, 2, 4], n))
    p["species"] = rng.integers(0, 3, n)
    y, pT, phi, eta, tau, r = rows.T
    m = MASS[p["species"]]
    p["px"], p["py"] = pT * np.cos(phi), pT * np.sin(phi)
    p["px"][phi == 0.0] = pT[phi == 0.0]                  # pT lands on the cut exactly
    mT = np.sqrt(m * m + pT * pT)
    p["pz"], p["E"] = mT * np.sinh(y), mT * np.cosh(y)
    p["eta"], p["tau"] = eta, tau
    a = rng.uniform(-math.pi, math.pi, n)
    p["x"], p["y"] = r * np.cos(a), r * np.sin(a)
    on_axis = rng.random(n) < 0.3
    p["x"][on_axis], p["y"][on_axis] = r[on_axis], 0.0    # r lands on its edges exactly
    p["t"], p["z"] = tau * np.cosh(eta), tau * np.sinh(eta)
    p["cell"] = np.arange(n)
    for i, f in enumerate(NAN_FIELDS):
        p[f][kinds == K_NAN + i] = np.nan
    return (p, kinds) if with_kinds else p


def interior_list(n, n_species=3, seed=5):
    """n particles well inside every range of BINS (every histogram counts every particle), events all 0: the caller sets p["event"]."""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=api.PARTICLE_DTYPE)
    p["species"] = rng.integers(0, n_species, n)
    y, pT, phi = rng.uniform(-1.4, 1.4, n), rng.uniform(0.3, 2.7, n), rng.uniform(-math.pi, math.pi, n)
    m = MASS[p["species"] % len(MASS)]
    p["px"], p["py"] = pT * np.cos(phi), pT * np.sin(phi)
    mT = np.sqrt(m * m + pT * pT)
    p["pz"], p["E"] = mT * np.sinh(y), mT * np.cosh(y)
    p["eta"], p["tau"] = rng.uniform(-3.9, 3.9, n), rng.uniform(1.1, 8.9, n)
    r, a = rng.uniform(0.6, 7.9, n), rng.uniform(-math.pi, math.pi, n)
    p["x"], p["y"] = r * np.cos(a), r * np.sin(a)
    p["t"], p["z"] = p["tau"] * np.cosh(p["eta"]), p["tau"] * np.sinh(p["eta"])
    p["cell"] = np.arange(n)
    return p


def numpy_hist(p, b, n_events, n_species, longdouble=False, gate=None):
    """The per-particle rule of the list writer (floor((v - lo) / width), the |yp| <= y_cut gate, phi in [0, 2 pi)), restated.  yp goes through
    math.log -- the C library's log, as the host code's -- so that the bins of particles ON a rapidity edge are decided by the same function;
    every other operation is correctly rounded in numpy as in C.  A NaN reaches no bin of the histograms it feeds; the yield counts it.

    longdouble = True: yp and its two decisions in np.longdouble instead, and the return is (histograms, u, d): per particle the bin coordinate
    u = (yp + y_cut) / yw and the distance d = | |yp| - y_cut | of the gate, both long double -- what says which particles' rapidity decisions
    are log's and not the rule's.  gate (bool per particle): the |yp| <= y_cut decision, overridden."""
    S = n_species
    yw, ew = 2.0 * b["y_cut"] / b["y_bins"], 2.0 * b["eta_cut"] / b["eta_bins"]
    pw = (b["pT_upper_cut"] - b["pT_lower_cut"]) / b["pT_bins"]
    tw, rw = (b["tau_max"] - b["tau_min"]) / b["tau_bins"], (b["r_max"] - b["r_min"]) / b["r_bins"]
    if longdouble:
        E, pz = p["E"].astype(np.longdouble), p["pz"].astype(np.longdouble)
        yp = np.longdouble(0.5) * np.log((E + pz) / (E - pz))
        u = (yp + np.longdouble(b["y_cut"])) / np.longdouble(yw)
    else:
        yp = np.array([0.5 * math.log(q) for q in (p["E"] + p["pz"]) / (p["E"] - p["pz"])])
        u = (yp + b["y_cut"]) / yw
    sp = p["species"].astype(np.int64)
    out = dict(dN_dy=np.zeros((S, b["y_bins"]), np.int64), dN_deta=np.zeros((S, b["eta_bins"]), np.int64), dN_pT=np.zeros((S, b["pT_bins"]), np.int64),
               dN_tau=np.zeros((S, b["tau_bins"]), np.int64), dN_r=np.zeros((S, b["r_bins"]), np.int64))
    out["yield"] = np.bincount(p["event"], minlength=n_events).astype(np.int64)

    def count(name, idx, nb, gate):
        ok = gate & (idx >= 0) & (idx < nb)
        np.add.at(out[name], (sp[ok], idx[ok].astype(np.int64)), 1)
        return ok

    everyone = np.ones(len(p), bool)
    mid = np.abs(yp) <= b["y_cut"] if gate is None else np.asarray(gate, bool)
    count("dN_dy", np.floor(u), b["y_bins"], everyone)
    count("dN_deta", np.floor((p["eta"] + b["eta_cut"]) / ew), b["eta_bins"], everyone)
    pT = np.sqrt(p["px"] * p["px"] + p["py"] * p["py"])
    ipT = np.floor((pT - b["pT_lower_cut"]) / pw)
    ok = count("dN_pT", ipT, b["pT_bins"], mid)
    count("dN_tau", np.floor((p["tau"] - b["tau_min"]) / tw), b["tau_bins"], mid)
    r = np.sqrt(p["x"] * p["x"] + p["y"] * p["y"])
    count("dN_r", np.floor((r - b["r_min"]) / rw), b["r_bins"], mid)
    phi = np.arctan2(p["py"], p["px"])
    phi = np.where(phi < 0.0, phi + 2.0 * math.pi, phi)
    out["vn_re"] = np.zeros((api.VN_HARMONICS, S, b["pT_bins"]), np.int64)
    out["vn_im"] = np.zeros_like(out["vn_re"])
    for k in range(api.VN_HARMONICS):
        np.add.at(out["vn_re"][k], (sp[ok], ipT[ok].astype(np.int64)), np.rint(np.cos((k + 1.0) * phi[ok]) * api.VN_SCALE).astype(np.int64))
        np.add.at(out["vn_im"][k], (sp[ok], ipT[ok].astype(np.int64)), np.rint(np.sin((k + 1.0) * phi[ok]) * api.VN_SCALE).astype(np.int64))
    if longdouble:
        return out, u, np.abs(np.abs(yp) - np.longdouble(b["y_cut"]))
    return out


def log_decided(u, d):
    """The particles whose rapidity bin or gate lies within LOG_DECIDED of an edge (u, d: numpy_hist(longdouble=True))."""
    with np.errstate(invalid="ignore"):
        return (np.abs(u - np.rint(u)) <= LOG_DECIDED) | (d <= LOG_DECIDED)


def layout_total(b, n_species):
    """The words of the device histogram block (SamplerHistLayout.total): the counts and 2 x 7 harmonic planes over dN_pT's bins."""
    return n_species * (b["y_bins"] + b["eta_bins"] + b["tau_bins"] + b["r_bins"] + (1 + 2 * api.VN_HARMONICS) * b["pT_bins"])
