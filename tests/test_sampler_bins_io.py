"""CPU: the integer histograms of the test_sampler = 1 distributions (is3d_sampler_bin_list, the host side of the one bin rule in
csrc/cf_sampler_bins.h) against a numpy restatement of sample_dN_dy ... sample_dN_dX (sampling_kernels.cpp:31-152), and the histogram
writer (is3d_write_sampler_tests_binned) against the list writer, on a hand-made list with particles on and beside every kind of edge."""
import math
import os

import numpy as np

from is3d_amd import api

BINS = dict(y_cut=1.5, eta_cut=4.0, pT_lower_cut=0.25, pT_upper_cut=2.75, tau_min=1.0, tau_max=9.0, r_min=0.5, r_max=8.0,
            y_bins=12, eta_bins=16, pT_bins=10, tau_bins=8, r_bins=15)
MASS = np.array([0.138, 0.494, 0.938])
IDS = [211, 321, 2212]
N_EVENTS = 5            # event 3 stays empty
DIRS = ("dN_dy", "dN_deta", "momentum_distribution", "vn", "spacetime_distribution")


def _edge_particles():
    """(y, pT, phi, eta, tau, r) by hand: on the edge, one step of the last bit to either side, and well inside."""
    b = BINS
    rows = []

    def beside(v):
        return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]

    for y in beside(b["y_cut"]) + beside(-b["y_cut"]) + beside(0.0) + [b["y_cut"] + 1e-12, -b["y_cut"] - 1e-12, 2 * b["y_cut"]]:
        rows.append((y, 1.0, 0.3, 0.1, 4.0, 3.0))
    pw = (b["pT_upper_cut"] - b["pT_lower_cut"]) / b["pT_bins"]
    for pT in beside(b["pT_lower_cut"]) + beside(b["pT_upper_cut"]) + beside(b["pT_lower_cut"] + 3 * pw) + [0.0, 1e-300, 10.0]:
        for phi in (0.0, -0.4, 2.5, -3.0, math.pi, -math.pi, -1e-17):     # phi < 0 is wrapped into [0, 2 pi)
            rows.append((0.2, pT, phi, -0.7, 4.0, 3.0))
    for tau in beside(b["tau_min"]) + beside(b["tau_max"]) + [0.5 * b["tau_min"], 2.0 * b["tau_max"], b["tau_min"] + 3.0]:
        rows.append((-0.3, 0.8, 1.0, 0.0, tau, 3.0))
    for r in beside(b["r_min"]) + beside(b["r_max"]) + [0.0, 0.5 * b["r_min"], 3.0 * b["r_max"]]:
        rows.append((0.4, 0.8, -2.0, 0.0, 4.0, r))
    for eta in beside(b["eta_cut"]) + beside(-b["eta_cut"]) + [0.0, 9.0, -9.0]:
        rows.append((0.0, 0.9, 0.7, eta, 4.0, 3.0))
    return np.array(rows)


def make_list():
    rng = np.random.default_rng(11)
    edge = _edge_particles()
    n_rand = 2000 - len(edge)
    rand = np.stack([rng.normal(0, 1.2, n_rand), rng.gamma(2.0, 0.4, n_rand), rng.uniform(-math.pi, math.pi, n_rand), rng.normal(0, 2.5, n_rand),
                     rng.uniform(0.2, 11.0, n_rand), np.abs(rng.normal(0, 4.0, n_rand))], axis=1)
    rows = np.concatenate([edge, rand])
    rows = rows[rng.permutation(len(rows))]
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
    return p


def numpy_hist(p, b, n_events, n_species):
    """The per-particle rule of the list writer (floor((v - lo) / width), the |yp| <= y_cut gate, phi in [0, 2 pi)), restated.  yp goes through
    math.log -- the C library's log, as the host code's -- so that the bins of particles ON a rapidity edge are decided by the same function;
    every other operation is correctly rounded in numpy as in C."""
    S = n_species
    yw, ew = 2.0 * b["y_cut"] / b["y_bins"], 2.0 * b["eta_cut"] / b["eta_bins"]
    pw = (b["pT_upper_cut"] - b["pT_lower_cut"]) / b["pT_bins"]
    tw, rw = (b["tau_max"] - b["tau_min"]) / b["tau_bins"], (b["r_max"] - b["r_min"]) / b["r_bins"]
    yp = np.array([0.5 * math.log(q) for q in (p["E"] + p["pz"]) / (p["E"] - p["pz"])])
    sp = p["species"].astype(np.int64)
    out = dict(dN_dy=np.zeros((S, b["y_bins"]), np.int64), dN_deta=np.zeros((S, b["eta_bins"]), np.int64), dN_pT=np.zeros((S, b["pT_bins"]), np.int64),
               dN_tau=np.zeros((S, b["tau_bins"]), np.int64), dN_r=np.zeros((S, b["r_bins"]), np.int64))
    out["yield"] = np.bincount(p["event"], minlength=n_events).astype(np.int64)

    def count(name, idx, nb, gate):
        ok = gate & (idx >= 0) & (idx < nb)
        np.add.at(out[name], (sp[ok], idx[ok].astype(np.int64)), 1)
        return ok

    everyone = np.ones(len(p), bool)
    mid = np.abs(yp) <= b["y_cut"]
    count("dN_dy", np.floor((yp + b["y_cut"]) / yw), b["y_bins"], everyone)
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
    return out


def _result_files(root):
    found = {}
    for d, _, names in os.walk(root):
        for n in names:
            path = os.path.join(d, n)
            found[os.path.relpath(path, root)] = open(path, "rb").read()
    return found


def test_bin_list_matches_the_numpy_restatement():
    p = make_list()
    assert 1900 <= len(p) <= 2100 and not (p["event"] == 3).any() and (np.arctan2(p["py"], p["px"]) < 0).any()
    got = api.sampler_bin_list(BINS, N_EVENTS, 3, p)
    want = numpy_hist(p, BINS, N_EVENTS, 3)
    for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    assert got["yield"][3] == 0 and got["yield"].sum() == len(p)
    # the edges did their work: every histogram left particles outside its range (or outside the rapidity gate)
    assert all(0 < got[k].sum() < len(p) for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r"))
    # fixed point: numpy's and the C library's cos / sin differ by ulps; one rounding of term * 2^32 makes that at most one step per term
    for k in ("vn_re", "vn_im"):
        assert np.all(np.abs(got[k] - want[k]) <= got["dN_pT"][None]), k
    assert np.abs(got["vn_re"]).max() > 2 ** 32      # the sums are the scaled ones


def test_binned_writer_matches_the_list_writer(tmp_path):
    p = make_list()
    roots = []
    for name in ("list", "binned"):
        root = str(tmp_path / name)
        for d in DIRS:
            os.makedirs(os.path.join(root, d))
        roots.append(root)
    api.write_sampler_tests(roots[0], BINS, N_EVENTS, IDS, p, mean_yield=412.25)
    api.write_sampler_tests_binned(roots[1], BINS, N_EVENTS, IDS, api.sampler_bin_list(BINS, N_EVENTS, 3, p), mean_yield=412.25)
    a, b = _result_files(roots[0]), _result_files(roots[1])
    assert sorted(a) == sorted(b) and len(a) == 7 * 3 + 2
    n_vn = 0
    for name in a:
        if name.startswith("vn" + os.sep):
            # the fixed point moves v_n by at most 2^-32 absolute; the stream prints 7 digits
            va, vb = np.loadtxt(os.path.join(roots[0], name)), np.loadtxt(os.path.join(roots[1], name))
            assert va.shape == vb.shape == (BINS["pT_bins"], 8)
            assert np.allclose(vb, va, atol=1e-9, rtol=2e-6), name
            n_vn += 1
        else:
            assert a[name] == b[name], name
    assert n_vn == 3
