"""What the tests of the decayed-and-binned entries share (tests/test_gpu_decays_mc_bins.py): the bins of the hand lists, the host route that
defines the result, and the condition under which host and device must reach the same bins.

The hand lists of tests/decays_mc_cases.py put every primary at tau = 1, r = 0.36, eta = 0.4, so with lifetime = 0 every final particle has
those coordinates.  BINS holds that point inside the tau, r and eta ranges; `spread` gives each primary a position of its own (same momenta,
species, events), so that with lifetime = 0 too every histogram has entries inside and particles outside its range.

host_route is the definition: is3d_decay_particles, species (a table entry) -> slot[species], slot -1 dropped, is3d_sampler_bin_list.

edge_clear is the condition of the parity tests on a relabelled list: no particle within 1e-9 of a bin edge (relative to the larger of the value and
the bin width; absolute for the rapidity) or of the |yp| <= y_cut gate.  Host and device see the same particle only up to the device's
contraction of multiply-adds, far below BOUND = 1.536e-12 of tests/decays_mc_cases.py, which is three orders below 1e-9."""
import numpy as np

BINS = dict(y_cut=1.2, y_bins=12, eta_cut=1.0, eta_bins=9, pT_lower_cut=0.1, pT_upper_cut=1.2, pT_bins=11, tau_min=0.3, tau_max=3.1, tau_bins=5,
            r_min=0.2, r_max=2.0, r_bins=6)
N_EVENTS = 7            # hand_list: 257 // 40 + 1; every_unstable: 303 // 50 + 1 = 346 // 50 + 1
COUNTS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield")
ALL = COUNTS + ("vn_re", "vn_im")
MARGIN = 1e-9


def spread(q, seed=11):
    """the list with a position of its own per primary: tau in [0.3, 3.6], eta in [-1.3, 1.3], x, y in [-1.5, 1.5]"""
    rng = np.random.default_rng(seed)
    out = q.copy()
    n = len(q)
    out["tau"], out["eta"] = rng.uniform(0.3, 3.6, n), rng.uniform(-1.3, 1.3, n)
    out["x"], out["y"] = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n)
    out["t"], out["z"] = out["tau"] * np.cosh(out["eta"]), out["tau"] * np.sinh(out["eta"])
    return out


def relabel(out, slot):
    """a decayed list (species = table entries) as the list that is binned: species -> slot, slot -1 dropped"""
    s = np.asarray(slot)[out["species"]]
    rel = out[s >= 0].copy()
    rel["species"] = s[s >= 0]
    return rel


def same(a, b, keys=ALL):
    return all(a[k].dtype == np.int64 and np.array_equal(a[k], b[k]) for k in keys)


def add(parts):
    return {k: sum(p[k] for p in parts) for k in ALL}


def edge_distance(p, bins):
    """the smallest distance of a particle of the list from a bin decision (absolute for the rapidity, else relative to the larger of the value
    and the bin width); inf for an empty list"""
    if len(p) == 0:
        return np.inf
    yp = 0.5 * np.log((p["E"] + p["pz"]) / (p["E"] - p["pz"]))
    yw = 2.0 * bins["y_cut"] / bins["y_bins"]
    u = (yp + bins["y_cut"]) / yw
    worst = min(np.abs(u - np.rint(u)).min() * yw, np.abs(np.abs(yp) - bins["y_cut"]).min())
    pT, r = np.sqrt(p["px"] ** 2 + p["py"] ** 2), np.sqrt(p["x"] ** 2 + p["y"] ** 2)
    for v, lo, hi, nb in ((p["eta"], -bins["eta_cut"], bins["eta_cut"], bins["eta_bins"]), (pT, bins["pT_lower_cut"], bins["pT_upper_cut"], bins["pT_bins"]),
                          (p["tau"], bins["tau_min"], bins["tau_max"], bins["tau_bins"]), (r, bins["r_min"], bins["r_max"], bins["r_bins"])):
        w = (hi - lo) / nb
        u = (v - lo) / w
        worst = min(worst, (np.abs(u - np.rint(u)) * w / np.maximum(np.abs(v), w)).min())
    return float(worst)


def edge_clear(p, bins):
    return edge_distance(p, bins) > MARGIN


def inside_and_outside(h, n, keys=("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r")):
    """every named histogram received entries and missed some of the n particles"""
    return all(0 < int(h[k].sum()) < n for k in keys)


def host_route(api, table, chosen, q, slot, n_slots, bins, n_events, lifetime=0, seed=1, first_particle=0):
    """-> (the decayed list, the relabelled list, its host histograms, the stats of is3d_decay_particles)"""
    out, _, st = api.decay_particles(table, chosen, q, seed=seed, lifetime=lifetime, first_particle=first_particle)
    rel = relabel(out, slot)
    return out, rel, api.sampler_bin_list(bins, n_events, n_slots, rel), st


def assert_parity(got, dst, want, rel, out, st):
    """counts and yields exactly, the harmonic sums within one unit per entry of the dN_pT bin, n_final, n_unbinned and every tally"""
    for k in COUNTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    for k in ("vn_re", "vn_im"):
        assert np.all(np.abs(got[k] - want[k]) <= want["dN_pT"][None]), k
    assert dst["n_final"] == len(out) and dst["n_unbinned"] == len(out) - len(rel) == dst["n_final"] - int(got["yield"].sum())
    for k in ("n_primaries", "n_decays", "n_final", "n_stuck", "n_trials", "n_exhausted", "max_stack", "max_depth", "n_closed_channels"):
        assert dst[k] == st[k], k
    assert dst["ms_count"] == dst["ms_fill"] == 0.0
