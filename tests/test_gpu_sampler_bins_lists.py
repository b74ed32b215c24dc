"""GPU (-m gpu): the device kernel of the test_sampler = 1 distributions (cf_sampler_bins, both forms) on lists made by hand, through
is3d_sampler_bin_list_device: particles on and beside every edge, NaN coordinates, event runs placed against the wave (length 1, 64, 65, a
run that starts at lane 63), list lengths around the wave, the workgroup and the grid-stride trip, a list that is not ordered by event,
particles whose species or event index is out of range, the histogram block at and one word past the LDS bound, and harmonic sums of either
sign.  The reference is the numpy restatement of the per-particle rule (tests/sampler_bins_ref.py: numpy_hist), compared bit for bit; the host
side of the library (is3d_sampler_bin_list) is compared as well, which states that host and device reach the same bins from the same bits.

What these cases found: nothing wrong in the kernel -- every case below passes on an MI355X in all three forms, bit for bit.  The 19 log-decided
particles of the hand-made list (of 2000) all take the bin the C library's log gives them (57 calls of 57); the launch with exactly 8192 words
(65 536 bytes of dynamic LDS) runs without a function attribute and gives the reference's bits.  On the host side the cases did find that
is3d_sampler_bin_list and the two writers accepted an empty range (a division by zero); they refuse it now, as the device entries do
(tests/test_sampler_bins_io.py)."""
import math
from functools import lru_cache

import numpy as np
import pytest

import sampler_bins_ref as R
from is3d_amd import api

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2)                      # the measured choice | global atomics | workgroup-private
SIZES = (1, 63, 64, 65, 255, 256, 257, 4096, 4097, 10000)
N_BIG = 10000                          # three workgroups of the private form, a multi-trip grid-stride loop, a ragged last trip
RUN_AT_63 = 130                        # the run that starts at lane 63 crosses two wave boundaries


def device_hist(bins, n_events, n_species, p, form):
    h, skipped = api.sampler_bin_list_device(dict(bins, kernel_form=form), n_events, n_species, p)
    assert all(h[k].dtype == np.int64 for k in R.ALL)
    return h, skipped


def assert_hist(got, want, what, keys=R.ALL):
    """Counts and yields bit for bit; the harmonic sums within one fixed-point step per particle of the bin (device and numpy atan2 / sin /
    cos differ by ulps, far below a step of 2^-32, so one rounding of term * 2^32 moves a term by at most one step)."""
    for k in keys:
        if k in ("vn_re", "vn_im"):
            assert np.all(np.abs(got[k] - want[k]) <= want["dN_pT"][None]), (what, k, int(np.abs(got[k] - want[k]).max()))
        else:
            assert np.array_equal(got[k], want[k]), (what, k)


# ---- references: computed once, shared, never written to ----
@lru_cache(maxsize=None)
def big():
    p = R.interior_list(N_BIG)
    yp = 0.5 * np.log((p["E"] + p["pz"]) / (p["E"] - p["pz"]))
    u = (yp + R.BINS["y_cut"]) / (2.0 * R.BINS["y_cut"] / R.BINS["y_bins"])
    assert np.abs(u - np.rint(u)).min() > 1e-9 and np.abs(np.abs(yp) - R.BINS["y_cut"]).min() > 1e-9     # no rapidity decision is log's
    p.setflags(write=False)
    return p


def events_of(layout, n):
    i = np.arange(n)
    if layout == "runs of 1":
        return i
    if layout == "runs of 64":
        return i // 64
    if layout == "runs of 65":
        return i // 65
    assert layout == "run from lane 63"
    return (i >= 63).astype(np.int64) + (i >= 63 + RUN_AT_63)


LAYOUTS = ("runs of 1", "runs of 64", "runs of 65", "run from lane 63")


@lru_cache(maxsize=None)
def prefix_reference(n):
    """The histograms of the first n particles of big() (all in event 0), by the restatement and by the library's host side."""
    p = big()[:n]
    want = R.numpy_hist(p, R.BINS, 1, 3)
    host = api.sampler_bin_list(R.BINS, 1, 3, p)
    assert_hist(host, want, ("host", n))
    assert all(want[k].sum() == n for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r"))      # interior: everybody is counted everywhere
    return want, host


@lru_cache(maxsize=None)
def edge_split():
    p, kinds = R.make_list(with_kinds=True)
    ref, u, d = R.numpy_hist(p, R.BINS, R.N_EVENTS, 3, longdouble=True)
    hard = R.log_decided(u, d)
    return p, kinds, u, d, hard


def test_edge_list_bulk_is_exact():
    """The hand-made list (edges of every histogram, one ulp to either side, phi wrapped, pT on a cut, empty events, NaN in E, px, tau, x, eta)
    without its 19 log-decided particles, in one call per form: every count equals the restatement's and the host's.
    On an MI355X: equal in forms 0, 1 and 2, the five NaN rows included; nothing found."""
    p, kinds, u, d, hard = edge_split()
    assert 0 < hard.sum() <= 0.02 * len(p) and (kinds[hard] == R.K_Y).all()
    easy = p[~hard]
    assert all((kinds[~hard] == R.K_NAN + i).sum() == 1 for i in range(len(R.NAN_FIELDS)))     # the NaN rows are compared here
    assert (kinds[~hard] == R.K_EDGE).sum() > 60
    want = R.numpy_hist(easy, R.BINS, R.N_EVENTS, 3)
    host = api.sampler_bin_list(R.BINS, R.N_EVENTS, 3, easy)
    assert want["yield"][3] == 0 and all(0 < want[k].sum() < len(easy) for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r"))
    for form in FORMS:
        got, skipped = device_hist(R.BINS, R.N_EVENTS, 3, easy, form)
        assert skipped == 0 and got["yield"].sum() == len(easy)
        assert_hist(got, want, ("restatement", form))
        assert_hist(got, host, ("host", form))


def test_nan_rows_reach_no_bin_on_the_device():
    """The NaN rule of sampler_bin_of and of the gate, one particle per call: NaN in E closes dN_dy and the gate, in px dN_pT and the harmonic
    sums, in tau, x, eta their own histogram; the yield counts the particle.  On an MI355X: as stated, in every form; nothing found."""
    p, kinds, *_ = edge_split()
    for i, f in enumerate(R.NAN_FIELDS):
        q = p[kinds == R.K_NAN + i]
        want = R.numpy_hist(q, R.BINS, R.N_EVENTS, 3)
        empty = dict(E=("dN_dy", "dN_pT", "dN_tau", "dN_r"), px=("dN_pT",), tau=("dN_tau",), x=("dN_r",), eta=("dN_deta",))[f]
        assert {k for k in R.COUNTS if want[k].sum() == 0} == set(empty)
        for form in FORMS:
            got, skipped = device_hist(R.BINS, R.N_EVENTS, 3, q, form)
            assert skipped == 0
            assert_hist(got, want, (f, form))


def test_log_decided_particles_land_beside_their_edge():
    """Each log-decided particle alone in a list: the device's log may differ from the C library's in the last bit, so its dN_dy bin is one of
    the two bins at the edge (or none, at an outer edge), and its gated histograms are the restatement's with the gate open, or empty; where the
    gate is not the close call (an inner edge) they are the restatement's.  On an MI355X: 19 log-decided particles, 57 calls, all 57 equal to
    the C library's decision (the device's log agreed in the last bit on every one); nothing found."""
    p, kinds, u, d, hard = edge_split()
    b = R.BINS
    n_same = n_calls = 0
    for i in np.flatnonzero(hard):
        q = p[i:i + 1]
        s = int(q["species"][0])
        edge = int(np.rint(u[i]))
        allowed = [k for k in (edge - 1, edge) if 0 <= k < b["y_bins"]]
        gate_close = d[i] <= R.LOG_DECIDED
        want = R.numpy_hist(q, b, R.N_EVENTS, 3)
        opened = R.numpy_hist(q, b, R.N_EVENTS, 3, gate=[True])
        for form in FORMS:
            got, skipped = device_hist(b, R.N_EVENTS, 3, q, form)
            assert skipped == 0
            assert_hist(got, want, (i, form), keys=("dN_deta", "yield"))
            row = got["dN_dy"][s]
            assert got["dN_dy"].sum() == row.sum() <= 1 and all(k in allowed for k in np.flatnonzero(row)), (i, form, u[i], row)
            if len(allowed) == 2:
                assert row.sum() == 1, (i, form, u[i])
            if gate_close:
                is_open = all(np.array_equal(got[k], opened[k]) for k in ("dN_pT", "dN_tau", "dN_r")) and \
                    all(np.all(np.abs(got[k] - opened[k]) <= opened["dN_pT"][None]) for k in ("vn_re", "vn_im"))
                assert is_open or not any(got[k].any() for k in R.GATED), (i, form, d[i])
            else:
                assert_hist(got, want, (i, form), keys=R.GATED)
            n_calls += 1
            n_same += all(np.array_equal(got[k], want[k]) for k in R.COUNTS)
    print("log-decided particles:", int(hard.sum()), "calls:", n_calls, "equal to the C library's decision:", n_same)


@pytest.mark.parametrize("n", SIZES)
def test_yield_runs_against_the_wave(n):
    """The first n particles of one interior list under four event layouts: runs of 1 (every lane leads), runs of 64 on the wave, runs of 65
    (the leader moves one lane per wave), one run that starts at lane 63.  The per-event yields are the run lengths; the histograms do not
    depend on the layout.  On an MI355X: every n, layout and form equal; nothing found."""
    p = big()[:n].copy()
    want, host = prefix_reference(n)
    for layout in LAYOUTS:
        ev = events_of(layout, n)
        n_events = int(ev.max()) + 2                         # the last event stays empty
        p["event"] = ev
        y = np.bincount(ev, minlength=n_events).astype(np.int64)
        assert y[-1] == 0 and y.sum() == n
        for form in FORMS:
            got, skipped = device_hist(R.BINS, n_events, 3, p, form)
            assert skipped == 0
            assert np.array_equal(got["yield"], y), (layout, form)
            assert_hist(got, want, (layout, form, "restatement"), keys=R.ALL[:5] + R.ALL[6:])
            assert_hist(got, host, (layout, form, "host"), keys=R.ALL[:5] + R.ALL[6:])


def test_an_unordered_list_is_counted_the_same():
    """The 10 000 particles in runs of 65 and the same particles shuffled (no order by event: every lane may lead): the same bits, harmonic
    sums included.  On an MI355X: equal in every form; nothing found."""
    p = big().copy()
    p["event"] = events_of("runs of 65", N_BIG)
    n_events = int(p["event"].max()) + 1
    want = R.numpy_hist(p, R.BINS, n_events, 3)
    q = p[np.random.default_rng(3).permutation(N_BIG)]
    assert (np.diff(q["event"]) < 0).sum() > N_BIG // 3
    for form in FORMS:
        a, _ = device_hist(R.BINS, n_events, 3, p, form)
        s, skipped = device_hist(R.BINS, n_events, 3, q, form)
        assert skipped == 0
        assert all(np.array_equal(a[k], s[k]) for k in R.ALL), form
        assert_hist(s, want, form)


def test_out_of_range_indices_add_nothing():
    """5 % of the 10 000 particles carry species = -1, species = n_species, event = -1 or event = n_events -- at run starts, inside runs, at
    lane 0, in adjacent pairs: the histograms are those of the list without them (the restatement on the filtered list; is3d_sampler_bin_list
    refuses the unfiltered one), the runs around them keep their lengths, n_skipped is their number.  On an MI355X: as stated in every form; nothing found."""
    p = big().copy()
    p["event"] = events_of("runs of 65", N_BIG)
    n_events = int(p["event"].max()) + 1
    rng = np.random.default_rng(17)
    i = np.arange(N_BIG)
    starts, lane0 = i[i % 65 == 0][:120], i[i % 64 == 0][40:140]          # whole neighbouring runs lose their first particle; lane 0 of a wave
    fixed = np.unique(np.concatenate([starts, lane0, lane0[:30] + 1]))      # ... and adjacent pairs
    inside = rng.choice(np.setdiff1d(i, fixed), 500 - len(fixed), replace=False)
    bad = np.sort(np.concatenate([fixed, inside]))
    assert len(bad) == 500 == len(np.unique(bad)) and (np.diff(bad) == 1).sum() >= 30
    for j, k in enumerate(bad):
        field, value = (("species", -1), ("species", 3), ("event", -1), ("event", n_events))[j % 4]
        p[field][k] = value
    keep = np.ones(N_BIG, bool)
    keep[bad] = False
    want = R.numpy_hist(p[keep], R.BINS, n_events, 3)
    with pytest.raises(api.Is3dError) as e:
        api.sampler_bin_list(R.BINS, n_events, 3, p)
    assert e.value.code == api.IS3D_EINVAL
    for form in FORMS:
        got, skipped = device_hist(R.BINS, n_events, 3, p, form)
        assert skipped == 500 and got["yield"].sum() == N_BIG - 500
        assert_hist(got, want, form)


LDS_FIT = dict(R.BINS, pT_bins=500, y_bins=200, eta_bins=200, tau_bins=146, r_bins=146)       # 15 * 500 + 200 + 200 + 146 + 146 = 8192 words
LDS_OVER = dict(LDS_FIT, r_bins=147)                                                           # 8193


def test_the_lds_boundary():
    """One species, the histogram block at exactly 8192 words (65 536 bytes of dynamic LDS, the bound of sampler_bins_lds_fits) and at 8193:
    forms 0, 1 and 2 on the first, forms 0 and 1 on the second (form 0 falls to global atomics), form 2 refused there before any device use.
    On an MI355X: the 8192-word launch ran (no launch error, no attribute needed) and every result equals the reference; nothing found."""
    assert R.layout_total(LDS_FIT, 1) == 8192 and R.layout_total(LDS_OVER, 1) == 8193
    p = big().copy()
    p["species"] = 0
    p["event"] = events_of("runs of 65", N_BIG)
    n_events = int(p["event"].max()) + 1
    for bins, forms in ((LDS_FIT, FORMS), (LDS_OVER, (0, 1))):
        want = R.numpy_hist(p, bins, n_events, 1)
        host = api.sampler_bin_list(bins, n_events, 1, p)
        assert want["dN_pT"].sum() == N_BIG and (want["dN_pT"] > 0).sum() > 400      # the whole block is in use
        for form in forms:
            got, skipped = device_hist(bins, n_events, 1, p, form)
            assert skipped == 0
            assert_hist(got, want, (bins["r_bins"], form, "restatement"))
            assert_hist(got, host, (bins["r_bins"], form, "host"))
    p0, a0 = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        device_hist(LDS_OVER, n_events, 1, p, 2)
    assert e.value.code == api.IS3D_EINVAL and "8193" in str(e.value)
    assert api.resource_counters() == (p0, a0)


def test_harmonic_sums_of_either_sign():
    """5000 particles at phi = pi in one pT bin, 5000 at phi = 0 in another, over several workgroups: the two's-complement adds through
    unsigned long long keep strongly negative and strongly positive sums.  phi = 0 (px = pT, py = 0) is exact: vn_re = count * 2^32, vn_im = 0;
    phi = pi against the restatement within the per-particle step, and odd harmonics below -0.99 count * 2^32.
    On an MI355X: as stated in every form; nothing found."""
    p = big().copy()
    p["event"] = events_of("runs of 65", N_BIG)
    n_events = int(p["event"].max()) + 1
    half = np.arange(N_BIG) % 2 == 0
    p["px"], p["py"] = np.where(half, -0.8, 1.6), 0.0
    pw = (R.BINS["pT_upper_cut"] - R.BINS["pT_lower_cut"]) / R.BINS["pT_bins"]
    neg, pos = int(math.floor((0.8 - R.BINS["pT_lower_cut"]) / pw)), int(math.floor((1.6 - R.BINS["pT_lower_cut"]) / pw))
    want = R.numpy_hist(p, R.BINS, n_events, 3)
    assert neg != pos and want["dN_pT"][:, neg].sum() == want["dN_pT"][:, pos].sum() == N_BIG // 2
    one = 2 ** 32
    for form in FORMS:
        got, _ = device_hist(R.BINS, n_events, 3, p, form)
        assert_hist(got, want, form)
        cnt = got["dN_pT"]
        assert np.array_equal(got["vn_re"][:, :, pos], np.broadcast_to(cnt[:, pos] * one, (api.VN_HARMONICS, 3))), form
        assert not got["vn_im"][:, :, pos].any(), form
        assert np.all(got["vn_re"][0::2, :, neg] < -0.99 * one * cnt[None, :, neg]) and np.all(got["vn_re"][1::2, :, neg] > 0.99 * one * cnt[None, :, neg])
        assert got["vn_re"].min() < -1000 * one and got["vn_re"].max() > 1000 * one


def test_an_empty_list_is_zero_histograms():
    """n_particles = 0: zero histograms and no launch (no allocation either).  On an MI355X: as stated; nothing found."""
    p0, a0 = api.resource_counters()
    got, skipped = device_hist(R.BINS, 4, 3, big()[:0], 0)
    assert skipped == 0 and got["yield"].shape == (4,) and not any(got[k].any() for k in R.ALL)
    assert api.resource_counters() == (p0, a0)
