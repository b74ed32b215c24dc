"""CPU: the host route of the HBT correlation functions (is3d_hbt_list, the explicit double loop: THE definition), the radii fit and the
writer.  den and M against the independent numpy restatement of the rule (tests/hbt_cases.py), exactly; closed forms; and physics that the
restatement cannot vouch for: Gaussian sources of known size, through the whole chain list -> histograms -> fit."""
import os

import numpy as np
import pytest

import hbt_cases as H
from is3d_amd import api


@pytest.mark.parametrize("bins", (H.BINS, H.BINS_ODD, H.BINS_BIG), ids=("even", "odd", "big"))
def test_den_and_M_are_the_numpy_restatement_exactly(bins):
    p, n_events = H.hand_list()
    got = api.hbt_list(bins, n_events, 4, H.SLOT4, p)
    want = H.numpy_hist(bins, n_events, 4, H.SLOT4, p)
    assert H.same_counts(got, want) and H.num_within_one_unit_per_pair(got, want)
    assert got["den"].sum() > 100000 and got["M"][:7, 0].tolist() == list(H.HAND_SIZES) and got["M"][:, 2].sum() == 0
    # a segment of n accepted particles holds at most n (n - 1) ordered pairs
    assert got["den"].sum(axis=(1, 2, 3, 4)).tolist() <= (got["M"] * (got["M"] - 1)).sum(axis=0).tolist()


def test_all_particles_of_a_slot_at_one_point():
    """dx = 0 for every pair: phase = 0, cos = 1, num = den 2^32 in every bin, whatever the momenta."""
    p, n_events = H.hand_list()
    q = p.copy()
    for k, v in (("t", 1.5), ("x", -2.0), ("y", 0.25), ("z", 3.0)):
        q[k] = v
    got = api.hbt_list(H.BINS, n_events, 4, H.SLOT4, q)
    assert got["den"].sum() > 100000 and np.array_equal(got["num"], got["den"] * 2 ** 32)


def test_the_order_of_the_list_does_not_matter():
    """Every ordered pair (i, j) comes with (j, i), which the rule bins on its own (q -> -q: the mirrored bin up to the rounding of the bin
    rule, which is why no implementation may mirror instead of computing); a shuffle or a reversal of the list swaps the roles of i and j
    and changes nothing, num included, because the sums are integers."""
    p, n_events = H.hand_list()
    q, _ = H.shuffled_list()
    a, b, c = (api.hbt_list(H.BINS, n_events, 4, H.SLOT4, x) for x in (p, q, p[::-1]))
    assert all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]) for k in a)
    # ... and the mirror is NOT exact: the two ordered pairs of the particles of equal momentum (q = 0, the last event) both land in bin
    # n_q / 2 of each direction, whose mirror n_q / 2 - 1 they leave empty
    last = p[p["event"] == n_events - 1]
    d = api.hbt_list(H.BINS, n_events, 4, H.SLOT4, last)["den"]
    assert d.sum() == 2 and d[0, :, 4, 4, 4].sum() == 2 and d[0, :, 3, 3, 3].sum() == 0


def test_pieces_of_one_event_are_not_additive():
    """The pairs across two pieces of an event are in neither piece: den of the whole exceeds the sum over pieces by exactly the cross pairs.
    Whole events are additive."""
    p, n_events = H.hand_list()
    ev = p[p["event"] == 5]                               # 65 + 65 accepted particles in two slots
    half = len(ev) // 2
    whole, a, b = (api.hbt_list(H.BINS, n_events, 4, H.SLOT4, x) for x in (ev, ev[:half], ev[half:]))
    assert np.array_equal(whole["M"], a["M"] + b["M"])
    assert whole["den"].sum() > (a["den"] + b["den"]).sum() and np.all(whole["den"] >= a["den"] + b["den"])
    lo, hi = p[p["event"] < 5], p[p["event"] >= 5]
    full, x, y = (api.hbt_list(H.BINS, n_events, 4, H.SLOT4, z) for z in (p, lo, hi))
    assert all(np.array_equal(full[k], x[k] + y[k]) for k in full)


def test_the_fit_returns_the_radii_of_an_exact_gaussian():
    bins = dict(H.BINS, n_kT=2, n_q=9)
    nq, dq = 9, 2.0 * bins["q_max"] / 9
    c = -bins["q_max"] + (np.arange(nq) + 0.5) * dq
    QO, QS, QL = np.meshgrid(c, c, c, indexing="ij")
    R2 = (4.0, 9.0, 2.25, 1.5, -0.5, 0.75)
    cc = 0.8 * np.exp(-(R2[0] * QO ** 2 + R2[1] * QS ** 2 + R2[2] * QL ** 2 + 2 * R2[3] * QO * QS + 2 * R2[4] * QO * QL + 2 * R2[5] * QS * QL) / H.HBARC ** 2)
    den = np.zeros((2, 2, nq, nq, nq), np.int64)
    den[1, 0] = 1000
    den[0, 1, :2, :2, :1] = 1000                          # 4 bins: fewer than the 7 unknowns
    num = np.rint(den * cc * 2.0 ** 32).astype(np.int64)
    r = api.hbt_radii(bins, dict(num=num, den=den, M=np.zeros((1, 2), np.int64)), min_pairs=10, c_min=1e-9)
    assert r["singular"].tolist() == [[1, 1], [0, 1]] and r["n_bins"].tolist() == [[0, 4], [nq ** 3, 0]]
    assert abs(r["lambda"][1, 0] - 0.8) < 1e-7 and np.allclose(r["R2"][1, 0], R2, rtol=0, atol=1e-6)
    assert not r["R2"][0].any() and not r["lambda"][0].any()
    # min_pairs and c_min select: only the bins with c >= 0.3 are used, and the exact Gaussian still gives its radii
    r = api.hbt_radii(bins, dict(num=num, den=den, M=np.zeros((1, 2), np.int64)), min_pairs=1000, c_min=0.3)
    assert r["n_bins"][1, 0] == int((cc >= 0.3).sum()) < nq ** 3 and np.allclose(r["R2"][1, 0], R2, rtol=0, atol=1e-5)
    assert api.hbt_radii(bins, dict(num=num, den=den, M=np.zeros((1, 2), np.int64)), min_pairs=1001, c_min=0.3)["singular"].all()


@pytest.fixture(scope="module")
def sources():
    """The host route on the two Gaussian sources of seed PHYS_SEEDS[0], once."""
    out = {}
    for name, bins, make in (("T", H.PHYS_T, H.transverse_source), ("Z", H.PHYS_Z, H.longitudinal_source)):
        p = make(H.PHYS_SEEDS[0])
        out[name] = api.hbt_list(bins, H.PHYS_EVENTS, 1, [0], p)
    return out


def test_a_transverse_gaussian_source_gives_its_radii(sources):
    """Physics the restatement cannot vouch for.  pi+ with thermal-like momenta, t = z = 0, x, y ~ N(0, SIGMA_T = 1.5 fm): the fit must
    give R_o^2 = R_s^2 = SIGMA_T^2 = 2.25 fm^2, R_l^2 = R_os^2 = R_ol^2 = R_sl^2 = 0 and lambda = 1.  Tolerance: 5 standard deviations of
    the host route over the 8 seeds PHYS_SEEDS at this list size (40 events x 400 particles, 562 606 pairs in 1331 bins), measured:
        lambda 0.0009, R_o^2 0.0365, R_s^2 0.0253, R_l^2 0.0107, R_os^2 0.0066, R_ol^2 0.0036, R_sl^2 0.0075 (fm^2)
    The means over those seeds were lambda 0.9962, R_o^2 2.204, R_s^2 2.218: the log-linear estimator is biased low by about 2 % at this
    bin width and pair count (c averaged over a bin, weights from the measured c), inside the tolerance."""
    h = sources["T"]
    assert H.core_bins_filled(H.PHYS_T, h, H.SIGMA_T) >= 0.5                        # the condition on the list
    lam, R2 = H.fit(H.PHYS_T, h)
    print("transverse source: lambda %.4f, R2 %s" % (lam, np.round(R2, 4)))
    tol = 5.0 * np.array(H.PHYS_STD_T)
    assert abs(lam - 1.0) <= tol[0]
    want = (H.SIGMA_T ** 2, H.SIGMA_T ** 2, 0.0, 0.0, 0.0, 0.0)
    assert np.all(np.abs(R2 - want) <= tol[1:]), (R2, tol)


def test_a_longitudinal_gaussian_source_gives_its_radius(sources):
    """x = y = t = 0, z ~ N(0, SIGMA_Z = 2.5 fm), y_cut = 0.05: the phase is -q_z dz with the lab q_z, which lies between q_l and
    q_l cosh(y) for |y| <= 0.05, so R_l^2 must lie in [SIGMA_Z^2, cosh^2(0.05) SIGMA_Z^2] = [6.25, 6.266] fm^2, R_o^2 = R_s^2 = 0 and the
    cross terms vanish.  Tolerance beyond that interval: 5 standard deviations over PHYS_SEEDS (1 461 462 pairs in 3375 bins), measured:
        lambda 0.0006, R_o^2 0.0054, R_s^2 0.0101, R_l^2 0.1022, R_os^2 0.0059, R_ol^2 0.0239, R_sl^2 0.0156 (fm^2)
    The mean of R_l^2 over those seeds was 6.133 (the same 2 % of the estimator)."""
    h = sources["Z"]
    assert H.core_bins_filled(H.PHYS_Z, h, H.SIGMA_Z) >= 0.5
    lam, R2 = H.fit(H.PHYS_Z, h)
    print("longitudinal source: lambda %.4f, R2 %s" % (lam, np.round(R2, 4)))
    tol = 5.0 * np.array(H.PHYS_STD_Z)
    assert abs(lam - 1.0) <= tol[0]
    assert H.SIGMA_Z ** 2 - tol[3] <= R2[2] <= np.cosh(0.05) ** 2 * H.SIGMA_Z ** 2 + tol[3]
    assert np.all(np.abs(R2[[0, 1, 3, 4, 5]]) <= tol[[1, 2, 4, 5, 6]]), (R2, tol)


def test_the_measured_spreads_are_those_of_the_host_route():
    """The standard deviations the two tests above allow five of, measured again over three of the seeds: the same order of magnitude (a
    guard against a list or bins changed without measuring again)."""
    rows = []
    for seed in H.PHYS_SEEDS[:3]:
        lam, R2 = H.fit(H.PHYS_T, api.hbt_list(H.PHYS_T, H.PHYS_EVENTS, 1, [0], H.transverse_source(seed)))
        rows.append([lam] + list(R2))
    sd = np.std(np.array(rows), axis=0, ddof=1)
    assert np.all(sd < 6.0 * np.array(H.PHYS_STD_T)), sd


def test_writer(tmp_path):
    p, n_events = H.hand_list()
    bins = dict(H.BINS, n_kT=2)
    h = api.hbt_list(bins, n_events, 4, H.SLOT4, p)
    with pytest.raises(api.Is3dError) as e:
        api.write_hbt(str(tmp_path), bins, h, ["a", "b", "c", "d"])
    assert e.value.code == api.IS3D_EIO and "hbt/" in str(e.value)
    os.makedirs(tmp_path / "hbt")
    for labels in (["a", "", "c", "d"], ["a", "b/c", "c", "d"]):
        with pytest.raises(api.Is3dError) as e:
            api.write_hbt(str(tmp_path), bins, h, labels)
        assert e.value.code == api.IS3D_EINVAL
    api.write_hbt(str(tmp_path), bins, h, ["211", "-211", "321", "-321"], min_pairs=20, c_min=0.05)
    names = sorted(os.listdir(tmp_path / "hbt"))
    assert names == sorted(["correlation_%s_kT%d.dat" % (l, k) for l in ("211", "-211", "321", "-321") for k in (0, 1)] +
                           ["radii_%s.dat" % l for l in ("211", "-211", "321", "-321")])
    rows = np.loadtxt(tmp_path / "hbt" / "correlation_-211_kT1.dat")
    assert rows.shape == (8 ** 3, 5) and np.array_equal(rows[:, 3].astype(np.int64), h["den"][1, 1].ravel())
    filled = h["den"][1, 1].ravel() > 0
    c = h["num"][1, 1].ravel()[filled] / (h["den"][1, 1].ravel()[filled] * 2.0 ** 32)
    assert np.allclose(rows[filled, 4], 1.0 + c, rtol=0, atol=2e-8) and np.all(rows[~filled, 4] == 1.0)
    dq = 2 * bins["q_max"] / 8
    assert np.allclose(rows[:8, 2], -bins["q_max"] + (np.arange(8) + 0.5) * dq, rtol=1e-8) and np.all(rows[:64, 0] == rows[0, 0])
    head = open(tmp_path / "hbt" / "correlation_-211_kT1.dat").read().split("\n")[1]
    assert head.endswith("pairs: %d" % h["den"][1, 1].sum())
    rad = np.loadtxt(tmp_path / "hbt" / "radii_-211.dat")
    want = api.hbt_radii(bins, h, 20, 0.05)
    assert rad.shape == (2, 10) and np.allclose(rad[:, 1], want["lambda"][1], rtol=1e-8) and np.allclose(rad[:, 2:8], want["R2"][1], rtol=1e-8, atol=1e-12)
    assert rad[:, 8].tolist() == want["n_bins"][1].tolist() and rad[:, 9].tolist() == want["singular"][1].tolist()
