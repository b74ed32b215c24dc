"""CPU: the integer histograms of the test_sampler = 1 distributions (is3d_sampler_bin_list, the host side of the one bin rule in
csrc/cf_sampler_bins.h) against a numpy restatement of sample_dN_dy ... sample_dN_dX (sampling_kernels.cpp:31-152), and the histogram
writer (is3d_write_sampler_tests_binned) against the list writer, on a hand-made list with particles on and beside every kind of edge."""
import os

import numpy as np
import pytest

from is3d_amd import api

from sampler_bins_ref import BINS, IDS, K_NAN, K_Y, N_EVENTS, NAN_FIELDS, log_decided, make_list, numpy_hist

DIRS = ("dN_dy", "dN_deta", "momentum_distribution", "vn", "spacetime_distribution")


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


def test_nan_rows_reach_no_bin_and_are_counted():
    """Each of the five NaN rows (E, px, tau, x, eta) stays out of the histograms its NaN feeds, adds to the others, and to the yield."""
    p, kinds = make_list(with_kinds=True)
    for i, f in enumerate(NAN_FIELDS):
        q = p[kinds == K_NAN + i]
        assert len(q) == 1 and np.isnan(q[f][0])
        got = api.sampler_bin_list(BINS, N_EVENTS, 3, q)
        want = numpy_hist(q, BINS, N_EVENTS, 3)
        sums = {k: int(got[k].sum()) for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield")}
        empty = dict(E=("dN_dy", "dN_pT", "dN_tau", "dN_r"), px=("dN_pT",), tau=("dN_tau",), x=("dN_r",), eta=("dN_deta",))[f]
        assert sums == {k: 0 if k in empty else 1 for k in sums}, (f, sums)
        assert all(np.array_equal(got[k], want[k]) for k in sums), f
        assert got["vn_re"].any() == ("dN_pT" not in empty)


def test_log_decided_particles_are_few_and_hand_made():
    """The split the device test makes (tests/test_gpu_sampler_bins_lists.py), checked where no device is needed: the particles whose rapidity
    bin or gate lies within 1e-12 of an edge in long double are 19 of the 2000 -- at most 2 % -- and every one is a row whose rapidity was put
    on or beside an edge by hand.  Away from them the long-double restatement and the C library's agree on every bin."""
    p, kinds = make_list(with_kinds=True)
    ref, u, d = numpy_hist(p, BINS, N_EVENTS, 3, longdouble=True)
    hard = log_decided(u, d)
    print("log-decided:", int(hard.sum()), "of", len(p))
    assert 0 < hard.sum() <= 0.02 * len(p) and (kinds[hard] == K_Y).all()
    assert hard.sum() == 19
    easy = p[~hard]
    a, b = numpy_hist(easy, BINS, N_EVENTS, 3), numpy_hist(easy, BINS, N_EVENTS, 3, longdouble=True)[0]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    got = api.sampler_bin_list(BINS, N_EVENTS, 3, easy)
    assert all(np.array_equal(got[k], a[k]) for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield"))


def test_empty_ranges_and_bad_counts_are_refused(tmp_path):
    """A zero-width or inverted range would divide by zero in the bin rule: IS3D_EINVAL from the host binning and from both writers."""
    p = make_list()
    hist = api.sampler_bin_list(BINS, N_EVENTS, 3, p)
    for bad in (dict(y_cut=0.0), dict(y_cut=-1.0), dict(eta_cut=0.0), dict(pT_upper_cut=BINS["pT_lower_cut"]), dict(pT_upper_cut=0.1),
                dict(tau_max=BINS["tau_min"]), dict(r_max=BINS["r_min"]), dict(r_max=0.0), dict(y_cut=float("nan")), dict(y_bins=0), dict(r_bins=-2)):
        b = dict(BINS, **bad)
        hb = hist if b["y_bins"] == BINS["y_bins"] and b["r_bins"] == BINS["r_bins"] else api._hist_arrays(b, N_EVENTS, 3)[1]
        calls = (lambda: api.sampler_bin_list(b, N_EVENTS, 3, p),
                 lambda: api.write_sampler_tests(str(tmp_path), b, N_EVENTS, IDS, p),
                 lambda: api.write_sampler_tests_binned(str(tmp_path), b, N_EVENTS, IDS, hb))
        for call in calls:
            with pytest.raises(api.Is3dError) as e:
                call()
            assert e.value.code == api.IS3D_EINVAL, bad
    assert not os.listdir(str(tmp_path))                     # refused before any file is opened
