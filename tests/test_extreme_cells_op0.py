"""CPU: the operation-0 fixture on the extreme cells (tests/golden/golden_extreme_op0.npz, .json, made by
tests/golden/make_golden_extreme_op0.py; the table, weights and bins in tests/extreme_cells.py, references and metric in
tests/extreme_cells_op0.py) -- that the inputs are fit for purpose before any device sees them.

For every committed case the double reference (the oracle's spectrum of one cell at a time; tests/dndx_feqmod_ref.py for the modified
equilibrium) is finite and within 1e-9 -- the bound of tests/test_extreme_cells.py, half the device tolerance -- of the long-double D, per
(species, pT node, cell) against max(|D|, 1e-280); the raw delta-f cases (outflow = 0, regulate_deltaf = 0) against the cancellation-aware
scale of tests/test_gpu_fuzz.py taken per cell and node.  Anisotropic hydro with regulate_deltaf = 0 holds the PLAIN relative bound on the
CPU (worst 9.5e-12, fast-flow 3+1D) and is judged by it, like regulate_deltaf = 1.  The 2+1D dN/dy deta partials are held the same way.

A case proves little unless most of it is alive: every case has at least half of its 1 080 entries above the 1e-280 floor (the least: 646,
delta-f fast-flow 3+1D df_mode 1) and every pT node at least one (the least: 94).  No seed or grid of the table had to change for that.

Worst double-reference errors at generation: delta-f 2.8e-11 (fast-flow 3+1D df_mode 1), baryon 2.5e-12, anisotropic hydro 9.5e-12,
modified equilibrium 9.3e-10 (large-stress 3+1D df_mode 4, whose matrix is near singular on the narrow cells: det A ~ 1e-3 carries the double
inverse's rounding into E_mod; the next is 2.4e-10).  Nothing touches a GPU."""
import os
import sys

import numpy as np
import pytest

import extreme_cells as X
import extreme_cells_op0 as O

TOL_DOUBLE = 1e-9
CASES = X.fixture_op0_cases()
IDS = [c["key"] for c in CASES]


def generator():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if here not in sys.path:
        sys.path.insert(0, here)
    import make_golden_extreme_op0 as G
    return G


def test_the_fixture_covers_the_cases_of_the_spectrum_fixture():
    arrays, meta = X.fixture_op0()
    assert meta["n_cells"] == X.N_CELLS and meta["species"] == X.species_ids() and tuple(meta["eta_nodes"]) == X.ETA_NODES
    assert IDS == [c["key"] for c in X.fixture_cases()]
    for c, src in zip(CASES, X.fixture_cases()):
        assert all(c[k] == src[k] for k in ("family", "case", "dim", "cells", "opts")), c["key"]
        assert arrays[c["key"]].shape == (5, 6, X.N_CELLS) and arrays[c["key"]].dtype == np.float64
        assert ((c["key"] + "_eta") in arrays) == (c["dim"] == 2)
        if c["dim"] == 2:
            assert arrays[c["key"] + "_eta"].shape == (5, len(X.ETA_NODES))
    assert len(arrays) == len(CASES) + sum(c["dim"] == 2 for c in CASES)
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, "golden_extreme_op0.npz")) < os.path.getsize(os.path.join(here, "golden_extreme.npz"))


def test_the_weights_and_bins_are_what_the_docstrings_say():
    phi_w, pT_w = X.op0_weights()
    assert phi_w.shape == (9,) and (phi_w > 0).all() and len(set(phi_w)) == 9
    assert tuple(pT_w) == X.PT_W_NAMES and np.array_equal(pT_w["ones"], np.ones(6))
    assert np.array_equal(np.stack([pT_w["e%d" % i] for i in range(6)]), np.eye(6))
    D = X.fixture_op0()[0][IDS[0]]
    assert np.array_equal(O.weighted(D, "ones"), D.sum(axis=1)) and np.array_equal(O.weighted(D, "e4"), D[:, 4, :])
    for case in ("tau-extremes", "fast-flow"):
        for dim in (3, 2):
            c = X.surface(case, dim)
            b = X.op0_bins(c)
            assert (c["tau"] < b["tau_min"]).any() and (c["tau"] >= b["tau_max"]).any() and (np.hypot(c["x"], c["y"]) >= b["r_max"]).any()
            if case == "tau-extremes":
                assert (c["tau"][0::2] < b["tau_min"]).all() and (c["tau"][1::2] >= b["tau_max"]).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_double_reference_reproduces_the_long_double_values(case):
    arrays = X.fixture_op0()[0]
    D, eta = arrays[case["key"]], arrays.get(case["key"] + "_eta")
    assert np.isfinite(D).all()
    live = np.abs(D) > O.FLOOR
    assert int(live.sum()) == case["n_live"] and 2 * case["n_live"] >= D.size, (case["n_live"], D.size)
    assert [int(x) for x in live.sum(axis=(0, 2))] == case["n_live_per_node"] and min(case["n_live_per_node"]) >= 1
    got_D, got_eta = O.double_reference(case)
    assert np.isfinite(got_D).all()
    sD, sE = O.scales(case, D, eta)
    err = O.error(got_D, D, sD)
    if eta is not None:
        assert np.isfinite(eta).all() and np.isfinite(got_eta).all() and (np.abs(eta) > O.FLOOR).all()
        err = max(err, O.error(got_eta, eta, sE))
    print("%s: double reference against long double %.3e (at generation %.3e)" % (case["key"], err, case["ref_err"]))
    assert err < TOL_DOUBLE and case["ref_err"] < TOL_DOUBLE
    cells = X.fixture_cells(case["cells"])
    if case["family"] == "vah":
        assert (case["n_skipped"], case["n_breakdown"], case["n_renorm_skipped"]) == (0, 0, 0)      # (this path skips no cell)
    else:
        dead = np.flatnonzero(~X.live(cells))
        assert case["n_skipped"] == len(dead) == len(X.expected_skipped(case["case"])) and (D[:, :, dead] == 0.0).all()
        assert case["n_renorm_skipped"] == 0
    if case["family"] == "fq":
        assert O.feqmod_reference(cells, case["opts"], np.float64)[2] == {k: case[k] for k in ("n_skipped", "n_breakdown", "n_renorm_skipped")}
    else:
        assert case["n_breakdown"] == 0


def test_breakdown_cells_are_reached():
    by_key = {c["key"]: c for c in CASES}
    for name in X.NARROW_CASES:
        for dim in (3, 2):
            assert by_key["fq_%s_%d_mode3" % (name, dim)]["n_breakdown"] >= 3 and by_key["fq_%s_%d_mode4" % (name, dim)]["n_breakdown"] == 0


@pytest.mark.parametrize("key", ["df_fast-flow_3_df1_raw", "fq_large-stress_3_mode4", "fq_isothermal-mix_2_mode3", "vah_anisotropy_2_reg0"])
def test_the_generator_regenerates_a_committed_case(key):
    case = next(c for c in CASES if c["key"] == key)
    with np.errstate(over="ignore", under="ignore"):
        D, eta, counts = generator().longdouble_reference(case)
    arrays = X.fixture_op0()[0]
    assert np.array_equal(D.astype(np.float64), arrays[key])
    if eta is not None:
        assert np.array_equal(eta.astype(np.float64), arrays[key + "_eta"])
    assert counts == {k: case[k] for k in counts}
