"""CPU: the extreme-cell table (tests/extreme_cells.py) and its committed long-double fixture (tests/golden/golden_extreme.npz, .json, made by
tests/golden/make_golden_extreme.py) -- that the inputs are fit for purpose before any device sees them.  For every committed case the oracle
is finite and within 1e-9 of the long-double spectrum (half the device tolerance of tests/test_gpu_extreme_cells.py; relerr's floor of 1e-280;
the raw cases, outflow = 0 and regulate_deltaf = 0, against the cancellation-aware scale of tests/test_gpu_fuzz.py), and the cases reach what
they were built to reach: mostly non-zero bins, exact zeros in far-eta, the clamp |delta-f| = 1 on most terms of large-stress in both signs,
breakdown cells of df_mode 3 and narrow rows in large-stress and table-edge-T with the oracle's breakdown count equal to the restatement's,
exactly the skipped cells of isothermal-mix, and no domain error anywhere.  The seeds of the table were tuned here.  Nothing touches a GPU."""
from functools import lru_cache

import numpy as np
import pytest

import extreme_cells as X
from is3d_amd import inputs
from oracle import oracle

TOL_ORACLE = 1e-9
CASES = X.fixture_cases()
IDS = [c["key"] for c in CASES]


@lru_cache(maxsize=None)
def df_tables(baryon):
    return inputs.df_tables_full() if baryon else inputs.df_tables()


def fq_for(cells):
    return inputs.feqmod_tables(inputs.surface_average_T(cells))


@lru_cache(maxsize=None)
def raw_scale(key):
    """tests/test_gpu_fuzz.py: max(|ref|, 1e-4 (pos + neg)) -- what was added up, from two oracle runs with the cut (dsigma as it is and negated)"""
    case = next(c for c in CASES if c["key"] == key)
    cells, ref = X.fixture_cells(case["cells"]), X.fixture()[0][key]
    o = dict(case["opts"], outflow=1, regulate_deltaf=1)
    pos = oracle.dN_pTdpTdphidy(cells, X.species(), X.grid(), df_tables(False), o)
    neg = oracle.dN_pTdpTdphidy({k: (-v if k in X.H.DS else v) for k, v in cells.items()}, X.species(), X.grid(), df_tables(False), o)
    s = np.maximum(np.abs(ref), 1e-4 * (pos + neg))
    s.setflags(write=False)
    return s


def scale_of(case):
    """the size a bin's error is judged against: |ref|, for the raw delta-f cases raw_scale; never below relerr's floor"""
    ref = X.fixture()[0][case["key"]]
    raw = case["family"] == "df" and not case["opts"].get("outflow", 1)
    return np.maximum(raw_scale(case["key"]) if raw else np.abs(ref), 1e-280)


def error(got, case):
    return float(np.max(np.abs(got - X.fixture()[0][case["key"]]) / scale_of(case)))


def oracle_run(case):
    """-> (spectrum, breakdown count or None); a domain error of the oracle surfaces as RuntimeError"""
    cells, o = X.fixture_cells(case["cells"]), case["opts"]
    if case["family"] == "fq":
        return oracle.dN_pTdpTdphidy_feqmod(cells, X.species(), X.grid(), df_tables(False), fq_for(cells), o)
    if case["family"] == "vah":
        return oracle.dN_pTdpTdphidy_vah(cells, X.species(), X.grid(), o), None
    return oracle.dN_pTdpTdphidy(cells, X.species(), X.grid(), df_tables(case["family"] == "dfb"), o), None


def test_the_table_is_what_the_docstring_says():
    assert X.N_CELLS == 36 and X.fixture()[1]["n_cells"] == 36 and X.fixture()[1]["species"] == X.species_ids()
    g = X.grid()
    assert (len(g["phi"]), len(g["y"]), len(g["pT"])) == (9, 8, 6) and len(g["eta"]) == 241
    assert g["y"][0] == -5.0 and g["y"][-1] == 5.0 and np.isclose(g["pT"][0], 0.05) and np.isclose(g["pT"][-1], 40.0)
    T0, T1 = X.table_T()
    for dim in (3, 2):
        b = X.H.base(dim, seed=6100)
        c = X.surface("fast-flow", dim)
        rho = np.arcsinh(np.hypot(c["ux"], c["uy"]))
        assert rho.min() >= 1.0 and 3.0 < rho.max() <= 3.7
        if dim == 3:
            assert np.abs(np.arcsinh(c["tau"] * c["un"] / np.sqrt(1 + c["ux"] ** 2 + c["uy"] ** 2))).max() <= 2.0 + 1e-12
        c = X.surface("table-edge-T", dim)
        assert ((c["T"][0::2] > T0) & (c["T"][0::2] <= T0 + 1e-3)).all() and ((c["T"][1::2] < T1) & (c["T"][1::2] >= T1 - 1e-3)).all()
        c = X.surface("large-stress", dim)
        keep = np.setdiff1d(np.arange(X.N_CELLS), X.NARROW if dim == 3 else [])
        assert np.array_equal(c["pixx"][keep], 25.0 * b["pixx"][keep]) and np.array_equal(c["piyy"][keep], 25.0 * b["piyy"][keep])
        ke, ko = keep[keep % 2 == 0], keep[keep % 2 == 1]
        assert np.array_equal(c["bulkPi"][ke], -0.9 * c["P"][ke]) and np.array_equal(c["bulkPi"][ko], 0.5 * c["P"][ko])
        c = X.surface("tau-extremes", dim)
        assert ((c["tau"][0::2] >= 0.05) & (c["tau"][0::2] <= 0.055)).all() and ((c["tau"][1::2] >= 50.0) & (c["tau"][1::2] <= 55.0)).all()
        c = X.surface("isothermal-mix", dim)
        corona = np.array(sorted(X.CORONA))
        assert np.array_equal(c["T"][corona], [X.CORONA[i] for i in corona]) and (np.delete(c["T"], corona) == X.T_ISO).all()
        assert np.array_equal(c["dat"][0::5], -b["dat"][0::5]) and np.array_equal(np.delete(c["dat"], np.arange(0, 36, 5)), np.delete(b["dat"], np.arange(0, 36, 5)))
        if dim == 3:
            assert (np.abs(c["eta"]) <= 6.0).all() and np.abs(c["eta"]).max() > 5.5 and (c["eta"] > 4.0).any() and (c["eta"] < -4.0).any() and (np.abs(c["eta"]) < 2.5).mean() > 0.5
        f = c["pixx"] / b["pixx"]
        assert f.min() >= 1.0 - 1e-12 and f.max() <= 25.0 + 1e-9 and f.max() / f.min() > 5.0
        v = X.surface("anisotropy", dim, vah=True)
        tab = inputs.vah_df_tables()
        L = v["Lambda"] / X.HBARC
        assert (v["aL"] >= tab["aL"][0]).all() and (v["aL"] <= tab["aL"][-1]).all() and (L >= tab["L"][0]).all() and (L <= tab["L"][-1]).all()
        assert (v["aL"][:2] - tab["aL"][0] <= 1e-3).all() and (tab["aL"][-1] - v["aL"][2:4] <= 1e-3).all()
        assert (L[:2] - tab["L"][0] <= 1e-3 + 1e-12).all() and (tab["L"][-1] - L[2:4] <= 1e-3 + 1e-12).all()
        assert v["aL"].max() - v["aL"].min() > 1.5 and L.max() - L.min() > 0.5
        m = X.surface("muB-edge", dim, baryon=True)
        last = df_tables(True)["muB"][-1]
        assert (m["muB"][0::2] == 0.0).all() and ((m["muB"][1::2] < last) & (m["muB"][1::2] >= last - 1e-3)).all()
        assert np.array_equal(m["nB"], 10.0 * X.H.base(dim, baryon=True, seed=6100)["nB"])
        # dsigma is touched by no case but isothermal-mix
        for case in X.CASES:
            if dim in X.DIMS[case] and case not in ("isothermal-mix", "anisotropy", "muB-edge"):
                for f in X.H.DS:
                    assert np.array_equal(X.surface(case, dim)[f], b[f]), (case, f)
    c = X.surface("far-eta", 3)
    assert (np.abs(c["eta"]) >= 4.0).all() and (np.abs(c["eta"]) <= 7.0).all() and (c["eta"] > 0).any() and (c["eta"] < 0).any()
    # a VAH cell's dependent components are those of its new flow and stress: orthogonal to u
    v = X.surface("fast-flow", 3, vah=True)
    ut = np.sqrt(1 + v["ux"] ** 2 + v["uy"] ** 2 + v["tau"] ** 2 * v["un"] ** 2)
    res = v["pitx"] * ut - v["pixx"] * v["ux"] - v["pixy"] * v["uy"] - v["tau"] ** 2 * v["pixn"] * v["un"]
    assert np.abs(res).max() <= 1e-10 * np.abs(v["pitx"] * ut).max()


def test_the_committed_cells_are_the_tables():
    seen = set()
    for case in CASES:
        tag = case["cells"]
        if tag in seen:
            continue
        seen.add(tag)
        got = X.fixture_cells(tag)
        want = X.surface(case["case"], case["dim"], vah=tag.endswith("v"), baryon=tag.endswith("b"))
        for k, v in got.items():
            if not (tag.endswith("v") and k in ("c0", "c1", "c2", "c3", "c4")):     # (the fixture's come from scipy's interpolator)
                assert np.array_equal(v, want[k]), (tag, k)
    assert len(seen) == sum(len(X.DIMS[c]) for c in X.VISCOUS_CASES + X.VAH_CASES + X.BARYON_CASES)


def test_every_family_and_flag_of_the_issue_is_committed():
    keys = set(IDS)
    for case in X.VISCOUS_CASES:
        for dim in X.DIMS[case]:
            assert {"df_%s_%d_df%d_%s" % (case, dim, m, f) for m in (1, 2) for f in ("std", "raw")} <= keys
            assert {"fq_%s_%d_mode%d" % (case, dim, m) for m in (3, 4)} <= keys
    for case in X.VAH_CASES:
        for dim in X.DIMS[case]:
            assert {"vah_%s_%d_reg%d" % (case, dim, r) for r in (0, 1)} <= keys
    for dim in (3, 2):
        assert {"dfb_muB-edge_%d_df%d_diff%d" % (dim, m, d) for m in (1, 2) for d in (0, 1)} <= keys


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_reproduces_the_long_double_spectrum(case):
    ref = X.fixture()[0][case["key"]]
    assert np.isfinite(ref).all()
    assert np.count_nonzero(ref) > 0.5 * ref.size, (np.count_nonzero(ref), ref.size)
    got, nb = oracle_run(case)                      # (a domain error would raise here)
    assert np.isfinite(got).all()
    err = error(got, case)
    print("%s: oracle against long double %.3e (at generation %.3e)" % (case["key"], err, case["oracle_err"]))
    assert err < TOL_ORACLE
    if case["family"] == "fq":
        assert nb == case["n_breakdown"] == case["n_breakdown_oracle"]
        assert case["n_renorm_dropped"] == 0
    if "n_skipped" in case:
        cells = X.fixture_cells(case["cells"])
        assert case["n_skipped"] == int((~X.live(cells)).sum()) == len(X.expected_skipped(case["case"]))


def test_far_eta_holds_exact_zeros():
    for case in CASES:
        if case["case"] == "far-eta":
            assert (X.fixture()[0][case["key"]] == 0.0).any(), case["key"]


def test_the_clamp_acts_on_most_of_large_stress_in_both_signs():
    n = 0
    for case in CASES:
        if case["case"] == "large-stress" and case["family"] == "df" and case["opts"].get("regulate_deltaf", 1):
            hi, lo, terms = case["n_clamp_hi"], case["n_clamp_lo"], case["n_terms"]
            assert terms > 0 and hi + lo > 0.5 * terms and hi > 0.1 * terms and lo > 0.1 * terms, case["key"]
            n += 1
    assert n == 4


@pytest.mark.parametrize("name", X.NARROW_CASES)
def test_breakdown_cells_and_narrow_rows(name):
    by_key = {c["key"]: c for c in CASES}
    for dim in (3, 2):
        assert by_key["fq_%s_%d_mode3" % (name, dim)]["n_breakdown"] >= 3
        assert by_key["fq_%s_%d_mode4" % (name, dim)]["n_breakdown"] == 0          # df_mode 4 knows no breakdown
    m4 = by_key["fq_%s_3_mode4" % name]
    assert m4["n_narrow_rows"] >= 1 and m4["n_narrow_cells"] >= m4["n_narrow_rows"]


def test_isothermal_mix_skips_the_cells_the_construction_says():
    for dim in (3, 2):
        lv = X.live(X.surface("isothermal-mix", dim))
        assert np.array_equal(np.flatnonzero(~lv), X.expected_skipped("isothermal-mix"))
    for case in X.CASES:
        if case != "isothermal-mix":
            for dim in X.DIMS[case]:
                assert X.live(X.surface(case, dim, vah=case == "anisotropy", baryon=case == "muB-edge")).all(), (case, dim)


@pytest.mark.parametrize("dim", [3, 2])
def test_the_exact_node_cells_are_inside_the_table_for_the_oracle(dim):
    """T exactly on the first and on the last node: the oracle's spline takes both (a value, no domain error); the device must do the same
    (tests/test_gpu_extreme_cells.py)"""
    cells = X.exact_nodes(dim)
    assert tuple(cells["T"]) == X.table_T()
    for dfm in (1, 2):
        assert np.isfinite(oracle.dN_pTdpTdphidy(cells, X.species(), X.grid(), df_tables(False), dict(dimension=dim, df_mode=dfm))).all()
    for dfm in (4, 3):
        got, _ = oracle.dN_pTdpTdphidy_feqmod(cells, X.species(), X.grid(), df_tables(False), fq_for(cells), dict(dimension=dim, df_mode=dfm))
        assert np.isfinite(got).all()


def make_golden():
    import os
    import sys
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if here not in sys.path:
        sys.path.insert(0, here)
    import make_golden as MG
    return MG


def test_the_extended_restatement_gives_the_old_fixture_bit_for_bit(fx, pins):
    """highprec_feqmod with its new branches on the benign cells of golden_highprec.npz (no branch is taken there): the committed arrays, every bit"""
    import os
    from is3d_amd import synth
    MG = make_golden()
    hp = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_highprec.npz"))
    n = 0
    for case in pins["highprec_cases"]:
        if case.get("feqmod"):
            cells = {k: hp["cells_%s_%s" % (case["cells"], k)] for k in synth.CELL_FIELDS}
            with np.errstate(over="ignore"):
                got, counts = MG.highprec_feqmod(cells, fx["pikp"], fx["grid"], fx["df"], fq_for(cells), case["opts"])
            assert np.array_equal(got.astype(np.float64), hp[case["key"]]), case["key"]
            assert not any(counts.values()), counts
            n += 1
    assert n == 4


@pytest.mark.parametrize("key", ["fq_table-edge-T_3_mode4", "fq_large-stress_3_mode3", "fq_isothermal-mix_2_mode3"])
def test_the_restatement_regenerates_a_committed_spectrum(key):
    """narrow rows (df_mode 4), 34 breakdown cells of 36, skipped cells with the 2+1D eta scale: the generator's bits and counts"""
    case = next(c for c in CASES if c["key"] == key)
    cells = X.fixture_cells(case["cells"])
    with np.errstate(over="ignore", under="ignore"):
        got, counts = make_golden().highprec_feqmod(cells, X.species(), X.grid(), df_tables(False), fq_for(cells), case["opts"])
    assert np.array_equal(got.astype(np.float64), X.fixture()[0][key])
    assert (counts["breakdown"], counts["narrow_cells"], counts["narrow_rows"], counts["skipped"]) == (
        case["n_breakdown"], case["n_narrow_cells"], case["n_narrow_rows"], case["n_skipped"])
