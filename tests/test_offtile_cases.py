"""CPU: the off-tile case table (tests/offtile_cases.py) -- that it covers the branches it names, and that the references of its cases are
what tests/test_gpu_offtile.py's metrics need (finite, no value on the relative metric's floor, non-zero scales).  Conditions on the
references alone: nothing here touches a GPU."""
import os

import numpy as np
import pytest

import decays_restated as R
import dndx_feqmod_ref
import offtile_cases as OC
from is3d_amd import api
from oracle import oracle
from test_gpu_polarization import restate
from test_gpu_spacetime import oracle_cells


def ids(cases):
    return [c.name for c in cases]


# ---- the table covers what it claims ----
def test_operation_0_shapes_cover_the_targets():
    for cases, modes in ((OC.OP0_DF, {1, 2}), (OC.OP0_FQ, {3, 4})):
        d3 = [c for c in cases if c.dim == 3]
        d2 = [c for c in cases if c.dim == 2]
        assert {c.df_mode for c in d3} == {c.df_mode for c in d2} == modes
        assert {c.shape[0] for c in d3} >= {1, 3, 5, 33, 64} and {c.shape[0] for c in d2} >= {1, 3, 5, 33, 64}
        assert {c.shape[1] for c in d3} >= {1, 5, 7, 9, 13} and {c.shape[1] for c in d2} >= {1, 5, 7, 9, 13}
        assert {c.shape[2] for c in d3} >= {1, 6, 8, 15}
        assert {c.shape[2] for c in d2} >= {2, 30, 32, 33, 62, 63}
        assert {c.n_cells for c in cases} == {1, 2, 37}
        assert {c.opts.get("cell_chunks", 0) for c in cases} == {0, 3, 5}
        assert any(c.opts.get("cell_chunks", 0) > c.n_cells for c in cases)          # more chunks than cells
        der = [OC.op0_derived(c) for c in cases]
        assert {d["npTp"] for d in der} >= {1, 4, 8, 64}
        assert {d["nlw"] % 4 for d in der} >= {1, 2, 3} and any(d["nlw"] > 4 for d in der)
        for c, d in zip(cases, der):
            # every case is off-tile along phi, and along its rows too (a single node included: the rest of the tile is padding) but for
            # the 62 eta nodes, two whole 31-row blocks, which are there for the block count
            assert d["phi"][0] != 0 and (d["rows"][0] != 0 or c.shape[2] == 62), c.name
        assert any(c.opts.get("outflow", 1) == 0 for c in cases)
        assert all(len(c.species) <= 8 for c in cases)
        assert any(OC.n_classes(OC.inputs.species(c.species), 0) < len(c.species) for c in cases)   # a particle / antiparticle pair
    # both phi tile widths of the delta-f kernels leave a remainder somewhere, and the 241-node table runs once, with 5 pT values
    widths = {OC.op0_derived(c)["phi"][1] for c in OC.OP0_DF if OC.op0_derived(c)["phi"][0]}
    assert widths == {6, 8}
    assert [c.shape for c in OC.OP0_DF if c.dim == 2 and c.shape[2] == 241] == [(5, 9, 241)]
    for dim in (2, 3):
        assert {c.df_mode for c in OC.OP0_DF if c.dim == dim and c.opts.get("include_baryon")} == {1, 2}
    assert sum(c.breakdown for c in OC.OP0_FQ) >= 1 and all(c.df_mode == 3 for c in OC.OP0_FQ if c.breakdown)


def test_lds_bound_cases_sit_on_the_bound():
    """4 waves x (64 / npTp) classes x K doubles within 64 KiB (48 KiB for feqmod): the largest admitted eta count is a case that runs, one
    more is a refusal; 65 pT values are refused in both dimensions."""
    for npT in (1, 2):
        for fq, cap, cases in ((False, 65536, OC.OP0_DF), (True, 49152, OC.OP0_FQ)):
            per_eta = 8 * 4 * (64 // OC.npTp_of(npT))
            kmax = OC.op0_lds_max_eta(npT, fq)
            assert per_eta * kmax <= cap < per_eta * (kmax + 1)
            assert any(c.dim == 2 and c.shape[0] == npT and c.shape[2] == kmax for c in cases)
            assert any(dim == 2 and shape[0] == npT and shape[2] == kmax + 1 and (dfm >= 3) == fq for _, dim, shape, dfm in OC.OP0_REFUSED)
    assert {(dim, dfm >= 3) for _, dim, shape, dfm in OC.OP0_REFUSED if shape[0] == 65} >= {(3, False), (2, False), (3, True)}
    # no shape of the run tables is one the library refuses: a refusal is asserted as one (OP0_REFUSED), never skipped
    for c in OC.OP0_DF + OC.OP0_FQ:
        assert c.shape[0] <= 64 and (c.dim == 3 or c.shape[2] <= OC.op0_lds_max_eta(c.shape[0], c.df_mode >= 3)), c.name


def test_vah_operation_0_shapes_cover_the_targets():
    """every branch the table names, derived from the restated host rules (OC.vah_derived), not from the names"""
    cases = OC.OP0_VAH
    der = {c.name: OC.vah_derived(c) for c in cases}
    assert {d["npTp"] for d in der.values()} >= {1, 4, 8, 64}
    nlw = [d["nlw"] for d in der.values()] + [OC.vah_derived(c)["nlw"] for c in OC.OP0_VAH_MANY]   # (75 lane waves there: 18 workgroups + 3 waves)
    assert {w % 4 for w in nlw} >= {1, 2, 3} and any(w > 4 for w in nlw)
    full_rows = {3: {7, 14}, 2: {31, 62, 124}}   # the named full-block cases, the dead-row grids (whole blocks of dead rows) among them
    for dim in (3, 2):
        dc = [c for c in cases if c.dim == dim]
        assert {c.shape[0] for c in dc} >= {1, 3, 5, 33, 64} and {c.shape[1] for c in dc} >= {1, 5, 7, 9, 13}
        assert {der[c.name]["npTp"] for c in dc} >= {1, 64}
        assert any(der[c.name]["nlw"] % 4 and der[c.name]["nlw"] > 4 for c in dc)      # G > 1 with a partly filled last workgroup
        assert {c.opts.get("regulate_deltaf", 1) for c in dc} == {0, 1}
        assert {c.tab for c in dc} == {False, True}
        assert {c.n_cells for c in dc} == {1, 2, 37}
        assert any(der[c.name]["n_passes"] > 1 for c in dc)
        assert sorted(c.shape[2] for c in dc if der[c.name]["rows"][0] == 0) == sorted(full_rows[dim])
        assert sum(c.grid != "random" for c in dc) == 1
        for c in dc:
            # off-tile along phi, and along the rows but for the full-block cases (a single node included: the rest of the block is padding)
            assert der[c.name]["phi"][0] != 0, c.name
            assert der[c.name]["rows"][0] != 0 or c.shape[2] in full_rows[dim], c.name
            assert len(c.species) <= 8
            assert (der[c.name]["n_passes"] > 1) == bool(c.workspace), c.name
            # one cell per chunk in every pass: what tests/test_gpu_spacetime_vah.py reaches too
            assert der[c.name]["chunk_sizes"] == [1], c.name
    assert {c.shape[2] for c in cases if c.dim == 3} >= {1, 6, 7, 8, 14, 15}          # a single y, one full block, 7 + 1, two blocks, two + 1
    assert {c.shape[2] for c in cases if c.dim == 2} >= {2, 30, 31, 32, 33, 62, 63, 124, 241}
    assert any(OC.vah_n_classes(OC.vah_species(c.species)) < len(c.species) for c in cases)   # a particle / antiparticle pair
    # npTp = 1: no shuffle tree, 64 classes' slots per wave of which 3 are live
    for c in cases:
        if c.shape[0] == 1:
            assert der[c.name]["npTp"] == 1 and der[c.name]["ncls"] == 3 and der[c.name]["nlw"] == 1
    d = der["3d-npT33-phi13-y1-nlw5"]
    assert (d["npTp"], d["nlw"], (d["nlw"] + 3) // 4, d["nlw"] % 4) == (64, 5, 2, 1)   # G = 2, the second workgroup holds one wave


def test_vah_lds_bound_cases_sit_on_the_bound():
    """4 waves x (64 / npTp) classes x K doubles within 64 KiB: the largest admitted eta count runs, one more is refused; 65 pT values are
    refused in both dimensions; no run case is one the library refuses"""
    for npT in (1, 2):
        per_eta = 8 * 4 * (64 // OC.npTp_of(npT))
        kmax = OC.vah_lds_max_eta(npT)
        assert per_eta * kmax <= 65536 < per_eta * (kmax + 1)
        assert any(c.dim == 2 and c.shape[0] == npT and c.shape[2] == kmax for c in OC.OP0_VAH)
        assert any(dim == 2 and shape[0] == npT and shape[2] == kmax + 1 for _, dim, shape in OC.OP0_VAH_REFUSED)
    assert {dim for _, dim, shape in OC.OP0_VAH_REFUSED if shape[0] == 65} == {2, 3}
    for _, dim, shape in OC.OP0_VAH_REFUSED:
        assert shape[0] > 64 or (dim == 2 and shape[2] > OC.vah_lds_max_eta(shape[0]))
    for c in OC.OP0_VAH + OC.OP0_VAH_MANY:
        assert c.shape[0] <= 64 and (c.dim == 3 or c.shape[2] <= OC.vah_lds_max_eta(c.shape[0])), c.name


def test_vah_many_cell_cases_put_two_cells_in_a_chunk():
    """75 classes x 64 lane slots: nlw = 75, G = 19, 862 chunks; 1000 cells give chunks of 1 and of 2 cells by cf_st_vah_cells' c0 / c1, their
    halves one cell per chunk"""
    assert {c.dim for c in OC.OP0_VAH_MANY} == {2, 3} and {c.tab for c in OC.OP0_VAH_MANY} == {False, True}
    for c in OC.OP0_VAH_MANY:
        npT, nphi, nk = c.shape
        sp = OC.vah_species(c.species)
        ncls = OC.vah_n_classes(sp)
        assert ncls == len(sp["mass"]) == 75 == OC.vah_n_classes(OC.inputs.species("urqmd"))
        d = OC.vah_derived(c)
        assert (d["npTp"], d["nlw"], (d["nlw"] + 3) // 4) == (64, 75, 19) and d["n_passes"] == 1
        bounds = OC.vah_chunk_bounds(ncls, npT, c.n_cells, c.dim, nk)
        assert len(bounds) == 16384 // 19 == 862 and bounds[0][0] == 0 and bounds[-1][1] == c.n_cells
        assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
        assert OC.vah_cells_per_chunk(ncls, npT, c.n_cells, c.dim, nk) == d["chunk_sizes"] == [1, 2]
        assert sum(c1 - c0 == 2 for c0, c1 in bounds) == c.n_cells - 862
        assert OC.vah_cells_per_chunk(ncls, npT, c.n_cells // 2, c.dim, nk) == [1]
        assert OC.vah_cells_per_chunk(ncls, npT, c.n_cells - c.n_cells // 2, c.dim, nk) == [1]
        neg = OC.build_op0_vah(c)["neg"]
        subset, two = OC.vah_many_subset(c, neg)
        assert len(subset) <= 150 and len(two) >= 10 and neg in subset
        assert all(c0 in subset and c0 + 1 in subset and c1 == c0 + 2 for c0, c1 in two)
        assert all(k in subset for b in (bounds[0], bounds[-1]) for k in range(*b))


def test_mode_5_shapes_cover_the_targets():
    d3 = [c for c in OC.POLZN if c.dim == 3]
    d2 = [c for c in OC.POLZN if c.dim == 2]
    assert {c.shape[1] for c in d3} >= {1, 3, 5, 9} and {c.shape[2] for c in d3} >= {1, 2, 4, 7} and {c.shape[0] for c in d3} >= {1, 3, 33, 64}
    assert {c.shape[1] for c in d2} >= {1, 7, 9} and {c.shape[2] for c in d2} >= {2, 5, 33}
    der = {c.name: OC.polzn_derived(c) for c in OC.POLZN}
    assert {d["npTp"] for d in der.values()} >= {1, 4, 64}
    assert all(der[c.name]["phi"][0] != 0 for c in OC.POLZN)
    assert all(der[c.name]["rows"][0] != 0 for c in d3)
    assert {c.n_cells for c in OC.POLZN} == {1, OC.POLZN_MANY}
    for c in OC.POLZN:
        # POLZN_MANY is the smallest count with more than one chunk
        if c.n_cells == OC.POLZN_MANY:
            d = der[c.name]
            assert d["chunks"] > 1
            assert OC.polzn_chunks(d["ncls"], c.shape[0], c.shape[1], c.shape[2], c.dim, OC.POLZN_MANY - 1) == 1
        else:
            assert der[c.name]["chunks"] == 1


def test_decay_grids_are_the_asked_ones():
    by = {c.name: OC.decay_grid(c) for c in OC.DECAYS}
    g = by["3d-7x5x4-nonuniform-y-1.3-to-0.9"]
    assert (len(g["pT"]), len(g["phi"]), len(g["y"])) == (7, 5, 4) and g["y"][0] == -1.3 and g["y"][-1] == 0.9
    assert abs(g["y"][0]) != abs(g["y"][-1]) and len(set(np.round(np.diff(g["y"]), 6))) > 1
    g = by["3d-7x2x2-two-node-axes"]
    assert (len(g["pT"]), len(g["phi"]), len(g["y"])) == (7, 2, 2) and abs(g["y"][0]) != abs(g["y"][-1])
    g = by["2d-9x3"]
    assert (len(g["pT"]), len(g["phi"])) == (9, 3)
    for g in by.values():
        assert g["pT"][-1] == 3.0 and np.all(np.diff(g["pT"]) > 0) and len(set(np.round(np.diff(g["pT"]), 6))) > 1
        assert int(np.sum(g["pT"] > np.sqrt(1.73) * 1.0195)) >= 2   # the heaviest parent's M_T fit has its points


# ---- the references are fit for the metrics ----
@pytest.mark.parametrize("case", OC.OP0_DF, ids=ids(OC.OP0_DF))
def test_operation_0_oracle_values(case):
    b = OC.build_op0(case)
    ref = oracle_cells(b["cells"], range(case.n_cells), b["sp"], b["grid"], b["df"], b["opts"])
    assert ref.shape == (len(case.species), case.n_cells) and np.all(np.isfinite(ref))
    assert np.max(np.abs(ref)) > 0.0
    if b["opts"].get("outflow", 1) == 1:
        assert np.all((ref == 0.0) | (ref > 1e-250))   # the relative metric never rests on its floor


@pytest.mark.parametrize("case", OC.OP0_FQ, ids=ids(OC.OP0_FQ))
def test_operation_0_feqmod_restatement_values(case):
    b = OC.build_op0(case)
    want = dndx_feqmod_ref.dndx(b["cells"], b["sp"], b["grid"], b["df"], b["fq"], b["opts"])
    ref = want["per_cell"]
    assert np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 0.0
    if case.dim == 2:
        assert np.all(np.isfinite(want["eta"])) and np.max(np.abs(want["eta"])) > 0.0
    if b["opts"].get("outflow", 1) == 1:
        assert np.all((ref == 0.0) | (ref > 1e-250))
    assert (want["n_breakdown"] > 0) == case.breakdown   # the breakdown cases hold a breakdown cell, the others none


def vah_case_checks(b, ref, n_species):
    assert b["found"].all()                                   # oracle.vah_coefficients(...)[1]: every cell inside the tables
    assert ref.shape[0] == n_species and np.all(np.isfinite(ref))
    assert np.all(np.max(np.abs(ref), axis=1) > 0.0)          # the per-species metric divides by each row's maximum
    if b["neg"] is not None:
        uds = OC.vah_uds(b["cells"])
        assert uds[b["neg"]] < 0.0 and int(np.sum(uds < 0.0)) >= 1


@pytest.mark.parametrize("case", OC.OP0_VAH, ids=ids(OC.OP0_VAH))
def test_vah_operation_0_oracle_values(case):
    b, ref = OC.vah_reference(case.name)
    assert ref.shape == (len(case.species), case.n_cells)
    vah_case_checks(b, ref, len(case.species))
    assert (b["neg"] is None) == (case.n_cells == 1)
    assert (b["tab"] is not None) == case.tab


@pytest.mark.parametrize("case", OC.OP0_VAH_MANY, ids=ids(OC.OP0_VAH_MANY))
def test_vah_many_cell_oracle_values(case):
    b, subset, two, ref = OC.vah_many_reference(case.name)
    assert ref.shape == (75, len(subset))
    vah_case_checks(b, ref, 75)


def vah_dead_case(dim):
    return next(c for c in OC.OP0_VAH if c.dim == dim and c.grid != "random")


@pytest.mark.parametrize("dim", [3, 2])
def test_vah_dead_rows_are_dead_in_the_oracle(dim):
    """the far rows alone give exactly 0 in every bin of the oracle's spectrum, the near rows alone a non-zero value in every bin; 2+1D: both
    mixed blocks hold a node whose term is exactly 0 everywhere and one whose term is not.  The dead rows stay dead with Lambda raised by
    5 % (E_a/Lambda lowered by 5 %) and the live nodes live with Lambda lowered by 5 %: no row sits near exp()'s underflow threshold, where
    two exponentials may round differently."""
    case = vah_dead_case(dim)
    b, _ = OC.vah_reference(case.name)
    cells, sp, g, o = b["cells"], b["sp"], b["grid"], b["opts"]
    far, near = OC.vah_dead_split(case, g)
    warm = dict(cells, Lambda=1.05 * cells["Lambda"])
    assert np.all(oracle.dN_pTdpTdphidy_vah(cells, sp, far, o) == 0.0)
    assert np.all(oracle.dN_pTdpTdphidy_vah(warm, sp, far, o) == 0.0)
    assert np.all(oracle.dN_pTdpTdphidy_vah(cells, sp, near, o) != 0.0)
    if dim == 2:
        K, R = case.shape[2], OC.VAH_TILE[2][1]
        assert K == 4 * R
        for reg in (1, 0):
            dead = OC.vah_dead_eta_nodes(case.name, reg)
            assert np.array_equal(dead, OC.vah_dead_eta_nodes(case.name, reg, 1.05)) and np.array_equal(dead, OC.vah_dead_eta_nodes(case.name, reg, 0.95))
            assert dead[:R].all() and dead[3 * R:].all()
            for blk in (1, 2):
                assert dead[blk * R:(blk + 1) * R].any() and not dead[blk * R:(blk + 1) * R].all()
        # the regulated delta-f only adds dead nodes (a factor clamped to 0 beside the last exponentials that do not underflow)
        assert np.all(OC.vah_dead_eta_nodes(case.name, 1) | ~OC.vah_dead_eta_nodes(case.name, 0))
        # the exponent bound of cf_prep_vah (E_a/Lambda < 1e9 for the grid's largest mT and pT) by the rule of its domain test
        mT = np.sqrt(sp["mass"].max() ** 2 + g["pT"].max() ** 2)
        ut = np.sqrt(1.0 + cells["ux"] ** 2 + cells["uy"] ** 2 + cells["tau"] ** 2 * cells["un"] ** 2)
        worst = (mT * np.cosh(16.0) * (ut + np.abs(cells["tau"] * cells["un"])) * max(1.0, np.max(np.sqrt(np.abs(1.0 / cells["aL"] ** 2 - 1.0))))
                 + g["pT"].max() * np.hypot(cells["ux"], cells["uy"])) / cells["Lambda"]
        assert np.max(worst) < 1.0e9


@pytest.mark.parametrize("case", OC.POLZN, ids=ids(OC.POLZN))
def test_mode_5_restatement_values(case):
    b = OC.build_polzn(case)
    ref = restate(b["cells"], b["w"], b["sp"], b["grid"], b["T"], b["dim"])
    for k in api.POLARIZATION_OUTPUTS:
        assert np.all(np.isfinite(ref[k])) and np.max(np.abs(ref[k])) > 0.0, k


@pytest.mark.parametrize("case", OC.DECAYS, ids=ids(OC.DECAYS))
def test_decay_restatement_feeds_down(reference, case):
    """on the oracle's thermal spectrum (the GPU test feeds the library's): no refused parent, a non-zero feed-down"""
    g = OC.decay_grid(case)
    sp = OC.decay_species(api.pdg_read(os.path.join(reference, "PDG", OC.DECAY_PDG)))
    dN = oracle.dN_pTdpTdphidy(OC.decay_surface(case), sp, OC.plain(g), OC.inputs.df_tables(), dict(OC.DECAY_OPTS, dimension=case.dim))
    assert np.all(np.isfinite(dN)) and np.all(dN > 0.0)
    t = api.pdg_read_decays(os.path.join(reference, "PDG", OC.DECAY_PDG))
    st = {}
    out = R.feed_down(dN, t, OC.DECAY_CHOSEN, g["pT"], g["phi"], y=g["y"] if case.dim == 3 else None, dim3=case.dim == 3, stats=st)
    S = len(OC.DECAY_CHOSEN)
    fed = np.max(np.abs(out - dN).reshape(-1, S), axis=0)
    assert np.all(np.isfinite(out)) and st["n_parents"] == 4 and np.any(fed > 0.0)
