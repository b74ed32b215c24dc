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
