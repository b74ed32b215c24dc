"""GPU: operation 0 (df_mode 1-4), the spin polarization and the decay feed-down on the off-tile shapes of tests/offtile_cases.py -- padded
pT lanes, phi tile tails, padded y / eta rows, partly filled workgroups, the 2+1D LDS bound, non-uniform and two-node grids -- each against
the checker the subsystem already has, with that checker's metric and tolerance.

What these cases found: cf_st_cells summed the padding rows of a 3+1D y grid that is no multiple of 7 (p.dsigma of a 3+1D row does not read
W, so a padding row added pT B_j f of the last y row: dN_dy_cell off by up to 9 % on 15 y nodes, non-zero where the oracle has 0 on a single
one); its row loop now stops at the last y row.  The one-shot entries refused a grid past the 64-pT / LDS bounds only after creating a
plan; they ask the grid check first.  Worst errors on an MI355X after the fix: operation 0 df_mode 1 / 2 3.8e-14 (held to 1e-10), df_mode
3 / 4 4.2e-14 (1e-9), mode 5 8.3e-14 (1e-10), feed-down 1.7e-13 (1e-10)."""
import os
from functools import lru_cache

import numpy as np
import pytest

import decays_restated as R
import dndx_feqmod_ref
import offtile_cases as OC
from is3d_amd import api
from oracle import oracle
from test_gpu_decays import feed_err
from test_gpu_polarization import assert_close, restate
from test_gpu_spacetime import binned, bins_of, contract, err_vs_max, live, oracle_cells
from test_gpu_spacetime_feqmod import check_against_restatement

pytestmark = pytest.mark.gpu

TOL = 1e-10


def ids(cases):
    return [c.name for c in cases]


# ---- references: computed once per case, shared by the parity and the plan tests, never written to ----
@lru_cache(maxsize=None)
def op0_df_reference(name):
    case = next(c for c in OC.OP0_DF if c.name == name)
    b = OC.build_op0(case)
    ref = oracle_cells(b["cells"], range(case.n_cells), b["sp"], b["grid"], b["df"], b["opts"])
    ref.setflags(write=False)
    return b, ref


@lru_cache(maxsize=None)
def op0_fq_reference(name):
    case = next(c for c in OC.OP0_FQ if c.name == name)
    b = OC.build_op0(case)
    return b, dndx_feqmod_ref.dndx(b["cells"], b["sp"], b["grid"], b["df"], b["fq"], b["opts"])


def run_op0(b):
    return api.spacetime_distributions(b["cells"], b["sp"], b["grid"], b["df"], b["bins"], b["opts"], per_cell=True, fq=b["fq"])


def rel_err(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))


@pytest.mark.parametrize("case", OC.OP0_DF, ids=ids(OC.OP0_DF))
def test_operation_0_against_the_oracle(case):
    b, ref_cell = op0_df_reference(case.name)
    cells, sp, g, o, bins = b["cells"], b["sp"], b["grid"], b["opts"], b["bins"]
    res = run_op0(b)
    signed = o.get("outflow", 1) == 0
    err = err_vs_max(res["dN_dy_cell"], ref_cell) if signed else rel_err(res["dN_dy_cell"], ref_cell)
    print("%s: dN_dy_cell %s error %.3e (tolerance %.0e)" % (case.name, "vs-max" if signed else "relative", err, TOL))
    assert err < TOL
    t, r, tr = binned(ref_cell, cells, bins)
    for name, ref in (("dN_taudtaudy", t), ("dN_twopirdrdy", r), ("dN_twopitaurdtaudrdy", tr), ("dN_dy", ref_cell.sum(axis=1))):
        assert res[name].shape == ref.shape
        assert err_vs_max(res[name], ref) < TOL, name
    S, K = len(case.species), case.shape[2]
    if case.dim == 3:
        assert res["dN_dydeta"].shape == (S, 1)
        assert err_vs_max(res["dN_dydeta"][:, 0], ref_cell.sum(axis=1)) < TOL
    else:
        assert res["dN_dydeta"].shape == (S, K)
        # one-point eta grids [eta_k], [w_k]: the oracle's spectrum divided by w_k -- the first, an interior and the last node
        for k in sorted({0, K // 2, K - 1}):
            g1 = dict(g, eta=g["eta"][k:k + 1], eta_w=g["eta_w"][k:k + 1])
            ref = contract(oracle.dN_pTdpTdphidy(cells, sp, g1, b["df"], o), sp, g1, 2) / g["eta_w"][k]
            e = err_vs_max(res["dN_dydeta"][:, k], ref)
            print("    dN_dydeta at eta node %d: %.3e" % (k, e))
            assert e < TOL, k
        assert err_vs_max(res["dN_dydeta"] @ g["eta_w"], ref_cell.sum(axis=1)) < TOL
    st = res["stats"]
    it, ir = bins_of(cells, bins)
    lv = live(cells)
    assert st["n_tau_outside"] == int(np.sum(lv & ((it < 0) | (it >= bins["tau_bins"]))))
    assert st["n_r_outside"] == int(np.sum(lv & ((ir < 0) | (ir >= bins["r_bins"]))))
    assert st["n_classes"] == OC.n_classes(sp, o.get("include_baryon", 0))


@pytest.mark.parametrize("case", OC.OP0_FQ, ids=ids(OC.OP0_FQ))
def test_operation_0_feqmod_against_the_restatement(case):
    b, want = op0_fq_reference(case.name)
    res = run_op0(b)
    signed = b["opts"].get("outflow", 1) == 0
    pc = want["per_cell"]
    err = err_vs_max(res["dN_dy_cell"], pc) if signed else rel_err(res["dN_dy_cell"], pc)
    print("%s: dN_dy_cell %s error %.3e (tolerance 1e-09)" % (case.name, "vs-max" if signed else "relative", err))
    if case.dim == 2:
        print("    dN_dydeta vs-max error %.3e" % err_vs_max(res["dN_dydeta"], want["eta"]))
    check_against_restatement(res, want, b["cells"], b["bins"], signed, case.dim)
    assert res["feqmod_stats"]["n_cells_breakdown"] == want["n_breakdown"]
    assert (want["n_breakdown"] > 0) == case.breakdown
    assert res["stats"]["n_classes"] == OC.n_classes(b["sp"], 0)


@pytest.mark.parametrize("name,dim,shape,df_mode", OC.OP0_REFUSED, ids=[r[0] for r in OC.OP0_REFUSED])
def test_operation_0_refuses_before_any_plan(name, dim, shape, df_mode):
    """One eta node past the LDS bound, and 65 pT values: IS3D_EINVAL from the host-side argument check, before a plan is created or
    anything is allocated."""
    b = OC.op0_inputs(dim, shape, df_mode, OC.THREE, 2, {}, False, 77)
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        run_op0(b)
    assert e.value.code == api.IS3D_EINVAL
    assert ("%d pT values x %d eta nodes" % (shape[0], shape[2]) in str(e.value)) if shape[0] <= 64 else ("64" in str(e.value))
    assert api.resource_counters() == before


def test_operation_0_plan_entry_refuses_without_allocating():
    """the same bound on the device-resident entry: the spectra plan of such a grid exists, its execute_spacetime returns IS3D_EINVAL"""
    import torch
    dev = torch.device("cuda:0")
    name, dim, shape, df_mode = OC.OP0_REFUSED[0]
    b = OC.op0_inputs(dim, shape, df_mode, OC.THREE, 2, {}, False, 77)
    plan = api.Plan(b["sp"], OC.plain(b["grid"]), b["df"], b["opts"], max_cells=2)
    try:
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b["cells"].items()}
        shapes = api.spacetime_shapes(len(b["sp"]["mass"]), 2, b["bins"], dim, shape[2])
        outs = {k: torch.zeros(v, dtype=torch.float64, device=dev) for k, v in shapes.items()}
        before = api.resource_counters()
        with pytest.raises(api.Is3dError) as e:
            plan.execute_spacetime(2, {k: v.data_ptr() for k, v in t.items()}, t["x"].data_ptr(), t["y"].data_ptr(), b["grid"]["pT_w"],
                                   b["grid"]["phi_w"], b["bins"], {k: v.data_ptr() for k, v in outs.items()},
                                   torch.cuda.current_stream().cuda_stream)
        assert e.value.code == api.IS3D_EINVAL and "eta nodes" in str(e.value)
        assert api.resource_counters() == before
    finally:
        plan.close()


@pytest.mark.parametrize("which,name", [("df", "3d-npT33-phi13-y1-nlw5"), ("df", "2d-npT3-phi13-eta63-baryon"),
                                        ("fq", "3d-npT64-phi9-y8-breakdown-signed-nlw2"), ("fq", "2d-npT33-phi5-eta62-nlw5-5chunks")])
def test_operation_0_plan_entry_same_bits(which, name):
    import torch
    b, _ = (op0_df_reference if which == "df" else op0_fq_reference)(name)
    one_shot = run_op0(b)
    dev = torch.device("cuda:0")
    cells, g, n = b["cells"], b["grid"], len(b["cells"]["tau"])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items()}
    shapes = api.spacetime_shapes(len(b["sp"]["mass"]), n, b["bins"], b["opts"]["dimension"], len(g["eta"]))
    outs = {k: torch.full(v, 7.0, dtype=torch.float64, device=dev) for k, v in shapes.items()}
    plan = api.Plan(b["sp"], OC.plain(g), b["df"], b["opts"], max_cells=n, fq=b["fq"])
    try:
        stream = torch.cuda.current_stream().cuda_stream
        for _ in range(2):
            plan.execute_spacetime(n, {k: v.data_ptr() for k, v in t.items()}, t["x"].data_ptr(), t["y"].data_ptr(), g["pT_w"], g["phi_w"],
                                   b["bins"], {k: v.data_ptr() for k, v in outs.items()}, stream)
            torch.cuda.synchronize()
            for k in api.SPACETIME_OUTPUTS:
                assert outs[k].cpu().numpy().tobytes() == one_shot[k].tobytes(), k
    finally:
        plan.close()


# ---- mode 5 ----
@lru_cache(maxsize=None)
def polzn_reference(name):
    case = next(c for c in OC.POLZN if c.name == name)
    b = OC.build_polzn(case)
    return b, restate(b["cells"], b["w"], b["sp"], b["grid"], b["T"], b["dim"])


@pytest.mark.parametrize("case", OC.POLZN, ids=ids(OC.POLZN))
def test_mode_5_against_the_restatement(case):
    b, ref = polzn_reference(case.name)
    got = api.spin_polarization(b["cells"], b["w"], b["sp"], b["grid"], b["T"], dict(dimension=case.dim))
    worst = max(float(np.max(np.abs(got[k] - ref[k])) / np.max(np.abs(ref[k]))) for k in api.POLARIZATION_OUTPUTS)
    print("%s: worst error against the array maximum %.3e (tolerance %.0e)" % (case.name, worst, TOL))
    assert_close(got, ref, tol=TOL)
    d = OC.polzn_derived(case)
    assert got["stats"]["n_classes"] == d["ncls"] and got["stats"]["n_chunks"] == d["chunks"]


def test_mode_5_refuses_65_pT_values():
    b = dict(OC.build_polzn(OC.POLZN[0]))
    b["grid"] = OC.plain(OC.make_grid(65, 3, 2, 3, 5))
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        api.spin_polarization(b["cells"], b["w"], b["sp"], b["grid"], b["T"], dict(dimension=3))
    assert e.value.code == api.IS3D_EINVAL and "65" in str(e.value)
    assert api.resource_counters() == before


def test_mode_5_plan_entry_same_bits():
    import torch
    case = next(c for c in OC.POLZN if c.name == "3d-npT33-phi9-y7")
    b, _ = polzn_reference(case.name)
    one_shot = api.spin_polarization(b["cells"], b["w"], b["sp"], b["grid"], b["T"], dict(dimension=case.dim))
    dev = torch.device("cuda:0")
    tc = {k: torch.from_numpy(np.ascontiguousarray(b["cells"][k])).to(dev) for k in api.CELL_FIELDS if k in b["cells"]}
    tw = {k: torch.from_numpy(v).to(dev) for k, v in b["w"].items()}
    plan = api.PolarizationPlan(b["sp"], b["grid"], dict(dimension=case.dim), max_cells=case.n_cells)
    outs = {k: torch.full((plan.output_size,), 7.0, dtype=torch.float64, device=dev) for k in api.POLARIZATION_OUTPUTS}
    try:
        for _ in range(2):
            plan.execute(case.n_cells, {k: v.data_ptr() for k, v in tc.items()}, {k: v.data_ptr() for k, v in tw.items()}, b["T"],
                         {k: v.data_ptr() for k, v in outs.items()}, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            for k in api.POLARIZATION_OUTPUTS:
                assert outs[k].cpu().numpy().tobytes() == one_shot[k].tobytes(), k
    finally:
        plan.close()


# ---- decay feed-down ----
@lru_cache(maxsize=None)
def decay_inputs(name, root):
    case = next(c for c in OC.DECAYS if c.name == name)
    g = OC.decay_grid(case)
    sp = OC.decay_species(api.pdg_read(os.path.join(root, "PDG", OC.DECAY_PDG)))
    dN, _ = api.smooth_spectra(OC.decay_surface(case), sp, OC.plain(g), OC.inputs.df_tables(), dict(OC.DECAY_OPTS, dimension=case.dim))
    dN = np.asarray(dN, dtype=np.float64)
    dN.setflags(write=False)
    t = api.pdg_read_decays(os.path.join(root, "PDG", OC.DECAY_PDG))
    rs = {}
    ref = R.feed_down(dN, t, OC.DECAY_CHOSEN, g["pT"], g["phi"], y=g["y"] if case.dim == 3 else None, dim3=case.dim == 3, stats=rs)
    return g, t, dN, ref, rs


def decay_grid_arg(g, dim):
    return dict(pT=g["pT"], phi=g["phi"], y=g["y"] if dim == 3 else None)


@pytest.mark.parametrize("case", OC.DECAYS, ids=ids(OC.DECAYS))
def test_decays_against_the_restatement(reference, case):
    g, t, dN, ref, rs = decay_inputs(case.name, reference)
    got, st = api.resonance_decays(t, OC.DECAY_CHOSEN, decay_grid_arg(g, case.dim), dN, dimension=case.dim)
    S = len(OC.DECAY_CHOSEN)
    err = feed_err(got, ref, dN, S)
    print("%s: worst feed-down error %.3e (tolerance %.0e); stats %s" % (case.name, err, TOL, st))
    assert np.isfinite(got).all() and (np.max(np.abs(ref - dN).reshape(-1, S), axis=0) > 0.0).any()
    assert err < TOL
    for k in ("n_parents", "n_channels", "n_adjusted"):
        assert st[k] == rs[k], k
    if case.dim == 2:
        assert st["n_clamps"] == rs["n_clamps"]   # (the restatement counts the clamps of the 2+1D integral only)


def test_decays_plan_entry_same_bits(reference):
    import torch
    case = OC.DECAYS[0]
    g, t, dN, _, _ = decay_inputs(case.name, reference)
    one_shot, _ = api.resonance_decays(t, OC.DECAY_CHOSEN, decay_grid_arg(g, case.dim), dN, dimension=case.dim)
    plan = api.DecayPlan(t, OC.DECAY_CHOSEN, decay_grid_arg(g, case.dim), dimension=case.dim, device=0)
    try:
        assert plan.output_size == dN.size
        for _ in range(2):
            d = torch.from_numpy(dN.copy()).to("cuda:0")
            plan.execute(d.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert d.cpu().numpy().tobytes() == one_shot.tobytes()
    finally:
        plan.close()
