"""GPU: operation 0 for anisotropic hydro (cf_spacetime_vah.hip; is3d_vah_plan_execute_spacetime on cf_spacetime_host.cpp's driver) on the
off-tile cases of tests/offtile_cases.py (OP0_VAH, OP0_VAH_MANY, OP0_VAH_REFUSED): npTp = 1 and 64, partly filled workgroups, a single y
node or phi, full and padded row blocks, the 2+1D LDS bound and its refusal, row blocks and rows that the exact-zero culls skip, several
passes, two cells in one chunk, and a plan executed with changed weights.  tests/test_offtile_cases.py proves on the CPU that the table
reaches those branches.

The reference is the per-cell oracle route of tests/test_gpu_spacetime_vah.py (oracle_cells_vah).  The error of species s is divided by
max |ref[s, :]|, so that a heavy species' error is not hidden behind the pions' maximum; tolerance 2e-9, the VAH parity tolerance of
tests/test_gpu_vah.py.

What these cases found: no fault in the library -- every case met the tolerance at the first run.  They did correct what "dead" means for a
2+1D node: with regulate_deltaf = 1 the oracle is exactly 0 at two more nodes than without, where the last exponentials that do not
underflow meet a factor 1 + fbar delta-f clamped to 0; the library gives exact zeros at the dead nodes of either setting.

Worst per-species errors measured on an MI355X (tolerance 2e-9):
    dN_dy_cell            3+1D 2.7e-14 (3 pT, 7 phi, 8 y, regulate_deltaf = 0)   2+1D 2.3e-14 (1 pT, 5 phi | 2 eta)
    2+1D dN_dydeta        block-boundary nodes 3.3e-14 (1 pT | 32 eta, the LDS bound)   all 124 nodes of the dead-row grid 2.7e-15
    1000 cells            dN_dy_cell of the subset 3+1D 9.4e-15, 2+1D 8.5e-15; dN_dy 5.2e-15 / 4.7e-15; 2+1D dN_dydeta, all 33 nodes 4.3e-15"""
import numpy as np
import pytest

import offtile_cases as OC
from is3d_amd import api
from oracle import oracle
from test_gpu_spacetime import binned, bins_of, contract

pytestmark = pytest.mark.gpu
TOL = 2e-9   # tests/test_gpu_vah.py


def ids(cases):
    return [c.name for c in cases]


def species_err(got, ref):
    """the worst error of a species row against that row's largest |reference value|; a row whose reference is all zero must be zero"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    S = ref.shape[0]
    g, r = got.reshape(S, -1), ref.reshape(S, -1)
    scale = np.max(np.abs(r), axis=1)
    err = np.max(np.abs(g - r), axis=1)
    assert np.all(err[scale == 0.0] == 0.0)
    return float(np.max(err[scale > 0.0] / scale[scale > 0.0])) if (scale > 0.0).any() else 0.0


def lib_cells(b):
    """what the library is given: without c0..c4 when the tables are"""
    return {k: v for k, v in b["cells"].items() if not (b["tab"] is not None and k in OC.VAH_COEF)}


def run(b, cells=None, grid=None, **extra):
    return api.spacetime_distributions_vah(lib_cells(b) if cells is None else cells, b["sp"], b["grid"] if grid is None else grid, b["bins"],
                                           dict(b["opts"], **extra), per_cell=True, tab=b["tab"])


_RUNS = {}


def result(name):
    """the library's result of a case, computed once"""
    if name not in _RUNS:
        many = any(c.name == name for c in OC.OP0_VAH_MANY)
        _RUNS[name] = run((OC.vah_many_reference if many else OC.vah_reference)(name)[0])
    return _RUNS[name]


def check_histograms_and_stats(case, b, res, ref_cell):
    cells, bins = b["cells"], b["bins"]
    t, r, tr = binned(ref_cell, cells, bins)
    for name, want in (("dN_taudtaudy", t), ("dN_twopirdrdy", r), ("dN_twopitaurdtaudrdy", tr), ("dN_dy", ref_cell.sum(axis=1))):
        assert species_err(res[name], want) < TOL, name
    check_stats(case, b, res)


def check_stats(case, b, res):
    cells, bins = b["cells"], b["bins"]
    st = res["stats"]
    it, ir = bins_of(cells, bins)
    d = OC.vah_derived(case)
    assert st["n_classes"] == OC.n_classes(b["sp"], 0) == d["ncls"]
    assert st["n_cells_skipped"] == 0
    # ALL cells, whatever the sign of u.dsigma
    assert st["n_tau_outside"] == int(np.sum((it < 0) | (it >= bins["tau_bins"]))) and st["n_tau_negative"] == int(np.sum(it < 0))
    assert st["n_r_outside"] == int(np.sum((ir < 0) | (ir >= bins["r_bins"]))) and st["n_r_negative"] == int(np.sum(ir < 0))
    assert st["n_passes"] == d["n_passes"]
    if case.workspace:
        assert st["n_passes"] > 1


def eta_terms(cells, sp, g, o, nodes):
    """[S][len(nodes)]: the oracle's dN/dy deta at the nodes -- node k's term of the eta sum over its effective weight w_k deta"""
    deta = g["eta"][1] - g["eta"][0]
    cols = []
    for k in nodes:
        g2 = OC.vah_eta_node_grid(g, k)
        cols.append(contract(oracle.dN_pTdpTdphidy_vah(cells, sp, g2, o), sp, g2, 2) / (g["eta_w"][k] * deta))
    return np.stack(cols, axis=1)


def check_eta_sum(res, g):
    """dN_dydeta @ (eta_w deta) is dN_dy summed in another order: within 1e-12 (the bound of tests/test_gpu_spacetime_vah.py) of the summed
    |terms| of each species"""
    w = g["eta_w"] * (g["eta"][1] - g["eta"][0])
    assert np.all(np.abs(res["dN_dydeta"] @ w - res["dN_dy"]) <= 1e-12 * (np.abs(res["dN_dydeta"]) @ w))


# ---- parity per case ----
@pytest.mark.parametrize("case", OC.OP0_VAH, ids=ids(OC.OP0_VAH))
def test_parity_with_the_oracle(case):
    b, ref = OC.vah_reference(case.name)
    res = result(case.name)
    S, n = len(case.species), case.n_cells
    assert res["dN_dy_cell"].shape == (S, n)
    err = species_err(res["dN_dy_cell"], ref)
    print("%s: dN_dy_cell worst per-species error %.3e (tolerance %.0e)" % (case.name, err, TOL))
    assert err < TOL
    if b["neg"] is not None:   # the negated cell is not skipped: it differs from 0 where the oracle does
        assert np.array_equal(res["dN_dy_cell"][:, b["neg"]] != 0.0, ref[:, b["neg"]] != 0.0) and (ref[:, b["neg"]] != 0.0).any()
    check_histograms_and_stats(case, b, res, ref)
    if case.dim == 3:
        assert res["dN_dydeta"].shape == (S, 1) and np.array_equal(res["dN_dydeta"][:, 0], res["dN_dy"])


D2 = [c for c in OC.OP0_VAH if c.dim == 2]


@pytest.mark.parametrize("case", D2, ids=ids(D2))
def test_dN_dydeta_2d(case):
    b, _ = OC.vah_reference(case.name)
    res = result(case.name)
    g, K = b["grid"], case.shape[2]
    assert res["dN_dydeta"].shape == (len(case.species), K)
    nodes = OC.vah_eta_check_nodes(K)
    want = eta_terms(b["cells"], b["sp"], g, b["opts"], nodes)
    err = species_err(res["dN_dydeta"][:, nodes], want)   # (a dead-row grid has exact zeros among these nodes: they count as any value)
    print("%s: dN_dydeta at the nodes %s worst per-species error %.3e" % (case.name, nodes, err))
    assert err < TOL
    check_eta_sum(res, g)


# ---- dead rows ----
DEAD = [c for c in OC.OP0_VAH if c.grid != "random"]


@pytest.mark.parametrize("case", DEAD, ids=ids(DEAD))
def test_dead_rows(case):
    """The culls change no bit (zero_skip = 2 runs every row; the parity test above holds the result to the oracle), the far rows alone give
    exact zeros, and so do the dead eta nodes with delta-f regulated or not (the oracle's dead nodes of either setting: regulated, two more
    nodes are exactly 0 through the clamp).  A cull bound read from the wrong header slot would skip a
    live row of the mixed blocks, or none of the dead ones."""
    b, _ = OC.vah_reference(case.name)
    res = result(case.name)
    every_row = run(b, zero_skip=2)
    for k in api.SPACETIME_OUTPUTS:
        assert np.array_equal(res[k], every_row[k]), k
    far, near = OC.vah_dead_split(case, b["grid"])
    for extra in (dict(), dict(zero_skip=2)):
        got = run(b, grid=far, **extra)
        assert np.all(got["dN_dy_cell"] == 0.0) and np.all(got["dN_dydeta"] == 0.0), extra
    # ... so the near rows alone give the bits of the whole grid (the far rows add +-0 and come after, or around, the near ones in the same order)
    got = run(b, grid=near)
    assert np.array_equal(got["dN_dy_cell"], res["dN_dy_cell"]) and np.all(np.any(got["dN_dy_cell"] != 0.0, axis=1))
    if case.dim == 2:
        for reg in (1, 0):
            dead = OC.vah_dead_eta_nodes(case.name, reg)   # the oracle's exact zeros with that regulate_deltaf
            assert dead.any() and not dead.all()
            for skip in (1, 2):
                got = run(b, regulate_deltaf=reg, zero_skip=skip)
                assert np.all(got["dN_dydeta"][:, dead] == 0.0), (reg, skip)
                assert np.all(np.any(got["dN_dydeta"][:, ~dead] != 0.0, axis=0)), (reg, skip)
        # every node, the ones next to a dead one included, against the oracle
        err = species_err(res["dN_dydeta"], eta_terms(b["cells"], b["sp"], b["grid"], b["opts"], range(case.shape[2])))
        print("%s: dN_dydeta at all %d nodes worst per-species error %.3e" % (case.name, case.shape[2], err))
        assert err < TOL


# ---- more than one cell per chunk ----
def halves(b, n):
    h = n // 2
    return [run(b, cells={k: v[lo:hi] for k, v in lib_cells(b).items()}) for lo, hi in ((0, h), (h, n))]


@pytest.mark.parametrize("case", OC.OP0_VAH_MANY, ids=ids(OC.OP0_VAH_MANY))
def test_two_cells_in_a_chunk(case):
    """1000 cells in 862 chunks.  D of a cell depends on that cell alone (cf_spacetime_vah.hip), so its columns equal, bit for bit, those of
    the two half surfaces, which run one cell per chunk -- the regime the cases above hold to the oracle; a subset that holds both cells of
    several two-cell chunks meets the per-cell oracle itself."""
    b, subset, two, ref = OC.vah_many_reference(case.name)
    res = result(case.name)
    n, cells, sp, g, o = case.n_cells, b["cells"], b["sp"], b["grid"], b["opts"]
    lo, hi = halves(b, n)
    assert np.array_equal(res["dN_dy_cell"], np.concatenate([lo["dN_dy_cell"], hi["dN_dy_cell"]], axis=1))
    err = species_err(res["dN_dy_cell"][:, subset], ref)
    print("%s: dN_dy_cell of %d cells (both cells of %d two-cell chunks) worst per-species error %.3e" % (case.name, len(subset), len(two), err))
    assert err < TOL
    assert np.all(res["dN_dy_cell"][:, b["neg"]] != 0.0)
    whole = contract(oracle.dN_pTdpTdphidy_vah(cells, sp, g, o), sp, g, case.dim)
    err = species_err(res["dN_dy"][:, None], whole[:, None])
    print("    dN_dy against the whole-surface oracle %.3e" % err)
    assert err < TOL
    # the histograms are the sums of dN_dy_cell in ascending cell order
    t, r, tr = binned(res["dN_dy_cell"], cells, b["bins"])
    assert np.array_equal(res["dN_taudtaudy"], t) and np.array_equal(res["dN_twopirdrdy"], r) and np.array_equal(res["dN_twopitaurdtaudrdy"], tr)
    check_stats(case, b, res)
    if case.dim == 3:
        return
    K = case.shape[2]
    err = species_err(res["dN_dydeta"], eta_terms(cells, sp, g, o, range(K)))
    print("    dN_dydeta against the whole-surface oracle, all %d nodes %.3e" % (K, err))
    assert err < TOL
    check_eta_sum(res, g)
    # against the sum of the halves: the same per-cell terms added in another order, n additions per value.  The summed |terms| are not an
    # output; |lo| + |hi| is a lower bound of them, so this asks no less than n 2^-52 of the summed |terms|
    both = lo["dN_dydeta"] + hi["dN_dydeta"]
    assert np.all(np.abs(res["dN_dydeta"] - both) <= n * 2.0 ** -52 * (np.abs(lo["dN_dydeta"]) + np.abs(hi["dN_dydeta"])))


# ---- refusals ----
def refused_inputs(dim, shape):
    case = OC._vah("refused", dim, shape, OC.THREE, 2)
    return OC.build_op0_vah(case)


@pytest.mark.parametrize("name,dim,shape", OC.OP0_VAH_REFUSED, ids=[r[0] for r in OC.OP0_VAH_REFUSED])
def test_refused_before_any_plan(name, dim, shape):
    b = refused_inputs(dim, shape)
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        run(b)
    assert e.value.code == api.IS3D_EINVAL
    assert ("%d pT values x %d eta nodes" % (shape[0], shape[2]) in str(e.value)) if shape[0] <= 64 else ("64" in str(e.value))
    assert api.resource_counters() == before


def device_io(b, fill):
    import torch
    dev = torch.device("cuda:0")
    n = len(b["cells"]["tau"])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b["cells"].items()}
    K = len(b["grid"]["eta"])
    shapes = api.spacetime_shapes(len(b["sp"]["mass"]), n, b["bins"], b["opts"]["dimension"], K)
    outs = {k: torch.full(v, fill, dtype=torch.float64, device=dev) for k, v in shapes.items()}
    ptrs = {k: v.data_ptr() for k, v in t.items() if k in api.VAH_FIELDS and not (b["tab"] is not None and k in OC.VAH_COEF)}
    return t, outs, ptrs


@pytest.mark.parametrize("name,dim,shape", OC.OP0_VAH_REFUSED, ids=[r[0] for r in OC.OP0_VAH_REFUSED])
def test_plan_entry_refuses_without_allocating(name, dim, shape):
    """the spectra plan of such a grid exists; its execute_spacetime returns IS3D_EINVAL before it allocates"""
    import torch
    b = refused_inputs(dim, shape)
    g = b["grid"]
    plan = api.VahPlan(b["sp"], OC.plain(g), b["opts"], tab=b["tab"], max_cells=2)
    try:
        t, outs, ptrs = device_io(b, 0.0)
        before = api.resource_counters()
        with pytest.raises(api.Is3dError) as e:
            plan.execute_spacetime(2, ptrs, t["x"].data_ptr(), t["y"].data_ptr(), g["pT_w"], g["phi_w"], b["bins"],
                                   {k: v.data_ptr() for k, v in outs.items()}, torch.cuda.current_stream().cuda_stream)
        assert e.value.code == api.IS3D_EINVAL
        assert api.resource_counters() == before
    finally:
        plan.close()


# ---- the plan entry, and its cached weights ----
@pytest.mark.parametrize("name", ["3d-npT5-phi9-y15-passes", "2d-npT3-phi13-eta63"])
def test_plan_entry_same_bits_and_changed_weights(name):
    """Twice into outputs pre-filled with 7.0: the one-shot's bits.  Then other weights on the same plan (the plan uploads pT_w / phi_w only
    when they differ from its copy): the one-shot with those weights; then the first weights again: the first result."""
    import torch
    case = next(c for c in OC.OP0_VAH if c.name == name)
    b, _ = OC.vah_reference(name)
    g, n = b["grid"], case.n_cells
    rng = np.random.default_rng(OC._seed(name) + 11)
    g2 = dict(g, pT_w=rng.uniform(0.5, 1.5, case.shape[0]), phi_w=rng.uniform(0.5, 1.5, case.shape[1]))
    g3 = dict(g, phi_w=g2["phi_w"])   # only phi_w differs from the first
    one_shot = {1: result(name), 2: run(b, grid=g2), 3: run(b, grid=g3)}
    assert not np.array_equal(one_shot[1]["dN_dy_cell"], one_shot[2]["dN_dy_cell"])
    assert not np.array_equal(one_shot[1]["dN_dy_cell"], one_shot[3]["dN_dy_cell"])
    t, outs, ptrs = device_io(b, 7.0)
    plan = api.VahPlan(b["sp"], OC.plain(g), b["opts"], tab=b["tab"], max_cells=n)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        for which, gw in ((1, g), (1, g), (2, g2), (1, g), (3, g3), (2, g2), (1, g)):
            st = plan.execute_spacetime(n, ptrs, t["x"].data_ptr(), t["y"].data_ptr(), gw["pT_w"], gw["phi_w"], b["bins"],
                                        {k: v.data_ptr() for k, v in outs.items()}, stream)
            torch.cuda.synchronize()
            for k in api.SPACETIME_OUTPUTS:
                assert outs[k].cpu().numpy().tobytes() == one_shot[which][k].tobytes(), (which, k)
            assert st["n_passes"] == one_shot[which]["stats"]["n_passes"]
    finally:
        plan.close()
