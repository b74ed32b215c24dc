"""GPU: is3d_spacetime_distributions_multi -- operation 0 with the per-cell stage on cell-axis shards (one per entry of the device list)
and ONE bin stage over the assembled D on devices[0].  Repeated ordinals of device 0 make every shard count run on one GPU.

Contract under test (include/is3d_amd.h): dN_dy, the three histograms, dN_dy_cell and the 3+1D dN_dydeta are BITWISE the single-device
result for any shard count; one shard is the single-device call bit for bit, dN_dydeta included; the 2+1D dN_dydeta of several shards
differs by the association of its additions only, is held to the oracle at the subsystem's tolerance (1e-10 for df_mode 1 / 2, 1e-9 for
df_mode 3 / 4) and is bitwise reproducible for a given shard count.

Shapes: 3+1D 8 pT x 5 phi x 15 y (15 is no multiple of the 7-row tile) on 61 cells, 2+1D 4 pT x 3 phi x 9 eta on 23 cells: unequal shards."""
from functools import lru_cache

import numpy as np
import pytest

import dndx_feqmod_ref
import offtile_cases as OC
from is3d_amd import api
from oracle import oracle
from test_gpu_spacetime import binned, contract, err_vs_max, live, oracle_cells

pytestmark = pytest.mark.gpu

SHARDS = [1, 2, 3, 4, 7]
EXACT = ["dN_dy", "dN_taudtaudy", "dN_twopirdrdy", "dN_twopitaurdtaudrdy", "dN_dy_cell"]

# name -> (dim, shape, df_mode, species, n_cells, opts, breakdown)
CASES = {
    "3d-df1": (3, (8, 5, 15), 1, OC.THREE, 61, {}, False),
    "3d-df2-baryon": (3, (8, 5, 15), 2, OC.BARYON3, 61, dict(include_baryon=1, include_baryondiff_deltaf=1), False),
    "3d-df3-breakdown": (3, (8, 5, 15), 3, OC.THREE, 61, {}, True),
    "3d-df4": (3, (8, 5, 15), 4, OC.THREE, 61, {}, False),
    "2d-df1": (2, (4, 3, 9), 1, OC.THREE, 23, {}, False),
    "2d-df4": (2, (4, 3, 9), 4, OC.THREE, 23, {}, False),
}


@lru_cache(maxsize=None)
def inputs_of(name):
    dim, shape, df_mode, species, n, opts, breakdown = CASES[name]
    return OC.op0_inputs(dim, shape, df_mode, species, n, opts, breakdown, 7000 + sorted(CASES).index(name))


def one_shot_of(b):
    return api.spacetime_distributions(b["cells"], b["sp"], b["grid"], b["df"], b["bins"], b["opts"], per_cell=True, fq=b["fq"])


def multi_of(b, devices, **kw):
    return api.spacetime_distributions_multi(b["cells"], b["sp"], b["grid"], b["df"], b["bins"], b["opts"], devices, fq=b["fq"], per_cell=True, **kw)


@lru_cache(maxsize=None)
def reference(name):
    """the single-device result of a case, computed once and never written to"""
    res = one_shot_of(inputs_of(name))
    for k in api.SPACETIME_OUTPUTS:
        res[k].setflags(write=False)
    return res


def assert_same_bits(got, want, keys=EXACT):
    for k in keys:
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]) and got[k].tobytes() == want[k].tobytes(), k


def assert_bins_are_running_sums(res, b):
    t, r, tr = binned(res["dN_dy_cell"], b["cells"], b["bins"])
    assert np.array_equal(res["dN_taudtaudy"], t)
    assert np.array_equal(res["dN_twopirdrdy"], r)
    assert np.array_equal(res["dN_twopitaurdtaudrdy"], tr)
    assert np.array_equal(res["dN_dy"], np.cumsum(res["dN_dy_cell"], axis=1)[:, -1])


# ---- 1. bitwise against the one-shot ----
@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_bitwise_against_the_one_shot(name, shards):
    b, want = inputs_of(name), reference(name)
    if CASES[name][6]:
        assert want["feqmod_stats"]["n_cells_breakdown"] > 0
        lo = api.shard_bounds(len(b["cells"]["tau"]), 1, 2)[0]
        assert (b["cells"]["bulkPi"][lo:] < -4.0 * b["cells"]["P"][lo:]).any()   # breakdown cells in a shard other than the first
    got = multi_of(b, [0] * shards)
    assert_same_bits(got, want)
    if CASES[name][0] == 3 or shards == 1:
        assert_same_bits(got, want, ["dN_dydeta"])
    assert_bins_are_running_sums(got, b)
    assert len(got["shard_stats"]) == shards and got["stats"]["code"] == 0


# ---- 2. the 2+1D dN_dydeta of several shards ----
@lru_cache(maxsize=None)
def eta_reference(name):
    """2+1D: what dN_dydeta is held to -- df_mode 1: the oracle on one-point eta grids (first, middle, last node) and its per-cell sum;
    df_mode 4: the restatement's rows"""
    b = inputs_of(name)
    cells, sp, g, o = b["cells"], b["sp"], b["grid"], b["opts"]
    if b["fq"] is not None:
        return dict(eta=dndx_feqmod_ref.dndx(cells, sp, g, b["df"], b["fq"], o)["eta"])
    K = len(g["eta"])
    nodes = {}
    for k in sorted({0, K // 2, K - 1}):
        g1 = dict(g, eta=g["eta"][k:k + 1], eta_w=g["eta_w"][k:k + 1])
        nodes[k] = contract(oracle.dN_pTdpTdphidy(cells, sp, g1, b["df"], o), sp, g1, 2) / g["eta_w"][k]
    return dict(nodes=nodes, total=oracle_cells(cells, range(len(cells["tau"])), sp, g, b["df"], o).sum(axis=1))


def eta_error(name, res):
    ref, g = eta_reference(name), inputs_of(name)["grid"]
    if "eta" in ref:
        return err_vs_max(res["dN_dydeta"], ref["eta"]), 1e-9
    errs = [err_vs_max(res["dN_dydeta"][:, k], v) for k, v in ref["nodes"].items()]
    errs.append(err_vs_max(res["dN_dydeta"] @ g["eta_w"], ref["total"]))
    return max(errs), 1e-10


@pytest.mark.parametrize("shards", SHARDS[1:])
@pytest.mark.parametrize("name", ["2d-df1", "2d-df4"])
def test_2d_dN_dydeta_of_several_shards(name, shards):
    b, single = inputs_of(name), reference(name)
    got = multi_of(b, [0] * shards)
    err, tol = eta_error(name, got)
    e1, _ = eta_error(name, single)
    diff = float(np.max(np.abs(got["dN_dydeta"] - single["dN_dydeta"]) / np.maximum(np.abs(single["dN_dydeta"]), 1e-300)))
    print("%s, %d shards: dN_dydeta error %.3e (single device %.3e, tolerance %.0e); worst relative difference to the single-device "
          "row %.3e" % (name, shards, err, e1, tol, diff))
    assert err < tol
    again = multi_of(b, [0] * shards)
    assert again["dN_dydeta"].tobytes() == got["dN_dydeta"].tobytes()
    if api.load().is3d_device_count() >= shards:   # a box with that many GPUs: the device list does not change the bits
        spread = multi_of(b, shards)
        assert spread["dN_dydeta"].tobytes() == got["dN_dydeta"].tobytes()
        assert_same_bits(spread, single)


# ---- 3. shards and cells ----
def subset(b, idx):
    cells = {k: np.ascontiguousarray(v[idx]) for k, v in b["cells"].items()}
    return dict(b, cells=cells)


@pytest.mark.parametrize("name", ["3d-df2-baryon", "2d-df4"])
def test_more_shards_than_cells(name):
    b = subset(inputs_of(name), slice(0, 3))
    want = one_shot_of(b)
    got = multi_of(b, [0] * 5)
    assert_same_bits(got, want)
    if CASES[name][0] == 3:
        assert_same_bits(got, want, ["dN_dydeta"])
    else:
        # three one-cell rows added in another association than the single device's: a few ulp of sums of same-signed terms
        assert err_vs_max(got["dN_dydeta"], want["dN_dydeta"]) < 1e-13
    assert [s["n_passes"] for s in got["shard_stats"]] == [1, 1, 1, 0, 0]
    assert np.any(got["dN_dy"] > 0.0)


@pytest.mark.parametrize("name", ["3d-df1", "2d-df1", "3d-df4"])
def test_skipped_cells_fill_one_whole_shard(name):
    b = inputs_of(name)
    n = len(b["cells"]["tau"])
    lo, hi = api.shard_bounds(n, 1, 3)
    cells = {k: v.copy() for k, v in b["cells"].items()}
    cells["dat"][lo:hi] = -np.abs(cells["dat"][lo:hi])   # u.dsigma = ut dat <= 0: the reference skips the cell
    for k in ("dax", "day", "dan"):
        cells[k][lo:hi] = 0.0
    b = dict(b, cells=cells)
    assert not live(cells)[lo:hi].any() and live(cells)[:lo].any() and live(cells)[hi:].any()
    want = one_shot_of(b)
    got = multi_of(b, [0, 0, 0])
    assert_same_bits(got, want)
    assert np.all(got["dN_dy_cell"][:, lo:hi] == 0.0)
    assert got["shard_stats"][1]["n_cells_skipped"] == hi - lo
    assert got["stats"]["n_cells_skipped"] == want["stats"]["n_cells_skipped"]


@pytest.mark.parametrize("name", ["3d-df1", "2d-df4"])
def test_empty_surface(name):
    b = subset(inputs_of(name), slice(0, 0))
    want = one_shot_of(b)
    got = multi_of(b, [0, 0, 0])
    assert_same_bits(got, want, api.SPACETIME_OUTPUTS)
    assert not got["dN_dy"].any() and got["dN_dy_cell"].shape[1] == 0


# ---- 4. passes inside a shard ----
@pytest.mark.parametrize("name", ["3d-df2-baryon", "3d-df3-breakdown", "2d-df1"])
def test_workspace_passes_inside_a_shard(name):
    b, want = inputs_of(name), reference(name)
    capped = dict(b, opts=dict(b["opts"], workspace_bytes=1 << 14))
    got = multi_of(capped, [0, 0])
    for s in got["shard_stats"]:
        assert s["n_passes"] >= 2, got["shard_stats"]
    assert_same_bits(got, want)
    if CASES[name][0] == 3:
        assert_same_bits(got, want, ["dN_dydeta"])
    else:
        assert eta_error(name, got)[0] < 1e-10


# ---- 5. the power-of-two p.dsigma scale ----
def test_pds_bound_2_to_the_40_between_shards():
    """one shard's largest |p.dsigma| is 2^45 times another's: the records take the bound of the whole surface, D stays bitwise.  (Every
    scaled term of this surface stays a normal number, where a power-of-two scale commutes with each rounding whatever the bound: this is
    the benign range.  The next test builds the range in which a shard-local bound changes the bits.)"""
    b = inputs_of("3d-df1")
    n = len(b["cells"]["tau"])
    lo, hi = api.shard_bounds(n, 2, 3)
    cells = {k: v.copy() for k, v in b["cells"].items()}
    for k in ("dat", "dax", "day", "dan"):
        cells[k][lo:hi] *= 2.0 ** -45

    def bound(c, sl):   # cf_pds_bound's per-cell quantity up to the grid's constants: it scales with dsigma
        return float(np.max(np.abs(c["dat"][sl]) + np.abs(c["dan"][sl] / c["tau"][sl]) + np.abs(c["dax"][sl]) + np.abs(c["day"][sl])))
    assert bound(cells, slice(0, lo)) >= 2.0 ** 40 * bound(cells, slice(lo, hi))
    b = dict(b, cells=cells)
    want = one_shot_of(b)
    for shards in (2, 3, 7):
        got = multi_of(b, [0] * shards)
        assert_same_bits(got, want, api.SPACETIME_OUTPUTS)
    assert np.any(want["dN_dy_cell"][:, lo:hi] > 0.0)


def test_pds_bound_where_a_shard_local_scale_changes_the_bits():
    """The range the exchange exists for.  The cells of the last shard sit 6-8 units of rapidity beyond the y grid, so every term of the
    proton lanes is near the bottom of the double range, and their dsigma is 2^-45 of the others': under the surface's bound their scaled
    terms fall into the denormal range, under a bound of their own they do not.  Run ALONE (a single-device call on those cells: the bound
    a shard would take without the exchange) their D has other bits than in the whole surface -- and the sharded call still gives the
    whole surface's bits, because every shard uses the surface's bound."""
    b0 = OC.op0_inputs(3, (8, 5, 15), 1, OC.TWO, 61, {}, False, 7100)
    n = len(b0["cells"]["tau"])
    lo, hi = api.shard_bounds(n, 2, 3)
    hazard = 0
    for shift in np.arange(6.0, 8.01, 0.25):
        cells = {k: v.copy() for k, v in b0["cells"].items()}
        cells["eta"][lo:hi] = shift
        for k in ("dat", "dax", "day", "dan"):
            cells[k][lo:hi] *= 2.0 ** -45
        b = dict(b0, cells=cells)
        whole = one_shot_of(b)
        alone = one_shot_of(subset(b, slice(lo, hi)))
        differ = int(np.sum(whole["dN_dy_cell"][:, lo:hi] != alone["dN_dy_cell"]))
        print("eta %.2f: %d of %d values of the shard's dN_dy_cell differ between the shard alone and the whole surface; %d are non-zero"
              % (shift, differ, alone["dN_dy_cell"].size, int(np.count_nonzero(whole["dN_dy_cell"][:, lo:hi]))))
        hazard += differ
        assert_same_bits(multi_of(b, [0, 0, 0]), whole, api.SPACETIME_OUTPUTS)
    assert hazard > 0   # else this surface never reached the range and the test shows nothing


# ---- 6. errors ----
@pytest.mark.parametrize("name", ["3d-df1", "2d-df4"])
def test_cell_outside_the_table_in_the_last_shard(name):
    b = inputs_of(name)
    n = len(b["cells"]["tau"])
    lo, hi = api.shard_bounds(n, 2, 3)
    cells = {k: v.copy() for k, v in b["cells"].items()}
    bad = lo + 3
    cells["T"][bad] = 5.0
    with pytest.raises(api.Is3dError) as e:
        multi_of(dict(b, cells=cells), [0, 0, 0])
    assert e.value.code == api.IS3D_EDOMAIN
    assert e.value.bad_cell == bad and e.value.stats["bad_cell"] == bad and ("cell %d" % bad) in str(e.value)
    ss = e.value.shard_stats
    assert ss[2]["bad_cell"] == 3 and ss[2]["code"] == api.IS3D_EDOMAIN
    assert ss[0]["bad_cell"] == -1 and ss[1]["bad_cell"] == -1 and ss[0]["code"] == 0


def test_refusals_leave_the_resource_counters_alone():
    b = inputs_of("3d-df1")
    visible = api.load().is3d_device_count()
    no_x = dict(b, cells={k: v for k, v in b["cells"].items() if k != "x"})
    tries = [(no_x, [0, 0], "x and y"), (dict(b, bins=dict(b["bins"], r_bins=0)), [0, 0], "r_bins"),
             (dict(b, bins=dict(b["bins"], tau_max=b["bins"]["tau_min"])), [0, 0], "tau_max"),
             (dict(b, opts=dict(b["opts"], df_mode=4)), [0, 0], "fq is NULL"),
             (dict(b, grid=OC.make_grid(65, 3, 2, 3, 5)), [0, 0], "64"),
             (b, [0, -2], "devices[1] = -2"), (b, visible + 1, "n_devices = %d" % (visible + 1)), (b, [0, visible], "devices[1] = %d" % visible)]
    for args, devices, needle in tries:
        before = api.resource_counters()
        with pytest.raises(api.Is3dError) as e:
            multi_of(args, devices)
        assert e.value.code == api.IS3D_EINVAL and needle in str(e.value), str(e.value)
        assert api.resource_counters() == before, needle


# ---- 7. stats ----
@pytest.mark.parametrize("name", ["3d-df2-baryon", "2d-df4"])
def test_stats_are_summed_over_the_shards(name):
    b = inputs_of(name)
    cells = {k: v.copy() for k, v in b["cells"].items()}
    n = len(cells["tau"])
    skip = [2, n // 2, n - 1]   # u.dsigma <= 0 in three shards of the four
    cells["dat"][skip] = -np.abs(cells["dat"][skip])
    for k in ("dax", "day", "dan"):
        cells[k][skip] = 0.0
    bins = dict(b["bins"], tau_min=float(np.median(cells["tau"])), r_min=float(np.median(np.hypot(cells["x"], cells["y"]))))
    b = dict(b, cells=cells, bins=bins)   # half of the cells below the first tau and r bin
    want = one_shot_of(b)
    got = multi_of(b, [0] * 4)
    assert_same_bits(got, want)
    assert want["stats"]["n_tau_negative"] > 0 and want["stats"]["n_r_negative"] > 0 and want["stats"]["n_cells_skipped"] == 3
    for k in ("n_tau_outside", "n_r_outside", "n_tau_negative", "n_r_negative", "n_cells_skipped", "n_classes"):
        assert got["stats"][k] == want["stats"][k], k
    assert sum(s["n_cells_skipped"] for s in got["shard_stats"]) == want["stats"]["n_cells_skipped"]
    assert {s["n_classes"] for s in got["shard_stats"]} == {want["stats"]["n_classes"]}
    assert got["stats"]["bad_cell"] == -1 and all(s["bad_cell"] == -1 for s in got["shard_stats"])
    assert got["stats"]["ms_cells"] == max(s["ms_cells"] for s in got["shard_stats"]) > 0.0
    assert got["stats"]["ms_bins"] > 0.0
    # the placement of a shard's D blocks in the assembled D is timed and counted in ms_d2h, next to the read-back
    assert all(s["ms_d2h"] > 0.0 for s in got["shard_stats"])
    assert got["stats"]["ms_d2h"] >= max(s["ms_d2h"] for s in got["shard_stats"])


# ---- 8. distinct devices ----
@pytest.mark.skipif(api.load().is3d_device_count() < 2, reason="needs two GPUs")
@pytest.mark.parametrize("name", ["3d-df2-baryon", "3d-df4", "2d-df4"])
def test_two_distinct_devices(name):
    b, want = inputs_of(name), reference(name)
    got = multi_of(b, [0, 1])
    assert_same_bits(got, want)
    if CASES[name][0] == 3:
        assert_same_bits(got, want, ["dN_dydeta"])
    else:
        assert got["dN_dydeta"].tobytes() == multi_of(b, [0, 0])["dN_dydeta"].tobytes()
    assert_bins_are_running_sums(got, b)
