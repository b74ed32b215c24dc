"""GPU (-m gpu): is3d_smooth_spectra_vah_multi -- the anisotropic-hydro spectra (mode 2) with the cells sharded over a device list -- and
is3d_vah_plan_observables.  One device with repeated ordinals: the shard spectra are the single-device entry's on the cells of
is3d_shard_bounds, added in the fixed binary tree the header defines for IS3D_REDUCE_ORDERED, so the expected bits are built from
api.smooth_spectra_vah and numpy additions; the oracle and the single-device result bound the whole."""
import numpy as np
import pytest

from conftest import relerr
from is3d_amd import api, inputs, synth
from oracle import oracle  # the checker

pytestmark = pytest.mark.gpu
TOL = 2e-9                 # tests/test_gpu_vah.py: device against oracle
CASES = [(3, True), (3, False), (2, True), (2, False)]
IDS = ["3d-tables", "3d-cell-coefficients", "2d-tables", "2d-cell-coefficients"]

_cache = {}


def case(fx, dim, with_tab):
    """The surface of tests/test_gpu_vah.py's shapes (70 cells in 3+1D, 9 in 2+1D), its single-device spectrum and the oracle's, computed once."""
    key = (dim, with_tab)
    if key not in _cache:
        cells = synth.synth_vah_surface(70 if dim == 3 else 9, dim, seed=940 + dim)
        tab = inputs.vah_df_tables() if with_tab else None
        o = dict(dimension=dim)
        single, st = api.smooth_spectra_vah(cells, fx["pikp"], fx["grid"], o, tab=tab)
        coef = {}
        if with_tab:
            coef, found = oracle.vah_coefficients(tab, cells["Lambda"], cells["aL"])
            assert found.all()
        ref = oracle.dN_pTdpTdphidy_vah(dict(cells, **coef), fx["pikp"], fx["grid"], o)
        for a in (single, ref):
            a.setflags(write=False)
        _cache[key] = dict(cells=cells, tab=tab, o=o, n=len(cells["tau"]), single=single, st=st, ref=ref, parts={})
    return _cache[key]


def shard_spectra(fx, c, n_shards):
    """s_i: the single-device entry on the cells of api.shard_bounds(n, i, n_shards)"""
    if n_shards not in c["parts"]:
        out = []
        for i in range(n_shards):
            lo, hi = api.shard_bounds(c["n"], i, n_shards)
            s, _ = api.smooth_spectra_vah({k: v[lo:hi] for k, v in c["cells"].items()}, fx["pikp"], fx["grid"], c["o"], tab=c["tab"])
            out.append(s)
        c["parts"][n_shards] = out
    return c["parts"][n_shards]


def multi(fx, c, devices, cells=None, opts=None, **kw):
    return api.smooth_spectra_vah_multi(c["cells"] if cells is None else cells, fx["pikp"], fx["grid"], dict(c["o"], **(opts or {})), devices,
                                        tab=c["tab"], **kw)


@pytest.mark.parametrize("dim,with_tab", CASES, ids=IDS)
def test_one_shard_is_the_single_device_entry(fx, dim, with_tab):
    c = case(fx, dim, with_tab)
    got, st = multi(fx, c, [0])
    assert np.array_equal(got, c["single"])
    assert len(st["shards"]) == 1 and st["code"] == 0 and st["shards"][0]["code"] == 0
    assert st["n_passes"] == c["st"]["n_passes"] and st["n_wave_rows"] == c["st"]["n_wave_rows"] and st["kernel_variant"] == 3


@pytest.mark.parametrize("dim,with_tab", CASES, ids=IDS)
def test_three_and_five_shards_add_in_the_fixed_tree(fx, dim, with_tab):
    c = case(fx, dim, with_tab)
    s = shard_spectra(fx, c, 3)
    got3, st3 = multi(fx, c, [0, 0, 0])
    assert np.array_equal(got3, (s[0] + s[1]) + s[2])
    s = shard_spectra(fx, c, 5)
    got5, st5 = multi(fx, c, [0] * 5)
    assert np.array_equal(got5, ((s[0] + s[1]) + (s[2] + s[3])) + s[4])
    for got, st, k in ((got3, st3, 3), (got5, st5, 5)):
        e_single, e_oracle = relerr(got, c["single"], floor=1e-250), relerr(got, c["ref"], floor=1e-270)
        print("%d shards: against the single device %.3e, against the oracle %.3e" % (k, e_single, e_oracle))
        assert e_single < 1e-10           # the bound test_vah_config5_size_properties puts on sums of parts
        assert e_oracle < TOL
        assert len(st["shards"]) == k and st["code"] == 0 and st["bad_cell"] == -1 and st["n_classes"] == c["st"]["n_classes"]
        assert st["n_wave_rows"] == sum(t["n_wave_rows"] for t in st["shards"]) and st["n_wave_rows"] > 0
        assert st["n_passes"] == 1 and st["ms_main"] == max(t["ms_main"] for t in st["shards"]) and st["ms_main"] > 0 and st["ms_d2h"] > 0
    again, _ = multi(fx, c, [0, 0, 0])
    assert np.array_equal(again, got3)    # a second call: the same bits


@pytest.mark.parametrize("dim,with_tab", CASES, ids=IDS)
def test_fewer_cells_than_shards(fx, dim, with_tab):
    c = case(fx, dim, with_tab)
    two = {k: v[:2] for k, v in c["cells"].items()}
    s = [api.smooth_spectra_vah({k: v[i:i + 1] for k, v in two.items()}, fx["pikp"], fx["grid"], c["o"], tab=c["tab"])[0] for i in range(2)]
    got, st = multi(fx, c, [0, 0, 0, 0], cells=two)
    zero = np.zeros_like(got)
    assert np.array_equal(got, (s[0] + s[1]) + (zero + zero))    # shards 2 and 3 have no cells
    whole, _ = api.smooth_spectra_vah(two, fx["pikp"], fx["grid"], c["o"], tab=c["tab"])
    assert relerr(got, whole, floor=1e-250) < 1e-10
    assert [t["n_wave_rows"] > 0 for t in st["shards"]] == [True, True, False, False]
    none = {k: v[:0] for k, v in c["cells"].items()}
    empty, st = multi(fx, c, [0, 0], cells=none)
    assert empty.shape == c["single"].shape and not empty.any() and st["code"] == 0 and st["n_passes"] == 0
    kept = np.full_like(empty, 3.25)
    multi(fx, c, [0, 0], cells=none, opts=dict(accumulate=1), out=kept)
    assert (kept == 3.25).all()                                  # accumulate: no cells leave dN_out alone


@pytest.mark.parametrize("dim,with_tab", CASES, ids=IDS)
def test_accumulate_adds_the_combined_result_on_the_host(fx, dim, with_tab):
    c = case(fx, dim, with_tab)
    three, _ = multi(fx, c, [0, 0, 0])
    prefill = np.random.default_rng(11).random(three.size) * np.abs(three).max()
    out = prefill.copy()
    got, _ = multi(fx, c, [0, 0, 0], opts=dict(accumulate=1), out=out)
    assert got is out and np.array_equal(out, prefill + three)


@pytest.mark.parametrize("dim", [3, 2])
def test_a_cell_beyond_the_tables_is_edomain_with_its_global_index(fx, dim):
    """(a status word only, as in tests/test_gpu_vah.py: cf_vah_coeffs reports the cell and stores zeros for it)"""
    c = case(fx, dim, True)
    lo2, hi2 = api.shard_bounds(c["n"], 2, 3)
    local = (hi2 - lo2) // 2
    bad = {k: v.copy() for k, v in c["cells"].items()}
    bad["aL"][lo2 + local] = 2.5
    with pytest.raises(api.Is3dError) as e:
        multi(fx, c, [0, 0, 0], cells=bad)
    assert e.value.code == api.IS3D_EDOMAIN and e.value.bad_cell == lo2 + local
    assert "cell %d of the surface" % (lo2 + local) in str(e.value) and "shard 2 (device 0)" in str(e.value) and "beyond the last node" in str(e.value)
    st = e.value.status
    assert st["code"] == api.IS3D_EDOMAIN and st["bad_cell"] == lo2 + local
    assert st["shards"][2]["bad_cell"] == local and st["shards"][2]["code"] == api.IS3D_EDOMAIN
    assert [t["code"] for t in st["shards"][:2]] == [0, 0] and [t["bad_cell"] for t in st["shards"][:2]] == [-1, -1]
    assert all(t["n_wave_rows"] > 0 for t in st["shards"][:2])          # a failed shard does not stop the others
    bad["aL"][1] = 2.5                                                  # a second one, in shard 0: the lower global index wins
    with pytest.raises(api.Is3dError) as e:
        multi(fx, c, [0, 0, 0], cells=bad)
    assert e.value.code == api.IS3D_EDOMAIN and e.value.bad_cell == 1
    assert "cell 1 of the surface" in str(e.value) and "shard 0 (device 0)" in str(e.value)
    assert e.value.status["shards"][0]["bad_cell"] == 1 and e.value.status["shards"][2]["bad_cell"] == local


def test_the_exponent_domain_check_keeps_its_global_index_too(fx):
    c = case(fx, 3, False)
    bad = {k: v.copy() for k, v in c["cells"].items()}
    bad["Lambda"][41] = 1e-12
    lo, _ = api.shard_bounds(c["n"], 1, 3)
    with pytest.raises(api.Is3dError) as e:
        multi(fx, c, [0, 0, 0], cells=bad)
    assert e.value.code == api.IS3D_EDOMAIN and e.value.bad_cell == 41 and "cell 41 of the surface" in str(e.value) and "1e9" in str(e.value)
    assert e.value.status["shards"][1]["bad_cell"] == 41 - lo


@pytest.mark.parametrize("dim", [3, 2])
def test_passes_over_a_shards_cells(fx, dim):
    """workspace_bytes = 256 KiB holds 31 cells of the 3+1D record stream and 2 of the 2+1D one: the 35 / 5 cells of a shard of two take
    several passes.  The bound is the one test_vah_2d_factored_kernel_against_the_round1_kernel puts on passes."""
    c = case(fx, dim, True)
    free, st_free = multi(fx, c, [0, 0])
    got, st = multi(fx, c, [0, 0], opts=dict(workspace_bytes=1 << 18))
    assert st_free["n_passes"] == 1 and st["n_passes"] > 1 and st["n_passes"] == max(t["n_passes"] for t in st["shards"])
    scale = np.abs(free).max()
    err = float(np.max(np.abs(got - free) / np.maximum(np.abs(free), 1e-12 * scale)))
    print("passes, dimension %d: %d passes, %.3e" % (dim, st["n_passes"], err))
    assert err < 1e-13


def test_rccl_needs_distinct_devices(fx):
    c = case(fx, 3, True)
    with pytest.raises(api.Is3dError) as e:
        multi(fx, c, [0, 0], reduce=api.REDUCE_RCCL)
    assert e.value.code == api.IS3D_EINVAL and "distinct" in str(e.value)
    got, st = multi(fx, c, [0], reduce=api.REDUCE_RCCL)      # one rank: nothing to reduce
    assert np.array_equal(got, c["single"]) and len(st["shards"]) == 1


@pytest.mark.parametrize("dim", [3, 2])
def test_vah_plan_observables(fx, dim):
    """VahPlan.observables on a spectrum resident in torch memory: bit for bit Plan.observables of a viscous plan with the same species and grid
    on the same buffer (the same kernels), and the numpy reductions of tests/test_gpu_parity.py::test_device_observables at its tolerances."""
    import torch
    c = case(fx, dim, True)
    g = fx["grid_w"]
    S, ny = len(fx["pikp"]["mass"]), 21 if dim == 3 else 1
    dev = torch.device("cuda:0")
    spectrum, _ = multi(fx, c, [0, 0, 0])
    buf = torch.from_numpy(spectrum).to(dev)
    vplan = api.VahPlan(fx["pikp"], fx["grid"], c["o"], tab=c["tab"], max_cells=1)
    plan = api.Plan(fx["pikp"], fx["grid"], fx["df"], dict(dimension=dim), max_cells=1)
    assert vplan.output_size == plan.output_size == buf.numel()
    st = torch.cuda.current_stream().cuda_stream
    sizes = (S * ny, S * ny * 32, S * ny * 32 * 7)
    mine = [torch.full((k,), -7.0, dtype=torch.float64, device=dev) for k in sizes]
    theirs = [torch.full((k,), -7.0, dtype=torch.float64, device=dev) for k in sizes]
    vplan.observables(buf.data_ptr(), g["pT_w"], g["phi_w"], *[t.data_ptr() for t in mine], st)
    plan.observables(buf.data_ptr(), g["pT_w"], g["phi_w"], *[t.data_ptr() for t in theirs], st)
    torch.cuda.synchronize()
    dndy, s2pi, vn = [t.cpu().numpy() for t in mine]
    for a, b in zip((dndy, s2pi, vn), theirs):
        assert np.array_equal(a, b.cpu().numpy()) and not (a == -7.0).any()
    r4 = c["ref"].reshape(ny, 24, 32, S)
    want_dndy = np.einsum("j,i,kjis->sk", g["phi_w"], g["pT_w"], r4)
    want_s2pi = np.einsum("j,kjis->ski", g["phi_w"], r4) / (2.0 * np.pi)
    print("observables, dimension %d: dN/dy %.3e, dN/2pipTdpTdy %.3e" % (dim, relerr(dndy.reshape(S, ny), want_dndy), relerr(s2pi.reshape(S, ny, 32), want_s2pi)))
    assert relerr(dndy.reshape(S, ny), want_dndy) < TOL
    assert relerr(s2pi.reshape(S, ny, 32), want_s2pi) < TOL
    den = np.einsum("j,kjis->ski", g["phi_w"], r4)
    got_vn = vn.reshape(S, ny, 32, 7)
    for k in range(7):
        num = np.abs(np.einsum("j,kjis->ski", np.exp(1j * (k + 1) * g["phi"]) * g["phi_w"], r4))
        want = np.where(den < 1e-15, 0.0, num / np.where(den == 0, 1.0, den))
        ok = den > 1e-200            # where the spectrum is ~1e-300 the ratio is numerical noise in both
        assert np.max(np.abs(got_vn[:, :, :, k] - want)[ok]) < 1e-7
        assert (got_vn[:, :, :, k][den < 1e-15] == 0.0).all()
    # pointers left 0 are not written
    only = [torch.full((k,), -7.0, dtype=torch.float64, device=dev) for k in sizes]
    vplan.observables(buf.data_ptr(), g["pT_w"], g["phi_w"], dndy_ptr=only[0].data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(only[0].cpu().numpy(), dndy) and (only[1] == -7.0).all() and (only[2] == -7.0).all()
    only[0].fill_(-7.0)
    vplan.observables(buf.data_ptr(), None, g["phi_w"], vn_ptr=only[2].data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(only[2].cpu().numpy(), vn) and (only[0] == -7.0).all() and (only[1] == -7.0).all()
    with pytest.raises(api.Is3dError) as e:      # dN/dy needs the pT weights, as is3d_plan_observables has it
        vplan.observables(buf.data_ptr(), None, g["phi_w"], dndy_ptr=only[0].data_ptr(), stream=st)
    assert e.value.code == api.IS3D_EINVAL
    vplan.close()
    plan.close()
