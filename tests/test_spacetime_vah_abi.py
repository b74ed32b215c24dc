"""CPU: operation 0 for anisotropic hydro -- is3d_spacetime_distributions_vah and is3d_vah_plan_execute_spacetime are exported with the
declared signatures and bound; the one-shot entry refuses bad arguments with IS3D_EINVAL and a message before any device is used or plan
created -- so on a box with or without a GPU alike -- and, given good arguments on a box without a GPU, fails with IS3D_ENODEVICE instead of
computing on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from is3d_amd import api, inputs, synth

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "is3d_amd.h")
BINS = dict(tau_min=0.5, tau_max=8.0, tau_bins=7, r_min=0.0, r_max=6.0, r_bins=5)


def inputs_of(dim=3, n_cells=7, **grid_over):
    g = inputs.grid()
    grid = dict(pT=g["pT"][:5], phi=g["phi"][:5], y=g["y"][:4], eta=g["eta"][:9], eta_w=g["eta_w"][:9], pT_w=g["pT_w"][:5], phi_w=g["phi_w"][:5])
    grid.update(grid_over)
    return dict(cells=synth.synth_vah_surface(n_cells, dim, seed=7272), sp=inputs.species("pikp"), grid=grid, opts=dict(dimension=dim))


def declared(name):
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S))
    m = re.search(r"int %s\(([^)]*)\);" % name, text)
    assert m, "the header does not declare %s" % name
    return [re.sub(r"\w+$", "", p.strip()).replace(" ", "") for p in m.group(1).split(",")]


def test_symbols_are_exported_with_the_declared_signatures():
    lib = api.load()
    for name in ("is3d_spacetime_distributions_vah", "is3d_vah_plan_execute_spacetime"):
        assert name in api.EXPORTS and hasattr(lib, name), name
    one = declared("is3d_spacetime_distributions_vah")
    assert one == ["constis3d_vah_cells*", "constdouble*", "constdouble*", "constis3d_species*", "constis3d_grid*", "constdouble*", "constdouble*",
                   "constis3d_vah_df_tables*", "constis3d_options*", "constis3d_spacetime_bins*", "is3d_spacetime_out*", "is3d_spacetime_stats*"]
    at = lib.is3d_spacetime_distributions_vah.argtypes
    assert len(at) == len(one) == 12
    assert at[0] == C.POINTER(api.VahCells) and at[7] == C.POINTER(api.VahDfTables) and at[9] == C.POINTER(api.SpacetimeBins)
    assert at[10] == C.POINTER(api.SpacetimeOut) and at[11] == C.POINTER(api.SpacetimeStats)
    # the plan entry: the arguments of is3d_plan_execute_spacetime behind the VAH plan and its cells
    plan = declared("is3d_vah_plan_execute_spacetime")
    assert plan == ["is3d_vah_plan*", "constis3d_vah_cells*"] + declared("is3d_plan_execute_spacetime")[2:]
    at = lib.is3d_vah_plan_execute_spacetime.argtypes
    assert len(at) == len(plan) == 10 and at[1] == C.POINTER(api.VahCells) and at[9] == C.POINTER(api.SpacetimeStats)
    assert callable(api.spacetime_distributions_vah) and callable(api.VahPlan.execute_spacetime)


def raw_call(b, bins=BINS, null=(), kernel_variant=0, tab=None):
    """The C entry itself, so that any pointer can be NULL: (return code, error text, stats)."""
    lib = api.load()
    sps, gs, _, os_, _, keep = api._pack_common(b["sp"], b["grid"], api._VAH_DUMMY_DF, dict(b["opts"], kernel_variant=kernel_variant))
    held = []
    cs = api._vah_cells_struct({k: v for k, v in b["cells"].items() if k in api.VAH_FIELDS}, held)
    n = cs.n_cells
    xa, ya = api._f64(b["cells"]["x"]), api._f64(b["cells"]["y"])
    pw, fw = api._f64(b["grid"]["pT_w"]), api._f64(b["grid"]["phi_w"])
    sized = dict(bins, tau_bins=max(bins["tau_bins"], 1), r_bins=max(bins["r_bins"], 1))   # the arrays of a refused call are never written
    shapes = api.spacetime_shapes(len(b["sp"]["mass"]), n, sized, b["opts"]["dimension"], len(b["grid"]["eta"]))
    res = {k: np.zeros(v) for k, v in shapes.items()}
    so = api.SpacetimeOut(*[None if k in null else res[k].ctypes.data for k in api.SPACETIME_OUTPUTS])
    bb = api._spacetime_bins(bins)
    ts = api._pack_vah_tables(tab, keep) if tab is not None else None
    a = dict(cells=C.byref(cs), x=api._p(xa), y=api._p(ya), species=C.byref(sps), grid=C.byref(gs), pT_w=api._p(pw), phi_w=api._p(fw),
             opts=C.byref(os_), bins=C.byref(bb), out=C.byref(so))
    for k in null:
        if k in a:
            a[k] = None
    st = api.SpacetimeStats()
    rc = lib.is3d_spacetime_distributions_vah(a["cells"], a["x"], a["y"], a["species"], a["grid"], a["pT_w"], a["phi_w"],
                                              C.byref(ts) if ts is not None else None, a["opts"], a["bins"], a["out"], C.byref(st))
    return rc, lib.is3d_last_error().decode(), st


REFUSALS = [
    ("null-x", dict(null=("x",)), {}, 3, "x and y"),
    ("null-y", dict(null=("y",)), {}, 2, "x and y"),
    ("null-pT-weights", dict(null=("pT_w",)), {}, 3, "null argument"),
    ("null-phi-weights", dict(null=("phi_w",)), {}, 3, "null argument"),
    ("null-cells", dict(null=("cells",)), {}, 3, "null argument"),
    ("null-out", dict(null=("out",)), {}, 3, "null argument"),
    ("null-bins", dict(null=("bins",)), {}, 3, "null spacetime bins"),
    ("null-output-array", dict(null=("dN_twopirdrdy",)), {}, 3, "output array is NULL"),
    ("tau-bins-0", dict(bins=dict(BINS, tau_bins=0)), {}, 3, "must be >= 1"),
    ("r-bins-negative", dict(bins=dict(BINS, r_bins=-2)), {}, 2, "must be >= 1"),
    ("empty-tau-range", dict(bins=dict(BINS, tau_max=BINS["tau_min"])), {}, 3, "tau_max > tau_min"),
    ("reversed-r-range", dict(bins=dict(BINS, r_min=3.0, r_max=1.0)), {}, 2, "r_max > r_min"),
    ("65-pT", {}, dict(pT=np.linspace(0.1, 3.0, 65), pT_w=np.full(65, 0.1)), 3, "up to 64 values"),
    # 2+1D: [4 waves][64 / npTp classes][K] doubles of LDS; 5 pT -> 8 lane slots -> 8 classes per wave: 256 eta nodes fit, 257 do not
    ("257-eta-with-5-pT", {}, dict(eta=np.linspace(-6, 6, 257), eta_w=np.full(257, 1.0)), 2, "more LDS"),
    ("kernel-variant-2", dict(kernel_variant=2), {}, 3, "kernel_variant 0 or 3"),
    ("kernel-variant-5", dict(kernel_variant=5), {}, 2, "kernel_variant 0 or 3"),
]


@pytest.mark.parametrize("with_tab", [False, True], ids=["cells-coefficients", "tables"])
@pytest.mark.parametrize("name,how,grid_over,dim,needle", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_arguments_are_refused_before_any_device_use(name, how, grid_over, dim, needle, with_tab):
    b = inputs_of(dim, **grid_over)
    before = api.resource_counters()
    rc, text, st = raw_call(b, tab=inputs.vah_df_tables() if with_tab else None, **how)
    assert rc == api.IS3D_EINVAL and needle in text, (rc, text)
    if "cells" not in how.get("null", ()):
        assert st.bad_cell == -1
    assert api.resource_counters() == before


def test_the_eta_bound_is_the_one_of_the_grid_check():
    """256 eta nodes with 5 pT values is the largest table that fits (the refusal above is the first that does not): it passes the argument
    checks, i.e. it gets as far as looking for a device."""
    b = inputs_of(2, eta=np.linspace(-6, 6, 256), eta_w=np.full(256, 1.0))
    rc, text, _ = raw_call(b)
    assert rc in (api.IS3D_OK, api.IS3D_ENODEVICE), (rc, text)


def test_a_missing_cell_array_is_refused_before_any_device_use():
    b = inputs_of()
    before = api.resource_counters()
    for drop, tab in (("aL", None), ("c3", None), ("Lambda", inputs.vah_df_tables())):
        with pytest.raises(api.Is3dError) as e:
            api.spacetime_distributions_vah({k: v for k, v in b["cells"].items() if k != drop}, b["sp"], b["grid"], BINS, b["opts"], tab=tab)
        assert e.value.code == api.IS3D_EINVAL and "VAH cell array is NULL" in str(e.value), drop
    assert api.resource_counters() == before


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("with_tab", [False, True], ids=["cells-coefficients", "tables"])
def test_good_call_without_a_device_is_enodevice(dim, with_tab):
    """(with a GPU the same call computes: tests/test_gpu_spacetime_vah.py)"""
    b = inputs_of(dim)
    tab = inputs.vah_df_tables() if with_tab else None
    if api.load().is3d_device_count() > 0:
        res = api.spacetime_distributions_vah(b["cells"], b["sp"], b["grid"], BINS, b["opts"], tab=tab)
        assert np.isfinite(res["dN_dy"]).all() and res["stats"]["n_cells_skipped"] == 0
        return
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        api.spacetime_distributions_vah(b["cells"], b["sp"], b["grid"], BINS, b["opts"], tab=tab)
    assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
    assert api.resource_counters() == before
