"""CPU: the three one-shot entries of operation 0 -- is3d_spacetime_distributions (df_mode 1 / 2), is3d_spacetime_distributions_feqmod
(df_mode 3 / 4) and is3d_spacetime_distributions_vah -- share their argument checks (cf_spacetime_host.cpp): the same malformed input gets the
same return code and the same is3d_last_error() text from each of them, before any device is used or plan created (is3d_resource_counters
does not move), so on a machine with or without a GPU alike.  The smallest shapes: 1 species, 1 cell, 4 pT values, 8 phi values."""
import ctypes as C

import numpy as np
import pytest

from is3d_amd import api, inputs, synth

ENTRIES = ("df", "feqmod", "vah")
BINS = dict(tau_min=0.5, tau_max=8.0, tau_bins=3, r_min=0.0, r_max=6.0, r_bins=2)
NPT, NPHI = 4, 8
LDS_BYTES = dict(df=64 * 1024, feqmod=48 * 1024, vah=64 * 1024)   # what each entry's per-cell kernel has for its 2+1D eta rows


def npTp_of(npT):
    p = 1
    while p < npT:
        p *= 2
    return p


def max_eta(entry, npT):
    """[4 waves][64 / npTp classes][K] doubles within the entry's LDS"""
    return LDS_BYTES[entry] // (8 * 4 * (64 // npTp_of(npT)))


def grid_of(npT=NPT, n_eta=3):
    g = inputs.grid()
    return dict(pT=np.linspace(0.1, 3.0, npT), phi=g["phi"][:NPHI], y=g["y"][:2], eta=np.linspace(-2.0, 2.0, n_eta), eta_w=np.full(n_eta, 0.1),
                pT_w=np.full(npT, 0.1), phi_w=g["phi_w"][:NPHI])


def call(entry, dim=3, bins=BINS, null=(), npT=NPT, n_eta=3):
    """The C entry itself, so that any pointer can be NULL: (return code, error text, stats).  The outputs of a refused call are never
    written: one small array stands behind each."""
    lib = api.load()
    grid = grid_of(npT, n_eta)
    vah = entry == "vah"
    surface = synth.synth_vah_surface(1, dim, seed=5) if vah else synth.synth_surface(1, dim, seed=5)
    df = api._VAH_DUMMY_DF if vah else inputs.df_tables()
    opts = dict(dimension=dim) if vah else dict(dimension=dim, df_mode=dict(df=1, feqmod=4)[entry])
    sps, gs, ds, os_, _, keep = api._pack_common(inputs.species([211]), grid, df, opts)
    held = []
    if vah:
        cs = api._vah_cells_struct({k: v for k, v in surface.items() if k in api.VAH_FIELDS}, held)
    else:
        cs = api.Cells()
        cs.n_cells = 1
        for f in api.CELL_FIELDS:
            if surface.get(f) is not None:
                held.append(api._f64(surface[f]))
                setattr(cs, f, held[-1].ctypes.data)
    xa, ya = api._f64(surface["x"]), api._f64(surface["y"])
    pw, fw = api._f64(grid["pT_w"]), api._f64(grid["phi_w"])
    res = {k: np.zeros(8) for k in api.SPACETIME_OUTPUTS}
    so = api.SpacetimeOut(*[None if k in null else res[k].ctypes.data for k in api.SPACETIME_OUTPUTS])
    bb = api._spacetime_bins(bins)
    x, y, pb = (None if k in null else v for k, v in (("x", api._p(xa)), ("y", api._p(ya)), ("bins", C.byref(bb))))
    st = api.SpacetimeStats()
    head = (C.byref(cs), x, y, C.byref(sps), C.byref(gs), api._p(pw), api._p(fw))
    if vah:
        rc = lib.is3d_spacetime_distributions_vah(*head, None, C.byref(os_), pb, C.byref(so), C.byref(st))
    elif entry == "feqmod":
        fqs = api._pack_feqmod(inputs.feqmod_tables(inputs.surface_average_T(surface)), keep)
        rc = lib.is3d_spacetime_distributions_feqmod(*head, C.byref(ds), C.byref(fqs), C.byref(os_), pb, C.byref(so), C.byref(st), None)
    else:
        rc = lib.is3d_spacetime_distributions(*head, C.byref(ds), C.byref(os_), pb, C.byref(so), C.byref(st))
    return rc, lib.is3d_last_error().decode(), st


RANGES = "the bin ranges need tau_max > tau_min and r_max > r_min (got [0.5, 0.5], [0, 6])"
MALFORMED = [
    ("null-x", dict(null=("x",)), "operation 0 needs the cells' x and y positions (NULL given)"),
    ("null-bins", dict(null=("bins",)), "null spacetime bins"),
    ("tau-bins-0", dict(bins=dict(BINS, tau_bins=0)), "tau_bins and r_bins must be >= 1 (got 0, 2)"),
    ("empty-tau-range", dict(bins=dict(BINS, tau_max=BINS["tau_min"])), RANGES),
    ("bins-past-2^28", dict(bins=dict(BINS, tau_bins=(1 << 14) + 1, r_bins=1 << 14)), "tau_bins x r_bins too large"),
    ("65-pT", dict(npT=65), "operation 0 takes pT grids of up to 64 values (got 65)"),
    ("65-pT-2d", dict(npT=65, dim=2), "operation 0 takes pT grids of up to 64 values (got 65)"),
    ("null-output-array", dict(null=("dN_twopirdrdy",)), "a required output array is NULL"),
    ("null-output-array-2d", dict(null=("dN_dydeta",), dim=2), "a required output array is NULL"),
]


@pytest.mark.parametrize("name,how,text", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_the_same_refusal_from_every_entry(name, how, text):
    before = api.resource_counters()
    got = {e: call(e, **how) for e in ENTRIES}
    assert api.resource_counters() == before
    for e, (rc, msg, st) in got.items():
        assert (rc, msg) == (api.IS3D_EINVAL, text), e
        assert st.code == api.IS3D_EINVAL and st.bad_cell == -1, e
    assert len({(rc, msg) for rc, msg, _ in got.values()}) == 1


@pytest.mark.parametrize("npT", [NPT, 1, 64])
def test_one_eta_node_past_each_entrys_lds_bound(npT):
    """2+1D: each entry refuses the first eta count its kernel's LDS does not hold -- the bound computed here from npTp and the entry's LDS, 64
    KiB, or 48 KiB for the modified equilibrium -- in the same words, and lets the count before it through to the search for a device."""
    before = api.resource_counters()
    for e in ENTRIES:
        K = max_eta(e, npT)
        rc, msg, st = call(e, dim=2, npT=npT, n_eta=K + 1)
        assert (rc, msg) == (api.IS3D_EINVAL, "operation 0 in 2+1D: %d pT values x %d eta nodes need more LDS than the per-cell kernel has (up to "
                             "%d eta nodes with this pT grid)" % (npT, K + 1, K)), e
        assert st.code == api.IS3D_EINVAL
    assert api.resource_counters() == before
    assert max_eta("feqmod", npT) * 4 == max_eta("df", npT) * 3 == max_eta("vah", npT) * 3
    if api.load().is3d_device_count() < 1:   # (with a device the largest tables run in tests/test_gpu_offtile.py)
        for e in ENTRIES:
            rc, msg, _ = call(e, dim=2, npT=npT, n_eta=max_eta(e, npT))
            assert rc == api.IS3D_ENODEVICE and "no CPU path" in msg, (e, msg)
        assert api.resource_counters() == before
