"""GPU (-m gpu): the shard rule of the sampler's five multi-device entries (is3d_sample_particles_multi, is3d_sample_binned_multi,
is3d_sample_fused_multi, is3d_sample_particles_vah_multi, is3d_sample_binned_vah_multi) at the smallest shapes at which it can go wrong:
more shards than cells, one active shard, no cells, a bad cell in a later shard, bad cells in two shards, a list buffer that is too small.
The yardstick is the single-device entry on the same arguments; every comparison is between integers or between the bits of two lists.

Shapes: 5 synthetic cells x 6 events, pi+ K+ p pbar, 3+1D; the volumes x 4000 so that a call keeps a few hundred hadrons (about 0.007 per
cell and event at volume 1: 30 000 cells x 7 events of tests/test_gpu_multi.py keep more than 1000).  Every test asserts its count first."""
import ctypes as C

import numpy as np
import pytest

from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu
PIKP = [211, 321, 2212, -2212]
ARRAYS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "vn_re", "vn_im", "yield")
COUNTERS = ("n_particles", "n_cells_skipped", "n_hadrons_drawn", "n_momentum_samples", "n_acceptances", "n_cells_breakdown")
BINS = dict(y_cut=2.0, y_bins=8, eta_cut=3.0, eta_bins=10, pT_lower_cut=0.1, pT_upper_cut=1.5, pT_bins=7, tau_min=1.0, tau_max=9.0, tau_bins=4,
            r_min=0.5, r_max=6.0, r_bins=3)            # the bins of the ABI tests
N_CELLS, N_EVENTS, VOLUME, FIRST = 5, 6, 4000.0, 1000
MIN_HADRONS = 200


def scaled(cells):
    v = {k: np.array(a, dtype=np.float64) for k, a in cells.items()}
    for f in ("dat", "dax", "day", "dan"):
        v[f] = VOLUME * v[f]
    return v


def part(cells, lo, hi):
    return {k: np.ascontiguousarray(a[lo:hi]) for k, a in cells.items()}


def same_list(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


def same_hist(a, b):
    return all(a[k].dtype == np.int64 and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in ARRAYS)


def same_counters(a, b):
    return all(a[k] == b[k] for k in COUNTERS)


class Family:
    """One sampler family as its list and binned wrappers with the family's fixed arguments bound: entry -> f(cells, **kw)."""

    def __init__(self, name, cells, entries, kw):
        self.name, self.cells, self.entries, self.kw = name, cells, entries, kw

    def run(self, entry, cells=None, **kw):
        return self.entries[entry](self.cells if cells is None else cells, **dict(self.kw, **kw))


@pytest.fixture(scope="module")
def fam():
    """The two families with the single-device result of every entry, computed once and left unchanged."""
    sp, df, gla, tab = inputs.species(PIKP), inputs.df_tables(), inputs.feqmod_tables(0.15), inputs.vah_df_tables()
    ov, oa = dict(dimension=3, df_mode=2), dict(dimension=3)
    vah = scaled(synth.synth_vah_surface(N_CELLS, 3, seed=9931))
    vah["bulkPi"] = 0.02 * vah["bulkPi"]
    out = dict(
        viscous=Family("viscous", scaled(synth.synth_surface(N_CELLS, 3, seed=9930)), dict(
            list=lambda c, **kw: api.sample_particles(c, sp, df, gla, ov, **kw),
            binned=lambda c, **kw: api.sample_binned(c, sp, df, gla, BINS, ov, **kw),
            fused=lambda c, **kw: api.sample_fused(c, sp, df, gla, BINS, ov, **kw)), dict(n_events=N_EVENTS, seed=17)),
        vah=Family("vah", vah, dict(
            list=lambda c, **kw: api.sample_particles_vah(c, sp, gla, oa, **kw),
            binned=lambda c, **kw: api.sample_binned_vah(c, sp, gla, BINS, oa, **kw)), dict(tab=tab, n_events=N_EVENTS, seed=18)))
    for f in out.values():
        f.single = {e: f.run(e) for e in f.entries}
        print(f.name, "hadrons", len(f.single["list"][0]), "per cell", np.bincount(f.single["list"][0]["cell"], minlength=N_CELLS))
    out["raw"] = dict(sp=sp, df=df, gla=gla, ov=ov)
    return out


ENTRIES = [("viscous", "list"), ("viscous", "binned"), ("viscous", "fused"), ("vah", "list"), ("vah", "binned")]
IDS = ["%s-%s" % e for e in ENTRIES]


def count_of(entry, result):
    return len(result[0]) if entry == "list" else int(result[0]["yield"].sum())


def same_result(entry, got, want):
    return (same_list if entry == "list" else same_hist)(got[0], want[0]) and same_counters(got[1], want[1])


# ---- 1. more shards than cells ----
@pytest.mark.parametrize("family,entry", ENTRIES, ids=IDS)
def test_more_shards_than_cells(fam, family, entry):
    """Seven shards of five cells: five one-cell shards and two that make no call."""
    f = fam[family]
    want = f.single[entry]
    assert count_of(entry, want) >= MIN_HADRONS and want[1]["n_particles"] == count_of(entry, want)
    got = f.run(entry, devices=[0] * 7)
    assert same_result(entry, got, want)


# ---- 2. one active shard: run_shards on the calling thread ----
@pytest.mark.parametrize("family,entry", [("viscous", "list"), ("viscous", "fused"), ("vah", "list"), ("vah", "binned")])
def test_one_active_shard(fam, family, entry):
    f = fam[family]
    k = int(np.argmax(np.bincount(f.single["list"][0]["cell"], minlength=N_CELLS)))       # the cell with the most hadrons
    one = part(f.cells, k, k + 1)
    want = f.run(entry, one, first_cell=k)
    assert count_of(entry, want) >= MIN_HADRONS // N_CELLS
    got = f.run(entry, one, first_cell=k, devices=[0, 0])
    assert same_result(entry, got, want)
    if entry == "list":                                            # ... and they are that cell's hadrons of the whole surface
        whole = f.single["list"][0]
        assert same_list(got[0], whole[whole["cell"] == k])


# ---- 3. the empty surface ----
@pytest.mark.parametrize("family,entry", ENTRIES, ids=IDS)
def test_the_empty_surface(fam, family, entry):
    f = fam[family]
    assert count_of(entry, f.single[entry]) >= MIN_HADRONS         # (the same call with cells is not empty)
    got, st = f.run(entry, part(f.cells, 0, 0), devices=[0, 0])
    assert st["n_particles"] == 0 and st["n_hadrons_drawn"] == 0
    if entry == "list":
        assert len(got) == 0 and got.dtype == api.PARTICLE_DTYPE
    else:
        want = f.single[entry][0]
        assert all(got[k].dtype == np.int64 and got[k].shape == want[k].shape and not got[k].any() for k in ARRAYS)


# ---- 4. a viscous bad cell in the second shard ----
def raw_binned_multi(name, raw, cells, devices, first_cell):
    """The entry `name` with histogram arrays that hold 7 everywhere at entry -> (return code, error text, histograms, n_particles)."""
    L = api.load()
    cs, sps, ds, si, os_, _held = api._pack_sampler(cells, raw["sp"], raw["df"], raw["gla"], raw["ov"], N_EVENTS, 17, 0.5, first_cell, None, 0,
                                                    0.0, 0.0, 0, 0.0)
    b = api._pack_bins(BINS)
    _, shapes = api._hist_arrays(BINS, N_EVENTS, sps.n)
    h, out = api._hist_arrays(BINS, N_EVENTS, sps.n, {k: np.full(a.shape, 7, dtype=np.int64) for k, a in shapes.items()})
    assert all((out[k] == 7).all() for k in ARRAYS)
    dv = (C.c_int32 * len(devices))(*devices)
    cnt, st = C.c_int64(-1), api.SamplerStats()
    rc = getattr(L, name)(C.byref(cs), C.byref(sps), C.byref(ds), C.byref(si), C.byref(os_), dv, C.c_int32(len(devices)), C.byref(b), C.byref(h),
                          C.byref(cnt), C.byref(st))
    return rc, L.is3d_last_error().decode(), out, int(cnt.value)


@pytest.mark.parametrize("entry", ["list", "binned", "fused"])
def test_a_viscous_bad_cell_in_the_second_shard(fam, entry):
    """T of cell 4 off the coefficient table; two shards.  The error is shard 1's own, as the single-device entry words it on that shard's
    slice; the binned and fused entries hand back zeroed histograms."""
    f = fam["viscous"]
    assert count_of(entry, f.single[entry]) >= MIN_HADRONS
    bad = {k: a.copy() for k, a in f.cells.items()}
    bad["T"][4] = 0.31
    lo, hi = api.shard_bounds(N_CELLS, 1, 2)
    assert lo <= 4 < hi and lo > 0
    with pytest.raises(api.Is3dError) as own:
        f.run(entry, part(bad, lo, hi), first_cell=FIRST + lo)
    assert own.value.code == api.IS3D_EDOMAIN and "cell %d" % (FIRST + 4) in str(own.value)
    with pytest.raises(api.Is3dError) as e:
        f.run(entry, bad, first_cell=FIRST, devices=[0, 0])
    prefix = "is3d_amd error %d: " % api.IS3D_EDOMAIN
    assert str(own.value).startswith(prefix)
    assert e.value.code == api.IS3D_EDOMAIN and str(e.value) == prefix + "shard 1 (device 0): " + str(own.value)[len(prefix):]
    if entry != "list":
        rc, text, hist, n = raw_binned_multi("is3d_sample_%s_multi" % entry, fam["raw"], bad, [0, 0], FIRST)
        assert rc == api.IS3D_EDOMAIN and prefix + text == str(e.value) and n == 0
        assert all(not hist[k].any() for k in ARRAYS)


# ---- 5. anisotropic-hydro bad cells in two different shards ----
@pytest.mark.parametrize("entry", ["list", "binned"])
def test_vah_bad_cells_in_two_shards(fam, entry):
    """Three shards, [0, 2) [2, 4) [4, 5).  Lambda = NaN at cell a of shard 0 and alpha_L beyond the last table node at cell b of a later
    shard, both cells that emit: IS3D_EDOMAIN names the lower one, and what comes back is the good run without the two cells' hadrons."""
    f = fam["vah"]
    good, _ = f.run("list", first_cell=FIRST)
    assert [api.shard_bounds(N_CELLS, r, 3) for r in range(3)] == [(0, 2), (2, 4), (4, 5)]
    per = np.bincount(good["cell"] - FIRST, minlength=N_CELLS)
    a, b = int(np.argmax(per[:2])), 2 + int(np.argmax(per[2:]))
    keep = ~np.isin(good["cell"], [FIRST + a, FIRST + b])
    assert per[a] > 0 and per[b] > 0 and keep.sum() >= MIN_HADRONS // N_CELLS
    bad = {k: x.copy() for k, x in f.cells.items()}
    bad["Lambda"][a] = np.nan
    bad["aL"][b] = 2.5
    with pytest.raises(api.Is3dError) as e:
        f.run(entry, bad, first_cell=FIRST, devices=[0, 0, 0])
    assert e.value.code == api.IS3D_EDOMAIN and e.value.bad_cell == FIRST + a, str(e.value)
    assert str(e.value).startswith("is3d_amd error %d: shard 0 (device 0): " % api.IS3D_EDOMAIN)
    assert e.value.stats["n_particles"] == keep.sum()
    if entry == "list":
        assert same_list(e.value.particles, good[keep])
    else:
        with pytest.raises(api.Is3dError) as one:                  # the single-device entry on the same surface: every array, bit for bit
            f.run(entry, bad, first_cell=FIRST)
        assert one.value.bad_cell == FIRST + a and same_hist(e.value.hist, one.value.hist)
        assert same_counters(e.value.stats, one.value.stats)
        want = api.sampler_bin_list(BINS, N_EVENTS, len(PIKP), good[keep])               # the integer counts of the list without the two cells
        assert all(np.array_equal(e.value.hist[k], want[k]) for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield"))


# ---- 6. a list buffer that is too small, through the multi entry ----
def test_vah_list_with_a_capacity_too_small(fam):
    f = fam["vah"]
    n = len(f.single["list"][0])
    assert n >= MIN_HADRONS
    with pytest.raises(api.Is3dError) as e:
        f.run("list", devices=[0, 0], capacity=10)
    assert e.value.code == api.IS3D_ENOMEM
    assert "%d particles, capacity 10" % n in str(e.value)          # the text carries the full count ...
    L = api.load()                                                  # ... and so does *n_particles
    sp, gla = inputs.species(PIKP), inputs.feqmod_tables(0.15)
    cs, sps, tp, si, os_, _held = api._pack_sampler_vah(f.cells, sp, gla, dict(dimension=3), f.kw["tab"], N_EVENTS, f.kw["seed"], 0.5, 0, 0, 0, None)
    buf = np.zeros(10, dtype=api.PARTICLE_DTYPE)
    dv, cnt, st = (C.c_int32 * 2)(0, 0), C.c_int64(-1), api.SamplerStats()
    rc = L.is3d_sample_particles_vah_multi(C.byref(cs), C.byref(sps), tp, C.byref(si), C.byref(os_), dv, C.c_int32(2), C.c_void_p(buf.ctypes.data),
                                           C.c_int64(10), C.byref(cnt), C.byref(st))
    assert rc == api.IS3D_ENOMEM and cnt.value == n
    assert same_list(buf, f.single["list"][0][:10])
