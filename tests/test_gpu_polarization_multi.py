"""GPU: is3d_spin_polarization_multi -- mode 5 with the per-chunk kernel and the chunk sums on cell-axis shards (one per entry of the device
list), the shards' class sums added in shard order on devices[0].  Repeated ordinals of device 0 make every shard count run on one GPU.

Contract under test (include/is3d_amd.h): one shard is is3d_spin_polarization bit for bit; N shards are bitwise scale x ((V_0 + V_1) + V_2 ...)
over the shards that have cells, hence reproducible; against the single device only the association of the additions differs (1e-10 of each
component's largest value, the subsystem's own rule, against the numpy restatement and against the single device).

Shapes: 3+1D 5 pT (8 lanes per class) x 5 phi (4-phi tile) x 4 y (3-y tile), 2+1D 5 pT x 5 phi (8-phi tile) x 9 uniform eta nodes; 61 / 23
cells (unequal shards of one chunk), 1100 cells (several chunks inside a shard, another chunk partition than the single device's), 3 cells
(empty shards at 7), 0 cells (every shard empty)."""
from functools import lru_cache

import numpy as np
import pytest

from is3d_amd import api, inputs, synth
from test_gpu_polarization import assert_close, mixed_cells, pick_species, restate

pytestmark = pytest.mark.gpu

OUTS = api.POLARIZATION_OUTPUTS
SHARDS = [1, 2, 3, 7]
T = 0.1503
# masses whose -1 / (4 m) is a power of two: the scale commutes with the sum over the shards bit for bit
POW2 = dict(mass=np.array([0.25, 0.5, 1.0]), sign=np.array([-1.0, 1.0, 0.0]), degeneracy=np.array([1.0, 2.0, 1.0]),
            baryon=np.array([0.0, 1.0, 0.0]))

# name -> (dim, n_cells)
CASES = {"3d-61": (3, 61), "3d-1100": (3, 1100), "3d-3": (3, 3), "2d-23": (2, 23), "2d-1100": (2, 1100), "2d-3": (2, 3)}


def grid_of(dim):
    g = inputs.grid()
    if dim == 3:
        return dict(pT=g["pT"][[1, 6, 11, 16, 21]], phi=g["phi"][[0, 5, 10, 15, 20]], y=g["y"][[2, 8, 12, 18]], eta=g["eta"], eta_w=g["eta_w"])
    return dict(pT=g["pT"][[1, 6, 11, 16, 21]], phi=g["phi"][[0, 5, 10, 15, 20]], y=g["y"], eta=g["eta"][::30], eta_w=g["eta_w"][::30])


@lru_cache(maxsize=None)
def inputs_of(name, pow2=False):
    dim, n = CASES[name]
    grid = grid_of(dim)
    assert len(grid["pT"]) == 5 and len(grid["phi"]) == 5 and (len(grid["y"]) == 4 if dim == 3 else len(grid["eta"]) == 9)
    seed = 8100 + sorted(CASES).index(name)
    cells = mixed_cells(n, dim, seed=seed)
    w = synth.synth_vorticity(n, seed=seed + 50)
    for a in list(cells.values()) + list(w.values()):
        a.setflags(write=False)
    return dict(dim=dim, n=n, cells=cells, w=w, sp=POW2 if pow2 else pick_species(2, (1, -1)), grid=grid, opts=dict(dimension=dim))


def one_shot_of(b, lo=0, hi=None):
    hi = b["n"] if hi is None else hi
    cells = {k: np.ascontiguousarray(v[lo:hi]) for k, v in b["cells"].items()}
    w = {k: np.ascontiguousarray(v[lo:hi]) for k, v in b["w"].items()}
    return api.spin_polarization(cells, w, b["sp"], b["grid"], T, b["opts"])


def multi_of(b, devices):
    return api.spin_polarization_multi(b["cells"], b["w"], b["sp"], b["grid"], T, b["opts"], devices)


def frozen(res):
    for k in OUTS:
        res[k].setflags(write=False)
    return res


@lru_cache(maxsize=None)
def single(name, pow2=False):
    """the single-device result of a case, computed once and never written to"""
    return frozen(one_shot_of(inputs_of(name, pow2)))


@lru_cache(maxsize=None)
def multi(name, shards, pow2=False):
    return frozen(multi_of(inputs_of(name, pow2), [0] * shards))


@lru_cache(maxsize=None)
def restated(name):
    b = inputs_of(name)
    return frozen(restate(b["cells"], b["w"], b["sp"], b["grid"], T, b["dim"]))


def bounds(n, shards):
    return [api.shard_bounds(n, r, shards) for r in range(shards)]


def worst_error(got, ref):
    return {k: float(np.max(np.abs(got[k] - ref[k])) / np.max(np.abs(ref[k]))) for k in OUTS}


# ---- 1. one shard is the one-shot ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_shard_is_the_one_shot(name):
    got, want = multi(name, 1), single(name)
    for k in OUTS:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["stats"]["n_chunks"] == want["stats"]["n_chunks"] and len(got["shard_stats"]) == 1


# ---- 2. several shards: bitwise the left-to-right sum of the one-shots on the shards' own slices ----
def model_of(b, shards):
    """left-to-right numpy sum, over the shards that have cells in shard order, of the one-shot on each shard's slice of cells and vorticity"""
    acc = None
    used = []
    for lo, hi in bounds(b["n"], shards):
        if hi <= lo:
            continue
        part = one_shot_of(b, lo, hi)
        used.append((lo, hi))
        acc = {k: part[k].copy() for k in OUTS} if acc is None else {k: acc[k] + part[k] for k in OUTS}
    return acc, used


def assert_slices_differ(b, used):
    """a shard that read the vorticity (or the cells) from offset 0 would see other numbers than its own"""
    for lo, hi in used[1:]:
        m = hi - lo
        for f in synth.VORTICITY_FIELDS:
            assert not np.array_equal(b["w"][f][lo:hi], b["w"][f][:m]), f
        assert not np.array_equal(b["cells"]["ux"][lo:hi], b["cells"]["ux"][:m])


@pytest.mark.parametrize("shards", SHARDS[1:])
@pytest.mark.parametrize("name", sorted(CASES))
def test_snorm_is_the_shard_ordered_sum_any_masses(name, shards):
    b = inputs_of(name)
    model, used = model_of(b, shards)
    assert len(used) == min(shards, b["n"])
    assert_slices_differ(b, used)
    got = multi(name, shards)
    assert got["Snorm"].tobytes() == model["Snorm"].tobytes()


@pytest.mark.parametrize("shards", SHARDS[1:])
@pytest.mark.parametrize("name", sorted(CASES))
def test_all_five_are_the_shard_ordered_sum_power_of_two_scale(name, shards):
    b = inputs_of(name, True)
    assert all(np.frexp(-1.0 / (4.0 * m))[0] == -0.5 for m in b["sp"]["mass"])
    model, used = model_of(b, shards)
    assert_slices_differ(b, used)
    got = multi(name, shards, True)
    for k in OUTS:
        assert np.all(np.isfinite(got[k])) and np.any(got[k] != 0.0), k
        assert got[k].tobytes() == model[k].tobytes(), k


def test_vorticity_offset_matters():
    """the model above separates a shard that reads its own vorticity slice from one that reads the first: the two sums differ"""
    b = inputs_of("3d-61", True)
    (lo0, hi0), (lo1, hi1) = bounds(b["n"], 2)
    cells1 = {k: np.ascontiguousarray(v[lo1:hi1]) for k, v in b["cells"].items()}
    wrong = api.spin_polarization(cells1, {k: np.ascontiguousarray(v[:hi1 - lo1]) for k, v in b["w"].items()}, b["sp"], b["grid"], T, b["opts"])
    right = one_shot_of(b, lo1, hi1)
    assert wrong["Snorm"].tobytes() == right["Snorm"].tobytes()   # the norm does not read the vorticity
    for k in OUTS[:4]:
        assert wrong[k].tobytes() != right[k].tobytes(), k


def test_every_shard_empty_gives_zeros():
    b = inputs_of("3d-3")
    empty = dict(b, n=0, cells={k: v[:0] for k, v in b["cells"].items()}, w={k: v[:0] for k, v in b["w"].items()})
    for devices in ([0], [0, 0, 0]):
        got = multi_of(empty, devices)
        for k in OUTS:
            assert got[k].shape == single("3d-3")[k].shape and np.all(got[k] == 0.0), (k, devices)
        assert got["stats"]["code"] == 0 and got["stats"]["n_chunks"] == 0 and len(got["shard_stats"]) == len(devices)


# ---- 3. reproducible ----
@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("name", ["3d-1100", "2d-1100", "3d-3"])
def test_two_calls_give_the_same_bits(name, shards):
    b = inputs_of(name)
    lists = [[0] * shards]
    visible = api.load().is3d_device_count()
    if visible >= 2:   # whatever the device list: the same shard count over distinct devices
        lists.append([i % visible for i in range(shards)])
    print("device lists run:", lists, "(%d device%s visible)" % (visible, "" if visible == 1 else "s"))
    want = multi(name, shards)
    for devices in lists:
        got = multi_of(b, devices)
        for k in OUTS:
            assert got[k].tobytes() == want[k].tobytes(), (k, devices)


# ---- 4. parity: the subsystem's own rule, 1e-10 of each component's largest value ----
@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_restatement_and_single_device(name, shards):
    got, ref, one = multi(name, shards), restated(name), single(name)
    print("parity %s shards=%d: vs restatement %s; vs single device %s" % (name, shards, worst_error(got, ref), worst_error(got, one)))
    assert_close(got, ref)
    assert_close(got, one)


# ---- 5. stats ----
@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_stats(name, shards):
    b, got = inputs_of(name), multi(name, shards)
    st, sst = got["stats"], got["shard_stats"]
    assert st["code"] == 0 and len(sst) == shards
    assert all(s["code"] == 0 for s in sst)
    assert st["n_chunks"] == sum(s["n_chunks"] for s in sst)
    assert st["ms_cells"] == max(s["ms_cells"] for s in sst) and st["ms_cells"] > 0
    assert st["n_classes"] == single(name)["stats"]["n_classes"] == len(set(zip(b["sp"]["mass"], b["sp"]["sign"])))
    for (lo, hi), s in zip(bounds(b["n"], shards), sst):
        assert (s["n_chunks"] >= 1) == (hi > lo)
    if name.endswith("1100") and shards == 2:
        assert all(s["n_chunks"] > 1 for s in sst)   # several chunks inside a shard
    if name.endswith("1100") and shards == 3:
        assert st["n_chunks"] != single(name)["stats"]["n_chunks"]   # another chunk partition than the single device's
