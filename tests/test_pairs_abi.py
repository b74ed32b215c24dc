"""CPU: the pair-correlation entries of include/is3d_amd.h exist, mirror the header's structs, and make every refusal without a device; a good
device call without a device is IS3D_ENODEVICE (no CPU path behind a device entry).  The writer, and the run driver's key with its texts."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import decays_mc_cases as cases
import pairs_cases as P
import test_flow_abi as flow_abi
import test_run_refusals as base
from conftest import ROOT
from is3d_amd import api, inputs, synth

PAIR_SYMBOLS = ("is3d_pairs_list", "is3d_pairs_list_device", "is3d_pairs_correlation", "is3d_write_pairs", "is3d_decay_particles_pairs",
                "is3d_sampler_plan_execute_pairs", "is3d_sample_pairs")
PYTHON_NAMES = ("PairBins", "PairHist", "pairs_list", "pairs_list_device", "decay_particles_pairs", "sample_pairs", "pairs_correlation", "write_pairs")


def test_symbols_are_exported_and_declared():
    lib = api.load()
    header = open(os.path.join(ROOT, "include", "is3d_amd.h")).read()
    for s in PAIR_SYMBOLS:
        assert hasattr(lib, s) and s in api.EXPORTS and "int %s(" % s in header, s
    assert all(hasattr(api, n) for n in PYTHON_NAMES) and hasattr(api.SamplerPlan, "execute_pairs")


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "is3d_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(is3d_pair_bins), offsetof(is3d_pair_bins, pT_max), offsetof(is3d_pair_bins, n_y), offsetof(is3d_pair_bins, n_phi),'
                   'sizeof(is3d_pair_hist), offsetof(is3d_pair_hist, M), sizeof(is3d_pair_result), offsetof(is3d_pair_result, V));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert c == [ctypes.sizeof(api.PairBins), api.PairBins.pT_max.offset, api.PairBins.n_y.offset, api.PairBins.n_phi.offset,
                 ctypes.sizeof(api.PairHist), api.PairHist.M.offset, ctypes.sizeof(api.PairResult), api.PairResult.V.offset]


NAN = float("nan")
BAD_BINS = (dict(y_cut=0.0), dict(y_cut=-1.0), dict(y_cut=NAN), dict(pT_min=-0.1), dict(pT_max=0.2), dict(pT_max=0.1), dict(pT_max=NAN), dict(pT_min=NAN),
            dict(n_y=0), dict(n_y=65), dict(n_y=-3), dict(n_phi=0), dict(n_phi=2), dict(n_phi=6), dict(n_phi=30), dict(n_phi=68), dict(n_phi=-4),
            dict(y_cut=400.0),                    # exp(800) is not finite
            dict(y_cut=1e-300, n_y=64))           # the edges do not increase: every one rounds to 1


def some_list():
    p = np.zeros(3, dtype=api.PARTICLE_DTYPE)
    p["E"], p["px"] = 1.0, 0.5
    return p


@pytest.mark.parametrize("entry", ("pairs_list", "pairs_list_device"))
def test_refusals_come_before_any_device_use(entry):
    p = some_list()
    call = getattr(api, entry)
    before = api.resource_counters()
    rows = [(dict(P.BINS, **bad), 2, 2, [0, 1]) for bad in BAD_BINS]
    rows += [(P.BINS, 0, 2, [0, 1]), (P.BINS, -1, 2, [0, 1]), (P.BINS, 2, 0, [0, 1]), (P.BINS, 2, 2, [0, 2]), (P.BINS, 2, 2, [-2, 1])]
    for bins, ne, ns, slot in rows:
        with pytest.raises(api.Is3dError) as e:
            call(bins, ne, ns, slot, p)
        assert e.value.code == api.IS3D_EINVAL, (bins, ne, ns, slot)
    assert api.resource_counters() == before
    for bad in (dict(species=5), dict(species=-1), dict(event=2), dict(event=-1)):         # the host entry refuses a particle out of range
        q = some_list()
        for k, v in bad.items():
            q[k][1] = v
        with pytest.raises(api.Is3dError) as e:
            api.pairs_list(P.BINS, 2, 2, [0, 1], q)
        assert e.value.code == api.IS3D_EINVAL and "particle 1" in str(e.value)


def test_null_arguments_are_refused():
    L = api.load()
    p = some_list()
    slot = np.zeros(1, dtype=np.int32)
    b = api._pack_pair_bins(P.BINS)
    h, _keep = api._pair_arrays(b, 2, 1)
    skipped = ctypes.c_int64(0)
    bp, hp = ctypes.POINTER(api.PairBins), ctypes.POINTER(api.PairHist)
    L.is3d_pairs_list.argtypes = [bp, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, hp]
    L.is3d_pairs_list_device.argtypes = L.is3d_pairs_list.argtypes + [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    good = [ctypes.byref(b), 2, 1, slot.ctypes.data, 1, 3, p.ctypes.data, ctypes.byref(h)]
    before = api.resource_counters()
    for k, bad in ((0, None), (3, None), (6, None), (7, None), (7, ctypes.byref(api.PairHist(h.same, None, h.M))),
                   (7, ctypes.byref(api.PairHist(None, h.mixed, h.M))), (7, ctypes.byref(api.PairHist(h.same, h.mixed, None))), (5, -1), (4, 0)):
        a = list(good)
        a[k] = bad
        assert L.is3d_pairs_list(*a) == api.IS3D_EINVAL, k
        assert L.is3d_pairs_list_device(*a, ctypes.byref(skipped), 0) == api.IS3D_EINVAL, k
    assert L.is3d_pairs_list_device(*good, None, 0) == api.IS3D_EINVAL
    V = ctypes.c_void_p
    L.is3d_pairs_correlation.argtypes = [bp, hp, ctypes.c_int32, ctypes.c_int32, V, V, V]
    res = (api.PairResult * 1)()
    assert L.is3d_pairs_correlation(ctypes.byref(b), ctypes.byref(h), 1, 0, None, None, res) == api.IS3D_OK      # C and C_phi are optional
    for a in ((None, ctypes.byref(h), 1, 0, None, None, res), (ctypes.byref(b), None, 1, 0, None, None, res), (ctypes.byref(b), ctypes.byref(h), 1, 0, None, None, None),
              (ctypes.byref(b), ctypes.byref(h), 0, 0, None, None, res), (ctypes.byref(b), ctypes.byref(h), 1, -1, None, None, res),
              (ctypes.byref(b), ctypes.byref(h), 1, 32, None, None, res), (ctypes.byref(api._pack_pair_bins(dict(P.BINS, n_phi=6))), ctypes.byref(h), 1, 0, None, None, res)):
        assert L.is3d_pairs_correlation(*a) == api.IS3D_EINVAL
    assert api.resource_counters() == before


def test_no_cpu_path_behind_the_device_entry():
    """Without a device a good call is IS3D_ENODEVICE; with one it is the host route's histograms (tests/test_gpu_pairs.py holds it to more)."""
    if api.load().is3d_device_count() == 0:
        with pytest.raises(api.Is3dError) as e:
            api.pairs_list_device(P.BINS, 2, 1, [0], some_list())
        assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
    else:
        got, skipped = api.pairs_list_device(P.BINS, 2, 1, [0], some_list())
        assert skipped == 0 and P.same_hist(got, api.pairs_list(P.BINS, 2, 1, [0], some_list()))


# ---- the decay entry and the one-shot sampler entry: every refusal without a device ----
RHO = cases.hand_table([cases.stable(211, 0.13957), cases.stable(-211, 0.13957), (113, 0.77526, 0.1491, 0, [(2, 1.0, [211, -211])])])


def test_decay_particles_pairs_refuses_before_any_device_use():
    import decays_mc_ref as ref
    q = ref.make_particles(api, RHO, RHO["mc_id"], [2, 0, 2], np.zeros((3, 3)), events=[0, 1, 1])
    slot = np.array([0, 0, -1], np.int32)
    before = api.resource_counters()
    bad_event = q.copy()
    bad_event["event"][1] = 2
    bad_species = q.copy()
    bad_species["species"][0] = 3
    lost = dict(RHO, mc_id=np.array([211, -2, 113], np.int64))          # the rho's second product is not in the table
    for kw in (dict(bins=dict(P.BINS, y_cut=0.0)), dict(bins=dict(P.BINS, pT_max=0.1)), dict(bins=dict(P.BINS, n_phi=10)), dict(n_slots=0),
               dict(slot=np.array([0, 1, -1], np.int32)), dict(slot=np.array([0, -2, -1], np.int32)), dict(n_events=0), dict(n_events=-3), dict(q=bad_event),
               dict(q=bad_species), dict(table=lost)):
        a = dict(q=q, slot=slot, n_slots=1, bins=P.BINS, n_events=2, table=RHO)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_pairs(a["table"], RHO["mc_id"], a["q"], a["slot"], a["n_slots"], a["bins"], a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    # NULLs through the bare entry: table, chosen list, inputs, particles, slot map, bins, hist, n_final, n_unbinned
    L = api.load()
    ts, ch, _, keep = api._decay_pack(RHO, RHO["mc_id"], dict(pT=[1.0], phi=[0.0], y=[0.0]))
    inp = api.DecayMcInputs(1, 0, 0, -1)
    b = api._pack_pair_bins(P.BINS)
    h, _keep = api._pair_arrays(b, 2, 1)
    st, nf, nu = api.DecayMcStats(), ctypes.c_int64(0), ctypes.c_int64(0)
    V = ctypes.c_void_p
    L.is3d_decay_particles_pairs.argtypes = [V, ctypes.c_int32, V, V, ctypes.c_int64, V, V, ctypes.c_int32, V, ctypes.c_int32, V, V, V, V]
    addr = lambda x: ctypes.cast(ctypes.byref(x), V)  # noqa: E731
    good = [addr(ts), 3, V(ch.ctypes.data), addr(inp), 3, V(q.ctypes.data), V(slot.ctypes.data), 1, addr(b), 2, addr(h), addr(nf), addr(nu), addr(st)]
    for k in (0, 2, 3, 5, 6, 8, 10, 11, 12):
        a = list(good)
        a[k] = None
        assert L.is3d_decay_particles_pairs(*a) == api.IS3D_EINVAL, k
    assert api.resource_counters() == before
    if L.is3d_device_count() == 0:
        assert L.is3d_decay_particles_pairs(*good) == api.IS3D_ENODEVICE
    # an empty list: zero histograms, no launch, no device needed
    hist, st0 = api.decay_particles_pairs(RHO, RHO["mc_id"], q[:0], slot, 1, P.BINS, 2)
    assert st0["n_final"] == st0["n_unbinned"] == 0 and all(not v.any() for v in hist.values()) and api.resource_counters() == before


def test_sample_pairs_refuses_before_any_device_use():
    cells = synth.synth_surface(3, 3, seed=1)
    sp, gla, df, o = inputs.species([211, 113]), inputs.feqmod_tables(0.15), inputs.df_tables(), dict(dimension=3, df_mode=2)
    slot_d = np.array([0, 0, -1], np.int32)
    before = api.resource_counters()
    lost = dict(RHO, mc_id=np.array([211, -211, 114], np.int64))          # the chosen rho0 is not in this table
    for kw in (dict(bins=dict(P.BINS, y_cut=-2.0)), dict(bins=dict(P.BINS, n_y=65)), dict(slot=[0, 1]), dict(n_slots=0), dict(n_events=0),
               dict(slot_decayed=np.array([0, 1, -1], np.int32)), dict(n_slots_decayed=0), dict(table=lost)):
        a = dict(bins=P.BINS, slot=[0, 0], n_slots=1, n_events=2, table=RHO, slot_decayed=slot_d, n_slots_decayed=1)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.sample_pairs(cells, sp, df, gla, a["bins"], a["slot"], a["n_slots"], o, table=a["table"], chosen_mc_id=sp["mc_id"],
                             slot_decayed=a["slot_decayed"], n_slots_decayed=a["n_slots_decayed"], n_events=a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    with pytest.raises(api.Is3dError) as e:                               # without a table too
        api.sample_pairs(cells, sp, df, gla, dict(P.BINS, pT_min=-1.0), [0, 0], 1, o, n_events=2)
    assert e.value.code == api.IS3D_EINVAL
    assert api.resource_counters() == before
    if api.load().is3d_device_count() == 0:
        for table in (None, RHO):
            with pytest.raises(api.Is3dError) as e:
                api.sample_pairs(cells, sp, df, gla, P.BINS, [0, 0], 1, o, table=table, chosen_mc_id=sp["mc_id"], slot_decayed=slot_d, n_slots_decayed=1,
                                 n_events=2)
            assert e.value.code == api.IS3D_ENODEVICE


# ---- the writer ----
def test_write_pairs_prints_every_class(tmp_path):
    p, n_events = P.hand_list()
    bins = P.bins_of((3, 8))
    hist = api.pairs_list(bins, n_events, 2, P.slot_map(2), p)
    with pytest.raises(api.Is3dError) as e:                               # <dir>/pairs/ must exist
        api.write_pairs(str(tmp_path), bins, hist, ["211", "other"])
    assert e.value.code == api.IS3D_EIO
    os.makedirs(tmp_path / "pairs")
    for labels in (["211", ""], ["a/b", "x"]):
        with pytest.raises(api.Is3dError) as e:
            api.write_pairs(str(tmp_path), bins, hist, labels)
        assert e.value.code == api.IS3D_EINVAL
    with pytest.raises(api.Is3dError) as e:
        api.write_pairs(str(tmp_path), dict(bins, y_cut=0.0), hist, ["211", "other"])
    assert e.value.code == api.IS3D_EINVAL and os.listdir(tmp_path / "pairs") == []
    api.write_pairs(str(tmp_path), bins, hist, ["211", "other"])
    assert sorted(os.listdir(tmp_path / "pairs")) == ["correlation_211_211.dat", "correlation_211_other.dat", "correlation_other_other.dat"]
    c = api.pairs_correlation(bins, hist)
    for (a, b), name in (((0, 0), "211_211"), ((0, 1), "211_other"), ((1, 1), "other_other")):
        k = api.pair_class(a, b, 2)
        path = tmp_path / "pairs" / ("correlation_%s.dat" % name)
        rows = np.loadtxt(path)
        assert rows.shape == (5 * 8, 5)
        dy, dphi = np.meshgrid((np.arange(5) - 2) * (2.0 * bins["y_cut"] / 3), np.arange(8) * (2.0 * np.pi / 8), indexing="ij")
        assert np.allclose(rows[:, 0], dy.ravel(), rtol=1e-8, atol=0) and np.allclose(rows[:, 1], dphi.ravel(), rtol=1e-8, atol=0)
        assert np.array_equal(rows[:, 2].astype(np.int64), hist["same"][k].ravel()) and np.array_equal(rows[:, 3].astype(np.int64), hist["mixed"][k].ravel())
        assert np.allclose(rows[:, 4], c["C"][k].ravel(), rtol=1e-8, atol=0)          # nine significant digits are printed
        head = open(path).read().split("\n")[:2]
        assert head[0].startswith("# delta_y\tdelta_phi\tsame\tmixed\tC") and "n_y = 3, n_phi = 8" in head[0]
        assert head[1] == "# n_same: %d, n_mixed: %d" % (c["n_same"][k], c["n_mixed"][k]) and c["n_same"][k] > 0


# ---- the run driver's key: every refusal with its exact text (tests/golden/run_refusals_pairs.json; `python tests/test_pairs_abi.py` records
# them from the build in the tree), nothing written, and the pinned texts of the older keys unchanged beside the new one ----
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_refusals_pairs.json")
KEY = "test_sampler_pairs = 1"
ON = dict(operation=2, test_sampler=1)
DEV = "test_sampler_on_device = 1"
# id -> (parameters of refformat.make_run_dir, lines appended to iS3D_parameters.dat, keys removed, directories made under results/)
ROWS = {
    "pairs-operation": (dict(operation=1, test_sampler=1), [KEY], [], ["pairs"]),
    "pairs-test_sampler-0": (dict(operation=2), [KEY], [], ["pairs"]),
    "pairs-mode-2": (dict(base.VAH2, test_sampler=1), ["vah_sampler = 1", KEY], [], ["pairs"]),
    "pairs-on-device-0": (dict(ON), [KEY], [], ["pairs"]),
    "pairs-fused": (dict(ON), [DEV, "test_sampler_fused = 1", KEY], [], ["pairs"]),
    "pairs-bad-y_cut": (dict(ON), [DEV, KEY, "pairs_y_cut = 0"], [], ["pairs"]),
    "pairs-bad-pT": (dict(ON), [DEV, KEY, "pairs_pT_min = 1.5", "pairs_pT_max = 1.5"], [], ["pairs"]),
    "pairs-bad-y_bins": (dict(ON), [DEV, KEY, "pairs_y_bins = 65"], [], ["pairs"]),
    "pairs-bad-y_bins-fraction": (dict(ON), [DEV, KEY, "pairs_y_bins = 2.5"], [], ["pairs"]),
    "pairs-bad-phi_bins": (dict(ON), [DEV, KEY, "pairs_phi_bins = 30"], [], ["pairs"]),
    "pairs-edges-not-finite": (dict(ON), [DEV, KEY, "pairs_y_cut = 400"], [], ["pairs"]),
    "pairs-missing-directory": (dict(ON), [DEV, KEY], [], []),
    "pairs-missing-decayed-directory": (dict(ON), [DEV, "test_sampler_decayed = 1", KEY], [], ["pairs"]),
    "pairs-missing-sampler-key": (dict(operation=2), [KEY], ["test_sampler"], ["pairs"]),
    # two things wrong: the earlier check speaks
    "order-pairs-operation-before-on-device": (dict(operation=0, test_sampler=1), [KEY], [], []),
    "order-pairs-bins-before-directory": (dict(ON), [DEV, KEY, "pairs_y_cut = -1"], [], []),
    "order-decayed-before-pairs": (dict(ON), ["test_sampler_decayed = 1", KEY], [], []),
    "order-flow-before-pairs": (dict(ON), [DEV, "test_sampler_flow = 1", KEY, "flow_y_cut = 0", "pairs_y_cut = 0"], [], ["flow", "pairs"]),
}
refused_run = flow_abi.refused_run


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_the_rows_of_this_module(golden):
    assert sorted(golden["stderr"]) == sorted(ROWS)
    own = {row: text for row, text in golden["stderr"].items() if row not in ("pairs-missing-sampler-key", "order-decayed-before-pairs", "order-flow-before-pairs")}
    for row, text in own.items():
        assert "test_sampler_pairs = 1" in text and text.rstrip().endswith("set test_sampler_pairs = 0"), row
    assert "results/pairs" in golden["stderr"]["pairs-missing-directory"] and "results/decayed/pairs" in golden["stderr"]["pairs-missing-decayed-directory"]
    assert "test_sampler_decayed = 1" in golden["stderr"]["order-decayed-before-pairs"] and "test_sampler_flow = 1" in golden["stderr"]["order-flow-before-pairs"]
    # the situations that refuse test_sampler_flow refuse this key too, in the same words but for what each key makes
    with open(flow_abi.GOLDEN) as f:
        flow = json.load(f)["stderr"]
    for k in ("missing-directory", "missing-decayed-directory", "missing-sampler-key"):
        assert golden["stderr"]["pairs-" + k] == flow["flow-" + k].replace("flow", "pairs")
    for k in ("operation", "test_sampler-0", "mode-2", "on-device-0", "fused"):
        assert golden["stderr"]["pairs-" + k].split(":")[1] == flow["flow-" + k].split(":")[1].replace("flow", "pairs"), k


@pytest.mark.parametrize("row", list(ROWS))
def test_driver_refuses_the_key_with_its_exact_text(tmp_path, golden, row):
    root, r = refused_run(tmp_path, ROWS, row)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr == golden["stderr"][row]
    assert [f for _, _, fs in os.walk(os.path.join(root, "results")) for f in fs] == []


@pytest.mark.parametrize("rows, pinned_path", ((base.ROWS, base.GOLDEN), (flow_abi.ROWS, flow_abi.GOLDEN)), ids=("base", "flow"))
def test_existing_refusals_keep_their_texts_beside_the_new_key(tmp_path, rows, pinned_path):
    with open(pinned_path) as f:
        pinned = json.load(f)["stderr"]
    for row in rows:
        root, r = refused_run(tmp_path / row, rows, row, extra=[KEY])
        assert r.returncode == 1 and r.stderr == pinned[row], (row, r.stderr)
        assert [f for _, _, fs in os.walk(os.path.join(root, "results")) for f in fs] == []


def record():
    """writes GOLDEN from the build in the tree"""
    import pathlib
    import tempfile
    out = {}
    for row in ROWS:
        with tempfile.TemporaryDirectory() as d:
            _, r = refused_run(pathlib.Path(d), ROWS, row)
            assert r.returncode == 1 and r.stderr.startswith("iS3D-amd: ") and r.stdout.count("\n") == 1, (row, r.returncode, r.stdout, r.stderr)
            out[row] = r.stderr
    with open(GOLDEN, "w") as f:
        json.dump(dict(stderr=out), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record()
