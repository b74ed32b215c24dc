"""CPU: the HBT entries of include/is3d_amd.h exist, mirror the header's structs, and make every refusal without a device; a good device
call without a device is IS3D_ENODEVICE (no CPU path behind a device entry).  The run driver's key test_sampler_hbt with its texts."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hbt_cases as H
import test_flow_abi as flow_abi
import test_pairs_abi as pairs_abi
import test_run_refusals as base
from conftest import ROOT
from is3d_amd import api, inputs, synth

HBT_SYMBOLS = ("is3d_hbt_list", "is3d_hbt_list_device", "is3d_hbt_radii", "is3d_write_hbt", "is3d_decay_particles_hbt",
               "is3d_sampler_plan_execute_hbt", "is3d_sample_hbt")
PYTHON_NAMES = ("HbtBins", "HbtHist", "HbtRadii", "hbt_list", "hbt_list_device", "decay_particles_hbt", "sample_hbt", "hbt_radii", "write_hbt")


def test_symbols_are_exported_and_declared():
    lib = api.load()
    header = open(os.path.join(ROOT, "include", "is3d_amd.h")).read()
    for s in HBT_SYMBOLS:
        assert hasattr(lib, s) and s in api.EXPORTS and "int %s(" % s in header, s
    assert all(hasattr(api, n) for n in PYTHON_NAMES) and hasattr(api.SamplerPlan, "execute_hbt")


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "is3d_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(is3d_hbt_bins), offsetof(is3d_hbt_bins, n_kT), offsetof(is3d_hbt_bins, q_max), offsetof(is3d_hbt_bins, n_q),'
                   'offsetof(is3d_hbt_bins, kernel_form), sizeof(is3d_hbt_hist), offsetof(is3d_hbt_hist, M), sizeof(is3d_hbt_radii_result),'
                   'offsetof(is3d_hbt_radii_result, R2), offsetof(is3d_hbt_radii_result, singular));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert c == [ctypes.sizeof(api.HbtBins), api.HbtBins.n_kT.offset, api.HbtBins.q_max.offset, api.HbtBins.n_q.offset, api.HbtBins.kernel_form.offset,
                 ctypes.sizeof(api.HbtHist), api.HbtHist.M.offset, ctypes.sizeof(api.HbtRadii), api.HbtRadii.R2.offset, api.HbtRadii.singular.offset]


NAN = float("nan")
BAD_BINS = (dict(y_cut=0.0), dict(y_cut=-1.0), dict(y_cut=NAN), dict(pT_min=-0.1), dict(pT_max=0.05), dict(pT_max=0.01), dict(pT_max=NAN), dict(pT_min=NAN),
            dict(kT_min=-0.1), dict(kT_max=0.1), dict(kT_max=NAN), dict(kT_min=NAN), dict(n_kT=0), dict(n_kT=17), dict(n_kT=-2),
            dict(q_max=0.0), dict(q_max=-0.1), dict(q_max=NAN), dict(q_max=float("inf")), dict(n_q=1), dict(n_q=0), dict(n_q=65), dict(n_q=-8),
            dict(y_cut=400.0),                    # exp(800) is not finite
            dict(kT_max=float("inf")))            # dkT is not finite
DEVICE_ONLY = (dict(kernel_form=3), dict(kernel_form=-1), dict(kernel_form=2, n_q=15))     # 3 x 3375 bins do not fit the LDS


def some_list():
    p = np.zeros(3, dtype=api.PARTICLE_DTYPE)
    p["E"], p["px"] = 1.0, 0.5
    return p


@pytest.mark.parametrize("entry", ("hbt_list", "hbt_list_device"))
def test_refusals_come_before_any_device_use(entry):
    p = some_list()
    call = getattr(api, entry)
    before = api.resource_counters()
    rows = [(dict(H.BINS, **bad), 2, 2, [0, 1]) for bad in BAD_BINS + (DEVICE_ONLY if entry == "hbt_list_device" else ())]
    rows += [(H.BINS, 0, 2, [0, 1]), (H.BINS, -1, 2, [0, 1]), (H.BINS, 2, 0, [0, 1]), (H.BINS, 2, 2, [0, 2]), (H.BINS, 2, 2, [-2, 1])]
    for bins, ne, ns, slot in rows:
        with pytest.raises(api.Is3dError) as e:
            call(bins, ne, ns, slot, p)
        assert e.value.code == api.IS3D_EINVAL, (bins, ne, ns, slot)
    assert api.resource_counters() == before
    with pytest.raises(api.Is3dError) as e:
        api.hbt_list_device(dict(H.BINS, kernel_form=2, n_q=15), 2, 2, [0, 1], p)
    assert "%d bins" % (3 * 15 ** 3) in str(e.value)                                        # the refusal names the word count
    for form in (3, -1, 2):                                                                 # the host entries do not read kernel_form
        assert api.hbt_list(dict(H.BINS, kernel_form=form, n_q=15), 2, 2, [0, 1], p)["den"].sum() == 6      # three particles of one momentum
    for bad in (dict(species=5), dict(species=-1), dict(event=2), dict(event=-1)):         # the host entry refuses a particle out of range
        q = some_list()
        for k, v in bad.items():
            q[k][1] = v
        with pytest.raises(api.Is3dError) as e:
            api.hbt_list(H.BINS, 2, 2, [0, 1], q)
        assert e.value.code == api.IS3D_EINVAL and "particle 1" in str(e.value)


def test_null_arguments_are_refused():
    L = api.load()
    p = some_list()
    slot = np.zeros(1, dtype=np.int32)
    b = api._pack_hbt_bins(H.BINS)
    h, _keep = api._hbt_arrays(b, 2, 1)
    skipped = ctypes.c_int64(0)
    bp, hp = ctypes.POINTER(api.HbtBins), ctypes.POINTER(api.HbtHist)
    L.is3d_hbt_list.argtypes = [bp, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, hp]
    L.is3d_hbt_list_device.argtypes = L.is3d_hbt_list.argtypes + [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    good = [ctypes.byref(b), 2, 1, slot.ctypes.data, 1, 3, p.ctypes.data, ctypes.byref(h)]
    before = api.resource_counters()
    for k, bad in ((0, None), (3, None), (6, None), (7, None), (7, ctypes.byref(api.HbtHist(h.num, None, h.M))),
                   (7, ctypes.byref(api.HbtHist(None, h.den, h.M))), (7, ctypes.byref(api.HbtHist(h.num, h.den, None))), (5, -1), (4, 0)):
        a = list(good)
        a[k] = bad
        assert L.is3d_hbt_list(*a) == api.IS3D_EINVAL, k
        assert L.is3d_hbt_list_device(*a, ctypes.byref(skipped), 0) == api.IS3D_EINVAL, k
    assert L.is3d_hbt_list_device(*good, None, 0) == api.IS3D_EINVAL
    L.is3d_hbt_radii.argtypes = [bp, hp, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p]
    res = (api.HbtRadii * 3)()
    assert L.is3d_hbt_radii(ctypes.byref(b), ctypes.byref(h), 1, 1, 0.1, res) == api.IS3D_OK and all(r.singular == 1 for r in res)
    for a in ((None, ctypes.byref(h), 1, 1, 0.1, res), (ctypes.byref(b), None, 1, 1, 0.1, res), (ctypes.byref(b), ctypes.byref(h), 1, 1, 0.1, None),
              (ctypes.byref(b), ctypes.byref(h), 0, 1, 0.1, res), (ctypes.byref(b), ctypes.byref(h), 1, 0, 0.1, res),
              (ctypes.byref(b), ctypes.byref(h), 1, 1, 0.0, res), (ctypes.byref(b), ctypes.byref(h), 1, 1, NAN, res),
              (ctypes.byref(api._pack_hbt_bins(dict(H.BINS, n_q=1))), ctypes.byref(h), 1, 1, 0.1, res)):
        assert L.is3d_hbt_radii(*a) == api.IS3D_EINVAL
    assert api.resource_counters() == before


def test_no_cpu_path_behind_the_device_entry():
    """Without a device a good call is IS3D_ENODEVICE; with one it is the host route's histograms (tests/test_gpu_hbt.py holds it to more)."""
    if api.load().is3d_device_count() == 0:
        with pytest.raises(api.Is3dError) as e:
            api.hbt_list_device(H.BINS, 2, 1, [0], some_list())
        assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
    else:
        got, skipped = api.hbt_list_device(H.BINS, 2, 1, [0], some_list())
        assert skipped == 0 and H.same_counts(got, api.hbt_list(H.BINS, 2, 1, [0], some_list()))


# ---- the decay entry and the one-shot sampler entry: every refusal without a device ----
RHO = pairs_abi.RHO


def test_decay_particles_hbt_refuses_before_any_device_use():
    import decays_mc_ref as ref
    q = ref.make_particles(api, RHO, RHO["mc_id"], [2, 0, 2], np.zeros((3, 3)), events=[0, 1, 1])
    slot = np.array([0, 0, -1], np.int32)
    before = api.resource_counters()
    bad_event = q.copy()
    bad_event["event"][1] = 2
    bad_species = q.copy()
    bad_species["species"][0] = 3
    lost = dict(RHO, mc_id=np.array([211, -2, 113], np.int64))          # the rho's second product is not in the table
    for kw in (dict(bins=dict(H.BINS, y_cut=0.0)), dict(bins=dict(H.BINS, pT_max=0.01)), dict(bins=dict(H.BINS, n_q=1)), dict(bins=dict(H.BINS, kernel_form=5)),
               dict(bins=dict(H.BINS, kernel_form=2, n_q=15)), dict(n_slots=0), dict(slot=np.array([0, 1, -1], np.int32)),
               dict(slot=np.array([0, -2, -1], np.int32)), dict(n_events=0), dict(n_events=-3), dict(q=bad_event), dict(q=bad_species), dict(table=lost)):
        a = dict(q=q, slot=slot, n_slots=1, bins=H.BINS, n_events=2, table=RHO)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_hbt(a["table"], RHO["mc_id"], a["q"], a["slot"], a["n_slots"], a["bins"], a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    L = api.load()
    ts, ch, _, keep = api._decay_pack(RHO, RHO["mc_id"], dict(pT=[1.0], phi=[0.0], y=[0.0]))
    inp = api.DecayMcInputs(1, 0, 0, -1)
    b = api._pack_hbt_bins(H.BINS)
    h, _keep = api._hbt_arrays(b, 2, 1)
    st, nf, nu = api.DecayMcStats(), ctypes.c_int64(0), ctypes.c_int64(0)
    V = ctypes.c_void_p
    L.is3d_decay_particles_hbt.argtypes = [V, ctypes.c_int32, V, V, ctypes.c_int64, V, V, ctypes.c_int32, V, ctypes.c_int32, V, V, V, V]
    addr = lambda x: ctypes.cast(ctypes.byref(x), V)  # noqa: E731
    good = [addr(ts), 3, V(ch.ctypes.data), addr(inp), 3, V(q.ctypes.data), V(slot.ctypes.data), 1, addr(b), 2, addr(h), addr(nf), addr(nu), addr(st)]
    for k in (0, 2, 3, 5, 6, 8, 10, 11, 12):
        a = list(good)
        a[k] = None
        assert L.is3d_decay_particles_hbt(*a) == api.IS3D_EINVAL, k
    assert api.resource_counters() == before
    if L.is3d_device_count() == 0:
        assert L.is3d_decay_particles_hbt(*good) == api.IS3D_ENODEVICE
    hist, st0 = api.decay_particles_hbt(RHO, RHO["mc_id"], q[:0], slot, 1, H.BINS, 2)
    assert st0["n_final"] == st0["n_unbinned"] == 0 and all(not v.any() for v in hist.values()) and api.resource_counters() == before


def test_sample_hbt_refuses_before_any_device_use():
    cells = synth.synth_surface(3, 3, seed=1)
    sp, gla, df, o = inputs.species([211, 113]), inputs.feqmod_tables(0.15), inputs.df_tables(), dict(dimension=3, df_mode=2)
    slot_d = np.array([0, 0, -1], np.int32)
    before = api.resource_counters()
    lost = dict(RHO, mc_id=np.array([211, -211, 114], np.int64))          # the chosen rho0 is not in this table
    for kw in (dict(bins=dict(H.BINS, y_cut=-2.0)), dict(bins=dict(H.BINS, n_kT=17)), dict(bins=dict(H.BINS, kernel_form=2, n_q=15)), dict(slot=[0, 1]),
               dict(n_slots=0), dict(n_events=0), dict(slot_decayed=np.array([0, 1, -1], np.int32)), dict(n_slots_decayed=0), dict(table=lost)):
        a = dict(bins=H.BINS, slot=[0, 0], n_slots=1, n_events=2, table=RHO, slot_decayed=slot_d, n_slots_decayed=1)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.sample_hbt(cells, sp, df, gla, a["bins"], a["slot"], a["n_slots"], o, table=a["table"], chosen_mc_id=sp["mc_id"],
                           slot_decayed=a["slot_decayed"], n_slots_decayed=a["n_slots_decayed"], n_events=a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    with pytest.raises(api.Is3dError) as e:                               # without a table too
        api.sample_hbt(cells, sp, df, gla, dict(H.BINS, pT_min=-1.0), [0, 0], 1, o, n_events=2)
    assert e.value.code == api.IS3D_EINVAL
    assert api.resource_counters() == before
    if api.load().is3d_device_count() == 0:
        for table in (None, RHO):
            with pytest.raises(api.Is3dError) as e:
                api.sample_hbt(cells, sp, df, gla, H.BINS, [0, 0], 1, o, table=table, chosen_mc_id=sp["mc_id"], slot_decayed=slot_d, n_slots_decayed=1,
                               n_events=2)
            assert e.value.code == api.IS3D_ENODEVICE


# ---- the run driver's key: every refusal with its exact text (tests/golden/run_refusals_hbt.json; `python tests/test_hbt_abi.py` records
# them from the build in the tree), nothing written, and the pinned texts of the older keys unchanged beside the new one ----
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_refusals_hbt.json")
KEY = "test_sampler_hbt = 1"
ON = dict(operation=2, test_sampler=1)
DEV = "test_sampler_on_device = 1"
ROWS = {
    "hbt-operation": (dict(operation=1, test_sampler=1), [KEY], [], ["hbt"]),
    "hbt-test_sampler-0": (dict(operation=2), [KEY], [], ["hbt"]),
    "hbt-mode-2": (dict(base.VAH2, test_sampler=1), ["vah_sampler = 1", KEY], [], ["hbt"]),
    "hbt-on-device-0": (dict(ON), [KEY], [], ["hbt"]),
    "hbt-fused": (dict(ON), [DEV, "test_sampler_fused = 1", KEY], [], ["hbt"]),
    "hbt-bad-y_cut": (dict(ON), [DEV, KEY, "hbt_y_cut = 0"], [], ["hbt"]),
    "hbt-bad-pT": (dict(ON), [DEV, KEY, "hbt_pT_min = 1.5", "hbt_pT_max = 1.5"], [], ["hbt"]),
    "hbt-bad-kT": (dict(ON), [DEV, KEY, "hbt_kT_min = 1.0", "hbt_kT_max = 0.5"], [], ["hbt"]),
    "hbt-bad-kT_bins": (dict(ON), [DEV, KEY, "hbt_kT_bins = 17"], [], ["hbt"]),
    "hbt-bad-q_bins-fraction": (dict(ON), [DEV, KEY, "hbt_q_bins = 2.5"], [], ["hbt"]),
    "hbt-bad-q_bins": (dict(ON), [DEV, KEY, "hbt_q_bins = 1"], [], ["hbt"]),
    "hbt-bad-q_max": (dict(ON), [DEV, KEY, "hbt_q_max = -0.1"], [], ["hbt"]),
    "hbt-thresholds-not-finite": (dict(ON), [DEV, KEY, "hbt_y_cut = 400"], [], ["hbt"]),
    "hbt-missing-directory": (dict(ON), [DEV, KEY], [], []),
    "hbt-missing-decayed-directory": (dict(ON), [DEV, "test_sampler_decayed = 1", KEY], [], ["hbt"]),
    "hbt-missing-sampler-key": (dict(operation=2), [KEY], ["test_sampler"], ["hbt"]),
    # two things wrong: the earlier check speaks
    "order-hbt-operation-before-on-device": (dict(operation=0, test_sampler=1), [KEY], [], []),
    "order-hbt-bins-before-directory": (dict(ON), [DEV, KEY, "hbt_y_cut = -1"], [], []),
    "order-decayed-before-hbt": (dict(ON), ["test_sampler_decayed = 1", KEY], [], []),
    "order-pairs-before-hbt": (dict(ON), [DEV, "test_sampler_pairs = 1", KEY, "pairs_y_cut = 0", "hbt_y_cut = 0"], [], ["pairs", "hbt"]),
}
refused_run = flow_abi.refused_run


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_the_rows_of_this_module(golden):
    assert sorted(golden["stderr"]) == sorted(ROWS)
    own = {row: text for row, text in golden["stderr"].items() if row not in ("hbt-missing-sampler-key", "order-decayed-before-hbt", "order-pairs-before-hbt")}
    for row, text in own.items():
        assert "test_sampler_hbt = 1" in text and text.rstrip().endswith("set test_sampler_hbt = 0"), row
    assert "results/hbt" in golden["stderr"]["hbt-missing-directory"] and "results/decayed/hbt" in golden["stderr"]["hbt-missing-decayed-directory"]
    assert "test_sampler_decayed = 1" in golden["stderr"]["order-decayed-before-hbt"] and "test_sampler_pairs = 1" in golden["stderr"]["order-pairs-before-hbt"]
    # the situations that refuse test_sampler_pairs refuse this key too, in the same words but for what each key makes
    with open(pairs_abi.GOLDEN) as f:
        pairs = json.load(f)["stderr"]
    for k in ("missing-directory", "missing-decayed-directory", "missing-sampler-key"):
        assert golden["stderr"]["hbt-" + k] == pairs["pairs-" + k].replace("pairs", "hbt")
    for k in ("operation", "mode-2"):
        assert golden["stderr"]["hbt-" + k] == pairs["pairs-" + k].replace("pairs", "hbt"), k


@pytest.mark.parametrize("row", list(ROWS))
def test_driver_refuses_the_key_with_its_exact_text(tmp_path, golden, row):
    root, r = refused_run(tmp_path, ROWS, row)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr == golden["stderr"][row]
    assert [f for _, _, fs in os.walk(os.path.join(root, "results")) for f in fs] == []


@pytest.mark.parametrize("rows, pinned_path", ((base.ROWS, base.GOLDEN), (flow_abi.ROWS, flow_abi.GOLDEN), (pairs_abi.ROWS, pairs_abi.GOLDEN)),
                         ids=("base", "flow", "pairs"))
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
