"""CPU: the flow entries of include/is3d_amd.h exist, mirror the header's structs, and make every refusal without a device; a good device call
without a device is IS3D_ENODEVICE (no CPU path behind a device entry)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import decays_mc_cases as cases
import flow_cases as F
import test_run_refusals as base
from conftest import ROOT
from is3d_amd import api, inputs, synth

FLOW_SYMBOLS = ("is3d_flow_list", "is3d_flow_list_device", "is3d_flow_merge", "is3d_flow_cumulants", "is3d_decay_particles_flow",
                "is3d_sampler_plan_execute_flow", "is3d_sample_flow", "is3d_write_flow")


def test_symbols_are_exported_and_declared():
    lib = api.load()
    header = open(os.path.join(ROOT, "include", "is3d_amd.h")).read()
    for s in FLOW_SYMBOLS:
        assert hasattr(lib, s) and s in api.EXPORTS and "int %s(" % s in header, s
    assert "#define IS3D_FLOW_HARMONICS 8" in header and api.FLOW_HARMONICS == 8


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "is3d_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(is3d_flow_cuts), offsetof(is3d_flow_cuts, kernel_form), sizeof(is3d_flow_records), sizeof(is3d_flow_result),'
                   'offsetof(is3d_flow_result, avg4), offsetof(is3d_flow_result, n_used_2));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert c == [ctypes.sizeof(api.FlowCuts), api.FlowCuts.kernel_form.offset, ctypes.sizeof(api.FlowRecords), ctypes.sizeof(api.FlowResult),
                 api.FlowResult.avg4.offset, api.FlowResult.n_used_2.offset]


BAD_CUTS = (dict(y_cut=0.0), dict(y_cut=-1.0), dict(y_gap=-0.1), dict(y_gap=2.0), dict(pT_min=-0.1), dict(pT_max=0.2), dict(pT_max=0.1),
            dict(y_cut=float("nan")), dict(pT_max=float("nan")))


def some_list():
    p = np.zeros(3, dtype=api.PARTICLE_DTYPE)
    p["E"], p["px"] = 1.0, 0.5
    return p


@pytest.mark.parametrize("entry", ("flow_list", "flow_list_device"))
def test_refusals_come_before_any_device_use(entry):
    p = some_list()
    call = getattr(api, entry)
    before = api.resource_counters()
    cases = [(dict(F.CUTS, **bad), 2, 2, [0, 1]) for bad in BAD_CUTS]
    cases += [(F.CUTS, 0, 2, [0, 1]), (F.CUTS, -1, 2, [0, 1]), (F.CUTS, 2, 0, [0, 1]), (F.CUTS, 2, 2, [0, 2]), (F.CUTS, 2, 2, [-2, 1]),
              (dict(F.CUTS, kernel_form=3), 2, 2, [0, 1]), (dict(F.CUTS, kernel_form=-1), 2, 2, [0, 1])]
    for cuts, ne, ns, slot in cases:
        with pytest.raises(api.Is3dError) as e:
            call(cuts, ne, ns, slot, p)
        assert e.value.code == api.IS3D_EINVAL, (cuts, ne, ns, slot)
    assert api.resource_counters() == before


def test_form_2_is_refused_when_one_events_records_do_not_fit():
    """160 slots x 51 = 8160 words fit the 8192 words of LDS, 161 x 51 = 8211 do not: the refusal names the size.  The host route has no
    form to refuse."""
    p = some_list()
    with pytest.raises(api.Is3dError) as e:
        api.flow_list_device(dict(F.CUTS, kernel_form=2), 2, 161, [0], p)
    assert e.value.code == api.IS3D_EINVAL and "8211 words" in str(e.value)
    assert api.flow_list(dict(F.CUTS, kernel_form=2), 2, 161, [0], p)["M"].sum() == 3


def test_null_arguments_are_refused():
    L = api.load()
    p = some_list()
    slot = np.zeros(1, dtype=np.int32)
    c = api._pack_cuts(F.CUTS)
    r, _keep = api._flow_arrays(2, 1)
    skipped = ctypes.c_int64(0)
    cp, rp = ctypes.POINTER(api.FlowCuts), ctypes.POINTER(api.FlowRecords)
    L.is3d_flow_list.argtypes = [cp, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, rp]
    L.is3d_flow_list_device.argtypes = L.is3d_flow_list.argtypes + [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    good = [ctypes.byref(c), 2, 1, slot.ctypes.data, 1, 3, p.ctypes.data, ctypes.byref(r)]
    null_r = api.FlowRecords(r.M, None, r.Q_im)
    for k, bad in ((0, None), (3, None), (6, None), (7, None), (7, ctypes.byref(null_r)), (5, -1)):
        a = list(good)
        a[k] = bad
        assert L.is3d_flow_list(*a) == api.IS3D_EINVAL, k
        assert L.is3d_flow_list_device(*a, ctypes.byref(skipped), 0) == api.IS3D_EINVAL, k
    assert L.is3d_flow_list_device(*good, None, 0) == api.IS3D_EINVAL
    L.is3d_flow_merge.argtypes = [rp, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, rp]
    g = np.zeros(1, dtype=np.int32)
    assert L.is3d_flow_merge(None, 2, 1, g.ctypes.data, 1, ctypes.byref(r)) == api.IS3D_EINVAL
    assert L.is3d_flow_merge(ctypes.byref(r), 2, 1, None, 1, ctypes.byref(r)) == api.IS3D_EINVAL
    assert L.is3d_flow_merge(ctypes.byref(r), 2, 1, g.ctypes.data, 0, ctypes.byref(r)) == api.IS3D_EINVAL
    g[0] = 1
    assert L.is3d_flow_merge(ctypes.byref(r), 2, 1, g.ctypes.data, 1, ctypes.byref(r)) == api.IS3D_EINVAL
    L.is3d_flow_cumulants.argtypes = [rp, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    assert L.is3d_flow_cumulants(ctypes.byref(r), 2, 1, None) == api.IS3D_EINVAL
    assert L.is3d_flow_cumulants(ctypes.byref(r), 0, 1, ctypes.byref(api.FlowResult())) == api.IS3D_EINVAL


def test_no_cpu_path_behind_the_device_entry():
    """Without a device a good call is IS3D_ENODEVICE; with one it is the host route's records (tests/test_gpu_flow.py holds it to more)."""
    if api.load().is3d_device_count() == 0:
        with pytest.raises(api.Is3dError) as e:
            api.flow_list_device(F.CUTS, 2, 1, [0], some_list())
        assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
    else:
        got, skipped = api.flow_list_device(F.CUTS, 2, 1, [0], some_list())
        assert skipped == 0 and np.array_equal(got["M"], api.flow_list(F.CUTS, 2, 1, [0], some_list())["M"])


# ---- the decay entry and the one-shot sampler entry: every refusal without a device ----
RHO = cases.hand_table([cases.stable(211, 0.13957), cases.stable(-211, 0.13957), (113, 0.77526, 0.1491, 0, [(2, 1.0, [211, -211])])])


def test_decay_particles_flow_refuses_before_any_device_use():
    import decays_mc_ref as ref
    q = ref.make_particles(api, RHO, RHO["mc_id"], [2, 0, 2], np.zeros((3, 3)), events=[0, 1, 1])
    slot = np.array([0, 0, -1], np.int32)
    before = api.resource_counters()
    bad_event = q.copy()
    bad_event["event"][1] = 2
    bad_species = q.copy()
    bad_species["species"][0] = 3
    lost = dict(RHO, mc_id=np.array([211, -2, 113], np.int64))          # the rho's second product is not in the table
    for kw in (dict(cuts=dict(F.CUTS, y_cut=0.0)), dict(cuts=dict(F.CUTS, pT_max=0.1)), dict(cuts=dict(F.CUTS, kernel_form=3)), dict(n_slots=0),
               dict(slot=np.array([0, 1, -1], np.int32)), dict(slot=np.array([0, -2, -1], np.int32)), dict(n_events=0), dict(n_events=-3), dict(q=bad_event),
               dict(q=bad_species), dict(table=lost), dict(n_slots=161, cuts=dict(F.CUTS, kernel_form=2))):
        a = dict(q=q, slot=slot, n_slots=1, cuts=F.CUTS, n_events=2, table=RHO)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_flow(a["table"], RHO["mc_id"], a["q"], a["slot"], a["n_slots"], a["cuts"], a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    # NULLs through the bare entry: table, chosen list, inputs, particles, slot map, cuts, records, a records array, n_final, n_unbinned
    L = api.load()
    ts, ch, _, keep = api._decay_pack(RHO, RHO["mc_id"], dict(pT=[1.0], phi=[0.0], y=[0.0]))
    inp = api.DecayMcInputs(1, 0, 0, -1)
    c = api._pack_cuts(F.CUTS)
    r, _keep = api._flow_arrays(2, 1)
    null_r = api.FlowRecords(None, r.Q_re, r.Q_im)
    st, nf, nu = api.DecayMcStats(), ctypes.c_int64(0), ctypes.c_int64(0)
    V = ctypes.c_void_p
    L.is3d_decay_particles_flow.argtypes = [V, ctypes.c_int32, V, V, ctypes.c_int64, V, V, ctypes.c_int32, V, ctypes.c_int32, V, V, V, V]
    addr = lambda x: ctypes.cast(ctypes.byref(x), V)  # noqa: E731
    good = [addr(ts), 3, V(ch.ctypes.data), addr(inp), 3, V(q.ctypes.data), V(slot.ctypes.data), 1, addr(c), 2, addr(r), addr(nf), addr(nu), addr(st)]
    for k in (0, 2, 3, 5, 6, 8, 10, 11, 12):
        a = list(good)
        a[k] = None
        assert L.is3d_decay_particles_flow(*a) == api.IS3D_EINVAL, k
    a = list(good)
    a[10] = addr(null_r)
    assert L.is3d_decay_particles_flow(*a) == api.IS3D_EINVAL
    assert api.resource_counters() == before
    if L.is3d_device_count() == 0:
        assert L.is3d_decay_particles_flow(*good) == api.IS3D_ENODEVICE
    # an empty list: zero records, no launch, no device needed
    rec, st0 = api.decay_particles_flow(RHO, RHO["mc_id"], q[:0], slot, 1, F.CUTS, 2)
    assert st0["n_final"] == st0["n_unbinned"] == 0 and all(not v.any() for v in rec.values()) and api.resource_counters() == before
    if L.is3d_device_count() == 0:
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_flow(RHO, RHO["mc_id"], q, slot, 1, F.CUTS, 2)
        assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)


def test_sample_flow_refuses_before_any_device_use():
    cells = synth.synth_surface(3, 3, seed=1)
    sp, gla, df, o = inputs.species([211, 113]), inputs.feqmod_tables(0.15), inputs.df_tables(), dict(dimension=3, df_mode=2)
    slot_d = np.array([0, 0, -1], np.int32)
    before = api.resource_counters()
    lost = dict(RHO, mc_id=np.array([211, -211, 114], np.int64))          # the chosen rho0 is not in this table
    for kw in (dict(cuts=dict(F.CUTS, y_gap=2.0)), dict(cuts=dict(F.CUTS, kernel_form=-1)), dict(slot=[0, 1]), dict(n_slots=0), dict(n_events=0),
               dict(slot_decayed=np.array([0, 1, -1], np.int32)), dict(n_slots_decayed=0), dict(table=lost),
               dict(n_slots=161, cuts=dict(F.CUTS, kernel_form=2))):
        a = dict(cuts=F.CUTS, slot=[0, 0], n_slots=1, n_events=2, table=RHO, slot_decayed=slot_d, n_slots_decayed=1)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.sample_flow(cells, sp, df, gla, a["cuts"], a["slot"], a["n_slots"], o, table=a["table"], chosen_mc_id=sp["mc_id"],
                            slot_decayed=a["slot_decayed"], n_slots_decayed=a["n_slots_decayed"], n_events=a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    with pytest.raises(api.Is3dError) as e:                               # without a table too
        api.sample_flow(cells, sp, df, gla, dict(F.CUTS, pT_min=-1.0), [0, 0], 1, o, n_events=2)
    assert e.value.code == api.IS3D_EINVAL
    assert api.resource_counters() == before
    if api.load().is3d_device_count() == 0:
        for table in (None, RHO):
            with pytest.raises(api.Is3dError) as e:
                api.sample_flow(cells, sp, df, gla, F.CUTS, [0, 0], 1, o, table=table, chosen_mc_id=sp["mc_id"], slot_decayed=slot_d, n_slots_decayed=1,
                                n_events=2)
            assert e.value.code == api.IS3D_ENODEVICE


# ---- the writer ----
def test_write_flow_prints_the_cumulants_and_the_multiplicities(tmp_path):
    p, n_events = F.hand_list()
    rec = api.flow_list(F.CUTS, n_events, 3, F.slot_map(3), p)
    with pytest.raises(api.Is3dError) as e:                               # <dir>/flow/ must exist
        api.write_flow(str(tmp_path), rec, ["211", "321", "other"])
    assert e.value.code == api.IS3D_EIO
    os.makedirs(tmp_path / "flow")
    for labels in (["211", "", "x"], ["211", "a/b", "x"]):
        with pytest.raises(api.Is3dError) as e:
            api.write_flow(str(tmp_path), rec, labels)
        assert e.value.code == api.IS3D_EINVAL
    assert os.listdir(tmp_path / "flow") == []
    api.write_flow(str(tmp_path), rec, ["211", "321", "other"])
    assert sorted(os.listdir(tmp_path / "flow")) == sorted(k + "_" + l + ".dat" for k in ("cumulants", "multiplicity") for l in ("211", "321", "other"))
    c = api.flow_cumulants(rec)
    for s, label in enumerate(("211", "321", "other")):
        rows = np.loadtxt(tmp_path / "flow" / ("cumulants_%s.dat" % label))
        assert rows.shape == (8, 8) and np.array_equal(rows[:, 0], np.arange(1, 9))
        four = lambda a: np.concatenate([a, np.zeros(4)])  # noqa: E731
        want = np.stack([c["c2"][s], four(c["c4"][s]), c["c2_gap"][s], c["v2"][s], four(c["v4"][s]), c["v2_gap"][s], c["v_rp"][s]], axis=1)
        assert np.allclose(rows[:, 1:], want, rtol=1e-8, atol=0)          # nine significant digits are printed
        m = np.loadtxt(tmp_path / "flow" / ("multiplicity_%s.dat" % label))
        head = open(tmp_path / "flow" / ("multiplicity_%s.dat" % label)).readline().split(":")[1].split()
        assert np.allclose([float(x) for x in head], [c["mean_M"][s], c["var_M"][s]], rtol=1e-8) and np.array_equal(m[:, 0], np.arange(n_events))
        assert np.array_equal(m[:, 1:].astype(np.int64), rec["M"][:, s, :])
        text = open(tmp_path / "flow" / ("cumulants_%s.dat" % label)).read()
        assert "events: %d, used for <2>: %d, <4>: %d, <2>_gap: %d" % (n_events, c["n_used_2"][s], c["n_used_4"][s], c["n_used_gap"][s]) in text


# ---- the run driver's key: every refusal with its exact text (tests/golden/run_refusals_flow.json; `python tests/test_flow_abi.py` records
# them from the build in the tree), nothing written, and the pinned texts of the older keys unchanged beside the new one ----
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_refusals_flow.json")
KEY = "test_sampler_flow = 1"
ON = dict(operation=2, test_sampler=1)
DEV = "test_sampler_on_device = 1"
# id -> (parameters of refformat.make_run_dir, lines appended to iS3D_parameters.dat, keys removed, directories made under results/)
ROWS = {
    "flow-operation": (dict(operation=1, test_sampler=1), [KEY], [], ["flow"]),
    "flow-test_sampler-0": (dict(operation=2), [KEY], [], ["flow"]),
    "flow-mode-2": (dict(base.VAH2, test_sampler=1), ["vah_sampler = 1", KEY], [], ["flow"]),
    "flow-on-device-0": (dict(ON), [KEY], [], ["flow"]),
    "flow-fused": (dict(ON), [DEV, "test_sampler_fused = 1", KEY], [], ["flow"]),
    "flow-bad-y_cut": (dict(ON), [DEV, KEY, "flow_y_cut = 0"], [], ["flow"]),
    "flow-bad-y_gap": (dict(ON), [DEV, KEY, "flow_y_gap = 2.0"], [], ["flow"]),
    "flow-bad-pT": (dict(ON), [DEV, KEY, "flow_pT_min = 1.5", "flow_pT_max = 1.5"], [], ["flow"]),
    "flow-missing-directory": (dict(ON), [DEV, KEY], [], []),
    "flow-missing-decayed-directory": (dict(ON), [DEV, "test_sampler_decayed = 1", KEY], [], ["flow"]),
    "flow-missing-sampler-key": (dict(operation=2), [KEY], ["test_sampler"], ["flow"]),
    # two things wrong: the earlier check speaks
    "order-flow-operation-before-on-device": (dict(operation=0, test_sampler=1), [KEY], [], []),
    "order-flow-cuts-before-directory": (dict(ON), [DEV, KEY, "flow_y_cut = -1"], [], []),
    "order-decayed-before-flow": (dict(ON), ["test_sampler_decayed = 1", KEY], [], []),
}


def refused_run(tmp_path, rows, row, extra=()):
    import refformat
    params, lines, drop = rows[row][:3]
    dirs = rows[row][3] if len(rows[row]) > 3 else []
    root = refformat.make_run_dir(str(tmp_path / "run"), synth.synth_surface(3, 3, seed=1), [211], params)
    for d in dirs:
        os.makedirs(os.path.join(root, "results", d), exist_ok=True)
    path = os.path.join(root, "iS3D_parameters.dat")
    with open(path) as f:
        kept = [ln for ln in f.read().split("\n") if ln.split("=")[0].strip().lower() not in drop]
    with open(path, "w") as f:
        f.write("\n".join(kept) + "".join(ln + "\n" for ln in list(lines) + list(extra)))
    env = dict(os.environ)
    env.pop("IS3D_DEVICES", None)
    return root, subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=120, env=env)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_the_rows_of_this_module(golden):
    assert sorted(golden["stderr"]) == sorted(ROWS)
    own = {row: text for row, text in golden["stderr"].items() if row not in ("flow-missing-sampler-key", "order-decayed-before-flow")}
    assert len(set(own.values())) == 12      # six refusals of the key's place (one at two operations), four sets of bad cuts, two directories
    for row, text in own.items():
        assert "test_sampler_flow = 1" in text and text.rstrip().endswith("set test_sampler_flow = 0"), row
    assert "results/flow" in golden["stderr"]["flow-missing-directory"] and "results/decayed/flow" in golden["stderr"]["flow-missing-decayed-directory"]
    assert "test_sampler_decayed = 1" in golden["stderr"]["order-decayed-before-flow"]


@pytest.mark.parametrize("row", list(ROWS))
def test_driver_refuses_the_key_with_its_exact_text(tmp_path, golden, row):
    root, r = refused_run(tmp_path, ROWS, row)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr == golden["stderr"][row]
    assert [f for _, _, fs in os.walk(os.path.join(root, "results")) for f in fs] == []


@pytest.mark.parametrize("row", list(base.ROWS))
def test_existing_refusals_keep_their_texts_beside_the_new_key(tmp_path, row):
    with open(base.GOLDEN) as f:
        pinned = json.load(f)["stderr"]
    root, r = refused_run(tmp_path, base.ROWS, row, extra=[KEY])
    assert r.returncode == 1 and r.stderr == pinned[row], r.stderr
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
