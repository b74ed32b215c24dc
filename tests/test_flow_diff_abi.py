"""CPU: the differential-flow entries of include/is3d_amd.h exist, mirror the header's structs, and make every refusal without a device; a
good device call without a device is IS3D_ENODEVICE (no CPU path behind a device entry); the writer's file byte for byte; the run driver's
key with every refusal's text."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import flow_cases as F
import flow_diff_cases as D
import test_flow_abi as flow_abi
from conftest import ROOT
from is3d_amd import api, inputs, synth

SYMBOLS = ("is3d_flow_diff_list", "is3d_flow_diff_list_device", "is3d_flow_diff_reference", "is3d_flow_diff_cumulants", "is3d_write_flow_diff",
           "is3d_decay_particles_flow_diff", "is3d_sampler_plan_execute_flow_diff", "is3d_sample_flow_diff")
HEADER = open(os.path.join(ROOT, "include", "is3d_amd.h")).read()
CSRC = os.path.join(ROOT, "is3d_amd", "csrc")


def test_symbols_are_exported_and_declared():
    lib = api.load()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in api.EXPORTS and "int %s(" % s in HEADER, s
    assert "#define IS3D_FLOW_DIFF_MAX_BINS 64" in HEADER and api.FLOW_DIFF_MAX_BINS == 64
    for f in ("flow_list_device", "decay_particles_flow", "sample_flow", "flow_list", "flow_reference", "flow_cumulants"):
        name = f.replace("flow", "flow_diff")
        assert callable(getattr(api, name)), name
    assert callable(api.write_flow_diff) and callable(api.SamplerPlan.execute_flow_diff)


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "is3d_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(is3d_flow_diff_records), sizeof(is3d_flow_diff_result), offsetof(is3d_flow_diff_result, avg4),'
                   'offsetof(is3d_flow_diff_result, mean_m), offsetof(is3d_flow_diff_result, sum_m), offsetof(is3d_flow_diff_result, n_used_2));'
                   'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert c == [ctypes.sizeof(api.FlowDiffRecords), ctypes.sizeof(api.FlowDiffResult), api.FlowDiffResult.avg4.offset,
                 api.FlowDiffResult.mean_m.offset, api.FlowDiffResult.sum_m.offset, api.FlowDiffResult.n_used_2.offset]


E3 = np.array([0.2, 1.0, 3.0])
NAN = float("nan")
BAD_EDGES = ([0.2, 1.0, 1.0, 3.0], [0.2, 2.0, 1.0, 3.0], [0.2, NAN, 3.0], [NAN, 1.0, 3.0], [0.2, 1.0, NAN], [-0.1, 1.0, 3.0], [0.2, 1.0, float("inf")],
             [3.0, 1.0, 0.2], [0.2], np.linspace(0.2, 3.0, 66))          # equal, descending, NaN, negative, infinite, n_pT = 0 and 65


def some_list():
    p = np.zeros(3, dtype=api.PARTICLE_DTYPE)
    p["E"], p["px"] = 1.0, 0.5
    return p


@pytest.mark.parametrize("entry", ("flow_diff_list", "flow_diff_list_device"))
def test_refusals_come_before_any_device_use(entry):
    p = some_list()
    call = getattr(api, entry)
    before = api.resource_counters()
    good = D.cuts_for(E3)
    rows = [(D.cuts_for(E3, **{k: v for k, v in bad.items() if k not in ("pT_min", "pT_max")}), E3, 2, 2, [0, 1])
            for bad in flow_abi.BAD_CUTS if not set(bad) & {"pT_min", "pT_max"}]
    assert len(rows) == 5
    rows += [(D.cuts_for(np.asarray(e, dtype=np.float64)), e, 2, 2, [0, 1]) for e in BAD_EDGES]
    # the ends of the table are the acceptance, bit for bit
    rows += [(dict(good, pT_min=np.nextafter(0.2, 1.0)), E3, 2, 2, [0, 1]), (dict(good, pT_min=0.0), E3, 2, 2, [0, 1]),
             (dict(good, pT_max=np.nextafter(3.0, 0.0)), E3, 2, 2, [0, 1]), (dict(good, pT_max=3.5), E3, 2, 2, [0, 1])]
    # every refusal of is3d_flow_list
    rows += [(good, E3, 0, 2, [0, 1]), (good, E3, -1, 2, [0, 1]), (good, E3, 2, 0, [0, 1]), (good, E3, 2, 2, [0, 2]), (good, E3, 2, 2, [-2, 1]),
             (dict(good, kernel_form=3), E3, 2, 2, [0, 1]), (dict(good, kernel_form=-1), E3, 2, 2, [0, 1])]
    for cuts, edges, ne, ns, slot in rows:
        with pytest.raises(api.Is3dError) as e:
            call(cuts, edges, ne, ns, slot, p)
        assert e.value.code == api.IS3D_EINVAL, (cuts, edges, ne, ns, slot)
    bad_particle = p.copy()
    bad_particle["species"][1] = 2
    with pytest.raises(api.Is3dError) as e:                                # the host route refuses a particle out of range
        api.flow_diff_list(good, E3, 2, 2, [0, 1], bad_particle)
    assert e.value.code == api.IS3D_EINVAL
    assert api.resource_counters() == before
    assert api.flow_diff_list(good, E3, 2, 2, [0, 1], p)["m"][0, 0, :, 0].tolist() == [3, 0]


def header_constants():
    """(LDS words, words per (event, slot, bin), words kept for the staged edges, the decay pass's tally words) from the headers."""
    flow = open(os.path.join(CSRC, "cf_sampler_flow.h")).read()
    diff = open(os.path.join(CSRC, "cf_sampler_flow_diff.h")).read()
    mc = open(os.path.join(CSRC, "cf_decays_mc.h")).read()
    assert "kFlowLdsWords = 65536 / sizeof(unsigned long long)" in flow and "kFlowRegions = 3;" in flow
    assert "kFlowRegionWords = 1 + 2 * IS3D_FLOW_HARMONICS" in flow and "kFlowRecordWords = kFlowRegions * kFlowRegionWords" in flow
    assert "kFlowDiffEdgeWords = kFlowDiffMaxBins + 2;" in diff and "kFlowDiffMaxBins = IS3D_FLOW_DIFF_MAX_BINS" in diff
    tallies = int(re.search(r"kDecayMcBinTallies = (\d+);", mc).group(1))
    return 65536 // 8, 3 * (1 + 2 * api.FLOW_HARMONICS), api.FLOW_DIFF_MAX_BINS + 2, tallies


def test_form_2_is_refused_when_one_events_records_do_not_fit():
    """The window has 8192 - 66 = 8126 words: 3 slots x 53 bins x 51 = 8109 words fit, 4 x 40 x 51 = 8160 do not.  The refusal names the
    size; the largest that fits is not refused (without a device: IS3D_ENODEVICE).  The host route has no form to refuse."""
    lds, rec, edge_words, tallies = header_constants()
    assert (lds, rec, edge_words, tallies) == (8192, 51, 66, 6)
    keys = (lds - edge_words) // rec
    assert keys == 159 == 3 * 53 and (keys + 1) * rec > lds - edge_words and 160 == 4 * 40
    assert (lds - edge_words - tallies) // rec == 159                       # the decay pass, beside its tally words, has the same limit
    p = some_list()
    e40, e53 = api.flow_diff_edges(0.2, 3.0, 40), api.flow_diff_edges(0.2, 3.0, 53)
    with pytest.raises(api.Is3dError) as e:
        api.flow_diff_list_device(D.cuts_for(e40, kernel_form=2), e40, 2, 4, [0], p)
    assert e.value.code == api.IS3D_EINVAL and "8160 words" in str(e.value)
    assert api.flow_diff_list(D.cuts_for(e40, kernel_form=2), e40, 2, 4, [0], p)["m"].sum() == 3
    if api.load().is3d_device_count() == 0:
        with pytest.raises(api.Is3dError) as e:
            api.flow_diff_list_device(D.cuts_for(e53, kernel_form=2), e53, 2, 3, [0], p)
        assert e.value.code == api.IS3D_ENODEVICE
        with pytest.raises(api.Is3dError) as e:                            # form 0 takes the global form where nothing fits
            api.flow_diff_list_device(D.cuts_for(e40), e40, 2, 4, [0], p)
        assert e.value.code == api.IS3D_ENODEVICE
    else:
        got, _ = api.flow_diff_list_device(D.cuts_for(e53, kernel_form=2), e53, 2, 3, [0], p)
        assert got["m"].sum() == 3


def test_null_arguments_are_refused():
    L = api.load()
    p = some_list()
    slot = np.zeros(1, dtype=np.int32)
    c = api._pack_cuts(D.cuts_for(E3))
    r, _keep = api._flow_diff_arrays(2, 1, 2)
    skipped = ctypes.c_int64(0)
    V, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    addr = lambda x: ctypes.cast(ctypes.byref(x), V)  # noqa: E731
    L.is3d_flow_diff_list.argtypes = [V, i32, V, i32, i32, V, i32, i64, V, V]
    L.is3d_flow_diff_list_device.argtypes = L.is3d_flow_diff_list.argtypes + [V, i32]
    good = [addr(c), 2, V(E3.ctypes.data), 2, 1, V(slot.ctypes.data), 1, 3, V(p.ctypes.data), addr(r)]
    assert L.is3d_flow_diff_list(*good) == 0
    holes = [api.FlowDiffRecords(None, r.p_re, r.p_im), api.FlowDiffRecords(r.m, None, r.p_im), api.FlowDiffRecords(r.m, r.p_re, None)]
    for k, bad in [(0, None), (2, None), (5, None), (8, None), (9, None), (7, -1)] + [(9, addr(h)) for h in holes]:
        a = list(good)
        a[k] = bad
        assert L.is3d_flow_diff_list(*a) == api.IS3D_EINVAL, k
        assert L.is3d_flow_diff_list_device(*a, addr(skipped), 0) == api.IS3D_EINVAL, k
    assert L.is3d_flow_diff_list_device(*good, None, 0) == api.IS3D_EINVAL
    # the reference, the cumulants, the writer
    ref_slot = np.ones(1, dtype=np.int32)
    o, _keep_o = api._flow_arrays(2, 1)
    res = (api.FlowDiffResult * 2)()
    L.is3d_flow_diff_reference.argtypes = [V, i32, i32, i32, V, i32, i32, V]
    L.is3d_flow_diff_cumulants.argtypes = [V, i32, i32, i32, V, i32, i32, V]
    good = [addr(r), 2, 1, 2, V(ref_slot.ctypes.data), 0, 2]
    assert L.is3d_flow_diff_reference(*good, addr(o)) == 0 and L.is3d_flow_diff_cumulants(*good, ctypes.cast(res, V)) == 0
    two = np.array([2], dtype=np.int32)
    for k, bad in [(0, None), (4, None), (1, 0), (2, 0), (3, 0), (3, 65), (5, -1), (6, 3), (5, 2), (4, V(two.ctypes.data))] + [(0, addr(h)) for h in holes]:
        a = list(good)
        a[k] = bad
        assert L.is3d_flow_diff_reference(*a, addr(o)) == api.IS3D_EINVAL, k
        assert L.is3d_flow_diff_cumulants(*a, ctypes.cast(res, V)) == api.IS3D_EINVAL, k
    assert L.is3d_flow_diff_reference(*good, None) == api.IS3D_EINVAL and L.is3d_flow_diff_cumulants(*good, None) == api.IS3D_EINVAL
    assert L.is3d_flow_diff_reference(*good, addr(api.FlowRecords(o.M, None, o.Q_im))) == api.IS3D_EINVAL


def test_no_cpu_path_behind_the_device_entry():
    if api.load().is3d_device_count() == 0:
        with pytest.raises(api.Is3dError) as e:
            api.flow_diff_list_device(D.cuts_for(E3), E3, 2, 1, [0], some_list())
        assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
    else:
        got, skipped = api.flow_diff_list_device(D.cuts_for(E3), E3, 2, 1, [0], some_list())
        assert skipped == 0 and np.array_equal(got["m"], api.flow_diff_list(D.cuts_for(E3), E3, 2, 1, [0], some_list())["m"])


# ---- the decay entry and the one-shot sampler entry: every refusal without a device ----
RHO = flow_abi.RHO


def test_decay_particles_flow_diff_refuses_before_any_device_use():
    import decays_mc_ref as ref
    q = ref.make_particles(api, RHO, RHO["mc_id"], [2, 0, 2], np.zeros((3, 3)), events=[0, 1, 1])
    slot = np.array([0, 0, -1], np.int32)
    good = D.cuts_for(E3)
    before = api.resource_counters()
    bad_event = q.copy()
    bad_event["event"][1] = 2
    bad_species = q.copy()
    bad_species["species"][0] = 3
    lost = dict(RHO, mc_id=np.array([211, -2, 113], np.int64))          # the rho's second product is not in the table
    e40 = api.flow_diff_edges(0.2, 3.0, 40)
    rows = [dict(cuts=dict(good, y_cut=0.0)), dict(cuts=dict(good, pT_max=0.1)), dict(cuts=dict(good, pT_max=3.5)), dict(cuts=dict(good, kernel_form=3)),
            dict(n_slots=0), dict(slot=np.array([0, 1, -1], np.int32)), dict(slot=np.array([0, -2, -1], np.int32)), dict(n_events=0), dict(n_events=-3),
            dict(q=bad_event), dict(q=bad_species), dict(table=lost), dict(n_slots=4, edges=e40, cuts=D.cuts_for(e40, kernel_form=2))]
    rows += [dict(edges=e, cuts=D.cuts_for(np.asarray(e, dtype=np.float64))) for e in BAD_EDGES]
    for kw in rows:
        a = dict(q=q, slot=slot, n_slots=1, cuts=good, edges=E3, n_events=2, table=RHO)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_flow_diff(a["table"], RHO["mc_id"], a["q"], a["slot"], a["n_slots"], a["cuts"], a["edges"], a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    # NULLs through the bare entry
    L = api.load()
    ts, ch, _, keep = api._decay_pack(RHO, RHO["mc_id"], dict(pT=[1.0], phi=[0.0], y=[0.0]))
    inp = api.DecayMcInputs(1, 0, 0, -1)
    c = api._pack_cuts(good)
    r, _keep = api._flow_diff_arrays(2, 1, 2)
    null_r = api.FlowDiffRecords(None, r.p_re, r.p_im)
    st, nf, nu = api.DecayMcStats(), ctypes.c_int64(0), ctypes.c_int64(0)
    V = ctypes.c_void_p
    L.is3d_decay_particles_flow_diff.argtypes = [V, ctypes.c_int32, V, V, ctypes.c_int64, V, V, ctypes.c_int32, V, ctypes.c_int32, V, ctypes.c_int32, V, V,
                                                 V, V]
    addr = lambda x: ctypes.cast(ctypes.byref(x), V)  # noqa: E731
    ok = [addr(ts), 3, V(ch.ctypes.data), addr(inp), 3, V(q.ctypes.data), V(slot.ctypes.data), 1, addr(c), 2, V(E3.ctypes.data), 2, addr(r), addr(nf),
          addr(nu), addr(st)]
    for k in (0, 2, 3, 5, 6, 8, 10, 12, 13, 14):
        a = list(ok)
        a[k] = None
        assert L.is3d_decay_particles_flow_diff(*a) == api.IS3D_EINVAL, k
    a = list(ok)
    a[12] = addr(null_r)
    assert L.is3d_decay_particles_flow_diff(*a) == api.IS3D_EINVAL
    assert api.resource_counters() == before
    if L.is3d_device_count() == 0:
        assert L.is3d_decay_particles_flow_diff(*ok) == api.IS3D_ENODEVICE
    # an empty list: zero records, no launch, no device needed
    rec, st0 = api.decay_particles_flow_diff(RHO, RHO["mc_id"], q[:0], slot, 1, good, E3, 2)
    assert st0["n_final"] == st0["n_unbinned"] == 0 and all(not v.any() for v in rec.values()) and api.resource_counters() == before
    assert rec["m"].shape == (2, 1, 2, 3)


def test_sample_flow_diff_refuses_before_any_device_use():
    cells = synth.synth_surface(3, 3, seed=1)
    sp, gla, df, o = inputs.species([211, 113]), inputs.feqmod_tables(0.15), inputs.df_tables(), dict(dimension=3, df_mode=2)
    slot_d = np.array([0, 0, -1], np.int32)
    good = D.cuts_for(E3)
    before = api.resource_counters()
    lost = dict(RHO, mc_id=np.array([211, -211, 114], np.int64))          # the chosen rho0 is not in this table
    e40 = api.flow_diff_edges(0.2, 3.0, 40)
    rows = [dict(cuts=dict(good, y_gap=2.0)), dict(cuts=dict(good, kernel_form=-1)), dict(cuts=dict(good, pT_min=0.1)), dict(slot=[0, 1]), dict(n_slots=0),
            dict(n_events=0), dict(slot_decayed=np.array([0, 1, -1], np.int32)), dict(n_slots_decayed=0), dict(table=lost),
            dict(n_slots=4, edges=e40, cuts=D.cuts_for(e40, kernel_form=2)), dict(n_slots_decayed=4, edges=e40, cuts=D.cuts_for(e40, kernel_form=2))]
    rows += [dict(edges=e, cuts=D.cuts_for(np.asarray(e, dtype=np.float64))) for e in BAD_EDGES]
    for kw in rows:
        a = dict(cuts=good, edges=E3, slot=[0, 0], n_slots=1, n_events=2, table=RHO, slot_decayed=slot_d, n_slots_decayed=1)
        a.update(kw)
        with pytest.raises(api.Is3dError) as e:
            api.sample_flow_diff(cells, sp, df, gla, a["cuts"], a["edges"], a["slot"], a["n_slots"], o, table=a["table"], chosen_mc_id=sp["mc_id"],
                                 slot_decayed=a["slot_decayed"], n_slots_decayed=a["n_slots_decayed"], n_events=a["n_events"])
        assert e.value.code == api.IS3D_EINVAL, kw
    with pytest.raises(api.Is3dError) as e:                               # without a table too
        api.sample_flow_diff(cells, sp, df, gla, good, [0.2, 0.1, 3.0], [0, 0], 1, o, n_events=2)
    assert e.value.code == api.IS3D_EINVAL
    assert api.resource_counters() == before
    if api.load().is3d_device_count() == 0:
        for table in (None, RHO):
            with pytest.raises(api.Is3dError) as e:
                api.sample_flow_diff(cells, sp, df, gla, good, E3, [0, 0], 1, o, table=table, chosen_mc_id=sp["mc_id"], slot_decayed=slot_d,
                                     n_slots_decayed=1, n_events=2)
            assert e.value.code == api.IS3D_ENODEVICE


# ---- the writer ----
def sci(v):
    """std::to_chars(scientific, 8)"""
    return "%.8e" % v


def test_write_flow_diff_is_reproduced_byte_for_byte_from_the_result(tmp_path):
    p, slot = D.random_list(), F.slot_map(3)
    rec = api.flow_diff_list(D.CUTS, D.EDGES, 3, 3, slot, p)
    labels = ["211", "321", "other"]
    ref_slot, ref_bins = [1, 0, 1], (1, 12)
    with pytest.raises(api.Is3dError) as e:                               # <dir>/flow/ must exist
        api.write_flow_diff(str(tmp_path), rec, D.EDGES, labels)
    assert e.value.code == api.IS3D_EIO
    os.makedirs(tmp_path / "flow")
    for bad in (["211", "", "x"], ["211", "a/b", "x"]):
        with pytest.raises(api.Is3dError) as e:
            api.write_flow_diff(str(tmp_path), rec, D.EDGES, bad)
        assert e.value.code == api.IS3D_EINVAL
    with pytest.raises(api.Is3dError) as e:
        api.write_flow_diff(str(tmp_path), rec, D.EDGES[::-1].copy(), labels)
    assert e.value.code == api.IS3D_EINVAL
    assert os.listdir(tmp_path / "flow") == []
    api.write_flow_diff(str(tmp_path), rec, D.EDGES, labels, ref_slot, ref_bins)
    assert sorted(os.listdir(tmp_path / "flow")) == sorted("differential_%s.dat" % l for l in labels)
    c = api.flow_diff_cumulants(rec, ref_slot, ref_bins)
    n_pT = len(D.EDGES) - 1
    for s, label in enumerate(labels):
        text = "# bin\tpT_lo\tpT_hi\tn\td_n{2}\td_n{4}\td_n{2,gap}\tv_n{2}\tv_n{4}\tv_n{2,gap}\tv_n (reaction plane)\tsum m_p; " \
               "d_n{4} and v_n{4} exist for n <= 4 (0 beyond)\n"
        text += "# events: 3, pT bins: %d, reference bins: [%d, %d), this slot in the reference: %d\n" % (n_pT, ref_bins[0], ref_bins[1], ref_slot[s])
        for b in range(n_pT):
            for n in range(8):
                four = lambda a: a[s, b, n] if n < 4 else 0.0  # noqa: E731
                row = [c["d2"][s, b, n], four(c["d4"]), c["d2_gap"][s, b, n], c["v2"][s, b, n], four(c["v4"]), c["v2_gap"][s, b, n], c["v_rp"][s, b, n]]
                text += "\t".join([str(b), sci(D.EDGES[b]), sci(D.EDGES[b + 1]), str(n + 1)] + [sci(v) for v in row] + [str(int(c["sum_m"][s, b]))]) + "\n"
        assert open(tmp_path / "flow" / ("differential_%s.dat" % label), "rb").read() == text.encode(), label
    assert c["sum_m"].sum() == rec["m"][..., 0].sum() and np.any(c["d2"] != 0)


# ---- the run driver's key: every refusal with its exact text (tests/golden/run_refusals_flow_diff.json; `python tests/test_flow_diff_abi.py`
# records them from the build in the tree), nothing written ----
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_refusals_flow_diff.json")
FLOW, KEY = flow_abi.KEY, "test_sampler_flow_diff = 1"
ON, DEV = flow_abi.ON, flow_abi.DEV
# the rows where test_sampler_flow is refused: the same parameters with the new key beside it, and the text of that refusal
INHERITED = ("flow-operation", "flow-test_sampler-0", "flow-mode-2", "flow-on-device-0", "flow-fused", "flow-bad-y_cut", "flow-bad-pT",
             "flow-missing-directory", "flow-missing-decayed-directory")
ROWS = {"diff-" + row: (v[0], list(v[1]) + [KEY], v[2], v[3]) for row, v in flow_abi.ROWS.items() if row in INHERITED}
ROWS.update({
    "diff-without-flow": (dict(ON), [DEV, KEY], [], ["flow"]),
    "diff-flow-0": (dict(ON), [DEV, "test_sampler_flow = 0", KEY], [], ["flow"]),
    "diff-bins-0": (dict(ON), [DEV, FLOW, KEY, "flow_diff_pt_bins = 0"], [], ["flow"]),
    "diff-bins-65": (dict(ON), [DEV, FLOW, KEY, "flow_diff_pt_bins = 65"], [], ["flow"]),
    "diff-bins-fraction": (dict(ON), [DEV, FLOW, KEY, "flow_diff_pt_bins = 7.5"], [], ["flow"]),
    "diff-pt-max-below-min": (dict(ON), [DEV, FLOW, KEY, "flow_pT_min = 0.5", "flow_diff_pt_max = 0.5"], [], ["flow"]),
    "diff-no-width": (dict(ON), [DEV, FLOW, KEY, "flow_pT_min = 1", "flow_pT_max = 2", "flow_diff_pt_max = 1.0000000000000004", "flow_diff_pt_bins = 64"], [],
                      ["flow"]),
    # two things wrong: the earlier check speaks
    "order-flow-before-diff-bins": (dict(ON), [DEV, FLOW, KEY, "flow_y_cut = -1", "flow_diff_pt_bins = 0"], [], ["flow"]),
    "order-diff-without-flow-before-bins": (dict(ON), [DEV, KEY, "flow_diff_pt_bins = 0"], [], ["flow"]),
})


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_the_rows_of_this_module(golden):
    assert sorted(golden["stderr"]) == sorted(ROWS)
    with open(flow_abi.GOLDEN) as f:
        flow = json.load(f)["stderr"]
    for row in INHERITED:                                                 # refused wherever test_sampler_flow is, in its words
        assert golden["stderr"]["diff-" + row] == flow[row], row
    for row in ("diff-without-flow", "diff-flow-0", "order-diff-without-flow-before-bins"):
        assert "test_sampler_flow_diff = 1 with test_sampler_flow = 0" in golden["stderr"][row], row
    for row in ("diff-bins-0", "diff-bins-65", "diff-bins-fraction", "diff-pt-max-below-min", "diff-no-width"):
        text = golden["stderr"][row]
        assert "flow_diff_pt_bins = " in text and "flow_diff_pt_max = " in text and text.rstrip().endswith("set test_sampler_flow_diff = 0"), row
    assert golden["stderr"]["order-flow-before-diff-bins"] == flow["order-flow-cuts-before-directory"]
    assert len(set(golden["stderr"].values())) == len(INHERITED) + 1 + 1 + 5   # ... one more set of bad cuts, the key without its companion, five sets of bad bins


@pytest.mark.parametrize("row", list(ROWS))
def test_driver_refuses_the_key_with_its_exact_text(tmp_path, golden, row):
    root, r = flow_abi.refused_run(tmp_path, ROWS, row)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr == golden["stderr"][row]
    assert [f for _, _, fs in os.walk(os.path.join(root, "results")) for f in fs] == []


def record():
    """writes GOLDEN from the build in the tree"""
    import pathlib
    import tempfile
    out = {}
    for row in ROWS:
        with tempfile.TemporaryDirectory() as d:
            _, r = flow_abi.refused_run(pathlib.Path(d), ROWS, row)
            assert r.returncode == 1 and r.stderr.startswith("iS3D-amd: ") and r.stdout.count("\n") == 1, (row, r.returncode, r.stdout, r.stderr)
            out[row] = r.stderr
    with open(GOLDEN, "w") as f:
        json.dump(dict(stderr=out), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record()
