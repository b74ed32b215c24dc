"""CPU: the decayed-and-binned entries (is3d_decay_mc_table_create, is3d_decay_particles_binned, is3d_sampler_plan_execute_decayed_binned,
is3d_sample_decayed_binned) as far as they go without a device -- the exported symbols and the struct layout against the header, every
IS3D_EINVAL before any device use (is3d_resource_counters does not move), the answer without a device, and the run driver's refusals of
test_sampler_decayed with their exact texts (tests/golden/run_refusals_decayed.json; `python tests/test_decays_mc_bins_abi.py` records them
from the build in the tree), with the pinned texts of tests/golden/run_refusals.json unchanged when the new key is present too."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import decays_mc_cases as cases
import decays_mc_ref as ref
import test_run_refusals as base
from conftest import ROOT
from is3d_amd import api, inputs, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_refusals_decayed.json")
KEY = "test_sampler_decayed = 1"
ON = dict(operation=2, test_sampler=1)
BINS = dict(y_cut=1.2, y_bins=12, eta_cut=1.0, eta_bins=10, pT_lower_cut=0.1, pT_upper_cut=1.2, pT_bins=11, tau_min=0.5, tau_max=3.0, tau_bins=5,
            r_min=0.2, r_max=2.0, r_bins=6)
NEW = ["is3d_decay_mc_table_create", "is3d_decay_mc_table_destroy", "is3d_decay_particles_binned", "is3d_sampler_plan_execute_decayed_binned",
       "is3d_sample_decayed_binned"]

# id -> (parameters of refformat.make_run_dir, lines appended to iS3D_parameters.dat, keys removed), in the order parse_config makes them
ROWS = {
    "decayed-operation": (dict(operation=1, test_sampler=1), [KEY, "test_sampler_on_device = 0"], []),
    "decayed-test_sampler-0": (dict(operation=2), [KEY], []),
    "decayed-mode-2": (dict(base.VAH2, test_sampler=1), ["vah_sampler = 1", KEY], []),
    "decayed-on-device-0": (dict(ON), [KEY], []),
    "decayed-fused": (dict(ON), ["test_sampler_on_device = 1", "test_sampler_fused = 1", KEY], []),
    "decayed-box": (dict(ON, hrg_eos=3), ["test_sampler_on_device = 1", KEY], []),
    "decayed-missing-sampler-key": (dict(operation=2), [KEY], ["test_sampler"]),
    # two things wrong: the earlier check speaks
    "order-decayed-operation-before-on-device": (dict(operation=0, test_sampler=1), [KEY], []),
    "order-decayed-on-device-before-box": (dict(ON, hrg_eos=3), [KEY], []),
}


def refused_run(tmp_path, rows, row, extra=()):
    saved = base.ROWS
    params, lines, drop = rows[row]
    base.ROWS = {row: (params, list(lines) + list(extra), drop)}
    try:
        return base.refused_run(tmp_path, row)
    finally:
        base.ROWS = saved


@pytest.fixture(scope="module")
def tabs(reference):
    return cases.tables(api, reference)


def test_symbols_and_struct_layout_match_the_header(tmp_path):
    L = api.load()
    assert all(n in api.EXPORTS and hasattr(L, n) for n in NEW)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "is3d_amd.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   'sizeof(is3d_decay_mc_stats), offsetof(is3d_decay_mc_stats, ms_h2d), offsetof(is3d_decay_mc_stats, ms_d2h),'
                   'offsetof(is3d_decay_mc_stats, ms_bin));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = api.DecayMcStats
    assert c == [ctypes.sizeof(S), S.ms_h2d.offset, S.ms_d2h.offset, S.ms_bin.offset]
    assert S.ms_bin.offset + 8 == ctypes.sizeof(S)            # appended: every earlier field keeps its place


def test_every_refusal_precedes_device_use(tabs):
    t = tabs["pdg_smash.dat"]
    chosen = [211, -211, 113]
    q = ref.make_particles(api, t, chosen, [2, 0, 1], np.ones((3, 3)) * 0.2, events=[0, 1, 1])
    slot, ids = api.stable_slots(t, chosen)
    assert list(ids) == [211, -211]
    before = api.resource_counters()

    def refused(needle="", table=t, ch=chosen, particles=q, slot=slot, n_slots=2, bins=BINS, n_events=2):
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_binned(table, ch, particles, slot, n_slots, bins, n_events)
        assert e.value.code == api.IS3D_EINVAL and needle in str(e.value), str(e.value)

    # the refusals of is3d_decay_particles, with its messages
    for s in (-1, 3):
        bad = q.copy()
        bad["species"][1] = s
        refused("species", particles=bad)
    refused("999999", ch=[211, 999999])
    first = np.concatenate([[0], np.cumsum(t["n_channels"])])
    rho = int(np.nonzero(t["mc_id"] == 113)[0][0])
    lost = dict(t, daughters=t["daughters"].copy())
    lost["daughters"][first[rho], 0] = 424242
    refused("424242", table=lost)
    six = dict(t, npart=t["npart"].copy())
    six["npart"][first[rho]] = -6
    refused("6 decay products", table=six)
    # the bins and kernel_form of is3d_sampler_bin_list_device
    for bad in (dict(y_bins=0), dict(pT_upper_cut=0.05), dict(tau_max=0.5), dict(kernel_form=3), dict(kernel_form=-1)):
        refused(bins=dict(BINS, **bad))
    refused("n_events", n_events=0)
    # its own: the slots, the events, a private form that cannot hold the block
    refused("n_slots", n_slots=0)
    for v in (-2, 2):
        bad = slot.copy()
        bad[5] = v
        refused("slot[5]", slot=bad)
    for ev in (-1, 2):
        bad = q.copy()
        bad["event"][2] = ev
        refused("event", particles=bad)
    all_slot, all_ids = api.stable_slots(t)
    big = dict(BINS, y_bins=50, eta_bins=70, pT_bins=100, tau_bins=120, r_bins=60, kernel_form=2)
    refused("do not fit", slot=all_slot, n_slots=len(all_ids), bins=big)
    # the table object makes the table's refusals at create
    for table, ch, needle in ((lost, chosen, "424242"), (six, chosen, "6 decay products"), (t, [211, 999999], "999999")):
        with pytest.raises(api.Is3dError) as e:
            api.DecayMcTable(table, ch)
        assert e.value.code == api.IS3D_EINVAL and needle in str(e.value)
    # the raw entry: NULL arguments, a NULL histogram array, a negative count
    L = api.load()
    ts, ch, _, keep = api._decay_pack(t, chosen, dict(pT=[1.0], phi=[0.0], y=[0.0]))
    inp, nf, nu = api.DecayMcInputs(1, 0, 0, -1), ctypes.c_int64(7), ctypes.c_int64(7)
    b = api._pack_bins(BINS)
    h, arrays = api._hist_arrays(BINS, 2, 2)
    V = ctypes.c_void_p
    L.is3d_decay_particles_binned.argtypes = [V, ctypes.c_int32, V, V, ctypes.c_int64, V, V, ctypes.c_int32, V, ctypes.c_int32, V, V, V, V]
    good = [ctypes.addressof(ts), 3, ch.ctypes.data, ctypes.addressof(inp), 3, q.ctypes.data, slot.ctypes.data, 2, ctypes.addressof(b), 2,
            ctypes.addressof(h), ctypes.addressof(nf), ctypes.addressof(nu), None]
    for k in (0, 2, 3, 5, 6, 8, 10, 11, 12):
        a = list(good)
        a[k] = None
        assert L.is3d_decay_particles_binned(*a) == api.IS3D_EINVAL, k
    a = list(good)
    a[4] = -1
    assert L.is3d_decay_particles_binned(*a) == api.IS3D_EINVAL
    h2, _ = api._hist_arrays(BINS, 2, 2)
    h2.vn_im = None
    a = list(good)
    a[10] = ctypes.addressof(h2)
    assert L.is3d_decay_particles_binned(*a) == api.IS3D_EINVAL
    L.is3d_decay_mc_table_create.argtypes = [V, V, ctypes.c_int32, V, ctypes.c_int32]
    handle = ctypes.c_void_p()
    for a in ([None, ctypes.addressof(ts), 3, ch.ctypes.data, -1], [ctypes.addressof(handle), None, 3, ch.ctypes.data, -1],
              [ctypes.addressof(handle), ctypes.addressof(ts), 3, None, -1], [ctypes.addressof(handle), ctypes.addressof(ts), 0, ch.ctypes.data, -1]):
        assert L.is3d_decay_mc_table_create(*a) == api.IS3D_EINVAL and not handle.value
    # the one-shot sampler entry: the table, the slots and the bins are refused before the plan exists
    cells = synth.synth_surface(3, 3, seed=1)
    sp, gla = inputs.species(chosen), inputs.feqmod_tables(0.15)
    for kw, tab, sl in ((dict(), lost, slot), (dict(n_slots=0), t, slot), (dict(bins=dict(BINS, r_bins=0)), t, slot), (dict(), t, np.full(len(slot), 7, np.int32))):
        with pytest.raises(api.Is3dError) as e:
            api.sample_decayed_binned(cells, sp, inputs.df_tables(), gla, kw.get("bins", BINS), tab, chosen, sl, kw.get("n_slots", 2),
                                      dict(dimension=3, df_mode=2), n_events=2)
        assert e.value.code == api.IS3D_EINVAL, str(e.value)
    assert api.resource_counters() == before
    # n_particles = 0: zero histograms, no launch, no device needed
    hist, st = api.decay_particles_binned(t, chosen, q[:0], slot, 2, BINS, 2)
    assert st["n_final"] == st["n_unbinned"] == 0 and all(not v.any() for v in hist.values()) and api.resource_counters() == before
    if L.is3d_device_count() == 0:
        L.is3d_decay_particles_binned.argtypes = [V, ctypes.c_int32, V, V, ctypes.c_int64, V, V, ctypes.c_int32, V, ctypes.c_int32, V, V, V, V]
        assert L.is3d_decay_particles_binned(*good) == api.IS3D_ENODEVICE
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles_binned(t, chosen, q, slot, 2, BINS, 2)
        assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value) and e.value.stats["n_final"] == 0
        with pytest.raises(api.Is3dError) as e:
            api.DecayMcTable(t, chosen)
        assert e.value.code == api.IS3D_ENODEVICE
        with pytest.raises(api.Is3dError) as e:
            api.sample_decayed_binned(cells, sp, inputs.df_tables(), gla, BINS, t, chosen, slot, 2, dict(dimension=3, df_mode=2), n_events=2)
        assert e.value.code == api.IS3D_ENODEVICE


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_the_rows_of_this_module(golden):
    assert sorted(golden["stderr"]) == sorted(ROWS)
    assert len(set(golden["stderr"].values())) == 8               # the six refusals the tool can reach (one of them at two operations) and the missing-key message
    for row, text in golden["stderr"].items():
        if row != "decayed-missing-sampler-key":
            assert "test_sampler_decayed = 1" in text and text.rstrip().endswith("set test_sampler_decayed = 0"), row


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
