"""CPU: every refusal the run driver (is3d_amd/csrc/is3d_run.cpp) makes from the parameter file alone, through the command line tool.  A refused
run touches no device, so it ends the same way on a machine without one: exit status 1, one banner line on stdout, the message on stderr,
an empty results/ and no average_thermodynamic_quantities.dat.  One row per refusal the tool can reach (the four that need the embedding
entry stay with their GPU tests), a missing required key, a line without "=", and doubly-wrong files that pin which message comes first.
No row here is an accepted run.

tests/golden/run_refusals.json holds each row's stderr as commit e664bc7 (before the driver was split into parse_config / load_inputs / one
routine per operation) printed it; `python tests/test_run_refusals.py` records it again from the build in the tree."""
import json
import os
import subprocess
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_refusals.json")
VAH2 = dict(mode=2, operation=2, df_mode=4)          # the anisotropic-hydro sampler's combination

# id -> (parameters of refformat.make_run_dir, lines appended to iS3D_parameters.dat, keys whose lines are removed from it)
ROWS = {
    # ---- one row per refusal, in the order parse_config makes them ----
    "operation": (dict(operation=3), [], []),
    "operation-0-feqmod": (dict(operation=0, df_mode=3), [], []),
    "resonance-decays-operation": (dict(operation=2), ["do_resonance_decays = 1"], []),
    "resonance-decays-box": (dict(hrg_eos=3), ["do_resonance_decays = 1"], []),
    "decay-sampled-operation": (dict(operation=1), ["decay_sampled_hadrons = 1"], []),
    "decay-sampled-box": (dict(operation=2, hrg_eos=3), ["decay_sampled_hadrons = 1"], []),
    "decay-sampled-test_sampler": (dict(operation=2, test_sampler=1), ["decay_sampled_hadrons = 1"], []),
    "on-device-operation": (dict(operation=1, test_sampler=1), ["test_sampler_on_device = 1"], []),
    "on-device-test_sampler-0": (dict(operation=2), ["test_sampler_on_device = 1"], []),
    "fused-operation": (dict(operation=0, test_sampler=1), ["test_sampler_fused = 1"], []),
    "fused-test_sampler-0": (dict(operation=2), ["test_sampler_fused = 1"], []),
    "fused-mode-2": (dict(VAH2, test_sampler=1), ["vah_sampler = 1", "test_sampler_fused = 1"], []),
    "vah_oversample": (dict(operation=2), ["vah_sampler = 1", "vah_oversample = 1"], []),
    "vah-on-device": (dict(VAH2), ["vah_sampler = 1", "vah_sampler_on_device = 1"], []),
    "vah-sampler-stub": (dict(VAH2), [], []),
    "on-device-mode-2": (dict(VAH2, test_sampler=1), ["vah_sampler = 1", "test_sampler_on_device = 1"], []),
    "oversample-mode-2": (dict(VAH2, oversample=1), ["vah_sampler = 1"], []),
    "mode-2-df_mode": (dict(mode=2, df_mode=2), [], []),
    "mode": (dict(mode=3), [], []),
    "df_mode": (dict(df_mode=5), [], []),
    "jonah-baryon": (dict(df_mode=4, include_baryon=1), [], []),
    "hrg_eos": ({}, ["hrg_eos = 4"], []),
    "deltaf_dir-empty": ({}, ["deltaf_dir = \t# nothing behind the sign"], []),
    # ---- the parameter file itself ----
    "missing-required-key": ({}, [], ["outflow"]),
    "missing-sampler-key": (dict(operation=2), ["decay_sampled_hadrons = 1"], ["test_sampler"]),
    "line-without-equals": ({}, ["an orphan line"], []),
    "line-without-equals-before-a-refusal": (dict(operation=3), ["an orphan line"], []),
    # ---- two things wrong: the earlier check speaks ----
    "order-feqmod-before-decays": (dict(operation=0, df_mode=3), ["do_resonance_decays = 1"], []),
    "order-operation-before-df_mode": (dict(operation=3, df_mode=5), [], []),
    "order-decays-before-decay-sampled": (dict(operation=2, test_sampler=1), ["do_resonance_decays = 1", "decay_sampled_hadrons = 1"], []),
    "order-decay-sampled-operation-before-box": (dict(operation=1, hrg_eos=3), ["decay_sampled_hadrons = 1"], []),
    "order-on-device-before-fused": (dict(operation=1), ["test_sampler_fused = 1", "test_sampler_on_device = 1"], []),
    "order-vah_oversample-before-vah-on-device": ({}, ["vah_sampler_on_device = 1", "vah_oversample = 1"], []),
    "order-stub-before-mode-2-df_mode": (dict(VAH2, df_mode=1), [], []),
    "order-mode-before-df_mode": (dict(mode=3, df_mode=5), [], []),
    "order-jonah-baryon-before-hrg_eos": (dict(df_mode=4, include_baryon=1), ["hrg_eos = 4"], []),
    "order-hrg_eos-before-deltaf_dir": ({}, ["hrg_eos = 0", "deltaf_dir ="], []),
    "order-missing-key-before-operation": (dict(operation=3), [], ["regulate_deltaf"]),
}


def refused_run(tmp_path, row):
    """the run directory of a row (a 3-cell surface, as tests/test_gpu_cli_sampler_vah.py::vah_run builds one) and the tool's run in it"""
    import refformat
    from is3d_amd import api, synth
    params, lines, drop = ROWS[row]
    root = refformat.make_run_dir(str(tmp_path / "run"), synth.synth_surface(3, 3, seed=1), [211], params)
    path = os.path.join(root, "iS3D_parameters.dat")
    with open(path) as f:
        kept = [ln for ln in f.read().split("\n") if ln.split("=")[0].strip().lower() not in drop]
    with open(path, "w") as f:       # the template of make_run_dir has no line for an optional key
        f.write("\n".join(kept) + "".join(ln + "\n" for ln in lines))
    env = dict(os.environ)
    env.pop("IS3D_DEVICES", None)
    return root, subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=120, env=env)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_the_rows_of_this_module(golden):
    assert sorted(golden["stderr"]) == sorted(ROWS)
    assert len(set(golden["stderr"].values())) >= 23 + 2          # the 23 refusals the tool can reach and the two faults of the file itself


@pytest.mark.parametrize("row", list(ROWS))
def test_refused_before_any_device_or_file(tmp_path, golden, row):
    from is3d_amd import api
    root, r = refused_run(tmp_path, row)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr == golden["stderr"][row]
    assert r.stdout == "iS3D-amd: MI355X-native smooth Cooper-Frye spectra (%s)\n" % api.load().is3d_version().decode()
    assert [f for _, _, fs in os.walk(os.path.join(root, "results")) for f in fs] == []
    assert not os.path.exists(os.path.join(root, "average_thermodynamic_quantities.dat"))


def record():
    """writes GOLDEN from the build in the tree (run it on the commit the file is to describe)"""
    import pathlib
    import tempfile
    out = {}
    for row in ROWS:
        with tempfile.TemporaryDirectory() as d:
            _, r = refused_run(pathlib.Path(d), row)
            assert r.returncode == 1 and r.stderr.startswith("iS3D-amd: ") and r.stdout.count("\n") == 1, (row, r.returncode, r.stdout, r.stderr)
            out[row] = r.stderr
    with open(GOLDEN, "w") as f:
        json.dump(dict(commit="e664bc7", stderr=out), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record()
