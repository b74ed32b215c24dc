"""GPU (-m gpu): the run driver with the optional key test_sampler_fused = 1 (operation = 2, test_sampler = 1, viscous hydro) -- every hadron
binned where it is sampled, no particle list -- against the same run with test_sampler_on_device = 1, which fills and bins a list per event
batch: one 3+1D run and one at the reference's shipped shape (2+1D, df_mode 4, fast = 1, oversampled); a spelled-out device list; the
refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refformat
from is3d_amd import api, synth

pytestmark = pytest.mark.gpu
IDS = [211, 321, 2212]
KEY = "test_sampler_fused"
SHAPES = {
    "3d": (dict(operation=2, dimension=3, df_mode=2, test_sampler=1, oversample=1, min_num_hadrons=20000, sampler_seed=11, hrg_eos=2), 3, 2000),
    "shipped-2d": (dict(operation=2, dimension=2, df_mode=4, fast=1, test_sampler=1, oversample=1, min_num_hadrons=20000, sampler_seed=5, hrg_eos=2), 2, 4000),
}


def run_dir(tmp_path, name, shape, keys, params=None):
    p, dim, n = SHAPES[shape]
    root = refformat.make_run_dir(str(tmp_path / name), synth.synth_surface(n, dim, seed=97), IDS, dict(p, **(params or {})))
    with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:       # the template of make_run_dir has no line for an optional key
        for k, v in keys:
            f.write("%s\t\t= %d\n" % (k, v))
    return root


def run(root, devices=None):
    env = dict(os.environ)
    env.pop("IS3D_DEVICES", None)
    if devices:
        env["IS3D_DEVICES"] = devices
    return subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600, env=env)


def result_files(root):
    found = {}
    for d, _, names in os.walk(os.path.join(root, "results")):
        for n in names:
            path = os.path.join(d, n)
            found[os.path.relpath(path, root)] = open(path, "rb").read()
    return found


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cli_fused_writes_the_files_of_the_on_device_run(tmp_path, shape):
    binned, fused = run_dir(tmp_path, "binned", shape, (("test_sampler_on_device", 1),)), run_dir(tmp_path, "fused", shape, ((KEY, 1),))
    rb, rf = run(binned), run(fused)
    assert rb.returncode == 0, rb.stdout[-3000:] + rb.stderr[-3000:]
    assert rf.returncode == 0, rf.stdout[-3000:] + rf.stderr[-3000:]
    a, b = result_files(binned), result_files(fused)
    assert sorted(a) == sorted(b) and len(a) == 7 * 3 + 2
    n_vn = 0
    for name in a:
        if name.startswith(os.path.join("results", "vn") + os.sep):
            va, vb = np.loadtxt(os.path.join(binned, name)), np.loadtxt(os.path.join(fused, name))
            print(shape, name, "identical" if a[name] == b[name] else "max |delta| %.3e" % np.abs(va - vb).max())
            assert va.shape == vb.shape and np.allclose(vb, va, atol=1e-9, rtol=2e-6), name       # the fixed point (tests/test_gpu_cli_sampler_bins.py)
            n_vn += 1
        else:
            assert a[name] == b[name], name
    assert n_vn == 3
    assert not os.path.exists(os.path.join(fused, "results", "particle_list_osc.dat"))
    # one sampling pass, the lines of the on-device run, the time of the fused passes
    assert "ms_bin" in rf.stdout and "no particle workspace" in rf.stdout
    line = [ln for ln in rf.stdout.splitlines() if ln.startswith("particles: ")]
    assert len(line) == 1 and line == [ln for ln in rb.stdout.splitlines() if ln.startswith("particles: ")]
    assert int(line[0].split()[1]) > 1000
    sized = [ln for ln in rf.stdout.splitlines() if ln.startswith("Sampling ") and "event(s)" in ln]
    assert len(sized) == 1 and sized == [ln for ln in rb.stdout.splitlines() if ln.startswith("Sampling ") and "event(s)" in ln]
    for want in ("Total particle yield", "Momentum sampling efficiency", "Writing the binned sampler test distributions...", "device time: prep",
                 "Done sampling particles."):
        assert want in rb.stdout and want in rf.stdout, want
    if shape == "3d":
        # test_sampler_on_device = 1 beside the key, and a spelled-out device list (two cell shards): the same integer histograms, the same bytes
        both = run_dir(tmp_path, "both", shape, (("test_sampler_on_device", 1), (KEY, 1)))
        r2 = run(both, "0,0")
        assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
        assert result_files(both) == b and "no particle workspace" in r2.stdout
        # the key set to 0 is the run without it
        zero = run_dir(tmp_path, "zero", shape, (("test_sampler_on_device", 1), (KEY, 0)))
        rz = run(zero)
        assert rz.returncode == 0 and "particle workspace" in rz.stdout and "no particle workspace" not in rz.stdout
        assert result_files(zero) == a


@pytest.mark.parametrize("params", [dict(operation=1), dict(test_sampler=0), dict(mode=2, df_mode=4)], ids=["operation-1", "test_sampler-0", "mode-2"])
def test_refusals_name_the_key_and_write_nothing(tmp_path, params):
    root = run_dir(tmp_path, "refused", "3d", ((KEY, 1),), params)
    r = run(root)
    assert r.returncode != 0 and KEY + " = 1" in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert result_files(root) == {}


def test_the_embedding_entry_refuses_the_key(tmp_path):
    """is3d_run_particlization returns the particle list, which this route never holds"""
    root = run_dir(tmp_path, "embedded", "3d", ((KEY, 1),))
    L = api.load()
    L.is3d_run_particlization.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    res = (C.c_char * 256)()                                  # an is3d_run_result: the refusal comes before anything is stored in it
    cwd = os.getcwd()
    os.chdir(root)
    try:
        rc = L.is3d_run_particlization(None, None, None, 0, C.byref(res))
    finally:
        os.chdir(cwd)
    assert rc != 0 and KEY + " = 1" in L.is3d_last_error().decode() and "embedding" in L.is3d_last_error().decode()
    assert result_files(root) == {}
