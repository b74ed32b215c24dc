"""GPU (-m gpu): the command line run of the shipped default shape (operation = 2, test_sampler = 1) with the optional key
test_sampler_on_device = 1 -- sampled once, binned on the device, no particle list -- against the same run without the key."""
import os
import subprocess

import numpy as np
import pytest

import refformat
from is3d_amd import api, synth

pytestmark = pytest.mark.gpu
IDS = [211, 321, 2212]
PARAMS = dict(operation=2, dimension=2, df_mode=4, fast=1, test_sampler=1, oversample=1, min_num_hadrons=20000, sampler_seed=5, hrg_eos=2)


def run_dir(tmp_path, name, params, on_device):
    root = refformat.make_run_dir(str(tmp_path / name), synth.synth_surface(4000, 2, seed=97), IDS, params)
    if on_device is not None:       # the template of make_run_dir has no line for an optional key
        with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
            f.write("test_sampler_on_device\t\t= %d\n" % on_device)
    return root


def result_files(root):
    found = {}
    for d, _, names in os.walk(os.path.join(root, "results")):
        for n in names:
            path = os.path.join(d, n)
            found[os.path.relpath(path, root)] = open(path, "rb").read()
    return found


def test_cli_bins_on_the_device_and_writes_the_same_files(tmp_path):
    roots = [run_dir(tmp_path, "list", PARAMS, None), run_dir(tmp_path, "device", PARAMS, 1)]
    outs = []
    for root in roots:
        r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout)
    a, b = result_files(roots[0]), result_files(roots[1])
    assert sorted(a) == sorted(b) and len(a) == 7 * 3 + 2
    n_vn = 0
    for name in a:
        if name.startswith(os.path.join("results", "vn") + os.sep):
            va, vb = np.loadtxt(os.path.join(roots[0], name)), np.loadtxt(os.path.join(roots[1], name))
            assert va.shape == vb.shape and np.allclose(vb, va, atol=1e-9, rtol=2e-6), name
            n_vn += 1
        else:
            assert a[name] == b[name], name
    assert n_vn == 3
    # one sampling pass, the same lines as the list run plus the binning time
    assert "ms_bin" in outs[1] and "ms_bin" not in outs[0]
    assert outs[1].count("Sampling particles with Jonah's modified distribution...") == 1
    line = [ln for ln in outs[1].splitlines() if ln.startswith("particles: ")]
    assert len(line) == 1 and line == [ln for ln in outs[0].splitlines() if ln.startswith("particles: ")]
    for want in ("Momentum sampling efficiency", "Writing the binned sampler test distributions...", "device time: prep", "Done sampling particles."):
        assert want in outs[0] and want in outs[1], want
    assert not os.path.exists(os.path.join(roots[1], "results", "particle_list_osc.dat"))
    # the key set to 0 is today's run
    r0 = subprocess.run([api.CLI_PATH], cwd=run_dir(tmp_path, "zero", PARAMS, 0), capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0 and "ms_bin" not in r0.stdout
    assert result_files(str(tmp_path / "zero")) == a


def test_cli_refuses_the_key_without_test_sampler(tmp_path):
    root = run_dir(tmp_path, "refused", dict(PARAMS, test_sampler=0), 1)
    r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "test_sampler_on_device" in r.stdout + r.stderr and "test_sampler = 0" in r.stdout + r.stderr
    assert not os.path.exists(os.path.join(root, "results", "particle_list_osc.dat"))
