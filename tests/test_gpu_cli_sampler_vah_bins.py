"""GPU (-m gpu): the run driver's anisotropic-hydro sampler (mode = 2, operation = 2, df_mode = 4, vah_sampler = 1, test_sampler = 1) with the
optional key vah_sampler_on_device = 1 -- sampled once, every hadron binned where it is sampled, no particle list -- against the same run
without the key, which bins the list on the host; the same with vah_oversample = 1 and over a spelled-out device list; the refusals."""
import os
import subprocess

import numpy as np
import pytest

import refformat
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu
IDS = [211, 321, 2212, -2212]
KEY = "vah_sampler_on_device"


def vah_run(tmp_path, name, dim, params=None, keys=(("vah_sampler", 1),)):
    """the run directory of tests/test_gpu_cli_sampler_vah.py with bulkPi * 0.02 (tests/test_gpu_cli_sampler_vah_oversample.py)"""
    cells = dict(synth.synth_vah_surface(37, dim, seed=70 + dim))
    for k in ("dat", "dax", "day", "dan"):
        cells[k] = 20.0 * cells[k]
    cells["bulkPi"] = 0.02 * cells["bulkPi"]
    vh = synth.synth_surface(3, dim)            # make_run_dir wants a mode-1 surface to write first; it is replaced below
    p = dict(operation=2, dimension=dim, df_mode=4, mode=2, sampler_seed=29, test_sampler=1)
    p.update(params or {})
    root = refformat.make_run_dir(str(tmp_path / name), vh, IDS, p)
    synth.write_surface_vah_dat(os.path.join(root, "input", "surface.dat"), cells)
    refformat.write_vah_df_tables(os.path.join(root, "deltaf_coefficients", "vah"), inputs.vah_df_tables())
    with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:       # the template of make_run_dir has no line for an optional key
        for k, val in keys:
            f.write("%s\t\t= %s\n" % (k, repr(val)))
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


def compare_runs(host_root, device_root, host_out, device_out):
    """every file outside vn/ byte for byte; vn/ to the tolerance tests/test_gpu_cli_sampler_bins.py holds the viscous path to"""
    a, b = result_files(host_root), result_files(device_root)
    assert sorted(a) == sorted(b) and len(a) == 7 * len(IDS) + 2
    n_vn = 0
    for name in a:
        if name.startswith(os.path.join("results", "vn") + os.sep):
            va, vb = np.loadtxt(os.path.join(host_root, name)), np.loadtxt(os.path.join(device_root, name))
            assert va.shape == vb.shape and np.allclose(vb, va, atol=1e-9, rtol=2e-6), name
            n_vn += 1
        else:
            assert a[name] == b[name], name
    assert n_vn == len(IDS)
    assert not os.path.exists(os.path.join(device_root, "results", "particle_list_osc.dat"))
    # one sampling pass, the lines of the host-binned run plus the binning time
    assert "ms_bin" in device_out and "ms_bin" not in host_out
    assert device_out.count("Sampling particles from vahydro (P_L matching) with df...") == 1
    line = [ln for ln in device_out.splitlines() if ln.startswith("particles: ")]
    assert len(line) == 1 and line == [ln for ln in host_out.splitlines() if ln.startswith("particles: ")]
    assert int(line[0].split()[1]) > 1000
    for want in ("Sampling ", "Momentum sampling efficiency", "Writing the binned sampler test distributions...", "device time: prep",
                 "Done sampling particles."):
        assert want in host_out and want in device_out, want
    return a


@pytest.mark.parametrize("dim", [3, 2])
def test_cli_bins_the_vah_sampler_on_the_device_and_writes_the_same_files(tmp_path, dim):
    host, device = vah_run(tmp_path, "host", dim), vah_run(tmp_path, "device", dim, keys=(("vah_sampler", 1), (KEY, 1)))
    rh, rd = run(host), run(device)
    assert rh.returncode == 0, rh.stdout[-3000:] + rh.stderr[-3000:]
    assert rd.returncode == 0, rd.stdout[-3000:] + rd.stderr[-3000:]
    files = compare_runs(host, device, rh.stdout, rd.stdout)
    if dim == 3:
        # a spelled-out device list shards the cells: the same integer histograms, so the same bytes, vn/ included
        listed = vah_run(tmp_path, "listed", dim, keys=(("vah_sampler", 1), (KEY, 1)))
        rl = run(listed, "0,0")
        assert rl.returncode == 0, rl.stdout[-3000:] + rl.stderr[-3000:]
        assert result_files(listed) == result_files(device)
        # the key set to 0 is the host-binned run
        zero = vah_run(tmp_path, "zero", dim, keys=(("vah_sampler", 1), (KEY, 0)))
        rz = run(zero)
        assert rz.returncode == 0 and "ms_bin" not in rz.stdout
        assert result_files(zero) == files


def test_cli_bins_on_the_device_with_the_oversampled_run(tmp_path):
    """vah_oversample = 1: the mean yield sizes both runs alike and reaches mean_yield.dat through both writers"""
    keys = (("vah_sampler", 1), ("vah_oversample", 1), ("min_num_hadrons", 2000.0))      # a few hadrons per event: some hundred events
    host, device = vah_run(tmp_path, "host", 3, keys=keys), vah_run(tmp_path, "device", 3, keys=keys + ((KEY, 1),))
    rh, rd = run(host), run(device)
    assert rh.returncode == 0, rh.stdout[-3000:] + rh.stderr[-3000:]
    assert rd.returncode == 0, rd.stdout[-3000:] + rd.stderr[-3000:]
    compare_runs(host, device, rh.stdout, rd.stdout)
    sized = [ln for ln in rd.stdout.splitlines() if ln.startswith("Sampling ") and "event(s)" in ln]
    assert len(sized) == 1 and sized == [ln for ln in rh.stdout.splitlines() if ln.startswith("Sampling ") and "event(s)" in ln]
    assert 1 < int(sized[0].split()[1]) < 1000 and "Total particle yield: " in rd.stdout


@pytest.mark.parametrize("params,keys", [
    (dict(test_sampler=0), (("vah_sampler", 1), (KEY, 1))),
    ({}, (("vah_sampler", 0), (KEY, 1))),
    ({}, ((KEY, 1),)),
    (dict(mode=1), (("vah_sampler", 1), (KEY, 1))),
    (dict(operation=1), (("vah_sampler", 1), (KEY, 1))),
], ids=["test_sampler-0", "vah_sampler-0", "no-vah_sampler", "mode-1", "operation-1"])
def test_refusals_name_the_key_and_write_nothing(tmp_path, params, keys):
    root = vah_run(tmp_path, "refused", 3, params, keys)
    r = run(root)
    assert r.returncode != 0 and KEY + " = 1" in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert result_files(root) == {}
    assert not os.path.exists(os.path.join(root, "average_thermodynamic_quantities.dat"))
