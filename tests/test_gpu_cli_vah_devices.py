"""GPU: the run driver's mode 2 (anisotropic hydro) on the run's device list.  A list that was spelled out (IS3D_DEVICES = 0,0,0) shards the cells
over it: every result file is byte for byte what api.write_results writes from the library's multi entry on that list.  Without a list the
first device computes alone and says nothing about devices; IS3D_DEVICES = 0 is one shard, which is that run."""
import os
import subprocess

import numpy as np
import pytest

import refformat
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu

IDS = [211, 321, 2212]
NAMED = ("dN_pTdpTdphidy.dat", "dN_pTdpTdphidy_321.dat", "dN_dy_2212.dat", os.path.join("vn_continuous", "vn_211.dat"))


def mode2_run(tmp_path, name, dim):
    """a mode-2 run directory, built as tests/test_gpu_cli.py::test_cli_mode2_anisotropic_hydro builds its own"""
    cells = synth.synth_vah_surface(19 if dim == 3 else 5, dim, seed=60 + dim)
    vh = synth.synth_surface(3, dim)            # make_run_dir wants a mode-1 surface to write first; it is replaced below
    root = refformat.make_run_dir(str(tmp_path / name), vh, IDS, dict(dimension=dim, df_mode=4, mode=2))
    synth.write_surface_vah_dat(os.path.join(root, "input", "surface.dat"), cells)
    refformat.write_vah_df_tables(os.path.join(root, "deltaf_coefficients", "vah"), inputs.vah_df_tables())
    return root


def run(root, devices=None):
    env = dict(os.environ)
    env.pop("IS3D_DEVICES", None)
    if devices:
        env["IS3D_DEVICES"] = devices
    r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def files_under(base):
    """every file under a results directory: relative path -> bytes"""
    out = {}
    for d, _, files in os.walk(base):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, base)] = open(p, "rb").read()
    return out


def results(root):
    return files_under(os.path.join(root, "results"))


def expected_files(tmp_path, root, dim, devices):
    """what api.write_results writes from the library's multi entry on the surface as the driver's reader returns it"""
    arrs, _, _ = api.surface_open(os.path.join(root, "input", "surface.dat"), mode=2, dimension=dim, cache=0)
    cells = {k: arrs[k] for k in api.VAH_FIELDS[:25]}
    tab = api.vah_df_read(os.path.join(root, "deltaf_coefficients", "vah"))
    pdg = api.pdg_read(os.path.join(root, "PDG", "pdg-urqmd_v3.3+.dat"))
    pos = [int(np.nonzero(pdg["mc_id"] == i)[0][0]) for i in IDS]
    sp = dict(mass=pdg["mass"][pos], sign=pdg["sign"][pos], degeneracy=pdg["gspin"][pos], baryon=pdg["baryon"][pos])
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    dN, st = api.smooth_spectra_vah_multi(cells, sp, grid, dict(dimension=dim), devices, tab=tab)
    d = tmp_path / "expected"
    for sub in sorted({os.path.dirname(nm) for nm in results(root)} - {""}):   # the directories the run wrote into
        (d / sub).mkdir(parents=True)
    d.mkdir(exist_ok=True)
    api.write_results(str(d), dim, IDS, g["pT"], g["pT_w"], g["phi"], g["phi_w"], g["y"], dN)
    return files_under(str(d)), st


@pytest.mark.parametrize("dim", [3, 2])
def test_a_run_without_a_list_is_the_first_device_alone(tmp_path, dim):
    plain_root, one_root = mode2_run(tmp_path, "plain", dim), mode2_run(tmp_path, "one", dim)
    plain, one = run(plain_root), run(one_root, "0")
    f_plain, f_one = results(plain_root), results(one_root)
    assert all(nm in f_plain and len(f_plain[nm]) > 0 for nm in NAMED)
    assert f_plain == f_one
    assert "devices:" not in plain.stdout and "vahydro" in plain.stdout
    assert "devices: 1 (cell-axis shards of ~" in one.stdout


@pytest.mark.parametrize("dim", [3, 2])
def test_listed_devices_shard_the_cells(tmp_path, dim):
    root = mode2_run(tmp_path, "listed", dim)
    r = run(root, "0,0,0")
    assert "devices: 3 (cell-axis shards of ~" in r.stdout and "shard-ordered device sum of the spectrum" in r.stdout
    exp, st = expected_files(tmp_path, root, dim, [0, 0, 0])
    assert len(st["shards"]) == 3 and all(t["n_wave_rows"] > 0 for t in st["shards"])
    got = results(root)
    assert all(nm in got and len(got[nm]) > 0 for nm in NAMED)
    assert sorted(got) == sorted(exp)
    for nm in sorted(exp):
        assert got[nm] == exp[nm], nm
