"""GPU: the run driver's mode 5 on the run's device list.  A list that was spelled out (IS3D_DEVICES = 0,0,0) shards the spin polarization
over it: results/S{t,x,y,n}.dat are byte for byte what the library's multi entry gives on that list.  IS3D_DEVICES = 0 is one shard, which is
the run without the variable: first device, one-shot."""
import os
import subprocess

import numpy as np

import pytest

import refformat
from is3d_amd import api, inputs
from test_gpu_polarization import CLI_IDS, mode5_run

pytestmark = pytest.mark.gpu

S_FILES = ("St.dat", "Sx.dat", "Sy.dat", "Sn.dat")
SPECTRA = ("dN_pTdpTdphidy.dat", "dN_dpTdphidy.dat")
SEL = dict(pT=[1, 6, 11, 16, 21], phi=[0, 5, 10, 15, 20], y=[2, 8, 12, 18])   # a grid of a few nodes: 5 x 5 x 4


def small_run(tmp_path, name, n=200):
    root, _, _ = mode5_run(tmp_path, name, n, dict(operation=1, set_FO_temperature=0))
    g = inputs.grid()
    t = os.path.join(root, "tables")
    refformat.write_table(os.path.join(t, "pT_gauss_legendre_table.dat"), g["pT"][SEL["pT"]], g["pT_w"][SEL["pT"]])
    refformat.write_table(os.path.join(t, "phi_gauss_legendre_table.dat"), g["phi"][SEL["phi"]], g["phi_w"][SEL["phi"]], leading_tab=True,
                          dangling_fragment=True)
    refformat.write_table(os.path.join(t, "y_trapezoid_table_21pt.dat"), g["y"][SEL["y"]], g["y_w"][SEL["y"]])
    return root


def run(root, devices=None):
    env = dict(os.environ)
    env.pop("IS3D_DEVICES", None)
    if devices:
        env["IS3D_DEVICES"] = devices
    r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def results(root, names):
    return {nm: open(os.path.join(root, "results", nm), "rb").read() for nm in names if os.path.exists(os.path.join(root, "results", nm))}


def expected_files(tmp_path, root, devices):
    """what api.write_polarization writes from the library's multi entry on the surface as the reader returns it"""
    surface = os.path.join(root, "input", "surface.dat")
    arrs, _, _ = api.surface_open(surface, mode=5, cache=0)
    w, _ = api.surface_vorticity(surface, cache=0)
    cells = {k: arrs[k] for k in api.CELL_FIELDS if arrs.get(k) is not None}
    pdg = api.pdg_read(os.path.join(root, "PDG", "pdg-urqmd_v3.3+.dat"))
    pos = [int(np.nonzero(pdg["mc_id"] == i)[0][0]) for i in CLI_IDS]
    sp = dict(mass=pdg["mass"][pos], sign=pdg["sign"][pos], degeneracy=pdg["gspin"][pos], baryon=pdg["baryon"][pos])
    g = inputs.grid()
    grid = dict(pT=g["pT"][SEL["pT"]], phi=g["phi"][SEL["phi"]], y=g["y"][SEL["y"]], eta=g["eta"], eta_w=g["eta_w"])
    with open(os.path.join(root, "average_thermodynamic_quantities.dat")) as f:
        T = float(f.readline())
    res = api.spin_polarization_multi(cells, w, sp, grid, T, dict(dimension=3), devices)
    d = tmp_path / "expected"
    d.mkdir()
    api.write_polarization(str(d), 3, grid["pT"], grid["phi"], grid["y"], res)
    return {nm: (d / nm).read_bytes() for nm in S_FILES}, res


def test_listed_devices_shard_the_polarization(tmp_path):
    root = small_run(tmp_path, "listed")
    r = run(root, "0,0,0")
    exp, res = expected_files(tmp_path, root, [0, 0, 0])
    assert len(res["shard_stats"]) == 3 and all(s["n_chunks"] >= 1 for s in res["shard_stats"])
    got = results(root, S_FILES)
    assert sorted(got) == sorted(S_FILES)
    for nm in S_FILES:
        assert len(exp[nm]) > 0 and got[nm] == exp[nm], nm
    assert "polarization: 3 shards; slowest shard's cells" in r.stdout
    assert "polarization: species classes evaluated:" in r.stdout   # the existing line is still printed


def test_one_listed_device_is_the_run_without_a_list(tmp_path):
    plain_root, one_root = small_run(tmp_path, "plain"), small_run(tmp_path, "one")
    plain, one = run(plain_root), run(one_root, "0")
    s_plain, s_one = results(plain_root, S_FILES), results(one_root, S_FILES)
    assert sorted(s_plain) == sorted(S_FILES) and s_plain == s_one
    assert "polarization: 1 shard;" in one.stdout and "shard" not in "".join(ln for ln in plain.stdout.splitlines() if ln.startswith("polarization"))
    f_plain, f_one = results(plain_root, SPECTRA), results(one_root, SPECTRA)
    assert sorted(f_plain) == sorted(f_one) and "dN_pTdpTdphidy.dat" in f_plain
    if api.load().is3d_device_count() == 1:   # (with more devices the plain run shards the spectra over all of them: another association)
        assert f_plain == f_one
