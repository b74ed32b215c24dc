"""CPU: operation 0's writer (is3d_write_spacetime) against a Python restatement of calculate_dN_dX's file output
(emissionfunction_smooth_kernels.cpp:1100-1127, :1403-1434), and the argument checks of the operation-0 entries, which run before any
device use."""
import math
import os

import numpy as np
import pytest

from is3d_amd import api, synth

BINS = dict(tau_min=0.5, tau_max=6.5, tau_bins=4, r_min=0.0, r_max=9.0, r_bins=3)


def restate(bins, mc_id, eta_values, res):
    """file name -> text, as the reference's streams (setprecision(6) << scientific == %.6e)."""
    tb, rb = bins["tau_bins"], bins["r_bins"]
    tw = (bins["tau_max"] - bins["tau_min"]) / tb
    rw = (bins["r_max"] - bins["r_min"]) / rb
    files = {}
    n_eta = len(eta_values)
    for ip, mc in enumerate(mc_id):
        ft, fr, ftr, fe = [], [], [], []
        for ir in range(rb):
            r_mid = bins["r_min"] + rw * (ir + 0.5)
            fr.append("%.6e\t%.6e\n" % (r_mid, res["dN_twopirdrdy"][ip, ir] / (2.0 * math.pi * r_mid * rw)))
            for it in range(tb):   # r outer, tau inner: written inside the r loop
                tau_mid = bins["tau_min"] + tw * (it + 0.5)
                ftr.append("%.6e\t%.6e\t%.6e\n" % (tau_mid, r_mid, res["dN_twopitaurdtaudrdy"][ip, it, ir] / (2.0 * math.pi * tau_mid * r_mid * tw * rw)))
        for it in range(tb):
            tau_mid = bins["tau_min"] + tw * (it + 0.5)
            ft.append("%.6e\t%.6e\n" % (tau_mid, res["dN_taudtaudy"][ip, it] / (tau_mid * tw)))
        for k in range(n_eta):
            fe.append("%.6e\t%.6e\n" % (eta_values[k], res["dN_dydeta"][ip, k]))
        files["dN_taudtaudy_%d.dat" % mc] = "".join(ft)
        files["dN_twopirdrdy_%d.dat" % mc] = "".join(fr)
        files["dN_twopitaurdtaudrdy_%d.dat" % mc] = "".join(ftr)
        files["dN_dydeta_%d_%dpt.dat" % (mc, n_eta)] = "".join(fe)
    return files


@pytest.mark.parametrize("n_eta", [1, 5])
def test_writer_bytes_equal_the_restatement(tmp_path, n_eta):
    rng = np.random.default_rng(7 + n_eta)
    mc_id = [211, -2212, 3122]
    S, tb, rb = len(mc_id), BINS["tau_bins"], BINS["r_bins"]
    res = dict(dN_taudtaudy=rng.uniform(-1, 5, (S, tb)), dN_twopirdrdy=rng.uniform(0, 3e3, (S, rb)),
               dN_twopitaurdtaudrdy=rng.uniform(0, 1e-3, (S, tb, rb)), dN_dydeta=rng.uniform(0, 40, (S, n_eta)))
    res["dN_taudtaudy"][1, 2] = 0.0   # an empty bin
    res["dN_twopitaurdtaudrdy"][0, 3, 1] = 0.0
    eta = np.linspace(-2.0, 2.0, n_eta) if n_eta > 1 else np.array([0.731])
    api.write_spacetime(str(tmp_path), BINS, mc_id, eta, res)
    want = restate(BINS, mc_id, eta, res)
    assert sorted(os.listdir(tmp_path)) == sorted(want)
    for name, text in want.items():
        assert open(os.path.join(tmp_path, name)).read() == text, name
    assert "0.000000e+00" in want["dN_taudtaudy_-2212.dat"]


def test_writer_missing_directory_is_eio(tmp_path):
    res = dict(dN_taudtaudy=np.zeros((1, 4)), dN_twopirdrdy=np.zeros((1, 3)), dN_twopitaurdtaudrdy=np.zeros((1, 4, 3)), dN_dydeta=np.zeros((1, 1)))
    with pytest.raises(api.Is3dError) as e:
        api.write_spacetime(str(tmp_path / "absent"), BINS, [211], [0.0], res)
    assert e.value.code == api.IS3D_EIO


def test_argument_checks_precede_device_use(fx):
    """df_mode 3 / 4, bins < 1, tau_max <= tau_min and NULL x or y are IS3D_EINVAL on a machine with or without a GPU."""
    cells = {k: v for k, v in synth.synth_surface(8, 3, seed=11).items() if k not in ("x", "y")}
    g = dict(fx["grid"], pT_w=fx["grid_w"]["pT_w"], phi_w=fx["grid_w"]["phi_w"])
    xy = dict(x=np.linspace(0.0, 3.0, 8), y=np.zeros(8))
    cases = [(dict(df_mode=3), BINS, xy), (dict(df_mode=4), BINS, xy), (dict(df_mode=1), dict(BINS, tau_bins=0), xy),
             (dict(df_mode=1), dict(BINS, r_bins=0), xy), (dict(df_mode=2), dict(BINS, tau_max=BINS["tau_min"]), xy),
             (dict(df_mode=2), dict(BINS, tau_max=0.1), xy), (dict(df_mode=1), BINS, dict(x=None, y=xy["y"])),
             (dict(df_mode=1), BINS, dict(x=xy["x"], y=None))]
    for opts, bins, pos in cases:
        with pytest.raises(api.Is3dError) as e:
            api.spacetime_distributions(cells, fx["pikp"], g, fx["df"], bins, dict(opts, dimension=3), x=pos["x"], y=pos["y"])
        assert e.value.code == api.IS3D_EINVAL, (opts, bins)
    with pytest.raises(api.Is3dError) as e:
        api.spacetime_distributions(cells, fx["pikp"], g, fx["df"], BINS, dict(df_mode=3), **xy)
    assert "calculate_dN_dX_feqmod" in str(e.value)
