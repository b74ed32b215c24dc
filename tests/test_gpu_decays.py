"""GPU (-m gpu): the resonance decay feed-down (is3d_resonance_decays, is3d_decay_plan_*, the command line's do_resonance_decays = 1) against
the numpy restatement of the reference loop (tests/decays_restated.py), physics invariants that do not depend on it, the divergences of
DESIGN.md section 3h, and bitwise determinism."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import decays_restated as R
import refformat
from is3d_amd import api, inputs, synth

pytestmark = pytest.mark.gpu

G = inputs.grid()
PT, PHI, Y = G["pT"], G["phi"], G["y"]
GRID = dict(pT=PT, phi=PHI, y=Y)


def table(reference, name):
    return api.pdg_read_decays(os.path.join(reference, "PDG", name))


def thermal(reference, name, chosen, dim, seed):
    """a thermal spectrum of the chosen list from is3d_smooth_spectra over a synthetic surface"""
    pdg = api.pdg_read(os.path.join(reference, "PDG", name))
    ids = list(pdg["mc_id"])
    k = [ids.index(c) for c in chosen]
    sp = dict(mass=pdg["mass"][k], sign=pdg["sign"][k], degeneracy=pdg["gspin"][k], baryon=pdg["baryon"][k])
    cells = synth.synth_surface(48 if dim == 2 else 24, dim, seed=seed)
    g = dict(pT=PT, phi=PHI, y=Y, eta=G["eta"], eta_w=G["eta_w"])
    out, _ = api.smooth_spectra(cells, sp, g, inputs.df_tables(), dict(dimension=dim, df_mode=2))
    return np.asarray(out, dtype=np.float64)


def feed_err(got, ref, base, S):
    """worst |feed-down difference| relative to the largest feed-down of the same daughter"""
    dg, dr = (got - base).reshape(-1, S), (ref - base).reshape(-1, S)
    scale = np.max(np.abs(dr), axis=0)
    live = scale > 0
    return float(np.max(np.abs(dg - dr)[:, live] / scale[live])) if live.any() else 0.0


@pytest.fixture(scope="module")
def smash2d(reference):
    t = table(reference, "pdg_smash.dat")
    chosen = [int(x) for x in open(os.path.join(reference, "PDG", "chosen_particles_smash.dat")).read().split()]
    dN = thermal(reference, "pdg_smash.dat", chosen, 2, 611)
    return t, chosen, dN


def test_parity_2d_full_smash(smash2d):
    t, chosen, dN = smash2d
    got, st = api.resonance_decays(t, chosen, GRID, dN, dimension=2)
    rs = {}
    ref = R.feed_down(dN, t, chosen, PT, PHI, stats=rs)
    err = feed_err(got, ref, dN, len(chosen))
    print("2+1D smash (%d species): worst feed-down error %.3e; stats %s; restated %s" % (len(chosen), err, st, rs))
    assert st["n_parents"] == rs["n_parents"] and st["n_channels"] == rs["n_channels"] and st["n_adjusted"] == rs["n_adjusted"]
    assert st["n_clamps"] == rs["n_clamps"]
    assert np.isfinite(got).all() and (got >= dN).all() and (got > dN).any()
    assert err < 1e-10


def test_parity_3d_chain_and_3body(reference):
    # omega: 3-body pi+ pi0 pi-; phi -> rho0 pi0 feeds a parent (the chain); K* -> K pi
    chosen = [211, -211, 111, 321, -321, 311, 113, 223, 313, 333]
    t = table(reference, "pdg-urqmd_v3.3+.dat")
    dN = thermal(reference, "pdg-urqmd_v3.3+.dat", chosen, 3, 612)
    got, st = api.resonance_decays(t, chosen, GRID, dN, dimension=3)
    rs = {}
    ref = R.feed_down(dN, t, chosen, PT, PHI, y=Y, dim3=True, stats=rs)
    err = feed_err(got, ref, dN, len(chosen))
    print("3+1D reduced urqmd list: worst feed-down error %.3e; stats %s" % (err, st))
    assert st["n_parents"] == rs["n_parents"] == 4 and st["n_channels"] == rs["n_channels"]
    assert err < 1e-10
    # the chain: rho0's row grew before rho0 was processed, and pi+ got more in all than rho0 alone gives it (bin by bin the log-linear
    # interpolation of a larger parent need not be larger everywhere in the tails)
    rho_only = R.feed_down(dN.reshape(-1, 10)[:, [0, 1, 2, 6]].reshape(-1), t, [211, -211, 111, 113], PT, PHI, y=Y, dim3=True)
    assert (got.reshape(-1, 10)[:, 6] > dN.reshape(-1, 10)[:, 6]).any()
    assert got.reshape(-1, 10)[:, 0].sum() > rho_only.reshape(-1, 4)[:, 0].sum()


def _exp_spectrum(masses, T=0.15, v2=0.0):
    mT = np.sqrt(PT[None, :] ** 2 + np.asarray(masses)[:, None] ** 2)       # [S][pT]
    a = np.exp(-mT / T)[None, :, :] * (1.0 + v2 * np.cos(2.0 * PHI))[:, None, None]
    return np.ascontiguousarray(np.transpose(a, (0, 2, 1))).reshape(-1)     # [phi][pT][S]


def test_phi_independent_parent(smash2d):
    t, chosen, _ = smash2d
    ids = list(t["mc_id"])
    dN = _exp_spectrum([t["mass"][ids.index(c)] for c in chosen])
    got, _ = api.resonance_decays(t, chosen, GRID, dN, dimension=2)
    d = got.reshape(len(PHI), len(PT), len(chosen))
    spread = np.max(np.abs(d - d[0:1]) / np.abs(d[0:1]))
    print("phi-independent parents: max relative spread over phi %.3e" % spread)
    assert spread < 1e-12


SINGLE = dict(mc_id=np.array([111, 9000]), mass=np.array([0.13498, 0.77]), width=np.array([0.0, 0.15]), stable=np.array([1, 0], np.int32),
              n_channels=np.array([1, 1], np.int32), npart=np.array([1, 2], np.int32), branch_ratio=np.array([1.0, 1.0]),
              daughters=np.array([[111, 0, 0, 0, 0], [111, 111, 0, 0, 0]]))


@pytest.mark.parametrize("T", [0.15, 0.3])
def test_two_body_conserves_yield(T):
    """X -> pi0 pi0 with branch ratio 1: the pi0's added dN/dy is 2 x X's dN/dy.  Tolerance 5e-4: the 12 x 12 Gauss-Legendre (v, zeta)
    rule and the daughter's 32-node pT grid integrate to ~7e-5 (T = 0.15) and ~4e-6 (T = 0.3); the rest is margin."""
    dN = _exp_spectrum([0.13498, 0.77], T)
    dN.reshape(-1, 2)[:, 0] = 0.0
    got, _ = api.resonance_decays(SINGLE, [111, 9000], GRID, dN, dimension=2)
    dy = lambda a: float(np.einsum("j,i,ji->", G["phi_w"], G["pT_w"], a.reshape(len(PHI), len(PT))))  # noqa: E731
    r = dy(got.reshape(-1, 2)[:, 0]) / (2.0 * dy(dN.reshape(-1, 2)[:, 1])) - 1.0
    print("T = %.2f: pi0 dN/dy / (2 X dN/dy) - 1 = %.3e" % (T, r))
    assert abs(r) < 5e-4


def test_recoil_mass_is_the_partner(reference):
    """divergence 3: K*0 -> K+ pi-: the pi- group's recoil is the kaon (the reference takes particle_2, the pion itself)"""
    t = table(reference, "pdg-urqmd_v3.3+.dat")
    chosen = [-211, 321, 313]
    dN = _exp_spectrum([0.13957, 0.49368, 0.8961])
    dN.reshape(-1, 3)[:, :2] = 0.0
    got, _ = api.resonance_decays(t, chosen, GRID, dN, dimension=2)
    partner = R.feed_down(dN, t, chosen, PT, PHI)
    particle_2 = R.feed_down(dN, t, chosen, PT, PHI, recoil="particle_2")
    e_ok, e_p2 = feed_err(got, partner, dN, 3), feed_err(got, particle_2, dN, 3)
    print("K* -> K pi: vs partner mass %.3e, vs particle_2 mass %.3e" % (e_ok, e_p2))
    assert e_ok < 1e-10 and e_p2 > 1e-3


def _rho_case():
    chosen = [211, -211, 111, 113]
    dN = _exp_spectrum([0.13957, 0.13957, 0.13498, 0.7755], v2=0.2)
    dN.reshape(-1, 4)[:, :3] = 0.0
    return chosen, dN


def test_nonpositive_tail_gives_finite_output(reference):
    """divergence 2: rows of the parent that turn non-positive at high pT; the switch point keeps the bilinear branch off their logs"""
    t = table(reference, "pdg-urqmd_v3.3+.dat")
    chosen, dN = _rho_case()
    d = dN.reshape(len(PHI), len(PT), 4)
    d[3, 25:, 3] = -1e-30
    d[7, 27:, 3] = 0.0
    got, _ = api.resonance_decays(t, chosen, GRID, dN, dimension=2)
    ref = R.feed_down(dN, t, chosen, PT, PHI)
    assert np.isfinite(got).all()
    assert feed_err(got, ref, dN, 4) < 1e-10


def test_too_few_fit_points_names_the_parent(reference):
    """divergence 5: a (y, phi) row with one positive value is IS3D_EDOMAIN naming the parent and the row (the reference exits)"""
    t = table(reference, "pdg-urqmd_v3.3+.dat")
    chosen, dN = _rho_case()
    dN.reshape(len(PHI), len(PT), 4)[2, 1:, 3] = 0.0
    with pytest.raises(api.Is3dError) as e:
        api.resonance_decays(t, chosen, GRID, dN, dimension=2)
    assert e.value.code == api.IS3D_EDOMAIN and "parent 113" in str(e.value) and "iphi = 2" in str(e.value)
    with pytest.raises(R.FitError):
        R.feed_down(dN, t, chosen, PT, PHI)


def test_bitwise_repeat_and_plan(smash2d):
    import torch
    t, chosen, dN = smash2d
    a, _ = api.resonance_decays(t, chosen, GRID, dN, dimension=2)
    b, _ = api.resonance_decays(t, chosen, GRID, dN, dimension=2)
    assert a.tobytes() == b.tobytes()
    plan = api.DecayPlan(t, chosen, GRID, dimension=2, device=0)
    assert plan.output_size == dN.size
    d = torch.from_numpy(dN.copy()).to("cuda:0")
    st = plan.execute(d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert d.cpu().numpy().tobytes() == a.tobytes()
    d2 = torch.from_numpy(dN.copy()).to("cuda:0")
    plan.execute(d2.data_ptr(), torch.cuda.current_stream().cuda_stream, want_stats=False)
    torch.cuda.synchronize()
    assert d2.cpu().numpy().tobytes() == a.tobytes()
    print("plan stats", st)
    plan.close()


class RunResult(C.Structure):
    _fields_ = [("operation", C.c_int32), ("n_events", C.c_int32), ("n_species", C.c_int32), ("reserved", C.c_int32), ("n_particles", C.c_int64),
                ("particles", C.c_void_p), ("mc_id", C.POINTER(C.c_int64)), ("mass", C.POINTER(C.c_double)), ("n_spectrum", C.c_int64),
                ("spectrum", C.POINTER(C.c_double))]


def _tree(root):
    out = {}
    for d, _, files in os.walk(os.path.join(root, "results")):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_cli_end_to_end(tmp_path, reference):
    chosen = [211, -211, 111, 321, -321, 2212, -2212, 113, 223, 313, 323, 2214, 3122, 3212]
    cells = synth.synth_surface(9, 2, seed=613)
    roots = []
    for k, key in enumerate((False, True, False)):
        root = refformat.make_run_dir(str(tmp_path / ("r%d" % k)), cells, chosen, dict(dimension=2, df_mode=2, hrg_eos=2))
        shutil.copy(os.path.join(reference, "PDG", "pdg_smash.dat"), os.path.join(root, "PDG", "pdg_smash.dat"))
        if key:
            with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
                f.write("do_resonance_decays\t= 1\n")
        roots.append(root)
    for root in roots[:2]:
        r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout[-600:])
    plain, fed = _tree(roots[0]), _tree(roots[1])
    extra = {"results/dN_pTdpTdphidy_resonance_decays.dat", "results/dN_dpTdphidy_resonance_decays.dat"}
    assert set(fed) == set(plain) | extra
    for k in plain:
        assert fed[k] == plain[k], k
    # the library on the thermal spectrum of the same run (the embedding entry's result), written by is3d_write_results_decays
    L = api.load()
    L.is3d_run_particlization.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RunResult)]
    res = RunResult()
    cwd = os.getcwd()
    os.chdir(roots[2])
    try:
        assert L.is3d_run_particlization(None, None, None, 0, C.byref(res)) == 0
    finally:
        os.chdir(cwd)
    spec = np.ctypeslib.as_array(res.spectrum, shape=(res.n_spectrum,)).copy()
    L.is3d_run_result_free(C.byref(res))
    t = table(reference, "pdg_smash.dat")
    got, _ = api.resonance_decays(t, chosen, GRID, spec, dimension=2)
    out = tmp_path / "lib"
    out.mkdir()
    api.write_results_decays(str(out), 2, PT, PHI, None, got)
    for name in extra:
        assert open(out / os.path.basename(name), "rb").read() == fed[name], name
