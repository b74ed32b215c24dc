"""CPU: the resonance-decay pieces that run on the host -- the decay-table reader (read_resonances_conventional in full), the 3-body Q factor,
the two writers of the fed-down spectra, the argument and device checks of the feed-down entries, and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import refformat
from is3d_amd import api, synth


def parse_conventional(path):
    """read_resonances_conventional (readindata.cpp:1440-1568) restated on a token stream: the entries and their channels, antibaryons
    synthesised with the daughter rule, the EOF entry dropped"""
    text = open(path).read()
    tok = text.split()
    ents = []
    i = 0
    while i < len(tok):
        dec = int(tok[i + 11])
        e = dict(id=int(tok[i]), m=float(tok[i + 2]), w=float(tok[i + 3]), b=int(tok[i + 5]), s=int(tok[i + 6]), q=int(tok[i + 10]), ch=[])
        for j in range(dec):
            k = i + 12 + 8 * j
            e["ch"].append((int(tok[k + 1]), float(tok[k + 2]), [int(x) for x in tok[k + 3:k + 8]]))
        e["stable"] = int(bool(e["ch"]) and e["ch"][0][0] == 1)
        i += 12 + 8 * dec
        ents.append(e)
        if e["b"] > 0:
            a = dict(e, id=-e["id"], b=-e["b"], s=-e["s"], q=-e["q"], ch=[])
            for npart, br, ds in e["ch"]:
                nd = []
                for d in ds:
                    if d == 0:
                        nd.append(0)
                        continue
                    f = next((x for x in ents if x["id"] == d), a)
                    nd.append(d if (f["b"] == 0 and f["q"] == 0 and f["s"] == 0) else -d)
                a["ch"].append((npart, br, nd))
            ents.append(a)
    if not text[-1:].isspace():
        ents.pop()
    return ents


@pytest.mark.parametrize("name,count", [("pdg-urqmd_v3.3+.dat", 327), ("pdg_smash.dat", 493)])
def test_reader_matches_independent_parse(reference, name, count):
    path = os.path.join(reference, "PDG", name)
    t = api.pdg_read_decays(path)
    ents = parse_conventional(path)
    assert len(t["mc_id"]) == len(ents) == count
    assert (t["mc_id"] == api.pdg_read(path)["mc_id"]).all()
    assert list(t["mc_id"]) == [e["id"] for e in ents]
    assert list(t["stable"]) == [e["stable"] for e in ents]
    assert np.array_equal(t["mass"], [e["m"] for e in ents]) and np.array_equal(t["width"], [e["w"] for e in ents])
    assert list(t["n_channels"]) == [len(e["ch"]) for e in ents]
    ch = [c for e in ents for c in e["ch"]]
    assert list(t["npart"]) == [c[0] for c in ch]
    assert np.array_equal(t["branch_ratio"], [c[1] for c in ch])
    assert t["daughters"].tolist() == [c[2] for c in ch]
    # the antibaryon rule on one channel: anti-Delta++ -> anti-p pi-  (the proton is negated, pi+ is charged: negated too)
    ids = list(t["mc_id"])
    off = np.concatenate([[0], np.cumsum(t["n_channels"])])
    a = ids.index(-2224)
    d = t["daughters"][off[a]]
    assert sorted(d[:2].tolist()) == [-2212, -211]
    # a daughter with baryon = charge = strangeness = 0 keeps its sign in every antibaryon channel: pi0 (111) stays 111, and some channel has one
    anti = [k for k, i in enumerate(ids) if i < 0]
    ds = np.concatenate([t["daughters"][off[k]:off[k + 1]].ravel() for k in anti])
    assert (ds == 111).any() and not (ds == -111).any()


def test_reader_refuses_malformed(tmp_path):
    p = tmp_path / "bad.dat"
    p.write_text("211 pi 0.138 0.0 1 0 0 0 0 3 1 1\n 211 1 1.0 211 0 0 0\n")   # truncated channel record
    with pytest.raises(api.Is3dError) as e:
        api.pdg_read_decays(str(p))
    assert e.value.code == api.IS3D_EIO
    p.write_text("211 pi 0.138 0.0 1 0 0 0 0 3 1 51\n")
    with pytest.raises(api.Is3dError) as e:
        api.pdg_read_decays(str(p))
    assert e.value.code == api.IS3D_EIO
    p.write_text("211 pi 0.138 0.0 1 0 0 0 0 3 1 1\n 211 6 1.0 211 0 0 0 0\n")   # 6 products
    with pytest.raises(api.Is3dError) as e:
        api.pdg_read_decays(str(p))
    assert e.value.code == api.IS3D_EIO


@pytest.mark.parametrize("masses", [(0.78265, 0.13957, 0.13957, 0.13498), (1.019, 0.13957, 0.13957, 0.13498), (1.4, 0.494, 0.2, 0.3)])
def test_q_factor_against_quad(masses):
    from scipy.integrate import quad
    M, m1, m2, m3 = masses
    a, b, c, d = (M + m1) ** 2, (M - m1) ** 2, (m2 + m3) ** 2, (m2 - m3) ** 2
    exact = quad(lambda s: np.sqrt(abs((a - s) * (b - s) * (s - c) * (s - d))) / s, c, b, epsabs=0, epsrel=1e-13, limit=200)[0]
    got = api.decay_q_factor(M, m1, m2, m3)
    # 24 Gauss-Legendre nodes on an integrand with square-root end points: accurate to ~1e-4 relative, not to rounding
    assert abs(got - exact) < 2e-4 * exact


def _render(dim, S, pT, phi, y, dN, times_pT):
    """the iostream text: scientific, setprecision(8), setw(5) (never pads a 14-character number)"""
    out = ["y\tphip\tpT\tdN_dpTdphidy\n"] if times_pT else []
    ny = 1 if dim == 2 else len(y)
    d = dN.reshape(ny, len(phi), len(pT), S)
    for s in range(S):
        for iy in range(ny):
            yv = 0.0 if dim == 2 else y[iy]
            for j, ph in enumerate(phi):
                for i, p in enumerate(pT):
                    v = d[iy, j, i, s] * (p if times_pT else 1.0)
                    out.append("%.8e\t%.8e\t%.8e\t%.8e\n" % (yv, ph, p, v))
                out.append("\n")
    return "".join(out)


@pytest.mark.parametrize("dim", [2, 3])
def test_writer_bytes(tmp_path, dim):
    rng = np.random.default_rng(3)
    S, pT, phi, y = 3, np.array([0.01, 0.5, 3.0, 40.0]), np.linspace(0.0, 6.0, 5), np.array([-5.0, 0.0, 2.5])
    n = S * len(pT) * len(phi) * (1 if dim == 2 else len(y))
    dN = rng.normal(size=n) * 10.0 ** rng.integers(-300, 30, size=n)
    dN[::11] = 0.0
    dN[5] = -0.0
    dN[7] = np.inf
    for _ in range(2):   # the files are appended to
        api.write_results_decays(str(tmp_path), dim, pT, phi, y if dim == 3 else None, dN)
    a = open(tmp_path / "dN_pTdpTdphidy_resonance_decays.dat").read()
    b = open(tmp_path / "dN_dpTdphidy_resonance_decays.dat").read()
    assert a == 2 * _render(dim, S, pT, phi, y, dN, False)
    assert b == 2 * _render(dim, S, pT, phi, y, dN, True)


def test_writer_missing_directory(tmp_path):
    with pytest.raises(api.Is3dError) as e:
        api.write_results_decays(str(tmp_path / "nope"), 2, [1.0], [0.0], None, [1.0])
    assert e.value.code == api.IS3D_EIO


def _small_table(reference):
    return api.pdg_read_decays(os.path.join(reference, "PDG", "pdg_smash.dat"))


GRID = dict(pT=np.linspace(0.1, 3.0, 8), phi=np.linspace(0.1, 6.1, 6), y=np.linspace(-2.0, 2.0, 5))


def test_argument_checks(reference):
    t = _small_table(reference)
    dN = np.ones(3 * 8 * 6)
    for bad, code in [(dict(chosen=[211]), api.IS3D_EINVAL), (dict(chosen=[211, -211, 999999]), api.IS3D_EINVAL),
                      (dict(grid=dict(GRID, pT=GRID["pT"][::-1])), api.IS3D_EDOMAIN), (dict(grid=dict(GRID, phi=GRID["phi"][::-1])), api.IS3D_EDOMAIN),
                      (dict(grid=dict(GRID, pT=np.r_[0.0, GRID["pT"][1:]])), api.IS3D_EDOMAIN), (dict(dimension=4), api.IS3D_EINVAL),
                      (dict(dimension=3, grid=dict(GRID, y=GRID["y"][::-1])), api.IS3D_EDOMAIN)]:
        a = dict(chosen=[211, -211, 113], grid=GRID, dimension=2)
        a.update(bad)
        with pytest.raises(api.Is3dError) as e:
            api.resonance_decays(t, a["chosen"], a["grid"], dN, dimension=a["dimension"])
        assert e.value.code == code, (bad, e.value)


def test_no_cpu_path(reference):
    """Without a HIP device both entries fail with IS3D_ENODEVICE after the argument checks; nothing is computed on the host."""
    if api.load().is3d_device_count() > 0:
        pytest.skip("a GPU is visible: covered by tests/test_gpu_decays.py")
    t = _small_table(reference)
    for call in (lambda: api.resonance_decays(t, [211, -211, 113], GRID, np.ones(3 * 8 * 6)),
                 lambda: api.DecayPlan(t, [211, -211, 113], GRID)):
        with pytest.raises(api.Is3dError) as e:
            call()
        assert e.value.code == api.IS3D_ENODEVICE
        assert "no CPU path" in str(e.value)


@pytest.mark.parametrize("params,why", [(dict(hrg_eos=3), "carries no decay data"), (dict(operation=0), "operation = 0"),
                                        (dict(operation=2), "operation = 2")])
def test_cli_refuses_resonance_decays(tmp_path, params, why):
    cells = synth.synth_surface(3, 3, seed=1)
    root = refformat.make_run_dir(str(tmp_path), cells, [211], params)
    with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
        f.write("do_resonance_decays\t= 1\n")
    r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "do_resonance_decays" in r.stderr and why in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(root, "results", "dN_pTdpTdphidy.dat"))
