"""GPU: is3d_df_generate (csrc/cf_dfgen.hip) -- the df-coefficient generator on the device -- against numbers the REFERENCE ITSELF holds.

The reference ships its generator's output for three hadron lists (deltaf_coefficients/vh/{urqmd, smash, smash_box}/*.dat, 81 x 101 rows x 10
tables each, printed `fixed` with six decimals); tests/test_oracle_dfcoef.py shows that the CPU restatement reproduces all of them digit for
digit.  Here the device kernel is held to the same printed digits and to the CPU restatement.

B(v) = 5.0e-7 + 1e-11 max(1, |v|): half a unit of the last printed decimal plus the project's device-against-oracle bound for this integrand
family (1e-11: test_total_yield_matches_the_oracle, the sampler momenta).  printed(v): "%.6f" with "-0.000000" read as "0.000000".

Baryon-odd integrals: N10, N30, N31, B10, nB and N20 carry one power of the baryon number and vanish at mu_B = 0 (baryon and antibaryon cancel);
the other integrals restricted to baryons (M20, M21, M10, M11) carry b^2 and do not."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import refformat
from is3d_amd import api, inputs, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = inputs.DF_NAMES_2D
ODD = [api.DFGEN_INTEGRALS.index(n) for n in ("N10", "N30", "N31", "B10", "nB", "N20")]
I_M10 = api.DFGEN_INTEGRALS.index("M10")
NOISE_AT_ZERO = [NAMES.index(n) for n in ("c1", "c4", "G")]          # ~ odd integrals: cancellation noise at mu_B = 0


def printed(v):
    s = "%.6f" % v
    return "0.000000" if s == "-0.000000" else s


def bound(v):
    return 5.0e-7 + 1e-11 * np.maximum(1.0, np.abs(v))


def pdg_urqmd():
    a = np.array(inputs.load_fixture()["pdg_urqmd"], dtype=np.float64)        # columns: mc_id, mass, gspin, baryon, sign
    return dict(mass=a[:, 1].copy(), gspin=a[:, 2].copy(), baryon=a[:, 3].copy(), sign=a[:, 4].copy())


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(HERE, "golden", "golden_dfcoef.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def gold_lists():
    z = np.load(os.path.join(HERE, "golden", "golden_dfcoef_lists.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def rows_device(gold):
    """the 15 x 23 fixture rows on the device, with the integrals"""
    tab, integ, st = api.df_generate(pdg_urqmd(), gold["root"], gold["weight"], gold["T"][gold["iT"]], gold["muB"][gold["iB"]], with_integrals=True)
    assert st["n_massive"] == 326
    return tab, integ


@pytest.fixture(scope="module")
def rows_oracle(gold):
    pdg = pdg_urqmd()
    tab, integ = np.zeros((10, 15, 23)), np.zeros((20, 15, 23))
    for jB, iB in enumerate(gold["iB"]):
        for jT, iT in enumerate(gold["iT"]):
            o, i = oracle.df_generator_row(pdg, gold["root"], gold["weight"], gold["T"][iT], gold["muB"][iB], with_integrals=True)
            tab[:, jB, jT], integ[:, jB, jT] = o, i
    return tab, integ


@pytest.fixture(scope="module")
def grid_device(gold):
    """the whole shipped 81 x 101 grid on the device"""
    full = inputs.df_tables_full()
    tab, _, st = api.df_generate(pdg_urqmd(), gold["root"], gold["weight"], full["T"], full["muB"])
    print("81 x 101 grid, urqmd list: kernel %.3f ms" % st["ms_kernel"])
    return tab


def text_mismatches(dev, text, T, B):
    bad = []
    for k in range(10):
        for jB in range(dev.shape[1]):
            for jT in range(dev.shape[2]):
                if printed(dev[k, jB, jT]) != printed(float(text[k, jB, jT])):
                    bad.append((NAMES[k], float(T[jT]), float(B[jB]), float(dev[k, jB, jT]), str(text[k, jB, jT])))
    return bad


def test_reference_held_digits_on_the_fixture_rows(gold, rows_device):
    """All 3 450 values print as the shipped text and lie within B of it."""
    dev = rows_device[0]
    assert gold["text"].shape == (10, 15, 23) and list(gold["names"]) == NAMES
    err = np.abs(dev - gold["shipped"])
    print("fixture rows: max |device - shipped| %.4e" % err.max())
    bad = text_mismatches(dev, gold["text"], gold["T"][gold["iT"]], gold["muB"][gold["iB"]])
    assert not bad, bad[:8]
    assert np.all(err <= bound(gold["shipped"])), float((err - bound(gold["shipped"])).max())


def test_device_against_the_cpu_restatement_on_the_fixture_rows(gold, rows_device, rows_oracle):
    """The ten outputs, and on rows with mu_B > 0 all 20 integrals, to 1e-11 relative; at mu_B = 0 the baryon-odd integrals are noise below
    1e-13 M10 and c1, c4, G (proportional to them) print 0.000000."""
    (dt, di), (ot, oi) = rows_device, rows_oracle
    B = gold["muB"][gold["iB"]]
    pos, zero = B > 0, B == 0
    assert zero.sum() == 1 and pos.sum() == 14
    with np.errstate(divide="ignore", invalid="ignore"):                                # exact zeros of the CPU restatement at mu_B = 0: left out below
        rel_t = np.abs(dt - ot) / np.abs(ot)
        rel_i = np.abs(di - oi) / np.abs(oi)
    worst_t = max(rel_t[:, pos].max(), np.delete(rel_t[:, zero], NOISE_AT_ZERO, axis=0).max())
    worst_i = max(rel_i[:, pos].max(), np.delete(rel_i[:, zero], ODD, axis=0).max())
    print("device vs CPU restatement: worst relative difference, outputs %.3e, integrals %.3e" % (worst_t, worst_i))
    for k in range(10):
        print("  %-8s %.3e" % (NAMES[k], rel_t[k][pos].max()))
    assert worst_t <= 1e-11 and worst_i <= 1e-11
    M10 = di[I_M10][zero]
    for i in ODD:
        assert np.all(np.abs(di[i][zero]) <= 1e-13 * M10), (api.DFGEN_INTEGRALS[i], di[i][zero], M10)
    for k in NOISE_AT_ZERO:
        assert all(printed(v) == "0.000000" for v in dt[k][zero].ravel()), NAMES[k]


def test_whole_shipped_grid(grid_device):
    """81 x 101 points against the shipped doubles: every value within B; the mu_B = 0 row print-exact; at most 8 of 81 810 values may print
    differently (boundary distances on the full grid go down to 1.9e-12 for betaV), each still within B."""
    full = inputs.df_tables_full()
    ship = np.array([full["2d"][n] for n in NAMES])
    assert ship.shape == grid_device.shape == (10, 81, 101) and full["muB"][0] == 0.0
    err = np.abs(grid_device - ship)
    print("whole grid: max |device - shipped| %.4e" % err.max())
    assert np.all(err <= bound(ship)), float((err - bound(ship)).max())
    row0 = np.array([[float(printed(v)) for v in grid_device[k, 0]] for k in range(10)])
    assert np.array_equal(row0, ship[:, 0, :]), np.argwhere(row0 != ship[:, 0, :])[:8]
    bad = text_mismatches(grid_device, ship, full["T"], full["muB"])
    print("whole grid: %d of %d values print differently" % (len(bad), ship.size))
    assert len(bad) <= 8, bad


@pytest.mark.parametrize("which", ["smash", "smash_box"])
def test_the_other_two_lists(which, gold, gold_lists):
    """smash (493 entries, with b = 2 bosons) and smash_box (400): printed digits and B on every 8th mu_B x every 10th T row."""
    g = gold_lists
    pdg = {k: g[which + "_" + k] for k in ("mass", "gspin", "baryon", "sign")}
    assert len(pdg["mass"]) == dict(smash=493, smash_box=400)[which]
    T, B = g["T"][g["iT"]], g["muB"][g["iB"]]
    dev, _, _ = api.df_generate(pdg, gold["root"], gold["weight"], T, B)
    ship = g[which + "_shipped"]
    err = np.abs(dev - ship)
    print("%s: max |device - shipped| %.4e" % (which, err.max()))
    bad = text_mismatches(dev, g[which + "_text"], T, B)
    assert not bad, bad[:8]
    assert np.all(err <= bound(ship))


def assert_matches_oracle(pdg, root, weight, T, B, tol=1e-11):
    dev, integ, _ = api.df_generate(pdg, root, weight, T, B, with_integrals=True)
    worst = 0.0
    for jB, b in enumerate(np.atleast_1d(B)):
        for jT, t in enumerate(np.atleast_1d(T)):
            o, i = oracle.df_generator_row(pdg, root, weight, t, b, with_integrals=True)
            worst = max(worst, np.max(np.abs(dev[:, jB, jT] - o) / np.abs(o)), np.max(np.abs(integ[:, jB, jT] - i) / np.abs(i)))
    print("worst relative difference %.3e" % worst)
    assert worst <= tol, worst
    return dev


OFF_T, OFF_B = np.array([0.30, 0.1234, 0.05]), np.array([0.0371, 0.4567])        # descending T, off the shipped grid, all mu_B > 0


def test_off_grid_points(gold):
    pdg = pdg_urqmd()
    assert_matches_oracle(pdg, gold["root"], gold["weight"], [0.1517], [0.2113])                    # 1 x 1
    assert_matches_oracle(pdg, gold["root"], gold["weight"], OFF_T, OFF_B)                          # 3 x 2


def test_list_shapes(gold):
    pdg = pdg_urqmd()
    T, B = [0.05, 0.1517], [0.2113]
    ib = int(np.argmax(pdg["baryon"] > 0))
    assert pdg["baryon"][ib + 1] == -pdg["baryon"][ib] and pdg["mass"][ib + 1] == pdg["mass"][ib]
    assert_matches_oracle({k: v[ib:ib + 2].copy() for k, v in pdg.items()}, gold["root"], gold["weight"], T, B)      # a baryon and its antibaryon
    assert_matches_oracle({k: v[:65].copy() for k, v in pdg.items()}, gold["root"], gold["weight"], T, B)             # 65 entries: 16 | 16 | 16 | 17 per wave
    assert pdg["mass"][0] == 0.0 and np.all(pdg["mass"][1:] > 0)
    last = assert_matches_oracle({k: np.roll(v, -1) for k, v in pdg.items()}, gold["root"], gold["weight"], T, B)     # 327 entries, the photon last
    assert np.all(np.isfinite(last))


@pytest.mark.parametrize("n_gla", [1, 32, 48, 63])
def test_truncated_rules(n_gla, gold):
    """Device and CPU restatement on the SAME nodes (the first n_gla of the fixture's rule): says nothing about the quadrature."""
    assert_matches_oracle(pdg_urqmd(), gold["root"][:, :n_gla], gold["weight"][:, :n_gla], [0.1517, 0.1], [0.2113])


def test_determinism(gold, grid_device):
    pdg, r, w = pdg_urqmd(), gold["root"], gold["weight"]
    a, ai, _ = api.df_generate(pdg, r, w, OFF_T, OFF_B, with_integrals=True)
    b, bi, _ = api.df_generate(pdg, r, w, OFF_T, OFF_B, with_integrals=True)
    assert a.tobytes() == b.tobytes() and ai.tobytes() == bi.tobytes()
    c, none, _ = api.df_generate(pdg, r, w, OFF_T, OFF_B)
    assert none is None and c.tobytes() == a.tobytes()                                  # integrals = NULL changes no bit
    for jB, mu in enumerate(OFF_B):
        for jT, t in enumerate(OFF_T):
            one, onei, _ = api.df_generate(pdg, r, w, [t], [mu], with_integrals=True)
            assert one[:, 0, 0].tobytes() == a[:, jB, jT].tobytes() and onei[:, 0, 0].tobytes() == ai[:, jB, jT].tobytes(), (t, mu)
    full = inputs.df_tables_full()
    for iB, iT in ((0, 0), (20, 17), (80, 100), (33, 64)):
        one, _, _ = api.df_generate(pdg, r, w, [full["T"][iT]], [full["muB"][iB]])
        assert one[:, 0, 0].tobytes() == grid_device[:, iB, iT].tobytes(), (iB, iT)


def test_refusals(gold):
    pdg, r, w = pdg_urqmd(), gold["root"], gold["weight"]
    mesons = {k: v[pdg["baryon"] == 0].copy() for k, v in pdg.items()}
    with pytest.raises(api.Is3dError) as e:
        api.df_generate(mesons, r, w, [0.14, 0.15], [0.1])
    assert e.value.code == api.IS3D_EDOMAIN and "diffusion" in str(e.value) and "T = 0.14, muB = 0.1" in str(e.value), str(e.value)
    # a boson with baryon * mu_B > mass: exp(E/T - b mu_B/T) - 1 < 0 at the low nodes
    bad = {k: v.copy() for k, v in pdg.items()}
    k = 40
    bad["baryon"][k], bad["sign"][k] = 2.0, -1.0
    muB = 0.75 * bad["mass"][k]
    assert 2.0 * muB > bad["mass"][k] > 0
    with pytest.raises(api.Is3dError) as e:
        api.df_generate(bad, r, w, [0.15], [muB])
    assert e.value.code == api.IS3D_EDOMAIN and "list entry %d " % k in str(e.value) and "f_eq is negative" in str(e.value), str(e.value)
    p0 = api.resource_counters()
    for kw in einval_cases(pdg, r, w):
        with pytest.raises(api.Is3dError) as e:
            api.df_generate(**kw)
        assert e.value.code == api.IS3D_EINVAL, kw
    assert api.resource_counters() == p0


def einval_cases(pdg, r, w):
    good = dict(pdg=pdg, root=r, weight=w, T=[0.15], muB=[0.1])
    nan = dict(pdg, mass=np.where(np.arange(len(pdg["mass"])) == 5, np.nan, pdg["mass"]))
    rinf = r.copy()
    rinf[2, 3] = np.inf
    return [dict(good, pdg={k: v[:0] for k, v in pdg.items()}), dict(good, root=r[:, :0], weight=w[:, :0]), dict(good, T=[0.15, 0.0]),
            dict(good, T=[-0.1]), dict(good, T=[np.nan]), dict(good, muB=[np.inf]), dict(good, pdg=nan), dict(good, root=rinf),
            dict(good, T=[]), dict(good, muB=[]), dict(good, device=-2)]


def write_gla_five_alpha(path, root, weight):
    with open(path, "w") as f:
        f.write("%d\t%d\n" % root.shape)
        for a in range(root.shape[0]):
            for rk, wk in zip(root[a], weight[a]):
                f.write("%d\t%s\t%s\n" % (a, repr(float(rk)), repr(float(wk))))


def test_driver_generates_and_a_run_reads_the_tables(tmp_path, gold):
    """iS3D_amd --generate-df out in a run directory, then a pi/K/p run with deltaf_dir = out against the same run on the shipped tables."""
    full = inputs.df_tables_full()
    ship = np.array([full["2d"][n] for n in NAMES])
    base = refformat.make_run_dir(str(tmp_path / "base"), synth.synth_surface(48, 3, seed=77), [211, 321, 2212], dict(dimension=3, df_mode=2))
    shipped_dir = os.path.join(base, "deltaf_coefficients", "vh", "urqmd")
    shutil.rmtree(shipped_dir)
    api.df_tables_write(shipped_dir, full["T"], full["muB"], ship)                       # the shipped files, from the fixture
    write_gla_five_alpha(os.path.join(base, "tables", "gla_roots_weights_64_points.txt"), gold["root"], gold["weight"])
    listed = api.pdg_read(os.path.join(base, "PDG", "pdg-urqmd_v3.3+.dat"))
    pdg = pdg_urqmd()
    assert all(np.array_equal(listed[k], pdg[k]) for k in pdg)

    r = subprocess.run([api.CLI_PATH, "--generate-df", "out"], cwd=base, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device time" in r.stdout and not os.listdir(os.path.join(base, "results", "dN_dy"))
    T = np.array([0.1] + [0.1 + i * ((0.2 - 0.1) / 100.0) for i in range(1, 101)])
    B = np.array([0.0] + [0.0 + i * ((0.8 - 0.0) / 80.0) for i in range(1, 81)])
    dev, _, _ = api.df_generate(pdg, gold["root"], gold["weight"], T, B)
    for k, n in enumerate(NAMES):
        Tf, Bf, v = api.df_table_read_full(os.path.join(base, "out", n + ".dat"))
        assert np.array_equal(Tf, full["T"]) and np.array_equal(Bf, full["muB"])
        want = np.array([float("%.6f" % x) for x in dev[k].ravel()]).reshape(81, 101)
        assert np.array_equal(v, want), n
        assert np.array_equal(v[0], ship[k, 0]), n                                       # mu_B = 0 rows: the shipped ones
        T1, v1 = api.df_table_read(os.path.join(base, "out", n + ".dat"))
        assert np.array_equal(T1, Tf) and np.array_equal(v1, v[0])
    again = subprocess.run([api.CLI_PATH, "--generate-df", "out"], cwd=base, capture_output=True, text=True, timeout=120)
    assert again.returncode != 0 and "never overwritten" in again.stderr

    def run(name, key):
        root = str(tmp_path / name)
        shutil.copytree(base, root)
        if key:
            with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
                f.write("deltaf_dir = %s   # coefficient tables from here\n" % key)
        rr = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=300)
        assert rr.returncode == 0, rr.stdout + rr.stderr
        files = {}
        for dp, _, fn in os.walk(os.path.join(root, "results")):
            for f in fn:
                files[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), "rb").read()
        assert len(files) >= 4 and all(files.values())
        return files, rr.stdout

    plain, out_plain = run("plain", None)                                                # no key: deltaf_coefficients/vh/urqmd/ as before
    assert "deltaf_dir" not in out_plain
    same, _ = run("same", "deltaf_coefficients/vh/urqmd")                                # the key names the default directory: nothing changes
    generated, out_gen = run("generated", "out")
    assert "out/ (deltaf_dir)" in out_gen
    assert same == plain
    assert generated == plain
