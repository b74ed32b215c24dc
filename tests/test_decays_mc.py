"""CPU: the Monte Carlo decay of sampled hadrons (is3d_decay_particles) as far as it runs without a device -- the restatement the device is held
to (tests/decays_mc_ref.py) checked on its own (conservation, mass shell, flat three-body phase space, its rounding floor), the table
analysis of the entry on the shipped and on hand-built tables, the layout of the two new structs, every refusal before any device use, the
answer without a device, and the run driver's refusals of decay_sampled_hadrons."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import decays_mc_cases as cases
import decays_mc_ref as ref
import refformat
from conftest import ROOT
from is3d_amd import api, synth
from oracle import oracle

NAMES = ["pdg-urqmd_v3.3+.dat", "pdg_smash.dat"]


@pytest.fixture(scope="module")
def tabs(reference):
    t = cases.tables(api, reference)
    return {k: (v, ref.prepare(v)) for k, v in t.items()}


def restate(t, prep, q, lifetime=0, dtype=np.float64, seed=cases.SEED):
    return ref.decay_particles(t, t["mc_id"], q, oracle.rng_uniforms, seed, 0, lifetime, dtype, prep)


@pytest.mark.parametrize("name,count", [(NAMES[0], 303), (NAMES[1], 346)])
def test_restatement_conserves_and_ends_on_final_particles(tabs, name, count):
    """One primary of every unstable species: the final particles of a primary carry its four-momentum, each sits on its table mass shell,
    and each is stable or has no open channel (10333 of the urqmd table, alone)."""
    t, prep = tabs[name]
    q = cases.every_unstable(api, t, 3)
    assert len(q) == count
    for lifetime in (0, 1):
        r = restate(t, prep, q, lifetime)
        tot = np.zeros((len(q), 4))
        np.add.at(tot, r["origin"], r["mom"])
        assert set(r["origin"]) == set(range(len(q)))
        assert np.max(np.abs(tot - np.stack([q[k] for k in ref.MOM], 1)) / q["E"][:, None]) <= cases.BOUND
        m, E = prep["mass"][r["species"]], r["mom"][:, 0]
        assert np.all(np.abs(E * E - (r["mom"][:, 1:] ** 2).sum(1) - m * m) <= cases.BOUND * E * E)
        stuck = [e for e in r["species"] if not t["stable"][e]]
        assert all(not prep["open"][e] for e in stuck) and len(stuck) == r["stats"]["n_stuck"]
        assert [int(t["mc_id"][e]) for e in stuck] == ([10333] if "urqmd" in name else [])
        assert r["stats"]["n_exhausted"] == 0
        if not lifetime:
            assert np.array_equal(r["pos"], np.stack([q[k] for k in ref.POS], 1)[r["origin"]])


def test_rounding_floor(tabs):
    """cases.FLOOR is the distance between the float64 and the longdouble run of the restatement on the lists of the device tests"""
    worst = 0.0
    for name in NAMES:
        t, prep = tabs[name]
        lists = [cases.every_unstable(api, t, 3)] + ([cases.hand_list(api, t, prep)] if "urqmd" in name else [])
        for q in lists:
            for lifetime in (0, 1):
                a, b = restate(t, prep, q, lifetime), restate(t, prep, q, lifetime, np.longdouble)
                assert np.array_equal(a["species"], b["species"]) and np.array_equal(a["origin"], b["origin"])
                worst = max(worst, cases.distance(a["mom"], a["pos"], b["mom"], b["pos"], a["origin"], q))
    print("float64 against longdouble: %.3g (FLOOR %.3g, BOUND %.3g)" % (worst, cases.FLOOR, cases.BOUND))
    assert 0.0 < worst <= cases.FLOOR


PI = [(211, 0.13957, 0.0, 1, [(1, 1.0, [211])]), (-211, 0.13957, 0.0, 1, [(1, 1.0, [-211])]), (111, 0.13498, 0.0, 1, [(1, 1.0, [111])])]
OMEGA_3PI = cases.hand_table(PI + [(223, 0.78265, 0.00849, 0, [(3, 0.89, [211, -211, 111])])])


def test_three_body_phase_space_is_flat():
    """omega -> pi+ pi- pi0 at rest, 20 000 times: the mean of m12^2 lies within 5 standard errors of the flat-Dalitz mean, in which m12^2
    is weighted with the length of the m23^2 interval, sqrt(lambda(m12^2, m1^2, m2^2) lambda(M^2, m12^2, m3^2)) / m12^2"""
    from scipy.integrate import quad
    N = 20000
    t = OMEGA_3PI
    q = ref.make_particles(api, t, t["mc_id"], [3] * N, np.zeros((N, 3)))
    r = restate(t, ref.prepare(t), q, seed=5)
    assert len(r["species"]) == 3 * N and r["stats"]["n_exhausted"] == 0 and r["stats"]["n_trials"] > N
    p12 = r["mom"][0::3] + r["mom"][1::3]
    m12sq = p12[:, 0] ** 2 - (p12[:, 1:] ** 2).sum(1)
    M, m1, m2, m3 = 0.78265, 0.13957, 0.13957, 0.13498
    lam = lambda a, b, c: a * a + b * b + c * c - 2.0 * (a * b + b * c + c * a)  # noqa: E731
    w = lambda s: np.sqrt(max(lam(s, m1 * m1, m2 * m2) * lam(M * M, s, m3 * m3), 0.0)) / s  # noqa: E731
    lo, hi = (m1 + m2) ** 2, (M - m3) ** 2
    mean = quad(lambda s: s * w(s), lo, hi, epsrel=1e-12)[0] / quad(w, lo, hi, epsrel=1e-12)[0]
    assert abs(m12sq.mean() - mean) <= 5.0 * m12sq.std(ddof=1) / np.sqrt(N)


def analysed(t):
    """the static stats of the entry for a table (an empty list needs no device)"""
    out, origin, st = api.decay_particles(t, t["mc_id"], np.zeros(0, api.PARTICLE_DTYPE))
    assert len(out) == 0 and len(origin) == 0 and st["n_final"] == 0
    return st


def chain_table(top_bodies):
    """X0 -> s s, Xk -> X(k-1) s s s s (k = 1..3), X4 -> X3 + (top_bodies - 1) s: a pending-stack need of 2, 6, 10, 14, 14 + top_bodies - 1"""
    e = [(1, 0.1, 0.0, 1, [(1, 1.0, [1])]), (100, 0.3, 0.1, 0, [(2, 1.0, [1, 1])])]
    for k in range(1, 4):
        e.append((100 + k, 0.3 + 0.5 * k, 0.1, 0, [(5, 1.0, [100 + k - 1, 1, 1, 1, 1])]))
    e.append((104, 2.4, 0.1, 0, [(top_bodies, 1.0, [103] + [1] * (top_bodies - 1))]))
    return cases.hand_table(e)


def test_table_analysis(tabs):
    for name, stack, depth, closed in ((NAMES[1], 3, 5, 222), (NAMES[0], 5, 4, 79)):
        st = analysed(tabs[name][0])
        prep = tabs[name][1]
        assert (st["max_stack"], st["n_closed_channels"]) == (stack, closed)
        assert (st["max_stack"], st["max_depth"], st["n_closed_channels"]) == (prep["max_stack"], prep["max_depth"], prep["n_closed"])
        assert st["max_depth"] == depth       # the deepest chain of the shipped tables is 5 decays
    assert analysed(chain_table(3))["max_stack"] == 16 and analysed(chain_table(3))["max_depth"] == 5
    with pytest.raises(api.Is3dError) as e:
        analysed(chain_table(4))
    assert e.value.code == api.IS3D_EINVAL and "17" in str(e.value)
    cyc = cases.hand_table(PI + [(9001, 1.0, 0.1, 0, [(2, 1.0, [9002, 111])]), (9002, 1.1, 0.1, 0, [(2, 1.0, [9001, 111])])])
    with pytest.raises(api.Is3dError) as e:
        analysed(cyc)
    assert e.value.code == api.IS3D_EINVAL and "cycle" in str(e.value)
    with pytest.raises(ref.TableError):
        ref.prepare(cyc)
    with pytest.raises(ref.TableError):
        ref.prepare(chain_table(4))


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "is3d_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n",'
                   'sizeof(is3d_decay_mc_inputs), offsetof(is3d_decay_mc_inputs, lifetime), offsetof(is3d_decay_mc_inputs, device),'
                   'sizeof(is3d_decay_mc_stats), offsetof(is3d_decay_mc_stats, n_exhausted), offsetof(is3d_decay_mc_stats, max_stack),'
                   'offsetof(is3d_decay_mc_stats, n_closed_channels), offsetof(is3d_decay_mc_stats, ms_h2d),'
                   'IS3D_DECAY_MC_MAX_BODIES, IS3D_DECAY_MC_MAX_STACK, IS3D_DECAY_MC_MAX_TRIALS);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    I, S = api.DecayMcInputs, api.DecayMcStats
    assert c == [ctypes.sizeof(I), I.lifetime.offset, I.device.offset, ctypes.sizeof(S), S.n_exhausted.offset, S.max_stack.offset,
                 S.n_closed_channels.offset, S.ms_h2d.offset, ref.MAX_BODIES, ref.MAX_STACK, ref.MAX_TRIALS]
    assert "is3d_decay_particles" in api.EXPORTS and hasattr(api.load(), "is3d_decay_particles")


def test_every_refusal_precedes_device_use(tabs):
    t, _ = tabs[NAMES[1]]
    chosen = [211, -211, 113]
    q = ref.make_particles(api, t, chosen, [2, 0, 1], np.ones((3, 3)) * 0.2)
    before = api.resource_counters()

    def refused(table=t, ch=chosen, particles=q, needle=""):
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles(table, ch, particles)
        assert e.value.code == api.IS3D_EINVAL and needle in str(e.value), str(e.value)

    for s in (-1, 3):
        bad = q.copy()
        bad["species"][1] = s
        refused(particles=bad, needle="species")
    refused(ch=[211, 999999], needle="999999")
    first = np.concatenate([[0], np.cumsum(t["n_channels"])])
    rho = int(np.nonzero(t["mc_id"] == 113)[0][0])
    lost = dict(t, daughters=t["daughters"].copy())
    lost["daughters"][first[rho], 0] = 424242
    refused(table=lost, needle="424242")
    six = dict(t, npart=t["npart"].copy())
    six["npart"][first[rho]] = -6
    refused(table=six, needle="6 decay products")
    refused(table=chain_table(4), ch=[104], particles=q[:0], needle="stack")
    # the raw entry: NULL arguments and a negative count
    L = api.load()
    ts, ch, _, keep = api._decay_pack(t, chosen, dict(pT=[1.0], phi=[0.0], y=[0.0]))
    inp, cnt = api.DecayMcInputs(1, 0, 0, -1), ctypes.c_int64(7)
    L.is3d_decay_particles.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    good = [ctypes.addressof(ts), 3, ch.ctypes.data, ctypes.addressof(inp), 3, q.ctypes.data, None, None, 0, ctypes.addressof(cnt), None]
    for k in (0, 2, 3, 5, 9):
        a = list(good)
        a[k] = None
        assert L.is3d_decay_particles(*a) == api.IS3D_EINVAL, k
    a = list(good)
    a[4] = -1
    assert L.is3d_decay_particles(*a) == api.IS3D_EINVAL
    assert api.resource_counters() == before
    if L.is3d_device_count() == 0:
        assert L.is3d_decay_particles(*good) == api.IS3D_ENODEVICE
        with pytest.raises(api.Is3dError) as e:
            api.decay_particles(t, chosen, q)
        assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)


@pytest.mark.parametrize("params,why", [(dict(operation=1), "operation = 1"), (dict(operation=0), "operation = 0"),
                                        (dict(operation=2, hrg_eos=3), "hrg_eos = 3"), (dict(operation=2, test_sampler=1), "test_sampler = 1")])
def test_cli_refuses_decay_sampled_hadrons(tmp_path, params, why):
    cells = synth.synth_surface(3, 3, seed=1)
    root = refformat.make_run_dir(str(tmp_path), cells, [211], params)
    with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:
        f.write("decay_sampled_hadrons\t= 1\n")
    r = subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "decay_sampled_hadrons = 1" in r.stderr and why in r.stderr, r.stderr
    assert not [f for _, _, fs in os.walk(os.path.join(root, "results")) for f in fs]
