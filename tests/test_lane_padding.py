"""CPU: the per-lane arrays a plan uploads (is3d::lane_arrays, is3d_amd/csrc/cf_plan_geometry.h) through a host-only program,
tests/cpp/lane_padding_main.cpp.  The slots in use carry the lane table's values bit for bit and what the plans derive from them (stated here
once more in numpy); every padding slot is a copy of slot L - 1 in every array, so that it casts that lane's cull votes and no others; a table
of whole waves comes back as it was."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
FLOATS = ("cmass", "t.mT", "t.pT", "t.sign", "t.b", "a.mT", "a.pT", "a.sign", "a.b", "a.mass", "max")
CASES = [(which, n_pT, split, use_b) for which in ("pikp", "urqmd") for n_pT in (1, 5, 32) for split in (1, 2, 4) for use_b in (0, 1)]
FOUR = dict(mass=np.array([0.3, 1.1, 0.7, 2.0]), sign=np.array([-1.0, 1.0, -1.0, 1.0]), baryon=np.array([0.0, 1.0, 0.0, -1.0]))   # x 32 pT: two whole waves


def pT_grid(n):
    return [0.05 + 0.1 * i for i in range(n)]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("lane_padding") / "lane_padding_main")
    subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "lane_padding_main.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=600)
    return out


def arrays(prog, tmp, sp, pT, split, use_b):
    path = os.path.join(str(tmp), "lanes_in.txt")
    with open(path, "w") as f:
        f.write("%d %d %d 0 %d 1\n" % (len(sp["mass"]), len(pT), split, use_b))
        for m, s, b in zip(sp["mass"], sp["sign"], sp["baryon"]):
            f.write("%r %r %r\n" % (float(m), float(s), float(b)))
        f.write(" ".join(repr(float(p)) for p in pT) + "\n")
    out = subprocess.run([prog, path], check=True, capture_output=True, text=True, timeout=120).stdout
    t = {}
    for r in out.split("\n"):
        if r:
            w = r.split()
            t[w[0]] = np.array([float.fromhex(x) for x in w[1:]]) if w[0] in FLOATS else np.array([int(x) for x in w[1:]], dtype=np.int64)
    return t


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def check(t, n_pT, split):
    Lbins, L, Lpad, aLpad = (int(x) for x in t["sizes"])
    assert L == Lbins * split and Lpad == -(-L // 64) * 64 and aLpad == Lpad   # Lpad unchanged
    names = ("mT", "pT", "sign", "b", "mass", "sub", "ipT", "pe", "cls")
    for n in names:
        assert len(t["a." + n]) == Lpad, n
    # slots in use: the lane table's own values, bit for bit ...
    for n in ("mT", "pT", "sign", "b"):
        assert np.array_equal(bits(t["a." + n][:L]), bits(t["t." + n][:L])), n
    assert np.array_equal(t["a.sub"][:L], t["t.sub"][:L])
    # ... and what the plans derive from them: every slot of a bin carries the bin's class, its mass and its pT index; pe from the maxima over the slots in use
    nat = np.tile(t["order"], split)
    assert np.array_equal(t["a.cls"][:L], nat // n_pT) and np.array_equal(t["a.ipT"][:L], nat % n_pT)
    assert np.array_equal(bits(t["a.mass"][:L]), bits(t["cmass"][nat // n_pT]))
    mTmax, pTmax = t["t.mT"][:L].max(), np.abs(t["t.pT"][:L]).max()
    assert np.array_equal(bits(t["max"]), bits([mTmax, pTmax]))
    f = np.maximum(t["t.mT"][:L] / mTmax, np.abs(t["t.pT"][:L]) / pTmax)
    assert np.array_equal(t["a.pe"][:L], np.minimum(np.frexp(f * (1.0 + 1.0e-12))[1], 0))
    assert np.all((f < 2.0 ** t["a.pe"][:L]) | (t["a.pe"][:L] == 0)) and np.all(t["a.pe"] <= 0)   # the bound it stands for, clamped at 0
    # every padding slot: slot L - 1, in every array (the heaviest bin of the last sub-lane, in the padding's own wave)
    assert (L - 1) // 64 == (Lpad - 1) // 64
    for n in names:
        a = t["a." + n]
        if n in ("mT", "pT", "sign", "b", "mass"):
            assert np.all(bits(a[L:]) == bits(a[L - 1:L])), n
        else:
            assert np.all(a[L:] == a[L - 1]), n
    assert t["a.sub"][L - 1] == split - 1 and t["a.mT"][L - 1] == t["t.mT"][:L].max()
    if L == Lpad:   # whole waves: nothing to pad, the table comes back as it was
        for n in ("mT", "pT", "sign", "b"):
            assert np.array_equal(bits(t["a." + n]), bits(t["t." + n])), n
        assert np.array_equal(t["a.sub"], t["t.sub"])
    else:           # the host table's own padding stays what tests/test_plan_geometry.py pins
        for n, pad in (("mT", 1), ("pT", 0), ("sign", 1), ("b", 0), ("sub", 0)):
            assert np.all(t["t." + n][L:] == pad)
    return L, Lpad


@pytest.mark.parametrize("which,n_pT,split,use_b", CASES)
def test_padding_copies_the_last_slot(prog, tmp_path, which, n_pT, split, use_b):
    from is3d_amd import inputs
    check(arrays(prog, tmp_path, inputs.species(which), pT_grid(n_pT), split, use_b), n_pT, split)


@pytest.mark.parametrize("split", [1, 2, 4])
def test_whole_wave_table_comes_back_unchanged(prog, tmp_path, split):
    L, Lpad = check(arrays(prog, tmp_path, FOUR, pT_grid(32), split, 1), 32, split)
    assert L == Lpad == 128 * split


def test_negative_pT_enters_the_bound_by_its_modulus(prog, tmp_path):
    """cf_plan.cpp took |pT| for pTmax and pe; the lane arrays do the same"""
    check(arrays(prog, tmp_path, FOUR, [-3.0, 0.5, 1.0], 1, 0), 3, 1)
