"""CPU: the plans' host-side geometry (is3d_amd/csrc/cf_plan_geometry.h) through a host-only program, tests/cpp/plan_geometry_main.cpp.
The golden tables under tests/golden/plan_*.json were recorded from the statements these functions replaced (cf_plan.cpp and cf_vah.hip at
1774277), compiled verbatim behind the same driver -- not from the functions themselves; where that commit held two copies of a rule the
recording checked that they agree.  The properties below are what the kernels and cf_finalize rely on."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
GOLDEN = os.path.join(ROOT, "tests", "golden")

HAND = dict(mass=np.array([0.5, 0.138, 0.5, 0.938, 0.938, 0.138, 0.938]), sign=np.array([-1.0, -1.0, 1.0, 1.0, 1.0, -1.0, 1.0]),
            baryon=np.array([0.0, 0.0, 0.0, 1.0, -1.0, 0.0, 1.0]))   # a repeated mass of opposite sign; a repeated (mass, sign) with another baryon number
LANE_CASES = [(which, n_pT, split, use_b, 0) for which in ("pikp", "urqmd", "hand") for n_pT in (1, 32, 33) for split in (1, 2, 4) for use_b in (0, 1)] + \
             [(which, n_pT, 1, 0, 1) for which in ("pikp", "urqmd") for n_pT in (32, 33)]


def pT_grid(n):
    """n ascending pT values"""
    return [0.05 + 0.1 * i for i in range(n)]


def species_list(which):
    if which == "hand":
        return HAND
    from is3d_amd import inputs
    return inputs.species(which)


def build_prog(out, extra=()):
    subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, os.path.join(ROOT, "tests", "cpp", "plan_geometry_main.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=600)
    return out


def rows(prog, mode):
    out = subprocess.run([prog, mode], check=True, capture_output=True, text=True, timeout=120).stdout
    table = {}
    for r in out.split("\n"):
        if r:
            table.setdefault(r[0], []).append([int(x) for x in r.split()[1:]])
    return table


def lanes(prog, tmp, sp, pT, split, use_b, inter, collapse=1):
    """(arrays by name, sha256 of the program's output) for one species list and pT grid"""
    path = os.path.join(str(tmp), "lanes_in.txt")
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n" % (len(sp["mass"]), len(pT), split, inter, use_b, collapse))
        for m, s, b in zip(sp["mass"], sp["sign"], sp["baryon"]):
            f.write("%r %r %r\n" % (float(m), float(s), float(b)))
        f.write(" ".join(repr(float(p)) for p in pT) + "\n")
    out = subprocess.run([prog, "lanes", path], check=True, capture_output=True, text=True, timeout=120).stdout
    t = {}
    for r in out.split("\n"):
        if r:
            w = r.split()
            t[w[0]] = np.array([float(x) for x in w[1:]]) if w[0] in ("cmass", "csign", "cbar", "mT", "pT", "sign", "b") else np.array([int(x) for x in w[1:]], dtype=np.int64)
    return t, hashlib.sha256(out.encode()).hexdigest()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return build_prog(str(tmp_path_factory.mktemp("plan_geometry") / "plan_geometry_main"))


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_variants_equal_the_recorded_table(prog):
    got = rows(prog, "variants")["v"]
    assert len(got) == 2 * 2 * 2 * 2 * 17 * 2 == 544
    assert got == golden("plan_variants.json")["rows"]


def test_variant_table_says_what_the_builds_honour(prog):
    """the decision as DESIGN.md states it, on the rows: (dim, fq, bar, fits, req, dev) -> (variant, e2tab)"""
    t = {tuple(r[:6]): tuple(r[6:]) for r in rows(prog, "variants")["v"]}
    for dev in (0, 1):
        for req in (-1, 0, 14, 15):   # no request, or none the plan knows: the defaults
            assert t[(3, 0, 0, 1, req, dev)] == (6, 1) and t[(3, 0, 1, 1, req, dev)] == (6, 1)
            assert t[(3, 0, 0, 0, req, dev)] == (3, 0) and t[(3, 0, 1, 0, req, dev)] == (2, 0)
            assert all(t[(3, 1, b, f, req, dev)] == (3, 0) for b in (0, 1) for f in (0, 1))
            assert all(t[(2, q, b, f, req, dev)] == (7, 0) for q in (0, 1) for b in (0, 1) for f in (0, 1))
    shipped = {k: v for k, v in t.items() if k[5] == 0}
    assert all(v == t[k[:4] + (0, 0)] for k, v in shipped.items() if not (k[:3] == (3, 0, 0) and k[4] == 3))   # one honoured request:
    assert t[(3, 0, 0, 1, 3, 0)] == (3, 0)                                                                        # 8 x 7 without the E2 stream
    assert all(v[1] == (1 if v[0] in (5, 6, 9, 10, 11, 12, 13) and k[:2] == (3, 0) else 0) for k, v in t.items())
    assert all(k[3] == 1 for k, v in t.items() if v[1])   # the E2 stream only where the pT grid fits it


def test_sizing_equals_the_recorded_table(prog):
    got, want = rows(prog, "sizing"), golden("plan_sizing.json")
    assert len(got["w"]) == 64 * 5 and got["w"] == want["waves_per_group"]
    assert len(got["c"]) == 2 * 7 * 19 * 4 * 5 and got["c"] == want["chunk_count"]
    assert len(got["s"]) == 512 * 8 and got["s"] == want["lane_split"]


def test_lane_split_rule(prog):
    s = {(b, r): v for b, r, v in rows(prog, "sizing")["s"]}
    assert s[(96, 4)] == 4 and s[(96, 2)] == 1 and s[(96, 3)] == 1 and s[(64, 4)] == 1
    for (bins, rb), S in s.items():
        assert S in (1, 2, 4) and rb % S == 0 and 4 % S == 0   # the invariant the kernels rely on
        waste = lambda n, q: 1.0 - n / float(-(-n // q) * q)
        if S > 1:
            assert waste(bins * S, 128) < waste(bins, 64) - 0.05


def test_chunk_count_bounds(prog):
    for rounds, tasks, pc, cc, slab, nch in rows(prog, "sizing")["c"]:
        assert 1 <= nch <= max(1, pc // 64)
        assert nch == 1 or nch * slab <= (32 if cc else 12) << 30
        if cc:
            assert nch <= cc


def test_waves_per_group_rule(prog):
    for lw, req, wpb in rows(prog, "sizing")["w"]:
        if req in (2, 4, 8):
            assert wpb == req
        else:
            idle = {w: -(-lw // w) * w - lw for w in (8, 4, 2)}
            assert idle[wpb] == min(idle.values()) and all(idle[w] > idle[wpb] for w in (8, 4, 2) if w > wpb)


@pytest.mark.parametrize("which,n_plain,n_baryon", [("pikp", None, None), ("urqmd", 75, 124), ("hand", 4, 5)])
def test_species_classes(prog, tmp_path, which, n_plain, n_baryon):
    sp = species_list(which)
    n = len(sp["mass"])
    for use_b, want in ((0, n_plain), (1, n_baryon)):
        t, _ = lanes(prog, tmp_path, sp, pT_grid(1), 1, use_b, 0)
        cls = t["cls"]
        if want is not None:
            assert t["ncls"][0] == want
        key = [(sp["mass"][s], sp["sign"][s], sp["baryon"][s] if use_b else 0.0) for s in range(n)]
        for a in range(n):
            for b in range(a):
                assert (cls[a] == cls[b]) == (key[a] == key[b])
        first = [int(np.argmax(cls == c)) for c in range(int(t["ncls"][0]))]
        assert first == sorted(first) and sorted(set(cls.tolist())) == list(range(len(first)))   # numbered by first appearance
        assert [(t["cmass"][c], t["csign"][c], t["cbar"][c]) for c in range(len(first))] == [key[s] for s in first]
        t1, _ = lanes(prog, tmp_path, sp, pT_grid(1), 1, use_b, 0, collapse=0)
        assert t1["cls"].tolist() == list(range(n))   # collapse off: one class per species
    if which == "hand":
        t, _ = lanes(prog, tmp_path, sp, pT_grid(1), 1, 1, 0)
        assert t["cls"].tolist() == [0, 1, 2, 3, 4, 1, 3]


@pytest.mark.parametrize("which,n_pT,split,use_b,inter", LANE_CASES)
def test_lane_table(prog, tmp_path, which, n_pT, split, use_b, inter):
    sp, pT = species_list(which), pT_grid(n_pT)
    t, digest = lanes(prog, tmp_path, sp, pT, split, use_b, inter)
    assert digest == golden("plan_lanes.json")["%s/%d/%d/%d/%d" % (which, n_pT, split, use_b, inter)]
    ncls = int(t["ncls"][0])
    Lbins, L, Lpad = (int(x) for x in t["sizes"])
    assert Lbins == ncls * n_pT and L == Lbins * split and Lpad == -(-L // 64) * 64
    order, slot_of = t["order"], t["slot_of"]
    mT_nat = np.sqrt(np.repeat(t["cmass"], n_pT) ** 2 + np.tile(np.array(pT), ncls) ** 2)
    plain = np.argsort(mT_nat, kind="stable")   # nondecreasing mT, ties in natural order
    if inter:
        want = plain.copy()
        for b in range(0, Lbins - 127, 128):
            want[b:b + 64], want[b + 64:b + 128] = plain[b:b + 128:2], plain[b + 1:b + 128:2]
        assert order.tolist() == want.tolist()
    else:
        assert order.tolist() == plain.tolist()
        assert np.all(np.diff(t["mT"][:Lbins]) >= 0)
    assert sorted(order.tolist()) == list(range(Lbins)) and slot_of[order].tolist() == list(range(Lbins))
    for sl in range(split):   # slot (bin s, sub sl) = sl * Lbins + s
        lo = sl * Lbins
        assert np.array_equal(t["mT"][lo:lo + Lbins], mT_nat[order])
        assert np.array_equal(t["pT"][lo:lo + Lbins], np.array(pT)[order % n_pT])
        assert np.array_equal(t["sign"][lo:lo + Lbins], t["csign"][order // n_pT])
        assert np.array_equal(t["b"][lo:lo + Lbins], t["cbar"][order // n_pT])
        assert np.all(t["sub"][lo:lo + Lbins] == sl)
    for name, pad in (("mT", 1), ("pT", 0), ("sign", 1), ("b", 0), ("sub", 0)):
        assert len(t[name]) == Lpad and np.all(t[name][L:] == pad)
    lane_of = t["lane_of"].reshape(len(sp["mass"]), n_pT)
    assert np.array_equal(lane_of, slot_of[t["cls"][:, None] * n_pT + np.arange(n_pT)[None, :]])
