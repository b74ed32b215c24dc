#!/usr/bin/env python3
"""Build tests/golden/golden_dfcoef_lists.npz -- REFERENCE-HELD coefficient rows for the other two hadron lists.

The reference ships its coefficient generator's output for three lists.  golden_dfcoef.npz (make_golden_dfcoef.py) holds rows of the urqmd
one; this file holds, for `smash` (hrg_eos = 2, PDG/pdg_smash.dat, 493 entries) and `smash_box` (hrg_eos = 3, PDG/pdg_box.dat, 400 entries):
  <list>_mass, _gspin, _baryon, _sign   the list as api.pdg_read returns it (every entry, the photon included)
  <list>_text     [10][len(iB)][len(iT)]  the printed strings of deltaf_coefficients/vh/<list>/{c0..betapi}.dat at every 8th mu_B x every
                  10th T row, parsed here with plain Python
  <list>_shipped  the same as doubles
  T, muB, iT, iB, names   the grid of the shipped tables, the sampled rows, the order of the ten tables
The 64-point Gauss-Laguerre rule is the one golden_dfcoef.npz carries (the three generators' files are identical; asserted here).
Before writing, every stored value's printed digits are recomputed on the CPU with oracle.df_generator_row and must agree.

The inputs are the reference's data files as tests/golden/reference_data.tar.xz packs them.  Run:  python tests/golden/make_golden_dfcoef_lists.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from conftest import unpack_reference_data  # noqa: E402
from is3d_amd import api  # noqa: E402
from make_golden_dfcoef import NAMES, read_gla, read_table_text  # noqa: E402
from oracle import oracle  # noqa: E402

OUT = os.path.join(HERE, "golden_dfcoef_lists.npz")
LISTS = {"smash": ("PDG/pdg_smash.dat", False, 493), "smash_box": ("PDG/pdg_box.dat", True, 400)}


def printed(v):
    s = "%.6f" % v
    return "0.000000" if s == "-0.000000" else s


def main():
    ref = unpack_reference_data(tempfile.mkdtemp())
    urqmd = np.load(os.path.join(HERE, "golden_dfcoef.npz"))
    iT, iB = np.arange(0, 101, 10), np.arange(0, 81, 8)
    out = dict(names=np.array(NAMES), iT=iT, iB=iB)
    for which, (path, box, n) in LISTS.items():
        pdg = api.pdg_read(os.path.join(ref, path), box=box)
        assert len(pdg["mass"]) == n
        root, weight = read_gla(os.path.join(ref, "generate_delta_f_coefficients", which, "df_vh_dimensionless/gauss_laguerre/gla_roots_weights_64_points.txt"))
        assert np.array_equal(root, urqmd["root"]) and np.array_equal(weight, urqmd["weight"])
        text = []
        for name in NAMES:
            T, B, txt = read_table_text(os.path.join(ref, "deltaf_coefficients/vh", which, name + ".dat"))
            text.append(txt[np.ix_(iB, iT)])
        text = np.array(text)
        assert np.array_equal(T, urqmd["T"]) and np.array_equal(B, urqmd["muB"])
        worst = 0.0
        for jB, b in enumerate(iB):
            for jT, t in enumerate(iT):
                row = oracle.df_generator_row(pdg, root, weight, T[t], B[b])
                for k in range(10):
                    assert printed(row[k]) == printed(float(text[k, jB, jT])), (which, NAMES[k], T[t], B[b], row[k], text[k, jB, jT])
                    worst = max(worst, abs(row[k] - float(text[k, jB, jT])))
        print("%s: %d entries, %d rows x 10 tables reproduced digit for digit, max |difference| %.3e" % (which, n, len(iB) * len(iT), worst))
        for k in ("mass", "gspin", "baryon", "sign"):
            out[which + "_" + k] = pdg[k]
        out[which + "_text"] = text
        out[which + "_shipped"] = text.astype(np.float64)
    out["T"], out["muB"] = T, B
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
