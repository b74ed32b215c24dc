#!/usr/bin/env python3
"""Generate tests/golden/golden_extreme_op0.npz and golden_extreme_op0.json (run in the build container; both are committed).

Operation 0 on the committed cells of golden_extreme.npz (no new cells): per case D [S][6][36], the numpy long-double single-cell spectrum
contracted with the seeded phi_w of tests/extreme_cells.py and summed over y (3+1D) or over the eta nodes with their weights (2+1D), per pT
node, as doubles; for the 2+1D cases also <key>_eta [S][5], the dN/dy deta partials of the whole surface at the eta nodes 0, 60, 120, 180, 240
under the all-ones pT weight.  The keys are those of golden_extreme.json.

  delta-f, baryon        make_golden.highprec_spectrum, one cell at a time
  anisotropic hydro      make_golden_vah.highprec_vah, one cell at a time, with the committed (scipy) coefficients
  modified equilibrium   tests/dndx_feqmod_ref.py in long double: operation 0 is not the spectra routine (no 3+1D narrow-row fallback, another
                         eta_scale and NaN test), so make_golden.highprec_feqmod does not apply

golden_extreme_op0.json: per case the double reference's largest error against D in the metric of tests/extreme_cells_op0.py (the oracle, or the
double dndx_feqmod_ref), the number of entries of D above the 1e-280 floor, and the skipped, breakdown and renorm-skipped counts.

The archive is written member by member with a fixed timestamp, so that a second run gives the same bytes."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
os.environ.setdefault("OMP_NUM_THREADS", "1")

import extreme_cells as X  # noqa: E402
import extreme_cells_op0 as O  # noqa: E402
import make_golden as MG  # noqa: E402
import make_golden_vah as MV  # noqa: E402
from make_golden_extreme import write_npz  # noqa: E402

LD = np.longdouble


def longdouble_reference(case):
    """-> (D, eta or None, counts) in long double"""
    cells, o, dim, fam = X.fixture_cells(case["cells"]), case["opts"], case["dim"], case["family"]
    sp, g = X.species(), dict(X.grid())
    if fam == "fq":
        return O.feqmod_reference(cells, o, LD)
    if fam == "vah":
        reg = bool(o["regulate_deltaf"])
        D = O.per_cell(lambda c1: MV.highprec_vah(c1, sp, g, dim, reg, rounded=False), cells, dim)
        eta = O.eta_partials(lambda g1: MV.highprec_vah(cells, sp, g1, 2, reg, rounded=False), True) if dim == 2 else None
        return D, eta, dict(n_skipped=0, n_breakdown=0, n_renorm_skipped=0)          # (this path skips no cell)
    df = O.df_tables(fam == "dfb")
    D = O.per_cell(lambda c1: MG.highprec_spectrum(c1, sp, g, df, o), cells, dim)
    eta = O.eta_partials(lambda g1: MG.highprec_spectrum(cells, sp, g1, df, o), False) if dim == 2 else None
    return D, eta, dict(n_skipped=int((~X.live(cells)).sum()), n_breakdown=0, n_renorm_skipped=0)


def main():
    out, cases = {}, []
    np.seterr(over="ignore", under="ignore")
    for src in X.fixture_cases():
        case = {k: src[k] for k in ("key", "family", "case", "dim", "cells", "opts")}
        D, eta, counts = longdouble_reference(case)
        D = D.astype(np.float64)
        eta = None if eta is None else eta.astype(np.float64)
        assert D.shape == (len(X.species()["mass"]), 6, X.N_CELLS) and np.isfinite(D).all(), case["key"]
        chk_D, chk_eta = O.double_reference(case)
        sD, sE = O.scales(case, D, eta)
        err = O.error(chk_D, D, sD)
        out[case["key"]] = D
        if eta is not None:
            assert np.isfinite(eta).all(), case["key"]
            out[case["key"] + "_eta"] = eta
            err = max(err, O.error(chk_eta, eta, sE))
        live = np.abs(D) > O.FLOOR
        case.update(ref_err=err, n_live=int(live.sum()), n_live_per_node=[int(x) for x in live.sum(axis=(0, 2))], **counts)
        cases.append(case)
        print("%-40s double reference vs long double %.3e  live %d of %d %s %s" % (case["key"], err, case["n_live"], D.size, case["n_live_per_node"],
                                                                                   {k: v for k, v in counts.items() if v}), flush=True)
    write_npz(os.path.join(HERE, "golden_extreme_op0.npz"), out)
    with open(os.path.join(HERE, "golden_extreme_op0.json"), "w") as f:
        json.dump(dict(species=X.species_ids(), n_cells=X.N_CELLS, eta_nodes=list(X.ETA_NODES), cases=cases), f, indent=1)
        f.write("\n")
    sizes = [os.path.getsize(os.path.join(HERE, n)) for n in ("golden_extreme_op0.npz", "golden_extreme_op0.json", "golden_extreme.npz")]
    assert sizes[0] < sizes[2]
    print("wrote golden_extreme_op0.npz (%d bytes), golden_extreme_op0.json (%d bytes); worst double-reference error %.3e" % (
        sizes[0], sizes[1], max(c["ref_err"] for c in cases)))


if __name__ == "__main__":
    main()
