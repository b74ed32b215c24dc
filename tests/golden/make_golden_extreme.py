#!/usr/bin/env python3
"""Generate tests/golden/golden_extreme.npz and golden_extreme.json (run in the build container; both are committed).

The three numpy long-double restatements -- highprec_spectrum and highprec_feqmod of make_golden.py, highprec_vah of make_golden_vah.py, none
of them written in C by the hand that wrote the kernels -- on every case of tests/extreme_cells.py: cells whose flow, temperature, viscous
stress, rapidity, proper time, anisotropy and mu_B lie far outside the box of the synthetic surfaces.

  golden_extreme.npz   the cells of every (case, dimension, family) and the spectra, as doubles:
                         df_<case>_<dim>_df<1|2>_<std|raw>      delta-f, raw = (outflow = 0, regulate_deltaf = 0)
                         dfb_<case>_<dim>_df<1|2>_diff<1|0>     include_baryon = 1, include_baryondiff_deltaf 1 | 0
                         fq_<case>_<dim>_mode<4|3>              modified equilibrium
                         vah_<case>_<dim>_reg<1|0>              anisotropic hydro, c0..c4 from scipy's multilinear interpolator
                         cells_<case>_<dim><|b|v>               one row per field: synth.CELL_FIELDS (b: + synth.BARYON_FIELDS; v: synth.VAH_FIELDS)
  golden_extreme.json  the case list; per case the oracle's largest error against the long-double value (the metric of
                       tests/test_extreme_cells.py) and the counts of the restatement: skipped cells, breakdown cells, narrow cells and rows,
                       dropped renormalisations, clamp statistics

The archive is written member by member with a fixed timestamp, so that a second run gives the same bytes."""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
os.environ.setdefault("OMP_NUM_THREADS", "1")

import extreme_cells as X  # noqa: E402
import make_golden as MG  # noqa: E402
import make_golden_vah as MV  # noqa: E402
from is3d_amd import inputs, synth  # noqa: E402
from oracle import oracle  # noqa: E402

RAW = dict(outflow=0, regulate_deltaf=0)
VAH_CELL_FIELDS = synth.VAH_FIELDS


def err_against(chk, ref, scale=None):
    s = np.abs(ref) if scale is None else scale
    return float(np.max(np.abs(chk - ref) / np.maximum(s, 1e-280)))


def raw_scale(cells, sp, grid, df, o, ref):
    """tests/test_gpu_fuzz.py: max(|ref|, 1e-4 (pos + neg)), pos / neg the oracle's spectra with the cut, dsigma as it is / negated"""
    oo = dict(o, outflow=1, regulate_deltaf=1)
    pos = oracle.dN_pTdpTdphidy(cells, sp, grid, df, oo)
    neg = oracle.dN_pTdpTdphidy({k: (-v if k in X.H.DS else v) for k, v in cells.items()}, sp, grid, df, oo)
    return np.maximum(np.abs(ref), 1e-4 * (pos + neg))


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue(), compresslevel=9)


def main():
    grid, sp = dict(X.grid()), X.species()
    df, dff, tab = inputs.df_tables(), inputs.df_tables_full(), inputs.vah_df_tables()
    out, cases = {}, []

    def keep_cells(tag, cells, fields):
        out["cells_" + tag] = np.stack([cells[k] for k in fields])

    def report(entry):
        cases.append(entry)
        print("%-40s oracle vs long double %.3e  %s" % (entry["key"], entry["oracle_err"], {k: v for k, v in entry.items() if k.startswith("n_") and v}))

    np.seterr(over="ignore", under="ignore")
    for case in X.VISCOUS_CASES:
        for dim in X.DIMS[case]:
            cells = X.surface(case, dim)
            keep_cells("%s_%d" % (case, dim), cells, synth.CELL_FIELDS)
            for dfm in (1, 2):
                for name, extra in (("std", {}), ("raw", RAW)):
                    o = dict(dimension=dim, df_mode=dfm, **extra)
                    key = "df_%s_%d_df%d_%s" % (case, dim, dfm, name)
                    st = {}
                    ref = MG.highprec_spectrum(cells, sp, grid, df, o, stats=st if name == "std" else None).astype(np.float64)
                    chk = oracle.dN_pTdpTdphidy(cells, sp, grid, df, o)
                    out[key] = ref
                    report(dict(key=key, family="df", case=case, dim=dim, cells="%s_%d" % (case, dim), opts=o,
                                oracle_err=err_against(chk, ref, raw_scale(cells, sp, grid, df, o, ref) if extra else None),
                                n_skipped=int((~X.live(cells)).sum()), n_terms=st.get("terms", 0), n_clamp_hi=st.get("clamp_hi", 0),
                                n_clamp_lo=st.get("clamp_lo", 0)))
            fq = inputs.feqmod_tables(inputs.surface_average_T(cells))
            for dfm in (4, 3):
                o = dict(dimension=dim, df_mode=dfm)
                key = "fq_%s_%d_mode%d" % (case, dim, dfm)
                ref, cnt = MG.highprec_feqmod(cells, sp, grid, df, fq, o)
                ref = ref.astype(np.float64)
                chk, nb = oracle.dN_pTdpTdphidy_feqmod(cells, sp, grid, df, fq, o)
                out[key] = ref
                report(dict(key=key, family="fq", case=case, dim=dim, cells="%s_%d" % (case, dim), opts=o, oracle_err=err_against(chk, ref),
                            n_skipped=cnt["skipped"], n_breakdown=cnt["breakdown"], n_breakdown_oracle=nb, n_narrow_cells=cnt["narrow_cells"],
                            n_narrow_rows=cnt["narrow_rows"], n_renorm_dropped=cnt["renorm_dropped"]))
    for case in X.BARYON_CASES:
        for dim in X.DIMS[case]:
            cells = X.surface(case, dim, baryon=True)
            keep_cells("%s_%db" % (case, dim), cells, synth.CELL_FIELDS + synth.BARYON_FIELDS)
            for dfm in (1, 2):
                for diff in (1, 0):
                    o = dict(dimension=dim, df_mode=dfm, include_baryon=1, include_baryondiff_deltaf=diff)
                    key = "dfb_%s_%d_df%d_diff%d" % (case, dim, dfm, diff)
                    ref = MG.highprec_spectrum(cells, sp, grid, dff, o).astype(np.float64)
                    chk = oracle.dN_pTdpTdphidy(cells, sp, grid, dff, o)
                    out[key] = ref
                    report(dict(key=key, family="dfb", case=case, dim=dim, cells="%s_%db" % (case, dim), opts=o, oracle_err=err_against(chk, ref),
                                n_skipped=int((~X.live(cells)).sum())))
    for case in X.VAH_CASES:
        for dim in X.DIMS[case]:
            cells = X.surface(case, dim, vah=True)
            cells = dict(cells, **MV.coefficients_scipy(tab, cells["Lambda"], cells["aL"]))
            keep_cells("%s_%dv" % (case, dim), cells, VAH_CELL_FIELDS)
            vc = {k: cells[k] for k in VAH_CELL_FIELDS}
            for reg in (1, 0):
                o = dict(dimension=dim, regulate_deltaf=reg)
                key = "vah_%s_%d_reg%d" % (case, dim, reg)
                ref = MV.highprec_vah(vc, sp, grid, dim, bool(reg))
                chk = oracle.dN_pTdpTdphidy_vah(vc, sp, grid, o)
                out[key] = ref
                report(dict(key=key, family="vah", case=case, dim=dim, cells="%s_%dv" % (case, dim), opts=o, oracle_err=err_against(chk, ref)))
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    write_npz(os.path.join(HERE, "golden_extreme.npz"), out)
    with open(os.path.join(HERE, "golden_extreme.json"), "w") as f:
        json.dump(dict(species=X.species_ids(), n_cells=X.N_CELLS, cases=cases), f, indent=1)
        f.write("\n")
    sizes = [os.path.getsize(os.path.join(HERE, n)) for n in ("golden_extreme.npz", "golden_extreme.json")]
    print("wrote golden_extreme.npz (%d bytes), golden_extreme.json (%d bytes); worst oracle error %.3e" % (
        sizes[0], sizes[1], max(c["oracle_err"] for c in cases)))


if __name__ == "__main__":
    main()
