#!/usr/bin/env python3
"""The anisotropic-hydro mean yield (is3d_total_yield_vah) on 1e6 synthetic cells x the 305-species list (75 classes), 32 Gauss-Laguerre nodes:
the device times the library reports -- ms_cells (coefficient interpolation + the per-cell kernel) and ms_classes (the radial integrals per
(cell, class) and their reduction) -- as medians over --steps calls after --warmup, beside ms_density of one count-only call of the VAH sampler
in the same process (cf_sampler_density does ONE of the three sums per node on the same (cell, class) grid).  Then, on a smaller surface, the
ratio per species of the hadrons the sampler keeps per event to yield_by_species: how far the regulated, outflow-cut sampler sits from the
linear yield that sizes it (printed, not asserted).  bulkPi x 0.02 throughout, so that the linear yields are positive.  Writes
profiles/r18_yield_vah.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from is3d_amd import api, inputs, synth  # noqa: E402

BULK_SCALE = 0.02


def surface(n, dim, volume=1.0):
    v = dict(synth.synth_vah_surface(n, dim))
    v["bulkPi"] = BULK_SCALE * v["bulkPi"]
    for k in ("dat", "dax", "day", "dan"):
        v[k] = volume * v[k]
    return v


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ratio-cells", type=int, default=20000)
    ap.add_argument("--ratio-events", type=int, default=200)
    ap.add_argument("--ratio-volume", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=20260018)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_yield_vah.json"))
    a = ap.parse_args()
    gla = inputs.feqmod_tables(0.15)
    tab = inputs.vah_df_tables()
    o = dict(dimension=3)
    sp = inputs.species("urqmd")
    v = surface(a.cells, 3)
    rows = []
    for i in range(a.warmup + a.steps):
        N, by, st = api.total_yield_vah(v, sp, gla, o, tab=tab)
        if i >= a.warmup:
            rows.append(st)
    med = {k: statistics.median(r[k] for r in rows) for k in ("ms_h2d", "ms_cells", "ms_classes")}
    _, sst = api.sample_particles_vah(v, sp, gla, o, tab=tab, n_events=1, seed=a.seed, capacity=0)      # warm-up
    dens = []
    for _ in range(a.steps):
        _, sst = api.sample_particles_vah(v, sp, gla, o, tab=tab, n_events=1, seed=a.seed, capacity=0)
        dens.append(sst["ms_density"])
    # the sampler against the yield that sizes it
    sp4 = inputs.species([211, 321, 2212, -2212])
    ratio = {}
    for dim in (3, 2):
        w = surface(a.ratio_cells, dim, a.ratio_volume)
        _, by4, _ = api.total_yield_vah(w, sp4, gla, dict(dimension=dim), tab=tab, y_cut=0.5)
        got, _ = api.sample_particles_vah(w, sp4, gla, dict(dimension=dim), tab=tab, n_events=a.ratio_events, seed=a.seed, y_cut=0.5)
        kept = np.bincount(got["species"], minlength=4) / float(a.ratio_events)
        ratio["%d+1D" % dim] = dict(kept_per_event=kept.tolist(), yield_by_species=by4.tolist(), ratio=(kept / by4).tolist())
        print("%d+1D kept hadrons per event / yield_by_species (pi+ K+ p pbar): %s  (kept %s, yield %s)" % (dim, kept / by4, kept, by4))
    out = dict(what="is3d_total_yield_vah: device ms (median of %d, %d warm-up) beside cf_sampler_density of is3d_sample_particles_vah" % (a.steps, a.warmup),
               cells=a.cells, species=len(sp["mass"]), n_classes=rows[-1]["n_classes"], n_gla=len(gla["root1"]), dimension=3,
               surface="synth_vah_surface, default seed, bulkPi x %g, coefficients from the tables" % BULK_SCALE, mean_yield=N,
               n_cells_skipped=rows[-1]["n_cells_skipped"], yield_ms=med, sampler_ms_density=statistics.median(dens),
               ms_classes_over_ms_density=med["ms_classes"] / statistics.median(dens),
               sampler_over_linear_yield=dict(cells=a.ratio_cells, events=a.ratio_events, volume_scale=a.ratio_volume, species=[211, 321, 2212, -2212], **ratio))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
