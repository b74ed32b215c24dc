#!/usr/bin/env python3
"""The anisotropic-hydro particle sampler (is3d_sample_particles_vah) beside the viscous-hydro one (is3d_sample_particles, df_mode 1) on
surfaces of the same size in one process: 1e6 synthetic cells x 20 events x the 305-species list by default.  Both go through the
host-pointer entries (count-only call, then the fill call with a buffer of that size); the figures are the device times the library reports
for the fill call -- ms_prep (density integrals + cell records), ms_count (Poisson numbers, compaction, count pass, scan) and ms_fill -- the
median over --steps after --warmup, and the cell-events per second of their sum.  Writes profiles/r17_sampler_vah.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from is3d_amd import api, inputs, synth  # noqa: E402

KEYS = ("ms_h2d", "ms_prep", "ms_density", "ms_poisson", "ms_count", "ms_fill")


def timed(call, steps, warmup):
    """call(capacity) -> (list, stats); the count-only call sizes the buffer once"""
    _, st = call(0)
    cap = st["n_particles"]
    rows, wall = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        got, st = call(cap)
        dt = time.perf_counter() - t0
        assert len(got) == cap
        if i >= warmup:
            rows.append(st)
            wall.append(dt)
    med = {k: statistics.median(r[k] for r in rows) for k in KEYS}
    med["wall_s"] = statistics.median(wall)
    med.update(n_particles=cap, n_hadrons_drawn=rows[-1]["n_hadrons_drawn"], n_momentum_samples=rows[-1]["n_momentum_samples"],
               n_classes=rows[-1]["n_classes"])
    return med


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--species", default="urqmd", choices=["urqmd", "pikp"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20260017)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_sampler_vah.json"))
    a = ap.parse_args()
    sp = inputs.species(a.species)
    gla = inputs.feqmod_tables(0.15)
    df = inputs.df_tables()
    vah = synth.synth_vah_surface(a.cells, 3)
    visc = synth.synth_surface(a.cells, 3)
    o = dict(dimension=3)
    res = {}
    res["vah"] = timed(lambda cap: api.sample_particles_vah(vah, sp, gla, o, n_events=a.events, seed=a.seed, capacity=cap), a.steps, a.warmup)
    res["viscous_df_mode_1"] = timed(lambda cap: api.sample_particles(visc, sp, df, gla, dict(o, df_mode=1), n_events=a.events, seed=a.seed, capacity=cap),
                                     a.steps, a.warmup)
    for r in res.values():
        r["ms_step"] = r["ms_prep"] + r["ms_count"] + r["ms_fill"]
        r["cell_events_per_s"] = a.cells * a.events / (r["ms_step"] * 1e-3)
    out = dict(what="is3d_sample_particles_vah beside is3d_sample_particles (df_mode 1): device ms of one fill call (median of %d, %d warm-up)" % (a.steps, a.warmup),
               cells=a.cells, events=a.events, species=len(sp["mass"]), dimension=3, surfaces="synth_vah_surface / synth_surface, default seed",
               results=res, ratio_vah_over_viscous={k: res["vah"][k] / res["viscous_df_mode_1"][k] for k in ("ms_prep", "ms_count", "ms_fill", "ms_step")})
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
