#!/usr/bin/env python3
"""The host side of the sampler's five multi-device entries on ONE MI355X: wall time around each call with devices = [0, 0] (two cell shards
on one device, a host thread each), after a warm-up, median of --steps with max - min beside it.  The shapes are those of
tools/bench_sampler_fused.py and tools/bench_sampler_vah_bins.py: 1e6 synthetic cells x 20 events, pi K p (anisotropic hydro: pi+ K+ p pbar,
bulkPi * 0.02, coefficients from the tables), 3+1D, the shipped bins.  The list entries fill a buffer sized by a count-only call before the
window.  One JSON line; --out FILE also writes it.

  python tools/bench_sampler_multi.py [--cells 1000000] [--events 20] [--steps 5] [--warmup 1] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from is3d_amd import api, inputs, synth  # noqa: E402

SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)             # iS3D_parameters.dat as shipped
DEVICES = [0, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    df, gla, tab = inputs.df_tables(), inputs.feqmod_tables(0.15), inputs.vah_df_tables()
    cells = synth.synth_surface(a.cells, 3, seed=19)
    vah = {k: np.array(v, dtype=np.float64) for k, v in synth.synth_vah_surface(a.cells, 3, seed=19).items()}
    vah["bulkPi"] = 0.02 * vah["bulkPi"]
    sp, sp4 = inputs.species("pikp"), inputs.species([211, 321, 2212, -2212])
    ov, oa = dict(dimension=3, df_mode=2), dict(dimension=3)
    kw = dict(n_events=a.events, seed=a.seed, devices=DEVICES)
    n_v = api.sample_particles(cells, sp, df, gla, ov, capacity=0, **kw)[1]["n_particles"]
    n_a = api.sample_particles_vah(vah, sp4, gla, oa, tab=tab, capacity=0, **kw)[1]["n_particles"]
    entries = dict(
        is3d_sample_particles_multi=lambda: api.sample_particles(cells, sp, df, gla, ov, capacity=n_v, **kw),
        is3d_sample_binned_multi=lambda: api.sample_binned(cells, sp, df, gla, SHIPPED_BINS, ov, **kw),
        is3d_sample_fused_multi=lambda: api.sample_fused(cells, sp, df, gla, SHIPPED_BINS, ov, **kw),
        is3d_sample_particles_vah_multi=lambda: api.sample_particles_vah(vah, sp4, gla, oa, tab=tab, capacity=n_a, **kw),
        is3d_sample_binned_vah_multi=lambda: api.sample_binned_vah(vah, sp4, gla, SHIPPED_BINS, oa, tab=tab, **kw))
    walls = {name: [] for name in entries}
    for step in range(a.warmup + a.steps):                  # the entries alternate inside a step
        for name, call in entries.items():
            t0 = time.perf_counter()
            _, st = call()
            t = 1e3 * (time.perf_counter() - t0)
            assert st["n_particles"] == (n_a if "vah" in name else n_v), name
            if step >= a.warmup:
                walls[name].append(t)
    out = dict(what="wall ms around each multi-device sampler entry, devices = [0, 0]: median of %d after %d warm-up" % (a.steps, a.warmup),
               device=torch.cuda.get_device_name(0), cells=a.cells, events=a.events, seed=a.seed, hadrons=dict(viscous=n_v, vah=n_a),
               wall_ms={n: dict(median=statistics.median(w), spread=max(w) - min(w)) for n, w in walls.items()})
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
