#!/usr/bin/env python3
"""The anisotropic-hydro sampler's test_sampler = 1 histograms, two routes on the same cells and seed in one process on one MI355X,
alternating, medians after a warm-up:

  (a) list:  is3d_sample_particles_vah into a host list (count pass, scan, fill pass, the copy of the list; the buffer is sized by a count-only
             call BEFORE the window) + is3d_sampler_bin_list_device of that list (upload, cf_sampler_bins, download).  The code of the list
             route is the yardstick.
  (b) fused: is3d_sample_binned_vah (Poisson, select, one sample-and-bin pass per event batch; no list)

once with pi+ K+ p pbar (the histogram block fits the LDS: workgroup-private form by default) and once with the 305-species list (global
form), at the shipped bins, coefficients from the tables, synth.synth_vah_surface with bulkPi * 0.02.  Where both forms can run (pi/K/p) the
fused route is also timed with kernel_form = 1.  One JSON line; --out FILE also writes it (profiles/r19_sampler_vah_bins.json).

  python tools/bench_sampler_vah_bins.py [--cells 1000000] [--events 20] [--steps 5] [--warmup 1] [--volume 1.0] [--out FILE]

ms_prep, ms_poisson, ms_count, ms_fill and ms_bin are device events from is3d_sampler_stats; the wall times are host clocks around calls that
return when their result is on the host.  Device bytes: the lowest free memory torch.cuda.mem_get_info shows while a route's first step runs,
polled from a second thread (the library allocates with hipMalloc, outside torch's allocator), against the free memory before it."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from is3d_amd import api, inputs, synth  # noqa: E402

SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)             # iS3D_parameters.dat as shipped
BULK_SCALE = 0.02


class PeakBytes:
    """device bytes in use above the level at entry, polled while the body runs"""

    def __enter__(self):
        torch.cuda.synchronize()
        self.free0 = torch.cuda.mem_get_info()[0]
        self.low = self.free0
        self.stop = False
        self.t = threading.Thread(target=self.poll)
        self.t.start()
        return self

    def poll(self):
        while not self.stop:
            self.low = min(self.low, torch.cuda.mem_get_info()[0])
            time.sleep(0.0005)

    def __exit__(self, *exc):
        self.stop = True
        self.t.join()
        self.bytes = int(self.free0 - self.low)


def med(rows, key):
    return statistics.median(r[key] for r in rows)


def spread(rows, key):
    v = [r[key] for r in rows]
    return max(v) - min(v)


def one(species, cells, tab, gla, n_events, seed, steps, warmup):
    sp = inputs.species(species)
    S = len(sp["mass"])
    o = dict(dimension=3, device=0)
    kw = dict(tab=tab, n_events=n_events, seed=seed)
    layout_words = S * sum(SHIPPED_BINS[k] for k in ("y_bins", "eta_bins", "pT_bins", "tau_bins", "r_bins")) + 2 * api.VN_HARMONICS * S * SHIPPED_BINS["pT_bins"]
    private_fits = layout_words * 8 <= 65536

    def fused(form):
        t0 = time.perf_counter()
        h, st = api.sample_binned_vah(cells, sp, gla, dict(SHIPPED_BINS, kernel_form=form), o, **kw)
        return h, dict(wall_ms=1e3 * (time.perf_counter() - t0), ms_prep=st["ms_prep"], ms_poisson=st["ms_poisson"], ms_bin=st["ms_bin"],
                       ms_h2d=st["ms_h2d"], n=st["n_particles"])

    _, count = api.sample_particles_vah(cells, sp, gla, o, capacity=0, **kw)          # sizes the list, outside every window
    n_list = count["n_particles"]

    def listed():
        t0 = time.perf_counter()
        plist, st = api.sample_particles_vah(cells, sp, gla, o, capacity=n_list, **kw)
        t1 = time.perf_counter()
        h, _ = api.sampler_bin_list_device(SHIPPED_BINS, n_events, S, plist)
        t2 = time.perf_counter()
        return h, dict(wall_sample_ms=1e3 * (t1 - t0), wall_bin_ms=1e3 * (t2 - t1), wall_ms=1e3 * (t2 - t0), ms_prep=st["ms_prep"],
                       ms_poisson=st["ms_poisson"], ms_count=st["ms_count"], ms_fill=st["ms_fill"], ms_h2d=st["ms_h2d"], n=len(plist))

    with PeakBytes() as pf:
        h_f, _ = fused(0)
    with PeakBytes() as pl:
        h_l, _ = listed()
    equal = all(np.array_equal(h_f[k], h_l[k]) for k in h_f)
    forms = [0] + ([1] if private_fits else [])
    rows = {("fused", f): [] for f in forms}
    rows["list"] = []
    for step in range(warmup + steps):
        for f in forms:
            _, r = fused(f)
            if step >= warmup:
                rows[("fused", f)].append(r)
        _, r = listed()
        if step >= warmup:
            rows["list"].append(r)
    out = dict(species=S, histogram_words=layout_words, default_form="workgroup-private" if private_fits else "global", hadrons=int(n_list),
               hadrons_drawn=int(count["n_hadrons_drawn"]), histograms_equal_bit_for_bit=bool(equal), list_bytes=int(n_list) * api.PARTICLE_DTYPE.itemsize,
               fused_peak_device_bytes=pf.bytes, list_peak_device_bytes=pl.bytes)
    f0 = rows[("fused", 0)]
    out["fused"] = {k: med(f0, k) for k in ("wall_ms", "ms_prep", "ms_poisson", "ms_bin", "ms_h2d")}
    out["fused"]["ms_bin_spread"] = spread(f0, "ms_bin")
    if private_fits:
        f1 = rows[("fused", 1)]
        out["fused_global_form"] = dict(wall_ms=med(f1, "wall_ms"), ms_bin=med(f1, "ms_bin"), ms_bin_spread=spread(f1, "ms_bin"))
        out["faster_form"] = "workgroup-private" if out["fused"]["ms_bin"] <= out["fused_global_form"]["ms_bin"] else "global"
    ls = rows["list"]
    out["list"] = {k: med(ls, k) for k in ("wall_ms", "wall_sample_ms", "wall_bin_ms", "ms_prep", "ms_poisson", "ms_count", "ms_fill", "ms_h2d")}
    both = [r["ms_count"] + r["ms_fill"] for r in ls]
    out["list"]["ms_count_plus_fill"] = statistics.median(both)
    out["list"]["ms_count_plus_fill_spread"] = max(both) - min(both)
    out["ms_bin_over_count_plus_fill"] = out["fused"]["ms_bin"] / out["list"]["ms_count_plus_fill"]
    out["wall_fused_over_list"] = out["fused"]["wall_ms"] / out["list"]["wall_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--volume", type=float, default=1.0, help="factor on the synthetic cells' dsigma (hadrons per cell)")
    ap.add_argument("--species", default="pikp,urqmd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cells = {k: np.array(v, dtype=np.float64) for k, v in synth.synth_vah_surface(a.cells, 3, seed=19).items()}
    cells["bulkPi"] = BULK_SCALE * cells["bulkPi"]
    for f in ("dat", "dax", "day", "dan"):
        cells[f] = a.volume * cells[f]
    tab, gla = inputs.vah_df_tables(), inputs.feqmod_tables(0.15)
    names = dict(pikp=[211, 321, 2212, -2212], urqmd="urqmd")
    out = dict(what="is3d_sample_binned_vah (fused sample-and-bin pass) beside is3d_sample_particles_vah + is3d_sampler_bin_list_device (list route): "
                    "medians of %d after %d warm-up, routes alternating in one process" % (a.steps, a.warmup),
               device=torch.cuda.get_device_name(0), cells=a.cells, events=a.events, seed=a.seed, volume=a.volume, bins="shipped", bulk_scale=BULK_SCALE,
               runs=[one(names[s], cells, tab, gla, a.events, a.seed, a.steps, a.warmup) for s in a.species.split(",")])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
