#!/usr/bin/env python3
"""The viscous sampler's test_sampler = 1 histograms, two routes on the same cells and seed in one process on one MI355X, alternating,
medians after a warm-up with max - min beside them:

  (a) binned: is3d_sample_binned / is3d_sampler_plan_execute_binned -- per event batch Poisson, select, count pass, scan, fill pass into a
              particle workspace, cf_sampler_bins over it.  Unchanged code: the yardstick.
  (b) fused:  is3d_sample_fused / is3d_sampler_plan_execute_fused -- per event batch Poisson, select, ONE sample-and-bin pass (cf_sampler_fused)

on three shapes, all at the shipped bins:

  pikp    1e6 synth_surface cells, 3+1D, df_mode 2, pi K p (the block fits the LDS: workgroup-private form), 20 events, host-pointer one-shot
  urqmd   the same cells, 305 species (global form), 20 events, host-pointer one-shot
  shipped 1e5 cells, 2+1D, df_mode 4, fast = 1, pi K p, a persistent plan on device-resident cells running enough events for >= 1e7 hadrons
          (sized by a short fused run before the window)

Every run asserts that the two routes' histograms are equal in counts and yields (and reports whether vn_* are identical too).  One JSON
line; --out FILE also writes it (profiles/r20_sampler_fused.json).

  python tools/bench_sampler_fused.py [--shapes pikp,urqmd,shipped] [--cells 1000000] [--events 20] [--steps 5] [--warmup 1] [--hadrons 1e7] [--out FILE]

ms_prep, ms_poisson, ms_count, ms_fill and ms_bin are device events from is3d_sampler_stats; the wall times are host clocks around calls that
return when their result is on the host.  Device bytes: the lowest free memory torch.cuda.mem_get_info shows while a route's first step runs,
polled from a second thread (the library allocates with hipMalloc, outside torch's allocator), against the free memory before it."""
import argparse
import json
import math
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
COUNTS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield")
KEYS = ("wall_ms", "ms_prep", "ms_poisson", "ms_count", "ms_fill", "ms_bin", "ms_h2d")


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


def timed(call):
    t0 = time.perf_counter()
    h, st = call()
    row = {k: st[k] for k in KEYS if k != "wall_ms"}
    row["wall_ms"] = 1e3 * (time.perf_counter() - t0)
    row["device_ms"] = st["ms_count"] + st["ms_fill"] + st["ms_bin"]
    # the binned route's ms_count holds Poisson + select (ms_poisson is part of it); the fused route reports ms_count = 0, so they are added back
    row["batch_ms"] = row["device_ms"] + (st["ms_poisson"] if st["ms_count"] == 0 else 0.0)
    row["n"] = st["n_particles"]
    row["workspace"] = st["particle_workspace_bytes"]
    return h, row


def compare(routes, steps, warmup):
    """routes: {"fused": call, "binned": call}, each -> (histograms, stats).  First steps under the memory poll, then alternating."""
    peak, first = {}, {}
    for name in ("fused", "binned"):
        with PeakBytes() as pk:
            first[name], _ = timed(routes[name])
        peak[name] = pk.bytes
    rows = dict(fused=[], binned=[])
    for step in range(warmup + steps):
        for name in ("fused", "binned"):
            h, r = timed(routes[name])
            assert all(np.array_equal(h[k], first["binned"][k]) for k in COUNTS), (name, step)     # counts and yields: every run, both routes
            if step >= warmup:
                rows[name].append(r)
    out = dict(hadrons=int(rows["fused"][0]["n"]), counts_and_yields_equal=True,
               vn_identical=bool(all(np.array_equal(first["fused"][k], first["binned"][k]) for k in ("vn_re", "vn_im"))),
               fused_peak_device_bytes=peak["fused"], binned_peak_device_bytes=peak["binned"],
               binned_particle_workspace_bytes=int(rows["binned"][0]["workspace"]))
    assert rows["fused"][0]["n"] == rows["binned"][0]["n"] and rows["fused"][0]["workspace"] == 0
    for name in ("fused", "binned"):
        out[name] = {k: statistics.median(r[k] for r in rows[name]) for k in KEYS + ("device_ms", "batch_ms")}
        for k in ("device_ms", "batch_ms", "wall_ms"):
            v = [r[k] for r in rows[name]]
            out[name][k + "_spread"] = max(v) - min(v)
    out["fused_ms_bin_over_binned_count_fill_bin"] = out["fused"]["device_ms"] / out["binned"]["device_ms"]
    out["fused_over_binned_with_poisson_on_both_sides"] = out["fused"]["batch_ms"] / out["binned"]["batch_ms"]
    out["wall_fused_over_binned"] = out["fused"]["wall_ms"] / out["binned"]["wall_ms"]
    return out


def one_shot(species, cells, n_events, seed, steps, warmup):
    sp, df, gla = inputs.species(species), inputs.df_tables(), inputs.feqmod_tables(0.15)
    S = len(sp["mass"])
    words = S * sum(SHIPPED_BINS[k] for k in ("y_bins", "eta_bins", "pT_bins", "tau_bins", "r_bins")) + 2 * api.VN_HARMONICS * S * SHIPPED_BINS["pT_bins"]
    o = dict(dimension=3, df_mode=2, device=0)
    kw = dict(n_events=n_events, seed=seed)
    out = dict(shape="%d cells x %d events, 3+1D, df_mode 2, one-shot" % (len(cells["T"]), n_events), species=S, histogram_words=words,
               form="workgroup-private" if words * 8 + 24 <= 65536 else "global")
    out.update(compare(dict(fused=lambda: api.sample_fused(cells, sp, df, gla, SHIPPED_BINS, o, **kw),
                            binned=lambda: api.sample_binned(cells, sp, df, gla, SHIPPED_BINS, o, **kw)), steps, warmup))
    return out


def shipped(n_cells, hadrons, seed, steps, warmup):
    """the reference's shipped configuration on a persistent plan: 2+1D, df_mode 4, fast = 1, device-resident cells"""
    cells = synth.synth_surface(n_cells, 2, seed=23)
    sp, df = inputs.species("pikp"), inputs.df_tables()
    gla = inputs.feqmod_tables(inputs.surface_average_T(cells))
    o = dict(dimension=2, df_mode=4, device=0)
    dev = torch.device("cuda:0")
    tens = {k: torch.from_numpy(np.ascontiguousarray(cells[k])).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    xy = dict(x_ptr=ptrs["x"], y_ptr=ptrs["y"])
    plan = api.SamplerPlan(sp, df, gla, o, max_cells=n_cells, fq=gla, fast=1, T_avg=gla["T_avg"], y_cut=SHIPPED_BINS["y_cut"])
    _, probe = plan.execute_fused(n_cells, ptrs, 20, seed, SHIPPED_BINS, 3, **xy)
    n_events = max(20, int(math.ceil(hadrons / max(probe["n_particles"] / 20.0, 1e-9))))
    for _ in range(4):                                   # the 20-event estimate can fall a fraction of a per cent short
        _, sized = plan.execute_fused(n_cells, ptrs, n_events, seed, SHIPPED_BINS, 3, **xy)
        if sized["n_particles"] >= hadrons:
            break
        n_events = int(math.ceil(1.01 * n_events * hadrons / sized["n_particles"]))
    out = dict(shape="%d cells x %d events, 2+1D, df_mode 4, fast = 1, persistent plan" % (n_cells, n_events), species=3, form="workgroup-private")
    out.update(compare(dict(fused=lambda: plan.execute_fused(n_cells, ptrs, n_events, seed, SHIPPED_BINS, 3, **xy),
                            binned=lambda: plan.execute_binned(n_cells, ptrs, n_events, seed, SHIPPED_BINS, 3, **xy)), steps, warmup))
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="pikp,urqmd,shipped")
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--plan-cells", type=int, default=100000)
    ap.add_argument("--hadrons", type=float, default=1e7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    shapes = a.shapes.split(",")
    cells = synth.synth_surface(a.cells, 3, seed=19) if ("pikp" in shapes or "urqmd" in shapes) else None
    runs = []
    for s in shapes:
        runs.append(shipped(a.plan_cells, a.hadrons, a.seed, a.steps, a.warmup) if s == "shipped"
                    else one_shot(s, cells, a.events, a.seed, a.steps, a.warmup))
    out = dict(what="is3d_sample_fused / is3d_sampler_plan_execute_fused (one sample-and-bin pass) beside is3d_sample_binned / "
                    "is3d_sampler_plan_execute_binned (count, scan, fill, bin): medians of %d after %d warm-up, routes alternating in one process; "
                    "device_ms = ms_count + ms_fill + ms_bin (the fused route's ms_count is 0 and leaves Poisson + select out), batch_ms = the same with ms_poisson "
                    "on both sides" % (a.steps, a.warmup),
               device=torch.cuda.get_device_name(0), seed=a.seed, bins="shipped", runs=runs)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
