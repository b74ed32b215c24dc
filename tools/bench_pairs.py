"""Two-particle (delta y, delta phi) histograms on the device (cf_pair_cells, cf_pair_correlate) beside the other passes over the same list, on
the `config5-sampler` surface of bench.py (cells and seed read from bench.py) with 20 events, the urqmd species list and the driver's default
cuts, in one process, alternating, medians of --steps after --warmup:

  per kernel  the device time of cf_pair_cells, cf_pair_correlate, cf_sampler_flow and cf_sampler_bins, summed over one call of the plan's
              execute_pairs / execute_flow / execute_binned (the kernels of all event batches), read from the kernel records of
              torch.profiler; 5 slots (pi+, pi-, K+, p, everything else: 15 classes) at 32 x 32 and at 64 x 64 bins.
  ms_bin      what the library's own events give around the pass over the list (cf_pair_cells, cf_sampler_flow, cf_sampler_bins).
  whole call  wall time of is3d_sample_pairs (host pointers in, histograms out) against the list route: is3d_sample_particles (the list moved
              to the host) followed by is3d_pairs_list on the host (the O(M^2) double loop), 32 x 32 bins.

Not covered: the decay sink (cf_decay_mc_pairs), other slot counts, other surfaces, several devices.

One JSON line, printed and written to --out.

  python tools/bench_pairs.py [--steps 5] [--warmup 2] [--cells N] [--events 20] [--out profiles/r28_pairs.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

from bench_sampler_bins import SHIPPED_BINS, bench_shape  # noqa: E402
from is3d_amd import api, inputs, synth  # noqa: E402

KERNELS = ("cf_pair_cells", "cf_pair_correlate", "cf_sampler_flow", "cf_sampler_bins")


def med(rows):
    return dict(median=statistics.median(rows), min=min(rows), max=max(rows), runs=rows)


def kernel_ms(fn):
    """(result of fn, {kernel: device ms summed over its launches inside fn}) from the profiler's kernel records."""
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    ms = {k: 0.0 for k in KERNELS}
    for e in prof.events():
        for k in KERNELS:
            if k in e.name:
                us = getattr(e, "device_time_total", None)
                if us is None:
                    us = getattr(e, "cuda_time_total", 0.0)
                ms[k] += us / 1e3
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_pairs.json"))
    a = ap.parse_args()
    n_cells, _, seed = bench_shape()
    n_cells, n_events = a.cells or n_cells, a.events
    steps, warmup = max(1, a.steps), max(0, a.warmup)
    dev = torch.device("cuda:0")
    sp, df, gla = inputs.species("urqmd"), inputs.df_tables(), inputs.feqmod_tables(0.15)
    S = len(sp["mass"])
    opts = dict(dimension=3, df_mode=2, device=0)
    cells = synth.synth_surface(n_cells, 3)
    tens = {k: torch.from_numpy(cells[k]).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    xy = dict(x_ptr=ptrs["x"], y_ptr=ptrs["y"])
    ids = [int(i) for i in sp["mc_id"]]
    slot5 = np.array([{211: 0, -211: 1, 321: 2, 2212: 3}.get(i, 4) for i in ids], dtype=np.int32)
    slot4 = np.array([{211: 0, 321: 1, 2212: 2}.get(i, 3) for i in ids], dtype=np.int32)
    bins32, bins64 = dict(api.PAIR_BINS), dict(api.PAIR_BINS, n_y=64, n_phi=64)
    plan = api.SamplerPlan(sp, df, gla, opts, max_cells=n_cells)

    def pairs(bins):
        (h, st), ms = kernel_ms(lambda: plan.execute_pairs(n_cells, ptrs, n_events, seed, bins, slot5, 5, **xy))
        return h, dict(ms_cf_pair_cells=ms["cf_pair_cells"], ms_cf_pair_correlate=ms["cf_pair_correlate"], ms_bin=st["ms_bin"], ms_fill=st["ms_fill"],
                       n_particles=st["n_particles"], accepted=int(h["M"].sum()))

    def flow():
        (r, st), ms = kernel_ms(lambda: plan.execute_flow(n_cells, ptrs, n_events, seed, api.FLOW_CUTS, slot4, 4, **xy))
        return r, dict(ms_cf_sampler_flow=ms["cf_sampler_flow"], ms_bin=st["ms_bin"])

    def binned():
        (h, st), ms = kernel_ms(lambda: plan.execute_binned(n_cells, ptrs, n_events, seed, SHIPPED_BINS, S, **xy))
        return h, dict(ms_cf_sampler_bins=ms["cf_sampler_bins"], ms_bin=st["ms_bin"])

    cases = {"pairs_32x32": lambda: pairs(bins32), "pairs_64x64": lambda: pairs(bins64), "flow_4slots": flow, "bins": binned}
    rows = {k: [] for k in cases}
    first, same = {}, True
    for i in range(warmup + steps):                         # alternating, so that drift hits every case alike
        for k, fn in cases.items():
            out, t = fn()
            if k.startswith("pairs"):
                first.setdefault(k, out)
                same = same and all(np.array_equal(out[f], first[k][f]) for f in out)
            if i >= warmup:
                rows[k].append(t)
    res = dict(workload="pair histograms (config5-sampler surface of bench.py, urqmd list, default cuts, 5 slots)", device=torch.cuda.get_device_name(0),
               cells=n_cells, events=n_events, species=S, bins=bins32, particles=rows["pairs_32x32"][0]["n_particles"],
               accepted=rows["pairs_32x32"][0]["accepted"], same_bits_across_repeats=bool(same))
    for k, r in rows.items():
        res[k] = {f: med([x[f] for x in r]) for f in r[0] if f.startswith("ms_")}
    res["profiler_saw_the_kernels"] = bool(res["pairs_32x32"]["ms_cf_pair_correlate"]["median"] > 0.0)

    # the whole host-pointer call against the list route
    whole, listr = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        h, st = api.sample_pairs(cells, sp, df, gla, bins32, slot5, 5, opts, n_events=n_events, seed=seed)
        t1 = time.perf_counter()
        plist, _ = api.sample_particles(cells, sp, df, gla, opts, n_events=n_events, seed=seed)
        t2 = time.perf_counter()
        want = api.pairs_list(bins32, n_events, 5, slot5, plist)
        t3 = time.perf_counter()
        if i >= warmup:
            whole.append((t1 - t0) * 1e3)
            listr.append(dict(ms=(t3 - t1) * 1e3, ms_sample_particles=(t2 - t1) * 1e3, ms_pairs_list_host=(t3 - t2) * 1e3))
    res["same_as_list_route"] = bool(all(np.array_equal(h[k], want[k]) for k in h))
    res["wall_ms_sample_pairs"] = med(whole)
    res["wall_ms_list_route"] = {f: med([x[f] for x in listr]) for f in listr[0]}
    res["list_bytes"] = int(len(plist)) * api.PARTICLE_DTYPE.itemsize
    res["same_event_pairs"] = int(h["same"].sum())
    c = api.pairs_correlation(bins32, h, gap_bins=8)
    res["pi+pi+"] = dict(V=[float(v) for v in c["V"][0]], n_same=int(c["n_same"][0]), n_mixed=int(c["n_mixed"][0]))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
