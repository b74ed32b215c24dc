#!/usr/bin/env python3
"""The anisotropic-hydro spectra sharded over devices (is3d_smooth_spectra_vah_multi) at BASELINE config 5's shape (1e6 synthetic 3+1D VAH
cells, 305 urqmd species, 32 x 24 x 21, coefficients from the tables), on the devices the machine shows:

  single   is3d_smooth_spectra_vah_df, the host step every list is held against, taken in the same process (median of --steps, its spread)
  lists    [0], [0, 0] and, where the machine has them, [0, 1], [0, 1, 2, 3], ... : the host step, the slowest shard's ms_main, ms_d2h
           (reduction + download), whether the result is bitwise the expected one, and compute_side_efficiency = t_single / (N x the slowest
           shard's prep + main + finalize).  On a list that repeats an ordinal the shards share one device: that figure and the step then
           measure the OVERHEAD of the sharded route (plans, uploads, the tree sum), not scaling.
  alone    the first 1 / N of the cells through the single-device entry, N = 2, 4: what a shard costs with a device to itself, and the
           compute-side efficiency t(n) / (N t(n / N)) PREDICTED from it.

One JSON object on stdout (and in --out)."""
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


def kernels_ms(st):
    return st["ms_prep"] + st["ms_main"] + st["ms_finalize"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    sp, tab = inputs.species("urqmd"), inputs.vah_df_tables()
    opts = dict(dimension=3)
    cells = synth.synth_vah_surface(a.total, 3)
    visible = torch.cuda.device_count()

    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return (time.perf_counter() - t0) * 1e3, res

    def measure(fn):
        fn()   # warm-up
        ts, last = [], None
        for _ in range(a.steps):
            ms, last = timed(fn)
            ts.append(ms)
        return ts, last

    ts, (ref, st1) = measure(lambda: api.smooth_spectra_vah(cells, sp, grid, opts, tab=tab))
    single = dict(step_ms=statistics.median(ts), steps_ms=ts, spread_ms=max(ts) - min(ts), ms_prep=st1["ms_prep"], ms_main=st1["ms_main"],
                  ms_finalize=st1["ms_finalize"], kernels_ms=kernels_ms(st1))

    alone = {}
    for N in (2, 4):
        sub = {k: v[:a.total // N] for k, v in cells.items()}
        ts, (_, st) = measure(lambda: api.smooth_spectra_vah(sub, sp, grid, opts, tab=tab))
        alone["N=%d" % N] = dict(cells=a.total // N, step_ms=statistics.median(ts), ms_main=st["ms_main"], kernels_ms=kernels_ms(st),
                                 compute_side_efficiency_predicted=kernels_ms(st1) / (N * kernels_ms(st)))

    lists = [[0], [0, 0]]
    n = 2
    while n <= visible:
        lists.append(list(range(n)))
        n *= 2
    if visible > 2 and list(range(visible)) not in lists:
        lists.append(list(range(visible)))
    runs = []
    for devices in lists:
        ts, (got, st) = measure(lambda: api.smooth_spectra_vah_multi(cells, sp, grid, opts, devices, tab=tab))
        N = len(devices)
        slowest = max(kernels_ms(t) for t in st["shards"])
        runs.append(dict(devices=devices, distinct_devices=len(set(devices)), step_ms=statistics.median(ts), steps_ms=ts,
                         slowest_shard_ms_main=st["ms_main"], slowest_shard_kernels_ms=slowest, ms_h2d=st["ms_h2d"], ms_d2h=st["ms_d2h"],
                         step_over_single=statistics.median(ts) / single["step_ms"],
                         compute_side_efficiency=single["kernels_ms"] / (N * slowest),
                         measures="scaling" if len(set(devices)) == N and N > 1 else "overhead of the sharded route on one device",
                         bitwise_equal_to_single=bool(np.array_equal(got, ref)),
                         max_rel_difference_from_single=float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-250))),
                         shard_ms_main=[t["ms_main"] for t in st["shards"]]))
    res = dict(what="is3d_smooth_spectra_vah_multi at BASELINE config 5's shape against is3d_smooth_spectra_vah_df in the same process",
               total_cells=a.total, steps=a.steps, single_device=single, shard_alone=alone, lists=runs, gpus_visible=visible,
               distinct_devices_measured=max(r["distinct_devices"] for r in runs), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
