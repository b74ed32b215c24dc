#!/usr/bin/env python3
"""Operation 0 sharded over devices (is3d_spacetime_distributions_multi) at BASELINE config 3's shape (1e6 synthetic 3+1D cells, seed
20260002, Chapman-Enskog, 305 urqmd species, 32 x 24 x 21), measured on ONE GPU -- what can be said without a multi-GPU box:

  shards   the record writer, the per-cell stage and the bin stage of the first 1e6 / 5e5 / 2.5e5 / 1.25e5 cells on the device-resident plan
           (median of --rounds interleaved rounds, HIP events), in the manner of tools/shard_sizes.py.  compute_side_efficiency at N =
           t(1e6) / (N t(1e6 / N)) of prep + per-cell; the bin stage runs once over all cells whatever N, so
           predicted_speedup_bound at N = t_step(1e6) / (t_shard(1e6 / N) + t_bins(1e6)) -- PREDICTED from one device, not measured.
  single   the host step of the new entry with one shard against is3d_spacetime_distributions, alternating in one process, median of
           --steps; the run-to-run spread of the one-shot (max - min over its steps) is what the difference is held against.
  two-on-one  two shards on the same device: not a scaling number, the cost of the assembled-D route (second plan, D placement).
  two      only if two GPUs are visible: the MEASURED step on devices [0, 1].

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    wg = dict(grid, pT_w=g["pT_w"], phi_w=g["phi_w"])
    sp, df = inputs.species("urqmd"), inputs.df_tables()
    opts = dict(dimension=3, df_mode=2)
    cells = synth.synth_surface(a.total, 3)
    r = np.sqrt(cells["x"] ** 2 + cells["y"] ** 2)
    bins = dict(tau_min=float(cells["tau"].min()), tau_max=float(cells["tau"].max()) + 1e-9, tau_bins=40, r_min=0.0, r_max=float(r.max()) + 1e-9,
                r_bins=40)
    dev = torch.device("cuda:0")

    # ---- shard sizes on the resident plan ----
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items()}
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    stream = torch.cuda.current_stream().cuda_stream
    sizes = [a.total, a.total // 2, a.total // 4, a.total // 8]
    plans, outs = [], []
    for n in sizes:
        plans.append(api.Plan(sp, grid, df, opts, max_cells=n))
        shapes = api.spacetime_shapes(len(sp["mass"]), n, bins, 3, len(g["eta"]))
        outs.append({k: torch.zeros(v, dtype=torch.float64, device=dev) for k, v in shapes.items() if k != "dN_dy_cell"})
    rec = [dict(ms_prep=[], ms_cells=[], ms_bins=[]) for _ in sizes]
    for rnd in range(a.rounds + 1):
        for i, n in enumerate(sizes):
            st = plans[i].execute_spacetime(n, ptrs, ptrs["x"], ptrs["y"], g["pT_w"], g["phi_w"], bins, {k: v.data_ptr() for k, v in outs[i].items()},
                                            stream)
            torch.cuda.synchronize()
            if rnd:
                for k in rec[i]:
                    rec[i][k].append(st[k])
    shards = [dict(cells=n, **{k: statistics.median(v) for k, v in rec[i].items()}) for i, n in enumerate(sizes)]
    for p in plans:
        p.close()
    del t, outs
    torch.cuda.empty_cache()
    base = shards[0]
    step0 = base["ms_prep"] + base["ms_cells"] + base["ms_bins"]
    eff, bound = {}, {}
    for d in shards[1:]:
        N = a.total // d["cells"]
        eff["N=%d" % N] = (base["ms_prep"] + base["ms_cells"]) / (N * (d["ms_prep"] + d["ms_cells"]))
        bound["N=%d" % N] = step0 / (d["ms_prep"] + d["ms_cells"] + base["ms_bins"])

    # ---- one shard of the new entry against the one-shot, alternating ----
    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return (time.perf_counter() - t0) * 1e3, res

    def one_shot():
        return api.spacetime_distributions(cells, sp, wg, df, bins, opts)

    def multi(devices):
        return api.spacetime_distributions_multi(cells, sp, wg, df, bins, opts, devices)

    timed(one_shot), timed(lambda: multi([0]))   # warm-up
    t_one, t_multi = [], []
    for _ in range(a.steps):
        ms, r1 = timed(one_shot)
        t_one.append(ms)
        ms, rm = timed(lambda: multi([0]))
        t_multi.append(ms)
    same = all(np.array_equal(r1[k], rm[k]) for k in api.SPACETIME_OUTPUTS if k in r1)
    single = dict(one_shot_step_ms=statistics.median(t_one), one_shot_steps_ms=t_one, one_shot_spread_ms=max(t_one) - min(t_one),
                  multi_1_shard_step_ms=statistics.median(t_multi), multi_1_shard_steps_ms=t_multi,
                  difference_ms=statistics.median(t_multi) - statistics.median(t_one), bitwise_equal=same,
                  one_shot_stats=r1["stats"], multi_stats=rm["stats"])
    res = dict(what="operation 0 over devices at BASELINE config 3's shape, one MI355X: shard sizes (predicted compute-side efficiency), "
                    "the single-shard route against the one-shot", total_cells=a.total, rounds=a.rounds, steps=a.steps, shards=shards,
               compute_side_efficiency_predicted=eff, predicted_speedup_bound_with_one_bin_stage=bound, single_shard=single,
               gpus_visible=torch.cuda.device_count(), device=torch.cuda.get_device_name(0))
    # two shards on the SAME device: no speed-up to be had, it shows what the assembled-D route costs (second plan, D placement, surface upload)
    multi([0, 0])
    t00 = []
    for _ in range(a.steps):
        ms, r00 = timed(lambda: multi([0, 0]))
        t00.append(ms)
    res["two_shards_on_one_device"] = dict(step_ms=statistics.median(t00), steps_ms=t00, stats=r00["stats"], shard_stats=r00["shard_stats"],
                                           bitwise_equal=all(np.array_equal(r1[k], r00[k]) for k in api.SPACETIME_OUTPUTS if k in r1))
    if torch.cuda.device_count() >= 2:
        multi([0, 1])
        t2 = []
        for _ in range(a.steps):
            ms, r2 = timed(lambda: multi([0, 1]))
            t2.append(ms)
        res["two_devices_MEASURED"] = dict(step_ms=statistics.median(t2), steps_ms=t2, stats=r2["stats"], shard_stats=r2["shard_stats"],
                                           bitwise_equal=all(np.array_equal(r1[k], r2[k]) for k in api.SPACETIME_OUTPUTS if k in r1))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
