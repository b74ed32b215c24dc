#!/usr/bin/env python3
"""Spin polarization sharded over devices (is3d_spin_polarization_multi) at BASELINE config 3's shape (1e6 synthetic 3+1D cells, seed
20260002, vorticity seed 20260005, 305 urqmd species, 32 x 24 x 21), measured on ONE GPU -- what can be said without a multi-GPU box:

  shards     the per-chunk kernel and the chunk reduction of the first 1e6 / 5e5 / 2.5e5 / 1.25e5 cells on the device-resident plan (median of
             --rounds rounds, the sizes alternating inside a round, HIP events).  compute_side_efficiency at N = t(1e6) / (N t(1e6 / N)) --
             PREDICTED from one device, not measured.
  placement  8 shards on the SAME device (no scaling number: they share the card): the placement of the 8 class-sum arrays on devices[0]
             (a device copy here; hipMemcpyPeer between cards is NOT measured), the combine kernel and the read-back, median of --rounds calls.
             share = (placement + combine) / (a 1.25e5-cell shard's cells + reduction + placement + combine).  predicted_speedup_bound at N =
             t_step(1e6) / (t_shard(1e6 / N) + N placement_per_shard + combine): the serial tail every shard count pays.
  single     the host step of the new entry with one shard against is3d_spin_polarization, alternating in one process, median of --rounds;
             the run-to-run spread of the one-shot (max - min over its steps) is what the difference is held against.
  two        only if two GPUs are visible: the MEASURED step on devices [0, 1].

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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    sp = inputs.species("urqmd")
    opts = dict(dimension=3)
    cells = synth.synth_surface(a.total, 3, seed=synth.SEED_CONFIG3)
    w = synth.synth_vorticity(a.total, seed=synth.SEED_VORTICITY)
    T = float(inputs.surface_average_T(cells))
    dev = torch.device("cuda:0")
    med = statistics.median

    # ---- shard sizes on the resident plan ----
    tc = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items()}
    tw = {k: torch.from_numpy(v).to(dev) for k, v in w.items()}
    cp, wp = {k: v.data_ptr() for k, v in tc.items()}, {k: v.data_ptr() for k, v in tw.items()}
    stream = torch.cuda.current_stream().cuda_stream
    sizes = [a.total, a.total // 2, a.total // 4, a.total // 8]
    plans = [api.PolarizationPlan(sp, grid, opts, max_cells=n) for n in sizes]
    outs = {k: torch.zeros(plans[0].output_size, dtype=torch.float64, device=dev) for k in api.POLARIZATION_OUTPUTS}
    op = {k: v.data_ptr() for k, v in outs.items()}
    rec = [dict(ms_cells=[], ms_reduce=[], n_chunks=[]) for _ in sizes]
    for rnd in range(a.rounds + 1):
        for i, n in enumerate(sizes):
            st = plans[i].execute(n, cp, wp, T, op, stream)
            torch.cuda.synchronize()
            if rnd:
                for k in rec[i]:
                    rec[i][k].append(st[k])
    shards = [dict(cells=n, ms_cells=med(rec[i]["ms_cells"]), ms_reduce=med(rec[i]["ms_reduce"]), n_chunks=rec[i]["n_chunks"][0],
                   ms_cells_all=rec[i]["ms_cells"]) for i, n in enumerate(sizes)]
    for p in plans:
        p.close()
    del tc, tw, outs
    torch.cuda.empty_cache()
    step = lambda d: d["ms_cells"] + d["ms_reduce"]   # noqa: E731
    eff = {"N=%d" % (a.total // d["cells"]): step(shards[0]) / ((a.total // d["cells"]) * step(d)) for d in shards[1:]}

    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return (time.perf_counter() - t0) * 1e3, res

    def one_shot():
        return api.spin_polarization(cells, w, sp, grid, T, opts)

    def multi(devices):
        return api.spin_polarization_multi(cells, w, sp, grid, T, opts, devices)

    # ---- placement + combine: 8 shards on one device ----
    multi([0] * 8)
    place, comb, back, step8 = [], [], [], []
    for _ in range(a.rounds):
        ms, r8 = timed(lambda: multi([0] * 8))
        step8.append(ms)
        p = sum(s["ms_d2h"] for s in r8["shard_stats"])
        place.append(p)
        comb.append(r8["stats"]["ms_reduce"] - max(s["ms_reduce"] for s in r8["shard_stats"]))
        back.append(r8["stats"]["ms_d2h"] - p)
    pc = med(place) + med(comb)
    small = shards[-1]
    placement = dict(shards=8, placement_ms=med(place), placement_ms_all=place, combine_ms=med(comb), combine_ms_all=comb,
                     placement_plus_combine_ms=pc, read_back_ms=med(back), host_step_ms=med(step8),
                     class_sums_ms_max=max(s["ms_reduce"] for s in r8["shard_stats"]),
                     share_of_a_125k_cell_shard_step=pc / (step(small) + pc), stats=r8["stats"], shard_stats=r8["shard_stats"],
                     note="the 8 shards share one card: a device copy, not hipMemcpyPeer; not a scaling number")
    bound = {}
    for d in shards[1:]:
        N = a.total // d["cells"]
        bound["N=%d" % N] = step(shards[0]) / (step(d) + N * med(place) / 8 + med(comb))

    # ---- one shard of the new entry against the one-shot, alternating ----
    timed(one_shot), timed(lambda: multi([0]))   # warm-up
    t_one, t_multi = [], []
    for _ in range(a.rounds):
        ms, r1 = timed(one_shot)
        t_one.append(ms)
        ms, rm = timed(lambda: multi([0]))
        t_multi.append(ms)
    same = all(np.array_equal(r1[k], rm[k]) for k in api.POLARIZATION_OUTPUTS)
    single = dict(one_shot_step_ms=med(t_one), one_shot_steps_ms=t_one, one_shot_spread_ms=max(t_one) - min(t_one),
                  multi_1_shard_step_ms=med(t_multi), multi_1_shard_steps_ms=t_multi, difference_ms=med(t_multi) - med(t_one),
                  bitwise_equal=same, one_shot_stats=r1["stats"], multi_stats=rm["stats"])

    def worst(x):
        return max(float(np.max(np.abs(x[k] - r1[k])) / np.max(np.abs(r1[k]))) for k in api.POLARIZATION_OUTPUTS)

    placement["max_error_vs_single_device"] = worst(r8)
    res = dict(what="spin polarization over devices at BASELINE config 3's shape, one MI355X: shard sizes (predicted compute-side efficiency), "
                    "placement + combine of 8 shards on one device, the single-shard route against the one-shot", total_cells=a.total,
               rounds=a.rounds, T=T, shards=shards, compute_side_efficiency_predicted=eff, placement_and_combine=placement,
               predicted_speedup_bound_with_serial_placement_and_combine=bound, single_shard=single,
               gpus_visible=torch.cuda.device_count(), device=torch.cuda.get_device_name(0))
    if torch.cuda.device_count() >= 2:
        multi([0, 1])
        t2 = []
        for _ in range(a.rounds):
            ms, r2 = timed(lambda: multi([0, 1]))
            t2.append(ms)
        res["two_devices_MEASURED"] = dict(step_ms=med(t2), steps_ms=t2, stats=r2["stats"], shard_stats=r2["shard_stats"],
                                           max_error_vs_single_device=worst(r2))
    else:
        res["two_devices_MEASURED"] = "not measured on more than one physical GPU"
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
