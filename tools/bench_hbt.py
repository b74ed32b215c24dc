"""HBT correlation histograms on the device (cf_hbt_select, cf_hbt_pairs) against the host double loop, in one process, medians of --steps
after --warmup:

  sampler   the `config5-sampler` surface of bench.py (cells and seed read from bench.py) with 20 events and the urqmd species list, the shape
            of tools/bench_pairs.py; slots pi+, pi-, K+, K-, the driver's default bins (4 x 20^3 bins per slot: kernel_form 2 does not fit,
            form 0 is form 1).  Device time of cf_hbt_select and cf_hbt_pairs summed over one call of the plan's execute_hbt (torch.profiler's
            kernel records), wall time of is3d_sample_hbt (host pointers in, histograms out), and the list route: is3d_sample_particles
            followed by is3d_hbt_list on the host (once).
  one event one oversampled event of --pions accepted pi+ (Gaussian momenta of 0.12 GeV, a 3 fm Gaussian source) through
            is3d_hbt_list_device: kernel_form 1 and 2 at 1 x 14^3 bins (form 2 fits), form 1 at 4 x 20^3; the host double loop on the first
            --host-pions of them (the whole event is --pions^2 pairs on one core), with its pair rate.

Not covered: the decay sink (cf_decay_mc_hbt), other slot counts, several devices.

One JSON line, printed and written to --out.

  python tools/bench_hbt.py [--steps 3] [--warmup 1] [--cells N] [--events 20] [--pions 100000] [--host-pions 20000] [--out profiles/r29_hbt.json]"""
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

from bench_sampler_bins import bench_shape  # noqa: E402
from is3d_amd import api, inputs, synth  # noqa: E402

KERNELS = ("cf_hbt_select", "cf_hbt_pairs")


def med(rows):
    return dict(median=statistics.median(rows), min=min(rows), max=max(rows), runs=rows)


def kernel_ms(fn):
    """(result of fn, {kernel: device ms summed over its launches inside fn}, wall ms of fn) from the profiler's kernel records."""
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
    ms = {k: 0.0 for k in KERNELS}
    for e in prof.events():
        for k in KERNELS:
            if k in e.name:
                us = getattr(e, "device_time_total", None)
                if us is None:
                    us = getattr(e, "cuda_time_total", 0.0)
                ms[k] += us / 1e3
    return out, ms, wall


def one_event(n, seed=7):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=api.PARTICLE_DTYPE)
    p["px"], p["py"], p["pz"] = (0.12 * rng.standard_normal(n) for _ in range(3))
    p["E"] = np.sqrt(0.13957 ** 2 + p["px"] ** 2 + p["py"] ** 2 + p["pz"] ** 2)
    p["x"], p["y"], p["z"] = (3.0 * rng.standard_normal(n) for _ in range(3))
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--pions", type=int, default=100000)
    ap.add_argument("--host-pions", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_hbt.json"))
    a = ap.parse_args()
    n_cells, _, seed = bench_shape()
    n_cells, n_events = a.cells or n_cells, a.events
    steps, warmup = max(1, a.steps), max(0, a.warmup)
    dev = torch.device("cuda:0")
    res = dict(workload="HBT histograms", device=torch.cuda.get_device_name(0))

    # ---- one oversampled event ----
    wide = dict(y_cut=20.0, pT_min=0.0, pT_max=100.0, kT_min=0.0, kT_max=100.0, q_max=0.1)
    p = one_event(a.pions)
    shapes = {"form1_1x14^3": dict(wide, n_kT=1, n_q=14, kernel_form=1), "form2_1x14^3": dict(wide, n_kT=1, n_q=14, kernel_form=2),
              "form1_4x20^3": dict(wide, n_kT=4, n_q=20, kernel_form=1)}
    rows = {k: [] for k in shapes}
    first = {}
    for i in range(warmup + steps):                         # alternating, so that drift hits every case alike
        for k, bins in shapes.items():
            (h, _), ms, wall = kernel_ms(lambda: api.hbt_list_device(bins, 1, 1, [0], p))
            first.setdefault(k, h)
            if i >= warmup:
                rows[k].append(dict(ms_cf_hbt_select=ms["cf_hbt_select"], ms_cf_hbt_pairs=ms["cf_hbt_pairs"], wall_ms=wall))
    ev = dict(pions=int(first["form1_1x14^3"]["M"].sum()), ordered_pairs=a.pions * (a.pions - 1), pairs_in_cube=int(first["form1_1x14^3"]["den"].sum()),
              forms_same_bits=bool(all(np.array_equal(first["form1_1x14^3"][f], first["form2_1x14^3"][f]) for f in ("num", "den", "M"))))
    for k, r in rows.items():
        ev[k] = {f: med([x[f] for x in r]) for f in r[0]}
        ev[k]["pairs_per_s"] = ev["ordered_pairs"] / (ev[k]["ms_cf_hbt_pairs"]["median"] * 1e-3) if ev[k]["ms_cf_hbt_pairs"]["median"] > 0 else None
    sub = p[:a.host_pions]
    t0 = time.perf_counter()
    want = api.hbt_list(shapes["form1_1x14^3"], 1, 1, [0], sub)
    t_host = time.perf_counter() - t0
    got, _ = api.hbt_list_device(shapes["form1_1x14^3"], 1, 1, [0], sub)
    ev["host_loop"] = dict(pions=len(sub), ordered_pairs=len(sub) * (len(sub) - 1), ms=t_host * 1e3, pairs_per_s=len(sub) * (len(sub) - 1) / t_host,
                           device_den_equal=bool(np.array_equal(got["den"], want["den"])), device_num_max_units=int(np.abs(got["num"] - want["num"]).max()))
    res["one_event"] = ev
    res["profiler_saw_the_kernels"] = bool(ev["form1_1x14^3"]["ms_cf_hbt_pairs"]["median"] > 0.0)

    # ---- the sampler's list ----
    sp, df, gla = inputs.species("urqmd"), inputs.df_tables(), inputs.feqmod_tables(0.15)
    opts = dict(dimension=3, df_mode=2, device=0)
    cells = synth.synth_surface(n_cells, 3)
    tens = {k: torch.from_numpy(cells[k]).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    ids = [int(i) for i in sp["mc_id"]]
    slot = np.array([{211: 0, -211: 1, 321: 2, -321: 3}.get(i, -1) for i in ids], dtype=np.int32)
    bins = dict(api.HBT_BINS)
    plan = api.SamplerPlan(sp, df, gla, opts, max_cells=n_cells)
    srows, whole = [], []
    for i in range(warmup + steps):
        (h, st), ms, _ = kernel_ms(lambda: plan.execute_hbt(n_cells, ptrs, n_events, seed, bins, slot, 4, x_ptr=ptrs["x"], y_ptr=ptrs["y"]))
        t0 = time.perf_counter()
        h2, st2 = api.sample_hbt(cells, sp, df, gla, bins, slot, 4, opts, n_events=n_events, seed=seed)
        t1 = time.perf_counter()
        if i >= warmup:
            srows.append(dict(ms_cf_hbt_select=ms["cf_hbt_select"], ms_cf_hbt_pairs=ms["cf_hbt_pairs"], ms_bin=st["ms_bin"]))
            whole.append((t1 - t0) * 1e3)
    plan.close()
    t1 = time.perf_counter()
    plist, _ = api.sample_particles(cells, sp, df, gla, opts, n_events=n_events, seed=seed)
    t2 = time.perf_counter()
    want = api.hbt_list(bins, n_events, 4, slot, plist)
    t3 = time.perf_counter()
    M = h["M"].astype(np.int64)
    res["sampler"] = dict(cells=n_cells, events=n_events, species=len(ids), bins=bins, particles=int(st["n_particles"]), accepted=int(M.sum()),
                          ordered_pairs=int((M * (M - 1)).sum()), pairs_in_cube=int(h["den"].sum()),
                          kernels={f: med([x[f] for x in srows]) for f in srows[0]}, wall_ms_sample_hbt=med(whole),
                          wall_ms_list_route=dict(ms=(t3 - t1) * 1e3, ms_sample_particles=(t2 - t1) * 1e3, ms_hbt_list_host=(t3 - t2) * 1e3),
                          same_den_as_list_route=bool(np.array_equal(h2["den"], want["den"]) and np.array_equal(h2["M"], want["M"])),
                          num_max_units=int(np.abs(h2["num"] - want["num"]).max()))
    r = api.hbt_radii(bins, h, 20, 0.05)
    res["sampler"]["pi+"] = dict(lambda_=[float(v) for v in r["lambda"][0]], R2_out=[float(v) for v in r["R2"][0, :, 0]], n_bins=[int(v) for v in r["n_bins"][0]])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
