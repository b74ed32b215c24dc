"""The test_sampler = 1 distributions of the sampler, two routes on the `config5-sampler` shape of bench.py (cells, events and seed are read
from bench.py, not restated), in one process, alternating, medians after a warm-up:

  (a) list:   is3d_sampler_plan_execute into a full device list + the device-to-host copy of the list + is3d_sampler_bin_list on the host
              (the count-only pass that sizes the list is NOT in the time: the buffer is allocated once, before the window)
  (b) binned: is3d_sampler_plan_execute_binned (fill per event batch into the plan's workspace, cf_sampler_bins, drop)

and the bin kernel's two forms (global atomics | workgroup-private) on pi/K/p, where both can run.  One JSON line.

  python tools/bench_sampler_bins.py [--steps 5] [--warmup 2] [--cells N] [--events N] [--out FILE]

Times are host clocks around calls that end in a device synchronise (both entries return when their result is on the host); ms_bin and
ms_fill are device events from is3d_sampler_stats.  Peak device bytes: torch.cuda.mem_get_info before / at the lowest free memory seen after each
route's first step (the library allocates with hipMalloc, outside torch's allocator)."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from is3d_amd import api, inputs, synth  # noqa: E402

# the reference's shipped bins (iS3D_parameters.dat)
SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)


def bench_shape():
    """cells, events and seed of bench.py --workload config5-sampler, from its source."""
    text = open(os.path.join(ROOT, "bench.py")).read()
    body = text[text.index("def bench_sampler("):]
    cells = int(re.search(r"a\.cells or (\d+)", body).group(1))
    seed = int(re.search(r"\n    seed = (\d+)", body).group(1))
    events = int(re.search(r'"--events", type=int, default=(\d+)', text).group(1))
    return cells, events, seed


def used_bytes():
    free, total = torch.cuda.mem_get_info()
    return total - free


def one(species_name, n_cells, n_events, seed, steps, warmup, forms):
    dev = torch.device("cuda:0")
    sp = inputs.species(species_name)
    S = len(sp["mass"])
    df = inputs.df_tables()
    gla = inputs.feqmod_tables(0.15)
    opts = dict(dimension=3, df_mode=2, device=0)
    cells = synth.synth_surface(n_cells, 3)
    tens = {k: torch.from_numpy(cells[k]).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    xy = dict(x_ptr=ptrs["x"], y_ptr=ptrs["y"])
    torch.cuda.synchronize()
    base = used_bytes()
    res = dict(species=S, cells=n_cells, events=n_events)

    # (b) first: its peak is measured before the list buffer exists
    plan_b = api.SamplerPlan(sp, df, gla, opts, max_cells=n_cells)
    hist_b, st_b = plan_b.execute_binned(n_cells, ptrs, n_events, seed, SHIPPED_BINS, S, **xy)
    peak_b = used_bytes() - base
    plan_a = api.SamplerPlan(sp, df, gla, opts, max_cells=n_cells)
    count, _ = plan_a.execute(n_cells, ptrs, n_events, seed, **xy)
    buf = torch.zeros(max(count, 1) * api.PARTICLE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    host = torch.empty(max(count, 1) * api.PARTICLE_DTYPE.itemsize, dtype=torch.uint8).pin_memory()
    plan_a.execute(n_cells, ptrs, n_events, seed, particles_ptr=buf.data_ptr(), capacity=count, **xy)
    peak_a = used_bytes() - base - peak_b

    def route_a():
        t0 = time.perf_counter()
        n, st = plan_a.execute(n_cells, ptrs, n_events, seed, particles_ptr=buf.data_ptr(), capacity=count, **xy)
        t1 = time.perf_counter()
        host.copy_(buf)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        plist = np.frombuffer(host.numpy(), dtype=api.PARTICLE_DTYPE)[:n]
        h = api.sampler_bin_list(SHIPPED_BINS, n_events, S, plist)
        t3 = time.perf_counter()
        return h, st, dict(ms=(t3 - t0) * 1e3, ms_execute=(t1 - t0) * 1e3, ms_d2h=(t2 - t1) * 1e3, ms_host_bin=(t3 - t2) * 1e3, ms_fill=st["ms_fill"])

    def route_b(form):
        t0 = time.perf_counter()
        h, st = plan_b.execute_binned(n_cells, ptrs, n_events, seed, dict(SHIPPED_BINS, kernel_form=form), S, **xy)
        return h, st, dict(ms=(time.perf_counter() - t0) * 1e3, ms_bin=st["ms_bin"], ms_fill=st["ms_fill"])

    runs = {"list": []}
    runs.update({"binned_form%d" % f: [] for f in forms})
    h_a = None
    for i in range(warmup + steps):                         # alternating, so that drift hits every route alike
        h_a, _, t = route_a()
        if i >= warmup:
            runs["list"].append(t)
        for f in forms:
            h, st_b, t = route_b(f)
            assert all(np.array_equal(h[k], hist_b[k]) for k in h), f
            if i >= warmup:
                runs["binned_form%d" % f].append(t)
    res["particles"] = int(count)
    res["same_counts_as_list"] = bool(all(np.array_equal(h_a[k], hist_b[k]) for k in ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield")))
    res["max_vn_step_difference"] = int(max(np.abs(h_a[k] - hist_b[k]).max() for k in ("vn_re", "vn_im")))
    for name, rows in runs.items():
        res[name] = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
        res[name]["ms_runs"] = [r["ms"] for r in rows]
    res["list"]["peak_device_bytes"] = int(peak_a)
    res["list"]["host_list_bytes"] = int(count) * api.PARTICLE_DTYPE.itemsize
    for f in forms:
        res["binned_form%d" % f]["peak_device_bytes"] = int(peak_b)
    res["particle_workspace_bytes"] = int(st_b["particle_workspace_bytes"])
    plan_a.close()
    plan_b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--events", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cells, events, seed = bench_shape()
    cells, events = a.cells or cells, a.events or events
    steps, warmup = max(1, a.steps), max(0, a.warmup)
    res = dict(workload="sampler_bins (config5-sampler shape of bench.py)", device=torch.cuda.get_device_name(0), bins=SHIPPED_BINS,
               kernel_forms={"0": "the shipped choice", "1": "global 64-bit atomics", "2": "workgroup-private histograms in LDS, one flush"},
               urqmd=one("urqmd", cells, events, seed, steps, warmup, [0]),
               pikp=one("pikp", cells, events, seed, steps, warmup, [1, 2]))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
