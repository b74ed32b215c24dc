"""Per-event flow records on the device (cf_sampler_flow, cf_decay_mc_flow) beside what they replace, on the `config5-sampler` surface of
bench.py (cells and seed read from bench.py) with 20 events, the urqmd species list and the default cuts, in one process, alternating, medians
after a warm-up:

  flow pass   ms_bin of is3d_sampler_plan_execute_flow (device events around cf_sampler_flow, summed over the event batches) for
              4 slots (pi+, K+, p, everything else) in the global form (1) and the workgroup-private form (2), and for 305 slots (one per
              species: no window fits, global form).  In the developer build (IS3D_USE_DEV_LIB=1) the private form also runs with the
              per-wave combine in front of its LDS adds (IS3D_FLOW_PRIVATE_COMBINE=1), the A/B of DESIGN.md section 3r.
  yardstick   ms_bin of is3d_sampler_plan_execute_binned on the same list: cf_sampler_bins, what a pass over this list costs today.
  decay pass  ms_bin of cf_decay_mc_flow (3 slots: pi+, K+, p of the final particles), forms 1 and 2.
  whole call  wall time of is3d_sample_flow (host pointers in, records out) against the list route: is3d_sample_particles (the list moved to
              the host) followed by is3d_flow_list on the host.

One JSON line, printed and written to --out.

  python tools/bench_flow.py [--steps 5] [--warmup 2] [--cells N] [--events 20] [--out profiles/r27_flow.json]"""
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

from bench_decays_mc import read_list  # noqa: E402
from bench_sampler_bins import SHIPPED_BINS, bench_shape  # noqa: E402
from is3d_amd import api, inputs, synth  # noqa: E402

CUTS = dict(api.FLOW_CUTS)


def med(rows):
    return dict(median=statistics.median(rows), min=min(rows), max=max(rows), runs=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_flow.json"))
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
    slot4 = np.array([{211: 0, 321: 1, 2212: 2}.get(i, 3) for i in ids], dtype=np.int32)
    slot305 = np.arange(S, dtype=np.int32)
    table = read_list("urqmd")[0]
    slot_d, ids_d = api.stable_slots(table, [211, 321, 2212])
    plan = api.SamplerPlan(sp, df, gla, opts, max_cells=n_cells)
    dtable = api.DecayMcTable(table, sp["mc_id"], device=0)

    def flow(slot, n_slots, form, decayed=False):
        cuts = dict(CUTS, kernel_form=form)
        if decayed:
            r, rd, st, dst = plan.execute_flow(n_cells, ptrs, n_events, seed, cuts, slot, n_slots, table=dtable, slot_decayed=slot_d,
                                               n_slots_decayed=len(ids_d), **xy)
            return (r, rd), dict(ms_flow=st["ms_bin"], ms_decay_flow=dst["ms_bin"], n_final=dst["n_final"])
        r, st = plan.execute_flow(n_cells, ptrs, n_events, seed, cuts, slot, n_slots, **xy)
        return (r,), dict(ms_flow=st["ms_bin"], ms_fill=st["ms_fill"], n_particles=st["n_particles"])

    def bins():
        h, st = plan.execute_binned(n_cells, ptrs, n_events, seed, SHIPPED_BINS, S, **xy)
        return dict(ms_bin=st["ms_bin"], ms_fill=st["ms_fill"])

    cases = {"flow_4slots_form1": lambda: flow(slot4, 4, 1), "flow_4slots_form2": lambda: flow(slot4, 4, 2),
             "flow_305slots_form1": lambda: flow(slot305, S, 1), "flow_305slots_form0": lambda: flow(slot305, S, 0),
             "decay_flow_form1": lambda: flow(slot4, 4, 1, True), "decay_flow_form2": lambda: flow(slot4, 4, 2, True)}
    if api.DEV_LIB:
        def with_combine():
            os.environ["IS3D_FLOW_PRIVATE_COMBINE"] = "1"
            try:
                return flow(slot4, 4, 2)
            finally:
                del os.environ["IS3D_FLOW_PRIVATE_COMBINE"]
        cases["flow_4slots_form2_with_combine"] = with_combine
    rows = {k: [] for k in cases}
    rows["cf_sampler_bins"] = []
    first = {}
    same = True
    for i in range(warmup + steps):                         # alternating, so that drift hits every case alike
        t = bins()
        if i >= warmup:
            rows["cf_sampler_bins"].append(t)
        for k, fn in cases.items():
            rec, t = fn()
            key = "4" if "4slots" in k else "305" if "305" in k else "decay"
            first.setdefault(key, rec)
            same = same and all(np.array_equal(x[f], y[f]) for x, y in zip(rec, first[key]) for f in x)
            if i >= warmup:
                rows[k].append(t)
    res = dict(workload="flow records (config5-sampler surface of bench.py, urqmd list, default cuts)", device=torch.cuda.get_device_name(0),
               dev_lib=bool(api.DEV_LIB), cells=n_cells, events=n_events, species=S, cuts=CUTS, particles=rows["flow_4slots_form1"][0]["n_particles"],
               same_bits_across_forms_and_repeats=bool(same))
    for k, r in rows.items():
        res[k] = {f: med([x[f] for x in r]) for f in r[0] if f.startswith("ms_")}
    res["decay_n_final"] = rows["decay_flow_form1"][0]["n_final"]

    # the whole host-pointer call against the list route
    whole, listr = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        rec, st = api.sample_flow(cells, sp, df, gla, CUTS, slot4, 4, opts, n_events=n_events, seed=seed)
        t1 = time.perf_counter()
        plist, _ = api.sample_particles(cells, sp, df, gla, opts, n_events=n_events, seed=seed)
        t2 = time.perf_counter()
        want = api.flow_list(CUTS, n_events, 4, slot4, plist)
        t3 = time.perf_counter()
        if i >= warmup:
            whole.append((t1 - t0) * 1e3)
            listr.append(dict(ms=(t3 - t1) * 1e3, ms_sample_particles=(t2 - t1) * 1e3, ms_flow_list_host=(t3 - t2) * 1e3))
    res["same_M_as_list_route"] = bool(np.array_equal(rec["M"], want["M"]))
    res["max_Q_difference_from_list_route"] = int(max(np.abs(rec[k] - want[k]).max() for k in ("Q_re", "Q_im")))
    res["wall_ms_sample_flow"] = med(whole)
    res["wall_ms_list_route"] = {f: med([x[f] for x in listr]) for f in listr[0]}
    res["list_bytes"] = int(len(plist)) * api.PARTICLE_DTYPE.itemsize
    c = api.flow_cumulants(api.flow_merge(rec, [0, 0, 0, 0], 1))
    res["all_hadrons"] = dict(v2_2=float(c["v2"][0][1]), v2_4=float(c["v4"][0][1]), v2_gap=float(c["v2_gap"][0][1]), v2_rp=float(c["v_rp"][0][1]),
                              mean_M=float(c["mean_M"][0]), var_M=float(c["var_M"][0]))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
