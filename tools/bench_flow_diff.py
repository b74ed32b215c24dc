"""Differential flow records on the device (cf_sampler_flow_diff, the differential sink of cf_decay_mc_flow) beside what they extend and what
they replace, on the list of profiles/r27_flow.json: the `config5-sampler` surface of bench.py (cells and seed read from bench.py) with 20
events, the urqmd species list and the default cuts; 4 slots (pi+, K+, p, everything else) x 14 pT bins.  One process, alternating, medians
after a warm-up:

  diff pass   ms_bin of is3d_sampler_plan_execute_flow_diff (device events around cf_sampler_flow_diff, summed over the event batches) in the
              global form (1) and the workgroup-private form (2).  In the developer build (IS3D_USE_DEV_LIB=1) the private form also runs
              with the per-wave combine in front of its LDS adds (IS3D_FLOW_DIFF_PRIVATE_COMBINE=1), the A/B of DESIGN.md section 3u.
  beside it   ms_bin of is3d_sampler_plan_execute_flow (cf_sampler_flow) on the same list, 4 slots, forms 1 and 2.
  decay pass  ms_bin of cf_decay_mc_flow on the differential sink (3 slots x 14 bins of the final particles), forms 1 and 2.
  whole call  wall time of is3d_sample_flow_diff (host pointers in, records out) against the list route: is3d_sample_particles (the list
              moved to the host) followed by is3d_flow_diff_list on the host.

One JSON line, printed and written to --out.

  python tools/bench_flow_diff.py [--steps 5] [--warmup 2] [--cells N] [--events 20] [--out profiles/r30_flow_diff.json]"""
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
from bench_sampler_bins import bench_shape  # noqa: E402
from is3d_amd import api, inputs, synth  # noqa: E402

CUTS = dict(api.FLOW_CUTS)
N_PT = 14
EDGES = api.flow_diff_edges(CUTS["pT_min"], CUTS["pT_max"], N_PT)


def med(rows):
    return dict(median=statistics.median(rows), min=min(rows), max=max(rows), runs=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_flow_diff.json"))
    a = ap.parse_args()
    n_cells, _, seed = bench_shape()
    n_cells, n_events = a.cells or n_cells, a.events
    steps, warmup = max(1, a.steps), max(0, a.warmup)
    dev = torch.device("cuda:0")
    sp, df, gla = inputs.species("urqmd"), inputs.df_tables(), inputs.feqmod_tables(0.15)
    opts = dict(dimension=3, df_mode=2, device=0)
    cells = synth.synth_surface(n_cells, 3)
    tens = {k: torch.from_numpy(cells[k]).to(dev) for k in list(synth.CELL_FIELDS) + ["x", "y"]}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    xy = dict(x_ptr=ptrs["x"], y_ptr=ptrs["y"])
    ids = [int(i) for i in sp["mc_id"]]
    slot4 = np.array([{211: 0, 321: 1, 2212: 2}.get(i, 3) for i in ids], dtype=np.int32)
    table = read_list("urqmd")[0]
    slot_d, ids_d = api.stable_slots(table, [211, 321, 2212])
    plan = api.SamplerPlan(sp, df, gla, opts, max_cells=n_cells)
    dtable = api.DecayMcTable(table, sp["mc_id"], device=0)

    def diff(form, decayed=False):
        cuts = dict(CUTS, kernel_form=form)
        if decayed:
            r, rd, st, dst = plan.execute_flow_diff(n_cells, ptrs, n_events, seed, cuts, EDGES, slot4, 4, table=dtable, slot_decayed=slot_d,
                                                    n_slots_decayed=len(ids_d), **xy)
            return (r, rd), dict(ms_flow_diff=st["ms_bin"], ms_decay_flow_diff=dst["ms_bin"], n_final=dst["n_final"])
        r, st = plan.execute_flow_diff(n_cells, ptrs, n_events, seed, cuts, EDGES, slot4, 4, **xy)
        return (r,), dict(ms_flow_diff=st["ms_bin"], ms_fill=st["ms_fill"], n_particles=st["n_particles"])

    def flow(form):
        r, st = plan.execute_flow(n_cells, ptrs, n_events, seed, dict(CUTS, kernel_form=form), slot4, 4, **xy)
        return (r,), dict(ms_flow=st["ms_bin"], ms_fill=st["ms_fill"])

    cases = {"diff_form1": lambda: diff(1), "diff_form2": lambda: diff(2), "flow_form1": lambda: flow(1), "flow_form2": lambda: flow(2),
             "decay_diff_form1": lambda: diff(1, True), "decay_diff_form2": lambda: diff(2, True)}
    if api.DEV_LIB:
        def with_combine():
            os.environ["IS3D_FLOW_DIFF_PRIVATE_COMBINE"] = "1"
            try:
                return diff(2)
            finally:
                del os.environ["IS3D_FLOW_DIFF_PRIVATE_COMBINE"]
        cases["diff_form2_with_combine"] = with_combine
    rows = {k: [] for k in cases}
    first = {}
    same = True
    for i in range(warmup + steps):                         # alternating, so that drift hits every case alike
        for k, fn in cases.items():
            rec, t = fn()
            key = "decay" if k.startswith("decay") else k.split("_")[0]
            first.setdefault(key, rec)
            same = same and all(np.array_equal(x[f], y[f]) for x, y in zip(rec, first[key]) for f in x)
            if i >= warmup:
                rows[k].append(t)
    sums = {"M": first["diff"][0]["m"].sum(axis=2), "Q_re": first["diff"][0]["p_re"].sum(axis=2), "Q_im": first["diff"][0]["p_im"].sum(axis=2)}
    res = dict(workload="differential flow records (config5-sampler surface of bench.py, urqmd list, default cuts, 4 slots x 14 pT bins)",
               device=torch.cuda.get_device_name(0), dev_lib=bool(api.DEV_LIB), cells=n_cells, events=n_events, species=len(ids), cuts=CUTS, n_pT=N_PT,
               particles=rows["diff_form1"][0]["n_particles"], same_bits_across_forms_and_repeats=bool(same),
               bins_add_up_to_cf_sampler_flow=bool(all(np.array_equal(sums[k], first["flow"][0][k]) for k in sums)))
    for k, r in rows.items():
        res[k] = {f: med([x[f] for x in r]) for f in r[0] if f.startswith("ms_")}
    res["decay_n_final"] = rows["decay_diff_form1"][0]["n_final"]

    # the whole host-pointer call against the list route
    whole, listr = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        rec, st = api.sample_flow_diff(cells, sp, df, gla, CUTS, EDGES, slot4, 4, opts, n_events=n_events, seed=seed)
        t1 = time.perf_counter()
        plist, _ = api.sample_particles(cells, sp, df, gla, opts, n_events=n_events, seed=seed)
        t2 = time.perf_counter()
        want = api.flow_diff_list(CUTS, EDGES, n_events, 4, slot4, plist)
        t3 = time.perf_counter()
        if i >= warmup:
            whole.append((t1 - t0) * 1e3)
            listr.append(dict(ms=(t3 - t1) * 1e3, ms_sample_particles=(t2 - t1) * 1e3, ms_flow_diff_list_host=(t3 - t2) * 1e3))
    res["same_m_as_list_route"] = bool(np.array_equal(rec["m"], want["m"]))
    res["max_p_difference_from_list_route"] = int(max(np.abs(rec[k] - want[k]).max() for k in ("p_re", "p_im")))
    res["wall_ms_sample_flow_diff"] = med(whole)
    res["wall_ms_list_route"] = {f: med([x[f] for x in listr]) for f in listr[0]}
    res["list_bytes"] = int(len(plist)) * api.PARTICLE_DTYPE.itemsize
    all_slots = {k: v.sum(axis=1, keepdims=True) for k, v in rec.items()}
    c = api.flow_diff_cumulants(all_slots)
    res["all_hadrons_v2_of_pT"] = dict(pT_edges=[float(x) for x in EDGES], v2_2=[float(x) for x in c["v2"][0, :, 1]], v2_4=[float(x) for x in c["v4"][0, :, 1]],
                                       v2_gap=[float(x) for x in c["v2_gap"][0, :, 1]], sum_m=[float(x) for x in c["sum_m"][0]])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
