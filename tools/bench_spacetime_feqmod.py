"""Operation 0 with the modified equilibrium (is3d_plan_execute_spacetime_feqmod) on the device-resident plan: ms per stage, the per-cell stage
against the feqmod spectra kernel cf_main_feqmod with culling off (zero_skip = 2) on the same surface in the same process, the bin stage's share
of the step, the df_mode 3 step (records, renormalisation, per-cell stage, linearised delta-f of the breakdown cells, bins) and a bitwise
repeat.  One JSON line per workload on stdout.

  python tools/bench_spacetime_feqmod.py [--workload config3|shipped|all] [--df-modes 4,3] [--steps 5] [--warmup 1] [--out FILE]

Workloads: config3 -- BASELINE config 3's shape (1e6 synthetic 3+1D cells, seed 20260002, 305 urqmd species, 32 x 24 x 21), df_mode 4;
shipped -- the reference's shipped parameters (iS3D_parameters.dat: df_mode 4, dimension 2): 1e5 cells, pi/K/p, 241 eta nodes.
Each workload is timed with df_mode 4 (its own) and again with df_mode 3."""
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

WORKLOADS = dict(config3=dict(dimension=3, species="urqmd", cells=1000000),
                 shipped=dict(dimension=2, species="pikp", cells=100000))


def time_op0(plan, n, ptrs, g, bins, optr, stream, steps, warmup):
    st_all, wall = [], []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = plan.execute_spacetime(n, ptrs, ptrs["x"], ptrs["y"], g["pT_w"], g["phi_w"], bins, optr, stream)
        torch.cuda.synchronize()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            st_all.append(st)
    med = {k: statistics.median(s[k] for s in st_all) for k in ("ms_prep", "ms_cells", "ms_bins")}
    med.update({k: statistics.median(s["feqmod"][k] for s in st_all) for k in ("ms_renorm", "ms_linear")})
    return statistics.median(wall), med, st_all[0]


def run(name, steps, warmup, modes=(4, 3)):
    wl = WORKLOADS[name]
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    sp = inputs.species(wl["species"])
    df = inputs.df_tables()
    n, dim = wl["cells"], wl["dimension"]
    cells = synth.synth_surface(n, dim)
    fq = inputs.feqmod_tables(inputs.surface_average_T(cells))
    r = np.sqrt(cells["x"] ** 2 + cells["y"] ** 2)
    bins = dict(tau_min=float(cells["tau"].min()), tau_max=float(cells["tau"].max()) + 1e-9, tau_bins=40, r_min=0.0, r_max=float(r.max()) + 1e-9,
                r_bins=40)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items() if v is not None}
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    shapes = api.spacetime_shapes(len(sp["mass"]), n, bins, dim, len(g["eta"]))
    outs = {k: torch.zeros(v, dtype=torch.float64, device=dev) for k, v in shapes.items() if k != "dN_dy_cell"}
    optr = {k: v.data_ptr() for k, v in outs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(workload=name, cells=n, dimension=dim, species=len(sp["mass"]), bins=bins, steps=steps, warmup=warmup)
    for dfm in modes:
        opts = dict(dimension=dim, df_mode=dfm)
        plan = api.Plan(sp, grid, df, opts, max_cells=n, fq=fq)
        step, med, st0 = time_op0(plan, n, ptrs, g, bins, optr, stream, steps, warmup)
        res0 = {k: v.cpu().numpy() for k, v in outs.items()}
        plan.execute_spacetime(n, ptrs, ptrs["x"], ptrs["y"], g["pT_w"], g["phi_w"], bins, optr, stream)
        torch.cuda.synchronize()
        same = all(np.array_equal(res0[k], outs[k].cpu().numpy()) for k in outs)
        plan.close()
        # the same surface through the feqmod spectra path, culling off: cf_main_feqmod is the comparison the issue names
        plan2 = api.Plan(sp, grid, df, dict(opts, zero_skip=2), max_cells=n, fq=fq)
        plan2.set_timing(True)
        spec = torch.zeros(plan2.output_size, dtype=torch.float64, device=dev)
        main_nc = []
        for i in range(1 + min(steps, 3)):
            plan2.execute(n, ptrs, spec.data_ptr(), stream)
            torch.cuda.synchronize()
            if i:
                main_nc.append(plan2.timings()["ms_main"])
        plan2.close()
        del spec
        mnc = statistics.median(main_nc)
        total = sum(med.values())
        out["df_mode_%d" % dfm] = dict(step_ms_median=step, stage_ms_median=med, n_passes=st0["n_passes"], classes=st0["n_classes"],
                                       n_cells_breakdown=st0["feqmod"]["n_cells_breakdown"], n_renorm_skipped=st0["feqmod"]["n_renorm_skipped"],
                                       main_feqmod_no_cull_ms=mnc, cells_over_main_no_cull=med["ms_cells"] / mnc,
                                       bins_share_of_step=med["ms_bins"] / total, bitwise_repeat=same)
    out["device"] = torch.cuda.get_device_name(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["all"] + sorted(WORKLOADS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--df-modes", default="4,3", help="comma-separated df_mode list (3, 4)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = sorted(WORKLOADS) if a.workload == "all" else [a.workload]
    for name in names:
        modes = tuple(int(m) for m in a.df_modes.split(",") if m.strip())
        line = json.dumps(run(name, max(1, a.steps), max(0, a.warmup), modes))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
