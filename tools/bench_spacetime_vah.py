"""Operation 0 for anisotropic hydro (is3d_vah_plan_execute_spacetime) on the device-resident plan: ms per stage (coefficients + records,
per-cell kernel cf_st_vah_cells, bin stage), and beside them ms_main of is3d_vah_plan_execute -- the spectra kernel cf_main_vah3 on the same
cells and grid in the same process, which is the same number of integrand evaluations -- with the ratio ms_cells / ms_main and a bitwise
repeat.  Writes the result as one JSON document.

  python tools/bench_spacetime_vah.py [--workload config5|shipped|all] [--steps 5] [--warmup 1] [--out profiles/r16_spacetime_vah.json]

Workloads: config5 -- BASELINE config 5's shape (1e6 synthetic 3+1D VAH cells, 305 urqmd species, 32 x 24 x 21), coefficients from the VAH
tables; shipped -- the shipped parameters' shape in 2+1D: 1e5 cells, pi/K/p, 241 eta nodes.  No time here is gated by a test."""
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

WORKLOADS = dict(config5=dict(dimension=3, species="urqmd", cells=1000000),
                 shipped=dict(dimension=2, species="pikp", cells=100000))
COEF = ("c0", "c1", "c2", "c3", "c4")


def run(name, steps, warmup, cells_override=None):
    wl = WORKLOADS[name]
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    sp = inputs.species(wl["species"])
    tab = inputs.vah_df_tables()
    n, dim = cells_override or wl["cells"], wl["dimension"]
    cells = synth.synth_vah_surface(n, dim)
    r = np.sqrt(cells["x"] ** 2 + cells["y"] ** 2)
    bins = dict(tau_min=float(cells["tau"].min()), tau_max=float(cells["tau"].max()) + 1e-9, tau_bins=40, r_min=0.0, r_max=float(r.max()) + 1e-9,
                r_bins=40)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items() if k in api.VAH_FIELDS + ["x", "y"] and k not in COEF}
    ptrs = {k: v.data_ptr() for k, v in t.items() if k in api.VAH_FIELDS}
    shapes = api.spacetime_shapes(len(sp["mass"]), n, bins, dim, len(g["eta"]))
    outs = {k: torch.zeros(v, dtype=torch.float64, device=dev) for k, v in shapes.items() if k != "dN_dy_cell"}
    optr = {k: v.data_ptr() for k, v in outs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    plan = api.VahPlan(sp, grid, dict(dimension=dim), tab=tab, max_cells=n)
    plan.set_timing(True)
    spec = torch.zeros(plan.output_size, dtype=torch.float64, device=dev)
    st_all, wall, main = [], [], []
    res0 = None
    same = True
    # the two paths alternate in the same process, on the same plan (the record stream is shared)
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = plan.execute_spacetime(n, ptrs, t["x"].data_ptr(), t["y"].data_ptr(), g["pT_w"], g["phi_w"], bins, optr, stream)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        res = {k: v.cpu().numpy() for k, v in outs.items()}
        same = same and (res0 is None or all(np.array_equal(res0[k], res[k]) for k in res))
        res0 = res0 or res
        plan.execute(n, ptrs, spec.data_ptr(), stream)
        torch.cuda.synchronize()
        tm = plan.timings()
        if i >= warmup:
            wall.append(dt)
            st_all.append(st)
            main.append(tm["ms_main"])
    plan.close()
    med = {k: statistics.median(s[k] for s in st_all) for k in ("ms_prep", "ms_cells", "ms_bins")}
    ms_main = statistics.median(main)
    return dict(workload=name, cells=n, dimension=dim, species=len(sp["mass"]), classes=st_all[0]["n_classes"], n_passes=st_all[0]["n_passes"],
                bins=bins, steps=steps, warmup=warmup, step_ms_median=statistics.median(wall), ms_prep=med["ms_prep"], ms_cells=med["ms_cells"],
                ms_bins=med["ms_bins"], ms_cells_all=[s["ms_cells"] for s in st_all], ms_main=ms_main, ms_main_all=main,
                cells_over_main=med["ms_cells"] / ms_main, bitwise_repeat=bool(same), finite=bool(all(np.isfinite(v).all() for v in res0.values())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["all"] + sorted(WORKLOADS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cells", type=int, default=None, help="override the workload's cell count (a rehearsal; the recorded figures use the default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_spacetime_vah.json"))
    a = ap.parse_args()
    names = sorted(WORKLOADS) if a.workload == "all" else [a.workload]
    doc = dict(what="is3d_vah_plan_execute_spacetime per stage against ms_main of is3d_vah_plan_execute on the same cells and grid, same process",
               device=torch.cuda.get_device_name(0), workloads={})
    for name in names:
        doc["workloads"][name] = run(name, max(1, a.steps), max(0, a.warmup), a.cells)
        print(json.dumps(doc["workloads"][name]), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
