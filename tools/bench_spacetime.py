"""Operation 0 (smooth spacetime distributions, is3d_plan_execute_spacetime) on the device-resident plan: ms per stage, evaluations
per second and the fp64 rate of the per-cell kernel, both NOMINAL (see below) and, on the same surface in the same process, the spectra path's main kernel with culling off
(zero_skip = 2).  One JSON line per workload on stdout.

  python tools/bench_spacetime.py [--workload config3|config2|all] [--steps 5] [--warmup 1] [--out FILE]

Workloads: BASELINE config 3's shape (1e6 synthetic 3+1D cells, seed 20260002, Chapman-Enskog, 305 urqmd species, 32 x 24 x 21) and config 2's
(1e5 cells, 2+1D, pi/K/p, 14-moment, 241 eta nodes).  Flop per evaluation: a hand count of cf_st_cells' evaluation body (FMA = 2 flop, the
Newton reciprocal rcp_nr = 1 + 4 FMA = 9 flop, min / max = 1): 14-moment 24, Chapman-Enskog 28.  Peak: 78.6 TFLOP/s fp64 vector.
"Nominal": the evaluation count is cells x classes x npT x J x (y | eta) points, the reference's; the kernel executes more lanes (the pT grid
padded to a power of two, the clamped phi copies of the last tile, rows padded to the tile) and fewer rows (exact-zero rows culled), and the
flop per evaluation is a hand count, not read from the ISA."""
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

PEAK_TFLOPS = 78.6
FLOP_PER_EVAL = {1: 24, 2: 28}
WORKLOADS = dict(config3=dict(dimension=3, df_mode=2, species="urqmd", cells=1000000),
                 config2=dict(dimension=2, df_mode=1, species="pikp", cells=100000))


def run(name, steps, warmup):
    wl = WORKLOADS[name]
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    sp = inputs.species(wl["species"])
    df = inputs.df_tables()
    n, dim = wl["cells"], wl["dimension"]
    cells = synth.synth_surface(n, dim)
    r = np.sqrt(cells["x"] ** 2 + cells["y"] ** 2)
    bins = dict(tau_min=float(cells["tau"].min()), tau_max=float(cells["tau"].max()) + 1e-9, tau_bins=40, r_min=0.0, r_max=float(r.max()) + 1e-9,
                r_bins=40)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items()}
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    opts = dict(dimension=dim, df_mode=wl["df_mode"])
    plan = api.Plan(sp, grid, df, opts, max_cells=n)
    shapes = api.spacetime_shapes(len(sp["mass"]), n, bins, dim, len(g["eta"]))
    outs = {k: torch.zeros(v, dtype=torch.float64, device=dev) for k, v in shapes.items() if k != "dN_dy_cell"}
    optr = {k: v.data_ptr() for k, v in outs.items()}
    stream = torch.cuda.current_stream().cuda_stream
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
    step = statistics.median(wall)
    res0 = {k: v.cpu().numpy() for k, v in outs.items()}
    # the same surface through the spectra path, culling off: its main kernel is the comparison the issue names
    plan2 = api.Plan(sp, grid, df, dict(opts, zero_skip=2), max_cells=n)
    plan2.set_timing(True)
    spec = torch.zeros(plan2.output_size, dtype=torch.float64, device=dev)
    main_no_cull = []
    for i in range(1 + min(steps, 3)):
        plan2.execute(n, ptrs, spec.data_ptr(), stream)
        torch.cuda.synchronize()
        if i:
            main_no_cull.append(plan2.timings()["ms_main"])
    main_nc = statistics.median(main_no_cull)
    # reproducibility of the resident execute (bitwise)
    plan.execute_spacetime(n, ptrs, ptrs["x"], ptrs["y"], g["pT_w"], g["phi_w"], bins, optr, stream)
    torch.cuda.synchronize()
    same = all(np.array_equal(res0[k], outs[k].cpu().numpy()) for k in outs)
    ncls = st_all[0]["n_classes"]
    K = len(g["y"]) if dim == 3 else len(g["eta"])
    evals = float(n) * ncls * len(g["pT"]) * len(g["phi"]) * K
    tflops = evals * FLOP_PER_EVAL[wl["df_mode"]] / (med["ms_cells"] * 1e-3) / 1e12
    plan.close()
    plan2.close()
    return dict(workload=name, cells=n, dimension=dim, df_mode=wl["df_mode"], species=len(sp["mass"]), classes=ncls, bins=bins, steps=steps,
                warmup=warmup, step_ms_median=step, stage_ms_median=med, n_passes=st_all[0]["n_passes"],
                evaluations_nominal=evals, evals_per_s_nominal=evals / (med["ms_cells"] * 1e-3),
                flop_per_eval=FLOP_PER_EVAL[wl["df_mode"]], flop_count="hand count of cf_st_cells' evaluation body (FMA = 2, rcp_nr = 9)",
                tflops_cells_nominal=tflops, frac_of_fp64_vector_peak_nominal=tflops / PEAK_TFLOPS,
                spectra_main_no_cull_ms=main_nc, cells_over_main_no_cull=med["ms_cells"] / main_nc,
                bins_share_of_step=med["ms_bins"] / sum(med.values()), bitwise_repeat=same,
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["all"] + sorted(WORKLOADS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = sorted(WORKLOADS) if a.workload == "all" else [a.workload]
    for name in names:
        line = json.dumps(run(name, max(1, a.steps), max(0, a.warmup)))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
