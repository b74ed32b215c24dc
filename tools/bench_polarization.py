"""Spin polarization from thermal vorticity (mode 5) on the device-resident plan (is3d_polarization_plan_execute): ms per step and per stage,
nominal class-evaluations per second, fp64 instructions and flop per evaluation READ FROM THE ISA, the fp64-VALU roofline fraction, and, on
the same surface in the same process, the spectra path's main kernel (cf_main_tile3e) with culling off (zero_skip = 2).  One JSON line.

  python tools/bench_polarization.py [--steps 5] [--warmup 1] [--out FILE]

Workload: BASELINE config 3's shape -- 1e6 cells of synth_surface(n, 3, seed=20260002), synth_vorticity(n, seed=20260005), the 305 urqmd
species, the 32 x 24 x 21 grid, T = the surface's volume-weighted average temperature (what the reader writes first into
average_thermodynamic_quantities.dat).
ISA: cf_polzn.hip is compiled for gfx950 with --save-temps; in cf_polzn_cells3 the innermost loop that holds v_rcp_f64 is the per-cell body
(every evaluation issues exactly one v_rcp_f64), so its fp64 opcode histogram divided by its v_rcp_f64 count is the cost of one evaluation
INCLUDING the per-cell (pT, y) and (pT, phi) sides amortised over the tile.  flop: v_fma / v_fmac = 2, every other fp64 op 1.
"Nominal": evaluations = cells x classes x npT x n_phi x n_y (the kernel also runs the pT lanes padded to a power of two)."""
import argparse
import collections
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from is3d_amd import api, inputs, synth  # noqa: E402

PEAK_TFLOPS = 78.6
F64 = ("v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_add_f64", "v_max_f64", "v_min_f64", "v_rcp_f64", "v_ldexp_f64", "v_rndne_f64",
       "v_cvt_i32_f64", "v_div_", "v_fract_f64", "v_frexp_mant_f64", "v_frexp_exp_i32_f64", "v_cmp_", "v_cndmask_b32", "v_mov_b64")


def isa_counts(kernel="cf_polzn_cells3"):
    """fp64 opcode histogram per evaluation of the kernel's per-cell loop, from hipcc --save-temps."""
    src = os.path.join(ROOT, "is3d_amd", "csrc", "cf_polzn.hip")
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--save-temps", "-c", src, "-o",
                               os.path.join(d, "p.o")], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = [f for f in os.listdir(d) if f.endswith(".s") and "gfx950" in f]
        text = open(os.path.join(d, asm[0])).read()
    lines = text.split("\n")
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_ZN4is3d\d+%s.*:" % kernel, ln))
    end = next(i for i in range(start + 1, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    body = lines[start:end]
    labels = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", ln)] if m}
    best = None
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\w+)|\s+s_branch\s+(\.LBB\w+)", ln)
        if not m:
            continue
        tgt = labels.get(m.group(1) or m.group(2))
        if tgt is None or tgt >= i:
            continue
        seg = body[tgt:i + 1]
        if any("v_rcp_f64" in s for s in seg) and (best is None or i - tgt < best[1] - best[0]):
            best = (tgt, i)
    seg = body[best[0]:best[1] + 1]
    hist = collections.Counter()
    for s in seg:
        op = s.strip().split(" ")[0]
        for f in F64:
            if op.startswith(f):
                hist[op] += 1
    # the cell's 1 / tau is a division (v_div_fixup_f64 behind its own v_rcp_f64): not an evaluation
    evals = sum(v for k, v in hist.items() if k.startswith("v_rcp_f64")) - sum(v for k, v in hist.items() if k.startswith("v_div_fixup_f64"))
    f64 = sum(v for k, v in hist.items() if "f64" in k)
    flop = sum((2 if k.startswith(("v_fma_f64", "v_fmac_f64")) else 1) * v for k, v in hist.items() if "f64" in k)
    return dict(kernel=kernel, loop_lines=len(seg), evaluations_per_loop=evals, fp64_instr_per_eval=f64 / evals, flop_per_eval=flop / evals,
                histogram={k: v for k, v in sorted(hist.items())})


def run(steps, warmup):
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    sp = inputs.species("urqmd")
    n = 1000000
    cells = synth.synth_surface(n, 3, seed=synth.SEED_CONFIG3)
    w = synth.synth_vorticity(n, seed=synth.SEED_VORTICITY)
    T = float(inputs.surface_average_T(cells))
    dev = torch.device("cuda:0")
    tc = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cells.items()}
    tw = {k: torch.from_numpy(v).to(dev) for k, v in w.items()}
    cp, wp = {k: v.data_ptr() for k, v in tc.items()}, {k: v.data_ptr() for k, v in tw.items()}
    plan = api.PolarizationPlan(sp, grid, dict(dimension=3), max_cells=n)
    outs = {k: torch.zeros(plan.output_size, dtype=torch.float64, device=dev) for k in api.POLARIZATION_OUTPUTS}
    op = {k: v.data_ptr() for k, v in outs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    st_all, wall = [], []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = plan.execute(n, cp, wp, T, op, stream)
        torch.cuda.synchronize()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            st_all.append(st)
    res0 = {k: v.cpu().numpy() for k, v in outs.items()}
    plan.execute(n, cp, wp, T, op, stream)
    torch.cuda.synchronize()
    same = all(np.array_equal(res0[k], outs[k].cpu().numpy()) for k in outs)
    med = {k: statistics.median(s[k] for s in st_all) for k in ("ms_cells", "ms_reduce")}
    ncls = st_all[0]["n_classes"]
    plan.close()
    # the spectra path's main kernel on the same surface, culling off
    plan2 = api.Plan(sp, grid, inputs.df_tables(), dict(dimension=3, df_mode=2, zero_skip=2), max_cells=n)
    plan2.set_timing(True)
    spec = torch.zeros(plan2.output_size, dtype=torch.float64, device=dev)
    main_nc = []
    for i in range(1 + min(steps, 3)):
        plan2.execute(n, cp, spec.data_ptr(), stream)
        torch.cuda.synchronize()
        if i:
            main_nc.append(plan2.timings()["ms_main"])
    main_kernel = plan2.main_kernel_name
    plan2.close()
    main_ms = statistics.median(main_nc)
    isa = isa_counts()
    evals = float(n) * ncls * len(g["pT"]) * len(g["phi"]) * len(g["y"])
    tflops = evals * isa["flop_per_eval"] / (med["ms_cells"] * 1e-3) / 1e12
    return dict(workload="config3_polarization", cells=n, species=len(sp["mass"]), classes=ncls, T=T, steps=steps, warmup=warmup,
                ms_per_step=statistics.median(wall), stage_ms_median=med, n_chunks=st_all[0]["n_chunks"],
                evaluations_nominal=evals, class_evals_per_s_nominal=evals / (med["ms_cells"] * 1e-3),
                fp64_instr_per_eval=isa["fp64_instr_per_eval"], flop_per_eval=isa["flop_per_eval"], isa=isa,
                tflops_cells_nominal=tflops, frac_of_fp64_vector_peak=tflops / PEAK_TFLOPS,
                spectra_main_kernel=main_kernel, spectra_main_no_cull_ms=main_ms, cells_over_main_no_cull=med["ms_cells"] / main_ms,
                bitwise_repeat=same, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--isa-only", action="store_true", help="print the ISA counts and exit (no GPU)")
    a = ap.parse_args()
    if a.isa_only:
        print(json.dumps(isa_counts()))
        return
    line = json.dumps(run(max(1, a.steps), max(0, a.warmup)))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
