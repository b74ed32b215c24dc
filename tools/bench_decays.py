"""Resonance decay feed-down on the device-resident plan (is3d_decay_plan_execute): ms per full feed-down of the smash list (hrg_eos = 2,
the shipped default: PDG/pdg_smash.dat with its 444 chosen species) on the 32 x 24 grid (2+1D) and the 32 x 24 x 21 grid (3+1D), quadrature
evaluations per second, the device time of the table and feed-down kernels, and, with --kernel-stats, the per-kernel summary of a
`rocprofv3 --kernel-trace --stats` run of this script.  One JSON line.

  python tools/bench_decays.py [--steps 3] [--warmup 1] [--out FILE] [--kernel-stats FILE_kernel_stats.csv]

Spectra: is3d_smooth_spectra (Chapman-Enskog) of the 444 species over synth_surface(2000, 2) and synth_surface(500, 3).  The PDG data are
read from tests/golden/reference_data.tar.xz (the data files of the original distribution)."""
import argparse
import csv
import json
import os
import statistics
import sys
import tarfile
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from is3d_amd import api, inputs, synth  # noqa: E402


def smash_inputs():
    with tempfile.TemporaryDirectory() as d:
        with tarfile.open(os.path.join(ROOT, "tests", "golden", "reference_data.tar.xz")) as t:
            for name in ("PDG/pdg_smash.dat", "PDG/chosen_particles_smash.dat"):
                t.extract(name, d)
        table = api.pdg_read_decays(os.path.join(d, "PDG", "pdg_smash.dat"))
        pdg = api.pdg_read(os.path.join(d, "PDG", "pdg_smash.dat"))
        chosen = [int(x) for x in open(os.path.join(d, "PDG", "chosen_particles_smash.dat")).read().split()]
    ids = list(pdg["mc_id"])
    k = [ids.index(c) for c in chosen]
    sp = dict(mass=pdg["mass"][k], sign=pdg["sign"][k], degeneracy=pdg["gspin"][k], baryon=pdg["baryon"][k])
    return table, chosen, sp


def one(dim, table, chosen, sp, steps, warmup):
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    cells = synth.synth_surface(2000 if dim == 2 else 500, dim, seed=20260009 + dim)
    dN, _ = api.smooth_spectra(cells, sp, grid, inputs.df_tables(), dict(dimension=dim, df_mode=2))
    dev = torch.device("cuda:0")
    base = torch.from_numpy(np.ascontiguousarray(dN)).to(dev)
    work = base.clone()
    plan = api.DecayPlan(table, chosen, grid, dimension=dim, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    wall = []
    for i in range(warmup + steps):
        work.copy_(base)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan.execute(work.data_ptr(), stream, want_stats=False)
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    first = work.cpu().numpy().copy()
    work.copy_(base)
    st = plan.execute(work.data_ptr(), stream)
    same = work.cpu().numpy().tobytes() == first.tobytes()
    plan.close()
    ms = statistics.median(wall)
    return dict(grid="32x24" if dim == 2 else "32x24x21", ms_per_feed_down=ms, ms_runs=wall, ms_tables=st["ms_tables"], ms_feed=st["ms_feed"],
                parents=st["n_parents"], channels=st["n_channels"], adjusted_channels=st["n_adjusted"], clamps=st["n_clamps"],
                quadrature_points=st["n_points"], quadrature_points_per_s=st["n_points"] / (ms * 1e-3), bitwise_repeat=same)


def kernel_stats(path):
    rows = list(csv.DictReader(open(path)))
    out = {}
    for r in rows:
        name = r.get("Name", "")
        if "cf_decay" in name:
            key = "cf_decay_tables" if "cf_decay_tables" in name else "cf_decay_feed"
            out[key] = dict(calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) / 1e6, average_us=float(r["AverageNs"]) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    table, chosen, sp = smash_inputs()
    res = dict(workload="resonance_decays_smash", species=len(chosen), device=torch.cuda.get_device_name(0),
               d2=one(2, table, chosen, sp, max(1, a.steps), max(0, a.warmup)), d3=one(3, table, chosen, sp, max(1, a.steps), max(0, a.warmup)))
    if a.kernel_stats:
        res["kernel_stats"] = kernel_stats(a.kernel_stats)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
