#!/usr/bin/env python3
"""Time is3d_df_generate (csrc/cf_dfgen.hip) on the reference's 101 x 81 coefficient grid.

Lists: the urqmd fixture list (327 entries, is3d_amd/data/inputs_urqmd.json) and, where tests/golden/golden_dfcoef_lists.npz is present, the
smash list (493 entries).  Rule: the 64-point Gauss-Laguerre rule of tests/golden/golden_dfcoef.npz.  Per list: median of --repeats calls,
`ms_kernel` (device events around the kernel) and the whole call (uploads, kernel, copies back) in ms, a bitwise-repeat flag and the largest
|value - shipped| against the shipped tables where the fixture holds them.  The result goes to the next free profiles/rNN_dfgen.json (--out).

CPU context: the checker under oracle/ restates the same generator on the host (one process: 41.9 s for the urqmd grid, tests/test_oracle_dfcoef.py
--all), but tools/ never import it (tests/test_abi.py), so no CPU time is measured here; `cpu_context` in the output says so."""
import argparse
import glob
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from is3d_amd import api, inputs  # noqa: E402


def next_free():
    rounds = [int(m.group(1)) for f in glob.glob(os.path.join(ROOT, "profiles", "r*_*")) for m in [re.match(r"r(\d+)_", os.path.basename(f))] if m]
    n = max(rounds, default=0) + 1
    while os.path.exists(os.path.join(ROOT, "profiles", "r%02d_dfgen.json" % n)):
        n += 1
    return os.path.join(ROOT, "profiles", "r%02d_dfgen.json" % n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_dfcoef.npz"))
    root, weight = gold["root"], gold["weight"]
    full = inputs.df_tables_full()
    T, B = full["T"], full["muB"]
    urqmd = np.array(inputs.load_fixture()["pdg_urqmd"], dtype=np.float64)
    lists = {"urqmd": dict(mass=urqmd[:, 1], gspin=urqmd[:, 2], baryon=urqmd[:, 3], sign=urqmd[:, 4])}
    extra = os.path.join(ROOT, "tests", "golden", "golden_dfcoef_lists.npz")
    if os.path.exists(extra):
        z = np.load(extra)
        lists["smash"] = {k: z["smash_" + k] for k in ("mass", "gspin", "baryon", "sign")}
    res = dict(tool="tools/bench_dfgen.py", grid=[len(T), len(B)], n_gla=int(root.shape[1]), repeats=a.repeats, lists={},
               cpu_context="not measured: tools/ do not import the CPU checker; its one-process time for the urqmd grid is 41.9 s (tests/test_oracle_dfcoef.py --all)")
    for name, pdg in lists.items():
        for _ in range(a.warmup):
            first, _, _ = api.df_generate(pdg, root, weight, T, B)
        ms_kernel, ms_call, same = [], [], True
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            tab, _, st = api.df_generate(pdg, root, weight, T, B)
            ms_call.append(1e3 * (time.perf_counter() - t0))
            ms_kernel.append(st["ms_kernel"])
            same = same and tab.tobytes() == first.tobytes()
        massive = st["n_massive"]
        row = dict(entries=len(pdg["mass"]), massive=massive, ms_kernel=statistics.median(ms_kernel), ms_call=statistics.median(ms_call),
                   ms_kernel_all=ms_kernel, ms_call_all=ms_call, bitwise_repeat=same,
                   exponentials=int(len(T) * len(B) * massive * 4 * root.shape[1]))
        row["exponentials_per_s"] = row["exponentials"] / (1e-3 * row["ms_kernel"])
        if name == "urqmd":
            ship = np.array([full["2d"][n] for n in inputs.DF_NAMES_2D])
            row["max_abs_diff_to_shipped"] = float(np.max(np.abs(tab - ship)))
        res["lists"][name] = row
        print(name, json.dumps(row))
    out = a.out or next_free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
