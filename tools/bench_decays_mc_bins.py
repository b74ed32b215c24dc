"""The decayed test_sampler distributions in one pass (is3d_decay_particles_binned, cf_decay_mc_bins) against the route it replaces --
is3d_decay_particles (count, scan, fill, the decayed list back to the host) followed by is3d_sampler_bin_list_device on the relabelled list --
on the workload of tools/bench_decays_mc.py: 1e6 primaries drawn from the chosen list of the smash and of the urqmd table at T = 0.15 GeV, one
event, the shipped bins (1800 words per species).

Slot sets: pi+ K+ p (5400 words: the workgroup-private form fits) and every stable entry of the table (urqmd 24 slots = 43 200 words, smash
147 slots: neither fits 64 KiB, global atomics only).  Per table and slot set, kernel_form 0, 1 and, where the block fits, 2; new route and replaced route in the same
process, in alternating order, medians of --steps runs:
  new       ms_bin (the one pass, device time), wall_ms_new (the whole host-pointer call)
  replaced  ms_count + ms_fill (device time of is3d_decay_particles), wall_ms_decay (its whole call, the decayed list downloaded),
            wall_ms_bin_list (is3d_sampler_bin_list_device on that list: upload, cf_sampler_bins, download -- the entry reports no device time
            of its own, so the kernel alone is not separated out), wall_ms_replaced = their sum
and whether the two routes' counts and yields are equal.  One JSON line, printed and written to --out.

  python tools/bench_decays_mc_bins.py [--primaries 1000000] [--steps 5] [--warmup 1] [--out profiles/r26_decays_mc_bins.json]"""
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

from bench_decays_mc import primaries, read_list  # noqa: E402
from is3d_amd import api  # noqa: E402

SHIPPED_BINS = dict(y_cut=5.0, y_bins=50, eta_cut=7.0, eta_bins=70, pT_lower_cut=0.0, pT_upper_cut=3.0, pT_bins=100, tau_min=0.0, tau_max=12.0,
                    tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)
WORDS_PER_SPECIES = 50 + 70 + 100 + 120 + 60 + 14 * 100
COUNTS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "yield")


def new_route(table, chosen, q, slot, S, bins):
    t0 = time.perf_counter()
    h, st = api.decay_particles_binned(table, chosen, q, slot, S, bins, 1, seed=7, device=0)
    return h, dict(ms_bin=st["ms_bin"], wall_ms_new=(time.perf_counter() - t0) * 1e3, n_final=st["n_final"], n_unbinned=st["n_unbinned"])


def replaced_route(table, chosen, q, slot, S, bins, capacity):
    t0 = time.perf_counter()
    out, _, st = api.decay_particles(table, chosen, q, seed=7, device=0, capacity=capacity)
    t1 = time.perf_counter()
    s = slot[out["species"]]
    rel = out[s >= 0]
    rel["species"] = s[s >= 0]
    t2 = time.perf_counter()
    h, _ = api.sampler_bin_list_device(bins, 1, S, rel, device=0)
    t3 = time.perf_counter()
    return h, dict(ms_count=st["ms_count"], ms_fill=st["ms_fill"], wall_ms_decay=(t1 - t0) * 1e3, wall_ms_bin_list=(t3 - t2) * 1e3,
                   wall_ms_replaced=(t1 - t0 + t3 - t2) * 1e3, n_final=st["n_final"])


def one(which, n, steps, warmup):
    table, chosen, mass, g = read_list(which)
    q = primaries(n, mass, g, 20260023)
    res = dict(table=which, primaries=n, chosen_species=len(chosen))
    for label, (slot, ids) in (("pikp", api.stable_slots(table, [211, 321, 2212])), ("all_stable", api.stable_slots(table))):
        S, words = len(ids), len(ids) * WORDS_PER_SPECIES
        fits = words + 6 <= 8192
        rows = {}
        capacity = None
        for form in (0, 1, 2) if fits else (0, 1):
            bins = dict(SHIPPED_BINS, kernel_form=form)
            new, old, equal = [], [], True
            for i in range(warmup + steps):
                order = (0, 1) if i % 2 == 0 else (1, 0)
                got = {}
                for r in order:
                    got[r] = new_route(table, chosen, q, slot, S, bins) if r == 0 else replaced_route(table, chosen, q, slot, S, bins, capacity)
                capacity = got[1][1]["n_final"]
                equal = equal and all(np.array_equal(got[0][0][k], got[1][0][k]) for k in COUNTS)
                if i >= warmup:
                    new.append(got[0][1])
                    old.append(got[1][1])
            med = lambda rows_, k: statistics.median(r[k] for r in rows_)  # noqa: E731
            row = {k: med(new, k) for k in ("ms_bin", "wall_ms_new")}
            row.update({k: med(old, k) for k in ("ms_count", "ms_fill", "wall_ms_decay", "wall_ms_bin_list", "wall_ms_replaced")})
            row.update(ms_count_plus_fill=row["ms_count"] + row["ms_fill"], counts_and_yields_equal=bool(equal), n_final=new[-1]["n_final"],
                       n_unbinned=new[-1]["n_unbinned"], ms_bin_runs=[r["ms_bin"] for r in new])
            rows["form%d" % form] = row
        res[label] = dict(slots=S, words=words, private_form_fits=fits, **rows)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--primaries", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tables", default="smash,urqmd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_decays_mc_bins.json"))
    a = ap.parse_args()
    res = dict(workload="decays_mc_bins", device=torch.cuda.get_device_name(0), bins=SHIPPED_BINS)
    for which in a.tables.split(","):
        res[which] = one(which, a.primaries, max(1, a.steps), max(1, a.warmup))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
