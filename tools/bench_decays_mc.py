"""Monte Carlo decays of a sampled list on the device (is3d_decay_particles): 1e6 primaries drawn from the chosen list of the smash table
(hrg_eos = 2, PDG/pdg_smash.dat) and of the urqmd table (hrg_eos = 1, PDG/pdg-urqmd_v3.3+.dat): the device time of the count pass with its
scan and of the fill pass, phase-space proposals per decay, decays per second of count + fill, final particles per primary and the wall time
of the host-pointer call (upload, count, scan, fill, download).  One JSON line, printed and written to --out.

  python tools/bench_decays_mc.py [--primaries 1000000] [--steps 5] [--warmup 1] [--lifetime 0] [--out profiles/r23_decays_mc.json]

The primaries: species drawn with the weight g m^(3/2) exp(-m / T) at T = 0.15 GeV (g = the spin degeneracy of the list), momentum
components normal with variance m T, all at tau = 1 fm, one event.  The PDG data are read from tests/golden/reference_data.tar.xz (the data
files of the original distribution)."""
import argparse
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

from is3d_amd import api  # noqa: E402

LISTS = dict(smash=("PDG/pdg_smash.dat", "PDG/chosen_particles_smash.dat"), urqmd=("PDG/pdg-urqmd_v3.3+.dat", "PDG/chosen_particles_urqmd_v3.3+.dat"))
T_FO = 0.15


def read_list(which):
    with tempfile.TemporaryDirectory() as d:
        with tarfile.open(os.path.join(ROOT, "tests", "golden", "reference_data.tar.xz")) as t:
            for name in LISTS[which]:
                t.extract(name, d)
        table = api.pdg_read_decays(os.path.join(d, LISTS[which][0]))
        pdg = api.pdg_read(os.path.join(d, LISTS[which][0]))
        chosen = [int(x) for x in open(os.path.join(d, LISTS[which][1])).read().split()]
    ids = list(pdg["mc_id"])
    k = [ids.index(c) for c in chosen]
    return table, chosen, pdg["mass"][k], pdg["gspin"][k]


def primaries(n, mass, g, seed):
    rng = np.random.default_rng(seed)
    w = g * mass ** 1.5 * np.exp(-mass / T_FO)
    species = rng.choice(len(mass), size=n, p=w / w.sum())
    m = mass[species]
    q = np.zeros(n, dtype=api.PARTICLE_DTYPE)
    q["species"], q["cell"] = species, np.arange(n)
    p3 = rng.normal(size=(n, 3)) * np.sqrt(m * T_FO)[:, None]
    q["px"], q["py"], q["pz"] = p3[:, 0], p3[:, 1], p3[:, 2]
    q["E"] = np.sqrt(m * m + (p3 * p3).sum(axis=1))
    q["tau"] = q["t"] = 1.0
    return q


def one(which, n, steps, warmup, lifetime):
    table, chosen, mass, g = read_list(which)
    q = primaries(n, mass, g, 20260023)
    runs = []
    first = None
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        out, origin, st = api.decay_particles(table, chosen, q, seed=7, lifetime=lifetime, device=0, capacity=None if first is None else len(first))
        wall = (time.perf_counter() - t0) * 1e3
        if first is None:
            first = out.copy()
        elif i >= warmup:
            runs.append(dict(st, wall_ms=wall, same_bits=out.tobytes() == first.tobytes()))
    if not runs:
        runs.append(dict(st, wall_ms=wall, same_bits=True))
    med = lambda k: statistics.median(r[k] for r in runs)  # noqa: E731
    ms = med("ms_count") + med("ms_fill")
    return dict(table=which, chosen_species=len(chosen), primaries=n, lifetime=lifetime, n_decays=st["n_decays"], n_final=st["n_final"],
                n_stuck=st["n_stuck"], n_exhausted=st["n_exhausted"], max_stack=st["max_stack"], max_depth=st["max_depth"],
                n_closed_channels=st["n_closed_channels"], ms_count=med("ms_count"), ms_fill=med("ms_fill"), ms_h2d=med("ms_h2d"), ms_d2h=med("ms_d2h"),
                wall_ms_fill_call=med("wall_ms"), trials_per_decay=st["n_trials"] / max(st["n_decays"], 1),
                decays_per_s=st["n_decays"] / (ms * 1e-3), final_per_primary=st["n_final"] / n, bitwise_repeat=all(r["same_bits"] for r in runs),
                ms_count_runs=[r["ms_count"] for r in runs], ms_fill_runs=[r["ms_fill"] for r in runs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--primaries", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lifetime", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_decays_mc.json"))
    a = ap.parse_args()
    res = dict(workload="decays_mc", device=torch.cuda.get_device_name(0),
               smash=one("smash", a.primaries, max(1, a.steps), max(1, a.warmup), a.lifetime),
               urqmd=one("urqmd", a.primaries, max(1, a.steps), max(1, a.warmup), a.lifetime))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
