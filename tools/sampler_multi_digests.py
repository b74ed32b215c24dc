#!/usr/bin/env python3
"""What the sampler's multi-device entries return, as digests, so that two builds can be compared bit for bit: per case a SHA-256 of the raw
particle-list bytes or of every histogram array, the return code, the full error text, n_particles and the integer stats counters (not the
ms_* times).  Run once per build in a fresh process, then compare:

  python tools/sampler_multi_digests.py --out A.json          (from one tree)
  python tools/sampler_multi_digests.py --out B.json          (from the other)
  python tools/sampler_multi_digests.py --compare A.json B.json [--out profiles/FILE.json]

Cases: is3d_sample_particles_multi, is3d_sample_binned_multi, is3d_sample_fused_multi, is3d_sample_particles_vah_multi and
is3d_sample_binned_vah_multi through the wrappers of is3d_amd.api, crossed with
  surfaces   viscous df_mode 2 in 3+1D; df_mode 4 in 2+1D with fast = 1; anisotropic hydro with and without the tables
             (--cells 400 x --events 30, pi K p, volumes x 50)
  devices    [0], [0, 0], [0, 0, 0], and [0] * 7 on the first 5 cells (volumes x 4000): more shards than cells
  lists      count-only, exact capacity, half the capacity (IS3D_ENOMEM)
  histograms kernel_form 1 and 2
  batching   batch_events 0 and 1
and, with two and three shards: a viscous cell off the coefficient table in the last shard (all three viscous entries), anisotropic-hydro
bad cells in the first and the last shard (both entries).  A case that raises is recorded with its code and text and with whatever the
error carries (the partial list or histograms and the stats of an anisotropic-hydro bad cell)."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

BINS = dict(y_cut=2.1, y_bins=14, eta_cut=3.0, eta_bins=20, pT_lower_cut=0.1, pT_upper_cut=1.0, pT_bins=10, tau_min=2.5, tau_max=8.5, tau_bins=6,
            r_min=1.0, r_max=6.0, r_bins=5)
ARRAYS = ("dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "vn_re", "vn_im", "yield")
COUNTERS = ("n_particles", "n_cells_skipped", "n_hadrons_drawn", "n_momentum_samples", "n_acceptances", "n_classes", "n_cells_breakdown",
            "particle_workspace_bytes")
DEVICE_LISTS = {"1": [0], "2": [0, 0], "3": [0, 0, 0], "7-on-5-cells": [0] * 7}


def digest(result):
    h = hashlib.sha256()
    if isinstance(result, dict):
        for k in ARRAYS:
            h.update(np.ascontiguousarray(result[k], dtype=np.int64).tobytes())
    else:
        h.update(np.ascontiguousarray(result).tobytes())
    return h.hexdigest()


def record(call):
    """one case: what the wrapper returns, or what its error carries"""
    from is3d_amd import api
    try:
        result, st = call()
        row = dict(rc=0, error="")
    except api.Is3dError as e:
        row = dict(rc=int(e.code), error=str(e), bad_cell=e.bad_cell)
        result = getattr(e, "particles", getattr(e, "hist", None))
        st = getattr(e, "stats", None)
    if result is not None:
        row["sha256"] = digest(result)
        row["size"] = int(len(result) if not isinstance(result, dict) else result["yield"].sum())
    if st is not None:
        row.update({k: int(st[k]) for k in COUNTERS})
    return row


def scaled(cells, volume):
    v = {k: np.array(a, dtype=np.float64) for k, a in cells.items()}
    for f in ("dat", "dax", "day", "dan"):
        v[f] = volume * v[f]
    return v


def families(n_cells, n_events):
    """name -> (cells, {entry: f(cells, **kw)}, the family's keyword arguments, bad(cells, n_shards) -> a surface with bad cells)"""
    from is3d_amd import api, inputs, synth
    sp, df, tab = inputs.species("pikp"), inputs.df_tables(), inputs.vah_df_tables()
    out = {}

    def viscous(name, dim, opts, seed, **extra):
        cells = synth.synth_surface(n_cells, dim, seed=seed)
        gla = inputs.feqmod_tables(inputs.surface_average_T(cells))
        kw = dict(n_events=n_events, seed=seed + 1)
        if extra.get("fast"):
            kw.update(fq=gla, fast=1, T_avg=gla["T_avg"], T_avg_switch=0.151, y_cut=0.7)

        def bad(c, n_shards):
            c = {k: a.copy() for k, a in c.items()}
            c["T"][api.shard_bounds(len(c["T"]), n_shards - 1, n_shards)[0] + 1] = 0.31
            return c
        out[name] = (cells, dict(list=lambda c, **k: api.sample_particles(c, sp, df, gla, opts, **k),
                                 binned=lambda c, bins, **k: api.sample_binned(c, sp, df, gla, bins, opts, **k),
                                 fused=lambda c, bins, **k: api.sample_fused(c, sp, df, gla, bins, opts, **k)), kw, bad)

    def vah(name, seed, from_tab):
        cells = {k: np.array(a, dtype=np.float64) for k, a in synth.synth_vah_surface(n_cells, 3, seed=seed).items()}
        cells["bulkPi"] = 0.02 * cells["bulkPi"]
        gla, opts = inputs.feqmod_tables(0.15), dict(dimension=3)
        kw = dict(tab=tab if from_tab else None, n_events=n_events, seed=seed + 1)

        def bad(c, n_shards):
            c = {k: a.copy() for k, a in c.items()}
            c["Lambda"][1] = np.nan
            c["aL"][api.shard_bounds(len(c["T"]), n_shards - 1, n_shards)[0] + 1] = np.nan
            return c
        out[name] = (cells, dict(list=lambda c, **k: api.sample_particles_vah(c, sp, gla, opts, **k),
                                 binned=lambda c, bins, **k: api.sample_binned_vah(c, sp, gla, bins, opts, **k)), kw, bad)

    viscous("viscous-df2-3d", 3, dict(dimension=3, df_mode=2), 2201)
    viscous("viscous-df4-2d-fast", 2, dict(dimension=2, df_mode=4), 2203, fast=1)
    vah("vah-tables", 2205, True)
    vah("vah-cells", 2207, False)
    return out


def dump(n_cells, n_events):
    rows = {}
    for fname, (cells, entries, kw, bad) in families(n_cells, n_events).items():
        big = scaled(cells, 50.0)
        small = {k: np.ascontiguousarray(a[:5]) for k, a in scaled(cells, 4000.0).items()}
        for dname, devices in DEVICE_LISTS.items():
            c = small if dname == "7-on-5-cells" else big
            for be in (0, 1):
                k = dict(kw, devices=devices, batch_events=be)
                tag = "%s dev=%s batch=%d " % (fname, dname, be)
                whole = rows[tag + "list exact"] = record(lambda: entries["list"](c, **k))
                n = whole["n_particles"]
                rows[tag + "list count-only"] = record(lambda: entries["list"](c, capacity=0, **k))
                rows[tag + "list exact-capacity"] = record(lambda: entries["list"](c, capacity=n, **k))
                rows[tag + "list half-capacity"] = record(lambda: entries["list"](c, capacity=n // 2, **k))
                for e in ("binned", "fused"):
                    for form in (1, 2):
                        if e in entries:
                            rows[tag + "%s form=%d" % (e, form)] = record(lambda: entries[e](c, dict(BINS, kernel_form=form), **k))
        for n_shards in (2, 3):
            b = bad(big, n_shards)
            k = dict(kw, devices=[0] * n_shards, first_cell=1000)
            for e in entries:
                rows["%s dev=%d bad-cells %s" % (fname, n_shards, e)] = record(
                    (lambda: entries[e](b, **k)) if e == "list" else (lambda: entries[e](b, BINS, **k)))
    return rows


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    ra, rb = A["cases"], B["cases"]
    differ = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
    ok = sum(1 for r in ra.values() if r["rc"] == 0)
    return dict(what="tools/sampler_multi_digests.py: the first dump beside the second", cases=len(ra), cases_that_return_ok=ok,
                cases_that_return_an_error=len(ra) - ok, hadrons_of_the_largest_case=max(r.get("size", 0) for r in ra.values()),
                differing_cases=differ, all_equal=not differ, first=A, second=B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=400)
    ap.add_argument("--events", type=int, default=30)
    ap.add_argument("--label", default="")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.compare:
        out = compare(*a.compare)
        print(json.dumps({k: out[k] for k in ("cases", "cases_that_return_ok", "cases_that_return_an_error", "differing_cases", "all_equal")}))
    else:
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        from is3d_amd import api
        out = dict(label=a.label, version=api.load().is3d_version().decode(), device=torch.cuda.get_device_name(0), cells=a.cells, events=a.events,
                   cases=dump(a.cells, a.events))
        print(json.dumps(dict(label=a.label, cases=len(out["cases"]), ok=sum(1 for r in out["cases"].values() if r["rc"] == 0))))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if not a.compare or out["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
