#!/usr/bin/env python3
"""Developer A/B on a GPU box of this tree's library against ANOTHER BUILD of it (--parent DIR: the directory that holds the other libis3d_amd.so, e.g.
the parent commit's is3d_amd/lib copied aside) in ONE process: tools/gpu_ab.py's method -- one resident config-3 surface, interleaved rounds, HIP-event
main-kernel times -- for changes that no kernel_variant separates.  Two plans per arm and culling mode: parent against parent is the spread the gain is
held to.  The two libraries are loaded side by side (ctypes, RTLD_LOCAL: each resolves its own symbols); the spectra are compared bitwise."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from is3d_amd import api, inputs, synth  # noqa: E402


def parent_api(libdir):
    """a second copy of is3d_amd.api bound to the library in `libdir`"""
    spec = importlib.util.spec_from_file_location("is3d_amd.api_parent", os.path.join(ROOT, "is3d_amd", "api.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["is3d_amd.api_parent"] = m
    spec.loader.exec_module(m)
    m.LIB_PATH = os.path.join(libdir, "libis3d_amd.so")
    assert os.path.exists(m.LIB_PATH), m.LIB_PATH
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--df", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent", required=True, help="directory of the other build's libis3d_amd.so")
    a = ap.parse_args()
    import torch
    old = parent_api(a.parent)
    print("new:", api.LIB_PATH, api.load().is3d_version().decode(), "| parent:", old.LIB_PATH, old.load().is3d_version().decode(), flush=True)
    assert api.load()._handle != old.load()._handle
    g = inputs.grid()
    grid = dict(pT=g["pT"], phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])
    df = inputs.df_tables()
    sp = inputs.species("urqmd")
    cells = synth.synth_surface(a.cells, 3)
    dev = torch.device("cuda:0")
    tens = {k: torch.from_numpy(cells[k]).to(dev) for k in synth.CELL_FIELDS}
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    stream = torch.cuda.current_stream().cuda_stream
    arms = [("parent on  a", old, 0), ("new    on  a", api, 0), ("parent on  b", old, 0), ("new    on  b", api, 0), ("parent off a", old, 2), ("new    off a", api, 2), ("parent off b", old, 2), ("new    off b", api, 2)]
    plans, outs = [], []
    for name, mod, zs in arms:
        p = mod.Plan(sp, grid, df, dict(dimension=3, df_mode=a.df, zero_skip=zs), max_cells=a.cells)
        p.set_timing(True)
        plans.append(p)
        outs.append(torch.zeros(p.output_size, dtype=torch.float64, device=dev))
    times = [[] for _ in arms]
    for r in range(a.rounds + 1):
        for i, p in enumerate(plans):
            p.execute(a.cells, ptrs, outs[i].data_ptr(), stream, want_status=False)
            t = p.timings()
            if r > 0:
                times[i].append(t["ms_main"])
        print("round", r, " ".join("%.2f" % (times[i][-1] if times[i] else float("nan")) for i in range(len(arms))), flush=True)
    culled = []
    for i, p in enumerate(plans):
        st = p.execute(a.cells, ptrs, outs[i].data_ptr(), stream)
        culled.append((st["n_wave_rows_culled"], st["n_wave_rows"]))
    ref = outs[0].cpu().numpy()
    med = []
    for i, (name, mod, zs) in enumerate(arms):
        got = outs[i].cpu().numpy()
        ms = np.array(times[i])
        med.append(float(np.median(ms)))
        print("%-14s %s main ms: median %.2f min %.2f max %.2f   wave-rows culled %d of %d = %.4f   bitwise the first arm's spectrum %s" % (
            name, plans[i].main_kernel_name, np.median(ms), ms.min(), ms.max(), culled[i][0], culled[i][1], culled[i][0] / max(culled[i][1], 1),
            bool(np.array_equal(got, ref))), flush=True)
    spread = abs(med[0] - med[2])
    gain = 0.5 * (med[0] + med[2]) - 0.5 * (med[1] + med[3])
    print("culling on: new %.2f / %.2f against parent %.2f / %.2f ms: gain %.2f ms = %.2f %%; parent against parent %.2f ms, new against new %.2f ms -> %.1f x the spread" % (
        med[1], med[3], med[0], med[2], gain, 100 * gain / (0.5 * (med[0] + med[2])), spread, abs(med[1] - med[3]), gain / max(spread, 1e-9)))
    print("culling off: new %.2f / %.2f against parent %.2f / %.2f ms: %+.2f ms; parent against parent %.2f ms, new against new %.2f ms" % (
        med[5], med[7], med[4], med[6], 0.5 * (med[5] + med[7]) - 0.5 * (med[4] + med[6]), abs(med[4] - med[6]), abs(med[5] - med[7])))


if __name__ == "__main__":
    main()
