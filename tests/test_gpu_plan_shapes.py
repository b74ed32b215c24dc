"""GPU: what the plans' host code decides, pinned per configuration -- main kernel, tile, output size, workspace bytes, and from the execute's
status the kernel variant that ran, the species classes and the passes -- against tests/golden/plan_shapes.json.  No kernel is under test here:
the file was recorded with this same module from the build before the geometry moved into cf_plan_geometry.h (1774277), shipped and developer
library each (`python tests/test_gpu_plan_shapes.py --record FILE [--lib DIR]`).

Every configuration runs a 192-cell synthetic surface (the smallest that still gives three 64-cell chunks) twice with an explicit
workspace_bytes, so that nothing depends on the card's memory: once in one pass, once with a cap of 80 cells per pass -- between a third and a
half of the cells -- which takes three."""
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_shapes.json")
N = 192
ONE_PASS = 1 << 30

# (dimension, df_mode, include_baryon, pT values, species, requested variant)
CASES = [(3, 1, 0, 32, "pikp", 0), (3, 1, 0, 33, "pikp", 0), (3, 2, 0, 32, "pikp", 0), (3, 2, 0, 32, "urqmd", 0), (3, 2, 0, 33, "urqmd", 0),
         (3, 2, 0, 32, "pikp", 3), (3, 2, 0, 32, "pikp", 6), (3, 2, 0, 33, "pikp", 6), (3, 2, 0, 32, "pikp", 7),
         (3, 1, 1, 32, "pikp", 0), (3, 2, 1, 33, "pikp", 0), (3, 2, 1, 32, "pikp", 3), (3, 2, 1, 32, "urqmd", 0),
         (2, 1, 0, 32, "pikp", 0), (2, 2, 0, 32, "pikp", 0), (2, 2, 0, 33, "urqmd", 0), (2, 2, 0, 32, "pikp", 3), (2, 2, 0, 32, "pikp", 7),
         (2, 2, 1, 32, "pikp", 0), (2, 1, 1, 32, "pikp", 6),
         (3, 3, 0, 32, "pikp", 0), (3, 3, 1, 32, "pikp", 0), (3, 4, 0, 33, "pikp", 0), (3, 4, 0, 32, "pikp", 6), (3, 3, 0, 32, "urqmd", 3),
         (2, 3, 0, 32, "pikp", 0), (2, 4, 0, 32, "pikp", 7), (2, 3, 1, 33, "pikp", 3), (2, 4, 0, 32, "urqmd", 0)]
# anisotropic hydro: (dimension, coefficients from the tables, pT values, species, requested variant)
VAH_CASES = [(3, 1, 32, "pikp", 0), (3, 0, 33, "pikp", 3), (2, 1, 32, "pikp", 0), (2, 0, 32, "urqmd", 0)]


def case_id(c):
    return "-".join(str(x) for x in c)


@functools.lru_cache(maxsize=None)
def _grid(n_pT):
    from is3d_amd import inputs
    g = inputs.grid()
    pT = g["pT"][:n_pT] if len(g["pT"]) >= n_pT else np.linspace(g["pT"][0], g["pT"][-1], n_pT)
    return dict(pT=np.ascontiguousarray(pT), phi=g["phi"], y=g["y"], eta=g["eta"], eta_w=g["eta_w"])


@functools.lru_cache(maxsize=None)
def _surface(kind, dim, baryon):
    """the cells on the host and, with them, on the device (kept alive here)"""
    import torch
    from is3d_amd import api, synth
    if kind == "vah":
        cells = synth.synth_vah_surface(N, dim, seed=7100 + dim)
        fields = [f for f in api.VAH_FIELDS if f != "T"]
    else:
        cells = synth.synth_surface(N, dim, seed=7000 + dim, baryon=bool(baryon))
        fields = list(synth.CELL_FIELDS)
    tens = {k: torch.from_numpy(np.ascontiguousarray(cells[k])).to("cuda:0") for k in fields if k in cells}
    return cells, tens


def _two_runs(make_plan, tens, per_cell_extra):
    """make_plan(max_cells, workspace_bytes) -> plan.  Returns (what the plan decided, the two spectra)."""
    import torch
    # bytes of streams per cell: two one-pass plans whose cell counts give the same three chunks differ by exactly that per cell
    a, b = make_plan(N, ONE_PASS), make_plan(N + 63, ONE_PASS)
    per_cell, rem = divmod(b.workspace_bytes - a.workspace_bytes, 63)
    b.close()
    assert rem == 0 and per_cell > per_cell_extra
    plans = [a, make_plan(N, (per_cell - per_cell_extra) * 80)]
    ptrs = {k: v.data_ptr() for k, v in tens.items()}
    shape, spectra = None, []
    for p in plans:
        out = torch.zeros(p.output_size, dtype=torch.float64, device="cuda:0")
        st = p.execute(N, ptrs, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        spectra.append(out.cpu().numpy())
        s = dict(kernel=p.main_kernel_name, tile=list(p.tile_shape), output_size=int(p.output_size), workspace_bytes=[int(p.workspace_bytes)],
                 kernel_variant=int(st["kernel_variant"]), n_classes=int(st["n_classes"]), n_passes=[int(st["n_passes"])])
        p.close()
        if shape is None:
            shape = s
        else:
            assert {k: v for k, v in s.items() if k not in ("workspace_bytes", "n_passes")} == {k: v for k, v in shape.items() if k not in ("workspace_bytes", "n_passes")}
            shape["workspace_bytes"] += s["workspace_bytes"]
            shape["n_passes"] += s["n_passes"]
    return shape, spectra


def run_case(api, c):
    from is3d_amd import inputs
    dim, df_mode, baryon, n_pT, which, variant = c
    cells, tens = _surface("vh", dim, baryon)
    df = inputs.df_tables_full() if baryon else inputs.df_tables()
    fq = inputs.feqmod_tables(inputs.surface_average_T(cells)) if df_mode >= 3 else None
    opts = dict(dimension=dim, df_mode=df_mode, include_baryon=baryon, kernel_variant=variant)
    return _two_runs(lambda n, ws: api.Plan(inputs.species(which), _grid(n_pT), df, dict(opts, workspace_bytes=ws), max_cells=n, fq=fq), tens, 0)


def run_vah_case(api, c):
    from is3d_amd import inputs
    dim, tables, n_pT, which, variant = c
    cells, tens = _surface("vah", dim, 0)
    tab = inputs.vah_df_tables() if tables else None
    if tables:
        tens = {k: v for k, v in tens.items() if k not in ("c0", "c1", "c2", "c3", "c4")}
    opts = dict(dimension=dim, kernel_variant=variant)
    # the interpolated coefficients (5 doubles per cell of max_cells) are workspace but not a stream of the pass
    return _two_runs(lambda n, ws: api.VahPlan(inputs.species(which), _grid(n_pT), dict(opts, workspace_bytes=ws), tab=tab, max_cells=n), tens, 40 if tables else 0)


@pytest.fixture(scope="module")
def golden():
    from is3d_amd import api
    with open(GOLDEN) as f:
        return json.load(f)["developer" if api.DEV_LIB else "shipped"]


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_plan_shape(golden, c):
    from is3d_amd import api
    shape, spectra = run_case(api, c)
    print(case_id(c), shape)
    assert shape["n_passes"] == [1, 3]
    assert shape == golden[case_id(c)]
    assert np.all(np.isfinite(spectra[0])) and np.all(np.isfinite(spectra[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("c", VAH_CASES, ids=case_id)
def test_vah_plan_shape(golden, c):
    from is3d_amd import api
    shape, spectra = run_vah_case(api, c)
    print("vah-" + case_id(c), shape)
    assert shape["n_passes"] == [1, 3]
    assert shape == golden["vah-" + case_id(c)]
    assert np.all(np.isfinite(spectra[0])) and np.all(np.isfinite(spectra[1]))


def all_shapes(api, keep_spectra=False):
    """{case id: shape} (and the spectra) of every configuration through `api` -- the recorder, and the comparison of two builds in one process"""
    shapes, spectra = {}, {}
    for prefix, cases, run in (("", CASES, run_case), ("vah-", VAH_CASES, run_vah_case)):
        for c in cases:
            try:
                shapes[prefix + case_id(c)], spectra[prefix + case_id(c)] = run(api, c)
            except (api.Is3dError, AssertionError) as e:   # a configuration the library refuses is recorded as that; no test then matches it
                shapes[prefix + case_id(c)], spectra[prefix + case_id(c)] = dict(error=str(e)), []
                print(prefix + case_id(c), "FAILED:", e, flush=True)
    return (shapes, spectra) if keep_spectra else shapes


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, help="JSON file to write (or update) with the section of the library that is loaded")
    ap.add_argument("--lib", help="directory of the libis3d_amd.so to record from (default: the one is3d_amd.api loads)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from is3d_amd import api
    if a.lib:
        api.LIB_PATH = os.path.join(a.lib, "libis3d_amd.so")
    dev = "DEV" in api.load().is3d_version().decode()
    doc = json.load(open(a.record)) if os.path.exists(a.record) else {}
    doc["developer" if dev else "shipped"] = all_shapes(api)
    with open(a.record, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print("recorded", len(doc["developer" if dev else "shipped"]), "configurations from", api.LIB_PATH)
