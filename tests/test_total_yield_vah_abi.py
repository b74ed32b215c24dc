"""CPU: the C ABI of the anisotropic-hydro mean yield -- is3d_total_yield_vah and is3d_oversample_events are exported, declared and bound
as include/is3d_amd.h declares them; every IS3D_EINVAL refusal comes before any device use; a good call has no CPU path; the events rule."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from is3d_amd import api, inputs, synth


@pytest.fixture(scope="module")
def sp():
    return inputs.species([211, 321, 2212, -2212])


@pytest.fixture(scope="module")
def gla():
    return inputs.feqmod_tables(0.15)


def header():
    return open(os.path.join(ROOT, "include", "is3d_amd.h")).read()


def test_symbols_are_exported_declared_and_bound(tmp_path):
    lib = api.load()
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    flat = " ".join(text.split())
    for name in ("is3d_total_yield_vah", "is3d_oversample_events"):
        assert name in api.EXPORTS and hasattr(lib, name), name
    assert ("int is3d_total_yield_vah(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab , "
            "const is3d_sampler_inputs *in , const is3d_options *opts, double *mean_yield, double *yield_by_species , "
            "is3d_yield_vah_stats *stats );") in flat
    assert "int is3d_oversample_events(double min_num_hadrons, double mean_yield, int32_t max_num_samples, int32_t *n_events);" in flat
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    c_syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"is3d_total_yield_vah", "is3d_oversample_events"} <= c_syms
    # the ctypes mirror of the stats struct is what a C compiler makes of the header
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "is3d_amd.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(is3d_yield_vah_stats),'
                   'offsetof(is3d_yield_vah_stats, n_classes), offsetof(is3d_yield_vah_stats, ms_h2d), offsetof(is3d_yield_vah_stats, ms_classes));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = api.YieldVahStats
    assert c == [ctypes.sizeof(S), S.n_classes.offset, S.ms_h2d.offset, S.ms_classes.offset]


def refused(call):
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        call()
    assert e.value.code == api.IS3D_EINVAL, str(e.value)
    assert api.resource_counters() == before, "a refused call used the device"
    return str(e.value)


def test_refusals_come_before_any_device_use(sp, gla):
    v3, v2 = dict(synth.synth_vah_surface(9, 3, seed=5)), dict(synth.synth_vah_surface(9, 2, seed=6))
    tab = inputs.vah_df_tables()

    def without(v, *fields):
        return {k: a for k, a in v.items() if k not in fields}

    refused(lambda: api.total_yield_vah(v3, sp, gla, dict(dimension=4)))
    refused(lambda: api.total_yield_vah(v3, sp, gla, dict(dimension=1)))
    refused(lambda: api.total_yield_vah(v3, sp, dict(root1=[], weight1=[]), dict(dimension=3)))
    refused(lambda: api.total_yield_vah(v3, sp, dict(root1=np.ones(257), weight1=np.ones(257)), dict(dimension=3)))
    assert "fast" in refused(lambda: api.total_yield_vah(v3, sp, gla, dict(dimension=3), fast=1))
    assert "feqmod" in refused(lambda: api.total_yield_vah(v3, sp, gla, dict(dimension=3), fq=gla))
    assert "y_cut" in refused(lambda: api.total_yield_vah(v2, sp, gla, dict(dimension=2), y_cut=0.0))
    refused(lambda: api.total_yield_vah(v2, sp, gla, dict(dimension=2), y_cut=-0.5))
    refused(lambda: api.total_yield_vah(v3, {k: a[:0] for k, a in sp.items()}, gla, dict(dimension=3)))
    refused(lambda: api.total_yield_vah(v3, sp, gla, dict(dimension=3), first_cell=-1))
    # a NULL cell array that would be read ...
    for f in ("ux", "un", "dat", "dan", "Lambda", "aL"):
        assert "NULL" in refused(lambda: api.total_yield_vah(without(v3, f), sp, gla, dict(dimension=3, include_bulk_deltaf=0, include_shear_deltaf=0)))
    refused(lambda: api.total_yield_vah(without(v3, "bulkPi"), sp, gla, dict(dimension=3, include_shear_deltaf=0)))
    refused(lambda: api.total_yield_vah(without(v3, "c2"), sp, gla, dict(dimension=3, include_shear_deltaf=0)))
    refused(lambda: api.total_yield_vah(without(v3, "c4"), sp, gla, dict(dimension=3, include_bulk_deltaf=0)))
    refused(lambda: api.total_yield_vah(without(v3, "pinn"), sp, gla, dict(dimension=3, include_bulk_deltaf=0), tab=tab))
    # ... NULL arguments of the C entry itself
    L = api.load()
    y = ctypes.c_double(0.0)
    before = api.resource_counters()
    assert L.is3d_total_yield_vah(None, None, None, None, None, ctypes.byref(y), None, None) == api.IS3D_EINVAL
    n = ctypes.c_int32(0)
    L.is3d_oversample_events.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    assert L.is3d_oversample_events(1.0e5, 250.0, 1000, None) == api.IS3D_EINVAL
    assert api.resource_counters() == before


def test_arrays_that_are_not_read_may_be_null_and_there_is_no_cpu_path(sp, gla):
    """T, eta, Wx, Wy and c3 are never read; pi_perp and c4 only with shear, bulkPi and c0..c2 only with bulk, the coefficients only without the
    tables: such a call is a good one -- IS3D_ENODEVICE without a device, a yield with one."""
    v = dict(synth.synth_vah_surface(9, 3, seed=5))
    v["bulkPi"] = 0.02 * v["bulkPi"]
    never = ("T", "eta", "Wx", "Wy", "c3")
    shear_only = ("pitt", "pitx", "pity", "pitn", "pixx", "pixy", "pixn", "piyy", "piyn", "pinn", "c4")
    bulk_only = ("bulkPi", "c0", "c1", "c2")
    calls = [lambda: api.total_yield_vah({k: a for k, a in v.items() if k not in never}, sp, gla, dict(dimension=3)),
             lambda: api.total_yield_vah({k: a for k, a in v.items() if k not in never + shear_only}, sp, gla, dict(dimension=3, include_shear_deltaf=0)),
             lambda: api.total_yield_vah({k: a for k, a in v.items() if k not in never + bulk_only}, sp, gla, dict(dimension=3, include_bulk_deltaf=0)),
             lambda: api.total_yield_vah({k: a for k, a in v.items() if k not in never + ("c0", "c1", "c2", "c4")}, sp, gla, dict(dimension=3),
                                         tab=inputs.vah_df_tables()),
             lambda: api.total_yield_vah({k: a[:0] for k, a in v.items()}, sp, gla, dict(dimension=3))]
    if api.load().is3d_device_count() == 0:
        for call in calls:
            with pytest.raises(api.Is3dError) as e:
                call()
            assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
    else:
        for call in calls[:-1]:
            N, by, st = call()
            assert np.isfinite(N) and N > 0.0 and np.all(by > 0.0) and st["n_classes"] == 3
        N, by, st = calls[-1]()
        assert N == 0.0 and not by.any()


def test_oversample_events():
    assert api.oversample_events(1.0e5, 250.0, 1000) == 400
    assert api.oversample_events(1.0e5, 10.0, 1000) == 1000
    assert api.oversample_events(10, 1.0e6, 1000) == 1
    assert api.oversample_events(1.0e5, -250.0, 1000) == 400          # the reference takes the magnitude; the run driver refuses a yield <= 0 earlier
    for bad in (0.0, -0.0, float("nan"), float("inf")):
        with pytest.raises(api.Is3dError) as e:
            api.oversample_events(1.0e5, bad, 1000)
        assert e.value.code == api.IS3D_EDOMAIN, bad
    for hadrons, samples in ((0.0, 1000), (-5.0, 1000), (float("nan"), 1000), (1.0e5, 0), (1.0e5, -3)):
        with pytest.raises(api.Is3dError) as e:
            api.oversample_events(hadrons, 250.0, samples)
        assert e.value.code == api.IS3D_EINVAL, (hadrons, samples)
