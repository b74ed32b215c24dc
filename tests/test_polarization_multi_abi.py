"""CPU: is3d_spin_polarization_multi (mode 5 sharded over devices) is exported with the declared signature, refuses bad arguments with
IS3D_EINVAL before any device is used or plan created -- so on a box with or without a GPU alike -- and, given good arguments on a box
without a GPU, fails with IS3D_ENODEVICE instead of computing on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from is3d_amd import api, inputs, synth

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "is3d_amd.h")


def inputs_of(n_cells=7):
    g = inputs.grid()
    grid = dict(pT=g["pT"][:5], phi=g["phi"][:5], y=g["y"][:4], eta=g["eta"], eta_w=g["eta_w"])
    sp = dict(mass=np.array([0.13957, 0.9383, 0.4937]), sign=np.array([-1.0, 1.0, -1.0]), degeneracy=np.array([1.0, 2.0, 1.0]),
              baryon=np.array([0.0, 1.0, 0.0]))
    return dict(cells=synth.synth_surface(n_cells, 3, seed=9191), w=synth.synth_vorticity(n_cells, seed=9192), sp=sp, grid=grid, T=0.15,
                opts=dict(dimension=3))


def call(b, devices, **over):
    a = dict(b, **over)
    return api.spin_polarization_multi(a["cells"], a["w"], a["sp"], a["grid"], a["T"], a["opts"], devices)


def test_symbol_is_exported_with_the_declared_signature():
    lib = api.load()
    assert "is3d_spin_polarization_multi" in api.EXPORTS
    assert hasattr(lib, "is3d_spin_polarization_multi")
    text = re.sub(r"\s+", " ", open(HEADER).read())
    m = re.search(r"int is3d_spin_polarization_multi\(([^)]*)\);", text)
    assert m, "the header does not declare is3d_spin_polarization_multi"
    params = [re.sub(r"\w+$", "", p.strip()).replace(" ", "") for p in m.group(1).split(",")]
    assert params == ["constis3d_cells*", "constis3d_vorticity*", "constis3d_species*", "constis3d_grid*", "double", "constis3d_options*",
                      "constint32_t*", "int32_t", "is3d_polarization_out*", "is3d_polarization_stats*", "is3d_polarization_stats*"]
    at = lib.is3d_spin_polarization_multi.argtypes
    assert len(at) == len(params) == 11
    assert at[4] is C.c_double and at[7] is C.c_int32 and at[6] == C.POINTER(C.c_int32)
    assert at[9] == at[10] == C.POINTER(api.PolarizationStats)
    # the stats struct keeps its layout
    assert C.sizeof(api.PolarizationStats) == 48
    assert callable(api.spin_polarization_multi)


def bad_mass(b):
    sp = {k: v.copy() for k, v in b["sp"].items()}
    sp["mass"][1] = 0.0
    return dict(sp=sp)


REFUSALS = [
    ("null-vorticity", lambda b: dict(w=None), [0, 0], "vorticity"),
    ("T-zero", lambda b: dict(T=0.0), [0, 0], "T > 0"),
    ("T-negative", lambda b: dict(T=-0.15), [0, 0], "T > 0"),
    ("mass-zero", bad_mass, [0, 0], "mass"),
    ("negative-ordinal", lambda b: {}, [0, -1, 0], "devices[1] = -1"),
    ("n-devices-beyond-visible", lambda b: {}, 999, "n_devices = 999"),
]


@pytest.mark.parametrize("name,change,devices,needle", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_precede_any_device_use(name, change, devices, needle):
    b = inputs_of()
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        call(b, devices, **change(b))
    assert e.value.code == api.IS3D_EINVAL, str(e.value)
    assert needle in str(e.value), str(e.value)
    assert e.value.stats["code"] == api.IS3D_EINVAL
    assert api.resource_counters() == before


def test_good_call_without_a_device_is_enodevice():
    """(with a GPU the same call computes: tests/test_gpu_polarization_multi.py)"""
    b = inputs_of()
    if api.load().is3d_device_count() > 0:
        res = call(b, [0, 0, 0])
        assert np.isfinite(res["Snorm"]).all() and len(res["shard_stats"]) == 3
        return
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        call(b, [0, 0, 0])
    assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
    assert e.value.stats["code"] == api.IS3D_ENODEVICE
    assert api.resource_counters() == before
