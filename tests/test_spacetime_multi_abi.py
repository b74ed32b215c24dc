"""CPU: is3d_spacetime_distributions_multi (operation 0 sharded over devices) is exported and bound, refuses bad arguments with
IS3D_EINVAL and a message that names the argument -- before any device is used, so on a box with or without a GPU alike -- and, given good
arguments on a box without a GPU, fails with IS3D_ENODEVICE instead of computing on the host."""
import numpy as np
import pytest

import offtile_cases as OC
from is3d_amd import api


def inputs_of(dim=3, df_mode=1, n_cells=5):
    return OC.op0_inputs(dim, (3, 5, 4), df_mode, OC.THREE, n_cells, {}, False, 4242)


def call(b, devices, **over):
    a = dict(b, **over)
    return api.spacetime_distributions_multi(a["cells"], a["sp"], a["grid"], a["df"], a["bins"], a["opts"], devices, fq=a["fq"])


def test_symbol_is_exported_and_bound():
    lib = api.load()
    assert "is3d_spacetime_distributions_multi" in api.EXPORTS
    assert hasattr(lib, "is3d_spacetime_distributions_multi")
    assert len(lib.is3d_spacetime_distributions_multi.argtypes) == 16
    assert callable(api.spacetime_distributions_multi)


def without(cells, *names):
    return {k: v for k, v in cells.items() if k not in names}


REFUSALS = [
    ("null-x", lambda b: dict(cells=without(b["cells"], "x")), [0, 0], "x and y"),
    ("null-y", lambda b: dict(cells=without(b["cells"], "y")), [0, 0], "x and y"),
    ("tau-bins-0", lambda b: dict(bins=dict(b["bins"], tau_bins=0)), [0, 0], "tau_bins"),
    ("r-bins-0", lambda b: dict(bins=dict(b["bins"], r_bins=0)), [0, 0], "r_bins"),
    ("empty-tau-range", lambda b: dict(bins=dict(b["bins"], tau_max=b["bins"]["tau_min"])), [0, 0], "tau_max > tau_min"),
    ("empty-r-range", lambda b: dict(bins=dict(b["bins"], r_max=b["bins"]["r_min"])), [0, 0], "r_max > r_min"),
    ("65-pT", lambda b: dict(grid=OC.make_grid(65, 3, 2, 3, 5)), [0, 0], "64"),
    ("df-mode-3-without-fq", lambda b: dict(opts=dict(b["opts"], df_mode=3)), [0, 0], "fq is NULL"),
    ("df-mode-4-without-fq", lambda b: dict(opts=dict(b["opts"], df_mode=4)), [0, 0], "fq is NULL"),
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
    assert api.resource_counters() == before


def test_eta_count_past_the_lds_bound_is_refused():
    name, dim, shape, df_mode = OC.OP0_REFUSED[0]
    b = OC.op0_inputs(dim, shape, df_mode, OC.THREE, 2, {}, False, 77)
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        call(b, [0, 0])
    assert e.value.code == api.IS3D_EINVAL and "eta nodes" in str(e.value)
    assert api.resource_counters() == before


def test_fq_with_df_mode_1_is_refused():
    b = inputs_of(df_mode=4)
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        call(b, [0, 0], opts=dict(b["opts"], df_mode=1))
    assert e.value.code == api.IS3D_EINVAL and "fq is given but df_mode is 1" in str(e.value)
    assert api.resource_counters() == before


@pytest.mark.parametrize("df_mode", [2, 4])
def test_good_call_without_a_device_is_enodevice(df_mode):
    """(with a GPU the same call computes: tests/test_gpu_spacetime_multi.py)"""
    b = inputs_of(df_mode=df_mode)
    if api.load().is3d_device_count() > 0:
        res = call(b, [0, 0, 0])
        assert np.isfinite(res["dN_dy"]).all() and len(res["shard_stats"]) == 3
        return
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        call(b, [0, 0, 0])
    assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
    assert e.value.stats["code"] == api.IS3D_ENODEVICE
    assert api.resource_counters() == before
