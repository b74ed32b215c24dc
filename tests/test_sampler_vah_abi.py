"""The C ABI of the anisotropic-hydro particle sampler (is3d_sample_particles_vah, is3d_sample_particles_vah_multi) where no GPU is needed:
the symbols, every refusal the header lists (IS3D_EINVAL before any device use: the resource counters stand still) and the no-CPU-path rule."""
import numpy as np
import pytest

from is3d_amd import api, inputs, synth


@pytest.fixture(scope="module")
def good():
    return dict(cells=synth.synth_vah_surface(5, 3, seed=21), sp=inputs.species([211, 321, 2212, -2212]), gla=inputs.feqmod_tables(0.15),
                tab=inputs.vah_df_tables())


def test_the_two_symbols_exist():
    lib = api.load()
    for name in ("is3d_sample_particles_vah", "is3d_sample_particles_vah_multi"):
        assert name in api.EXPORTS and hasattr(lib, name), name


def without(cells, *names):
    return {k: v for k, v in cells.items() if k not in names}


REFUSALS = {
    "fast": lambda g: dict(fast=1),
    "feqmod": lambda g: dict(fq=g["gla"]),
    "n_events-0": lambda g: dict(n_events=0),
    "n_events-negative": lambda g: dict(n_events=-3),
    "n_gla-0": lambda g: dict(gla=dict(root1=np.zeros(0), weight1=np.zeros(0))),
    "n_gla-257": lambda g: dict(gla=dict(root1=np.ones(257), weight1=np.ones(257))),
    "no-Lambda": lambda g: dict(cells=without(g["cells"], "Lambda")),
    "no-aL": lambda g: dict(cells=without(g["cells"], "aL")),
    "no-eta-3d": lambda g: dict(cells=without(g["cells"], "eta")),
    "no-c3-without-tables": lambda g: dict(cells=without(g["cells"], "c3")),
    "no-pitn-with-shear": lambda g: dict(cells=without(g["cells"], "pitn")),
    "no-bulkPi-with-bulk": lambda g: dict(cells=without(g["cells"], "bulkPi")),
    "no-Wy-with-shear": lambda g: dict(cells=without(g["cells"], "Wy")),
    "dimension-4": lambda g: dict(opts=dict(dimension=4)),
}


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_come_before_any_device_use(good, case, multi):
    kw = dict(cells=good["cells"], gla=good["gla"], opts=dict(dimension=3), n_events=2, seed=3)
    kw.update(REFUSALS[case](good))
    cells, gla, opts = kw.pop("cells"), kw.pop("gla"), kw.pop("opts")
    if multi:
        kw["devices"] = [0, 0]
    before = api.resource_counters()
    with pytest.raises(api.Is3dError) as e:
        api.sample_particles_vah(cells, good["sp"], gla, opts, **kw)
    assert e.value.code == api.IS3D_EINVAL, str(e.value)
    assert api.resource_counters() == before


def test_arrays_that_are_not_read_may_be_missing(good):
    """T is never read; c0..c4 not with the tables; pi_perp, W and bulkPi not with their delta-f terms off; eta not in 2+1D: such a call is
    refused for no NULL array -- it reaches the device check (IS3D_ENODEVICE without one, a list with one)."""
    have_gpu = api.load().is3d_device_count() > 0
    lean = without(good["cells"], "T", "c0", "c1", "c2", "c3", "c4")
    bare = without(good["cells"], "T", "pitt", "pitx", "pity", "pitn", "pixx", "pixy", "pixn", "piyy", "piyn", "pinn", "Wx", "Wy", "bulkPi")
    flat = without(synth.synth_vah_surface(5, 2, seed=21), "eta")
    for cells, opts, tab in ((lean, dict(dimension=3), good["tab"]), (bare, dict(dimension=3, include_shear_deltaf=0, include_bulk_deltaf=0), None),
                             (flat, dict(dimension=2), None)):
        if have_gpu:
            api.sample_particles_vah(cells, good["sp"], good["gla"], opts, tab=tab, n_events=1)
            continue
        with pytest.raises(api.Is3dError) as e:
            api.sample_particles_vah(cells, good["sp"], good["gla"], opts, tab=tab, n_events=1)
        assert e.value.code == api.IS3D_ENODEVICE, str(e.value)


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_a_good_call_has_no_cpu_path(good, multi):
    kw = dict(devices=[0, 0]) if multi else {}
    if api.load().is3d_device_count() > 0:
        api.sample_particles_vah(good["cells"], good["sp"], good["gla"], dict(dimension=3), n_events=2, seed=3, **kw)
        return
    with pytest.raises(api.Is3dError) as e:
        api.sample_particles_vah(good["cells"], good["sp"], good["gla"], dict(dimension=3), n_events=2, seed=3, **kw)
    assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
