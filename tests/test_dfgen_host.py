"""CPU: the host side of the df-coefficient generator -- is3d_df_tables_write against the reference's 30 shipped files, the round trip through
both readers, is3d_df_generate's argument checks (before any device use) and its refusal to compute without a device (no CPU path)."""
import ctypes as C
import os

import numpy as np
import pytest

from is3d_amd import api, inputs

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = inputs.DF_NAMES_2D


def pdg_urqmd():
    a = np.array(inputs.load_fixture()["pdg_urqmd"], dtype=np.float64)        # columns: mc_id, mass, gspin, baryon, sign
    return dict(mass=a[:, 1].copy(), gspin=a[:, 2].copy(), baryon=a[:, 3].copy(), sign=a[:, 4].copy())


def rule():
    z = np.load(os.path.join(HERE, "golden", "golden_dfcoef.npz"))
    return z["root"], z["weight"]


@pytest.mark.parametrize("which", ["urqmd", "smash", "smash_box"])
def test_writer_reproduces_the_shipped_files_byte_for_byte(which, reference, tmp_path):
    """The ten shipped files of a list, parsed and written again: the same bytes (count lines, label line, setw(8) fixed rows, mu_B outer)."""
    src = os.path.join(reference, "deltaf_coefficients", "vh", which)
    tabs = []
    for n in NAMES:
        T, B, v = api.df_table_read_full(os.path.join(src, n + ".dat"))
        tabs.append(v)
    assert np.array(tabs).shape == (10, 81, 101)
    out = str(tmp_path / which)
    api.df_tables_write(out, T, B, np.array(tabs))
    assert sorted(os.listdir(out)) == sorted(n + ".dat" for n in NAMES)
    for n in NAMES:
        assert open(os.path.join(out, n + ".dat"), "rb").read() == open(os.path.join(src, n + ".dat"), "rb").read(), n


def test_round_trip_through_both_readers_and_no_overwrite(tmp_path):
    """An off-shape grid (3 T x 2 mu_B, descending T, negative values) read back by is3d_df_table_read_full and is3d_df_table_read: the values
    rounded to the six printed decimals; a second write into the same directory is refused and leaves the files alone."""
    rng = np.random.default_rng(5)
    T, B = np.array([0.3, 0.1234, 0.05]), np.array([0.0, 0.4567])
    tab = rng.normal(size=(10, 2, 3)) * np.array([1e-3, 1, 10, 100, 1e3, 1, 1, 1, 1, 2000]).reshape(10, 1, 1)
    out = str(tmp_path / "t" / "")                                             # a trailing slash is accepted
    api.df_tables_write(out, T, B, tab)
    rounded = lambda a: np.array([float("%.6f" % x) for x in np.ravel(a)]).reshape(np.shape(a))
    for k, n in enumerate(NAMES):
        Tf, Bf, v = api.df_table_read_full(os.path.join(out, n + ".dat"))
        assert np.array_equal(Tf, rounded(T)) and np.array_equal(Bf, rounded(B)) and np.array_equal(v, rounded(tab[k])), n
        T1, v1 = api.df_table_read(os.path.join(out, n + ".dat"))
        assert np.array_equal(T1, Tf) and np.array_equal(v1, v[0])
    before = open(os.path.join(out, "F.dat"), "rb").read()
    with pytest.raises(api.Is3dError) as e:
        api.df_tables_write(out, T, B, tab + 1.0)
    assert e.value.code == api.IS3D_EINVAL and "never overwritten" in str(e.value)
    assert open(os.path.join(out, "F.dat"), "rb").read() == before
    bad = tab.copy()
    bad[7, 1, 2] = np.nan
    with pytest.raises(api.Is3dError) as e:
        api.df_tables_write(str(tmp_path / "nan"), T, B, bad)
    assert e.value.code == api.IS3D_EINVAL and "betabulk" in str(e.value) and not os.path.exists(str(tmp_path / "nan"))
    with pytest.raises(api.Is3dError) as e:
        api.df_tables_write(str(tmp_path / "no" / "such" / "parent"), T, B, tab)
    assert e.value.code == api.IS3D_EIO


def test_generate_refuses_bad_arguments_before_any_device_use():
    """Every IS3D_EINVAL case, with or without a device, and no allocation made (is3d_resource_counters unchanged)."""
    pdg, (r, w) = pdg_urqmd(), rule()
    good = dict(pdg=pdg, root=r, weight=w, T=[0.15], muB=[0.1])
    nan = dict(pdg, gspin=np.where(np.arange(len(pdg["mass"])) == 5, np.nan, pdg["gspin"]))
    neg = dict(pdg, mass=np.where(np.arange(len(pdg["mass"])) == 7, -0.5, pdg["mass"]))
    rinf, rzero, wnan = r.copy(), r.copy(), w.copy()
    rinf[2, 3], rzero[4, 0], wnan[1, 63] = np.inf, 0.0, np.nan
    counters = api.resource_counters()
    for kw in (dict(good, pdg={k: v[:0] for k, v in pdg.items()}), dict(good, root=r[:, :0], weight=w[:, :0]), dict(good, T=[0.15, 0.0]),
               dict(good, T=[-0.1]), dict(good, T=[np.nan]), dict(good, T=[np.inf]), dict(good, muB=[np.inf]), dict(good, pdg=nan), dict(good, pdg=neg),
               dict(good, root=rinf), dict(good, root=rzero), dict(good, weight=wnan), dict(good, T=[]), dict(good, muB=[]), dict(good, device=-2)):
        with pytest.raises(api.Is3dError) as e:
            api.df_generate(**kw)
        assert e.value.code == api.IS3D_EINVAL, kw
    # null pointers, through the C ABI itself
    L = api.load()
    cols = [np.ascontiguousarray(pdg[k]) for k in ("mass", "gspin", "baryon", "sign")]
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)
    rows = [np.ascontiguousarray(r[a]) for a in range(1, 5)], [np.ascontiguousarray(w[a]) for a in range(1, 5)]
    r4, w4 = (dp * 4)(*[ptr(a) for a in rows[0]]), (dp * 4)(*[ptr(a) for a in rows[1]])
    r4_hole = (dp * 4)(ptr(rows[0][0]), None, ptr(rows[0][2]), ptr(rows[0][3]))
    hl = api.HadronList(len(cols[0]), *[ptr(c) for c in cols])
    hl_hole = api.HadronList(len(cols[0]), ptr(cols[0]), None, ptr(cols[2]), ptr(cols[3]))
    T, B, tab = np.array([0.15]), np.array([0.1]), np.zeros(10)
    call = lambda list_=C.byref(hl), root=r4, weight=w4, T_=ptr(T), B_=ptr(B), out=ptr(tab): L.is3d_df_generate(list_, 64, root, weight, 1, T_, 1, B_, -1, out, None, None)
    for rc in (call(list_=None), call(root=None), call(weight=None), call(T_=None), call(B_=None), call(out=None), call(root=r4_hole), call(list_=C.byref(hl_hole))):
        assert rc == api.IS3D_EINVAL
    assert L.is3d_df_tables_write(None, 1, ptr(T), 1, ptr(B), ptr(np.zeros(10))) == api.IS3D_EINVAL
    assert L.is3d_df_tables_write(b"x", 1, ptr(T), 1, ptr(B), None) == api.IS3D_EINVAL
    assert api.resource_counters() == counters


def test_generate_has_no_cpu_path():
    """A good call without a device is IS3D_ENODEVICE; with one it computes (the gpu tests say what)."""
    pdg, (r, w) = pdg_urqmd(), rule()
    if api.load().is3d_device_count() > 0:
        tab, integ, st = api.df_generate(pdg, r, w, [0.15], [0.1], with_integrals=True)
        assert np.all(np.isfinite(tab)) and np.all(np.isfinite(integ)) and st["n_massive"] == 326
        return
    with pytest.raises(api.Is3dError) as e:
        api.df_generate(pdg, r, w, [0.15], [0.1])
    assert e.value.code == api.IS3D_ENODEVICE and "no CPU path" in str(e.value)
