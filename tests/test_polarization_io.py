"""CPU: the spin polarization's host side -- the writer (is3d_write_polarization) against a small g++ / iostream program that does what
write_polzn_vector_toFile does (emissionfunction.cpp:775-821), the mode-5 reader's thermal vorticity (readindata.cpp:470-551) and its
sidecar, and the argument checks of is3d_spin_polarization, which run before any device use."""
import os
import struct
import subprocess

import numpy as np
import pytest

from is3d_amd import api, synth

# the loop and the stream expression of write_polzn_vector_toFile (emissionfunction.cpp:775-821), reading the raw arrays from a binary file:
# int32 npart, npT, nphi, ny, dim; then pT, phi, y, St, Sx, Sy, Sn, Snorm as doubles
WRITER_CPP = r'''
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <string>
#include <vector>
using namespace std;
int main(int argc, char **argv)
{
    FILE *in = fopen(argv[1], "rb");
    int hdr[5];
    if (fread(hdr, sizeof(int), 5, in) != 5) return 1;
    const int npart = hdr[0], npT = hdr[1], nphi = hdr[2], ny = hdr[3], dim = hdr[4];
    const int y_pts = dim == 2 ? 1 : ny;
    const size_t n = (size_t)npart * npT * nphi * y_pts;
    vector<double> pT(npT), phi(nphi), y(ny), S[5];
    if (fread(pT.data(), 8, npT, in) != (size_t)npT || fread(phi.data(), 8, nphi, in) != (size_t)nphi || fread(y.data(), 8, ny, in) != (size_t)ny) return 1;
    for (int m = 0; m < 5; m++) { S[m].resize(n); if (fread(S[m].data(), 8, n, in) != n) return 1; }
    fclose(in);
    const char *names[4] = {"St.dat", "Sx.dat", "Sy.dat", "Sn.dat"};
    for (int m = 0; m < 4; m++) {
        ofstream F(string(argv[2]) + "/" + names[m], ios_base::app);
        for (int ipart = 0; ipart < npart; ipart++) {
            for (int iy = 0; iy < y_pts; iy++) {
                double yy;
                if (dim == 2) yy = 0.0;
                else yy = y[iy];
                for (int iphip = 0; iphip < nphi; iphip++) {
                    double phip = phi[iphip];
                    for (int ipT = 0; ipT < npT; ipT++) {
                        double pt = pT[ipT];
                        long long int iS3D = (long long int)ipart + (long long int)npart * ((long long int)ipT + (long long int)npT * ((long long int)iphip + (long long int)nphi * (long long int)iy));
                        F << scientific << setw(5) << setprecision(8) << yy << "\t" << phip << "\t" << pt << "\t" << (S[m][iS3D] / S[4][iS3D]) << "\n";
                    }
                    F << "\n";
                }
            }
        }
    }
    return 0;
}
'''

NAMES = ["St.dat", "Sx.dat", "Sy.dat", "Sn.dat"]


@pytest.fixture(scope="module")
def writer_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("polzn_writer")
    src = d / "w.cpp"
    src.write_text(WRITER_CPP)
    exe = str(d / "w")
    subprocess.check_call(["g++", "-O0", "-std=c++11", str(src), "-o", exe])
    return exe


def _case(dim, kind, seed=5):
    rng = np.random.default_rng(seed)
    npart, npT, nphi, ny = 3, 4, 5, 3
    pT = np.linspace(0.01, 3.0, npT)
    phi = np.linspace(0.0, 6.0, nphi)
    y = np.array([-5.0, 0.0, 2.5])
    n = npart * npT * nphi * (1 if dim == 2 else ny)
    res = {k: rng.normal(size=n) * 10.0 ** rng.integers(-30, 30, size=n) for k in api.POLARIZATION_OUTPUTS}
    if kind == "special":
        res["Snorm"][::7] = 0.0                       # x / 0 = +-inf, 0 / 0 = nan (printed "-nan" when the sign bit is set)
        res["St"][::7] = 0.0
        res["Sx"][1::7] = np.inf
        res["Sy"][2::7] = -np.inf
        res["Sn"][3::7] = np.nan
        res["Snorm"][4::7] = 5e-324                   # subnormal denominator and numerators
        res["St"][5::7] = 2.2e-310
        res["Sx"][6::7] = -0.0
    return dict(npart=npart, pT=pT, phi=phi, y=y, res=res)


def _run_reference(exe, tmp, dim, c):
    raw = tmp / "raw.bin"
    with open(raw, "wb") as f:
        f.write(struct.pack("5i", c["npart"], len(c["pT"]), len(c["phi"]), len(c["y"]), dim))
        for a in (c["pT"], c["phi"], c["y"]) + tuple(c["res"][k] for k in api.POLARIZATION_OUTPUTS):
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    subprocess.check_call([exe, str(raw), str(tmp)])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", ["normal", "special"])
def test_writer_matches_iostream(tmp_path, writer_exe, dim, kind):
    c = _case(dim, kind)
    ref, got = tmp_path / "ref", tmp_path / "got"
    ref.mkdir()
    got.mkdir()
    _run_reference(writer_exe, ref, dim, c)
    api.write_polarization(str(got), dim, c["pT"], c["phi"], c["y"] if dim == 3 else None, c["res"], n_species=c["npart"])
    for name in NAMES:
        a, b = (got / name).read_bytes(), (ref / name).read_bytes()
        assert a == b, name
        assert len(a) > 0
    if kind == "special":
        text = (got / "Sn.dat").read_text()
        assert "nan" in text and "inf" in text
    # ios_base::app: a second write appends the same block
    api.write_polarization(str(got), dim, c["pT"], c["phi"], c["y"] if dim == 3 else None, c["res"], n_species=c["npart"])
    for name in NAMES:
        assert (got / name).read_bytes() == (ref / name).read_bytes() * 2, name


def test_writer_missing_directory(tmp_path):
    c = _case(3, "normal")
    with pytest.raises(api.Is3dError) as e:
        api.write_polarization(str(tmp_path / "absent"), 3, c["pT"], c["phi"], c["y"], c["res"], n_species=c["npart"])
    assert e.value.code == -5


# ---- the mode-5 reader ----------------------------------------------------------------------
def write_mode5(path, s, w):
    """A mode-5 surface.dat (read_surf_VH_Vorticity, readindata.cpp:470-551): the mode-1 columns, then wtx wty wtn wxy wxn wyn."""
    h = synth.HBARC
    cols = [s["tau"], s["x"], s["y"], s["eta"], s["dat"], s["dax"], s["day"], s["dan"], s["ux"], s["uy"], s["un"],
            s["E"] / h, s["T"] / h, s["P"] / h, s["pixx"] / h, s["pixy"] / h, s["pixn"] / h, s["piyy"] / h, s["piyn"] / h, s["bulkPi"] / h]
    cols += [w[f] for f in synth.VORTICITY_FIELDS]
    np.savetxt(path, np.column_stack(cols), fmt="%.17e", delimiter=" ")


@pytest.fixture
def mode5_file(tmp_path):
    s = synth.synth_surface(57, 3, seed=91)
    w = synth.synth_vorticity(57, seed=92)
    p = str(tmp_path / "surface.dat")
    write_mode5(p, s, w)
    return p, s, w


def test_vorticity_equals_text_columns(mode5_file):
    p, _, w = mode5_file
    got, source = api.surface_vorticity(p, cache=0)
    assert source == 0
    tab = np.loadtxt(p, ndmin=2)
    for k, f in enumerate(synth.VORTICITY_FIELDS):
        assert np.array_equal(got[f], tab[:, 20 + k]), f
        assert np.array_equal(got[f], w[f]), f


def test_vorticity_sidecar_round_trip(mode5_file):
    p, _, _ = mode5_file
    first, s1 = api.surface_vorticity(p, cache=1)
    assert s1 == 1 and os.path.exists(p + ".is3dcache")
    second, s2 = api.surface_vorticity(p, cache=1)
    assert s2 == 2
    for f in synth.VORTICITY_FIELDS:
        assert first[f].tobytes() == second[f].tobytes(), f
    a1, _, _ = api.surface_open(p, mode=5, cache=0)
    a2, _, src = api.surface_open(p, mode=5, cache=1)
    assert src == 2
    for k in a1:
        assert (a1[k] is None and a2[k] is None) or a1[k].tobytes() == a2[k].tobytes(), k


def test_sidecar_without_vorticity_is_reparsed(mode5_file):
    """A mode-5 sidecar as the build before this one wrote it (the 25 arrays only, array_mask bits 25-30 clear) is never served."""
    p, _, w = mode5_file
    _, s1 = api.surface_vorticity(p, cache=1)
    assert s1 == 1
    cp = p + ".is3dcache"
    blob = bytearray(open(cp, "rb").read())
    n = struct.unpack_from("<q", blob, 64)[0]
    mask = struct.unpack_from("<Q", blob, 72)[0]
    assert n == 57 and (mask >> 25) & 0x3F == 0x3F
    struct.pack_into("<Q", blob, 72, mask & ~(0x3F << 25))
    with open(cp, "wb") as f:
        f.write(bytes(blob[:len(blob) - 6 * 8 * n]))
    got, s2 = api.surface_vorticity(p, cache=1)
    assert s2 == 1   # parsed again (and the sidecar rewritten)
    for f in synth.VORTICITY_FIELDS:
        assert np.array_equal(got[f], w[f]), f
    _, s3 = api.surface_vorticity(p, cache=1)
    assert s3 == 2


def test_other_modes_have_no_vorticity(tmp_path):
    s = synth.synth_surface(9, 3, seed=93)
    p = str(tmp_path / "surface.dat")
    synth.write_surface_dat(p, s)
    L = api.load()
    h = api.C.c_void_p()
    assert L.is3d_surface_open(p.encode(), 1, 0, 0, 3, 0, api.C.byref(h)) == 0
    try:
        ptrs = (api._dp * 6)()
        assert L.is3d_surface_vorticity(h, ptrs) == -1
        assert b"mode-5" in L.is3d_last_error()
    finally:
        L.is3d_surface_close(h)


def test_mode5_keeps_25_array_contract(mode5_file):
    p, s, _ = mode5_file
    arrs, avg, _ = api.surface_open(p, mode=5, cache=0)
    ref, ref_avg = api.surface_read(p, 5)
    assert set(arrs) == set(api.SURFACE_READ_ORDER) | {"x", "y"}
    for f in api.SURFACE_READ_ORDER:
        if arrs[f] is not None:
            assert np.array_equal(arrs[f], ref[f]), f
    assert np.array_equal(avg, ref_avg)
    assert np.array_equal(arrs["x"], s["x"]) and np.array_equal(arrs["y"], s["y"])
    # asking for 31 arrays is refused: the vorticity comes through is3d_surface_vorticity only
    L = api.load()
    h = api.C.c_void_p()
    assert L.is3d_surface_open(p.encode(), 5, 0, 0, 3, 0, api.C.byref(h)) == 0
    try:
        ptrs = (api._dp * 31)()
        assert L.is3d_surface_arrays(h, ptrs, 31, None) == -1
    finally:
        L.is3d_surface_close(h)


# ---- argument checks (before any device use) ------------------------------------------------
def _inputs(dim=3, n=4):
    from is3d_amd import inputs
    g = inputs.grid()
    grid = dict(pT=g["pT"][:3], phi=g["phi"][:4], y=g["y"][:3], eta=g["eta"], eta_w=g["eta_w"])
    sp = {k: np.asarray(v)[:3] for k, v in inputs.species("pikp").items() if k in ("mass", "sign", "degeneracy", "baryon")}
    cells = synth.synth_surface(n, dim, seed=94)
    w = synth.synth_vorticity(n)
    return cells, w, sp, grid


def _einval(*args, **kw):
    with pytest.raises(api.Is3dError) as e:
        api.spin_polarization(*args, **kw)
    assert e.value.code == -1, str(e.value)
    return str(e.value)


def test_argument_checks():
    cells, w, sp, grid = _inputs()
    assert "vorticity" in _einval(cells, None, sp, grid, 0.15, dict(dimension=3))
    _einval(cells, dict(w, wxn=None), sp, grid, 0.15, dict(dimension=3))
    assert "NULL" in _einval(dict(cells, tau=None), w, sp, grid, 0.15, dict(dimension=3))
    _einval(dict(cells, eta=None), w, sp, grid, 0.15, dict(dimension=3))
    _einval(dict(cells, dan=None), w, sp, grid, 0.15, dict(dimension=3))
    for T in (0.0, -0.1, float("nan"), float("inf")):
        assert "temperature" in _einval(cells, w, sp, grid, T, dict(dimension=3))
    for m in (0.0, -0.2):
        bad = dict(sp, mass=np.array([0.138, m, 0.938]))
        assert "mass" in _einval(cells, w, bad, grid, 0.15, dict(dimension=3))
    c2, w2, _, _ = _inputs(dim=2)
    for k in (0, 1):
        g1 = dict(grid, eta=grid["eta"][:k], eta_w=grid["eta_w"][:k])
        assert "eta" in _einval(c2, w2, sp, g1, 0.15, dict(dimension=2))
    _einval(cells, w, sp, grid, 0.15, dict(dimension=4))
