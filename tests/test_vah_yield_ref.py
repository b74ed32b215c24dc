"""CPU: the numpy restatement of is3d_total_yield_vah (tests/vah_yield_ref.py) against the CPU oracle's smooth VAH spectrum
(oracle.dN_pTdpTdphidy_vah, regulate_deltaf = 0: the linear delta-f, no outflow cut) integrated over momentum.

Grids: pT 96-point Gauss-Legendre on [0, 7] GeV, 48 uniform phi, y (3+1D) or eta (2+1D, eta_w = 1) trapezoid of step 0.1 on +-9.
Cells: synth_vah_surface(6, 3, seed=4321) with its own bulk pressure (the linear yields are negative there with bulk on: the breakdown the
sampler tests avoid) and synth_vah_surface(5, 2, seed=777) with bulkPi x 0.02; those with u.dsigma > 0 (the oracle skips none).  Species
pi+, K+, p, pbar.

Worst relative difference per case, measured when this test was written (species in list order):
    3+1D  bulk 0 shear 0: 3.05e-8   bulk 0 shear 1: 3.15e-8   bulk 1 shear 0: 1.98e-7   bulk 1 shear 1: 1.93e-7     (pion; K+, p, pbar <= 1.5e-8)
    2+1D  bulk 0 shear 0: 1.60e-8   bulk 0 shear 1: 1.63e-8   bulk 1 shear 0: 1.56e-8   bulk 1 shear 1: 1.60e-8     (pion; K+, p, pbar <= 2.9e-10)
The pion's figure is the 32-node Gauss-Laguerre quadrature of the restatement (the other species sit at the oracle's own grid error); the
bound asserted is 10 x the worst figure of the table, BOUND below, far under the 1e-4 that resolving the shear term (1e-2 of the yield) asks for."""
import numpy as np
import pytest

import vah_yield_ref as ref
from is3d_amd import inputs, synth
from oracle import oracle  # the checker

BOUND = 1.98e-6         # 10 x 1.98e-7
Y_NODES = np.arange(-90, 91) * 0.1
CASES = [(3, 6, 4321, 1.0), (2, 5, 777, 0.02)]       # dimension, cells, seed, bulkPi scale
Y_CUT = 0.7


@pytest.fixture(scope="module")
def sp():
    return inputs.species([211, 321, 2212, -2212])


@pytest.fixture(scope="module")
def gla():
    return inputs.feqmod_tables(0.15)


def momentum_grid():
    x, w = np.polynomial.legendre.leggauss(96)
    pT, pT_w = 3.5 * (x + 1.0), 3.5 * w
    phi = 2.0 * np.pi * np.arange(48) / 48.0
    yw = np.full(len(Y_NODES), 0.1)
    yw[0] = yw[-1] = 0.05
    return pT, pT_w, phi, np.full(48, 2.0 * np.pi / 48.0), yw


def cells_of(dim, n, seed, bulk_scale):
    v = dict(synth.synth_vah_surface(n, dim, seed=seed))
    v["bulkPi"] = bulk_scale * v["bulkPi"]
    uds, _ = ref.lrf_dsigma(v)
    assert np.count_nonzero(uds > 0.0) >= 3
    return {k: np.ascontiguousarray(a[uds > 0.0]) for k, a in v.items()}


def oracle_yield(v, sp, dim, bulk, shear):
    """the oracle's spectrum integrated over momentum: the whole rapidity range in 3+1D, dN/dy (y = 0) times 2 y_cut in 2+1D"""
    pT, pT_w, phi, phi_w, yw = momentum_grid()
    grid = dict(pT=pT, phi=phi, y=Y_NODES if dim == 3 else np.zeros(1), eta=Y_NODES if dim == 2 else np.zeros(1),
                eta_w=np.ones(len(Y_NODES)) if dim == 2 else np.ones(1))
    dN = oracle.dN_pTdpTdphidy_vah(v, sp, grid, dict(dimension=dim, regulate_deltaf=0, outflow=0, include_bulk_deltaf=bulk, include_shear_deltaf=shear))
    ny = len(Y_NODES) if dim == 3 else 1
    dN = dN.reshape(ny, len(phi), len(pT), len(sp["mass"]))                       # [iy][iphi][ipT][ipart]
    w_y = yw if dim == 3 else np.array([2.0 * Y_CUT])                             # (2+1D: the oracle's eta sum is the trapezoid but for its negligible ends)
    w = w_y[:, None, None, None] * phi_w[None, :, None, None] * (pT_w * pT)[None, None, :, None]
    return np.sum(w * dN, axis=(0, 1, 2))


@pytest.fixture(scope="module")
def table(sp, gla):
    """per (dimension, bulk, shear): the cells, the oracle's yields and the restatement's -- computed once"""
    out = {}
    for dim, n, seed, scale in CASES:
        v = cells_of(dim, n, seed, scale)
        for bulk in (0, 1):
            for shear in (0, 1):
                want = oracle_yield(v, sp, dim, bulk, shear)
                tot, by, skipped = ref.total_yield_vah_ref(v, sp, gla, dict(dimension=dim, include_bulk_deltaf=bulk, include_shear_deltaf=shear), y_cut=Y_CUT)
                assert skipped == 0 and tot == float(np.cumsum(by)[-1])
                out[(dim, bulk, shear)] = dict(cells=v, oracle=want, ref=by)
    return out


@pytest.mark.parametrize("shear", [0, 1])
@pytest.mark.parametrize("bulk", [0, 1])
@pytest.mark.parametrize("dim", [3, 2])
def test_restatement_matches_the_oracles_momentum_integral(table, dim, bulk, shear):
    t = table[(dim, bulk, shear)]
    rel = np.abs(t["ref"] - t["oracle"]) / np.abs(t["oracle"])
    print("dim %d bulk %d shear %d: restatement %s oracle %s relative difference %s" % (dim, bulk, shear, t["ref"], t["oracle"], rel))
    assert BOUND <= 1.0e-4
    assert np.all(rel <= BOUND), rel


@pytest.mark.parametrize("dim", [3, 2])
def test_the_comparison_resolves_the_shear_and_the_anisotropy_terms(table, sp, gla, dim):
    """shear on / off and alpha_L <-> 1 each move the restatement by more than 100 x the bound: the agreement above says something about them"""
    on, off = table[(dim, 1, 1)]["ref"], table[(dim, 1, 0)]["ref"]
    d_shear = np.abs(on - off) / np.abs(on)
    v = dict(table[(dim, 1, 1)]["cells"])
    v["aL"] = np.ones_like(v["aL"])
    _, iso, _ = ref.total_yield_vah_ref(v, sp, gla, dict(dimension=dim), y_cut=Y_CUT)
    d_aL = np.abs(on - iso) / np.abs(on)
    print("dim %d: shear on/off moves the yields by %s, alpha_L -> 1 by %s" % (dim, d_shear, d_aL))
    assert np.all(d_shear > 100.0 * BOUND) and np.all(d_aL > 100.0 * BOUND)
