"""GPU (-m gpu): the spin polarization (mode 5, cf_polzn.hip) on the extreme cells of tests/extreme_cells.py, per bin, against the numpy
long-double restatement computed at test time (tests/test_extreme_polarization.py: surfaces, species, temperatures, metric).  cf_polzn
factorises z = E1_k E2_j in a way of its own, with its own proof that neither factor overflows; before this file it had been judged against
the largest value of each array, on flow up to u = 8 and one temperature near 0.15.  Here: gamma to 20, |eta| to 7, tau = 0.05 / 50, the
skipped and flying cells of isothermal-mix, pT to 40 GeV, T = 0.101 / 0.151 / 0.199, a fermion / boson pair of equal mass and a Boltzmann copy.

Every bin of St, Sx, Sy, Sn within TOL = 2e-9 of the reference against max(|ref|, 1e-4 sum |summands|, 1e-280), Snorm against
max(|ref|, 1e-280): the exponent is that of the spectrum kernels (50 roundings x 1e4 x 2^-53, tests/test_gpu_extreme_cells.py).  One shard is
bitwise the single call; three shards on one device are held to the same bound.

Worst errors on an MI355X over the five outputs, the single call and three shards (also DESIGN.md, section 2, "Extreme cells"): 3+1D 2.4e-10,
2+1D 6.3e-11, both on isothermal-mix at T = 0.101.  No case needed a conditioning factor and no defect was found.

Sensitivity, once, on a scratch build: with the bound of cf_polzn's factorisation, u_perp in E2 = exp(pT (B - u_perp) / T) and
E1 = exp((pT u_perp - mT A) / T), replaced by 0.75 u_perp in both (z = E1 E2 is the same number; E2 <= 1 no longer holds), all six fast-flow
cases and four of the six isothermal-mix cases fail -- E2 overflows at gamma = 20 and St .. Snorm are not finite -- while
tests/test_gpu_polarization.py and tests/test_gpu_polarization_multi.py pass (115 tests): with u <= 8 and pT <= 3 GeV, e^40 is still a double."""
import numpy as np
import pytest

import extreme_cells as X
from is3d_amd import api
from test_extreme_polarization import CASES, IDS, errors, species, vorticity
from test_gpu_polarization import OUTS

pytestmark = pytest.mark.gpu

TOL = 2e-9            # tests/test_gpu_extreme_cells.py


@pytest.mark.parametrize("case,dim,T", CASES, ids=IDS)
def test_every_bin_against_long_double(case, dim, T):
    args = (X.surface(case, dim), vorticity(), species(), X.grid(), T, dict(dimension=dim))
    got = api.spin_polarization(*args)
    err = errors(got, case, dim, T)
    print("%s %d+1D T = %.3f: device against long double %s" % (case, dim, T, {k: "%.2e" % v for k, v in err.items()}))
    assert max(err.values()) < TOL, err
    one = api.spin_polarization_multi(*args, devices=[0])
    for k in OUTS:
        assert one[k].tobytes() == got[k].tobytes(), k
    three = api.spin_polarization_multi(*args, devices=[0] * 3)
    assert len(three["shard_stats"]) == 3
    err3 = errors(three, case, dim, T)
    print("%s %d+1D T = %.3f: three shards against long double %s" % (case, dim, T, {k: "%.2e" % v for k, v in err3.items()}))
    assert max(err3.values()) < TOL, err3
