"""The primary lists the Monte Carlo decay tests share (tests/test_decays_mc.py on the CPU, tests/test_gpu_decays_mc.py on the device), the
measure of the distance between two decayed lists, and the bound the device is held to.

FLOOR is the largest distance between the float64 and the longdouble run of the restatement (tests/decays_mc_ref.py) over every list below,
with lifetime = 0 and 1: tests/test_decays_mc.py::test_rounding_floor measures it again and holds it to this figure.  BOUND = 64 x FLOOR
covers the device's sin / cos / log1p / atanh and fused multiply-adds against libm; it also serves the conservation and mass-shell checks."""
import os

import numpy as np

import decays_mc_ref as ref

FLOOR = 2.4e-14     # measured 2.32e-14 (the rho0 at 20 GeV: gamma^2 x 2^-53); the other lists stay below 1e-15
BOUND = 64 * FLOOR  # 1.536e-12
SEED = 20231
LENGTHS = (1, 63, 65, 257)     # off the wave (64) and workgroup (128) sizes


def tables(api, reference):
    return {name: api.pdg_read_decays(os.path.join(reference, "PDG", name)) for name in ("pdg-urqmd_v3.3+.dat", "pdg_smash.dat")}


def four_body_parent(table, prep):
    """the first entry of the table with an open 4-body channel"""
    for e, chs in enumerate(prep["open"]):
        if any(n == 4 for _, n, _ in chs):
            return e
    raise AssertionError("no open 4-body channel")


def hand_list(api, table, prep):
    """257 primaries of the urqmd table, the chosen list being the table itself: rho0 -> pi pi, eta -> gamma gamma (and its other channels),
    omega -> pi0 gamma | 3 pi, a parent with a 4-body channel, stable pions; [0] is a rho0 at rest and [1] one at |p| = 20 GeV"""
    idx = prep["index"]
    kinds = [idx[113], idx[221], idx[223], four_body_parent(table, prep), idx[223], idx[211], idx[113]]
    rng = np.random.default_rng(7)
    species = [idx[113], idx[113]] + [kinds[i % len(kinds)] for i in range(255)]
    p3 = rng.normal(size=(257, 3)) * 0.7
    p3[0] = 0.0
    p3[1] = (12.0, -9.0, 13.2)
    return ref.make_particles(api, table, table["mc_id"], species, p3, events=np.arange(257) // 40)


def every_unstable(api, table, seed):
    """one primary of every unstable entry of the table"""
    species = [e for e in range(len(table["mc_id"])) if not table["stable"][e]]
    p3 = np.random.default_rng(seed).normal(size=(len(species), 3)) * 0.8
    return ref.make_particles(api, table, table["mc_id"], species, p3, events=np.arange(len(species)) // 50)


def distance(a_mom, a_pos, b_mom, b_pos, origin, primaries):
    """max over the final particles of |dE, dp| / E_primary, |d(t, x, y, z, tau)| / t of the particle and |d eta|, in longdouble"""
    L = np.longdouble
    E0 = primaries["E"][origin].astype(L)[:, None]
    dm = np.abs(a_mom.astype(L) - b_mom.astype(L)) / E0
    t = np.abs(b_pos[:, 0].astype(L))[:, None]
    dp = np.abs(a_pos.astype(L) - b_pos.astype(L))
    dp[:, :5] = dp[:, :5] / t
    return float(max(dm.max(initial=0.0), dp.max(initial=0.0)))


def device_arrays(out):
    """the [N, 4] momenta and [N, 6] positions of a PARTICLE_DTYPE list, in the restatement's column order"""
    return np.stack([out[k] for k in ref.MOM], axis=1), np.stack([out[k] for k in ref.POS], axis=1)
