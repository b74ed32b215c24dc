"""The primary lists the Monte Carlo decay tests share (tests/test_decays_mc.py on the CPU, tests/test_gpu_decays_mc.py on the device), the
measure of the distance between two decayed lists, and the bound the device is held to; and the hand-made decay tables (hand_table and what is
built with it below) of those tests and of tests/test_decays_physics.py and tests/test_gpu_decays_physics.py.

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


def hand_table(entries):
    """entries: [(mc_id, mass, width, stable, [(npart, branch_ratio, [daughter ids])])] -> pdg_read_decays' dict"""
    ch = [c for e in entries for c in e[4]]
    return dict(mc_id=np.array([e[0] for e in entries], np.int64), mass=np.array([e[1] for e in entries], np.float64),
                width=np.array([e[2] for e in entries], np.float64), stable=np.array([e[3] for e in entries], np.int32),
                n_channels=np.array([len(e[4]) for e in entries], np.int32), npart=np.array([c[0] for c in ch], np.int32),
                branch_ratio=np.array([c[1] for c in ch], np.float64),
                daughters=np.array([list(c[2]) + [0] * (5 - len(c[2])) for c in ch], np.int64).reshape(-1, 5))


def stable(mc_id, mass):
    return (mc_id, mass, 0.0, 1, [(1, 1.0, [mc_id])])


# ---- the phase-space tables of tests/test_decays_physics.py and tests/test_gpu_decays_physics.py: one parent (id 900, the last entry), one
# channel of ratio 1, every product stable and an entry of its own (ids 1 .. n, entries 0 .. n - 1), so the species names the product ----
_P5 = (0.14, 0.135, 0.49, 0.55, 0.14)
PHASE_SPACE = {"P3": (0.78265, (0.13957, 0.13957, 0.13498)),
               "P4": (1.6, (0.14, 0.49, 0.94, 0.0)),                 # a massless product: pstar with c = 0
               "P5": (2.0, _P5),
               "P5t": (float(np.sum(_P5)) + 0.02, _P5)}                # non-relativistic: 20 MeV above threshold
PARENT_ID = 900


def phase_space_table(name):
    M, m = PHASE_SPACE[name]
    ids = list(range(1, len(m) + 1))
    return hand_table([stable(i, mk) for i, mk in zip(ids, m)] + [(PARENT_ID, M, 0.1, 0, [(len(m), 1.0, ids)])])


# X(1.5, width 0.1) -> R(0.77, width 0.15) pi0, R -> pi+ pi-: a second-generation vertex
CHAIN = hand_table([stable(211, 0.13957), stable(-211, 0.13957), stable(111, 0.13498),
                    (9113, 0.77, 0.15, 0, [(2, 1.0, [211, -211])]), (9900, 1.5, 0.1, 0, [(2, 1.0, [9113, 111])])])

# ---- the tables both decay paths read (feed-down against Monte Carlo): every channel open, ratios summing to 1, no 4-body channel, no massless
# product; `chosen` lists the daughters first and the parent last, as the feed-down's schedule needs it ----
_PIONS = [stable(211, 0.13957), stable(-211, 0.13957), stable(111, 0.13498)]
FEED = {"F2": (hand_table(_PIONS + [stable(321, 0.49368), (313, 0.8961, 0.0474, 0, [(2, 1.0, [321, -211])])]), [321, -211, 313]),
        "F3": (hand_table(_PIONS + [(223, 0.78265, 0.00849, 0, [(3, 1.0, [211, -211, 111])])]), [211, -211, 111, 223]),
        "F3m": (hand_table(_PIONS + [(9001, 1.0, 0.1, 0, [(3, 1.0, [211, 211, -211])])]), [211, -211, 9001]),      # a group of multiplicity 2
        "Fbr": (hand_table(_PIONS + [(9002, 0.9, 0.1, 0, [(2, 0.6, [211, -211]), (3, 0.4, [211, -211, 111])])]), [211, -211, 111, 9002])}


def expected_yields(table, chosen, defect=None):
    """per daughter of chosen[:-1]: sum over the parent's channels of mult x BR; defect(M, m1, m2, m3), if given, is added as a relative
    correction to every 3-body group (the feed-down's 12-point s rule against its own normalisation)"""
    ids = [int(i) for i in table["mc_id"]]
    e = ids.index(int(chosen[-1]))
    first = int(np.sum(table["n_channels"][:e]))
    mass = lambda i: float(table["mass"][ids.index(int(i))])  # noqa: E731
    out = {int(c): 0.0 for c in chosen[:-1]}
    for c in range(first, first + int(table["n_channels"][e])):
        n = abs(int(table["npart"][c]))
        prod = [int(d) for d in table["daughters"][c][:n]]
        for d in out:
            if d in prod:
                rest = list(prod)
                rest.remove(d)
                corr = defect(mass(chosen[-1]), mass(d), mass(rest[0]), mass(rest[1])) if (defect and n == 3) else 0.0
                out[d] += prod.count(d) * float(table["branch_ratio"][c]) * (1.0 + corr)
    return out
