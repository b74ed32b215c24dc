"""A scalar numpy restatement of the Monte Carlo decay rule of include/is3d_amd.h (is3d_decay_particles), for the tests: the table analysis
(open channels and their running sums, closed channels, cycle, pending-stack need, depth) and the walk of one primary's decay tree, which
consumes the uniforms of Philox stream 5 in the order the header gives.  `dtype` is the type every momentum and position is computed in:
numpy.float64 (what the device computes in) or numpy.longdouble (the yardstick of the rounding floor).  The uniforms, the table's masses,
widths and running sums, hbarc and 2 pi are the same float64 values in both."""
import math

import numpy as np

HBARC = 0.197327053
MAX_BODIES, MAX_STACK, MAX_TRIALS = 5, 16, 4096
POS = ["t", "x", "y", "z", "tau", "eta"]
MOM = ["E", "px", "py", "pz"]


class TableError(ValueError):
    pass


def prepare(table):
    """dict(index, mass, width, stable, open[e] = [(running sum, n, [daughter entries])], n_closed, max_stack, max_depth); TableError for what
    is3d_decay_particles refuses with IS3D_EINVAL"""
    ids = [int(i) for i in table["mc_id"]]
    index = {}
    for e, i in enumerate(ids):
        index.setdefault(i, e)
    mass = np.asarray(table["mass"], np.float64)
    stable = [int(s) for s in table["stable"]]
    off = np.concatenate([[0], np.cumsum(table["n_channels"])]).astype(int)
    dau = np.asarray(table["daughters"], np.int64).reshape(-1, 5)
    chans, opened, n_closed = [], [], 0
    for e in range(len(ids)):
        chans.append([])
        opened.append([])
        if stable[e]:
            continue
        run = np.float64(0.0)
        for c in range(off[e], off[e + 1]):
            n = abs(int(table["npart"][c]))
            if n > MAX_BODIES or n < 2:
                raise TableError("parent %d: %d products" % (ids[e], n))
            ds = []
            for k in range(n):
                if int(dau[c, k]) == 0 or int(dau[c, k]) not in index:
                    raise TableError("parent %d: daughter %d is not in the table" % (ids[e], dau[c, k]))
                ds.append(index[int(dau[c, k])])
            chans[e].append(ds)
            s = np.float64(0.0)
            for d in ds:
                s = s + mass[d]
            if not s < mass[e]:
                n_closed += 1
                continue
            run = run + np.float64(table["branch_ratio"][c])
            opened[e].append((run, n, ds))
    final = [bool(stable[e]) or not opened[e] for e in range(len(ids))]
    need, depth, state = {}, {}, {}

    def visit(e):
        state[e] = 1
        nd, dp = 1, 0
        for ds in chans[e]:
            for i, d in enumerate(ds):
                if state.get(d) == 1:
                    raise TableError("cycle through %d and %d" % (ids[e], ids[d]))
                if d not in state:
                    visit(d)
                if not final[e]:
                    nd, dp = max(nd, need[d] + len(ds) - 1 - i), max(dp, depth[d] + 1)
        need[e], depth[e], state[e] = nd, dp, 2

    for e in range(len(ids)):
        if e not in state:
            visit(e)
    max_stack = max([1] + list(need.values()))
    if max_stack > MAX_STACK:
        raise TableError("pending stack of %d" % max_stack)
    return dict(index=index, mass=mass, width=np.asarray(table["width"], np.float64), stable=stable, open=opened, n_closed=n_closed,
                max_stack=max_stack, max_depth=max([0] + list(depth.values())))


class Stream:
    """the uniforms of Rng(seed, 5, lo32(g), hi32(g)) in order, fetched in growing blocks from rng_uniforms(seed, stream, cell, event, n)"""

    def __init__(self, rng_uniforms, seed, g):
        self.fetch = lambda n: rng_uniforms(int(seed), 5, int(g) & 0xFFFFFFFF, (int(g) >> 32) & 0xFFFFFFFF, n)
        self.buf, self.pos = self.fetch(64), 0

    def __call__(self):
        if self.pos >= len(self.buf):
            self.buf = self.fetch(8 * len(self.buf))
        self.pos += 1
        return self.buf[self.pos - 1]


def pstar(a, b, c, F):
    v = (a - b - c) * (a + b + c) * (a + b - c) * (a - b + c)
    return np.sqrt(max(v, F(0))) / (F(2) * a)


def boost(b, b2, gamma, e, q, F):
    if b2 > 0:
        bq = b[0] * q[0] + b[1] * q[1] + b[2] * q[2]
        f = (gamma - F(1)) * bq / b2 + gamma * e
        return [gamma * (e + bq), q[0] + f * b[0], q[1] + f * b[1], q[2] + f * b[2]]
    return [e, q[0], q[1], q[2]]


def decay_tree(prep, e, P, X, u, lifetime, F, stats):
    """the final particles [(entry, [E, px, py, pz], [t, x, y, z, tau, eta])] of one primary, in output order; u() is its stream"""
    out, stack = [], []
    cur = (e, [F(v) for v in P], [F(v) for v in X])
    while True:
        e, P, X = cur
        chs = prep["open"][e]
        if prep["stable"][e] or not chs:
            stats["n_stuck"] += 0 if prep["stable"][e] else 1
            out.append(cur)
            if not stack:
                return out
            cur = stack.pop()
            continue
        stats["n_decays"] += 1
        M = F(prep["mass"][e])
        uc = F(u()) * F(chs[-1][0])
        j = len(chs) - 1
        for k in range(len(chs) - 1):
            if uc < F(chs[k][0]):
                j = k
                break
        if lifetime:
            u_tau, width = F(u()), prep["width"][e]
            if width > 0.0:
                ts = -(F(HBARC) / F(width)) * np.log1p(-u_tau)
                X = [X[0] + (P[0] / M) * ts, X[1] + (P[1] / M) * ts, X[2] + (P[2] / M) * ts, X[3] + (P[3] / M) * ts, None, None]
                X[4] = np.sqrt(X[0] * X[0] - X[3] * X[3])
                X[5] = np.arctanh(X[3] / X[0])
        _, n, ds = chs[j]
        m = [F(prep["mass"][d]) for d in ds]
        S = [m[0]]
        for k in range(1, n):
            S.append(S[k - 1] + m[k])
        T = M - S[n - 1]
        wmax = F(1)
        for k in range(1, n):
            wmax = wmax * pstar(T + S[k], S[k - 1], m[k], F)
        trial = 0
        while True:
            trial += 1
            stats["n_trials"] += 1
            r = sorted(F(u()) for _ in range(n - 2))
            mu = [m[0]] + [S[k] + r[k - 1] * T for k in range(1, n - 1)] + [S[n - 1] + T]
            if n == 2:
                break
            w = F(1)
            for k in range(1, n):
                w = w * pstar(mu[k], mu[k - 1], m[k], F)
            if F(u()) * wmax < w:
                break
            if trial == MAX_TRIALS:
                stats["n_exhausted"] += 1
                break
        Pc = P
        for k in range(n - 1, 0, -1):
            u_cos, u_phi = F(u()), F(u())
            ct = F(2) * u_cos - F(1)
            st = np.sqrt(max(F(1) - ct * ct, F(0)))
            phi = F(2.0 * math.pi) * u_phi
            p = pstar(mu[k], mu[k - 1], m[k], F)
            d = [p * (st * np.cos(phi)), p * (st * np.sin(phi)), p * ct]
            b = [Pc[1] / Pc[0], Pc[2] / Pc[0], Pc[3] / Pc[0]]
            b2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2]
            gamma = F(1) / np.sqrt(F(1) - b2)
            stack.append((ds[k], boost(b, b2, gamma, np.sqrt(p * p + m[k] * m[k]), d, F), X))
            Pc = boost(b, b2, gamma, np.sqrt(p * p + mu[k - 1] * mu[k - 1]), [-d[0], -d[1], -d[2]], F)
        cur = (ds[0], Pc, X)


def decay_particles(table, chosen_mc_id, particles, rng_uniforms, seed=1, first_particle=0, lifetime=0, dtype=np.float64, prep=None):
    """-> dict(species, origin, cell, event (int arrays), mom [N, 4], pos [N, 6] in `dtype`, stats)"""
    prep = prep or prepare(table)
    F = dtype
    stats = dict(n_primaries=len(particles), n_decays=0, n_final=0, n_stuck=0, n_trials=0, n_exhausted=0, max_stack=prep["max_stack"],
                 max_depth=prep["max_depth"], n_closed_channels=prep["n_closed"])
    sp, org, cell, ev, mom, pos = [], [], [], [], [], []
    for i, q in enumerate(particles):
        e = prep["index"][int(chosen_mc_id[int(q["species"])])]
        u = Stream(rng_uniforms, seed, first_particle + i)
        for fe, P, X in decay_tree(prep, e, [q[k] for k in MOM], [q[k] for k in POS], u, lifetime, F, stats):
            sp.append(fe), org.append(i), cell.append(int(q["cell"])), ev.append(int(q["event"])), mom.append(P), pos.append(X)
    stats["n_final"] = len(sp)
    return dict(species=np.array(sp, np.int64), origin=np.array(org, np.int64), cell=np.array(cell, np.int64), event=np.array(ev, np.int64),
                mom=np.array(mom, dtype=F).reshape(-1, 4), pos=np.array(pos, dtype=F).reshape(-1, 6), stats=stats)


def make_particles(api, table, chosen_mc_id, species, p3, pos=(1.0, 0.3, -0.2, 0.4), cell0=100, events=None):
    """a hand-made primary list: species[i] (index into chosen_mc_id) with three-momentum p3[i] on its table mass shell, at (tau, x, y, eta)"""
    prep_index = {int(i): e for e, i in reversed(list(enumerate(table["mc_id"])))}
    n = len(species)
    q = np.zeros(n, dtype=api.PARTICLE_DTYPE)
    p3 = np.asarray(p3, np.float64).reshape(n, 3)
    m = np.array([table["mass"][prep_index[int(chosen_mc_id[s])]] for s in species])
    q["species"], q["cell"] = species, cell0 + np.arange(n)
    q["event"] = np.arange(n) // 7 if events is None else events
    q["px"], q["py"], q["pz"] = p3[:, 0], p3[:, 1], p3[:, 2]
    q["E"] = np.sqrt(m * m + (p3 * p3).sum(axis=1))
    q["tau"], q["x"], q["y"], q["eta"] = pos
    q["t"], q["z"] = q["tau"] * np.cosh(q["eta"]), q["tau"] * np.sinh(q["eta"])
    return q
