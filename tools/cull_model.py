#!/usr/bin/env python3
"""tools/cull_model.py -- host model of the row-culling rules of cf_main_tile3e on one cell chunk of BASELINE config 3.

Not part of the product or of any test: a design tool.  For a chunk of the seeded config-3 surface it forms, per (lane, cell,
phi tile, y row), the exponent bound earg = pT Dmax - mT C'_k the kernel tests, an estimate of the chunk's final accumulators
acc[lane][j][k] (equilibrium integrand, u = 1/2), and counts the (wave, cell, tile, row) quadruples each rule keeps:

  A  the kernel's rule: one threshold per (lane, tile) from the minimum over the tile's JT x R accumulators
  B  one threshold per (lane, tile, row): minimum over the row's JT accumulators
  C  per (lane, j, k): a row is live if any of its JT terms can reach half an ulp of ITS accumulator (needs E2_j per lane)
  G  (--row-groups 2,3,2) one threshold per (lane, tile, group of consecutive rows): minimum over the group's accumulators -- the rule of the
     kernels since round 24 (cull_refresh, cf_kernels.hip).  The unit-level test of the kernel is held against the smallest group threshold; the
     model's "live units" are units with at least one live row, which is what the empty-mask exit of the kernel makes of them.
  P  (--pds-bound unit|group|row) rule G (rule A without --row-groups) with lambda added to the tested exponent: earg + lambda >= thr, where
     lambda = clamp(log((mTmax max_k |A_k| + pTmax max_j |B_j|) psc), -LAMBDA_MAX, 0) is the bound of the scaled p.dsigma over the unit's rows and
     phi (unit: what cf_prep writes into header slot 11, the kernels' rule since round 25), over a row group's rows, or over one row.

--pad none|legacy|copy: what the slots that pad the lanes to whole waves do.  none: they never vote (the tool's rule until round 26, and what the
plans' copies of the last lane amount to: copy gives the same counts); legacy: 32 slots mT = 1, pT = 0, pe = 0 with accumulators, thresholds and votes
of their own, which is what the plans uploaded until round 26 (+3.1 % live wave-rows on the config-3 chunks, LABBOOK round 26).

--seed / --chunks: another seeded surface, cut into equal consecutive cell chunks with accumulators of their own (the counts are summed) -- e.g. the
surface tests/test_gpu_parity.py::test_row_culling_changes_no_bit pins its cross-variant counts on: --cells 2000 --seed 80 --chunks 3.

Thresholds use the final accumulators of the chunk (the best any stale running minimum can do), so the live fractions are
lower bounds; rule A's number is compared with what the device reports (status.n_wave_rows_culled).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from is3d_amd import inputs, synth  # noqa: E402


def unit_list_model():
    """under zero_skip = 3 (static threshold floors) cf_cull_floor could also emit, per (chunk, phi tile, row block,
    workgroup), the list of units that are live for at least one of the workgroup's lane-waves, and the main kernel could stage only those.
    What that can return is bounded by the cycle accounting of the kernel as it is (profiles/r02_cycle_accounting.log, culling on): the phases
    that scale with the number of units that pass through LDS.  Pure arithmetic on the committed counters -- build only if >= 6 % of the wave cycles."""
    import re
    log = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r02_cycle_accounting.log")).readline()
    f = {}
    for k, v in re.findall(r"(record part of stage|vmcnt part of wait|stage|wait|dead units|live units) (\d\.\d+)", log):
        f.setdefault(k, float(v))
    dead_n, live_n = [int(x) for x in re.findall(r"(?:dead|live) units (\d+) \(", log)]
    dead_frac = dead_n / (dead_n + live_n)
    # a unit can be left out of a workgroup's stream only if it is dead for BOTH of its lane-waves; neighbouring lane-waves (m_T-sorted) agree on
    # most units -- take the per-wave dead fraction as the upper bound
    save_dead = f["dead units"]                       # the dead units' own test: two LDS reads, three instructions, a vote
    save_stage = f["stage"] * dead_frac               # staging scales with the units staged
    # what the indirection costs: the records are 928 B, the staging pieces 1 KiB -- a gathered unit costs one whole piece for its record (today
    # 0.906 pieces per unit on average) and an address per unit instead of per four pieces; the E2 table (2 KiB per unit) is piece-aligned
    cost_gather = f["record part of stage"] * (1.0 - dead_frac) * (1.0 / 0.906 - 1.0) + f["stage"] * (1.0 - dead_frac) * 0.25
    net = save_dead + save_stage - cost_gather
    print("unit-list model (zero_skip = 3 only): staged units %.0f M, dead on arrival %.1f %%" % ((dead_n + live_n) / 1e6, 100 * dead_frac))
    print("  upper bound of what is saved: dead-unit tests %.2f %% + staging of dead units %.2f %% of the wave cycles = %.2f %%" % (
        100 * save_dead, 100 * save_stage, 100 * (save_dead + save_stage)))
    print("  gathered staging costs back ~%.2f %% (whole pieces per record, one address per unit)" % (100 * cost_gather))
    print("  net <= %.2f %% of the wave cycles; the barrier wait (%.1f %%) is the two waves' imbalance, not a per-unit cost" % (100 * net, 100 * f["wait"]))
    print("  threshold for building it: 6 %% -> %s" % ("build" if net >= 0.06 else "not built"))


def main():
    if "--unit-list-model" in sys.argv:
        unit_list_model()
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4525)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--JT", type=int, default=8)
    ap.add_argument("--R", type=int, default=7)
    ap.add_argument("--order", default="mT", choices=["mT", "pT", "pTpad", "band8", "band4", "band16"],
                    help="lane order: sorted by mT (the plan's), pT-major with the classes sorted by mass inside, or pT-major with "
                         "every pT padded to whole waves")
    ap.add_argument("--eta-bin", type=float, default=None,
                    help="eta-binned chunk (VERDICT round 2, item 5): take only cells with |eta - ETA_BIN| < half the y spacing, i.e. what a chunk "
                         "would hold if cf_prep binned the cells by eta")
    ap.add_argument("--origin", default="0", help="row-block origin: an integer row, or 'eta': the row nearest the bin's eta minus R // 2, so that the "
                                                  "live window of the chunk's cells sits in one block (blocks then cover rows origin + R m, clipped to the grid)")
    ap.add_argument("--row-groups", default=None, help="rule G: sizes of the groups of consecutive rows of a row block that share a threshold, e.g. 2,3,2")
    ap.add_argument("--pds-bound", default="none", choices=["none", "unit", "group", "row"],
                    help="rule P: the bound of the scaled p.dsigma over the unit / the row group / the row, in place of the surface-wide 2^pe alone")
    ap.add_argument("--seed", type=int, default=None, help="seed of the surface (default: the config-3 seed)")
    ap.add_argument("--pad", default="none", choices=["none", "legacy", "copy"],
                    help="the slots that pad the lanes to whole waves: never vote (none); the lane table's own padding mT = 1, pT = 0 with pe = 0, with "
                         "accumulators, thresholds and votes of its own (legacy: what the plans uploaded before round 26); copies of the last lane "
                         "(copy: what they upload now -- the votes of 'none')")
    ap.add_argument("--chunks", type=int, default=1, help="cut the cells into this many equal consecutive chunks, each with its own accumulators")
    a = ap.parse_args()
    groups = [int(x) for x in a.row_groups.split(",")] if a.row_groups else None
    if groups and sum(groups) != a.R:
        ap.error("--row-groups must add up to R")
    g = inputs.grid()
    sp = inputs.species("urqmd")
    pT, phi, yv = g["pT"], g["phi"], g["y"]
    cls = sorted(set(zip(sp["mass"].tolist(), sp["sign"].tolist())))
    mass = np.array([c[0] for c in cls])
    mT = np.sqrt(mass[:, None] ** 2 + pT[None, :] ** 2).ravel()
    pTl = np.broadcast_to(pT[None, :], (len(cls), len(pT))).ravel()
    if a.order == "mT":
        order = np.argsort(mT, kind="stable")
    elif a.order.startswith("band"):
        bw = int(a.order[4:])          # bands of bw adjacent pT values, lanes sorted by mT inside a band
        ipT = np.broadcast_to(np.arange(len(pT))[None, :], (len(cls), len(pT))).ravel()
        order = np.lexsort((mT, ipT // bw))
    else:
        order = np.lexsort((mT, pTl))      # pT-major, then mass
    mT, pTl = mT[order], pTl[order]
    if a.order == "pTpad":
        ncl = len(cls)
        npad = (ncl + 63) // 64 * 64
        m2 = np.zeros((len(pT), npad)); p2 = np.zeros((len(pT), npad))
        m2[:, :ncl] = mT.reshape(len(pT), ncl); p2[:, :ncl] = pTl.reshape(len(pT), ncl)
        m2[:, ncl:] = m2[:, ncl - 1:ncl]; p2[:, ncl:] = p2[:, ncl - 1:ncl]      # duplicates of the heaviest class: never change a vote
        mT, pTl = m2.ravel(), p2.ravel()
    mTmax, pTmax = mT.max(), pTl.max()           # over the real lanes, as in the plan
    pe = np.ceil(np.log2(np.maximum(mT / mTmax, pTl / pTmax))).astype(int)
    pe = np.minimum(pe, 0)
    npad = -len(mT) % 64
    if a.pad != "none" and npad:
        legacy = a.pad == "legacy"
        mT = np.concatenate([mT, np.full(npad, 1.0 if legacy else mT[-1])])
        pTl = np.concatenate([pTl, np.full(npad, 0.0 if legacy else pTl[-1])])
        pe = np.concatenate([pe, np.full(npad, 0 if legacy else pe[-1], dtype=int)])
    L = len(mT)
    nw = (L + 63) // 64

    if a.eta_bin is None:
        s = synth.synth_surface(a.cells, 3, seed=a.seed, first_cell=a.first)
    else:
        hw = 0.5 * (yv[1] - yv[0])
        big = synth.synth_surface(a.cells * 24, 3, seed=a.seed, first_cell=a.first)
        sel = np.nonzero(np.abs(big["eta"] - a.eta_bin) < hw)[0][:a.cells]
        s = {k: v[sel] for k, v in big.items()}
        a.cells = len(sel)
    tau, eta, T = s["tau"], s["eta"], s["T"]
    ut = np.sqrt(1 + s["ux"] ** 2 + s["uy"] ** 2 + tau ** 2 * s["un"] ** 2)
    dy = yv[None, :] - eta[:, None]                       # [c][k]
    ch, sh = np.cosh(dy), np.sinh(dy)
    Cp = (ch * ut[:, None] - sh * (tau * s["un"])[:, None]) / T[:, None]
    Ak = ch * s["dat"][:, None] + sh * (s["dan"] / tau)[:, None]
    Dp = (np.cos(phi)[None, :] * s["ux"][:, None] + np.sin(phi)[None, :] * s["uy"][:, None]) / T[:, None]   # [c][j]
    Bj = np.cos(phi)[None, :] * s["dax"][:, None] + np.sin(phi)[None, :] * s["day"][:, None]
    kmin, kmax = yv.min(), yv.max()
    gmax = np.cosh(np.maximum(np.abs(kmin - eta), np.abs(kmax - eta)))
    bound = ((mTmax * (np.abs(s["dat"]) + np.abs(s["dan"] / tau)) + pTmax * (np.abs(s["dax"]) + np.abs(s["day"]))) * gmax).max()
    e_sc = int(np.frexp(bound)[1])
    psc = 2.0 ** -e_sc
    J, K, JT, R = len(phi), len(yv), a.JT, a.R
    if a.origin == "eta":
        center = int(round(((a.eta_bin if a.eta_bin is not None else 0.0) - yv[0]) / (yv[1] - yv[0])))
        origin = (center - R // 2) % R
        origin = origin - R if origin > 0 else origin          # first block starts at or before row 0
    else:
        origin = -(int(a.origin) % R) if int(a.origin) % R else 0
    blocks = [(max(o, 0), min(o + R, K)) for o in range(origin, K, R) if min(o + R, K) > max(o, 0)]
    jt_n, kt_n = (J + JT - 1) // JT, len(blocks)
    C = a.cells

    if a.pds_bound == "group" and not groups:
        ap.error("--pds-bound group needs --row-groups")
    rules = ("ABCG" if groups else "ABC") + ("P" if a.pds_bound != "none" else "")
    LAMBDA_MAX = 40 * 0.6931471805599453          # kPdsLambdaMax, cf_device.h
    lam_all = []
    live = {k: 0 for k in rules}
    unit_live = {k: 0 for k in rules}
    lane_live = {k: 0 for k in rules if k not in "CP"}
    per_kt = {k: np.zeros(kt_n) for k in rules if k not in "CP"}
    total_rows = 0
    for ich in range(a.chunks):
        lo, hi = C * ich // a.chunks, C * (ich + 1) // a.chunks
        Cc = hi - lo
        # accumulators acc[l][j][k] (equilibrium, u = 1/2) and the exponent bounds
        acc = np.zeros((L, J, K))
        cb = 64
        for c0 in range(lo, hi, cb):
            c1 = min(hi, c0 + cb)
            x = mT[:, None, None, None] * Cp[None, c0:c1, None, :] - pTl[:, None, None, None] * Dp[None, c0:c1, :, None]   # [l][c][j][k]
            pds = np.maximum(mT[:, None, None, None] * Ak[None, c0:c1, None, :] + pTl[:, None, None, None] * Bj[None, c0:c1, :, None], 0.0) * psc
            acc += (pds * np.exp(-x)).sum(axis=1) * 0.5
        with np.errstate(divide="ignore"):
            e_acc = np.where(acc > 1e-290, np.floor(np.log2(np.maximum(acc, 1e-300))) + 1, -np.inf)    # frexp exponent
        ln2 = 0.6931471805599453

        def thr_from(e):   # e: frexp exponent(s) of a lower bound on the accumulators a row adds to
            return np.maximum(-745.2, (e - 58 - pe.reshape((-1,) + (1,) * (e.ndim - 1))) * ln2)

        for jt in range(jt_n):
            js = slice(jt * JT, min(J, (jt + 1) * JT))
            Dmax = Dp[lo:hi, js].max(axis=1)                                   # [c]
            for kt in range(kt_n):
                ks = slice(blocks[kt][0], blocks[kt][1])
                earg = pTl[:, None, None] * Dmax[None, :, None] - mT[:, None, None] * Cp[None, lo:hi, ks]     # [l][c][r]
                eA = e_acc[:, js, ks].min(axis=(1, 2))                        # [l]
                eB = e_acc[:, js, ks].min(axis=1)                             # [l][r]
                thrA = thr_from(eA)[:, None, None]
                thrB = thr_from(eB)[:, None, :]
                lvA = earg >= thrA
                lvB = earg >= thrB
                if groups:   # G: the rows of the block in consecutive groups, a threshold each (a clipped block keeps the groups' positions)
                    eG = np.empty_like(eB)
                    r0 = 0
                    for gs in groups:
                        if r0 < eB.shape[1]:
                            eG[:, r0:r0 + gs] = eB[:, r0:r0 + gs].min(axis=1, keepdims=True)
                        r0 += gs
                    lvG = earg >= thr_from(eG)[:, None, :]
                if a.pds_bound != "none":
                    absA = np.abs(Ak[lo:hi, ks])                               # [c][r]
                    bB = np.abs(Bj[lo:hi, js]).max(axis=1)                    # [c]
                    if a.pds_bound == "unit":
                        aA = np.broadcast_to(absA.max(axis=1, keepdims=True), absA.shape)
                    elif a.pds_bound == "row":
                        aA = absA
                    else:
                        aA = np.empty_like(absA)
                        r0 = 0
                        for gs in groups:
                            if r0 < absA.shape[1]:
                                aA[:, r0:r0 + gs] = absA[:, r0:r0 + gs].max(axis=1, keepdims=True)
                            r0 += gs
                    with np.errstate(divide="ignore"):
                        lam = np.clip(np.log((mTmax * aA + pTmax * bB[:, None]) * psc), -LAMBDA_MAX, 0.0)      # [c][r]
                    lam_all.append(lam[:, 0] if a.pds_bound == "unit" else lam.ravel())
                    thrP = thr_from(eG)[:, None, :] if groups else thrA
                    # a lane adds lambda only while all its group thresholds are relative bounds (no group at the floor: a padded row, a zero accumulator)
                    lamk = (np.isfinite(eG).all(axis=1) if groups else np.isfinite(eA)).astype(float)            # [l]
                    lvP = (earg + lamk[:, None, None] * lam[None, :, :]) >= thrP
                # C: exists j: earg + log E2_j >= thr(acc[j][k]);  log E2_j = pT (Dp_j - Dmax)
                lvC = np.zeros_like(lvA)
                for j in range(js.start, js.stop):
                    thrC = thr_from(e_acc[:, j, ks])[:, None, :]
                    lE2 = pTl[:, None] * (Dp[None, lo:hi, j] - Dmax[None, :])
                    lvC |= (earg + lE2[:, :, None]) >= thrC
                nr = ks.stop - ks.start
                total_rows += nw * Cc * nr
                for key, lv in (("A", lvA), ("B", lvB), ("C", lvC)) + ((("G", lvG),) if groups else ()) + ((("P", lvP),) if a.pds_bound != "none" else ()):
                    pad = np.zeros((nw * 64 - L,) + lv.shape[1:], dtype=bool)
                    w = np.concatenate([lv, pad]).reshape(nw, 64, Cc, nr).any(axis=1)    # [w][c][r]
                    live[key] += int(w.sum())
                    unit_live[key] += int(w.any(axis=2).sum())
                    if key in per_kt:
                        per_kt[key][kt] += w.sum() * R / nr
                        lane_live[key] += int(lv.sum())
    units = nw * C * jt_n * kt_n
    print("cells %d in %d chunk(s)  lanes %d (%d waves)  tiles %d x %d  row blocks %s  scale 2^-%d" % (C, a.chunks, L, nw, jt_n, kt_n, blocks, e_sc))
    for key in rules:
        print("rule %s: live wave-rows %.4f  live units %.4f  rows per live unit %.2f" % (
            key, live[key] / total_rows, unit_live[key] / units, live[key] / max(unit_live[key], 1)))
    # issued fp64-VALU instructions per (wave, cell, phi tile) under rule A, priced with the instruction counts of cf_main_tile3e (DESIGN.md
    # section 5): a live row 8 x 14 + 25 (operands, row exponential), a live unit's header 59 (24 multiplications, 21 row-test instructions,
    # 14 v_readfirstlane), a dead row inside a live unit 3, a unit culled whole 3
    lr, lu = live["A"], unit_live["A"]
    dead_rows_in_live_units = lu * R - lr
    instr = lr * (8 * 14 + 25) + lu * 59 + max(dead_rows_in_live_units, 0) * 3 + (units - lu) * 3
    print("rule A: modelled issued instructions per (wave, cell, phi tile): %.1f   (units per cell and tile: %d)" % (instr / (nw * C * jt_n), kt_n))
    if groups:
        ca, cg = 1.0 - live["A"] / total_rows, 1.0 - live["G"] / total_rows
        print("rule G (row groups %s): culled wave-rows %.4f against A's %.4f: %+.2f %% relative" % (a.row_groups, cg, ca, 100.0 * (cg - ca) / ca))
    if a.pds_bound != "none":
        lam = np.concatenate(lam_all)
        base = "G" if groups else "A"
        print("rule P (lambda per %s): mean %.2f median %.2f min %.2f max %.2f;  live wave-rows %.4f against %s's %.4f: %+.2f %%;  live units %+.2f %%" % (
            a.pds_bound, lam.mean(), np.median(lam), lam.min(), lam.max(), live["P"] / total_rows, base, live[base] / total_rows,
            100.0 * (live["P"] - live[base]) / live[base], 100.0 * (unit_live["P"] - unit_live[base]) / unit_live[base]))
    for key in per_kt:
        print("rule %s: live (lane, row) pairs %.4f;  live wave-rows by row block: %s" % (
            key, lane_live[key] / (L * C * jt_n * K), np.round(per_kt[key] / (nw * C * jt_n * R), 4)))


if __name__ == "__main__":
    main()
