// cf_plan_geometry.h -- what a plan decides on the host before it touches the device: species classes, the lane table, the lane split, the
// workgroup size, the chunk count and the kernel variant.  Pure functions on plain structs, no HIP: tests/cpp/plan_geometry_main.cpp runs
// them on the CPU against tables recorded from the statements they replaced (tests/golden/plan_*.json).  These decide bits, not only text:
// the lane order and the chunk count fix the summation order of a spectrum.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace is3d {

// ---- species classes: identical (mass, sign[, baryon number]) => identical integrand up to the degeneracy ----
struct SpeciesClasses {
    std::vector<int32_t> cls;                 // [n] species -> class
    std::vector<double> cmass, csign, cbar;   // [classes]; cbar is 0 where no baryon numbers were given
};
// Classes are numbered in order of first appearance; two species share a class exactly when their keys compare equal with ==.
// collapse = false: one class per species.
inline SpeciesClasses species_classes(const double *mass, const double *sign, const double *baryon_or_null, int n, bool collapse)
{
    SpeciesClasses k;
    k.cls.resize(n > 0 ? n : 0);
    for (int s = 0; s < n; s++) {
        int found = -1;
        const double bs = baryon_or_null ? baryon_or_null[s] : 0.0;
        if (collapse)
            for (size_t c = 0; c < k.cmass.size(); c++)
                if (k.cmass[c] == mass[s] && k.csign[c] == sign[s] && k.cbar[c] == bs) { found = (int)c; break; }
        if (found < 0) { found = (int)k.cmass.size(); k.cmass.push_back(mass[s]); k.csign.push_back(sign[s]); k.cbar.push_back(bs); }
        k.cls[s] = found;
    }
    return k;
}

// ---- unit-strided lanes (the 2+1D 8 x 31 tile kernels): lane slots per momentum bin ----
// S in {1, 2, 4}: the smallest S whose slots fill whole two-wave workgroups better, by more than 0.05 of the lanes, than what was found before it
// (96 bins: 128 slots = 25 % idle lanes with S = 1, 384 = 6 full waves with S = 4).
// Invariant the kernels rely on: S divides rblocks, the units per cell of the stream (the eta table's row blocks), and S divides the 4 units of
// an LDS batch -- the sub-lanes of a bin then take whole, equal shares of every batch, and a wave's unit bound is uniform (cf_vah.hip reads it
// with readfirstlane).
inline int lane_split(int n_bins, int rblocks)
{
    int S_best = 1;
    double best = 1.0 - (double)n_bins / (double)(((n_bins + 63) / 64) * 64);
    for (int S : {2, 4}) {
        if (rblocks % S) continue;
        const int tot = n_bins * S, pad = ((tot + 127) / 128) * 128;   // whole 2-wave workgroups
        const double waste = 1.0 - (double)tot / (double)pad;
        if (waste < best - 0.05) { best = waste; S_best = S; }
    }
    return S_best;
}

// ---- lane table: the momentum bins (class x pT) sorted by mT, `split` slots per bin, padded to whole waves ----
// Sorted by mT a wave holds momenta of similar energy, which is what makes the exact-zero row culling of the main kernels wave-uniform more
// often (and keeps the exp arguments of a wave close together).
struct LaneTable {
    int Lbins = 0, L = 0, Lpad = 0;    // bins; slots in use (bins x split); slots padded to whole waves
    std::vector<int> order, slot_of;   // [Lbins] slot -> natural bin (class * n_pT + i) and back; E2 lane -> pT index is order % n_pT, lane -> class order / n_pT
    std::vector<double> mT, pT, sign, b;   // [Lpad]; padding lanes hold 1, 0, 1, 0 HERE, in the host table; what a plan uploads is lane_arrays()
    std::vector<int32_t> sub;              // [Lpad] sub-lane of the slot within its bin; padding 0
    std::vector<int> lane_of;              // [species x n_pT] -> slot of the class's bin
};
// order is the stable mT order (ties in natural order); slot (bin s, sub sl) is sl * Lbins + s, the order in which cf_finalize adds a bin's slots.
// interleave128 (developer A/B): the two waves of a workgroup take the even and the odd slots of each full 128-slot span of that order.
inline LaneTable lane_table(const SpeciesClasses &k, const double *pT, int n_pT, int split, bool interleave128)
{
    LaneTable t;
    const int ncls = (int)k.cmass.size(), npart = (int)k.cls.size();
    t.Lbins = ncls * n_pT;
    t.L = t.Lbins * split;
    t.Lpad = ((t.L + 63) / 64) * 64;
    t.mT.assign(t.Lpad, 1.0); t.pT.assign(t.Lpad, 0.0); t.sign.assign(t.Lpad, 1.0); t.b.assign(t.Lpad, 0.0);
    t.sub.assign(t.Lpad, 0);
    t.order.resize(t.Lbins); t.slot_of.resize(t.Lbins);
    std::vector<double> mT_nat(t.Lbins);
    for (int c = 0; c < ncls; c++)
        for (int i = 0; i < n_pT; i++) {
            const double m = k.cmass[c], p = pT[i];
            mT_nat[c * n_pT + i] = std::sqrt(m * m + p * p);
            t.order[c * n_pT + i] = c * n_pT + i;
        }
    std::stable_sort(t.order.begin(), t.order.end(), [&](int a, int b) { return mT_nat[a] < mT_nat[b]; });
    if (interleave128) {
        std::vector<int> o2(t.order);
        for (int b = 0; b + 128 <= t.Lbins; b += 128)
            for (int i = 0; i < 64; i++) { o2[b + i] = t.order[b + 2 * i]; o2[b + 64 + i] = t.order[b + 2 * i + 1]; }
        t.order.swap(o2);
    }
    for (int s = 0; s < t.Lbins; s++) {
        const int nat = t.order[s], c = nat / n_pT, i = nat % n_pT;
        t.slot_of[nat] = s;
        for (int sl = 0; sl < split; sl++) {
            const int l = sl * t.Lbins + s;
            t.mT[l] = mT_nat[nat];
            t.pT[l] = pT[i];
            t.sign[l] = k.csign[c];
            t.b[l] = k.cbar[c];
            t.sub[l] = sl;
        }
    }
    t.lane_of.resize((size_t)npart * n_pT);
    for (int s = 0; s < npart; s++)
        for (int i = 0; i < n_pT; i++) t.lane_of[(size_t)s * n_pT + i] = t.slot_of[k.cls[s] * n_pT + i];
    return t;
}

// ---- lane arrays: what a plan uploads of a lane table, one value per slot ----
// Slots [0, L) hold the table's values and what the plans derive from them.  A padding slot [L, Lpad) is a copy of slot L - 1 in every array: the
// heaviest bin of the last sub-lane, which always sits in the padding's own wave.  A copy reads the same operands, does the same arithmetic, holds the same
// accumulators and thresholds and casts the same vote as its source, so it never changes a wave-wide cull vote; the table's own padding (1, 0, 1, 0 with
// pe = 0: a light boson at rest) was alive in several times as many (unit, row) pairs as the real lanes of its wave and kept their rows running.  Every
// index a copy carries (sub, ipT, cls) is one a real lane carries, hence in range wherever slot L - 1 is.  Nothing reads a padding slot's sums: lane_of
// and the slots sl * Lbins + s that cf_finalize adds are all below L.
struct LaneArrays {
    int Lpad = 0;
    std::vector<double> mT, pT, sign, b, mass;   // [Lpad]; mass: of the slot's class (modified equilibrium)
    std::vector<int32_t> sub, ipT, pe, cls;      // [Lpad]; ipT: index of the slot's pT in the grid (E2 table column); cls: the slot's class;
                                                 // pe: max(mT/mTmax, |pT|/pTmax) < 2^pe, pe <= 0 (the lane's share of the p.dsigma bound, cf_pds_bound)
    double mTmax = 0.0, pTmax = 0.0;             // over the slots in use: max mT, max |pT|
};
inline LaneArrays lane_arrays(const LaneTable &t, const SpeciesClasses &k, int n_pT)
{
    LaneArrays a;
    a.Lpad = t.Lpad;
    a.mT = t.mT; a.pT = t.pT; a.sign = t.sign; a.b = t.b; a.sub = t.sub;
    a.mass.assign(t.Lpad, 1.0);
    a.ipT.assign(t.Lpad, 0); a.pe.assign(t.Lpad, 0); a.cls.assign(t.Lpad, 0);
    for (int s = 0; s < t.L; s++) { a.mTmax = std::max(a.mTmax, t.mT[s]); a.pTmax = std::max(a.pTmax, std::fabs(t.pT[s])); }
    for (int l = 0; l < t.L; l++) {
        const int nat = t.order[l % t.Lbins];   // every slot of a bin carries the bin's class and pT index
        a.cls[l] = nat / n_pT;
        a.ipT[l] = nat % n_pT;
        a.mass[l] = k.cmass[nat / n_pT];
        // scaled p.dsigma of a lane: mT |A| + pT |B W| <= max(mT/mTmax, pT/pTmax) (mTmax |A| + pTmax |B W|) <= that factor (cf_pds_bound)
        const double f = std::max(a.mTmax > 0.0 ? t.mT[l] / a.mTmax : 1.0, a.pTmax > 0.0 ? std::fabs(t.pT[l]) / a.pTmax : 0.0);
        int e = 0;
        (void)std::frexp(f * (1.0 + 1.0e-12), &e);     // f (1 + eps) = m 2^e, m in [0.5, 1): f < 2^e with room for the roundings
        a.pe[l] = std::min(e, 0);                      // the clamp keeps the scaled p.dsigma in [0, 1] whatever the lane
    }
    if (t.L > 0)
        for (int l = t.L; l < t.Lpad; l++) {
            const int c = t.L - 1;
            a.mT[l] = a.mT[c]; a.pT[l] = a.pT[c]; a.sign[l] = a.sign[c]; a.b[l] = a.b[c]; a.mass[l] = a.mass[c];
            a.sub[l] = a.sub[c]; a.ipT[l] = a.ipT[c]; a.pe[l] = a.pe[c]; a.cls[l] = a.cls[c];
        }
    return a;
}

// ---- waves per workgroup of a tile kernel ----
// All waves of a workgroup stream the same records; idle waves (lane-wave count not a multiple) still occupy their SIMD slots, so: the size
// of {8, 4, 2} that wastes fewest, the larger one on ties; an explicit request of 2, 4 or 8 wins.  One-wave workgroups are a property of single
// kernels and stay with the callers that own them.
inline int waves_per_group(int lane_waves, int requested)
{
    int wpb = 4, best_waste = 1 << 30;
    for (int w : {8, 4, 2}) {
        const int waste = ((lane_waves + w - 1) / w) * w - lane_waves;
        if (waste < best_waste) { best_waste = waste; wpb = w; }
    }
    if (requested == 2 || requested == 4 || requested == 8) wpb = requested;
    return wpb;
}

// ---- cell chunks of one pass ----
// Two floors: enough wave tasks for `rounds` rounds of the chip (4096 wave slots: 256 CUs x 4 SIMDs x ~4 waves; load balance -- lane-wave
// groups cull differently), and chunks of at most ~1152 cells (the streams of one (phi tile, chunk) pair then stay about the size of an XCD's
// 4 MB L2; profiles/r03_chunks.log).  Two caps: chunks of at least 64 cells, and partial slabs of at most 12 GiB -- 32 GiB when the caller asked
// for cell_chunks explicitly, which replaces the floors.  Never less than 1.
inline int chunk_count(int64_t rounds, int64_t tasks_per_chunk, int64_t pass_cells, int64_t cell_chunks, int64_t partial_bytes_per_chunk)
{
    const int64_t capacity = 256LL * 4 * 4;
    int64_t nch = cell_chunks > 0 ? cell_chunks : std::max<int64_t>((rounds * capacity + tasks_per_chunk - 1) / tasks_per_chunk, (pass_cells + 1151) / 1152);
    nch = std::min(nch, std::max<int64_t>(1, pass_cells / 64));
    const int64_t by_mem = ((int64_t)(cell_chunks > 0 ? 32 : 12) << 30) / partial_bytes_per_chunk;
    return (int)std::max<int64_t>(1, std::min(nch, by_mem));
}

// ---- kernel variant of the delta-f / modified-equilibrium plan ----
struct VariantChoice {
    int variant;
    bool e2tab;   // the kernel reads the E2 table stream (3+1D delta-f, pT grid within kE2Stride)
};
// The shipped library holds the kernels the defaults reach; the developer build (make DEV=1) also the A/B forms of rounds 1-5.  A request the
// build does not honour runs the default -- status.kernel_variant says which one ran.  (A/B figures: DESIGN.md section 4.)
//   3+1D delta-f        default 6 (8 x 7 tile, E2 table stream) when the pT grid fits the stream, else 3 (8 x 7), or 2 (6 x 7) with baryon slots.
//                       shipped: 3 without baryon slots.   developer: 1-4; 5, 6 when the grid fits; 9-13 when it fits and there are no baryon slots.
//   3+1D mod. equil.    default 3 (8 x 7).   shipped: none.   developer: 1-4; 5, 6 (row walks of the same tile) without baryon slots.
//   2+1D delta-f        default 7 (8 x 31, unit-strided lanes).   shipped: none.   developer: 1-4, 7; 8 without baryon slots (7 with); 5, 6 run 2.
//   2+1D mod. equil.    default 7.   shipped: none.   developer: 2-4 (the 61-row tiles).
inline VariantChoice choose_variant(int dimension, bool feqmod, bool include_baryon, bool pT_fits_e2, int requested, bool dev_build)
{
    const int r = requested;
    if (dimension == 3 && !feqmod) {
        const int def = pT_fits_e2 ? 6 : (include_baryon ? 2 : 3);
        int v = def;
        if (dev_build) {
            if (r >= 1 && r <= 4) v = r;
            else if (r == 5 || r == 6) v = pT_fits_e2 ? r : def;
            else if (r >= 9 && r <= 13) v = (pT_fits_e2 && !include_baryon) ? r : def;
        } else if (r == 3 && !include_baryon)
            v = 3;
        return {v, v == 5 || v == 6 || v >= 9};   // these survive only where the grid fits
    }
    if (dimension == 3) {
        int v = 3;
        if (dev_build && r >= 1 && r <= 4) v = r;
        if (dev_build && (r == 5 || r == 6) && !include_baryon) v = r;
        return {v, false};
    }
    if (feqmod) return {(dev_build && r >= 2 && r <= 4) ? r : 7, false};
    int v = 7;
    if (dev_build) {
        if ((r >= 1 && r <= 4) || r == 7) v = r;
        else if (r == 5 || r == 6) v = 2;
        else if (r == 8) v = include_baryon ? 7 : 8;
    }
    return {v, false};
}

}  // namespace is3d
