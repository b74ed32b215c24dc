// cf_sampler_hbt.h -- the rule of the HBT correlation functions (include/is3d_amd.h): which particle is accepted,
// and for an ordered pair of accepted records of one (event, slot) the bin (ikT, io, is, il) and the phase q . dx / hbarc.  Stated ONCE for
// the host (hbt_host.cpp: is3d_hbt_list) and the device (cf_sampler_hbt.hip, cf_decays_mc.hip).
//
// Everything that decides acceptance or a bin is +, -, *, / and sqrt on doubles, compiled with floating-point contraction OFF on both
// sides, products rounded one by one in the order written; the thresholds and bin widths are computed once on the host (hbt_derived) and
// handed to the kernels as bits.  So host and device reach the same bin from the same record bits: den and M are equal bit for bit.  cos
// feeds only the numerator's term, llrint(cos(phase) 2^32) (sampler_vn_fixed): one unit per pair is what the two libm may differ by.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/is3d_amd.h"
#include "cf_sampler_bins.h"
#if defined(__HIP__) || defined(__HIPCC__)
#include "cf_host.h"
#endif

namespace is3d {

constexpr int kHbtMaxKT = 16, kHbtMaxQ = 64;
constexpr double kHbtHbarC = 0.197327053;   // kHbarC of cf_device.h (src/cpp/iS3D.h:9), restated for the host-only translation units

// exp(-2 y_cut), exp(2 y_cut): the rapidity cut as bounds on (E + pz) / (E - pz) = e^{2y}; the kT and q bin widths
struct HbtDerived { double lo, hi, dkT, dq; };

inline HbtDerived hbt_derived(const is3d_hbt_bins &b)
{
    IS3D_BINS_NO_CONTRACT
    HbtDerived d;
    d.lo = exp(-2.0 * b.y_cut);
    d.hi = exp(2.0 * b.y_cut);
    d.dkT = (b.kT_max - b.kT_min) / (double)b.n_kT;
    d.dq = 2.0 * b.q_max / (double)b.n_q;
    return d;
}

inline bool hbt_bins_valid(const is3d_hbt_bins &b)
{
    if (!(b.y_cut > 0.0 && b.pT_min >= 0.0 && b.pT_max > b.pT_min && b.kT_min >= 0.0 && b.kT_max > b.kT_min && b.q_max > 0.0)) return false;   // (NaN: false)
    if (!(b.n_kT >= 1 && b.n_kT <= kHbtMaxKT && b.n_q >= 2 && b.n_q <= kHbtMaxQ)) return false;
    const HbtDerived d = hbt_derived(b);
    const double big = 1.7976931348623157e308;
    return d.lo > 0.0 && d.lo <= big && d.hi > 0.0 && d.hi <= big && d.dkT > 0.0 && d.dkT <= big && d.dq > 0.0 && d.dq <= big && b.pT_max <= big;
}

// a compact record of an accepted particle: 64 bytes
struct HbtRecord { double E, px, py, pz, t, x, y, z; };

// the single-particle rule (the slot is the caller's)
IS3D_BINS_HD bool hbt_accept(const is3d_hbt_bins &b, const HbtDerived &d, double E, double px, double py, double pz)
{
    IS3D_BINS_NO_CONTRACT
    const double num = E + pz, den = E - pz;
    if (!(den > 0.0)) return false;
    const double ratio = num / den;
    if (!(ratio >= d.lo && ratio <= d.hi)) return false;                          // (NaN compares false: not accepted)
    const double px2 = px * px, py2 = py * py;
    const double pT = sqrt(px2 + py2);
    return pT >= b.pT_min && pT < b.pT_max;
}

IS3D_BINS_HD int64_t hbt_slot_bins(const is3d_hbt_bins &b) { return (int64_t)b.n_kT * b.n_q * b.n_q * b.n_q; }

// the ordered pair (i, j): the bin inside a slot's block, ((ikT n_q + io) n_q + is) n_q + il, or -1 (adds nothing).  No phase yet: this
// is the cheap reject on the q cube, which most pairs of an event end in
IS3D_BINS_HD int hbt_pair_bin(const is3d_hbt_bins &b, const HbtDerived &d, const HbtRecord &i, const HbtRecord &j)
{
    IS3D_BINS_NO_CONTRACT
    const double Kx = (i.px + j.px) * 0.5, Ky = (i.py + j.py) * 0.5;
    const double Kx2 = Kx * Kx, Ky2 = Ky * Ky;
    const double KT = sqrt(Kx2 + Ky2);
    if (!(KT > 0.0 && KT >= b.kT_min && KT < b.kT_max)) return -1;
    const double qx = i.px - j.px, qy = i.py - j.py;
    const double nq = (double)b.n_q;
    const double o1 = qx * Kx, o2 = qy * Ky;
    const double qo = (o1 + o2) / KT;
    const double uo = (qo + b.q_max) / d.dq;
    if (!(uo >= 0.0 && uo < nq)) return -1;
    const double s1 = qx * Ky, s2 = qy * Kx;
    const double qs = (s1 - s2) / KT;
    const double us = (qs + b.q_max) / d.dq;
    if (!(us >= 0.0 && us < nq)) return -1;
    const double K0 = (i.E + j.E) * 0.5, Kz = (i.pz + j.pz) * 0.5;
    const double q0 = i.E - j.E, qz = i.pz - j.pz;
    const double beta = Kz / K0;
    const double bb = beta * beta;
    const double g2 = 1.0 - bb;
    if (!(g2 > 0.0)) return -1;
    const double bq = beta * q0;
    const double ql = (qz - bq) / sqrt(g2);
    const double ul = (ql + b.q_max) / d.dq;
    if (!(ul >= 0.0 && ul < nq)) return -1;
    int ikT = (int)((KT - b.kT_min) / d.dkT);
    if (ikT > b.n_kT - 1) ikT = b.n_kT - 1;
    return ((ikT * b.n_q + (int)uo) * b.n_q + (int)us) * b.n_q + (int)ul;
}

// the phase of an accepted pair
IS3D_BINS_HD double hbt_pair_phase(const HbtRecord &i, const HbtRecord &j)
{
    IS3D_BINS_NO_CONTRACT
    const double q0 = i.E - j.E, qx = i.px - j.px, qy = i.py - j.py, qz = i.pz - j.pz;
    const double dt = i.t - j.t, dx = i.x - j.x, dy = i.y - j.y, dz = i.z - j.z;
    const double e0 = q0 * dt, e1 = qx * dx, e2 = qy * dy, e3 = qz * dz;
    return (((e0 - e1) - e2) - e3) / kHbtHbarC;
}

// the numerator's term of an accepted pair
IS3D_BINS_HD long long hbt_pair_term(const HbtRecord &i, const HbtRecord &j) { return sampler_vn_fixed(cos(hbt_pair_phase(i, j))); }

// kernel_form = 2: the workgroup keeps den and num of ONE slot's block in LDS beside its staged j tile
constexpr int kHbtThreads = 256;                                                   // a tile of i, a tile of j
constexpr int64_t kHbtLdsBytes = 65536;
constexpr int64_t kHbtPrivateWords = (kHbtLdsBytes - kHbtThreads * (int64_t)sizeof(HbtRecord)) / (2 * (int64_t)sizeof(int64_t));   // 3072 bins
inline bool hbt_private_fits(const is3d_hbt_bins &b) { return hbt_slot_bins(b) <= kHbtPrivateWords; }

// the argument checks of every HBT entry (IS3D_EINVAL, no device use): null, sizes, bins, the slot map; device: kernel_form too
int hbt_check_args(const is3d_hbt_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                   const is3d_hbt_hist *hist, bool device);
void hbt_hist_zero(const is3d_hbt_bins &b, const is3d_hbt_hist *h, int32_t n_events, int32_t n_slots);
// IS3D_EDOMAIN for a den word above IS3D_SAMPLER_VN_MAX_COUNT
int hbt_hist_check(const is3d_hbt_bins &b, const is3d_hbt_hist *h, int32_t n_slots);

#if defined(__HIP__) || defined(__HIPCC__)
// one run of workgroup work: the tile of i [i0, i0 + 256) of the segment [base, base + n) against its records [j0, j1)
struct HbtItem {
    int64_t base;
    int32_t n, slot, i0, j0, j1, pad;
};

// The device side of one run (cf_sampler_hbt.hip).  begin() sizes and zeroes the histogram block den | num (2 n_slots n_kT n_q^3 words,
// kept until finish()) and the host's M.  A batch of particles whose events are complete in it goes through
//   batch_begin()                       the per-segment counts zeroed
//   a count pass  (count_dev)           the caller's kernel: +1 per accepted particle of (event, slot)
//   batch_plan()                        counts to the host: M, the scan, the record block sized, the cursors zeroed, the work items
//   a fill pass   (cursor_dev, offset_dev, records_dev)   the caller's kernel: the same particles again, a record each
//   batch_pairs()                       cf_hbt_pairs over the work items
// and its records are discarded.  finish() copies the histograms out.
struct HbtRun {
    is3d_hbt_bins b;
    HbtDerived d;
    int32_t n_events = 0, n_slots = 0;
    int form = 1;                       // 1 or 2, resolved from b.kernel_form
    DevBuf<unsigned char> d_hist, d_count, d_offset, d_records, d_items;
    std::vector<int64_t> M;
    std::vector<unsigned> counts;
    int64_t n_items = 0, n_records = 0;
    double ms_pairs = 0.0;

    int begin(const is3d_hbt_bins &bins, int32_t events, int32_t slots);
    int batch_begin();
    int batch_plan();
    int batch_pairs();
    int finish(const is3d_hbt_hist *hist);
    unsigned *count_dev() const { return d_count.as<unsigned>(); }                 // [n_events n_slots], then the cursors [n_events n_slots]
    unsigned *cursor_dev() const { return d_count.as<unsigned>() + (size_t)n_events * n_slots; }
    const int64_t *offset_dev() const { return d_offset.as<int64_t>(); }
    HbtRecord *records_dev() const { return d_records.as<HbtRecord>(); }
};

// what a count or fill pass needs in a kernel
struct HbtSelectArgs {
    is3d_hbt_bins b;
    HbtDerived d;
    int32_t n_events, n_slots;
    unsigned *count;                    // count pass: the counts; fill pass: the cursors
    const int64_t *offset;              // fill pass only (NULL: count pass)
    HbtRecord *records;
};
inline HbtSelectArgs hbt_select_args(const HbtRun &r, bool fill)
{
    return HbtSelectArgs{r.b, r.d, r.n_events, r.n_slots, fill ? r.cursor_dev() : r.count_dev(), fill ? r.offset_dev() : nullptr, r.records_dev()};
}
// one accepted particle of (ev, s): a count, or its record at the segment's cursor (order inside a segment is free: the sums are integers)
__device__ __forceinline__ void hbt_select_put(const HbtSelectArgs &a, int ev, int s, const HbtRecord &r)
{
    const int64_t seg = (int64_t)ev * a.n_slots + s;
    const unsigned k = atomicAdd(&a.count[seg], 1u);
    if (a.offset) a.records[a.offset[seg] + k] = r;
}
// cf_hbt_select over a DEVICE list on the null stream: the count pass (fill = false) or the fill pass
hipError_t hbt_select_launch(const HbtRun &r, const int32_t *slot_dev, int n_species, const is3d_particle *particles_dev, int64_t n, bool fill);
// a whole batch of a device list: batch_begin, count, batch_plan, fill, batch_pairs
int hbt_batch_list(HbtRun &r, const int32_t *slot_dev, int n_species, const is3d_particle *particles_dev, int64_t n);
#endif

}  // namespace is3d
