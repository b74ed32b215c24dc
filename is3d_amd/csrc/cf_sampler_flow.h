// cf_sampler_flow.h -- the per-particle rule of the per-event flow records (multiplicity M and flow vectors Q_n = sum e^{i n phi}, n = 1..8, for
// the full acceptance and two rapidity sub-events), stated ONCE for the host (flow_host.cpp: is3d_flow_list) and the device (cf_sampler_flow.hip, cf_decays_mc.hip).
//
// The arithmetic that decides a region -- E + pz, E - pz, their ONE division, the sum of squares under the square root, the comparisons -- is
// compiled with floating-point contraction OFF on both sides.  +, -, *, / and sqrt are correctly rounded on both sides and the four rapidity
// thresholds are computed once on the host (flow_thresholds) and handed to the kernel as bits, so host and device reach the same region from
// the same particle bits: no region decision goes through log, atan2 or any other libm function.  phi = atan2(py, px) feeds only the terms,
// each added as llrint(term * 2^32) (sampler_vn_fixed), so every record word is an integer sum.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/is3d_amd.h"
#include "cf_sampler_bins.h"

namespace is3d {

constexpr int kFlowRegions = 3;                                              // 0 full acceptance, 1 sub-event A, 2 sub-event B
constexpr int kFlowRegionWords = 1 + 2 * IS3D_FLOW_HARMONICS;                // M, Q_re[8], Q_im[8]
constexpr int kFlowRecordWords = kFlowRegions * kFlowRegionWords;            // 51 words per (event, slot)

// exp(-2 y_cut), exp(2 y_cut), exp(-y_gap), exp(y_gap): the rapidity cuts as bounds on (E + pz) / (E - pz) = e^{2y}
struct FlowThresholds { double lo, hi, a, b; };

IS3D_BINS_HD bool flow_cuts_valid(const is3d_flow_cuts &c)
{
    return c.y_cut > 0.0 && c.y_gap >= 0.0 && c.y_gap < 2.0 * c.y_cut && c.pT_min >= 0.0 && c.pT_max > c.pT_min;   // (NaN: false)
}

inline FlowThresholds flow_thresholds(const is3d_flow_cuts &c)
{
    FlowThresholds t;
    t.lo = exp(-2.0 * c.y_cut);
    t.hi = exp(2.0 * c.y_cut);
    t.a = exp(-c.y_gap);
    t.b = exp(c.y_gap);
    return t;
}

// the region of one particle: -1 adds nothing, 0 full acceptance only, 1 sub-event A (and full), 2 sub-event B (and full)
IS3D_BINS_HD int flow_region(const is3d_flow_cuts &c, const FlowThresholds &t, const is3d_particle &q)
{
    IS3D_BINS_NO_CONTRACT
    const double num = q.E + q.pz, den = q.E - q.pz;
    if (!(den > 0.0)) return -1;
    const double ratio = num / den;
    if (!(ratio >= t.lo && ratio <= t.hi)) return -1;                         // (NaN compares false: no region)
    const double px2 = q.px * q.px, py2 = q.py * q.py;
    const double pT = sqrt(px2 + py2);
    if (!(pT >= c.pT_min && pT < c.pT_max)) return -1;
    if (ratio < t.a) return 1;
    if (ratio > t.b) return 2;
    return 0;
}

// the 16 fixed-point terms of one particle: re[n - 1] = llrint(cos(n phi) 2^32), im[n - 1] = llrint(sin(n phi) 2^32)
IS3D_BINS_HD void flow_terms(const is3d_particle &q, long long *re, long long *im)
{
    const double phi = atan2(q.py, q.px);
    for (int m = 0; m < IS3D_FLOW_HARMONICS; m++) {
        double sn, cs;
#if defined(__HIP_DEVICE_COMPILE__)
        sincos(((double)m + 1.0) * phi, &sn, &cs);
#else
        cs = cos(((double)m + 1.0) * phi);
        sn = sin(((double)m + 1.0) * phi);
#endif
        re[m] = sampler_vn_fixed(cs);
        im[m] = sampler_vn_fixed(sn);
    }
}

// the device block of a run: n_events * n_slots records of 51 words, a record laid out  M | Q_re[8] | Q_im[8]  per region
IS3D_BINS_HD int64_t flow_record_word(int64_t event, int64_t slot, int n_slots, int region)
{
    return ((event * n_slots + slot) * kFlowRegions + region) * kFlowRegionWords;
}

// the argument checks of every flow entry (IS3D_EINVAL, no device use): null, sizes, cuts, the slot map, kernel_form, and kernel_form = 2
// when not even one event's records fit the LDS beside device_static_words words of static LDS (-1: a host entry, no form to refuse)
int flow_check_args(const is3d_flow_cuts *cuts, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                    const is3d_flow_records *records, int device_static_words);
// device block (n_events * n_slots * 51 words) <-> the caller's three arrays
void flow_records_zero(const is3d_flow_records *r, int32_t n_events, int32_t n_slots);
void flow_records_scatter(const int64_t *block, const is3d_flow_records *r, int32_t n_events, int32_t n_slots);
// IS3D_EDOMAIN for a record whose M is above IS3D_SAMPLER_VN_MAX_COUNT
int flow_records_check(const is3d_flow_records *r, int32_t n_events, int32_t n_slots);

constexpr int64_t kFlowLdsWords = 65536 / sizeof(unsigned long long);
// the number of consecutive events whose records the workgroup-private form keeps in LDS (0: not even one fits); static_words: what the
// kernel keeps in static LDS beside the window (the decay kernel's tally words)
inline int flow_window_events(int32_t n_events, int32_t n_slots, int static_words = 0)
{
    const int64_t w = (kFlowLdsWords - static_words) / ((int64_t)n_slots * kFlowRecordWords);
    return (int)(w < n_events ? w : n_events);
}

#if defined(__HIP__) || defined(__HIPCC__)
// where a kernel's adds go: the workgroup's window of `window` events from event `base` in LDS (PRIVATE form), the global block otherwise
struct FlowTarget {
    unsigned long long *priv, *records;
    int base, window, n_slots, n_events;
};

// word w of the record (ev, s): in the window, or in the global block -- two address spaces, two atomics, no flat access
template <bool PRIVATE>
__device__ __forceinline__ void flow_add_word(const FlowTarget &t, int ev, int s, int w, unsigned long long v)
{
    if (PRIVATE) {
        const unsigned d = (unsigned)(ev - t.base);
        if (ev >= t.base && d < (unsigned)t.window) {
            extern __shared__ unsigned long long flow_window[];   // the kernel's dynamic LDS, named here so that the add is a DS one
            atomicAdd(&flow_window[((int64_t)d * t.n_slots + s) * kFlowRecordWords + w], v);
            return;
        }
    }
    atomicAdd(&t.records[flow_record_word(ev, s, t.n_slots, 0) + w], v);
}

// the adds of ONE particle of region >= 0: to region 0 and to its sub-event, 17 words each (two's complement: signed sums)
template <bool PRIVATE>
__device__ __forceinline__ void flow_add_particle(const FlowTarget &t, int ev, int s, int region, const long long *re, const long long *im)
{
    for (int r = 0; r <= region; r += (region ? region : 1)) {
        flow_add_word<PRIVATE>(t, ev, s, r * kFlowRegionWords, 1ULL);
        for (int m = 0; m < IS3D_FLOW_HARMONICS; m++) {
            flow_add_word<PRIVATE>(t, ev, s, r * kFlowRegionWords + 1 + m, (unsigned long long)re[m]);
            flow_add_word<PRIVATE>(t, ev, s, r * kFlowRegionWords + 1 + IS3D_FLOW_HARMONICS + m, (unsigned long long)im[m]);
        }
    }
}

__device__ __forceinline__ long long flow_wave_sum(long long v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The adds of ONE trip of a list kernel: every lane of every wave calls this, act = the lane holds a particle of region >= 0 for the record
// (ev, s).  COMBINE: the lanes of a wave that hold the same (event, slot, region) key sum their 17 values with cross-lane adds and ONE lane
// does the 17 adds (34 with a sub-event) -- a ballot loop over the distinct keys of the wave, which retires its leader's key on every trip.
template <bool PRIVATE, bool COMBINE>
__device__ __forceinline__ void flow_add_trip(const FlowTarget &t, int lane, bool act, int ev, int s, int region, const long long *re,
                                              const long long *im)
{
    if (COMBINE) {
        const long long key = act ? ((long long)ev * t.n_slots + s) * kFlowRegions + region : -1;
        unsigned long long rem = __ballot(act);
        while (rem) {                                  // wave-uniform; every trip retires the key of its leader
            const int leader = __ffsll((long long)rem) - 1;
            const long long k = __shfl(key, leader);
            const bool mine = act && key == k;
            const unsigned long long match = __ballot(mine);
            rem &= ~match;
            const bool alone = (match & (match - 1)) == 0;
            const bool add = lane == leader;
            const long long cnt = __popcll(match);
            if (add) {
                flow_add_word<PRIVATE>(t, ev, s, 0, (unsigned long long)cnt);
                if (region) flow_add_word<PRIVATE>(t, ev, s, region * kFlowRegionWords, (unsigned long long)cnt);
            }
            for (int m = 0; m < IS3D_FLOW_HARMONICS; m++) {
                long long vr = mine ? re[m] : 0, vi = mine ? im[m] : 0;
                if (!alone) { vr = flow_wave_sum(vr); vi = flow_wave_sum(vi); }
                if (add) {
                    flow_add_word<PRIVATE>(t, ev, s, 1 + m, (unsigned long long)vr);      // two's complement: signed sums
                    flow_add_word<PRIVATE>(t, ev, s, 1 + IS3D_FLOW_HARMONICS + m, (unsigned long long)vi);
                    if (region) {
                        flow_add_word<PRIVATE>(t, ev, s, region * kFlowRegionWords + 1 + m, (unsigned long long)vr);
                        flow_add_word<PRIVATE>(t, ev, s, region * kFlowRegionWords + 1 + IS3D_FLOW_HARMONICS + m,
                                               (unsigned long long)vi);
                    }
                }
            }
        }
    } else if (act) {
        flow_add_particle<PRIVATE>(t, ev, s, region, re, im);
    }
}

// the launch geometry of a list kernel of `threads` threads over n particles: contiguous slices, a multiple of the trip
constexpr int kFlowPrivateBlocks = 512;                  // workgroup-private form: at most this many flushes
constexpr int64_t kFlowPrivateParticles = 4096;          // ... and at least this many particles per workgroup
constexpr int64_t kFlowGlobalBlocks = (int64_t)1 << 20;
inline void flow_list_geometry(bool priv, int64_t n, int threads, int64_t *blocks, int64_t *slice)
{
    if (priv) {
        int64_t b = (n + kFlowPrivateParticles - 1) / kFlowPrivateParticles;
        b = b < 1 ? 1 : (b > kFlowPrivateBlocks ? kFlowPrivateBlocks : b);
        *slice = ((n + b - 1) / b + threads - 1) / threads * threads;
    } else {
        *slice = ((n + kFlowGlobalBlocks - 1) / kFlowGlobalBlocks + threads - 1) / threads * threads;
    }
    *blocks = (n + *slice - 1) / *slice;
}

// The window of a workgroup that walks the slice [begin, end) in trips of THREADS: it starts at the event of the slice's first valid entry
// (event_of(i) >= 0) -- the lowest thread that holds one names it, through two control words of the block, which is zeroed afterwards.
// Every thread of the workgroup calls this with the same arguments; all leave the search together.  Returns the base (0: no valid entry).
template <int THREADS, class EventOf>
__device__ __forceinline__ int flow_window_open(unsigned long long *priv, int64_t words, int64_t begin, int64_t end, EventOf event_of)
{
    int *ctl = (int *)priv;
    if (threadIdx.x == 0) { ctl[0] = THREADS; ctl[1] = -1; }
    __syncthreads();
    for (int64_t i0 = begin; i0 < end; i0 += THREADS) {
        const int64_t i = i0 + threadIdx.x;
        const int ev = i < end ? event_of(i) : -1;
        if (ev >= 0) atomicMin(&ctl[0], (int)threadIdx.x);
        __syncthreads();
        if (ctl[0] == (int)threadIdx.x) ctl[1] = ev;
        __syncthreads();
        if (ctl[1] >= 0) break;                            // the same word for every thread
    }
    const int base = ctl[1] >= 0 ? ctl[1] : 0;
    __syncthreads();
    for (int64_t j = threadIdx.x; j < words; j += THREADS) priv[j] = 0ULL;
    __syncthreads();
    return base;
}

// ... and its one flush: the non-zero words, with global 64-bit adds
template <int THREADS>
__device__ __forceinline__ void flow_window_flush(const FlowTarget &t)
{
    __syncthreads();
    const int64_t words = (int64_t)t.window * t.n_slots * kFlowRecordWords;
    const int64_t first = flow_record_word(t.base, 0, t.n_slots, 0), total = flow_record_word(t.n_events, 0, t.n_slots, 0);
    for (int64_t j = threadIdx.x; j < words; j += THREADS) {
        const unsigned long long v = t.priv[j];
        if (v && first + j < total) atomicAdd(&t.records[first + j], v);
    }
}

// the device side (cf_sampler_flow.hip): n particles (a DEVICE list, ordered by event as the sampler fills it; any order is counted
// correctly) added into records_dev (n_events * n_slots * 51 words) on the null stream.  form: 0 = the measured choice, 1 = global
// atomics after a per-wave combine, 2 = workgroup-private window (needs flow_window_events >= 1).
hipError_t flow_launch(const is3d_flow_cuts &c, const FlowThresholds &t, int n_events, int n_slots, const int32_t *slot_dev, int n_species,
                       const is3d_particle *particles_dev, int64_t n, unsigned long long *records_dev, int form);
#endif

}  // namespace is3d
