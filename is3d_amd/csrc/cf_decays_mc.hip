// cf_decays_mc.hip -- Monte Carlo decays of sampled hadrons to stable particles on the device (is3d_decay_particles; the reference has no
// counterpart: include/is3d_amd.h is the definition, DESIGN.md section 3p the account).
//
// Thread <-> primary.  A primary's whole decay tree is walked depth-first by one thread and draws from ONE Philox stream
// (stream 5, keyed by the primary's global index), so the count pass and the fill pass replay the same tree:
//   cf_decay_mc<false>  counts the final particles of every primary (int32) and adds the run-wide tallies
//   hipCUB exclusive scan of the counts (as the samplers')
//   cf_decay_mc<true>   the same loop body, every final particle stored at the primary's offset
// and, for a caller that wants the test_sampler distributions of the decayed list and not the list (is3d_decay_particles_binned, the batch
// loop of cf_sampler.hip), ONE pass without counts, offsets or scan:
//   cf_decay_mc_bins    the same loop body, every final particle built in registers and given to the bin rule of cf_sampler_bins.h at once
// What a pass does with a final particle is its sink (SinkCount, SinkStore, SinkBin): the one thing in which the three differ.
// The particle in hand lives in registers; its pending siblings wait on a stack in private memory (kStack entries of 88 bytes: the
// table analysis on the host proves the need before any launch).  The table goes to the device flat, OPEN channels only, with the
// running sums of their branching ratios, so the channel of a decay is the first whose sum exceeds u * (last sum).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_host.h"
#include "cf_sampler_common.h"
#include "cf_decays_mc.h"
#include "errors.h"

namespace {

using is3d::DevBuf;
using is3d::kHbarC;
using is3d::Rng;
using is3d::set_error;

constexpr int kBodies = IS3D_DECAY_MC_MAX_BODIES, kStack = IS3D_DECAY_MC_MAX_STACK, kTrials = IS3D_DECAY_MC_MAX_TRIALS;
constexpr int kThreads = 128;
constexpr int kTallies = 5;   // decays, stuck, trials, exhausted, primaries whose stack would have overflowed (never: the host proves it)
constexpr int kBinThreads = 256;                         // cf_decay_mc_bins
constexpr int kBinTallies = is3d::kDecayMcBinTallies;    // ... which has no count pass to learn the number of final particles from: word kTallies
constexpr int kBinPrivateBlocks = 512;                   // private form: at most this many flushes (its VGPRs let two workgroups share a CU: one round on 256 CUs)
static_assert(kBinTallies == kTallies + 1, "the bin pass adds the final particles to the tallies of the count pass");

struct McTable {              // device arrays: per entry | per open channel
    const double *mass, *width;
    const int32_t *stable, *ch0;      // ch0[n + 1]: entry e's open channels are [ch0[e], ch0[e + 1])
    const double *cum;                // running sum of the entry's open branching ratios, file order
    const int32_t *nbody, *dau;       // products; their table entries [channel][kBodies]
};

struct McArgs {
    McTable t;
    const int32_t *chosen_entry;      // species of the input list -> table entry
    const is3d_particle *in;
    int64_t n, first;
    uint64_t seed;
    int32_t lifetime;
    int32_t *counts;                  // written by the count pass; the fill pass stores no more than it counted
    const int64_t *offsets;           // fill pass
    is3d_particle *out;
    int64_t *origin;                  // may be null
    unsigned long long *tally;        // [kTallies]
};

struct Pending {
    double E, px, py, pz, t, x, y, z, tau, eta;
    int32_t e;
};

// momentum of the two products b, c of a at rest
__device__ __forceinline__ double pstar(double a, double b, double c)
{
    return sqrt(fmax((a - b - c) * (a + b + c) * (a + b - c) * (a - b + c), 0.0)) / (2.0 * a);
}

// (e, q) of a frame that moves with velocity b (gamma, b2 = b.b) taken to the lab by one pure boost; b = 0 leaves it as it is
__device__ __forceinline__ void boost(double bx, double by, double bz, double b2, double gamma, double e, double qx, double qy, double qz,
                                      Pending &o)
{
    if (b2 > 0.0) {
        const double bq = bx * qx + by * qy + bz * qz;
        const double f = (gamma - 1.0) * bq / b2 + gamma * e;
        o.E = gamma * (e + bq); o.px = qx + f * bx; o.py = qy + f * by; o.pz = qz + f * bz;
    } else {
        o.E = e; o.px = qx; o.py = qy; o.pz = qz;
    }
}

// ---- what a pass does with a final particle (decay_tree): kMomenta tells whether the pass needs the products' momenta at all ----
struct SinkCount {
    static constexpr bool kMomenta = false;
    __device__ __forceinline__ void operator()(int, const Pending &, const is3d_particle &) {}
};
// the fill pass: final particle number nfinal of the primary at its offset, no more than the count pass counted
struct SinkStore {
    static constexpr bool kMomenta = true;
    const McArgs &a;
    int64_t i, slot0;
    int counted;
    __device__ __forceinline__ void operator()(int nfinal, const Pending &c, const is3d_particle &q)
    {
        if (nfinal < counted) {
            is3d_particle o;
            o.cell = q.cell; o.event = q.event; o.species = c.e;
            o.tau = c.tau; o.x = c.x; o.y = c.y; o.eta = c.eta; o.t = c.t; o.z = c.z;
            o.E = c.E; o.px = c.px; o.py = c.py; o.pz = c.pz;
            a.out[slot0 + nfinal] = o;
            if (a.origin) a.origin[slot0 + nfinal] = i;
        }
    }
};
// the bin pass: the same is3d_particle, built in registers, goes to the rule of cf_sampler_bins.h with slot[entry] as its species; slot -1
// (or a primary whose event has no yield word) adds nothing.  kept counts what was binned: the primary's share of its event's yield.
struct McBinArgs {
    is3d_sampler_test_bins b;
    is3d::SamplerBinWidths w;
    is3d::SamplerHistLayout l;        // of n_slots species
    int32_t n_slots, n_events;
    const int32_t *slot;              // [table entries]
    unsigned long long *hist, *yield, *tally;   // tally[kBinTallies]
};
struct SinkBin {
    static constexpr bool kMomenta = true;
    const McBinArgs &b;
    unsigned long long *h;            // the workgroup's LDS block, or the global one
    bool live;
    long long kept;
    __device__ __forceinline__ void operator()(int, const Pending &c, const is3d_particle &q)
    {
        const int s = b.slot[c.e];
        if (!live || s < 0 || s >= b.n_slots) return;
        is3d_particle o;
        o.cell = q.cell; o.event = q.event; o.species = s;
        o.tau = c.tau; o.x = c.x; o.y = c.y; o.eta = c.eta; o.t = c.t; o.z = c.z;
        o.E = c.E; o.px = c.px; o.py = c.py; o.pz = c.pz;
        const is3d::SamplerBinIndex k = is3d::sampler_bin_particle(b.b, b.w, o);
        is3d::sampler_bin_add(b.b, b.l, b.n_slots, k, s, h);
        kept++;
    }
};

// the decay tree of primary i; returns its number of final particles
template <class Sink>
__device__ __forceinline__ int decay_tree(const McArgs &a, int64_t i, unsigned long long (&tally)[kTallies], Sink &sink)
{
    constexpr bool KEEP = Sink::kMomenta;
    const is3d_particle q = a.in[i];
    const uint64_t gi = (uint64_t)(a.first + i);
    Rng g;
    g.init(a.seed, 5, (uint32_t)gi, (uint32_t)(gi >> 32));
    Pending stack[kStack];
    int sp = 0, nfinal = 0;
    Pending c;
    c.E = q.E; c.px = q.px; c.py = q.py; c.pz = q.pz; c.t = q.t; c.x = q.x; c.y = q.y; c.z = q.z; c.tau = q.tau; c.eta = q.eta;
    c.e = a.chosen_entry[q.species];
    for (;;) {
        const int c0 = a.t.ch0[c.e], c1 = a.t.ch0[c.e + 1];
        const bool stable = a.t.stable[c.e] != 0;
        if (stable || c0 == c1) {                       // final: stable, or stuck without an open channel
            if (!stable) tally[1]++;
            sink(nfinal, c, q);
            nfinal++;
            if (sp == 0) break;
            c = stack[--sp];
            continue;
        }
        tally[0]++;
        const double M = a.t.mass[c.e];
        // channel: the first open one whose running sum exceeds u * (last sum); the last one otherwise
        const double uc = g.uniform() * a.t.cum[c1 - 1];
        int j = c1 - 1;
        for (int k = c0; k < c1 - 1; k++)
            if (uc < a.t.cum[k]) { j = k; break; }
        if (a.lifetime) {
            const double u_tau = g.uniform(), width = a.t.width[c.e];
            if (width > 0.0) {
                const double ts = -(kHbarC / width) * log1p(-u_tau);
                c.t += (c.E / M) * ts; c.x += (c.px / M) * ts; c.y += (c.py / M) * ts; c.z += (c.pz / M) * ts;
                c.tau = sqrt(c.t * c.t - c.z * c.z);
                c.eta = atanh(c.z / c.t);
            }
        }
        const int n = a.t.nbody[j];
        if (sp + n - 1 > kStack) { tally[4]++; break; }   // (the host's table analysis rules it out)
        double m[kBodies], S[kBodies], mu[kBodies];
        int de[kBodies];
#pragma unroll
        for (int k = 0; k < kBodies; k++) {
            de[k] = k < n ? a.t.dau[j * kBodies + k] : 0;
            m[k] = k < n ? a.t.mass[de[k]] : 0.0;
            S[k] = k ? S[k - 1] + m[k] : m[0];
        }
        const double T = M - S[n - 1];
        double wmax = 1.0;
        for (int k = 1; k < n; k++) wmax *= pstar(T + S[k], S[k - 1], m[k]);
        // cluster masses: flat n-body phase space by mass generation with rejection
        for (int trial = 1;; trial++) {
            tally[2]++;
            double r[kBodies - 2];
            for (int k = 0; k < n - 2; k++) {           // insertion sort, ascending
                const double u = g.uniform();
                int l = k;
                while (l > 0 && r[l - 1] > u) { r[l] = r[l - 1]; l--; }
                r[l] = u;
            }
            mu[0] = m[0];
            for (int k = 1; k < n - 1; k++) mu[k] = S[k] + r[k - 1] * T;
            mu[n - 1] = S[n - 1] + T;
            if (n == 2) break;
            double w = 1.0;
            for (int k = 1; k < n; k++) w *= pstar(mu[k], mu[k - 1], m[k]);
            const double u_acc = g.uniform();
            if (u_acc * wmax < w) break;
            if (trial == kTrials) { tally[3]++; break; }
        }
        // momenta, top-down: cluster k splits into particle k and cluster k - 1 (the count pass draws the two angles and moves on: nothing it
        // counts depends on a momentum)
        Pending P = c;                                   // the current cluster's lab momentum, and the vertex every product is born at
        for (int k = n - 1; k >= 1; k--) {
            const double u_cos = g.uniform(), u_phi = g.uniform();
            Pending d = P;
            d.e = de[k];
            if (KEEP) {
                const double ct = 2.0 * u_cos - 1.0, st = sqrt(fmax(1.0 - ct * ct, 0.0));
                double sn, cs;
                sincos(2.0 * M_PI * u_phi, &sn, &cs);
                const double p = pstar(mu[k], mu[k - 1], m[k]);
                const double dx = p * (st * cs), dy = p * (st * sn), dz = p * ct;
                const double bx = P.px / P.E, by = P.py / P.E, bz = P.pz / P.E, b2 = bx * bx + by * by + bz * bz;
                const double gamma = 1.0 / sqrt(1.0 - b2);
                boost(bx, by, bz, b2, gamma, sqrt(p * p + m[k] * m[k]), dx, dy, dz, d);
                boost(bx, by, bz, b2, gamma, sqrt(p * p + mu[k - 1] * mu[k - 1]), -dx, -dy, -dz, P);
            }
            stack[sp++] = d;
        }
        P.e = de[0];
        c = P;
    }
    return nfinal;
}

template <bool KEEP>
__global__ void __launch_bounds__(kThreads) cf_decay_mc(const McArgs a)
{
    unsigned long long tally[kTallies] = {0ULL, 0ULL, 0ULL, 0ULL, 0ULL};
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < a.n) {
        if (KEEP) {
            SinkStore sink{a, i, a.offsets[i], a.counts[i]};
            decay_tree(a, i, tally, sink);
        } else {
            SinkCount sink;
            a.counts[i] = decay_tree(a, i, tally, sink);
        }
    }
    if (!KEEP) {   // one global add per counter and workgroup
        __shared__ unsigned long long blk[kTallies];
        if (threadIdx.x < kTallies) blk[threadIdx.x] = 0ULL;
        __syncthreads();
        for (int k = 0; k < kTallies; k++)
            if (tally[k]) atomicAdd(&blk[k], tally[k]);
        __syncthreads();
        if (threadIdx.x < kTallies && blk[threadIdx.x]) atomicAdd(&a.tally[threadIdx.x], blk[threadIdx.x]);
    }
}

// The one-pass bin kernel.  Every workgroup walks a grid-stride slice of the primaries (the trip count is the same for every thread of the
// workgroup, so the wave operations of sampler_yield_runs see whole waves).  PRIVATE: the histogram block lives in LDS (dynamic, l.total
// words, beside the static tally words) and is flushed once, non-zero words only; otherwise every add is a global 64-bit atomic.  The
// pending stack stays in private memory in both forms.  Yields: a primary's binned finals share its event, and the primaries come ordered
// by event, so the first lane of a run of equal events adds the run's sum -- one add per distinct event per wave.
template <bool PRIVATE>
__global__ void __launch_bounds__(kBinThreads) cf_decay_mc_bins(const McArgs a, const McBinArgs b)
{
    extern __shared__ unsigned long long priv[];
    __shared__ unsigned long long blk[kBinTallies];
    if (threadIdx.x < kBinTallies) blk[threadIdx.x] = 0ULL;
    if (PRIVATE)
        for (int64_t j = threadIdx.x; j < b.l.total; j += kBinThreads) priv[j] = 0ULL;
    __syncthreads();
    unsigned long long tally[kTallies] = {0ULL, 0ULL, 0ULL, 0ULL, 0ULL}, finals = 0ULL;
    for (int64_t i0 = (int64_t)blockIdx.x * kBinThreads; i0 < a.n; i0 += (int64_t)gridDim.x * kBinThreads) {
        const int64_t i = i0 + threadIdx.x;
        int ev = INT_MAX;                                  // lanes past the end, or with an event outside the yields: no add at all
        long long kept = 0;
        if (i < a.n) {
            const int event = a.in[i].event;
            const bool live = event >= 0 && event < b.n_events;
            SinkBin sink{b, PRIVATE ? priv : b.hist, live, 0};
            finals += (unsigned long long)decay_tree(a, i, tally, sink);
            if (live) { ev = event; kept = sink.kept; }
        }
        is3d::sampler_yield_runs(ev, kept, b.yield);
    }
    for (int k = 0; k < kTallies; k++)
        if (tally[k]) atomicAdd(&blk[k], tally[k]);
    if (finals) atomicAdd(&blk[kTallies], finals);
    __syncthreads();
    if (threadIdx.x < kBinTallies && blk[threadIdx.x]) atomicAdd(&b.tally[threadIdx.x], blk[threadIdx.x]);
    if (PRIVATE)
        for (int64_t j = threadIdx.x; j < b.l.total; j += kBinThreads) {
            const unsigned long long v = priv[j];
            if (v) atomicAdd(&b.hist[j], v);
        }
}

// the flow pass: the final particle's momentum, built in registers, goes to the rule of cf_sampler_flow.h with slot[entry]; slot -1, a particle
// outside the cuts or a primary whose event has no record adds nothing.  DIFF: the differential records of cf_sampler_flow_diff.h -- the
// accepted particle's pT bin, by bisection over the edges the workgroup staged in LDS, makes its record that of the slot  slot * n_pT + bin
struct McFlowArgs {
    is3d_flow_cuts c;
    is3d::FlowThresholds t;
    int32_t n_slots, n_events, window;
    const int32_t *slot;              // [table entries]
    unsigned long long *records, *tally;   // tally[kBinTallies]
    int32_t n_pT;                     // DIFF only
    const double *edges;              // DIFF only: [n_pT + 1]
};
template <bool PRIVATE, bool DIFF>
struct SinkFlow {
    static constexpr bool kMomenta = true;
    const McFlowArgs &f;
    const is3d::FlowTarget &target;
    bool live;
    __device__ __forceinline__ void operator()(int, const Pending &c, const is3d_particle &q)
    {
        int s = f.slot[c.e];
        if (!live || s < 0 || s >= f.n_slots) return;
        is3d_particle o;
        o.E = c.E; o.px = c.px; o.py = c.py; o.pz = c.pz;
        const int region = is3d::flow_region(f.c, f.t, o);
        if (region < 0) return;
        if (DIFF) s = is3d::flow_diff_slot(s, f.n_pT, is3d::flow_diff_bin_lds(f.n_pT, o));
        long long re[IS3D_FLOW_HARMONICS], im[IS3D_FLOW_HARMONICS];
        is3d::flow_terms(o, re, im);
        is3d::flow_add_particle<PRIVATE>(target, q.event, s, region, re, im);
    }
};

// The one-pass flow kernel.  Every workgroup walks a CONTIGUOUS slice of the primaries in trips of kBinThreads (the same trip count for every
// thread).  A primary's products share its event and the primaries come ordered by event, so the window of cf_sampler_flow applies to the
// primaries' order: PRIVATE keeps the records of `window` events from the event of the slice's first primary in LDS (dynamic, beside the
// static tally words) and flushes the non-zero words once; products of a primary outside the window, and every product of the global form,
// add to global memory.  The threads of a wave reach their final particles at different times, so there is no per-wave combine here.
template <bool PRIVATE, bool DIFF>
__global__ void __launch_bounds__(kBinThreads) cf_decay_mc_flow(const McArgs a, const McFlowArgs f, const int64_t slice)
{
    extern __shared__ unsigned long long priv[];
    __shared__ unsigned long long blk[kBinTallies];
    if (threadIdx.x < kBinTallies) blk[threadIdx.x] = 0ULL;
    const int64_t begin = (int64_t)blockIdx.x * slice, end = begin + slice < a.n ? begin + slice : a.n;
    const int n_keys = DIFF ? f.n_slots * f.n_pT : f.n_slots;
    is3d::FlowTarget target{priv, f.records, 0, f.window, n_keys, f.n_events};
    if (DIFF) is3d::flow_diff_stage_edges(f.edges, f.n_pT);
    if (PRIVATE)
        target.base = is3d::flow_window_open<kBinThreads>(priv, (int64_t)f.window * n_keys * is3d::kFlowRecordWords, begin, end, [&](int64_t i) {
            const int e = a.in[i].event;
            return e >= 0 && e < f.n_events ? e : -1;
        });
    else
        __syncthreads();
    unsigned long long tally[kTallies] = {0ULL, 0ULL, 0ULL, 0ULL, 0ULL}, finals = 0ULL;
    for (int64_t i0 = begin; i0 < end; i0 += kBinThreads) {
        const int64_t i = i0 + threadIdx.x;
        if (i < end) {
            const int event = a.in[i].event;
            SinkFlow<PRIVATE, DIFF> sink{f, target, event >= 0 && event < f.n_events};
            finals += (unsigned long long)decay_tree(a, i, tally, sink);
        }
    }
    for (int k = 0; k < kTallies; k++)
        if (tally[k]) atomicAdd(&blk[k], tally[k]);
    if (finals) atomicAdd(&blk[kTallies], finals);
    __syncthreads();
    if (threadIdx.x < kBinTallies && blk[threadIdx.x]) atomicAdd(&f.tally[threadIdx.x], blk[threadIdx.x]);
    if (PRIVATE) is3d::flow_window_flush<kBinThreads>(target);
}

// the pair pass: the final particle's momentum, built in registers, goes to the rule of cf_sampler_pairs.h with slot[entry]; an accepted
// particle makes ONE 32-bit add into the occupancy block; slot -1, a particle outside the bins or a primary whose event has no grid adds nothing
struct McPairArgs {
    is3d_pair_bins b;
    is3d::PairTables t;
    int32_t n_slots, n_events;
    const int32_t *slot;              // [table entries]
    unsigned *occ;
    unsigned long long *tally;        // tally[kBinTallies]
};
struct SinkPairs {
    static constexpr bool kMomenta = true;
    const McPairArgs &f;
    bool live;
    __device__ __forceinline__ void operator()(int, const Pending &c, const is3d_particle &q)
    {
        const int s = f.slot[c.e];
        if (!live || s < 0 || s >= f.n_slots) return;
        const int cell = is3d::pair_cell(f.b, f.t, c.E, c.px, c.py, c.pz);
        if (cell >= 0) is3d::pair_add(f.b, f.occ, f.n_slots, q.event, s, cell);
    }
};

// The one-pass pair kernel: thread <-> primary in a grid-stride walk; the tallies go through six static LDS words as in cf_decay_mc_bins.
__global__ void __launch_bounds__(kBinThreads) cf_decay_mc_pairs(const McArgs a, const McPairArgs f)
{
    __shared__ unsigned long long blk[kBinTallies];
    if (threadIdx.x < kBinTallies) blk[threadIdx.x] = 0ULL;
    __syncthreads();
    unsigned long long tally[kTallies] = {0ULL, 0ULL, 0ULL, 0ULL, 0ULL}, finals = 0ULL;
    for (int64_t i = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBinThreads) {
        const int event = a.in[i].event;
        SinkPairs sink{f, event >= 0 && event < f.n_events};
        finals += (unsigned long long)decay_tree(a, i, tally, sink);
    }
    for (int k = 0; k < kTallies; k++)
        if (tally[k]) atomicAdd(&blk[k], tally[k]);
    if (finals) atomicAdd(&blk[kTallies], finals);
    __syncthreads();
    if (threadIdx.x < kBinTallies && blk[threadIdx.x]) atomicAdd(&f.tally[threadIdx.x], blk[threadIdx.x]);
}

// the HBT passes: the final particle's momentum goes to the single-particle rule of cf_sampler_hbt.h with slot[entry]; an accepted one is
// counted (count pass) or written as a compact record with its position at the cursor of its (event, slot) segment (fill pass)
struct McHbtArgs {
    is3d::HbtSelectArgs s;
    const int32_t *slot;              // [table entries]
    unsigned long long *tally;        // tally[kBinTallies], count pass
};
struct SinkHbt {
    static constexpr bool kMomenta = true;
    const McHbtArgs &f;
    bool live;
    __device__ __forceinline__ void operator()(int, const Pending &c, const is3d_particle &q)
    {
        const int s = f.slot[c.e];
        if (!live || s < 0 || s >= f.s.n_slots) return;
        if (!is3d::hbt_accept(f.s.b, f.s.d, c.E, c.px, c.py, c.pz)) return;
        is3d::hbt_select_put(f.s, q.event, s, is3d::HbtRecord{c.E, c.px, c.py, c.pz, c.t, c.x, c.y, c.z});
    }
};

// thread <-> primary in a grid-stride walk; the count pass (FILL = false) adds the tallies through six static LDS words as cf_decay_mc_bins
template <bool FILL>
__global__ void __launch_bounds__(kBinThreads) cf_decay_mc_hbt(const McArgs a, const McHbtArgs f)
{
    __shared__ unsigned long long blk[kBinTallies];
    if (threadIdx.x < kBinTallies) blk[threadIdx.x] = 0ULL;
    __syncthreads();
    unsigned long long tally[kTallies] = {0ULL, 0ULL, 0ULL, 0ULL, 0ULL}, finals = 0ULL;
    for (int64_t i = (int64_t)blockIdx.x * kBinThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBinThreads) {
        const int event = a.in[i].event;
        SinkHbt sink{f, event >= 0 && event < f.s.n_events};
        finals += (unsigned long long)decay_tree(a, i, tally, sink);
    }
    if (FILL) return;
    for (int k = 0; k < kTallies; k++)
        if (tally[k]) atomicAdd(&blk[k], tally[k]);
    if (finals) atomicAdd(&blk[kTallies], finals);
    __syncthreads();
    if (threadIdx.x < kBinTallies && blk[threadIdx.x]) atomicAdd(&f.tally[threadIdx.x], blk[threadIdx.x]);
}

struct Widen {
    __host__ __device__ int64_t operator()(int32_t v) const { return (int64_t)v; }
};

// ---- host: the table as the kernel reads it, with what can be said about it before any launch ----
struct McHostTable {
    std::vector<int32_t> ch0, nbody, dau, chosen_entry;
    std::vector<double> cum;
    int32_t max_stack = 1, max_depth = 0, n_closed = 0;
};

int analyse(const is3d_decay_table &T, int32_t n_chosen, const int64_t *chosen, McHostTable &H)
{
    if (T.n < 0) return set_error(IS3D_EINVAL, "decay table: n = %d", T.n);
    if (T.n > 0 && (!T.mc_id || !T.mass || !T.width || !T.stable || !T.n_channels)) return set_error(IS3D_EINVAL, "a decay table array is NULL");
    std::unordered_map<int64_t, int32_t> index;          // first match, as particle_index
    for (int32_t e = 0; e < T.n; e++) index.emplace(T.mc_id[e], e);
    H.chosen_entry.resize((size_t)n_chosen);
    for (int32_t s = 0; s < n_chosen; s++) {
        const auto it = index.find(chosen[s]);
        if (it == index.end()) return set_error(IS3D_EINVAL, "chosen particle %lld is not in the decay table", (long long)chosen[s]);
        H.chosen_entry[(size_t)s] = it->second;
    }
    // every channel of every unstable entry, open or not: its products as table entries
    std::vector<int64_t> first((size_t)T.n + 1, 0);
    for (int32_t e = 0; e < T.n; e++) {
        if (T.n_channels[e] < 0) return set_error(IS3D_EINVAL, "entry %d has %d channels", e, T.n_channels[e]);
        first[(size_t)e + 1] = first[(size_t)e] + T.n_channels[e];
    }
    if (first[(size_t)T.n] > 0 && (!T.npart || !T.branch_ratio || !T.daughters)) return set_error(IS3D_EINVAL, "a decay table array is NULL");
    std::vector<int32_t> all_n((size_t)first[(size_t)T.n], 0), all_d((size_t)first[(size_t)T.n] * kBodies, 0);
    H.ch0.assign((size_t)T.n + 1, 0);
    for (int32_t e = 0; e < T.n; e++) {
        H.ch0[(size_t)e + 1] = H.ch0[(size_t)e];
        if (T.stable[e]) continue;
        double run = 0.0;
        for (int64_t c = first[(size_t)e]; c < first[(size_t)e + 1]; c++) {
            const int n = std::abs(T.npart[c]);
            const int j = (int)(c - first[(size_t)e]);
            if (n > kBodies) return set_error(IS3D_EINVAL, "parent %lld channel %d: %d decay products (at most %d)", (long long)T.mc_id[e], j, n, kBodies);
            if (n < 2) return set_error(IS3D_EINVAL, "parent %lld channel %d: %d decay product(s) of an unstable particle", (long long)T.mc_id[e], j, n);
            all_n[(size_t)c] = n;
            double sum = 0.0;
            for (int k = 0; k < n; k++) {
                const int64_t id = T.daughters[c * 5 + k];
                const auto it = index.find(id);
                if (id == 0 || it == index.end())
                    return set_error(IS3D_EINVAL, "parent %lld channel %d: daughter %lld is not in the decay table", (long long)T.mc_id[e], j, (long long)id);
                all_d[(size_t)c * kBodies + k] = it->second;
                sum += T.mass[it->second];
            }
            if (!(sum < T.mass[e])) { H.n_closed++; continue; }
            run += T.branch_ratio[c];
            H.cum.push_back(run);
            H.nbody.push_back(n);
            for (int k = 0; k < kBodies; k++) H.dau.push_back(all_d[(size_t)c * kBodies + k]);
            H.ch0[(size_t)e + 1]++;
        }
    }
    // the decay graph over all channels: a cycle, the pending-stack need and the longest chain of decays (iterative depth-first search)
    std::vector<int32_t> need((size_t)T.n, 0), depth((size_t)T.n, 0);
    std::vector<uint8_t> state((size_t)T.n, 0);          // 0 new, 1 on the path, 2 done
    struct Frame { int32_t e; int64_t c; int k; };
    std::vector<Frame> path;
    for (int32_t root = 0; root < T.n; root++) {
        if (state[(size_t)root]) continue;
        path.push_back({root, first[(size_t)root], 0});
        state[(size_t)root] = 1;
        while (!path.empty()) {
            Frame &f = path.back();
            const int32_t e = f.e;
            const bool final_ = T.stable[e] || H.ch0[(size_t)e + 1] == H.ch0[(size_t)e];
            if (T.stable[e] || f.c >= first[(size_t)e + 1]) {
                if (final_) { need[(size_t)e] = 1; depth[(size_t)e] = 0; }
                state[(size_t)e] = 2;
                path.pop_back();
                continue;
            }
            const int n = all_n[(size_t)f.c];
            if (f.k >= n) { f.c++; f.k = 0; continue; }
            const int32_t d = all_d[(size_t)f.c * kBodies + f.k];
            if (state[(size_t)d] == 1)
                return set_error(IS3D_EINVAL, "the decay graph has a cycle through %lld and %lld", (long long)T.mc_id[e], (long long)T.mc_id[d]);
            if (state[(size_t)d] == 0) {
                state[(size_t)d] = 1;
                path.push_back({d, first[(size_t)d], 0});   // (f is stale from here: the loop re-reads path.back())
                continue;
            }
            if (!final_) {
                need[(size_t)e] = std::max(need[(size_t)e], need[(size_t)d] + (n - 1 - f.k));
                depth[(size_t)e] = std::max(depth[(size_t)e], depth[(size_t)d] + 1);
            }
            f.k++;
        }
    }
    for (int32_t e = 0; e < T.n; e++) {
        H.max_stack = std::max(H.max_stack, need[(size_t)e]);
        H.max_depth = std::max(H.max_depth, depth[(size_t)e]);
    }
    if (H.max_stack > kStack)
        return set_error(IS3D_EINVAL, "the decay table needs a pending stack of %d particles (at most %d)", H.max_stack, kStack);
    return IS3D_OK;
}

double ms_between(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Events()
    {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

}  // namespace

// The table as the kernels read it, resident on one device: the analysis (every table refusal) happens on the host before any device use,
// the upload once.  is3d_decay_particles builds one per call; a caller that keeps its primaries on the device keeps the table there too.
struct is3d_decay_mc_table {
    int device = -1;                  // where the arrays live; -1: analysed only
    int32_t n = 0, n_chosen = 0;
    McHostTable H;
    DevBuf<double> d_mass, d_width, d_cum;
    DevBuf<int32_t> d_stable, d_ch0, d_nbody, d_dau, d_chosen;
    McTable dev() const { return McTable{d_mass.p, d_width.p, d_stable.p, d_ch0.p, d_cum.p, d_nbody.p, d_dau.p}; }
};

namespace {

// the arrays of an analysed table to the current device
int table_upload(is3d_decay_mc_table &t, const is3d_decay_table &table)
{
    HIP_TRY(hipGetDevice(&t.device));
    HIP_TRY(t.d_mass.upload(table.mass, (size_t)table.n));
    HIP_TRY(t.d_width.upload(table.width, (size_t)table.n));
    HIP_TRY(t.d_stable.upload(table.stable, (size_t)table.n));
    HIP_TRY(t.d_ch0.upload(t.H.ch0));
    HIP_TRY(t.d_cum.upload(t.H.cum));
    HIP_TRY(t.d_nbody.upload(t.H.nbody));
    HIP_TRY(t.d_dau.upload(t.H.dau));
    HIP_TRY(t.d_chosen.upload(t.H.chosen_entry));
    return IS3D_OK;
}

// what both host-list entries check of their list before the table is looked at ...
int check_list_head(int32_t n_chosen, int64_t n_particles, const is3d_particle *particles)
{
    if (n_chosen < 1) return set_error(IS3D_EINVAL, "n_chosen = %d: the list's species index a chosen list of at least one", n_chosen);
    if (n_particles < 0 || n_particles > INT32_MAX) return set_error(IS3D_EINVAL, "n_particles = %lld: 0 .. 2^31 - 1", (long long)n_particles);
    if (n_particles > 0 && !particles) return set_error(IS3D_EINVAL, "particles is NULL");
    return IS3D_OK;
}
// ... and after it
int check_list_species(int32_t n_chosen, int64_t n_particles, const is3d_particle *particles)
{
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].species < 0 || particles[i].species >= n_chosen)
            return set_error(IS3D_EINVAL, "particle %lld: species %d outside the chosen list (%d)", (long long)i, particles[i].species, n_chosen);
    return IS3D_OK;
}

int no_device() { return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path"); }

}  // namespace

void is3d::decay_mc_table_stats(const is3d_decay_mc_table *t, is3d_decay_mc_stats *st)
{
    st->max_stack = t->H.max_stack;
    st->max_depth = t->H.max_depth;
    st->n_closed_channels = t->H.n_closed;
}
int32_t is3d::decay_mc_table_entries(const is3d_decay_mc_table *t) { return t->n; }
int32_t is3d::decay_mc_table_chosen(const is3d_decay_mc_table *t) { return t->n_chosen; }
int is3d::decay_mc_table_device(const is3d_decay_mc_table *t) { return t->device; }

namespace {
int table_analyse(is3d_decay_mc_table &t, const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id)
{
    if (!table || !chosen_mc_id) return set_error(IS3D_EINVAL, "table and chosen_mc_id are required");
    if (n_chosen < 1) return set_error(IS3D_EINVAL, "n_chosen = %d: the list's species index a chosen list of at least one", n_chosen);
    return analyse(*table, n_chosen, chosen_mc_id, t.H);
}
}  // namespace

int is3d::decay_mc_table_check(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id)
{
    is3d_decay_mc_table t;
    return table_analyse(t, table, n_chosen, chosen_mc_id);
}

extern "C" int is3d_decay_mc_table_create(is3d_decay_mc_table **out, const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                                          int32_t device)
{
    if (!out) return set_error(IS3D_EINVAL, "null argument");
    *out = nullptr;
    std::unique_ptr<is3d_decay_mc_table> t(new is3d_decay_mc_table);
    if (int rc = table_analyse(*t, table, n_chosen, chosen_mc_id)) return rc;
    t->n = table->n;
    t->n_chosen = n_chosen;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return no_device();
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    if (int rc = table_upload(*t, *table)) return rc;
    *out = t.release();
    return IS3D_OK;
}

extern "C" void is3d_decay_mc_table_destroy(is3d_decay_mc_table *t)
{
    if (!t) return;
    if (t->device >= 0) (void)hipSetDevice(t->device);
    delete t;
}

extern "C" int is3d_decay_particles(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id, const is3d_decay_mc_inputs *in,
                                    int64_t n_particles, const is3d_particle *particles, is3d_particle *out, int64_t *origin, int64_t capacity,
                                    int64_t *n_out, is3d_decay_mc_stats *stats)
{
    if (!table || !chosen_mc_id || !in || !n_out) return set_error(IS3D_EINVAL, "table, chosen_mc_id, in and n_out are required");
    if (int rc = check_list_head(n_chosen, n_particles, particles)) return rc;
    if (out && capacity < 0) return set_error(IS3D_EINVAL, "capacity = %lld", (long long)capacity);
    is3d_decay_mc_table tb;
    if (int rc = analyse(*table, n_chosen, chosen_mc_id, tb.H)) return rc;
    tb.n = table->n;
    tb.n_chosen = n_chosen;
    if (int rc = check_list_species(n_chosen, n_particles, particles)) return rc;
    is3d_decay_mc_stats st{};
    st.n_primaries = n_particles;
    is3d::decay_mc_table_stats(&tb, &st);
    *n_out = 0;
    if (n_particles == 0) {
        if (stats) *stats = st;
        return IS3D_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return no_device();
    if (in->device >= 0) HIP_TRY(hipSetDevice(in->device));
    // ---- upload ----
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<int32_t> d_counts;
    DevBuf<int64_t> d_offsets, d_origin;
    DevBuf<is3d_particle> d_in, d_out;
    DevBuf<unsigned long long> d_tally;
    DevBuf<unsigned char> d_tmp;
    if (int rc = table_upload(tb, *table)) return rc;
    HIP_TRY(d_in.upload(particles, (size_t)n_particles));
    HIP_TRY(d_counts.alloc((size_t)n_particles));
    HIP_TRY(d_offsets.alloc((size_t)n_particles + 1));
    HIP_TRY(d_tally.alloc(kTallies));
    HIP_TRY(hipMemset(d_tally.p, 0, kTallies * sizeof(unsigned long long)));
    const hipcub::TransformInputIterator<int64_t, Widen, const int32_t *> wide(d_counts.p, Widen());
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, wide, d_offsets.p, (int)n_particles, nullptr));
    HIP_TRY(d_tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
    Events ev;
    for (hipEvent_t &e : ev.e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipDeviceSynchronize());
    const auto t1 = std::chrono::steady_clock::now();
    // ---- count, scan ----
    McArgs a{};
    a.t = tb.dev();
    a.chosen_entry = tb.d_chosen.p;
    a.in = d_in.p;
    a.n = n_particles;
    a.first = in->first_particle;
    a.seed = in->seed;
    a.lifetime = in->lifetime;
    a.counts = d_counts.p;
    a.tally = d_tally.p;
    const dim3 grid((unsigned)((n_particles + kThreads - 1) / kThreads)), block(kThreads);
    HIP_TRY(hipEventRecord(ev.e[0], nullptr));
    hipLaunchKernelGGL(cf_decay_mc<false>, grid, block, 0, nullptr, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, wide, d_offsets.p, (int)n_particles, nullptr));
    HIP_TRY(hipEventRecord(ev.e[1], nullptr));
    int64_t last_offset = 0;
    int32_t last_count = 0;
    unsigned long long tally[kTallies];
    HIP_TRY(hipMemcpy(&last_offset, d_offsets.p + (n_particles - 1), sizeof last_offset, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&last_count, d_counts.p + (n_particles - 1), sizeof last_count, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tally, d_tally.p, sizeof tally, hipMemcpyDeviceToHost));
    if (tally[4]) return set_error(IS3D_EINVAL, "the pending stack of %d particles overflowed for %llu primaries", kStack, tally[4]);
    const int64_t total = last_offset + last_count;
    *n_out = total;
    st.n_decays = (int64_t)tally[0];
    st.n_stuck = (int64_t)tally[1];
    st.n_trials = (int64_t)tally[2];
    st.n_exhausted = (int64_t)tally[3];
    st.n_final = total;
    st.ms_h2d = std::chrono::duration<double, std::milli>(t1 - t0).count();
    st.ms_count = ms_between(ev.e[0], ev.e[1]);
    if (out && capacity < total) {
        if (stats) *stats = st;
        return set_error(IS3D_ENOMEM, "the list holds %lld particles, the decayed one needs %lld", (long long)capacity, (long long)total);
    }
    if (out && total > 0) {
        // ---- fill ----
        HIP_TRY(d_out.alloc((size_t)total));
        if (origin) HIP_TRY(d_origin.alloc((size_t)total));
        a.offsets = d_offsets.p;
        a.out = d_out.p;
        a.origin = origin ? d_origin.p : nullptr;
        HIP_TRY(hipEventRecord(ev.e[1], nullptr));
        hipLaunchKernelGGL(cf_decay_mc<true>, grid, block, 0, nullptr, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev.e[2], nullptr));
        HIP_TRY(hipEventSynchronize(ev.e[2]));
        st.ms_fill = ms_between(ev.e[1], ev.e[2]);
        const auto t2 = std::chrono::steady_clock::now();
        HIP_TRY(hipMemcpy(out, d_out.p, (size_t)total * sizeof(is3d_particle), hipMemcpyDeviceToHost));
        if (origin) HIP_TRY(hipMemcpy(origin, d_origin.p, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost));
        st.ms_d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    }
    if (stats) *stats = st;
    return IS3D_OK;
}

// ---- decayed and binned in one pass ----
int is3d::decay_mc_check_slots(int32_t n_entries, const int32_t *slot, int32_t n_slots, const is3d_sampler_test_bins *bins)
{
    if (n_slots < 1) return set_error(IS3D_EINVAL, "n_slots = %d: the decayed histograms hold at least one species", n_slots);
    if (!slot) return set_error(IS3D_EINVAL, "slot is NULL");
    for (int32_t e = 0; e < n_entries; e++)
        if (slot[e] < -1 || slot[e] >= n_slots) return set_error(IS3D_EINVAL, "slot[%d] = %d: -1 .. %d", e, slot[e], n_slots - 1);
    const SamplerHistLayout l = sampler_hist_layout(*bins, n_slots);
    if (bins->kernel_form == 2 && !decay_mc_bins_lds_fits(l))
        return set_error(IS3D_EINVAL, "kernel_form = 2: %lld histogram words do not fit the LDS", (long long)l.total);
    return IS3D_OK;
}

hipError_t is3d::decay_mc_bins_launch(const DecayMcBinRun &r, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle)
{
    if (n <= 0) return hipSuccess;
    const bool fits = decay_mc_bins_lds_fits(r.layout);
    const int form = r.bins.kernel_form;
    if (form == 2 && !fits) return hipErrorInvalidValue;
    const bool priv = form == 2 || (form == 0 && fits);
    McArgs a{};
    a.t = r.table->dev();
    a.chosen_entry = r.table->d_chosen.p;
    a.in = primaries_dev;
    a.n = n;
    a.first = first_particle;
    a.seed = r.seed;
    a.lifetime = r.lifetime;
    McBinArgs b{r.bins, r.widths, r.layout, r.n_slots, r.n_events, r.slot_dev, r.block_dev, r.block_dev + r.layout.total,
                r.block_dev + r.layout.total + r.n_events};
    const int64_t trips = (n + kBinThreads - 1) / kBinThreads;
    if (priv)
        hipLaunchKernelGGL(cf_decay_mc_bins<true>, dim3((unsigned)std::min<int64_t>(trips, kBinPrivateBlocks)), dim3(kBinThreads),
                           (size_t)r.layout.total * sizeof(unsigned long long), nullptr, a, b);
    else
        hipLaunchKernelGGL(cf_decay_mc_bins<false>, dim3((unsigned)trips), dim3(kBinThreads), 0, nullptr, a, b);
    return hipGetLastError();
}

int is3d::decay_mc_bins_tallies(const unsigned long long *tally, is3d_decay_mc_stats *st)
{
    st->n_decays = (int64_t)tally[0];
    st->n_stuck = (int64_t)tally[1];
    st->n_trials = (int64_t)tally[2];
    st->n_exhausted = (int64_t)tally[3];
    st->n_final = (int64_t)tally[5];
    if (tally[4]) return set_error(IS3D_EINVAL, "the pending stack of %d particles overflowed for %llu primaries", kStack, tally[4]);
    return IS3D_OK;
}

extern "C" int is3d_decay_particles_binned(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                                           const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                                           const int32_t *slot, int32_t n_slots, const is3d_sampler_test_bins *bins, int32_t n_events,
                                           const is3d_sampler_hist *hist, int64_t *n_final, int64_t *n_unbinned, is3d_decay_mc_stats *stats)
{
    if (!table || !chosen_mc_id || !in || !n_final || !n_unbinned)
        return set_error(IS3D_EINVAL, "table, chosen_mc_id, in, n_final and n_unbinned are required");
    *n_final = *n_unbinned = 0;
    if (int rc = check_list_head(n_chosen, n_particles, particles)) return rc;
    is3d_decay_mc_table tb;
    if (int rc = analyse(*table, n_chosen, chosen_mc_id, tb.H)) return rc;
    tb.n = table->n;
    tb.n_chosen = n_chosen;
    if (int rc = check_list_species(n_chosen, n_particles, particles)) return rc;
    if (n_slots < 1) return set_error(IS3D_EINVAL, "n_slots = %d: the decayed histograms hold at least one species", n_slots);
    if (int rc = is3d::sampler_check_bin_args(bins, hist, n_events, n_slots)) return rc;
    if (int rc = is3d::decay_mc_check_slots(table->n, slot, n_slots, bins)) return rc;
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].event < 0 || particles[i].event >= n_events)
            return set_error(IS3D_EINVAL, "particle %lld: event %d outside the %d events", (long long)i, particles[i].event, n_events);
    is3d_decay_mc_stats st{};
    st.n_primaries = n_particles;
    is3d::decay_mc_table_stats(&tb, &st);
    const is3d::SamplerHistLayout l = is3d::sampler_hist_layout(*bins, n_slots);
    DevBuf<unsigned char> d_block;
    if (n_particles == 0) {
        if (int rc = is3d::sampler_hist_begin(d_block, hist, l, n_events, 0, false)) return rc;
        if (stats) *stats = st;
        return IS3D_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return no_device();
    if (in->device >= 0) HIP_TRY(hipSetDevice(in->device));
    // ---- upload: the table, the primaries, the slot map; the block of histograms, yields and tallies zeroed ----
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<is3d_particle> d_in;
    DevBuf<int32_t> d_slot;
    if (int rc = table_upload(tb, *table)) return rc;
    HIP_TRY(d_in.upload(particles, (size_t)n_particles));
    HIP_TRY(d_slot.upload(slot, (size_t)table->n));
    if (int rc = is3d::sampler_hist_begin(d_block, hist, l, n_events, kBinTallies, true)) return rc;
    Events ev;
    for (int k = 0; k < 2; k++) HIP_TRY(hipEventCreate(&ev.e[k]));
    HIP_TRY(hipDeviceSynchronize());
    const auto t1 = std::chrono::steady_clock::now();
    // ---- the one pass ----
    const is3d::DecayMcBinRun run{&tb,   d_slot.p, n_slots, n_events, in->seed, in->lifetime, *bins, is3d::sampler_bin_widths(*bins),
                                  l,     d_block.as<unsigned long long>()};
    HIP_TRY(hipEventRecord(ev.e[0], nullptr));
    HIP_TRY(is3d::decay_mc_bins_launch(run, d_in.p, n_particles, in->first_particle));
    HIP_TRY(hipEventRecord(ev.e[1], nullptr));
    HIP_TRY(hipEventSynchronize(ev.e[1]));
    st.ms_h2d = std::chrono::duration<double, std::milli>(t1 - t0).count();
    st.ms_bin = ms_between(ev.e[0], ev.e[1]);
    const auto t2 = std::chrono::steady_clock::now();
    unsigned long long tally[kBinTallies];
    HIP_TRY(hipMemcpy(tally, run.block_dev + l.total + n_events, sizeof tally, hipMemcpyDeviceToHost));
    if (int rc = is3d::sampler_hist_end(d_block, hist, l, n_events)) return rc;
    st.ms_d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    const int rc = is3d::decay_mc_bins_tallies(tally, &st);
    int64_t binned = 0;
    for (int32_t e = 0; e < n_events; e++) binned += hist->yield[e];
    *n_final = st.n_final;
    *n_unbinned = st.n_final - binned;
    if (stats) *stats = st;
    if (rc) return rc;
    return is3d::sampler_hist_check_counts(hist, l);
}

// ---- decayed into flow records in one pass ----
hipError_t is3d::decay_mc_flow_launch(const DecayMcFlowRun &r, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle)
{
    if (n <= 0) return hipSuccess;
    const bool diff = r.n_pT > 0;
    const int n_keys = diff ? r.n_slots * r.n_pT : r.n_slots;
    const int window = diff ? flow_diff_window_events(r.n_events, r.n_slots, r.n_pT, kBinTallies) : flow_window_events(r.n_events, r.n_slots, kBinTallies);
    const int form = r.cuts.kernel_form;
    if (form == 2 && window < 1) return hipErrorInvalidValue;
    const bool priv = form == 2 || (form == 0 && window >= 1);
    McArgs a{};
    a.t = r.table->dev();
    a.chosen_entry = r.table->d_chosen.p;
    a.in = primaries_dev;
    a.n = n;
    a.first = first_particle;
    a.seed = r.seed;
    a.lifetime = r.lifetime;
    const int64_t words = (int64_t)r.n_events * n_keys * kFlowRecordWords;
    const McFlowArgs f{r.cuts, r.thresholds, r.n_slots, r.n_events, window, r.slot_dev, r.block_dev, r.block_dev + words, r.n_pT, r.edges_dev};
    const size_t lds = priv ? (size_t)window * n_keys * kFlowRecordWords * sizeof(unsigned long long) : 0;
    const int64_t trips = (n + kBinThreads - 1) / kBinThreads;
    const int64_t blocks0 = priv ? std::min<int64_t>(trips, kBinPrivateBlocks) : trips;
    const int64_t slice = ((n + blocks0 - 1) / blocks0 + kBinThreads - 1) / kBinThreads * kBinThreads;
    const unsigned blocks = (unsigned)((n + slice - 1) / slice);
    if (diff) {
        if (priv) hipLaunchKernelGGL((cf_decay_mc_flow<true, true>), dim3(blocks), dim3(kBinThreads), lds, nullptr, a, f, slice);
        else hipLaunchKernelGGL((cf_decay_mc_flow<false, true>), dim3(blocks), dim3(kBinThreads), 0, nullptr, a, f, slice);
    } else {
        if (priv) hipLaunchKernelGGL((cf_decay_mc_flow<true, false>), dim3(blocks), dim3(kBinThreads), lds, nullptr, a, f, slice);
        else hipLaunchKernelGGL((cf_decay_mc_flow<false, false>), dim3(blocks), dim3(kBinThreads), 0, nullptr, a, f, slice);
    }
    return hipGetLastError();
}

// the one body of is3d_decay_particles_flow (diff == NULL: records) and is3d_decay_particles_flow_diff (diff: the differential records on the
// table pT_edges[n_pT + 1], which are flow records of n_slots * n_pT slots)
static int decay_particles_flow(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id, const is3d_decay_mc_inputs *in,
                                int64_t n_particles, const is3d_particle *particles, const int32_t *slot, int32_t n_slots, const is3d_flow_cuts *cuts,
                                bool differential, int32_t n_pT, const double *pT_edges, int32_t n_events, const is3d_flow_records *plain,
                                const is3d_flow_diff_records *diff, int64_t *n_final, int64_t *n_unbinned, is3d_decay_mc_stats *stats)
{
    if (!table || !chosen_mc_id || !in || !n_final || !n_unbinned)
        return set_error(IS3D_EINVAL, "table, chosen_mc_id, in, n_final and n_unbinned are required");
    *n_final = *n_unbinned = 0;
    if (int rc = check_list_head(n_chosen, n_particles, particles)) return rc;
    is3d_decay_mc_table tb;
    if (int rc = analyse(*table, n_chosen, chosen_mc_id, tb.H)) return rc;
    tb.n = table->n;
    tb.n_chosen = n_chosen;
    if (int rc = check_list_species(n_chosen, n_particles, particles)) return rc;
    if (table->n < 1) return set_error(IS3D_EINVAL, "decay table: n = %d", table->n);
    if (int rc = differential ? is3d::flow_diff_check_args(cuts, n_pT, pT_edges, n_events, n_slots, slot, table->n, diff, kBinTallies)
                              : is3d::flow_check_args(cuts, n_events, n_slots, slot, table->n, plain, kBinTallies))
        return rc;
    const is3d_flow_records view = differential ? is3d::flow_diff_view(*diff) : *plain;
    const is3d_flow_records *records = &view;
    if (differential) n_slots *= n_pT;                 // from here on: the slots of the block
    else n_pT = 0;
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].event < 0 || particles[i].event >= n_events)
            return set_error(IS3D_EINVAL, "particle %lld: event %d outside the %d events", (long long)i, particles[i].event, n_events);
    is3d_decay_mc_stats st{};
    st.n_primaries = n_particles;
    is3d::decay_mc_table_stats(&tb, &st);
    if (n_particles == 0) {
        is3d::flow_records_zero(records, n_events, n_slots);
        if (stats) *stats = st;
        return IS3D_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return no_device();
    is3d::flow_records_zero(records, n_events, n_slots);
    if (in->device >= 0) HIP_TRY(hipSetDevice(in->device));
    // ---- upload: the table, the primaries, the slot map; the block of records and tallies zeroed ----
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<is3d_particle> d_in;
    DevBuf<int32_t> d_slot;
    DevBuf<unsigned long long> d_block;
    DevBuf<double> d_edges;
    const size_t words = (size_t)n_events * n_slots * is3d::kFlowRecordWords;
    if (int rc = table_upload(tb, *table)) return rc;
    HIP_TRY(d_in.upload(particles, (size_t)n_particles));
    HIP_TRY(d_slot.upload(slot, (size_t)table->n));
    if (differential) HIP_TRY(d_edges.upload(pT_edges, (size_t)n_pT + 1));
    HIP_TRY(d_block.alloc(words + kBinTallies));
    HIP_TRY(hipMemsetAsync(d_block.p, 0, (words + kBinTallies) * sizeof(unsigned long long), nullptr));
    Events ev;
    for (int k = 0; k < 2; k++) HIP_TRY(hipEventCreate(&ev.e[k]));
    HIP_TRY(hipDeviceSynchronize());
    const auto t1 = std::chrono::steady_clock::now();
    // ---- the one pass ----
    const is3d::DecayMcFlowRun run{&tb, d_slot.p, differential ? n_slots / n_pT : n_slots, n_events, in->seed, in->lifetime, *cuts,
                                   is3d::flow_thresholds(*cuts), d_block.p, n_pT, d_edges.p};
    HIP_TRY(hipEventRecord(ev.e[0], nullptr));
    HIP_TRY(is3d::decay_mc_flow_launch(run, d_in.p, n_particles, in->first_particle));
    HIP_TRY(hipEventRecord(ev.e[1], nullptr));
    HIP_TRY(hipEventSynchronize(ev.e[1]));
    st.ms_h2d = std::chrono::duration<double, std::milli>(t1 - t0).count();
    st.ms_bin = ms_between(ev.e[0], ev.e[1]);
    const auto t2 = std::chrono::steady_clock::now();
    std::vector<int64_t> h(words + kBinTallies);
    HIP_TRY(hipMemcpy(h.data(), d_block.p, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    st.ms_d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    is3d::flow_records_scatter(h.data(), records, n_events, n_slots);
    const int rc = is3d::decay_mc_bins_tallies((const unsigned long long *)(h.data() + words), &st);
    int64_t kept = 0;
    for (size_t j = 0; j < (size_t)n_events * n_slots; j++) kept += records->M[j * is3d::kFlowRegions];
    *n_final = st.n_final;
    *n_unbinned = st.n_final - kept;
    if (stats) *stats = st;
    if (rc) return rc;
    return is3d::flow_records_check(records, n_events, n_slots);
}

extern "C" int is3d_decay_particles_flow(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                                         const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                                         const int32_t *slot, int32_t n_slots, const is3d_flow_cuts *cuts, int32_t n_events,
                                         const is3d_flow_records *records, int64_t *n_final, int64_t *n_unbinned, is3d_decay_mc_stats *stats)
{
    return decay_particles_flow(table, n_chosen, chosen_mc_id, in, n_particles, particles, slot, n_slots, cuts, false, 0, nullptr, n_events, records,
                                nullptr, n_final, n_unbinned, stats);
}

extern "C" int is3d_decay_particles_flow_diff(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                                              const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                                              const int32_t *slot, int32_t n_slots, const is3d_flow_cuts *cuts, int32_t n_pT,
                                              const double *pT_edges, int32_t n_events, const is3d_flow_diff_records *records, int64_t *n_final,
                                              int64_t *n_unbinned, is3d_decay_mc_stats *stats)
{
    return decay_particles_flow(table, n_chosen, chosen_mc_id, in, n_particles, particles, slot, n_slots, cuts, true, n_pT, pT_edges, n_events,
                                nullptr, records, n_final, n_unbinned, stats);
}

// ---- decayed into pair histograms: one decay pass into the occupancies, then cf_pair_correlate ----
hipError_t is3d::decay_mc_pairs_launch(const DecayMcPairRun &r, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle)
{
    if (n <= 0) return hipSuccess;
    McArgs a{};
    a.t = r.table->dev();
    a.chosen_entry = r.table->d_chosen.p;
    a.in = primaries_dev;
    a.n = n;
    a.first = first_particle;
    a.seed = r.seed;
    a.lifetime = r.lifetime;
    const McPairArgs f{r.bins, r.tables, r.n_slots, r.n_events, r.slot_dev, r.occ_dev, r.tally_dev};
    const int64_t trips = (n + kBinThreads - 1) / kBinThreads;
    hipLaunchKernelGGL(cf_decay_mc_pairs, dim3((unsigned)std::min<int64_t>(trips, (int64_t)1 << 20)), dim3(kBinThreads), 0, nullptr, a, f);
    return hipGetLastError();
}

extern "C" int is3d_decay_particles_pairs(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                                          const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                                          const int32_t *slot, int32_t n_slots, const is3d_pair_bins *bins, int32_t n_events,
                                          const is3d_pair_hist *hist, int64_t *n_final, int64_t *n_unbinned, is3d_decay_mc_stats *stats)
{
    if (!table || !chosen_mc_id || !in || !n_final || !n_unbinned)
        return set_error(IS3D_EINVAL, "table, chosen_mc_id, in, n_final and n_unbinned are required");
    *n_final = *n_unbinned = 0;
    if (int rc = check_list_head(n_chosen, n_particles, particles)) return rc;
    is3d_decay_mc_table tb;
    if (int rc = analyse(*table, n_chosen, chosen_mc_id, tb.H)) return rc;
    tb.n = table->n;
    tb.n_chosen = n_chosen;
    if (int rc = check_list_species(n_chosen, n_particles, particles)) return rc;
    if (table->n < 1) return set_error(IS3D_EINVAL, "decay table: n = %d", table->n);
    if (int rc = is3d::pair_check_args(bins, n_events, n_slots, slot, table->n, hist)) return rc;
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].event < 0 || particles[i].event >= n_events)
            return set_error(IS3D_EINVAL, "particle %lld: event %d outside the %d events", (long long)i, particles[i].event, n_events);
    is3d_decay_mc_stats st{};
    st.n_primaries = n_particles;
    is3d::decay_mc_table_stats(&tb, &st);
    if (n_particles == 0) {
        is3d::pair_hist_zero(*bins, hist, n_events, n_slots);
        if (stats) *stats = st;
        return IS3D_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return no_device();
    is3d::pair_hist_zero(*bins, hist, n_events, n_slots);
    if (in->device >= 0) HIP_TRY(hipSetDevice(in->device));
    // ---- upload: the table, the primaries, the slot map; the tallies and the occupancy block zeroed ----
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<is3d_particle> d_in;
    DevBuf<int32_t> d_slot;
    DevBuf<unsigned char> d_block, d_out;
    constexpr size_t head = kBinTallies * sizeof(unsigned long long);
    const size_t out_words = is3d::pair_out_words(*bins, n_events, n_slots);
    if (int rc = table_upload(tb, *table)) return rc;
    HIP_TRY(d_in.upload(particles, (size_t)n_particles));
    HIP_TRY(d_slot.upload(slot, (size_t)table->n));
    if (int rc = is3d::pair_occ_begin(d_block, head, is3d::pair_occ_words(*bins, n_events, n_slots))) return rc;
    HIP_TRY(d_out.alloc(out_words * sizeof(int64_t)));
    Events ev;
    for (int k = 0; k < 2; k++) HIP_TRY(hipEventCreate(&ev.e[k]));
    HIP_TRY(hipDeviceSynchronize());
    const auto t1 = std::chrono::steady_clock::now();
    // ---- the decay pass, then the correlation of the occupancies ----
    const is3d::DecayMcPairRun run{&tb, d_slot.p, n_slots, n_events, in->seed, in->lifetime, *bins, is3d::pair_tables(*bins),
                                   d_block.as<unsigned long long>(), (unsigned *)(d_block.p + head)};
    HIP_TRY(hipEventRecord(ev.e[0], nullptr));
    HIP_TRY(is3d::decay_mc_pairs_launch(run, d_in.p, n_particles, in->first_particle));
    HIP_TRY(hipEventRecord(ev.e[1], nullptr));
    HIP_TRY(is3d::pair_correlate_launch(*bins, n_events, n_slots, run.occ_dev, d_out.as<unsigned long long>()));
    HIP_TRY(hipEventSynchronize(ev.e[1]));
    st.ms_h2d = std::chrono::duration<double, std::milli>(t1 - t0).count();
    st.ms_bin = ms_between(ev.e[0], ev.e[1]);
    const auto t2 = std::chrono::steady_clock::now();
    std::vector<int64_t> h(out_words);
    unsigned long long tally[kBinTallies];
    HIP_TRY(hipMemcpy(h.data(), d_out.p, out_words * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tally, d_block.p, sizeof tally, hipMemcpyDeviceToHost));
    st.ms_d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    is3d::pair_hist_scatter(*bins, h.data(), hist, n_events, n_slots);
    const int rc = is3d::decay_mc_bins_tallies(tally, &st);
    int64_t kept = 0;
    for (size_t j = 0; j < (size_t)n_events * n_slots; j++) kept += hist->M[j];
    *n_final = st.n_final;
    *n_unbinned = st.n_final - kept;
    if (stats) *stats = st;
    if (rc) return rc;
    return is3d::pair_hist_check(hist, n_events, n_slots);
}

// ---- decayed into HBT histograms: the decay loop twice (count, fill) into compact records, then cf_hbt_pairs ----
hipError_t is3d::decay_mc_hbt_launch(const DecayMcHbtRun &r, const HbtRun &run, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle,
                                     bool fill)
{
    if (n <= 0) return hipSuccess;
    McArgs a{};
    a.t = r.table->dev();
    a.chosen_entry = r.table->d_chosen.p;
    a.in = primaries_dev;
    a.n = n;
    a.first = first_particle;
    a.seed = r.seed;
    a.lifetime = r.lifetime;
    const McHbtArgs f{is3d::hbt_select_args(run, fill), r.slot_dev, r.tally_dev};
    const int64_t trips = (n + kBinThreads - 1) / kBinThreads;
    const dim3 grid((unsigned)std::min<int64_t>(trips, (int64_t)1 << 20));
    if (fill)
        hipLaunchKernelGGL(cf_decay_mc_hbt<true>, grid, dim3(kBinThreads), 0, nullptr, a, f);
    else
        hipLaunchKernelGGL(cf_decay_mc_hbt<false>, grid, dim3(kBinThreads), 0, nullptr, a, f);
    return hipGetLastError();
}

int is3d::decay_mc_hbt_batch(const DecayMcHbtRun &r, HbtRun &run, const is3d_particle *primaries_dev, int64_t n, int64_t first_particle)
{
    if (n <= 0) return IS3D_OK;
    if (int rc = run.batch_begin()) return rc;
    HIP_TRY(decay_mc_hbt_launch(r, run, primaries_dev, n, first_particle, false));
    if (int rc = run.batch_plan()) return rc;
    HIP_TRY(decay_mc_hbt_launch(r, run, primaries_dev, n, first_particle, true));
    return run.batch_pairs();
}

extern "C" int is3d_decay_particles_hbt(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                                        const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                                        const int32_t *slot, int32_t n_slots, const is3d_hbt_bins *bins, int32_t n_events,
                                        const is3d_hbt_hist *hist, int64_t *n_final, int64_t *n_unbinned, is3d_decay_mc_stats *stats)
{
    if (!table || !chosen_mc_id || !in || !n_final || !n_unbinned)
        return set_error(IS3D_EINVAL, "table, chosen_mc_id, in, n_final and n_unbinned are required");
    *n_final = *n_unbinned = 0;
    if (int rc = check_list_head(n_chosen, n_particles, particles)) return rc;
    is3d_decay_mc_table tb;
    if (int rc = analyse(*table, n_chosen, chosen_mc_id, tb.H)) return rc;
    tb.n = table->n;
    tb.n_chosen = n_chosen;
    if (int rc = check_list_species(n_chosen, n_particles, particles)) return rc;
    if (table->n < 1) return set_error(IS3D_EINVAL, "decay table: n = %d", table->n);
    if (int rc = is3d::hbt_check_args(bins, n_events, n_slots, slot, table->n, hist, true)) return rc;
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].event < 0 || particles[i].event >= n_events)
            return set_error(IS3D_EINVAL, "particle %lld: event %d outside the %d events", (long long)i, particles[i].event, n_events);
    is3d_decay_mc_stats st{};
    st.n_primaries = n_particles;
    is3d::decay_mc_table_stats(&tb, &st);
    if (n_particles == 0) {
        is3d::hbt_hist_zero(*bins, hist, n_events, n_slots);
        if (stats) *stats = st;
        return IS3D_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return no_device();
    is3d::hbt_hist_zero(*bins, hist, n_events, n_slots);
    if (in->device >= 0) HIP_TRY(hipSetDevice(in->device));
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<is3d_particle> d_in;
    DevBuf<int32_t> d_slot;
    DevBuf<unsigned long long> d_tally;
    is3d::HbtRun run;
    if (int rc = table_upload(tb, *table)) return rc;
    HIP_TRY(d_in.upload(particles, (size_t)n_particles));
    HIP_TRY(d_slot.upload(slot, (size_t)table->n));
    HIP_TRY(d_tally.alloc(kBinTallies));
    HIP_TRY(hipMemsetAsync(d_tally.p, 0, kBinTallies * sizeof(unsigned long long), nullptr));
    if (int rc = run.begin(*bins, n_events, n_slots)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const auto t1 = std::chrono::steady_clock::now();
    const is3d::DecayMcHbtRun drun{&tb, d_slot.p, in->seed, in->lifetime, d_tally.p};
    if (int rc = is3d::decay_mc_hbt_batch(drun, run, d_in.p, n_particles, in->first_particle)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const auto t2 = std::chrono::steady_clock::now();
    st.ms_h2d = std::chrono::duration<double, std::milli>(t1 - t0).count();
    st.ms_bin = std::chrono::duration<double, std::milli>(t2 - t1).count();
    unsigned long long tally[kBinTallies];
    HIP_TRY(hipMemcpy(tally, d_tally.p, sizeof tally, hipMemcpyDeviceToHost));
    const int rc_h = run.finish(hist);
    st.ms_d2h = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    const int rc = is3d::decay_mc_bins_tallies(tally, &st);
    int64_t kept = 0;
    for (size_t j = 0; j < (size_t)n_events * n_slots; j++) kept += hist->M[j];
    *n_final = st.n_final;
    *n_unbinned = st.n_final - kept;
    if (stats) *stats = st;
    return rc ? rc : rc_h;
}
