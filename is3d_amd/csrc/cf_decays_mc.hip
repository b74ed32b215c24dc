// cf_decays_mc.hip -- Monte Carlo decays of sampled hadrons to stable particles on the device (is3d_decay_particles; the reference has no
// counterpart: include/is3d_amd.h is the definition, DESIGN.md section 3p the account).
//
// Thread <-> primary.  A primary's whole decay tree is walked depth-first by one thread and draws from ONE Philox stream
// (stream 5, keyed by the primary's global index), so the count pass and the fill pass replay the same tree:
//   cf_decay_mc<false>  counts the final particles of every primary (int32) and adds the run-wide tallies
//   hipCUB exclusive scan of the counts (as the samplers')
//   cf_decay_mc<true>   the same loop body, every final particle stored at the primary's offset
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
#include <unordered_map>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_host.h"
#include "cf_sampler_common.h"
#include "errors.h"

namespace {

using is3d::DevBuf;
using is3d::kHbarC;
using is3d::Rng;
using is3d::set_error;

constexpr int kBodies = IS3D_DECAY_MC_MAX_BODIES, kStack = IS3D_DECAY_MC_MAX_STACK, kTrials = IS3D_DECAY_MC_MAX_TRIALS;
constexpr int kThreads = 128;
constexpr int kTallies = 5;   // decays, stuck, trials, exhausted, primaries whose stack would have overflowed (never: the host proves it)

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

// the decay tree of primary i; returns its number of final particles
template <bool KEEP>
__device__ __forceinline__ int decay_tree(const McArgs &a, int64_t i, unsigned long long (&tally)[kTallies])
{
    const is3d_particle q = a.in[i];
    const uint64_t gi = (uint64_t)(a.first + i);
    Rng g;
    g.init(a.seed, 5, (uint32_t)gi, (uint32_t)(gi >> 32));
    Pending stack[kStack];
    int sp = 0, nfinal = 0;
    Pending c;
    c.E = q.E; c.px = q.px; c.py = q.py; c.pz = q.pz; c.t = q.t; c.x = q.x; c.y = q.y; c.z = q.z; c.tau = q.tau; c.eta = q.eta;
    c.e = a.chosen_entry[q.species];
    const int64_t slot0 = KEEP ? a.offsets[i] : 0;
    const int counted = KEEP ? a.counts[i] : 0;
    for (;;) {
        const int c0 = a.t.ch0[c.e], c1 = a.t.ch0[c.e + 1];
        const bool stable = a.t.stable[c.e] != 0;
        if (stable || c0 == c1) {                       // final: stable, or stuck without an open channel
            if (!stable) tally[1]++;
            if (KEEP && nfinal < counted) {
                is3d_particle o;
                o.cell = q.cell; o.event = q.event; o.species = c.e;
                o.tau = c.tau; o.x = c.x; o.y = c.y; o.eta = c.eta; o.t = c.t; o.z = c.z;
                o.E = c.E; o.px = c.px; o.py = c.py; o.pz = c.pz;
                a.out[slot0 + nfinal] = o;
                if (a.origin) a.origin[slot0 + nfinal] = i;
            }
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
        const int nf = decay_tree<KEEP>(a, i, tally);
        if (!KEEP) a.counts[i] = nf;
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

extern "C" int is3d_decay_particles(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id, const is3d_decay_mc_inputs *in,
                                    int64_t n_particles, const is3d_particle *particles, is3d_particle *out, int64_t *origin, int64_t capacity,
                                    int64_t *n_out, is3d_decay_mc_stats *stats)
{
    if (!table || !chosen_mc_id || !in || !n_out) return set_error(IS3D_EINVAL, "table, chosen_mc_id, in and n_out are required");
    if (n_chosen < 1) return set_error(IS3D_EINVAL, "n_chosen = %d: the list's species index a chosen list of at least one", n_chosen);
    if (n_particles < 0 || n_particles > INT32_MAX) return set_error(IS3D_EINVAL, "n_particles = %lld: 0 .. 2^31 - 1", (long long)n_particles);
    if (n_particles > 0 && !particles) return set_error(IS3D_EINVAL, "particles is NULL");
    if (out && capacity < 0) return set_error(IS3D_EINVAL, "capacity = %lld", (long long)capacity);
    McHostTable H;
    if (int rc = analyse(*table, n_chosen, chosen_mc_id, H)) return rc;
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].species < 0 || particles[i].species >= n_chosen)
            return set_error(IS3D_EINVAL, "particle %lld: species %d outside the chosen list (%d)", (long long)i, particles[i].species, n_chosen);
    is3d_decay_mc_stats st{};
    st.n_primaries = n_particles;
    st.max_stack = H.max_stack;
    st.max_depth = H.max_depth;
    st.n_closed_channels = H.n_closed;
    *n_out = 0;
    if (n_particles == 0) {
        if (stats) *stats = st;
        return IS3D_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    if (in->device >= 0) HIP_TRY(hipSetDevice(in->device));
    // ---- upload ----
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<double> d_mass, d_width, d_cum;
    DevBuf<int32_t> d_stable, d_ch0, d_nbody, d_dau, d_chosen, d_counts;
    DevBuf<int64_t> d_offsets, d_origin;
    DevBuf<is3d_particle> d_in, d_out;
    DevBuf<unsigned long long> d_tally;
    DevBuf<unsigned char> d_tmp;
    HIP_TRY(d_mass.upload(table->mass, (size_t)table->n));
    HIP_TRY(d_width.upload(table->width, (size_t)table->n));
    HIP_TRY(d_stable.upload(table->stable, (size_t)table->n));
    HIP_TRY(d_ch0.upload(H.ch0));
    HIP_TRY(d_cum.upload(H.cum));
    HIP_TRY(d_nbody.upload(H.nbody));
    HIP_TRY(d_dau.upload(H.dau));
    HIP_TRY(d_chosen.upload(H.chosen_entry));
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
    a.t = McTable{d_mass.p, d_width.p, d_stable.p, d_ch0.p, d_cum.p, d_nbody.p, d_dau.p};
    a.chosen_entry = d_chosen.p;
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
