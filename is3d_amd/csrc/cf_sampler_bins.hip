// cf_sampler_bins.hip -- the test_sampler = 1 distributions binned on the device (gfx950), one thread per particle of an event batch.
//
// The per-particle rule is cf_sampler_bins.h, the one the host writer uses.  Everything that is added is a 64-bit integer: counts, the
// per-event yields and the harmonic sums in fixed point (llrint(term * 2^32)), so the histograms do not depend on the order in which the
// adds arrive -- launch geometry, event batching and cell sharding give the same bits.  No float atomics.
//
// Two forms, chosen by sampler_bins_launch:
//   workgroup-private: the whole histogram block (counts + harmonic sums) lives in LDS, every workgroup walks a grid-stride slice of the
//       batch with ds_add_u64 and flushes its non-zero words once with global 64-bit adds.  pi/K/p at the shipped bins: 43 KB.
//   global: every add is a no-return global 64-bit atomic (hundreds of species: the block does not fit the LDS, and the adds spread over
//       as many addresses).
// Per-event yields: the list is ordered by event, so the lanes of a wave see runs of equal events; the first lane of a run adds the
// run's length -- one add per distinct event per wave instead of one per particle on one address.  (A list that is not ordered is still
// counted correctly, with more adds.)
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>

#include "cf_sampler_bins.h"

namespace is3d {
namespace {

constexpr int kBinThreads = 256;
constexpr int kBinPrivateBlocks = 512;                   // workgroup-private form: at most this many flushes
constexpr int64_t kBinPrivateParticles = 4096;           // ... and at least this many particles per workgroup
constexpr int64_t kBinLdsWords = 65536 / sizeof(unsigned long long);

struct BinArgs {
    is3d_sampler_test_bins b;
    SamplerBinWidths w;
    SamplerHistLayout l;
    int n_species, n_events;
};

template <bool PRIVATE>
__global__ void __launch_bounds__(kBinThreads)
cf_sampler_bins(BinArgs a, const is3d_particle *__restrict__ particles, int64_t n, unsigned long long *__restrict__ hist,
                unsigned long long *__restrict__ yield)
{
    extern __shared__ unsigned long long priv[];
    if (PRIVATE) {
        for (int64_t j = threadIdx.x; j < a.l.total; j += kBinThreads) priv[j] = 0ULL;
        __syncthreads();
    }
    unsigned long long *h = PRIVATE ? priv : hist;
    const int lane = threadIdx.x & 63;
    // the trip count is the same for every thread of the workgroup: the wave operations below see whole waves
    for (int64_t i0 = (int64_t)blockIdx.x * kBinThreads; i0 < n; i0 += (int64_t)gridDim.x * kBinThreads) {
        const int64_t i = i0 + threadIdx.x;
        is3d_particle q;
        bool ok = false;
        int ev = INT_MAX;                                  // lanes past the end, or with an index outside the arrays: no add at all
        if (i < n) {
            q = particles[i];
            ok = q.species >= 0 && q.species < a.n_species && q.event >= 0 && q.event < a.n_events;
            if (ok) ev = q.event;
        }
        const int prev = __shfl_up(ev, 1);
        const bool lead = lane == 0 || prev != ev;
        const unsigned long long leaders = __ballot(lead);
        if (lead && ok) {
            const unsigned long long above = lane == 63 ? 0ULL : (leaders >> (lane + 1)) << (lane + 1);
            const int next = above ? __ffsll((long long)above) - 1 : 64;
            atomicAdd(&yield[ev], (unsigned long long)(next - lane));
        }
        if (!ok) continue;
        const SamplerBinIndex k = sampler_bin_particle(a.b, a.w, q);
        sampler_bin_add(a.b, a.l, a.n_species, k, q.species, h);
    }
    if (PRIVATE) {
        __syncthreads();
        for (int64_t j = threadIdx.x; j < a.l.total; j += kBinThreads) {
            const unsigned long long v = priv[j];
            if (v) atomicAdd(&hist[j], v);
        }
    }
}

}  // namespace

bool sampler_bins_lds_fits(const SamplerHistLayout &l) { return l.total <= kBinLdsWords; }

hipError_t sampler_bins_launch(const is3d_sampler_test_bins &b, const SamplerBinWidths &w, const SamplerHistLayout &l, int n_species, int n_events,
                               const is3d_particle *particles_dev, int64_t n, unsigned long long *hist_dev, unsigned long long *yield_dev,
                               int form)
{
    if (n <= 0) return hipSuccess;
    const bool fits = sampler_bins_lds_fits(l);
    if (form == 2 && !fits) return hipErrorInvalidValue;
    const bool priv = form == 2 || (form == 0 && fits);
    const BinArgs a{b, w, l, n_species, n_events};
    if (priv) {
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(kBinPrivateBlocks, (n + kBinPrivateParticles - 1) / kBinPrivateParticles));
        hipLaunchKernelGGL(cf_sampler_bins<true>, dim3((unsigned)blocks), dim3(kBinThreads), (size_t)l.total * sizeof(unsigned long long), nullptr, a,
                           particles_dev, n, hist_dev, yield_dev);
    } else {
        const int64_t blocks = std::min<int64_t>((int64_t)1 << 20, (n + kBinThreads - 1) / kBinThreads);
        hipLaunchKernelGGL(cf_sampler_bins<false>, dim3((unsigned)blocks), dim3(kBinThreads), 0, nullptr, a, particles_dev, n, hist_dev, yield_dev);
    }
    return hipGetLastError();
}

}  // namespace is3d
