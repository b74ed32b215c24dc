// cf_sampler_flow.hip -- the per-event flow records of a particle list on the device (gfx950), one thread per particle.
//
// The per-particle rule is cf_sampler_flow.h, the one is3d_flow_list uses.  Everything that is added is a 64-bit integer (counts, and the
// flow-vector terms in fixed point), so the records do not depend on the order in which the adds arrive: kernel form, launch geometry and the
// pieces a list comes in give the same bits.  No float atomics.
//
// All hadrons of an event add to the same 51 * n_slots words, so the kernel is built against contention, not bandwidth:
//   combine (global form): the lanes of a wave that hold the same (event, slot, region) key sum their 17 values with cross-lane adds and ONE
//       lane does the 17 adds (34 with a sub-event) -- a ballot loop over the distinct keys of the wave, which retires its leader's key on
//       every trip.  The private form does NOT combine first: measured, its plain LDS adds are 4.6 times faster.
//   workgroup-private: every workgroup takes a CONTIGUOUS slice of the list (ordered by event: a slice sees few events) and keeps the records
//       of a window of W consecutive events in LDS, from the event of the slice's first valid particle; adds inside the window are ds_add_u64,
//       the non-zero words are flushed once with global 64-bit adds.  A particle whose event lies outside the window (an unordered list, a
//       slice of many tiny events) adds to global memory directly: counted all the same, with more adds.
//   global: every add goes to global memory (hundreds of slots: not even one event's records fit the LDS).
// Every thread of a workgroup makes the same number of trips and reaches every __syncthreads; the wave operations see whole waves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "cf_host.h"
#include "cf_sampler_flow.h"

namespace is3d {
namespace {

constexpr int kFlowThreads = 256;
constexpr bool kFlowPrivateCombine = false;              // measured: plain ds_add_u64 into the window is 4.6 times faster than combining first

struct FlowArgs {
    is3d_flow_cuts c;
    FlowThresholds t;
    int n_events, n_slots, n_species, window;            // window: events in LDS (private form)
};

template <bool PRIVATE, bool COMBINE>
__global__ void __launch_bounds__(kFlowThreads)
cf_sampler_flow(FlowArgs a, const int32_t *__restrict__ slot, const is3d_particle *__restrict__ particles, int64_t n, int64_t slice,
                unsigned long long *__restrict__ records)
{
    extern __shared__ unsigned long long priv[];
    const int64_t begin = (int64_t)blockIdx.x * slice, end = begin + slice < n ? begin + slice : n;
    const int lane = threadIdx.x & 63;
    FlowTarget t{priv, records, 0, a.window, a.n_slots, a.n_events};
    if (PRIVATE)
        t.base = flow_window_open<kFlowThreads>(priv, (int64_t)a.window * a.n_slots * kFlowRecordWords, begin, end, [&](int64_t i) {
            const int e = particles[i].event, sp = particles[i].species;
            return sp >= 0 && sp < a.n_species && e >= 0 && e < a.n_events ? e : -1;
        });
    // the trip count is the same for every thread of the workgroup: the wave operations below see whole waves
    for (int64_t i0 = begin; i0 < end; i0 += kFlowThreads) {
        const int64_t i = i0 + threadIdx.x;
        int ev = 0, s = 0, region = -1;
        long long re[IS3D_FLOW_HARMONICS], im[IS3D_FLOW_HARMONICS];
        for (int m = 0; m < IS3D_FLOW_HARMONICS; m++) re[m] = im[m] = 0;
        if (i < end) {
            const is3d_particle q = particles[i];
            if (q.species >= 0 && q.species < a.n_species && q.event >= 0 && q.event < a.n_events) {
                ev = q.event;
                s = slot[q.species];
                if (s >= 0) region = flow_region(a.c, a.t, q);
                if (region >= 0) flow_terms(q, re, im);
            }
        }
        const bool act = region >= 0;
        flow_add_trip<PRIVATE, COMBINE>(t, lane, act, ev, s, region, re, im);
    }
    if (PRIVATE) flow_window_flush<kFlowThreads>(t);
}

template <bool PRIVATE, bool COMBINE>
void launch(const FlowArgs &a, const int32_t *slot_dev, const is3d_particle *particles_dev, int64_t n, unsigned long long *records_dev)
{
    int64_t blocks, slice;
    flow_list_geometry(PRIVATE, n, kFlowThreads, &blocks, &slice);
    const size_t lds = PRIVATE ? (size_t)a.window * a.n_slots * kFlowRecordWords * sizeof(unsigned long long) : 0;
    hipLaunchKernelGGL((cf_sampler_flow<PRIVATE, COMBINE>), dim3((unsigned)blocks), dim3(kFlowThreads), lds, nullptr, a, slot_dev, particles_dev, n, slice,
                       records_dev);
}

}  // namespace

hipError_t flow_launch(const is3d_flow_cuts &c, const FlowThresholds &t, int n_events, int n_slots, const int32_t *slot_dev, int n_species,
                       const is3d_particle *particles_dev, int64_t n, unsigned long long *records_dev, int form)
{
    if (n <= 0) return hipSuccess;
    const int window = flow_window_events(n_events, n_slots);
    if (form == 2 && window < 1) return hipErrorInvalidValue;
    const bool priv = form == 2 || (form == 0 && window >= 1);
    const FlowArgs a{c, t, n_events, n_slots, n_species, window};
#ifdef IS3D_DEV
    // developer build only: the private form with the per-wave combine, the A/B of DESIGN.md section 3r
    bool combine = kFlowPrivateCombine;
    if (const char *e = dev_env("IS3D_FLOW_PRIVATE_COMBINE")) combine = atoi(e) != 0;
    if (priv && combine) {
        launch<true, true>(a, slot_dev, particles_dev, n, records_dev);
        return hipGetLastError();
    }
#endif
    if (priv) launch<true, kFlowPrivateCombine>(a, slot_dev, particles_dev, n, records_dev);
    else launch<false, true>(a, slot_dev, particles_dev, n, records_dev);
    return hipGetLastError();
}

}  // namespace is3d

// a caller's list through the kernel: upload, flow_launch, download
extern "C" int is3d_flow_list_device(const is3d_flow_cuts *cuts, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                                     int64_t n_particles, const is3d_particle *particles, const is3d_flow_records *records, int64_t *n_skipped,
                                     int32_t device)
{
    using is3d::set_error;
    if (!n_skipped) return set_error(IS3D_EINVAL, "null argument");
    *n_skipped = 0;
    if (int rc = is3d::flow_check_args(cuts, n_events, n_slots, slot, n_species, records, 0)) return rc;
    if (n_particles < 0 || (n_particles > 0 && !particles)) return set_error(IS3D_EINVAL, "n_particles must be >= 0 and particles non-null");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    is3d::flow_records_zero(records, n_events, n_slots);
    if (n_particles == 0) return IS3D_OK;
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].species < 0 || particles[i].species >= n_species || particles[i].event < 0 || particles[i].event >= n_events) ++*n_skipped;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    const size_t words = (size_t)n_events * n_slots * is3d::kFlowRecordWords;
    is3d::DevBuf<unsigned char> d_list, d_slot, d_rec;
    HIP_TRY(d_rec.alloc(words * sizeof(int64_t)));
    HIP_TRY(hipMemsetAsync(d_rec.p, 0, words * sizeof(int64_t), nullptr));
    HIP_TRY(d_slot.upload(slot, (size_t)n_species));
    HIP_TRY(d_list.upload(particles, (size_t)n_particles));
    HIP_TRY(is3d::flow_launch(*cuts, is3d::flow_thresholds(*cuts), n_events, n_slots, d_slot.as<int32_t>(), n_species, d_list.as<is3d_particle>(),
                              n_particles, d_rec.as<unsigned long long>(), cuts->kernel_form));
    std::vector<int64_t> h(words);
    HIP_TRY(hipMemcpy(h.data(), d_rec.p, words * sizeof(int64_t), hipMemcpyDeviceToHost));
    is3d::flow_records_scatter(h.data(), records, n_events, n_slots);
    return is3d::flow_records_check(records, n_events, n_slots);
}
