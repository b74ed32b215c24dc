// cf_sampler_flow_diff.hip -- the differential flow records of a particle list on the device (gfx950), one thread per particle.
//
// The per-particle rule is cf_sampler_flow_diff.h, the one is3d_flow_diff_list uses: flow_region and flow_terms of cf_sampler_flow.h, then
// the pT bin by bisection over the edge table, which the workgroup stages in static LDS (66 words) so that the bisection reads are DS reads
// of a wave-divergent index -- no scratch copy of a kernel argument, no flat access.  The record of (event, slot, bin) is the flow record
// of the slot  slot * n_pT + bin, so the adds, the per-wave combine, the window of consecutive events in LDS and its flush are those of
// cf_sampler_flow (cf_sampler_flow.h), with n_slots * n_pT slots.  Everything that is added is a 64-bit integer: kernel form, launch
// geometry and the pieces a list comes in give the same bits.
//   kernel_form 1: global adds after the per-wave combine of equal (event, slot, bin, region) keys.
//   kernel_form 2: the workgroup-private window, n_slots * n_pT * 51 words per event beside the staged edges.
//   kernel_form 0: the window where one event fits, the global form otherwise.  The private form does NOT combine first: measured at 4 slots
//       x 14 bins its plain LDS adds are 6.2 times faster (developer build: IS3D_FLOW_DIFF_PRIVATE_COMBINE for the A/B).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <vector>

#include "cf_host.h"
#include "cf_sampler_flow_diff.h"

namespace is3d {
namespace {

constexpr int kFlowDiffThreads = 256;
static_assert(kFlowDiffThreads >= kFlowDiffEdgeWords, "one thread stages one edge");
constexpr bool kFlowDiffPrivateCombine = false;          // measured: plain ds_add_u64 into the window is 6.2 times faster than combining first

struct FlowDiffArgs {
    is3d_flow_cuts c;
    FlowThresholds t;
    int n_events, n_slots, n_pT, n_species, window;      // window: events in LDS (private form)
};

template <bool PRIVATE, bool COMBINE>
__global__ void __launch_bounds__(kFlowDiffThreads)
cf_sampler_flow_diff(FlowDiffArgs a, const double *__restrict__ edges, const int32_t *__restrict__ slot, const is3d_particle *__restrict__ particles,
                     int64_t n, int64_t slice, unsigned long long *__restrict__ records)
{
    extern __shared__ unsigned long long priv[];
    const int64_t begin = (int64_t)blockIdx.x * slice, end = begin + slice < n ? begin + slice : n;
    const int lane = threadIdx.x & 63;
    const int n_keys = a.n_slots * a.n_pT;
    FlowTarget t{priv, records, 0, a.window, n_keys, a.n_events};
    flow_diff_stage_edges(edges, a.n_pT);
    if (PRIVATE)
        t.base = flow_window_open<kFlowDiffThreads>(priv, (int64_t)a.window * n_keys * kFlowRecordWords, begin, end, [&](int64_t i) {
            const int e = particles[i].event, sp = particles[i].species;
            return sp >= 0 && sp < a.n_species && e >= 0 && e < a.n_events ? e : -1;
        });
    else
        __syncthreads();
    // the trip count is the same for every thread of the workgroup: the wave operations of flow_add_trip see whole waves
    for (int64_t i0 = begin; i0 < end; i0 += kFlowDiffThreads) {
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
                if (region >= 0) {
                    s = flow_diff_slot(s, a.n_pT, flow_diff_bin_lds(a.n_pT, q));
                    flow_terms(q, re, im);
                }
            }
        }
        flow_add_trip<PRIVATE, COMBINE>(t, lane, region >= 0, ev, s, region, re, im);
    }
    if (PRIVATE) flow_window_flush<kFlowDiffThreads>(t);
}

template <bool PRIVATE, bool COMBINE>
void launch(const FlowDiffArgs &a, const double *edges_dev, const int32_t *slot_dev, const is3d_particle *particles_dev, int64_t n,
            unsigned long long *records_dev)
{
    int64_t blocks, slice;
    flow_list_geometry(PRIVATE, n, kFlowDiffThreads, &blocks, &slice);
    const size_t lds = PRIVATE ? (size_t)a.window * a.n_slots * a.n_pT * kFlowRecordWords * sizeof(unsigned long long) : 0;
    hipLaunchKernelGGL((cf_sampler_flow_diff<PRIVATE, COMBINE>), dim3((unsigned)blocks), dim3(kFlowDiffThreads), lds, nullptr, a, edges_dev, slot_dev,
                       particles_dev, n, slice, records_dev);
}

}  // namespace

hipError_t flow_diff_launch(const is3d_flow_cuts &c, const FlowThresholds &t, int n_pT, const double *edges_dev, int n_events, int n_slots,
                            const int32_t *slot_dev, int n_species, const is3d_particle *particles_dev, int64_t n,
                            unsigned long long *records_dev, int form)
{
    if (n <= 0) return hipSuccess;
    const int window = flow_diff_window_events(n_events, n_slots, n_pT);
    if (form == 2 && window < 1) return hipErrorInvalidValue;
    const bool priv = form == 2 || (form == 0 && window >= 1);
    const FlowDiffArgs a{c, t, n_events, n_slots, n_pT, n_species, window};
#ifdef IS3D_DEV
    // developer build only: the private form with the per-wave combine, the A/B of DESIGN.md section 3u
    bool combine = kFlowDiffPrivateCombine;
    if (const char *e = dev_env("IS3D_FLOW_DIFF_PRIVATE_COMBINE")) combine = atoi(e) != 0;
    if (priv && combine) {
        launch<true, true>(a, edges_dev, slot_dev, particles_dev, n, records_dev);
        return hipGetLastError();
    }
#endif
    if (priv) launch<true, kFlowDiffPrivateCombine>(a, edges_dev, slot_dev, particles_dev, n, records_dev);
    else launch<false, true>(a, edges_dev, slot_dev, particles_dev, n, records_dev);
    return hipGetLastError();
}

}  // namespace is3d

// a caller's list through the kernel: upload, flow_diff_launch, download
extern "C" int is3d_flow_diff_list_device(const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges, int32_t n_events, int32_t n_slots,
                                          const int32_t *slot, int32_t n_species, int64_t n_particles, const is3d_particle *particles,
                                          const is3d_flow_diff_records *records, int64_t *n_skipped, int32_t device)
{
    using is3d::set_error;
    if (!n_skipped) return set_error(IS3D_EINVAL, "null argument");
    *n_skipped = 0;
    if (int rc = is3d::flow_diff_check_args(cuts, n_pT, pT_edges, n_events, n_slots, slot, n_species, records, 0)) return rc;
    if (n_particles < 0 || (n_particles > 0 && !particles)) return set_error(IS3D_EINVAL, "n_particles must be >= 0 and particles non-null");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    const is3d_flow_records view = is3d::flow_diff_view(*records);
    const int32_t n_keys = n_slots * n_pT;
    is3d::flow_records_zero(&view, n_events, n_keys);
    if (n_particles == 0) return IS3D_OK;
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].species < 0 || particles[i].species >= n_species || particles[i].event < 0 || particles[i].event >= n_events) ++*n_skipped;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    const size_t words = (size_t)n_events * n_keys * is3d::kFlowRecordWords;
    is3d::DevBuf<unsigned char> d_list, d_slot, d_edges, d_rec;
    HIP_TRY(d_rec.alloc(words * sizeof(int64_t)));
    HIP_TRY(hipMemsetAsync(d_rec.p, 0, words * sizeof(int64_t), nullptr));
    HIP_TRY(d_slot.upload(slot, (size_t)n_species));
    HIP_TRY(d_edges.upload(pT_edges, (size_t)n_pT + 1));
    HIP_TRY(d_list.upload(particles, (size_t)n_particles));
    HIP_TRY(is3d::flow_diff_launch(*cuts, is3d::flow_thresholds(*cuts), n_pT, d_edges.as<double>(), n_events, n_slots, d_slot.as<int32_t>(), n_species,
                                   d_list.as<is3d_particle>(), n_particles, d_rec.as<unsigned long long>(), cuts->kernel_form));
    std::vector<int64_t> h(words);
    HIP_TRY(hipMemcpy(h.data(), d_rec.p, words * sizeof(int64_t), hipMemcpyDeviceToHost));
    is3d::flow_records_scatter(h.data(), &view, n_events, n_keys);
    return is3d::flow_records_check(&view, n_events, n_keys);
}
