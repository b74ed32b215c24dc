// cf_sampler_flow_diff.h -- the per-particle rule of the differential flow records: the flow records of
// cf_sampler_flow.h with the pT bin as a second key, stated ONCE for the host (flow_diff_host.cpp: is3d_flow_diff_list) and the device
// (cf_sampler_flow_diff.hip, cf_decays_mc.hip).
//
// Acceptance, region and terms are flow_region and flow_terms, unchanged: the edge table IS the acceptance in pT (cuts.pT_min and
// cuts.pT_max equal its first and last edge bit for bit).  The bin of an accepted particle is found by bisection over the edges -- host
// doubles handed to the kernels as bits -- with comparisons only, on pT = sqrt(px^2 + py^2) computed as flow_region computes it, with
// floating-point contraction OFF on both sides: no division by a bin width, no libm in any decision, so host and device reach the same bin
// from the same particle bits.
//
// A record of (event, slot, bin) is laid out as a flow record of the slot  slot * n_pT + bin  among n_slots * n_pT: the block
// [event][slot][bin][region][17] is the flow block of that many slots, and the target, the adds, the window and its flush, the zeroing,
// the scatter and the count check of cf_sampler_flow.h serve both.
#pragma once
#include "cf_sampler_flow.h"

namespace is3d {

constexpr int kFlowDiffMaxBins = IS3D_FLOW_DIFF_MAX_BINS;
// what the kernels keep in static LDS beside the window: the 65 edges and a pad word, so that static blocks that the compiler aligns to
// 16 bytes (this one, the decay kernel's six tally words) end where the budget says they do
constexpr int kFlowDiffEdgeWords = kFlowDiffMaxBins + 2;

// finite, strictly ascending, first edge >= 0, 1 <= n_pT <= 64 (NaN compares false)
inline bool flow_diff_edges_valid(int32_t n_pT, const double *edges)
{
    if (n_pT < 1 || n_pT > kFlowDiffMaxBins || !edges) return false;
    if (!(edges[0] >= 0.0)) return false;
    for (int k = 1; k <= n_pT; k++)
        if (!(edges[k] > edges[k - 1] && edges[k] <= 1.7976931348623157e308)) return false;
    return true;
}

// pT exactly as flow_region computes it
IS3D_BINS_HD double flow_diff_pT(const is3d_particle &q)
{
    IS3D_BINS_NO_CONTRACT
    const double px2 = q.px * q.px, py2 = q.py * q.py;
    return sqrt(px2 + py2);
}

// the bin of a particle flow_region accepted (edge(0) <= pT < edge(n_pT)): the largest b with edge(b) <= pT.  edge: k -> the k-th edge
// (the host's table, the kernel's LDS copy)
template <class Edge>
IS3D_BINS_HD int flow_diff_bin(const Edge &edge, int n_pT, double pT)
{
    int lo = 0, hi = n_pT;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (edge(mid) <= pT) lo = mid; else hi = mid;
    }
    return lo;
}

IS3D_BINS_HD int flow_diff_slot(int s, int n_pT, int bin) { return s * n_pT + bin; }

// the records as flow records of n_slots * n_pT slots
inline is3d_flow_records flow_diff_view(const is3d_flow_diff_records &r) { return is3d_flow_records{r.m, r.p_re, r.p_im}; }

// the number of consecutive events the workgroup-private form keeps in LDS beside the staged edges (and static_words more)
inline int flow_diff_window_events(int32_t n_events, int32_t n_slots, int32_t n_pT, int static_words = 0)
{
    return flow_window_events(n_events, n_slots * n_pT, static_words + kFlowDiffEdgeWords);
}

// the argument checks of every differential entry (IS3D_EINVAL, no device use): those of flow_check_args, the edge table, the ends of
// the table against cuts.pT_min / pT_max, and kernel_form = 2 when not even one event's records fit (device_static_words as there)
int flow_diff_check_args(const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges, int32_t n_events, int32_t n_slots, const int32_t *slot,
                         int32_t n_species, const is3d_flow_diff_records *records, int device_static_words);

#if defined(__HIP__) || defined(__HIPCC__)
// the edge table of the running kernel in static LDS, named here so that every read of the bisection is a DS one; staged by
// flow_diff_stage_edges, which every thread of the workgroup calls before a barrier that precedes the first bin
__device__ __forceinline__ double &flow_diff_lds_edge(int k)
{
    __shared__ double edge[kFlowDiffEdgeWords];
    return edge[k];
}
__device__ __forceinline__ void flow_diff_stage_edges(const double *__restrict__ edges_dev, int n_pT)
{
    if ((int)threadIdx.x <= n_pT) flow_diff_lds_edge((int)threadIdx.x) = edges_dev[threadIdx.x];
}
__device__ __forceinline__ int flow_diff_bin_lds(int n_pT, const is3d_particle &q)
{
    return flow_diff_bin([](int k) { return flow_diff_lds_edge(k); }, n_pT, flow_diff_pT(q));
}

// the device side (cf_sampler_flow_diff.hip): as flow_launch, with the edges as a DEVICE array of n_pT + 1 doubles
hipError_t flow_diff_launch(const is3d_flow_cuts &c, const FlowThresholds &t, int n_pT, const double *edges_dev, int n_events, int n_slots,
                            const int32_t *slot_dev, int n_species, const is3d_particle *particles_dev, int64_t n,
                            unsigned long long *records_dev, int form);
#endif

}  // namespace is3d
