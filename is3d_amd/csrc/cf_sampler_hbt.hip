// cf_sampler_hbt.hip -- the HBT correlation histograms of a particle list on the device (gfx950): a true loop over the ordered
// identical-particle pairs of every event, because the weight cos(q . dx / hbarc) depends on both positions.
//
// The rule is cf_sampler_hbt.h, the one is3d_hbt_list uses; den, num and M are 64-bit integer sums, so the result does not depend on the
// order of the records, on the batching or on the kernel form.
//   cf_hbt_select   thread <-> particle, run twice over the same list: the count pass adds 1 to count[event][slot] for every accepted
//                   particle; the host reads the counts (they are M, and they size the work), scans them into segment offsets and cuts
//                   the pair loop into work items; the fill pass takes a place from the segment's cursor and writes the 64-byte record
//                   (E, px, py, pz, t, x, y, z) there.
//   cf_hbt_pairs    workgroup <-> work item = (segment, tile of 256 i, run of j): a thread owns ONE i in registers; the run of j is staged
//                   in LDS 256 records at a time and read by all lanes at the same address (a broadcast).  hbt_pair_bin rejects a pair on
//                   kT and on each side of the q cube in turn, before the phase and its cos are formed; an accepted pair makes two 64-bit
//                   integer adds -- into global memory (form 1), or into the workgroup's private copy of its slot's block in LDS, flushed
//                   once with global adds of the non-zero words (form 2).  The run of j is at most kHbtRunTiles tiles, more for a very
//                   large segment, so one event of 10^5 pions is spread over thousands of workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "cf_host.h"
#include "cf_sampler_hbt.h"

namespace is3d {
namespace {

constexpr int64_t kHbtSelectBlocks = (int64_t)1 << 20;
constexpr int kHbtRunTiles = 16;                 // tiles of j per work item ...
constexpr int64_t kHbtRunsPerTile = 64;          // ... or more, so that a tile of i has at most this many items

__global__ void __launch_bounds__(kHbtThreads)
cf_hbt_select(const HbtSelectArgs a, const int32_t *__restrict__ slot, const int n_species, const is3d_particle *__restrict__ particles, const int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kHbtThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kHbtThreads) {
        const int sp = particles[i].species, ev = particles[i].event;
        if (sp < 0 || sp >= n_species || ev < 0 || ev >= a.n_events) continue;
        const int s = slot[sp];
        if (s < 0 || s >= a.n_slots) continue;
        const is3d_particle q = particles[i];
        if (!hbt_accept(a.b, a.d, q.E, q.px, q.py, q.pz)) continue;
        hbt_select_put(a, ev, s, HbtRecord{q.E, q.px, q.py, q.pz, q.t, q.x, q.y, q.z});
    }
}

struct HbtPairArgs {
    is3d_hbt_bins b;
    HbtDerived d;
    int64_t slot_bins, hist_words;               // n_kT n_q^3; n_slots times that: den at [0, hist_words), num behind it
};

// the workgroup's private block, den [slot_bins] | num [slot_bins]: the kernel's dynamic LDS, named here so that every access is a DS one
__device__ __forceinline__ void hbt_priv_add(int64_t w, unsigned long long v)
{
    extern __shared__ unsigned long long hbt_priv[];
    atomicAdd(&hbt_priv[w], v);
}
__device__ __forceinline__ void hbt_priv_put(int64_t w, unsigned long long v)
{
    extern __shared__ unsigned long long hbt_priv[];
    hbt_priv[w] = v;
}
__device__ __forceinline__ unsigned long long hbt_priv_get(int64_t w)
{
    extern __shared__ unsigned long long hbt_priv[];
    return hbt_priv[w];
}

template <bool PRIVATE>
__global__ void __launch_bounds__(kHbtThreads)
cf_hbt_pairs(const HbtPairArgs a, const HbtItem *__restrict__ items, const HbtRecord *__restrict__ records, unsigned long long *__restrict__ hist)
{
    __shared__ HbtRecord tile[kHbtThreads];
    const HbtItem it = items[blockIdx.x];
    const HbtRecord *seg = records + it.base;
    const int i = it.i0 + (int)threadIdx.x;
    const bool own = i < it.n;
    const HbtRecord me = seg[own ? i : it.i0];    // i0 < n: a thread beyond the segment carries a copy and adds nothing
    unsigned long long *den = hist + (int64_t)it.slot * a.slot_bins, *num = den + a.hist_words;
    if (PRIVATE)
        for (int64_t w = threadIdx.x; w < 2 * a.slot_bins; w += kHbtThreads) hbt_priv_put(w, 0ULL);
    for (int j0 = it.j0; j0 < it.j1; j0 += kHbtThreads) {
        __syncthreads();
        const int cnt = min(kHbtThreads, it.j1 - j0);
        if ((int)threadIdx.x < cnt) tile[threadIdx.x] = seg[j0 + (int)threadIdx.x];
        __syncthreads();
        if (!own) continue;
        for (int k = 0; k < cnt; k++) {
            if (j0 + k == i) continue;
            const HbtRecord other = tile[k];
            const int bin = hbt_pair_bin(a.b, a.d, me, other);
            if (bin < 0) continue;
            const unsigned long long term = (unsigned long long)hbt_pair_term(me, other);   // two's complement: signed sums
            if (PRIVATE) {
                hbt_priv_add(bin, 1ULL);
                hbt_priv_add(a.slot_bins + bin, term);
            } else {
                atomicAdd(&den[bin], 1ULL);
                atomicAdd(&num[bin], term);
            }
        }
    }
    if (PRIVATE) {
        __syncthreads();
        for (int64_t w = threadIdx.x; w < a.slot_bins; w += kHbtThreads) {
            const unsigned long long c = hbt_priv_get(w);
            if (c) {
                atomicAdd(&den[w], c);
                atomicAdd(&num[w], hbt_priv_get(a.slot_bins + w));
            }
        }
    }
}

// grows d to at least `bytes`; IS3D_ENOMEM naming the size and what it is
int hbt_grow(DevBuf<unsigned char> &d, size_t bytes, const char *what)
{
    if (bytes <= d.n) return IS3D_OK;
    const hipError_t e = d.alloc(bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        d.release();
        return set_error(IS3D_ENOMEM, "out of device memory allocating %s of the HBT histograms: %zu bytes", what, bytes);
    }
    HIP_TRY(e);
    return IS3D_OK;
}

}  // namespace

int HbtRun::begin(const is3d_hbt_bins &bins, int32_t events, int32_t slots)
{
    b = bins;
    d = hbt_derived(bins);
    n_events = events;
    n_slots = slots;
    // form 0, the measured choice: the private block where it fits
    form = bins.kernel_form == 0 ? (hbt_private_fits(bins) ? 2 : 1) : bins.kernel_form;
    const size_t segs = (size_t)events * slots, hist_bytes = 2 * (size_t)slots * (size_t)hbt_slot_bins(bins) * sizeof(int64_t);
    if (int rc = hbt_grow(d_hist, hist_bytes, "the den and num block (2 x n_slots x n_kT x n_q^3 64-bit words)")) return rc;
    if (int rc = hbt_grow(d_count, 2 * segs * sizeof(unsigned), "the segment counts and cursors")) return rc;
    if (int rc = hbt_grow(d_offset, segs * sizeof(int64_t), "the segment offsets")) return rc;
    HIP_TRY(hipMemsetAsync(d_hist.p, 0, hist_bytes, nullptr));
    M.assign(segs, 0);
    counts.assign(segs, 0u);
    ms_pairs = 0.0;
    return IS3D_OK;
}

int HbtRun::batch_begin()
{
    HIP_TRY(hipMemsetAsync(d_count.p, 0, 2 * (size_t)n_events * n_slots * sizeof(unsigned), nullptr));
    return IS3D_OK;
}

int HbtRun::batch_plan()
{
    const size_t segs = (size_t)n_events * n_slots;
    HIP_TRY(hipMemcpy(counts.data(), d_count.p, segs * sizeof(unsigned), hipMemcpyDeviceToHost));
    std::vector<int64_t> offset(segs);
    std::vector<HbtItem> items;
    int64_t total = 0;
    for (size_t g = 0; g < segs; g++) {
        const int64_t n = counts[g];
        offset[g] = total;
        M[g] += n;
        if (n > 0x7fffffffLL - kHbtThreads)
            return set_error(IS3D_EDOMAIN, "HBT histograms: (event %lld, slot %lld) holds %lld accepted hadrons in one batch", (long long)(g / (size_t)n_slots),
                             (long long)(g % (size_t)n_slots), (long long)n);
        if (n >= 2) {
            const int64_t tiles = (n + kHbtThreads - 1) / kHbtThreads;
            const int64_t run = std::max<int64_t>(kHbtRunTiles, (tiles + kHbtRunsPerTile - 1) / kHbtRunsPerTile) * kHbtThreads;
            for (int64_t i0 = 0; i0 < n; i0 += kHbtThreads)
                for (int64_t j0 = 0; j0 < n; j0 += run)
                    items.push_back(HbtItem{total, (int32_t)n, (int32_t)(g % (size_t)n_slots), (int32_t)i0, (int32_t)j0, (int32_t)std::min(n, j0 + run), 0});
        }
        total += n;
    }
    n_records = total;
    n_items = (int64_t)items.size();
    if (n_items > 0x7fffffffLL) return set_error(IS3D_EDOMAIN, "HBT histograms: %lld work items in one batch", (long long)n_items);
    if (int rc = hbt_grow(d_records, (size_t)std::max<int64_t>(total, 1) * sizeof(HbtRecord), "the accepted 64-byte records of one batch")) return rc;
    if (int rc = hbt_grow(d_items, (size_t)std::max<int64_t>(n_items, 1) * sizeof(HbtItem), "the work items of one batch")) return rc;
    HIP_TRY(hipMemcpy(d_offset.p, offset.data(), segs * sizeof(int64_t), hipMemcpyHostToDevice));
    if (n_items) HIP_TRY(hipMemcpy(d_items.p, items.data(), (size_t)n_items * sizeof(HbtItem), hipMemcpyHostToDevice));
    return IS3D_OK;
}

int HbtRun::batch_pairs()
{
    if (n_items <= 0) return IS3D_OK;
    const HbtPairArgs a{b, d, hbt_slot_bins(b), (int64_t)n_slots * hbt_slot_bins(b)};
    hipEvent_t ev[2];
    for (int k = 0; k < 2; k++) HIP_TRY(hipEventCreate(&ev[k]));
    HIP_TRY(hipEventRecord(ev[0], nullptr));
    if (form == 2)
        hipLaunchKernelGGL(cf_hbt_pairs<true>, dim3((unsigned)n_items), dim3(kHbtThreads), 2 * (size_t)a.slot_bins * sizeof(unsigned long long), nullptr, a,
                           d_items.as<HbtItem>(), d_records.as<HbtRecord>(), d_hist.as<unsigned long long>());
    else
        hipLaunchKernelGGL(cf_hbt_pairs<false>, dim3((unsigned)n_items), dim3(kHbtThreads), 0, nullptr, a, d_items.as<HbtItem>(),
                           d_records.as<HbtRecord>(), d_hist.as<unsigned long long>());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev[1], nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    for (int k = 0; k < 2; k++) (void)hipEventDestroy(ev[k]);
    HIP_TRY(e);
    ms_pairs += ms;
    return IS3D_OK;
}

int HbtRun::finish(const is3d_hbt_hist *hist)
{
    const size_t words = (size_t)n_slots * (size_t)hbt_slot_bins(b);
    HIP_TRY(hipMemcpy(hist->den, d_hist.p, words * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hist->num, d_hist.p + words * sizeof(int64_t), words * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::copy(M.begin(), M.end(), hist->M);
    return hbt_hist_check(b, hist, n_slots);
}

hipError_t hbt_select_launch(const HbtRun &r, const int32_t *slot_dev, int n_species, const is3d_particle *particles_dev, int64_t n, bool fill)
{
    if (n <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n + kHbtThreads - 1) / kHbtThreads, kHbtSelectBlocks);
    hipLaunchKernelGGL(cf_hbt_select, dim3((unsigned)blocks), dim3(kHbtThreads), 0, nullptr, hbt_select_args(r, fill), slot_dev, n_species, particles_dev, n);
    return hipGetLastError();
}

int hbt_batch_list(HbtRun &r, const int32_t *slot_dev, int n_species, const is3d_particle *particles_dev, int64_t n)
{
    if (n <= 0) return IS3D_OK;
    if (int rc = r.batch_begin()) return rc;
    HIP_TRY(hbt_select_launch(r, slot_dev, n_species, particles_dev, n, false));
    if (int rc = r.batch_plan()) return rc;
    HIP_TRY(hbt_select_launch(r, slot_dev, n_species, particles_dev, n, true));
    return r.batch_pairs();
}

}  // namespace is3d

// a caller's list through both kernels: upload, select (count, fill), pairs, download
extern "C" int is3d_hbt_list_device(const is3d_hbt_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                                    int64_t n_particles, const is3d_particle *particles, const is3d_hbt_hist *hist, int64_t *n_skipped,
                                    int32_t device)
{
    using is3d::set_error;
    if (!n_skipped) return set_error(IS3D_EINVAL, "null argument");
    *n_skipped = 0;
    if (int rc = is3d::hbt_check_args(bins, n_events, n_slots, slot, n_species, hist, true)) return rc;
    if (n_particles < 0 || (n_particles > 0 && !particles)) return set_error(IS3D_EINVAL, "n_particles must be >= 0 and particles non-null");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    is3d::hbt_hist_zero(*bins, hist, n_events, n_slots);
    if (n_particles == 0) return IS3D_OK;
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].species < 0 || particles[i].species >= n_species || particles[i].event < 0 || particles[i].event >= n_events) ++*n_skipped;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    is3d::HbtRun run;
    is3d::DevBuf<unsigned char> d_list, d_slot;
    if (int rc = run.begin(*bins, n_events, n_slots)) return rc;
    HIP_TRY(d_slot.upload(slot, (size_t)n_species));
    {
        const hipError_t e = d_list.upload(particles, (size_t)n_particles);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return set_error(IS3D_ENOMEM, "out of device memory allocating the particle list of the HBT histograms: %zu bytes", (size_t)n_particles * sizeof(is3d_particle));
        }
        HIP_TRY(e);
    }
    if (int rc = is3d::hbt_batch_list(run, d_slot.as<int32_t>(), n_species, d_list.as<is3d_particle>(), n_particles)) return rc;
    return run.finish(hist);
}
