// cf_sampler_pairs.hip -- the two-particle (delta y, delta phi) histograms of a particle list on the device (gfx950), without a loop over
// particle pairs.
//
// The per-particle rule is cf_sampler_pairs.h, the one is3d_pairs_list uses.  Counts are integers, so the pair histogram of an event is the
// cross-correlation of its per-cell occupancies:
//   same[a, b][dy][dphi]  = sum over cells (iy, iphi) of n_a(e)[iy][iphi] * n_b(e)[iy + dy][iphi + dphi]   (minus M_a(e) at (0, 0) for a == b)
//   mixed[a, b][dy][dphi] = the same with n_b(e + 1)
// whose cost depends on the grid and on the number of occupied cells, not on M^2.
//   cf_pair_cells      thread <-> particle: the rule, then ONE 32-bit atomicAdd into occ[event][slot][iy][iphi] in global memory.  The adds
//                      of an event spread over n_slots * n_y * n_phi words.
//   cf_pair_correlate  workgroup <-> (event, class, block of 256 output bins: a few delta y rows): the trigger grid n_a(e) and the associate
//                      grids n_b(e), n_b(e + 1) are staged in LDS (at most 3 * 64 * 64 * 4 B = 48 KiB); a thread owns ONE output bin
//                      (dy, dphi) and loops over the OCCUPIED trigger cells,
//                      which a 64-bit mask per trigger row names.  Mask and trigger word are read through readfirstlane: they live in
//                      SGPRs, so the loop and its skip of empty cells are uniform by construction.  Lanes with consecutive dphi read
//                      consecutive LDS words.  No atomics inside the loop; after it the two 64-bit sums of a bin go to the global blocks
//                      with integer adds, so the result is bit for bit independent of launch geometry and batching.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cf_host.h"
#include "cf_sampler_pairs.h"

namespace is3d {
namespace {

constexpr int kPairThreads = 256;
constexpr int64_t kPairCellBlocks = (int64_t)1 << 20;

struct PairCellArgs {
    is3d_pair_bins b;
    PairTables t;
    int n_events, n_slots, n_species;
};

__global__ void __launch_bounds__(kPairThreads)
cf_pair_cells(const PairCellArgs a, const int32_t *__restrict__ slot, const is3d_particle *__restrict__ particles, const int64_t n,
              unsigned *__restrict__ occ)
{
    for (int64_t i = (int64_t)blockIdx.x * kPairThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPairThreads) {
        const int sp = particles[i].species, ev = particles[i].event;
        if (sp < 0 || sp >= a.n_species || ev < 0 || ev >= a.n_events) continue;
        const int s = slot[sp];
        if (s < 0 || s >= a.n_slots) continue;
        const int cell = pair_cell(a.b, a.t, particles[i].E, particles[i].px, particles[i].py, particles[i].pz);
        if (cell >= 0) pair_add(a.b, occ, a.n_slots, ev, s, cell);
    }
}

struct PairCorrArgs {
    int n_y, n_phi, n_slots, n_events, n_classes, n_blocks;   // n_blocks: blocks of kPairThreads output bins per (event, class)
};

// the three staged grids, [0, cells) trigger, [cells, 2 cells) associate of e, [2 cells, 3 cells) associate of e + 1: the kernel's dynamic
// LDS, named here so that every access is a DS one
__device__ __forceinline__ unsigned pair_grid_get(int j)
{
    extern __shared__ unsigned pair_grids[];
    return pair_grids[j];
}
__device__ __forceinline__ void pair_grid_put(int j, unsigned v)
{
    extern __shared__ unsigned pair_grids[];
    pair_grids[j] = v;
}

__global__ void __launch_bounds__(kPairThreads)
cf_pair_correlate(const PairCorrArgs a, const unsigned *__restrict__ occ, unsigned long long *__restrict__ same, unsigned long long *__restrict__ mixed,
                  unsigned long long *__restrict__ M)
{
    __shared__ unsigned long long row_mask[kPairMaxBins];   // bit iphi of word iy: the trigger cell is occupied
    __shared__ unsigned long long part[kPairThreads / 64];
    const int blk = (int)(blockIdx.x % (unsigned)a.n_blocks), ec = (int)(blockIdx.x / (unsigned)a.n_blocks);
    const int e = ec / a.n_classes, cls = ec % a.n_classes;
    int sa = 0, sb = cls;                                    // class -> (a <= b): the same for the whole workgroup
    while (sb >= a.n_slots - sa) { sb -= a.n_slots - sa; sa++; }
    sb += sa;
    const int cells = a.n_y * a.n_phi, nbins = (2 * a.n_y - 1) * a.n_phi;
    const bool mix = a.n_events >= 2;
    const int e1 = e + 1 < a.n_events ? e + 1 : 0;
    const unsigned *ga = occ + ((int64_t)e * a.n_slots + sa) * cells, *gb = occ + ((int64_t)e * a.n_slots + sb) * cells,
                   *gm = occ + ((int64_t)e1 * a.n_slots + sb) * cells;
    if (threadIdx.x < kPairMaxBins) row_mask[threadIdx.x] = 0ULL;
    __syncthreads();
    unsigned long long m = 0ULL;
    for (int j = threadIdx.x; j < cells; j += kPairThreads) {
        const unsigned na = ga[j];
        pair_grid_put(j, na);
        pair_grid_put(cells + j, gb[j]);
        pair_grid_put(2 * cells + j, mix ? gm[j] : 0u);
        m += na;
        if (na) {
            const int iy = j / a.n_phi;
            atomicOr(&row_mask[iy], 1ULL << (j - iy * a.n_phi));
        }
    }
    for (int d = 32; d >= 1; d >>= 1) m += __shfl_xor(m, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    unsigned long long Ma = 0ULL;
    for (int w = 0; w < kPairThreads / 64; w++) Ma += part[w];
    if (sa == sb && blk == 0 && threadIdx.x == 0) M[(int64_t)e * a.n_slots + sa] = Ma;   // ONE workgroup per (event, slot) writes it
    if (Ma == 0ULL) return;                                  // the same word for every thread: no trigger, nothing to add
    // a thread beyond the last bin carries zeros through the same loop
    {
        const int k = blk * kPairThreads + (int)threadIdx.x;
        const bool own = k < nbins;
        const int dy = own ? k / a.n_phi : 0, dphi = own ? k - dy * a.n_phi : 0;
        const int shift = dy - (a.n_y - 1);
        unsigned long long acc_same = 0ULL, acc_mixed = 0ULL;
        // the trigger rows that have an associate row inside the grid for at least one delta y of this block (the block's own bounds: uniform)
        const int k_last = min(blk * kPairThreads + kPairThreads - 1, nbins - 1);
        const int dy_lo = blk * kPairThreads / a.n_phi, dy_hi = k_last / a.n_phi;
        const int row_lo = max(0, a.n_y - 1 - dy_hi), row_hi = min(a.n_y - 1, 2 * a.n_y - 2 - dy_lo);
        for (int iya = row_lo; iya <= row_hi; iya++) {
            const unsigned long long rm = row_mask[iya];
            // the mask in SGPRs: the loop over the occupied cells of the row is uniform for the wave by construction
            unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)rm), hi = __builtin_amdgcn_readfirstlane((unsigned)(rm >> 32));
            const int iyb = iya + shift;
            const bool in = own && iyb >= 0 && iyb < a.n_y;
            const int rowb = cells + (in ? iyb : 0) * a.n_phi;
            for (int half = 0; half < 2; half++) {
                unsigned bits = half ? hi : lo;
                while (bits) {
                    const int ipa = half * 32 + __builtin_ctz(bits);
                    bits &= bits - 1;
                    const unsigned na = __builtin_amdgcn_readfirstlane(pair_grid_get(iya * a.n_phi + ipa));
                    int ipb = ipa + dphi;
                    if (ipb >= a.n_phi) ipb -= a.n_phi;
                    const unsigned nb = in ? pair_grid_get(rowb + ipb) : 0u;
                    acc_same += (unsigned long long)na * nb;
                    if (mix) {
                        const unsigned nm = in ? pair_grid_get(cells + rowb + ipb) : 0u;
                        acc_mixed += (unsigned long long)na * nm;
                    }
                }
            }
        }
        if (sa == sb && k == (a.n_y - 1) * a.n_phi) acc_same -= Ma;           // the self pairs i == j
        if (own && acc_same) atomicAdd(&same[(int64_t)cls * nbins + k], acc_same);
        if (own && acc_mixed) atomicAdd(&mixed[(int64_t)cls * nbins + k], acc_mixed);
    }
}

}  // namespace

hipError_t pair_cells_launch(const is3d_pair_bins &b, const PairTables &t, int n_events, int n_slots, const int32_t *slot_dev, int n_species,
                             const is3d_particle *particles_dev, int64_t n, unsigned *occ_dev)
{
    if (n <= 0) return hipSuccess;
    const PairCellArgs a{b, t, n_events, n_slots, n_species};
    const int64_t blocks = std::min<int64_t>((n + kPairThreads - 1) / kPairThreads, kPairCellBlocks);
    hipLaunchKernelGGL(cf_pair_cells, dim3((unsigned)blocks), dim3(kPairThreads), 0, nullptr, a, slot_dev, particles_dev, n, occ_dev);
    return hipGetLastError();
}

hipError_t pair_correlate_launch(const is3d_pair_bins &b, int n_events, int n_slots, const unsigned *occ_dev, unsigned long long *out_dev)
{
    const int64_t n_classes = pair_classes(n_slots), n_blocks = (pair_hist_bins(b) + kPairThreads - 1) / kPairThreads;
    const int64_t blocks = n_classes * n_events * n_blocks;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t hist_words = (size_t)n_classes * (size_t)pair_hist_bins(b);
    hipError_t e = hipMemsetAsync(out_dev, 0, pair_out_words(b, n_events, n_slots) * sizeof(unsigned long long), nullptr);
    if (e != hipSuccess) return e;
    const PairCorrArgs a{b.n_y, b.n_phi, n_slots, n_events, (int)n_classes, (int)n_blocks};
    hipLaunchKernelGGL(cf_pair_correlate, dim3((unsigned)blocks), dim3(kPairThreads), 3 * (size_t)pair_grid_cells(b) * sizeof(unsigned), nullptr, a,
                       occ_dev, out_dev, out_dev + hist_words, out_dev + 2 * hist_words);
    return hipGetLastError();
}

int pair_occ_begin(DevBuf<unsigned char> &d, size_t head_bytes, size_t words)
{
    const size_t bytes = head_bytes + words * sizeof(unsigned);
    if (bytes > d.n) {
        const hipError_t e = d.alloc(bytes);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            d.release();
            return set_error(IS3D_ENOMEM, "out of device memory allocating the occupancy block of the pair histograms: %zu bytes (n_events x n_slots x "
                             "n_y x n_phi 32-bit words)", bytes);
        }
        HIP_TRY(e);
    }
    HIP_TRY(hipMemsetAsync(d.p, 0, bytes, nullptr));
    return IS3D_OK;
}

}  // namespace is3d

// a caller's list through both kernels: upload, cf_pair_cells, cf_pair_correlate, download
extern "C" int is3d_pairs_list_device(const is3d_pair_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                                      int64_t n_particles, const is3d_particle *particles, const is3d_pair_hist *hist, int64_t *n_skipped,
                                      int32_t device)
{
    using is3d::set_error;
    if (!n_skipped) return set_error(IS3D_EINVAL, "null argument");
    *n_skipped = 0;
    if (int rc = is3d::pair_check_args(bins, n_events, n_slots, slot, n_species, hist)) return rc;
    if (n_particles < 0 || (n_particles > 0 && !particles)) return set_error(IS3D_EINVAL, "n_particles must be >= 0 and particles non-null");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    is3d::pair_hist_zero(*bins, hist, n_events, n_slots);
    if (n_particles == 0) return IS3D_OK;
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].species < 0 || particles[i].species >= n_species || particles[i].event < 0 || particles[i].event >= n_events) ++*n_skipped;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    is3d::DevBuf<unsigned char> d_list, d_slot, d_occ, d_out;
    if (int rc = is3d::pair_occ_begin(d_occ, 0, is3d::pair_occ_words(*bins, n_events, n_slots))) return rc;
    const size_t out_words = is3d::pair_out_words(*bins, n_events, n_slots);
    HIP_TRY(d_out.alloc(out_words * sizeof(int64_t)));
    HIP_TRY(d_slot.upload(slot, (size_t)n_species));
    HIP_TRY(d_list.upload(particles, (size_t)n_particles));
    HIP_TRY(is3d::pair_cells_launch(*bins, is3d::pair_tables(*bins), n_events, n_slots, d_slot.as<int32_t>(), n_species, d_list.as<is3d_particle>(),
                                    n_particles, d_occ.as<unsigned>()));
    HIP_TRY(is3d::pair_correlate_launch(*bins, n_events, n_slots, d_occ.as<unsigned>(), d_out.as<unsigned long long>()));
    std::vector<int64_t> h(out_words);
    HIP_TRY(hipMemcpy(h.data(), d_out.p, out_words * sizeof(int64_t), hipMemcpyDeviceToHost));
    is3d::pair_hist_scatter(*bins, h.data(), hist, n_events, n_slots);
    return is3d::pair_hist_check(hist, n_events, n_slots);
}
