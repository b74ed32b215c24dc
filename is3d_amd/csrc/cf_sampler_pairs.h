// cf_sampler_pairs.h -- the per-particle rule of the two-particle (delta y, delta phi) correlations: a particle maps to a cell (iy, iphi)
// of a rapidity-azimuth grid or to nothing.  Stated ONCE for the host (pairs_host.cpp: is3d_pairs_list) and the device
// (cf_sampler_pairs.hip, cf_decays_mc.hip).
//
// The arithmetic that decides a cell -- E + pz, E - pz, their ONE division, the sum of squares under the square root, the two products and
// the subtraction of the azimuth test, the comparisons -- is compiled with floating-point contraction OFF on both sides.  +, -, *, / and sqrt
// are correctly rounded on both sides; the rapidity edges and the bin directions are computed once on the host (pair_tables) and handed to
// the kernels as bits.  So host and device reach the same cell from the same particle bits, everywhere: no decision goes through log, atan2
// or any other libm function.  The two bisections below ARE the definition of the cell.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/is3d_amd.h"
#include "cf_sampler_bins.h"
#if defined(__HIP__) || defined(__HIPCC__)
#include "cf_host.h"
#endif

namespace is3d {

constexpr int kPairMaxBins = 64;       // n_y and n_phi at most

// edge[k] = exp(2 (-y_cut + k (2 y_cut / n_y))), k = 0..n_y: the rapidity edges as bounds on (E + pz) / (E - pz) = e^{2y};
// (dx, dy)[k] = (cos, sin)(2 pi k / n_phi), the four axis directions exactly (+-1, 0) and (0, +-1)
struct PairTables {
    double edge[kPairMaxBins + 1];
    double dx[kPairMaxBins], dy[kPairMaxBins];
};

inline PairTables pair_tables(const is3d_pair_bins &b)
{
    PairTables t;
    for (int k = 0; k <= kPairMaxBins; k++) t.edge[k] = 0.0;
    for (int k = 0; k < kPairMaxBins; k++) t.dx[k] = t.dy[k] = 0.0;
    if (!(b.n_y >= 1 && b.n_y <= kPairMaxBins && b.n_phi >= 4 && b.n_phi <= kPairMaxBins && b.n_phi % 4 == 0)) return t;
    const double w = 2.0 * b.y_cut / (double)b.n_y;
    for (int k = 0; k <= b.n_y; k++) t.edge[k] = exp(2.0 * (-b.y_cut + (double)k * w));
    const int q = b.n_phi / 4;
    for (int k = 0; k < b.n_phi; k++) {
        const double a = 2.0 * M_PI * (double)k / (double)b.n_phi;
        t.dx[k] = cos(a);
        t.dy[k] = sin(a);
    }
    t.dx[0] = 1.0;      t.dy[0] = 0.0;
    t.dx[q] = 0.0;      t.dy[q] = 1.0;
    t.dx[2 * q] = -1.0; t.dy[2 * q] = 0.0;
    t.dx[3 * q] = 0.0;  t.dy[3 * q] = -1.0;
    return t;
}

// y_cut > 0, pT_max > pT_min >= 0, 1 <= n_y <= 64, n_phi a multiple of 4 in 4..64, and edges that come out finite and strictly increasing
inline bool pair_bins_valid(const is3d_pair_bins &b)
{
    if (!(b.y_cut > 0.0 && b.pT_min >= 0.0 && b.pT_max > b.pT_min)) return false;                                   // (NaN: false)
    if (!(b.n_y >= 1 && b.n_y <= kPairMaxBins && b.n_phi >= 4 && b.n_phi <= kPairMaxBins && b.n_phi % 4 == 0)) return false;
    const PairTables t = pair_tables(b);
    for (int k = 0; k <= b.n_y; k++) {
        if (!(t.edge[k] > 0.0 && t.edge[k] <= 1.7976931348623157e308)) return false;
        if (k && !(t.edge[k] > t.edge[k - 1])) return false;
    }
    return true;
}

// the cell of one momentum: iy * n_phi + iphi, or -1 (adds nothing)
IS3D_BINS_HD int pair_cell(const is3d_pair_bins &b, const PairTables &t, double E, double px, double py, double pz)
{
    IS3D_BINS_NO_CONTRACT
    const double num = E + pz, den = E - pz;
    if (!(den > 0.0)) return -1;
    const double ratio = num / den;
    if (!(ratio >= t.edge[0] && ratio < t.edge[b.n_y])) return -1;               // (NaN compares false: no cell)
    const double px2 = px * px, py2 = py * py;
    const double pT = sqrt(px2 + py2);
    if (!(pT >= b.pT_min && pT < b.pT_max && pT > 0.0)) return -1;
    int lo = 0, hi = b.n_y;                                                      // the largest k with edge[k] <= ratio
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.edge[mid] <= ratio) lo = mid; else hi = mid;
    }
    const int iy = lo;
    // the quadrant from the signs (pT > 0: not both zero); its first direction is an axis and always passes the test below
    const int q = b.n_phi >> 2;
    const int quad = px > 0.0 && py >= 0.0 ? 0 : (px <= 0.0 && py > 0.0 ? 1 : (px < 0.0 && py <= 0.0 ? 2 : 3));
    lo = quad * q;
    hi = lo + q;                                                                 // the largest k of the quadrant with dir[k] x p >= 0
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const double a = t.dx[mid] * py, c = t.dy[mid] * px;
        if (a - c >= 0.0) lo = mid; else hi = mid;
    }
    return iy * b.n_phi + lo;
}

IS3D_BINS_HD int64_t pair_classes(int64_t n_slots) { return n_slots * (n_slots + 1) / 2; }
// class (a <= b)
IS3D_BINS_HD int64_t pair_class(int64_t a, int64_t b, int64_t n_slots) { return a * n_slots - a * (a - 1) / 2 + (b - a); }
IS3D_BINS_HD int64_t pair_hist_bins(const is3d_pair_bins &b) { return (int64_t)(2 * b.n_y - 1) * b.n_phi; }
IS3D_BINS_HD int64_t pair_grid_cells(const is3d_pair_bins &b) { return (int64_t)b.n_y * b.n_phi; }

// the argument checks of every pair entry (IS3D_EINVAL, no device use): null, sizes, bins, the slot map
int pair_check_args(const is3d_pair_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                    const is3d_pair_hist *hist);
void pair_hist_zero(const is3d_pair_bins &b, const is3d_pair_hist *h, int32_t n_events, int32_t n_slots);
// the device's out block same | mixed | M (host copy) -> the caller's three arrays
void pair_hist_scatter(const is3d_pair_bins &b, const int64_t *block, const is3d_pair_hist *h, int32_t n_events, int32_t n_slots);
// IS3D_EDOMAIN for an M[e][s] above IS3D_SAMPLER_VN_MAX_COUNT
int pair_hist_check(const is3d_pair_hist *h, int32_t n_events, int32_t n_slots);

#if defined(__HIP__) || defined(__HIPCC__)
// The device block of a run: occ[event][slot][iy][iphi], 32-bit counts, zeroed once per run and kept across event batches (mixing needs
// event e + 1).  IS3D_ENOMEM naming its size when it cannot be allocated.
inline size_t pair_occ_words(const is3d_pair_bins &b, int32_t n_events, int32_t n_slots)
{
    return (size_t)n_events * (size_t)n_slots * (size_t)pair_grid_cells(b);
}
// one accepted particle: ONE 32-bit add (global memory: the adds of an event spread over n_slots * n_y * n_phi words)
__device__ __forceinline__ void pair_add(const is3d_pair_bins &b, unsigned *occ, int n_slots, int ev, int s, int cell)
{
    atomicAdd(&occ[((int64_t)ev * n_slots + s) * pair_grid_cells(b) + cell], 1u);
}
// cf_pair_cells: n particles of a DEVICE list (any order) added into occ_dev on the null stream; a particle whose species or event is out
// of range adds nothing
hipError_t pair_cells_launch(const is3d_pair_bins &b, const PairTables &t, int n_events, int n_slots, const int32_t *slot_dev, int n_species,
                             const is3d_particle *particles_dev, int64_t n, unsigned *occ_dev);
// cf_pair_correlate: occ_dev -> out_dev = same [n_classes][2 n_y - 1][n_phi] | mixed (the same shape) | M [n_events][n_slots], 64-bit words
// that this call zeroes first, on the null stream
inline size_t pair_out_words(const is3d_pair_bins &b, int32_t n_events, int32_t n_slots)
{
    return 2 * (size_t)pair_classes(n_slots) * (size_t)pair_hist_bins(b) + (size_t)n_events * (size_t)n_slots;
}
hipError_t pair_correlate_launch(const is3d_pair_bins &b, int n_events, int n_slots, const unsigned *occ_dev, unsigned long long *out_dev);
// allocates (grows) and zeroes an occupancy block of `words` 32-bit words at the front of d after `head_bytes` bytes (zeroed too)
int pair_occ_begin(DevBuf<unsigned char> &d, size_t head_bytes, size_t words);
#endif

}  // namespace is3d
