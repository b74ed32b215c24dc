// cf_polzn.h -- launch entry points of cf_polzn.hip (spin polarization from thermal vorticity, mode 5).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

#include "../../include/is3d_amd.h"
namespace is3d {

// per-chunk stage: lanes <-> (class, pT) with npTp (a power of two <= 64) lane slots per class; the workgroup's tile of JT phi x KT y bins
// (2+1D: JT phi, every eta node summed), the loop over the chunk's cells wave-uniform.  slab[((chunk * 5 + mu) * NB + bin) * (nlw * 64) + lane],
// bin = iphi + n_phi * iy, mu = t, x, y, n (without the -1 / (4 m) of the class), norm.
struct PolznArgs {
    const double *tau, *eta, *ux, *uy, *un, *dat, *dax, *day, *dan;
    const double *wtx, *wty, *wtn, *wxy, *wxn, *wyn;
    int32_t n_cells, nch, nlw, ntj, ntk, J, K;   // K: y nodes (3+1D) | eta nodes (2+1D)
    double invT;
    const double *lane_mT, *lane_pT, *lane_sign;  // [nlw * 64]
    const double *cphi, *sphi;                    // [ntj * JT], clamped copies past J
    const double *ka, *kb, *kw;                   // 3+1D: e^y, e^-y [ntk * KT] clamped; 2+1D: cosh(eta_k), -sinh(eta_k), eta_w[k] deta [K]
    double *slab;
    int64_t NB;                                   // n_phi * n_y_eff
};
constexpr int kPolznJT3 = 4, kPolznKT3 = 3, kPolznJT2 = 8;
hipError_t launch_polzn_cells(const PolznArgs &a, int three_d, hipStream_t st);
// out_mu[i] = scale_mu(s) * sum over the nch chunks, in chunk order, of slab[chunk][mu][bin][cls(s) * npTp + ipT], i = s + S (ipT + npT bin);
// scale = -1 / (4 m_s) for t, x, y, n and 1 for norm
hipError_t launch_polzn_reduce(const double *slab, int nch, int64_t NB, int64_t Lp, const int32_t *cls, const double *scale, int S, int npT,
                               int npTp, double *St, double *Sx, double *Sy, double *Sn, double *Snorm, hipStream_t st);

// ---- the cell-axis split over several devices (is3d_spin_polarization_multi, cf_multi.hip) ----
// V[i] = sum over the nch chunks, in chunk order, of slab[chunk * per + i], i < per = 5 * NB * Lp: a shard's class-lane sums, bit for bit the
// v that cf_polzn_reduce forms before it scales (the same additions from the same 0.0), not expanded to species
hipError_t launch_polzn_class_sums(const double *slab, int nch, int64_t per, double *V, hipStream_t st);
// out_mu[i] = scale_mu(s) * ((V_0 + V_1) + V_2 ...) over the n_sh class-lane arrays stage[k * per + ...], in that order (n_sh == 0: zeros),
// indexed and scaled as launch_polzn_reduce does
hipError_t launch_polzn_shards(const double *stage, int n_sh, int64_t NB, int64_t Lp, const int32_t *cls, const double *scale, int S, int npT,
                               int npTp, double *St, double *Sx, double *Sy, double *Sn, double *Snorm, hipStream_t st);
}  // namespace is3d

struct is3d_polarization_plan;
namespace is3d {
// every argument check of is3d_spin_polarization, in its order; no device is used
int polzn_check_args(const is3d_cells *cells, const is3d_vorticity *w, const is3d_species *species, const is3d_grid *grid, double T,
                     const is3d_options *opts, const is3d_polarization_out *out);
int polzn_plan_classes(const is3d_polarization_plan *P);
int64_t polzn_plan_output_size(const is3d_polarization_plan *P);      // S * npT * NB: the length of each of the five outputs
int64_t polzn_plan_class_sum_size(const is3d_polarization_plan *P);   // 5 * NB * Lp doubles
// a shard's half of the execute: the cells kernel over DEVICE cells and vorticity with the chunk count of this many cells, then the class-lane
// sums into V (device, polzn_plan_class_sum_size doubles) on st; synchronises st and fills stats (code, n_classes, n_chunks, ms_cells, ms_reduce)
int polzn_plan_class_sums(is3d_polarization_plan *P, const is3d_cells *cells, const is3d_vorticity *w, double T, double *V, hipStream_t st,
                          is3d_polarization_stats *stats);
// the shards' class-lane sums (n_sh arrays next to each other on the plan's device) added in that order and expanded to species with the
// plan's class index and scale tables; out: DEVICE arrays; enqueued on st
int polzn_plan_combine(is3d_polarization_plan *P, const double *stage, int n_sh, const is3d_polarization_out *out, hipStream_t st);
}  // namespace is3d
