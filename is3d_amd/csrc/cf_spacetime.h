// cf_spacetime.h -- launch entry points of cf_spacetime.hip (operation 0: smooth Cooper-Frye spacetime distributions).
#pragma once
#include "cf_device.h"
#include "cf_host.h"
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <functional>
#include "../../include/is3d_amd.h"
namespace is3d {

// operation 0 with the modified equilibrium (cf_spacetime_feqmod.hip): the per-cell stage on cf_prep_feqmod's OP0 records of one pass of nc
// cells (3+1D 8 x 7, 2+1D 8 x 31), D[cls * nc + cell] = sum_pT w_pT sum_phi w_phi sum_(y | eta) p.dsigma f; 2+1D: eta_slab[chunk][cls][k]
struct StFqCellArgs {
    const double *TS;
    int32_t nc, J, K, jtiles, rblocks;
    int32_t ncls, npTp, nlw, G, nch;
    int32_t zskip;
    const double *lane_mT, *lane_pT, *lane_sign, *lane_b, *lane_wpT;   // [nlw * 64]
    const double *wphi;                                                // [jtiles * JT], 0 past J
    const double *RN;                                                  // df_mode 3: [nc][ncls] |renorm| (cf_feqmod_renorm<true>)
    double *D;                                                         // [ncls][nc]
    double *eta_slab;                                                  // 2+1D: [nch + GL][ncls][K]
};
// the breakdown cells of a pass (cf_feqmod_compact's list): D of those cells, 2+1D eta partials into slab slots nch .. nch + GL - 1
struct StFqLinearArgs {
    const double *FB;
    const int32_t *list, *count;
    const double *lane_mT, *lane_pT, *lane_sign, *lane_mass, *lane_b, *lane_wpT;   // lane_b: include_baryon, else NULL
    const double *cosphi, *sinphi, *wphi, *kgrid, *kweight;
    const double *RN;                                                  // df_mode 3
    int32_t nc, J, K, ncls, npTp, nlw, G, GL, nch;
    int32_t dim3, mode, outflow, regulate;
    double *D, *eta_slab;
};
bool spacetime_feqmod_shape_supported(int dim3, int JT, int R);
size_t spacetime_feqmod_eta_lds(int dim3, int npTp, int K);
hipError_t launch_spacetime_feqmod_cells(const StFqCellArgs &a, int dim3, int mode3, int baryon, int outflow, int JT, int R, hipStream_t st);
hipError_t launch_spacetime_feqmod_linear(const StFqLinearArgs &a, hipStream_t st);

// per-cell stage: lanes <-> (class, pT) with npTp (a power of two <= 64) lane slots per class; reads the unit-record stream TS that cf_prep
// wrote for one pass of nc cells and writes D[cls * nc + cell] = unscale * sum_pT w_pT sum_phi w_phi sum_(y | eta) p.dsigma f
// (prefactor and degeneracy not applied).  2+1D: eta_slab[chunk][cls][k] receives the chunk's (cls, eta node) partials.
struct StCellArgs {
    const double *TS;
    int32_t nc, J, K, jtiles, rblocks;
    int32_t ncls, npTp, nlw, G, nch;
    int32_t outflow, regulate, zskip;
    const double *lane_mT, *lane_pT, *lane_sign, *lane_b, *lane_wpT;   // [nlw * 64]
    const double *wphi;                                                // [jtiles * JT], 0 past J
    const unsigned long long *pds_bound;                               // bits of the stream's p.dsigma bound (cf_pds_bound)
    double *D;                                                         // [ncls][nc]
    double *eta_slab;                                                  // 2+1D: [nch][ncls][K]
};
bool spacetime_shape_supported(int dim3, int JT, int R);
hipError_t launch_spacetime_cells(const StCellArgs &a, int ce, int dim3, int baryon, int JT, int R, hipStream_t st);
// 2+1D: eta_cls[cls][k] (+)= sum over the nch chunks of eta_slab, in chunk order
hipError_t launch_spacetime_eta_reduce(const double *eta_slab, int nch, int64_t n_per_chunk, int first_pass, double *eta_cls, hipStream_t st);
// 2+1D, several shards: eta_cls[i] = parts[0][i] + parts[1][i] + ..., left to right in shard order
hipError_t launch_spacetime_eta_shards(const double *parts, int nparts, int64_t n_per_part, double *eta_cls, hipStream_t st);
// dN_dydeta[s][k] = (pg[s] * eta_cls[cls[s]][k]) / w[k]
hipError_t launch_spacetime_eta_final(const double *eta_cls, const int32_t *cls, const double *pg, const double *w, int S, int K, double *out,
                                      hipStream_t st);

// operation 0 for anisotropic hydro (cf_spacetime_vah.hip): the per-cell stage on cf_prep_vah's "F" records of one pass of nc cells (3+1D 8 x 7,
// 2+1D 8 x 31), D[cls * nc + cell] = sum_pT w_pT sum_phi w_phi sum_(y | eta) p.dsigma f_a (1 + fbar_a df); 2+1D: eta_slab[chunk][cls][k]
struct StVahCellArgs {
    const double *TS;
    int32_t nc, J, K, jtiles, rblocks;
    int32_t ncls, npTp, nlw, G, nch;
    int32_t zskip;
    const double *lane_mT, *lane_pT, *lane_sign, *lane_wpT;            // [nlw * 64]
    const double *wphi;                                                // [jtiles * JT], 0 past J
    double *D;                                                         // [ncls][nc]
    double *eta_slab;                                                  // 2+1D: [nch][ncls][K]
};
bool spacetime_vah_shape_supported(int dim3, int JT, int R);
hipError_t launch_spacetime_vah_cells(const StVahCellArgs &a, int dim3, int regulate, int JT, int R, hipStream_t st);

// bin stage: keys of every cell (tau bin, r bin, (tau, r) bin; -1 outside), counters[0..3] += live cells (u.dsigma > 0, the reference's
// test at :1170; all_cells != 0: every cell -- anisotropic hydro skips none) with tau bin outside [0, bins), r bin outside, tau bin < 0, r bin < 0
hipError_t launch_spacetime_keys(const double *tau, const double *ux, const double *uy, const double *un, const double *dat, const double *dax,
                                 const double *day, const double *dan, const double *x, const double *y, int64_t n, double tau_min, double dtau, int tau_bins,
                                 double r_min, double dr, int r_bins, int32_t *key_tau, int32_t *key_r, int32_t *key_tr,
                                 unsigned long long *counters, int all_cells, hipStream_t st);
// stable counting sort of the cells by key: list[start[b] .. start[b + 1]) = the cells of bin b in ascending index order.
// cnt: [ntile][B] ints of scratch, tot: [B], start: [B + 1]
int spacetime_sort_tiles(int64_t n, int64_t B);
hipError_t launch_spacetime_sort(const int32_t *key, int64_t n, int64_t B, int ntile, int32_t *cnt, int32_t *tot, int64_t *start, int32_t *list,
                                 hipStream_t st);
// out[s * nseg + seg] (first_pass ? 0 : out) + sum, left to right over the segment's cells c in [c0, c0 + nc) in ascending order, of
// pg[s] * D[cls[s] * nc + (c - c0)], each product one rounding, each sum one rounding.  list == nullptr: one segment, all cells.
hipError_t launch_spacetime_segsum(const double *D, int64_t nc, int64_t c0, const int32_t *cls, const double *pg, int S, const int64_t *start,
                                   const int32_t *list, int64_t nseg, int first_pass, double *out, hipStream_t st);
// per_cell[s * n_total + c0 + i] = pg[s] * D[cls[s] * nc + i]
hipError_t launch_spacetime_per_cell(const double *D, int64_t nc, int64_t c0, int64_t n_total, const int32_t *cls, const double *pg, int S,
                                     double *per_cell, hipStream_t st);

// ---- the bin stage over plain device arrays (is3d_plan and is3d_vah_plan alike): keys and the stable sort of every histogram once per
// execute (begin), then blocks of D, cells [c0, c0 + nc) in ascending order, onto the running sums (add) ----
struct StBinWork {   // scratch of the sorts, grown on demand and kept by the plan
    DevBuf<int32_t> keys, cnt, tot, list;
    DevBuf<int64_t> start;
};
struct StBinStage {
    const double *tau, *ux, *uy, *un, *dat, *dax, *day, *dan, *x, *y;   // [n]: bin keys and the u.dsigma test of the counters
    int64_t n;
    const int32_t *cls;                                                 // [S] species -> class row of D
    const double *pg;                                                   // [S] prefactor x degeneracy
    int32_t S, all_cells;                                               // all_cells: see launch_spacetime_keys
    const is3d_spacetime_bins *bins;
    const is3d_spacetime_out *out;
    unsigned long long *counters;                                       // [4], zeroed by the caller
    // set by spacetime_bins_begin
    int32_t *lists[3];
    int64_t *starts[3], Bs[3];
    double *hout[3];
};
int spacetime_bins_begin(StBinWork &w, StBinStage &s, hipStream_t st);
// D: [class][nc]; first != 0 starts the sums, otherwise they continue from out
int spacetime_bins_add(const StBinStage &s, const double *D, int64_t nc, int64_t c0, int first, hipStream_t st);

// ---- the two halves of an execute, for the cell-axis split over devices (cf_multi.hip; defined in cf_plan.cpp) ----
// ST_CELLS: records and the per-cell stage of a shard's cells; every pass's D block [class][nc] lands in D_full[class][n_total] at cell
//           c_off + c0 (a 2-D copy on D_device, row-wise hipMemcpyPeerAsync from another device); in 2+1D the shard's class rows of
//           dN/dy deta stay in the plan (plan_st_eta).  No keys, no sort, no sums; bins, x, y and out are not read.
// ST_BINS:  keys, sort, segment sums, dN_dy walk and dN_dy_cell over the assembled D_full of all n_total = cells->n_cells cells, which only
//           need tau, u and dsigma; 2+1D: dN_dydeta from the plan's class rows as the caller left them (plan_st_eta).
enum { ST_CELLS = 1, ST_BINS = 2 };
struct StSplit {
    int role = 0;
    double *D_full = nullptr;
    int D_device = 0;
    int64_t n_total = 0, c_off = 0;
    // df_mode 1 / 2: the shard's |p.dsigma| bound (bits) goes in, the bound of the whole surface comes out; called once, before the records
    std::function<int(unsigned long long, unsigned long long *)> exchange;
};
int spacetime_execute_split(is3d_plan *plan, const is3d_cells *cells, const double *x, const double *y, const double *pT_w, const double *phi_w,
                            const is3d_spacetime_bins *bins, const is3d_spacetime_out *out, void *hip_stream, is3d_spacetime_stats *stats,
                            StSplit *split);
// the argument checks of the one-shot entries of operation 0, none of which touches a device (fq == NULL: df_mode 1 / 2)
int spacetime_check_args(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species, const is3d_grid *grid,
                         const double *pT_w, const double *phi_w, const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts,
                         const is3d_spacetime_bins *bins, const is3d_spacetime_out *out);
int plan_classes(const is3d_plan *plan);      // species classes (rows of D)
double *plan_st_eta(const is3d_plan *plan);   // 2+1D: [classes][n_eta] class rows of dN/dy deta on the plan's device (after a spacetime execute)
}  // namespace is3d
