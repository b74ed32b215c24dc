// cf_spacetime.h -- operation 0 (smooth Cooper-Frye spacetime distributions): the launch entry points of cf_spacetime.hip,
// cf_spacetime_feqmod.hip and cf_spacetime_vah.hip, and the host driver that is3d_plan (cf_plan.cpp) and is3d_vah_plan (cf_vah.hip) share
// (cf_spacetime_host.cpp: state, setup, checks, weights, the pass loop around the plans' own records and per-cell launches, the one-shot wrapper).
#pragma once
#include "cf_device.h"
#include "cf_host.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <array>
#include <cstdint>
#include <functional>
#include <vector>
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

// ---- the two halves of an execute, for the cell-axis split over devices (cf_multi.hip) ----
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

// ---- the host driver of operation 0 (cf_spacetime_host.cpp), whichever plan it serves ----
// what a plan keeps for operation 0: the shape, the lane tables of the per-cell kernels (class-major, npTp lane slots per class, nlw waves),
// the weights now on the device and their host copies, and the workspaces; made by spacetime_setup on the first such execute
struct StState {
    bool ready = false;
    int ncls = 0, npT = 0, J = 0, K = 0, S = 0, dim3 = 1, nphi = 0;   // nphi = jtiles * JT slots of d_wphi
    int npTp = 0, nlw = 0;
    int64_t pass = 0;                                                  // cells per pass
    std::vector<double> hwpT, hwphi;                                   // the weights now on the device (d_wpT, d_wphi)
    DevBuf<double> d_mT, d_pT, d_sign, d_b, d_mass, d_wpT, d_wphi, d_pg, d_D, d_slab, d_eta;
    DevBuf<int32_t> d_cls;
    DevBuf<unsigned long long> d_counters;
    StBinWork bins;
};
// the lanes past the classes and past the pT grid (w_pT = 0) take part in the kernels' wave-wide tests:
// ST_PAD_UNIT: mT = 1, pT = 0, sign = 1, b = 0, mass = 1;  ST_PAD_REPEAT: class 0 / pT index 0 stand in for whichever of the two is past its end
enum StPad { ST_PAD_UNIT, ST_PAD_REPEAT };
struct StSetup {
    int ncls, npT, J, K, dim3, jtiles, JT, npart;
    const double *cls_mass, *cls_sign, *cls_bar;   // [ncls]; cls_bar may be NULL
    const double *pT_grid, *sp_deg;                // [npT], [npart]
    const int32_t *sp_cls;                         // [npart]
    double prefactor;
    int64_t bytes_per_cell, pass_cells, workspace_bytes;   // the plan's record stream; D (8 B per class and cell) shares its cap
    bool mass_lanes, b_lanes;                      // upload d_mass, d_b
    StPad pad;
};
int spacetime_setup(StState &s, const StSetup &a);
// the checks, none of which touches a device.  lds_cap_bytes: what the per-cell kernel has for its 2+1D eta rows
int spacetime_check_bins(const is3d_spacetime_bins *b, const double *x, const double *y);
int spacetime_check_grid(bool dim3, size_t lds_cap_bytes, int npT, int K);
int spacetime_check_out(const is3d_spacetime_out *out);
// the momentum weights of the reduction, uploaded when they differ from the state's copy (the first execute, or new weights; only then does
// the host wait for the stream)
int spacetime_upload_weights(StState &s, const double *pT_w, const double *phi_w, hipStream_t st);

// one execute.  Stage tags of the timer: 0 prep, 1 cells, 2 bins, 3 renormalisation, 4 linearised delta-f, 5 a shard's D blocks placed
using StMark = std::function<hipError_t(int)>;   // ends a timed interval of the given stage (nothing without stats)
struct StRun {
    StBinStage bs;                       // the caller's part: the device arrays of the n cells, x, y, n, bins, out, all_cells
    int linear_slots;                    // 2+1D: slab slots past the chunks' (cf_st_fq_linear), else 0
    const double *kweight;               // 2+1D: [K] effective eta weights
    int device;
    StSplit *split;                      // the halves of an execute; NULL: both
    hipStream_t stream;
    unsigned long long *d_status;        // the plan's 8 status words (cf_device.h), started here
    unsigned long long *d_sticky;        // may be NULL: launch_fold_status after an execute of n > 0 cells without stats
    unsigned long long *status;          // [8]: the status words, read back when stats != NULL
    is3d_spacetime_stats *stats;         // NULL: no timer, no read-back, the host does not wait
    double *ms_renorm, *ms_linear;       // stages 3 and 4 (may be NULL)
    // records and per-cell launch(es) of pass `pass`, cells [c0, c0 + nc), into d_D (2+1D: nch chunks' eta partials in d_slab, reduced into d_eta)
    std::function<int(int pass, int64_t c0, int32_t nc, int nch, const StMark &mark)> pass;
};
// fills stats' times, n_classes, n_passes and the four bin counters; bad_cell, code and n_cells_skipped are the caller's to decode from status
int spacetime_run(StState &s, const StRun &r);

// the one-shot entries: host cells, x, y and outputs through one device block each around `exec` (plan execute on the device copies, its
// stats into *stt); H2D and D2H times into stats.  keep(i): cell array i is staged.  S species, n_eta_eff eta points of dN_dydeta
template <class Cells, class Keep, class Exec>
int spacetime_oneshot(const Cells &cells, const double *x, const double *y, Keep keep, int S, int n_eta_eff, const is3d_spacetime_bins *bins,
                      const is3d_spacetime_out *out, is3d_spacetime_stats *stats, Exec exec)
{
    const int64_t n = cells.n_cells, tb = bins->tau_bins, rbn = bins->r_bins;
    const size_t narr = cell_arrays(cells).size();
    const size_t sizes[6] = {(size_t)S, (size_t)(S * tb), (size_t)(S * rbn), (size_t)(S * tb * rbn), (size_t)S * n_eta_eff,
                             out->dN_dy_cell ? (size_t)S * n : 0};
    double *host_out[6] = {out->dN_dy, out->dN_taudtaudy, out->dN_twopirdrdy, out->dN_twopitaurdtaudrdy, out->dN_dydeta, out->dN_dy_cell};
    size_t total = 0;
    for (size_t s : sizes) total += s;
    DevBuf<double> dcell, dout;
    HIP_TRY(dcell.alloc((size_t)std::max<int64_t>(n, 1) * (narr + 2)));   // the cell arrays, then x and y
    HIP_TRY(dout.alloc(total));
    hipEvent_t e[4] = {};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 4; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{e};
    for (auto &v : e) HIP_TRY(hipEventCreate(&v));
    HIP_TRY(hipEventRecord(e[0], nullptr));
    Cells dc;
    HIP_TRY(stage_cells(cells, keep, 0, n, dcell.p, nullptr, &dc));
    std::array<const double *, 2> xy = {x, y};
    HIP_TRY(stage_arrays(xy, 0, n, dcell.p + narr * (size_t)n, nullptr));
    HIP_TRY(hipEventRecord(e[1], nullptr));
    const double *dx = n > 0 ? xy[0] : dcell.p, *dy = n > 0 ? xy[1] : dcell.p;
    double *dev_out[6];
    size_t off = 0;
    for (int i = 0; i < 6; i++) { dev_out[i] = sizes[i] ? dout.p + off : nullptr; off += sizes[i]; }
    const is3d_spacetime_out dev{dev_out[0], dev_out[1], dev_out[2], dev_out[3], dev_out[4], dev_out[5]};
    is3d_spacetime_stats stt{};
    const int rc = exec(dc, dx, dy, dev, &stt);
    if (rc) { if (stats) *stats = stt; return rc; }
    HIP_TRY(hipEventRecord(e[2], nullptr));
    for (int i = 0; i < 6; i++)
        if (sizes[i]) HIP_TRY(hipMemcpyAsync(host_out[i], dev_out[i], sizes[i] * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipEventRecord(e[3], nullptr));
    HIP_TRY(hipEventSynchronize(e[3]));
    float h2d = 0, d2h = 0;
    HIP_TRY(hipEventElapsedTime(&h2d, e[0], e[1]));
    HIP_TRY(hipEventElapsedTime(&d2h, e[2], e[3]));
    stt.ms_h2d = h2d;
    stt.ms_d2h = d2h;
    stt.code = IS3D_OK;
    if (stats) *stats = stt;
    return IS3D_OK;
}

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
