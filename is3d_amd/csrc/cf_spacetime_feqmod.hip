// cf_spacetime_feqmod.hip -- hand-written gfx950 kernels of operation 0 with the modified equilibrium (df_mode 3, 4).
//
// Replaces EmissionFunctionArray::calculate_dN_dX_feqmod (reference src/cpp/emissionfunction_smooth_kernels.cpp:1449-2135).  The per-cell
// integrand is that of the feqmod spectra path with the routine's own three departures, which cf_prep_feqmod<.., OP0 = true> and
// cf_feqmod_renorm<true> (cf_feqmod.hip) build into the records; the binning is cf_spacetime.hip's, unchanged.  Stages:
//   cf_prep_feqmod (OP0)   per-cell quadratic-form records of the plan's tile shape, fallback records of the breakdown cells
//   cf_feqmod_renorm (OP0) df_mode 3: |renorm| per (cell, class), 0 for the pairs the reference skips
//   cf_st_fq_cells         lanes <-> (species class, pT), loop over cells; the workgroup stages the cell's unit records in LDS once (the
//                          record operands are wave-uniform: one LDS broadcast read instead of a global load per lane), every lane sums
//                          w_phi p.dsigma f over (phi, y | eta), times w_pT, and a fixed xor tree over a class's pT lanes gives D[class][cell].
//                          2+1D: the same tree per eta node feeds the class's dN/dy deta partials (one row per class and workgroup).
//   cf_feqmod_compact      (cf_feqmod.hip) the ordered list of breakdown cells
//   cf_st_fq_linear        the linearised delta-f of the breakdown cells (:1938-1996): overwrites their D[class][cell] (the records are
//                          neutral there: 0) and writes its own eta partial slots, reduced after those of cf_st_fq_cells in a fixed order.
// No floating-point atomics: the results are bitwise the same from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cf_feqmod.h"
#include "cf_math.h"
#include "cf_spacetime.h"

namespace is3d {

// ------------------------------------------------------------------------------------------------
// cf_st_fq_cells.  Unit record (cf_feqmod.h): header jj < JT {B_j, gammaf_j, s2, s3} (s2 of jj = 0: alpha_B,mod; slots 3, 6, 7: min alphaf,
// min betaf, min gammaf of the unit), rows r < R in the slot order of fq_row_slots {A_k, alphaf_k, W_k, min_j betaf_jk} + betaf_jk.
// For a lane (mT, pT, sign, b) and its class's rn (df_mode 3: |renorm| of the cell; df_mode 4: 1, folded into A_k and W_k):
//   X^2 = mT^2 alphaf_k + mT pT betaf_jk + pT^2 gammaf_j,  f = z / (1 + sign z),  z = exp(b alpha_B,mod - X)
//   p.dsigma = rn (mT A_k + W_k pT B_j)   (outflow: max(p.dsigma, 0))
// A row is culled only when z == +0 for every lane and phi: its terms are exactly +0.
// ------------------------------------------------------------------------------------------------
constexpr int kStFqLds = 2048;   // doubles of unit records per staging batch (16 KiB)

template <bool DIM3, bool MODE3, bool BARYON, bool OUTFLOW, int JT, int R>
__global__ void __launch_bounds__(256) cf_st_fq_cells(const StFqCellArgs a)
{
    constexpr int HDR = 4 * JT;
    constexpr int RW = 4 + JT;
    constexpr int REC = HDR + R * RW;
    constexpr int NBU = kStFqLds / REC;   // units per staging batch
    static_assert(NBU >= 1 && REC % 2 == 0, "unit record too large for the staging buffer");
    constexpr FqRowSlots SL = fq_row_slots(DIM3);
    __shared__ double2 ubuf[NBU * REC / 2];
    extern __shared__ double st_eta[];   // 2+1D: [4 waves][64 / npTp classes][K], each row owned by the head lane of its class

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int grp = blockIdx.x % a.G, chunk = blockIdx.x / a.G;
    const int lw = grp * 4 + wave;
    const bool wave_on = lw < a.nlw;   // idle waves still stage and meet the barriers
    const int l = (wave_on ? lw : 0) * 64 + lane;
    const double mT = a.lane_mT[l], pT = a.lane_pT[l], sign = a.lane_sign[l], wpT = a.lane_wpT[l];
    const double bq = BARYON ? a.lane_b[l] : 0.0;
    const double mT2 = mT * mT, mTpT = mT * pT, pT2 = pT * pT;
    const int npTp = a.npTp, K = a.K;
    const int cls = l / npTp, ci = lane / npTp;
    const int clsc = cls < a.ncls ? cls : a.ncls - 1;
    const bool head = wave_on && (lane & (npTp - 1)) == 0 && cls < a.ncls;
    const int c0 = (int)(((int64_t)chunk * a.nc) / a.nch), c1 = (int)(((int64_t)(chunk + 1) * a.nc) / a.nch);
    const int nunits = a.jtiles * a.rblocks;
    double *eta_row = st_eta + ((size_t)wave * (64 / npTp) + ci) * K;
    if (!DIM3 && head)
        for (int k = 0; k < K; k++) eta_row[k] = 0.0;

    double wph[JT];
    for (int c = c0; c < c1; c++) {
        const double rn = MODE3 ? a.RN[(int64_t)c * a.ncls + clsc] : 1.0;   // one gather per (cell, lane)
        const double rmT = MODE3 ? rn * mT : mT, rpT = MODE3 ? rn * pT : pT;
        double tot = 0.0;
        double accj[JT];
#pragma unroll
        for (int jj = 0; jj < JT; jj++) accj[jj] = 0.0;
        for (int u0 = 0; u0 < nunits; u0 += NBU) {
            const int nb = min(NBU, nunits - u0);
            // stage units u0 .. u0 + nb of the cell (u = jt * rblocks + rb), 16 bytes per thread and trip
            __syncthreads();   // the previous batch has been read
            for (int i = tid; i < nb * (REC / 2); i += 256) {
                const int ub = i / (REC / 2), e2 = i - ub * (REC / 2);
                const int u = u0 + ub, jt = u / a.rblocks, rb = u - jt * a.rblocks;
                const int64_t unit = DIM3 ? (int64_t)(jt * a.rblocks + rb) * a.nc + c : ((int64_t)jt * a.nc + c) * a.rblocks + rb;
                ubuf[i] = ((const double2 *)(a.TS + unit * REC))[e2];
            }
            __syncthreads();
            if (!wave_on) continue;
            for (int ub = 0; ub < nb; ub++) {
                const int u = u0 + ub, jt = u / a.rblocks, rb = u - jt * a.rblocks;
                const double *__restrict__ U = (const double *)ubuf + ub * REC;
                if (rb == 0) {
#pragma unroll
                    for (int jj = 0; jj < JT; jj++) wph[jj] = a.wphi[jt * JT + jj];
                }
                double pTB[JT], pT2g[JT];
#pragma unroll
                for (int jj = 0; jj < JT; jj++) {
                    pTB[jj] = rpT * U[4 * jj + 0];
                    pT2g[jj] = pT2 * U[4 * jj + 1];
                }
                const double cm = BARYON ? bq * U[2] : 0.0;
                const double xcut = BARYON ? 745.25 + __builtin_fmax(cm, 0.0) : 745.25;   // exp(cm - X) == +0 beyond
                const double x2cut = BARYON ? xcut * xcut : 555400.0;
                const double gmin = pT2 * U[7];   // min_j pT^2 gammaf_j of the unit (pT^2 >= 0: monotone rounding)
                bool dead = false;
                if (DIM3 && a.zskip) dead = __all(__builtin_fma(mTpT, U[6], mT2 * U[3] + gmin) > x2cut);
                if (!dead) {
                    const double *__restrict__ rows = U + HDR;
                    for (int r = 0; r < R; r++) {
                        const double *__restrict__ row = rows + r * RW;
                        const double a2 = mT2 * row[SL.AL];
                        if (a.zskip && __all(__builtin_fma(mTpT, row[SL.BM], a2 + gmin) > x2cut)) continue;
                        const double mTA = rmT * row[SL.A], W = row[SL.W];
                        double rv = 0.0;
#pragma unroll
                        for (int jj = 0; jj < JT; jj++) {
                            double X = sqrt_g1(__builtin_fma(mTpT, row[4 + jj], a2 + pT2g[jj]));
                            // 2+1D: the rows sit at eta_scale eta_k with eta_scale = detA and no upper bound (:1847-1849), which the exponent-range
                            // bound of cf_prep_feqmod (cosh(max |eta_k|), right for the spectra's detA < 1) does not cover: X can pass exp_p9's
                            // |v| < 1.4e9 on a row that the wave-uniform cull keeps, or with the cull off.  e^-1e9 is the same +0 as e^-X there.
                            if (!DIM3) X = X > 1.0e9 ? 1.0e9 : X;
                            const double z = exp_p9(BARYON ? cm - X : -X);
                            const double w = z * rcp_nr(__builtin_fma(sign, z, 1.0));
                            double pds = __builtin_fma(pTB[jj], W, mTA);
                            if (OUTFLOW) pds = __builtin_fmax(pds, 0.0);
                            if (DIM3) accj[jj] = __builtin_fma(pds, w, accj[jj]);
                            else rv = __builtin_fma(wph[jj], pds * w, rv);
                        }
                        if (!DIM3) {
                            // this eta node's share of the class: w_pT-weighted, summed over the class's pT lanes by a fixed xor tree
                            tot += rv;
                            double e = wpT * rv;
                            for (int o = npTp >> 1; o > 0; o >>= 1) e += __shfl_xor(e, o);
                            const int k = rb * R + r;
                            if (head && k < K) eta_row[k] += e;
                        }
                    }
                }
                if (DIM3 && rb == a.rblocks - 1) {
#pragma unroll
                    for (int jj = 0; jj < JT; jj++) {
                        tot = __builtin_fma(wph[jj], accj[jj], tot);
                        accj[jj] = 0.0;
                    }
                }
            }
        }
        if (wave_on) {
            double v = wpT * tot;
            for (int o = npTp >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (head) a.D[(int64_t)cls * a.nc + c] = v;
        }
    }
    if (!DIM3 && head) {
        double *__restrict__ dst = a.eta_slab + ((int64_t)chunk * a.ncls + cls) * K;
        for (int k = 0; k < K; k++) dst[k] = eta_row[k];
    }
}

bool spacetime_feqmod_shape_supported(int dim3, int JT, int R) { return dim3 ? (JT == 8 && R == 7) : (JT == 8 && R == 31); }

size_t spacetime_feqmod_eta_lds(int dim3, int npTp, int K) { return dim3 ? 0 : sizeof(double) * 4 * (64 / npTp) * (size_t)K; }

template <bool DIM3, bool MODE3, bool BARYON, bool OUTFLOW>
static hipError_t launch_fq_cells_t(const StFqCellArgs &a, hipStream_t st)
{
    constexpr int JT = 8, R = DIM3 ? 7 : 31;
    hipLaunchKernelGGL((cf_st_fq_cells<DIM3, MODE3, BARYON, OUTFLOW, JT, R>), dim3((unsigned)(a.G * a.nch)), dim3(256),
                       spacetime_feqmod_eta_lds(DIM3, a.npTp, a.K), st, a);
    return hipGetLastError();
}

template <bool DIM3, bool MODE3>
static hipError_t launch_fq_cells_b(const StFqCellArgs &a, int baryon, int outflow, hipStream_t st)
{
    if constexpr (MODE3) {
        if (baryon) return outflow ? launch_fq_cells_t<DIM3, true, true, true>(a, st) : launch_fq_cells_t<DIM3, true, true, false>(a, st);
    }
    return outflow ? launch_fq_cells_t<DIM3, MODE3, false, true>(a, st) : launch_fq_cells_t<DIM3, MODE3, false, false>(a, st);
}

hipError_t launch_spacetime_feqmod_cells(const StFqCellArgs &a, int dim3, int mode3, int baryon, int outflow, int JT, int R, hipStream_t st)
{
    if (a.nc <= 0) return hipSuccess;
    if (!spacetime_feqmod_shape_supported(dim3, JT, R) || (baryon && !mode3)) return hipErrorInvalidValue;
    if (dim3) return mode3 ? launch_fq_cells_b<true, true>(a, baryon, outflow, st) : launch_fq_cells_b<true, false>(a, baryon, outflow, st);
    return mode3 ? launch_fq_cells_b<false, true>(a, baryon, outflow, st) : launch_fq_cells_b<false, false>(a, baryon, outflow, st);
}

// ------------------------------------------------------------------------------------------------
// cf_st_fq_linear: the linearised delta-f of the cells whose feqmod breaks down (df_mode 3), in the reference's form (:1938-1996): libm
// exp / cosh / sinh, lanes <-> (class, pT) as above, workgroup b of the GL slots takes the list entries b, b + GL, ... in order.  A class
// whose renormalisation failed the nan / inf test (RN == 0, cf_feqmod_renorm<true>) adds 0 (the test precedes the branch, :1881).
// D[class][cell] is written (the records of these cells are neutral: cf_st_fq_cells wrote 0); 2+1D: the slot's eta partials go to slab
// slot nch + b whether or not it had a cell, so that cf_st_eta_reduce adds every slot in a fixed order.
// ------------------------------------------------------------------------------------------------
enum { LFB_DAT = 0, LFB_DAX, LFB_DAY, LFB_DAN, LFB_UT, LFB_UX, LFB_UY, LFB_UN, LFB_TAU, LFB_ETA, LFB_T,
       LFB_PITT, LFB_PITX, LFB_PITY, LFB_PITN, LFB_PIXX, LFB_PIXY, LFB_PIXN, LFB_PIYY, LFB_PIYN, LFB_PINN,
       LFB_SHEAR, LFB_CA, LFB_CB, LFB_DETA, LFB_KIND, LFB_ALPHAB, LFB_B1, LFB_BER, LFB_IBV, LFB_VT, LFB_VX, LFB_VY, LFB_VN };   // cf_feqmod.hip::FbIdx

__global__ void __launch_bounds__(256) cf_st_fq_linear(const StFqLinearArgs a)
{
    extern __shared__ double st_eta[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int grp = blockIdx.x % a.G, b = blockIdx.x / a.G;
    const int lw = grp * 4 + wave;
    if (lw >= a.nlw) return;   // no barrier below
    const int l = lw * 64 + lane;
    const double mT = a.lane_mT[l], pT = a.lane_pT[l], sign = a.lane_sign[l], wpT = a.lane_wpT[l], mass = a.lane_mass[l];
    const double baryon = a.lane_b ? a.lane_b[l] : 0.0;
    const double mass2 = mass * mass;
    const int npTp = a.npTp, K = a.K;
    const int cls = l / npTp, ci = lane / npTp;
    const int clsc = cls < a.ncls ? cls : a.ncls - 1;
    const bool head = (lane & (npTp - 1)) == 0 && cls < a.ncls;
    double *eta_row = st_eta + ((size_t)wave * (64 / npTp) + ci) * K;
    if (!a.dim3 && head)
        for (int k = 0; k < K; k++) eta_row[k] = 0.0;
    const int n = *a.count;
    for (int e = b; e < n; e += a.GL) {
        const int cell = a.list[e];
        const double *fb = a.FB + (int64_t)cell * kFbRec;
        const bool on = a.mode != 3 || !a.RN || a.RN[(int64_t)cell * a.ncls + clsc] != 0.0;
        const double tau = fb[LFB_TAU], tau2 = tau * tau, T = fb[LFB_T];
        const double mT_over_tau = mT / tau;
        double tot = 0.0;
        for (int k = 0; k < K; k++) {
            const double y = a.dim3 ? a.kgrid[k] : 0.0;
            const double eta = a.dim3 ? fb[LFB_ETA] : a.kgrid[k];
            const double eta_weight = a.dim3 ? 1.0 : a.kweight[k];
            const double pt = mT * cosh(y - eta), pn = mT_over_tau * sinh(y - eta), tau2_pn = tau2 * pn;
            double rv = 0.0;
            for (int j = 0; j < a.J; j++) {
                const double px = pT * a.cosphi[j], py = pT * a.sinphi[j];
                const double pdotdsigma = eta_weight * (pt * fb[LFB_DAT] + px * fb[LFB_DAX] + py * fb[LFB_DAY] + pn * fb[LFB_DAN]);   // :1943
                if (!on || (a.outflow && pdotdsigma <= 0.0)) continue;
                const double pdotu = pt * fb[LFB_UT] - px * fb[LFB_UX] - py * fb[LFB_UY] - tau2_pn * fb[LFB_UN];
                const double pimunu_pmu_pnu = fb[LFB_PITT] * pt * pt + fb[LFB_PIXX] * px * px + fb[LFB_PIYY] * py * py + fb[LFB_PINN] * tau2_pn * tau2_pn
                    + 2.0 * (-(fb[LFB_PITX] * px + fb[LFB_PITY] * py) * pt + fb[LFB_PIXY] * px * py + tau2_pn * (fb[LFB_PIXN] * px + fb[LFB_PIYN] * py - fb[LFB_PITN] * pt));
                const double chem = (a.mode == 3) ? baryon * fb[LFB_ALPHAB] : 0.0;
                const double feq = 1.0 / (exp(pdotu / T - chem) + sign), feqbar = 1.0 - sign * feq;
                const double df_shear = fb[LFB_SHEAR] * pimunu_pmu_pnu / pdotu;
                double df;
                if (a.mode == 3) {
                    const double Vmu_pmu = fb[LFB_VT] * pt - fb[LFB_VX] * px - fb[LFB_VY] * py - fb[LFB_VN] * tau2_pn;
                    const double df_bulk = fb[LFB_CA] * pdotu + fb[LFB_B1] * baryon + fb[LFB_CB] * (pdotu - mass2 / pdotu);
                    const double df_diff = (fb[LFB_BER] - baryon / pdotu) * Vmu_pmu * fb[LFB_IBV];
                    df = feqbar * (df_shear + df_bulk + df_diff);
                } else df = feqbar * df_shear + fb[LFB_CA] + feqbar * fb[LFB_CB] * (pdotu - mass2 / pdotu);
                if (a.regulate) df = fmax(-1.0, fmin(df, 1.0));
                rv += a.wphi[j] * (pdotdsigma * (feq * (1.0 + df)));
            }
            tot += rv;
            if (!a.dim3) {
                double ev = wpT * rv;
                for (int o = npTp >> 1; o > 0; o >>= 1) ev += __shfl_xor(ev, o);
                if (head) eta_row[k] += ev;
            }
        }
        double v = wpT * tot;
        for (int o = npTp >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (head) a.D[(int64_t)cls * a.nc + cell] = v;
    }
    if (!a.dim3 && head) {
        double *__restrict__ dst = a.eta_slab + ((int64_t)(a.nch + b) * a.ncls + cls) * K;
        for (int k = 0; k < K; k++) dst[k] = eta_row[k];
    }
}

hipError_t launch_spacetime_feqmod_linear(const StFqLinearArgs &a, hipStream_t st)
{
    if (a.nc <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_st_fq_linear, dim3((unsigned)(a.G * a.GL)), dim3(256), spacetime_feqmod_eta_lds(a.dim3, a.npTp, a.K), st, a);
    return hipGetLastError();
}

}  // namespace is3d
