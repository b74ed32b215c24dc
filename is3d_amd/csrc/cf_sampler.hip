// cf_sampler.hip -- particle sampler (operation = 2) on the device: SURVEY.md 8f rank 4.
//
// Device path of EmissionFunctionArray::sample_dN_pTdpTdphidy
// (/root/reference/src/cpp/emissionfunction_sampling_kernels.cpp:833-1225) for viscous hydro, df_mode 1-4 (linear delta-f with
// its viscous weight; modified equilibrium with momentum rescaling), regular and "fast" mode, include_baryon = 1 in regular
// mode for df_mode 1-3 (chemical potential, bulk1 / diffusion terms, diffusion in the momentum rescaling); helpers
// max_particle_number / fast_max_particle_number (:239-359), sample_momentum (:456-617), compute_df_weight (:361-453),
// rescale_momentum (:619-650), does_feqmod_breakdown (emissionfunction.cpp:109-150), Milne_Basis / Surface_Element_Vector /
// boost_pimunu_to_lrf (viscous_correction.cpp:8-115), boost_pLRF_to_lab_frame (emissionfunction.cpp:40-51).
//
// The reference walks the cells serially and feeds five std::default_random_engine streams through implementation-defined
// std:: distributions; that order dependence cannot (and need not) be reproduced.  Here every (cell, event, stream) owns a
// counter-based Philox4x32-10 sequence (Salmon et al., SC'11): key = the 64-bit seed, counter = (block, stream, global cell
// index, event); streams 0..4 = hadron number, species, momentum, keep test, rapidity (the roles of the reference's five
// engines, :846-850); u = ((a >> 5) 2^26 + (b >> 6)) 2^-53 from two consecutive 32-bit outputs; Poisson numbers by
// sequential-search inversion in chunks of mean <= 256; species and the heavy-hadron K mixture by inversion of the cumulative
// weights; cos(theta) = 2u - 1.  The hadrons of a cell therefore depend on nothing but (seed, global cell index, event): any
// launch geometry, any cell sharding over GPUs and any event batching give the same particle list.
//
//   cf_sampler_density  thread <-> (cell, species class): 32-point Gauss-Laguerre equilibrium density integral
//   cf_sampler_cells    thread <-> cell: LRF basis, dsigma and pi^{mu nu} in the LRF, delta-f coefficients, mean hadron number
//   cf_sampler_poisson  thread <-> (event, cell): the Poisson number only.  A few per cent of the pairs emit anything, but nearly
//                       every wave holds one that does: sampling right here would drag 64 lanes through the rejection loops
//                       of one.  hipCUB compacts the emitting pairs into a dense, ordered list instead.
//   cf_sampler_run      thread <-> emitting (event, cell) pair: species, momentum rejection loop, viscous and flux weights, keep
//                       test; pass 1 counts, an exclusive scan turns counts into offsets, pass 2 replays the same streams and
//                       writes the particles -- the list comes out ordered by (event, cell, draw), no atomics, no sort.
//   cf_sampler_fused    the same pairs sampled once and binned where they are sampled, without a list
// The last two and the per-pair loop they run are cf_sampler_common.h's, instantiated here with ViscousModel.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_device.h"
#include "cf_host.h"
#include "cf_math.h"
#include "cf_plan_geometry.h"
#include "cf_sampler_bins.h"
#include "cf_sampler_flow.h"
#include "cf_sampler_flow_diff.h"
#include "cf_sampler_pairs.h"
#include "cf_sampler_hbt.h"
#include "cf_decays_mc.h"
#include "cf_sampler_common.h"
#include "errors.h"
#include "jonah.h"
#include "spline.h"

namespace is3d {

// GT[cell][class] = the n_eq integral; GT2 (df_mode 3, regular mode) = the J20 integral of n_linear, GT3 (with include_baryon) its
// J10 integral; muB_fo != NULL (include_baryon && include_baryondiff_deltaf): chem = baryon mu_B / T
// The integrands are those of gt_neq / gt_J20 / gt_J10 above with the node-only factors taken out and tabulated once per workgroup
// (c1 = w p e^p for the alpha = 1 nodes, c2 = w e^p for the alpha = 2 nodes: one exponential per node and integral instead of two), and with
// exp_full / sqrt_nr / rcp_nr of cf_math.h (1e-15 relative; arguments of order 1 .. 1e3) in place of libm's exp, sqrt and the division -- as
// cf_feqmod_renorm does since round 3: 3.3 -> ~1 ms per 1e6 cells x 75 classes.  An exponential that overflowed is held at 1e300 so that its
// node adds < 1e-300 of its weight instead of a division by inf.
__global__ void __launch_bounds__(256)
cf_sampler_density(const double *__restrict__ T_fo, const double *__restrict__ muB_fo, int64_t n_cells, SamplerSpecies sp,
                   const double *__restrict__ gl, int ngl, double *__restrict__ GT, double *__restrict__ GT2, double *__restrict__ GT3)
{
    __shared__ double l_p1[kSmpGlMax], l_c1[kSmpGlMax], l_p2[kSmpGlMax], l_c2[kSmpGlMax];
    for (int k = threadIdx.x; k < ngl; k += blockDim.x) {
        const double p1 = gl[k];
        l_p1[k] = p1 * p1; l_c1[k] = gl[ngl + k] * (p1 * exp(p1));
        if (GT2) { const double p2 = gl[2 * ngl + k]; l_p2[k] = p2 * p2; l_c2[k] = gl[3 * ngl + k] * exp(p2); }
    }
    __syncthreads();
    // class-major, GT[class][cell]: the lanes of a wave are consecutive cells of ONE class -- T_fo and the stores coalesce, the class constants
    // are wave-uniform -- and the readers (thread <-> cell) read a class's value of consecutive cells as one run
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_cells * sp.ncls) return;
    const int c = (int)(idx / n_cells);
    const int64_t cell = idx - (int64_t)c * n_cells;
    const double T = T_fo[cell];
    const double mbar = sp.cls_mass[c] / T, mb2 = mbar * mbar, sign = sp.cls_sign[c];
    const double alphaB = muB_fo ? muB_fo[cell] / T : 0.0;
    const double chem = sp.cls_baryon ? sp.cls_baryon[c] * alphaB : 0.0;
    double s_neq = 0.0, s_j10 = 0.0, s_j20 = 0.0;
    for (int k = 0; k < ngl; k++) {
        const double e = __builtin_fmin(exp_full(sqrt_nr(l_p1[k] + mb2) - chem), 1.0e300), r = rcp_nr(e + sign);
        s_neq = __builtin_fma(l_c1[k], r, s_neq);
        if (GT3) s_j10 = __builtin_fma(l_c1[k], (e * r) * r, s_j10);
    }
    GT[idx] = s_neq;
    if (GT3) GT3[idx] = s_j10;
    if (GT2) {
        for (int k = 0; k < ngl; k++) {
            const double E2 = sqrt_nr(l_p2[k] + mb2), e2 = __builtin_fmin(exp_full(E2 - chem), 1.0e300), r2 = rcp_nr(e2 + sign);
            s_j20 = __builtin_fma(l_c2[k], E2 * ((e2 * r2) * r2), s_j20);
        }
        GT2[idx] = s_j20;
    }
}

// The cell's n_eq integrals are summed over the SPECIES in list order (the order the reference adds them in).  With GT[cell][class] that was 305
// gathers per lane from rows 600 B apart -- 3.0 of the kernel's 3.1 ms (64 cache lines per load instruction); staged through LDS (38 KB per 64
// cells: four waves per CU) 1.75 ms; with the class-major tables a lane's read of class k is word `cell` of row k: consecutive lanes, one run,
// no LDS, full occupancy.  Same values, same order of additions.
__global__ void __launch_bounds__(128)
cf_sampler_cells(SamplerParams p, SamplerSpecies sp, const double *__restrict__ GT, const double *__restrict__ GT2,
                 const double *__restrict__ GT3, SamplerCell *__restrict__ out)
{
    const int64_t ic = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ic >= p.n_cells) return;
    SamplerCell c;
    memset(&c, 0, sizeof c);
    const double tau = p.cells.tau[ic], tau2 = tau * tau;
    const double dat = p.cells.dat[ic], dax = p.cells.dax[ic], day = p.cells.day[ic], dan = p.cells.dan[ic];
    const double ux = p.cells.ux[ic], uy = p.cells.uy[ic], un = p.cells.un[ic];
    const double ut = sqrt(1.0 + ux * ux + uy * uy + tau2 * un * un);
    const double udsigma = ut * dat + ux * dax + uy * day + un * dan;
    if (udsigma <= 0.0) {                                                          // :899
        atomicAdd(&p.status[1], 1ULL);
        out[ic] = c;
        return;
    }
    const double T = p.cells.T[ic], P = p.cells.P[ic], E = p.cells.E[ic];
    double muB = 0.0, nB = 0.0, Vt = 0.0, Vx = 0.0, Vy = 0.0, Vn = 0.0;               // :942-964
    if (p.baryon && p.baryondiff) {
        muB = p.cells.muB[ic]; nB = p.cells.nB[ic]; Vx = p.cells.Vx[ic]; Vy = p.cells.Vy[ic]; Vn = p.cells.Vn[ic];
        Vt = (Vx * ux + Vy * uy + tau2 * Vn * un) / ut;
        c.alphaB = muB / T;
        c.ber = nB / (E + P);
    }
    double bl[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (p.baryon ? !bilinear5(p.bil, T, muB, bl) : !(T >= p.spl.x[0] && T <= p.spl.x[p.spl.n - 1])) {   // exit(-1) / GSL domain error in the reference
        atomicMin(&p.status[0], (unsigned long long)(p.first_cell + ic));
        memset(&c, 0, sizeof c);
        out[ic] = c;
        return;
    }
    const double ut2 = ut * ut, ux2 = ux * ux, uy2 = uy * uy;
    const double uperp = sqrt(ux * ux + uy * uy), utperp = sqrt(1.0 + ux * ux + uy * uy);
    double pitt = 0, pitx = 0, pity = 0, pitn = 0, pixx = 0, pixy = 0, pixn = 0, piyy = 0, piyn = 0, pinn = 0;
    if (p.include_shear) {                                                          // :922-934
        pixx = p.cells.pixx[ic]; pixy = p.cells.pixy[ic]; pixn = p.cells.pixn[ic]; piyy = p.cells.piyy[ic]; piyn = p.cells.piyn[ic];
        pinn = (pixx * (ux2 - ut2) + piyy * (uy2 - ut2) + 2.0 * (pixy * ux * uy + tau2 * un * (pixn * ux + piyn * uy))) / (tau2 * utperp * utperp);
        pitn = (pixn * ux + piyn * uy + tau2 * pinn * un) / ut;
        pity = (pixy * ux + piyy * uy + tau2 * piyn * un) / ut;
        pitx = (pixx * ux + pixy * uy + tau2 * pixn * un) / ut;
        pitt = (pitx * ux + pity * uy + tau2 * pitn * un) / ut;
    }
    double bulkPi = p.include_bulk ? p.cells.bulkPi[ic] : 0.0;
    const double T4 = T * T * T * T;
    const int nT = p.spl.n;
    double lambda = 0.0;
    if (p.baryon) {                                                                 // deltafReader.cpp:436-468 (bilinear branch)
        const double T3 = T * T * T;
        if (p.df_mode == 1) { c.c0 = bl[0] / T4; c.c1 = bl[1] / T3; c.c2 = bl[2] / T4; c.c3 = bl[3] / T4; c.c4 = bl[4] / (T4 * T); }
        else { c.F = bl[0] * T; c.G = bl[1]; c.betabulk = bl[2] * T4; c.betaV = bl[3] * T3; c.betapi = bl[4] * T4; }
    } else if (p.df_mode == 1) {                                                    // deltafReader.cpp:337-344
        c.c0 = spline_eval_lds(nT, p.spl.x, p.spl.y[0], p.spl.c[0], T) / T4;
        c.c2 = spline_eval_lds(nT, p.spl.x, p.spl.y[1], p.spl.c[1], T) / T4;
    } else if (p.df_mode <= 3) {                                                    // :352-358
        c.F = spline_eval_lds(nT, p.spl.x, p.spl.y[0], p.spl.c[0], T) * T;
        c.betabulk = spline_eval_lds(nT, p.spl.x, p.spl.y[1], p.spl.c[1], T) * T4;
        c.betapi = spline_eval_lds(nT, p.spl.x, p.spl.y[2], p.spl.c[2], T) * T4;
    } else {                                                                        // :966-972, deltafReader.cpp:364-384
        if (bulkPi <= -P) bulkPi = -(1.0 - 1.e-5) * P;
        else if (bulkPi / P >= p.bp_max) bulkPi = P * (p.bp_max - 1.e-5);
        const double r = bulkPi / P;
        if (!(r >= p.jx[0] && r <= p.jx[p.nj - 1])) {
            atomicMin(&p.status[0], (unsigned long long)(p.first_cell + ic));
            out[ic] = c;
            return;
        }
        const double lambda_squared = spline_eval_lds(p.nj, p.jx, p.jl2, p.jcl, r);
        if (bulkPi < 0.0) lambda = -sqrt(lambda_squared);
        else if (bulkPi > 0.0) lambda = sqrt(lambda_squared);
        c.z = spline_eval_lds(p.nj, p.jx, p.jz, p.jcz, r);
        c.betapi = spline_eval_lds(nT, p.spl.x, p.spl.y[2], p.spl.c[2], T) * T4;
    }
    c.bulkPi = bulkPi;
    c.shear14 = 2.0 * T * T * (E + P);
    // Milne_Basis (viscous_correction.cpp:8-27)
    const double sinhL = tau * un / utperp, coshL = ut / utperp;
    c.Xt = uperp * coshL; c.Zt = sinhL; c.Xn = uperp * sinhL / tau; c.Zn = coshL / tau;
    c.Xx = 1.0; c.Yx = 0.0; c.Xy = 0.0; c.Yy = 1.0;
    if (uperp > 1.e-5) { c.Xx = utperp * ux / uperp; c.Yx = -uy / uperp; c.Xy = utperp * uy / uperp; c.Yy = ux / uperp; }
    const double Xt = c.Xt, Xx = c.Xx, Xy = c.Xy, Xn = c.Xn, Yx = c.Yx, Yy = c.Yy, Zt = c.Zt, Zn = c.Zn;
    // boost_dsigma_to_lrf, compute_dsigma_magnitude (:69-86)
    c.dst = dat * ut + dax * ux + day * uy + dan * un;
    c.dsx = -(dat * Xt + dax * Xx + day * Xy + dan * Xn);
    c.dsy = -(dax * Yx + day * Yy);
    c.dsz = -(dat * Zt + dan * Zn);
    c.ds_max = fabs(c.dst) + sqrt(c.dsx * c.dsx + c.dsy * c.dsy + c.dsz * c.dsz);
    // boost_pimunu_to_lrf (:99-115)
    c.pixx = pitt * Xt * Xt + pixx * Xx * Xx + piyy * Xy * Xy + tau2 * tau2 * pinn * Xn * Xn
           + 2.0 * (-Xt * (pitx * Xx + pity * Xy) + pixy * Xx * Xy + tau2 * Xn * (pixn * Xx + piyn * Xy - pitn * Xt));
    c.pixy = Yx * (-pitx * Xt + pixx * Xx + pixy * Xy + tau2 * pixn * Xn) + Yy * (-pity * Xt + pixy * Xx + piyy * Xy + tau2 * piyn * Xn);
    c.pixz = Zt * (pitt * Xt - pitx * Xx - pity * Xy - tau2 * pitn * Xn) - tau2 * Zn * (pitn * Xt - pixn * Xx - piyn * Xy - tau2 * pinn * Xn);
    c.piyy = pixx * Yx * Yx + 2.0 * pixy * Yx * Yy + piyy * Yy * Yy;
    c.piyz = -Zt * (pitx * Yx + pity * Yy) + tau2 * Zn * (pixn * Yx + piyn * Yy);
    c.pizz = -(c.pixx + c.piyy);
    // boost_Vmu_to_lrf (viscous_correction.cpp:161-173)
    c.Vx = -Vt * Xt + Vx * Xx + Vy * Xy + tau2 * Vn * Xn;
    c.Vy = Vx * Yx + Vy * Yy;
    c.Vz = -Vt * Zt + tau2 * Vn * Zn;
    c.tau = tau; c.x = p.x ? p.x[ic] : 0.0; c.y = p.y ? p.y[ic] : 0.0;
    c.eta = p.dim3 ? p.cells.eta[ic] : 0.0;
    c.ut = ut; c.ux = ux; c.uy = uy; c.un = un; c.T = T;
    // max_particle_number, df_mode 1 / 2: 2 n_eq per species (:282-303); total mean number of the cell (:1077)
    const double two_pi2_hbarC3 = 2.0 * M_PI * M_PI * (kHbarC * kHbarC * kHbarC);
    c.neq_fact = T * T * T / two_pi2_hbarC3;
    // modified temperature and rescaling coefficients (:1017-1036), detA and the breakdown test (:1038)
    c.T_mod = T;
    c.alphaB_mod = c.alphaB;
    if (p.df_mode == 3) {
        c.T_mod = T + bulkPi * c.F / c.betabulk; c.shear_mod = 0.5 / c.betapi; c.bulk_mod = bulkPi / (3.0 * c.betabulk);
        c.alphaB_mod = c.alphaB + bulkPi * c.G / c.betabulk;
        c.diff_mod = p.baryon ? T / c.betaV : 0.0;
    }
    else if (p.df_mode == 4) { c.shear_mod = 0.5 / c.betapi; c.bulk_mod = lambda; }
    if (p.df_mode == 3) {
        const double Axx = 1.0 + c.pixx * c.shear_mod + c.bulk_mod, Axy = c.pixy * c.shear_mod, Axz = c.pixz * c.shear_mod;
        const double Ayy = 1.0 + c.piyy * c.shear_mod + c.bulk_mod, Ayz = c.piyz * c.shear_mod, Azz = 1.0 + c.pizz * c.shear_mod + c.bulk_mod;
        const double detA = Axx * (Ayy * Azz - Ayz * Ayz) - Axy * (Axy * Azz - Ayz * Axz) + Axz * (Axy * Ayz - Ayy * Axz);
        double Tb = T, Fb = c.F, bbb = c.betabulk;
        if (p.fast) { Tb = p.T_sw; Fb = p.F_avg; bbb = p.betabulk_avg; }
        const double nf = Tb * Tb * Tb / two_pi2_hbarC3, Jf = Tb * nf, mbar_pion0 = p.mass_pion0 / Tb;
        const double neq_pion0 = nf * gt_neq(p.gl, p.gl + p.ngl, p.ngl, mbar_pion0, -1.0);
        const double J20_pion0 = Jf * gt_J20(p.gl + 2 * p.ngl, p.gl + 3 * p.ngl, p.ngl, mbar_pion0, -1.0);
        const double dn_pion0 = bulkPi * (neq_pion0 + J20_pion0 * Fb / Tb / Tb) / bbb;
        if (detA <= p.detA_min || (neq_pion0 + dn_pion0) < 0.0) { c.breakdown = 1.0; atomicAdd(&p.status[5], 1ULL); }
    }
    const double *gt = GT + ic, *gt2 = GT2 ? GT2 + ic : nullptr, *gt3 = GT3 ? GT3 + ic : nullptr;
    // the running sums are kept (species-major, so that the lanes of a wave -- consecutive cells -- store adjacent words): the sampling kernels
    // then find a hadron's species by bisection of exactly these sums instead of re-adding up to 305 gathered weights per hadron
    const double dn = species_running_sums(p, sp, c, gt, gt2, gt3, ic);
    c.dn_sum = dn;
    c.dn_tot = dn * (2.0 * p.y_max * c.ds_max);
    c.live = (c.dn_tot > 0.0) ? 1.0 : 0.0;                                          // :1079
    out[ic] = c;
}

// stream 0 of every (event, cell) pair of the batch: the Poisson number of hadrons (std::poisson_distribution(dn_tot), :1085-1090)
__global__ void __launch_bounds__(256)
cf_sampler_poisson(SamplerParams p, const SamplerCell *__restrict__ cellrec, int event0, int n_events, int32_t *__restrict__ n_drawn,
                   uint8_t *__restrict__ emits)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)n_events * p.n_cells) return;
    const int64_t ic = idx % p.n_cells;
    long N = 0;
    if (cellrec[ic].live != 0.0) {
        Rng g;
        g.init(p.seed, 0, (uint32_t)(p.first_cell + ic), (uint32_t)(event0 + (int)(idx / p.n_cells)));
        N = g.poisson(cellrec[ic].dn_tot);
    }
    n_drawn[idx] = (int32_t)(N < 0x7fffffffL ? N : 0x7fffffffL);
    emits[idx] = N > 0;
}

// the viscous route's Model (cf_sampler_common.h): the df_mode 3 integral tables beside GT, and per hadron the linear delta-f draw with its
// viscous weight or, for modified equilibrium away from breakdown, the rescaled momentum with weight 1
struct ViscousModel {
    const double *gt2, *gt3;
    using Pair = bool;      // linear: df_mode 1, 2, or a modified-equilibrium cell that broke down
    __device__ __forceinline__ Pair pair(const SamplerParams &p, const SamplerCell &c, int64_t) const { return p.df_mode <= 2 || c.breakdown != 0.0; }
    __device__ __forceinline__ double draw(const SamplerParams &p, const SamplerSpecies &sp, const SamplerCell &c, Pair linear, int chosen,
                                           double mass, double mass_squared, double sign, Rng &g_momentum, long &acceptances, long &samples,
                                           LrfMom &q) const
    {
        const double baryon = sp.baryon ? sp.baryon[chosen] : 0.0;
        double w_visc = 1.0;
        if (linear) {                                                               // :1100-1110, switch_to_linear_df
            const double chem = baryon * c.alphaB;
            q = sample_momentum(g_momentum, acceptances, samples, mass, sign, c.T, chem);
            // compute_df_weight (:361-453); df_mode 3 takes the Chapman-Enskog branch
            const double pimunu_pmu_pnu = q.px * q.px * c.pixx + q.py * q.py * c.piyy + q.pz * q.pz * c.pizz
                                        + 2.0 * (q.px * q.py * c.pixy + q.px * q.pz * c.pixz + q.py * q.pz * c.piyz);
            const double Vmu_pmu = -(q.px * c.Vx + q.py * c.Vy + q.pz * c.Vz);        // :384
            const double feqbar = 1.0 - sign / (exp(q.E / c.T - chem) + sign);
            double df_tot;
            if (p.df_mode == 1) {
                const double df_shear = pimunu_pmu_pnu / c.shear14;
                const double df_bulk = ((c.c0 - c.c2) * mass_squared + (baryon * c.c1 + (4.0 * c.c2 - c.c0) * q.E) * q.E) * c.bulkPi;
                const double df_diff = (baryon * c.c3 + c.c4 * q.E) * Vmu_pmu;
                df_tot = feqbar * (df_shear + df_bulk + df_diff);
            } else {
                const double betaV = p.baryon ? c.betaV : 1.0;
                const double df_shear = pimunu_pmu_pnu / (2.0 * q.E * c.betapi * c.T);
                const double df_bulk = (baryon * c.G + c.F * q.E / c.T / c.T + (q.E - mass_squared / q.E) / (3.0 * c.T)) * c.bulkPi / c.betabulk;
                const double df_diff = (c.ber - baryon / q.E) * Vmu_pmu / betaV;
                df_tot = feqbar * (df_shear + df_bulk + df_diff);
            }
            df_tot = fmax(-1.0, fmin(df_tot, 1.0));
            w_visc = (1.0 + df_tot) / 2.0;
        } else {                                                                    // :1112-1131 + rescale_momentum (:619-650)
            const bool mike = p.df_mode == 3;
            const LrfMom m = sample_momentum(g_momentum, acceptances, samples, mass, sign, c.T_mod, mike ? baryon * c.alphaB_mod : 0.0);
            const double diff_mod = c.diff_mod * (m.E * c.ber + (mike ? baryon : 0.0));   // :638
            q.px = (1.0 + c.bulk_mod) * m.px + c.shear_mod * (c.pixx * m.px + c.pixy * m.py + c.pixz * m.pz) + diff_mod * c.Vx;
            q.py = (1.0 + c.bulk_mod) * m.py + c.shear_mod * (c.pixy * m.px + c.piyy * m.py + c.piyz * m.pz) + diff_mod * c.Vy;
            q.pz = (1.0 + c.bulk_mod) * m.pz + c.shear_mod * (c.pixz * m.px + c.piyz * m.py + c.pizz * m.pz) + diff_mod * c.Vz;
            q.E = sqrt(mass_squared + q.px * q.px + q.py * q.py + q.pz * q.pz);
        }
        return w_visc;
    }
};

}  // namespace is3d

// ------------------------------------------------------------------------------------------------
// host entry
// ------------------------------------------------------------------------------------------------
namespace {

using DevMem = is3d::DevBuf<unsigned char>;

}  // namespace

struct is3d_sampler_plan {
    int device = 0;
    int64_t max_cells = 0;
    is3d_options o{};
    bool three_d = true;
    int ngla = 0, ncls = 0;
    is3d::SamplerParams p{};
    is3d::SamplerSpecies sp{};
    DevMem d_mass, d_sign, d_deg, d_cls, d_cmass, d_csign, d_gl, d_splx, d_sply[3], d_splc[3];
    DevMem d_bar, d_cbar, d_bilT, d_bilB, d_biltab[5];
    DevMem d_jonah, d_eqd, d_bkd;
    DevMem d_status, d_GT, d_GT2, d_GT3, d_rec, d_counts, d_offsets, d_scan_tmp;
    DevMem d_drawn, d_emits, d_active, d_nactive, d_cdf;
    DevMem d_particles, d_hist;             // a binned run: one batch of particles (list-and-bin only); the histograms, then the yields
    DevMem d_hist_decayed, d_slot;          // a decayed-and-binned run: the second block (histograms, yields, tallies) and the slot map
    DevMem d_flow, d_flow_decayed, d_flow_slot, d_flow_slot_decayed, d_flow_edges;   // a flow run: the record blocks (the decayed one with its tallies) and the slot maps
    DevMem d_pair_occ, d_pair_occ_decayed, d_pair_out, d_pair_slot, d_pair_slot_decayed;   // a pair run: the occupancy blocks (the decayed one behind its tallies), the histograms, the slot maps
    int64_t cap_cells = 0, cap_bt = 0;      // what the workspaces above were sized for
    int64_t cap_list = 0;                   // ... d_counts and d_offsets, which a fused binned run never has
    size_t tmp_select = 0, tmp_scan = 0;
    int64_t cap_particles = 0;
    size_t tmp_bytes = 0;
    hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    is3d::ViscousModel model{};             // the viscous sampler as a variant of its own plan (is3d_sampler_plan_create; unused by other variants)
    is3d::SamplerVariant viscous;
};

namespace {
// what every sampler plan checks of its species list and Gauss-Laguerre nodes
int check_species_nodes(const is3d_species *species, const is3d_sampler_inputs *in)
{
    using is3d::set_error;
    if (species->n < 1 || !species->mass || !species->sign || !species->degeneracy) return set_error(IS3D_EINVAL, "empty species list");
    for (int s = 0; s < species->n; s++)
        if (!(species->mass[s] > 0.0)) return set_error(IS3D_EINVAL, "species %d has mass 0: photons cannot be sampled with this method (reference: exit, sampling_kernels.cpp:478-482)", s);
    if (in->n_gla < 1 || in->n_gla > is3d::kSmpGlMax || !in->root1 || !in->weight1)
        return set_error(IS3D_EINVAL, "the sampler needs the Gauss-Laguerre roots and weights for alpha = 1 (1 to %d nodes)", is3d::kSmpGlMax);
    return IS3D_OK;
}
// the part of a plan that takes no coefficient tables: the device, the species classes (mass, sign[, baryon number]) and the Gauss-Laguerre nodes
int plan_base(std::unique_ptr<is3d_sampler_plan> &P, const is3d_species *species, const is3d_sampler_inputs *in, const is3d_options *opts,
              int64_t max_cells, const is3d_feqmod_tables *fq, bool baryon)
{
    using is3d::set_error;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    P.reset(new is3d_sampler_plan);
    is3d::count_resource(0);
    if (opts->device >= 0) HIP_TRY(hipSetDevice(opts->device));
    HIP_TRY(hipGetDevice(&P->device));
    P->max_cells = max_cells;
    P->o = *opts;
    P->three_d = opts->dimension == 3;
    P->ngla = in->n_gla;
    auto &d_mass = P->d_mass; auto &d_sign = P->d_sign; auto &d_deg = P->d_deg; auto &d_cls = P->d_cls; auto &d_cmass = P->d_cmass; auto &d_csign = P->d_csign;
    auto &d_gl = P->d_gl; auto &d_bar = P->d_bar; auto &d_cbar = P->d_cbar;
    is3d::SamplerSpecies &sp = P->sp;
    // ---- species classes (mass, sign[, baryon number]): the density integral is per class ----
    const int npart = species->n;
    const is3d::SpeciesClasses kc = is3d::species_classes(species->mass, species->sign, baryon ? species->baryon : nullptr, npart, true);
    const std::vector<int32_t> &cls = kc.cls;
    const std::vector<double> &cmass = kc.cmass, &csign = kc.csign, &cbar = kc.cbar;
    const int ncls = (int)cmass.size();
    HIP_TRY(d_mass.upload(std::vector<double>(species->mass, species->mass + npart)));
    HIP_TRY(d_sign.upload(std::vector<double>(species->sign, species->sign + npart)));
    HIP_TRY(d_deg.upload(std::vector<double>(species->degeneracy, species->degeneracy + npart)));
    HIP_TRY(d_cls.upload(cls));
    HIP_TRY(d_cmass.upload(cmass));
    HIP_TRY(d_csign.upload(csign));
    std::vector<double> gl((size_t)4 * in->n_gla, 0.0);
    for (int k = 0; k < in->n_gla; k++) {
        gl[k] = in->root1[k]; gl[in->n_gla + k] = in->weight1[k];
        if (fq) { gl[2 * in->n_gla + k] = fq->root2[k]; gl[3 * in->n_gla + k] = fq->weight2[k]; }
    }
    HIP_TRY(d_gl.upload(gl));
    if (baryon) {
        HIP_TRY(d_bar.upload(std::vector<double>(species->baryon, species->baryon + npart)));
        HIP_TRY(d_cbar.upload(cbar));
    }
    sp = is3d::SamplerSpecies{d_mass.as<double>(), d_sign.as<double>(), d_deg.as<double>(), d_cls.as<int32_t>(),
                              d_cmass.as<double>(), d_csign.as<double>(), npart, ncls, d_bar.as<double>(), d_cbar.as<double>()};
    P->ncls = ncls;
    return IS3D_OK;
}
// the rapidity range, the status words and the events
int plan_finish(is3d_sampler_plan *P, const is3d_sampler_inputs *in)
{
    is3d::SamplerParams &p = P->p;
    const bool three_d = P->three_d;
    p.y_max = three_d ? 0.5 : in->y_cut;                                              // :837-838
    HIP_TRY(P->d_status.alloc(8 * sizeof(unsigned long long)));
    p.status = P->d_status.as<unsigned long long>();
    for (auto &e : P->ev) HIP_TRY(hipEventCreate(&e));
    return IS3D_OK;
}
}  // namespace

namespace {
// SamplerVariant::cells of the viscous sampler: cf_sampler_cells on the cell arrays of P->p.cells
int viscous_cells(void *ctx, const is3d::SamplerParams &p, const is3d::SamplerSpecies &sp, const double *GT, is3d::SamplerCell *rec)
{
    is3d_sampler_plan *P = (is3d_sampler_plan *)ctx;
    P->model = is3d::ViscousModel{P->d_GT2.as<double>(), P->d_GT3.as<double>()};
    hipLaunchKernelGGL(is3d::cf_sampler_cells, dim3((unsigned)((p.n_cells + 127) / 128)), dim3(128), 0, nullptr, p, sp, GT, P->model.gt2, P->model.gt3, rec);
    return IS3D_OK;
}
}  // namespace

extern "C" int is3d_sampler_plan_create(is3d_sampler_plan **out, const is3d_species *species, const is3d_df_tables *df,
                                        const is3d_sampler_inputs *in, const is3d_options *opts, int64_t max_cells)
{
    using is3d::set_error;
    if (!out || !species || !df || !in || !opts) return set_error(IS3D_EINVAL, "null argument");
    *out = nullptr;
    if (max_cells < 1) max_cells = 1;
    if (opts->dimension != 2 && opts->dimension != 3) return set_error(IS3D_EINVAL, "dimension must be 2 or 3 (got %d)", opts->dimension);
    if (opts->df_mode < 1 || opts->df_mode > 4) return set_error(IS3D_EINVAL, "the sampler takes df_mode 1, 2, 3 or 4 (got %d)", opts->df_mode);
    const is3d_feqmod_tables *fq = in->feqmod;
    const bool need_alpha2 = opts->df_mode == 3 || (in->fast && opts->df_mode == 2);
    if ((opts->df_mode >= 3 || need_alpha2) && !fq) return set_error(IS3D_EINVAL, "df_mode 3 / 4 (and fast mode with df_mode 2) need in->feqmod");
    if (fq && (fq->n_gla != in->n_gla || !fq->root2 || !fq->weight2)) return set_error(IS3D_EINVAL, "in->feqmod: Gauss-Laguerre alpha = 2 nodes missing or of another size");
    if (opts->df_mode == 4 && (fq->n_pdg < 1 || !fq->pdg_mass || !fq->pdg_degeneracy || !fq->pdg_sign || !(fq->T_avg > 0.0)))
        return set_error(IS3D_EINVAL, "df_mode 4 needs the full PDG list and the surface-averaged temperature");
    if (in->fast && !(in->T_avg > 0.0)) return set_error(IS3D_EINVAL, "fast = 1 needs the surface-averaged temperature");
    const bool baryon = opts->include_baryon != 0, baryondiff = baryon && opts->include_baryondiff_deltaf != 0;
    if (baryon) {
        if (opts->df_mode == 4)   // deltafReader.cpp:470-474: "Jonah df doesn't work for nonzero muB. Exiting.."
            return set_error(IS3D_EINVAL, "df_mode 4 does not work with include_baryon = 1 (the reference exits there too)");
        if (!species->baryon) return set_error(IS3D_EINVAL, "include_baryon = 1 needs the species' baryon numbers");
        if (df->n_muB < 2 || !df->muB) return set_error(IS3D_EINVAL, "include_baryon = 1 needs the full (T, muB) coefficient tables");
        for (int i = 1; i < df->n_muB; i++)
            if (!(df->muB[i] > df->muB[i - 1])) return set_error(IS3D_EINVAL, "coefficient table muB values must ascend");
        if (opts->df_mode == 1 && (!df->c0 || !df->c1 || !df->c2 || !df->c3 || !df->c4)) return set_error(IS3D_EINVAL, "include_baryon = 1, df_mode 1 needs c0..c4 tables");
        if (opts->df_mode != 1 && (!df->F || !df->G || !df->betabulk || !df->betaV || !df->betapi))
            return set_error(IS3D_EINVAL, "include_baryon = 1, df_mode 2 / 3 need F, G, betabulk, betaV, betapi tables");
    }
    if (int rc = check_species_nodes(species, in)) return rc;
    if (df->n_T < 3 || !df->T) return set_error(IS3D_EINVAL, "coefficient table needs >= 3 temperatures");
    if (opts->df_mode == 1 && (!df->c0 || !df->c2)) return set_error(IS3D_EINVAL, "df_mode 1 needs c0 and c2 tables");
    if ((opts->df_mode == 2 || opts->df_mode == 3) && (!df->F || !df->betabulk || !df->betapi))
        return set_error(IS3D_EINVAL, "df_mode 2 / 3 need F, betabulk, betapi tables");
    if (opts->df_mode == 4 && !df->betapi) return set_error(IS3D_EINVAL, "df_mode 4 needs the betapi table");
    std::unique_ptr<is3d_sampler_plan> P;
    if (int rc = plan_base(P, species, in, opts, max_cells, fq, baryon)) return rc;
    const bool three_d = P->three_d;
    auto &d_gl = P->d_gl; auto &d_splx = P->d_splx; auto &d_sply = P->d_sply; auto &d_splc = P->d_splc;
    auto &d_bilT = P->d_bilT; auto &d_bilB = P->d_bilB; auto &d_biltab = P->d_biltab;
    auto &d_jonah = P->d_jonah; auto &d_eqd = P->d_eqd; auto &d_bkd = P->d_bkd;
    is3d::SamplerParams &p = P->p;
    const int npart = species->n;

    // ---- splines (deltafReader.cpp:300-322) ----
    std::vector<double> xs(df->T, df->T + df->n_T);
    for (int i = 1; i < df->n_T; i++)
        if (!(xs[i] > xs[i - 1])) return set_error(IS3D_EINVAL, "coefficient table temperatures must ascend");
    HIP_TRY(d_splx.upload(xs));
    const double *tabs[3] = {nullptr, nullptr, nullptr};
    int nspl;
    if (opts->df_mode == 1) { tabs[0] = df->c0; tabs[1] = df->c2; nspl = 2; }
    else if (opts->df_mode == 4) { tabs[0] = tabs[1] = tabs[2] = df->betapi; nspl = 3; }   // only slot 2 (betapi) is read
    else { tabs[0] = df->F; tabs[1] = df->betabulk; tabs[2] = df->betapi; nspl = 3; }
    p.spl.n = df->n_T; p.spl.x = d_splx.as<double>(); p.spl.nspl = nspl;
    for (int s = 0; s < nspl; s++) {
        std::vector<double> ys(tabs[s], tabs[s] + df->n_T), cc;
        if (!is3d::natural_cspline_init(xs, ys, cc)) return set_error(IS3D_EINVAL, "spline construction failed");
        HIP_TRY(d_sply[s].upload(ys));
        HIP_TRY(d_splc[s].upload(cc));
        p.spl.y[s] = d_sply[s].as<double>();
        p.spl.c[s] = d_splc[s].as<double>();
    }
    if (baryon) {   // full (mu_B, T) grids for the bilinear branch (deltafReader.cpp:412-484)
        const double *t5[5];
        if (opts->df_mode == 1) { t5[0] = df->c0; t5[1] = df->c1; t5[2] = df->c2; t5[3] = df->c3; t5[4] = df->c4; }
        else { t5[0] = df->F; t5[1] = df->G; t5[2] = df->betabulk; t5[3] = df->betaV; t5[4] = df->betapi; }
        HIP_TRY(d_bilT.upload(xs));
        HIP_TRY(d_bilB.upload(std::vector<double>(df->muB, df->muB + df->n_muB)));
        p.bil.nT = df->n_T; p.bil.nB = df->n_muB;
        p.bil.swap = opts->reference_bilinear_indexing != 0;
        p.bil.T = d_bilT.as<double>(); p.bil.muB = d_bilB.as<double>();
        for (int k = 0; k < 5; k++) {
            HIP_TRY(d_biltab[k].upload(std::vector<double>(t5[k], t5[k] + (size_t)df->n_T * df->n_muB)));
            p.bil.tab[k] = d_biltab[k].as<double>();
        }
    }
    p.baryon = baryon; p.baryondiff = baryondiff;
    p.dim3 = three_d; p.df_mode = opts->df_mode;
    p.include_bulk = opts->include_bulk_deltaf != 0; p.include_shear = opts->include_shear_deltaf != 0;
    p.ngl = in->n_gla; p.gl = d_gl.as<double>();
    // ---- df_mode 4: lambda(Pi/P), z(Pi/P) tables (deltafReader.cpp:222-297) ----
    if (opts->df_mode == 4) {
        std::vector<double> bp, l2, zz, cl, cz, jon;
        is3d::jonah_tables(fq, bp, l2, zz, p.bp_max);
        if (!is3d::natural_cspline_init(bp, l2, cl) || !is3d::natural_cspline_init(bp, zz, cz))
            return set_error(IS3D_EINVAL, "df_mode 4: bulkPi/Peq(lambda) is not ascending at T_avg = %.6g GeV (GSL would abort here)", fq->T_avg);
        p.nj = (int)bp.size();
        for (const auto *v : {&bp, &l2, &zz, &cl, &cz}) jon.insert(jon.end(), v->begin(), v->end());
        HIP_TRY(d_jonah.upload(jon));
        p.jx = d_jonah.as<double>(); p.jl2 = p.jx + p.nj; p.jz = p.jx + 2 * p.nj; p.jcl = p.jx + 3 * p.nj; p.jcz = p.jx + 4 * p.nj;
    }
    if (fq) { p.detA_min = fq->deta_min; p.mass_pion0 = fq->mass_pion0; }
    // ---- fast mode: Deltaf_Data::compute_particle_densities at the average temperature (deltafReader.cpp:536-650) ----
    p.fast = in->fast != 0;
    if (p.fast) {
        const double two_pi2_hbarC3 = 2.0 * std::pow(M_PI, 2) * std::pow(is3d::kHbarC, 3);
        auto spline_at = [&](int slot, double Tq) {   // gsl_spline_eval on the host copies of the spline slot
            std::vector<double> ys(tabs[slot], tabs[slot] + df->n_T), cc;
            (void)is3d::natural_cspline_init(xs, ys, cc);
            int lo = 0, hi = df->n_T - 1;
            while (hi > lo + 1) { int i = (hi + lo) >> 1; if (xs[i] > Tq) hi = i; else lo = i; }
            const double dx = xs[lo + 1] - xs[lo], dy = ys[lo + 1] - ys[lo], delx = Tq - xs[lo];
            const double b_i = (dy / dx) - dx * (cc[lo + 1] + 2.0 * cc[lo]) / 3.0, d_i = (cc[lo + 1] - cc[lo]) / (3.0 * dx);
            return ys[lo] + delx * (b_i + delx * (cc[lo] + delx * d_i));
        };
        auto in_table = [&](double Tq) { return Tq >= xs.front() && Tq <= xs.back(); };
        const double T = in->T_avg, Tsw = in->T_avg_switch > 0.0 ? in->T_avg_switch : in->T_avg;
        if (!in_table(T) || !in_table(Tsw)) return set_error(IS3D_EDOMAIN, "fast = 1: the average temperature %.6g GeV is outside the coefficient table", T);
        // include_baryon: Deltaf_Data::bilinear_interpolation at (T, muB_avg) on the host (deltafReader.cpp:412-484; cf_math.h::bilinear5 on the
        // host tables, same indexing option as the kernels)
        auto bilinear_at = [&](double Tq, double Bq, double (&v)[5]) -> bool {
            is3d::BilinearDev hb{};
            hb.nT = df->n_T; hb.nB = df->n_muB; hb.T = df->T; hb.muB = df->muB;
            hb.tab[0] = df->F; hb.tab[1] = df->G; hb.tab[2] = df->betabulk; hb.tab[3] = df->betaV; hb.tab[4] = df->betapi;
            hb.swap = opts->reference_bilinear_indexing != 0;
            return is3d::bilinear5(hb, Tq, Bq, v);
        };
        const double muB_avg = baryon ? in->muB_avg : 0.0, alphaB_avg = muB_avg / T;   // deltafReader.cpp:545-551
        double F = 0.0, G = 0.0, betabulk = 1.0;
        if (baryon && opts->df_mode != 1) {
            double bl[5];
            if (!bilinear_at(T, muB_avg, bl)) return set_error(IS3D_EDOMAIN, "fast = 1: the average (T, muB) = (%.6g, %.6g) GeV is outside the coefficient table", T, muB_avg);
            F = bl[0] * T; G = bl[1]; betabulk = bl[2] * (T * T * T * T);
        } else if (baryon) {   // df_mode 1: only the table range is checked (the 14-moment coefficients do not enter the fast densities used here)
            const double dB = std::fabs(df->muB[1] - df->muB[0]);
            const int iBL = (int)std::floor((muB_avg - df->muB[0]) / dB);
            if (!(iBL >= 0 && iBL + 1 < df->n_muB)) return set_error(IS3D_EDOMAIN, "fast = 1: the average muB = %.6g GeV is outside the coefficient table", muB_avg);
        } else if (opts->df_mode == 2 || opts->df_mode == 3) { F = spline_at(0, T) * T; betabulk = spline_at(1, T) * T * T * T * T; }
        std::vector<double> eqd(npart, 0.0), bkd(npart, 0.0);
        for (int ip = 0; ip < npart; ip++) {
            const double mbar = species->mass[ip] / T, sign = species->sign[ip];
            const double bnum = baryon ? species->baryon[ip] : 0.0, chem = bnum * alphaB_avg;
            double s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int k = 0; k < in->n_gla; k++) {
                const double pbar = in->root1[k], Ebar = std::sqrt(pbar * pbar + mbar * mbar);
                s1 += in->weight1[k] * (pbar * std::exp(pbar) / (std::exp(Ebar - chem) + sign));
            }
            const double neq = species->degeneracy[ip] * std::pow(T, 3) / two_pi2_hbarC3 * s1;
            eqd[ip] = neq;
            if (opts->df_mode == 2 || opts->df_mode == 3) {
                for (int k = 0; k < in->n_gla; k++) {
                    const double pbar = fq->root2[k], Ebar = std::sqrt(pbar * pbar + mbar * mbar), qstat = std::exp(Ebar - chem) + sign;
                    s2 += fq->weight2[k] * (Ebar * std::exp(pbar + Ebar - chem) / (qstat * qstat));
                }
                for (int k = 0; k < in->n_gla; k++) {
                    const double pbar = in->root1[k], Ebar = std::sqrt(pbar * pbar + mbar * mbar), qstat = std::exp(Ebar - chem) + sign;
                    s3 += in->weight1[k] * (pbar * std::exp(pbar + Ebar - chem) / (qstat * qstat));
                }
                const double J10 = species->degeneracy[ip] * std::pow(T, 3) / two_pi2_hbarC3 * s3;
                const double J20 = species->degeneracy[ip] * std::pow(T, 4) / two_pi2_hbarC3 * s2;
                bkd[ip] = (neq + (bnum * J10 * G) + (J20 * F / std::pow(T, 2))) / betabulk;
            }
        }
        HIP_TRY(d_eqd.upload(eqd));
        HIP_TRY(d_bkd.upload(bkd));
        p.eqd = d_eqd.as<double>(); p.bkd = d_bkd.as<double>();
        p.T_sw = Tsw;
        if (opts->df_mode == 3 && baryon) {                                            // :862-867 at (Tavg with T_switch, muBavg)
            double bl[5];
            if (!bilinear_at(Tsw, muB_avg, bl)) return set_error(IS3D_EDOMAIN, "fast = 1: (T_switch, muB_avg) = (%.6g, %.6g) GeV is outside the coefficient table", Tsw, muB_avg);
            p.F_avg = bl[0] * Tsw; p.betabulk_avg = bl[2] * (Tsw * Tsw * Tsw * Tsw);
        } else if (opts->df_mode == 3) { p.F_avg = spline_at(0, Tsw) * Tsw; p.betabulk_avg = spline_at(1, Tsw) * Tsw * Tsw * Tsw * Tsw; }
    }
    if (int rc = plan_finish(P.get(), in)) return rc;
    is3d::SamplerVariant &v = P->viscous;
    v.domain_text = std::string("T") + (opts->df_mode == 4 ? " (or bulkPi/P)" : (baryon ? " or (T, muB)" : "")) +
                    " outside the coefficient table (the reference aborts in gsl_spline_eval here)";
    v.ctx = P.get();
    v.cells = viscous_cells;
    v.set_model(&P->model);
    *out = P.release();
    return IS3D_OK;
}

namespace {
// cell-array checks shared by the host and the device entry (pointers are only tested for NULL here)
int check_cells(const is3d_cells *cells, const is3d_options *o, int64_t first_cell)
{
    const int64_t n = cells->n_cells;
    if (n < 0 || n + first_cell > 0xffffffffLL) return is3d::set_error(IS3D_EINVAL, "cell indices must fit 32 bits for the counter-based streams");
    return is3d::check_cells(cells, o->dimension == 3, *o, o->include_baryon != 0 && o->include_baryondiff_deltaf != 0);
}
// which of the 23 cell arrays (CellPtrs order) the kernels read under these options
bool cell_array_needed(int a, const is3d_options *o)
{
    const bool three_d = o->dimension == 3;
    const bool baryondiff = o->include_baryon != 0 && o->include_baryondiff_deltaf != 0;
    return a < 12 ? (a != 1 || three_d) : (a < 17 ? o->include_shear_deltaf != 0 : (a == 17 ? o->include_bulk_deltaf != 0 : baryondiff));
}
// the needed cell arrays of a DEVICE surface become the plan's, and the viscous variant's temperature and chemical potential
int bind_cells(is3d_sampler_plan *P, const is3d_cells *cells, int64_t first_cell)
{
    if (int rc = check_cells(cells, &P->o, first_cell)) return rc;
    if (cells->n_cells > 0) {
        auto arrays = is3d::cell_arrays(*cells);
        for (int a = 0; a < is3d::kCellArrays; a++)
            if (!cell_array_needed(a, &P->o)) arrays[a] = nullptr;
        P->p.cells = is3d::cell_ptrs(is3d::cells_from_arrays(cells->n_cells, arrays));
    }
    P->viscous.T = P->p.cells.T;
    P->viscous.muB = P->p.cells.muB;
    return IS3D_OK;
}
using BinRun = is3d::SamplerBinRun;
// a flow run of the batch loop: each batch's list in the plan's workspace goes through cf_sampler_flow into records_dev and, with decay,
// through cf_decay_mc_flow (first_particle = the hadrons of the batches before it), whose time is added to ms_decay
struct FlowRun {
    is3d_flow_cuts cuts;
    is3d::FlowThresholds thresholds;
    int32_t n_slots;
    const int32_t *slot_dev;          // [species]
    unsigned long long *records_dev;
    const is3d::DecayMcFlowRun *decay;
    double ms_decay;
    // a pair run instead (records_dev == NULL): the batch's list goes through cf_pair_cells into occ_dev and, with pair_decay, through
    // cf_decay_mc_pairs; slot_dev and n_slots as above
    const is3d_pair_bins *pair_bins;
    const is3d::PairTables *pair_tables;
    unsigned *occ_dev;
    const is3d::DecayMcPairRun *pair_decay;
    // an HBT run instead (records_dev == NULL, occ_dev == NULL): the batch's list is selected and paired (hbt) and, with hbt_decay, decayed
    // twice into records that are paired (hbt_decayed); the histograms stay in the two runs
    is3d::HbtRun *hbt, *hbt_decayed;
    const is3d::DecayMcHbtRun *hbt_decay;
    // a differential flow run (n_pT > 0): records_dev holds n_slots * n_pT records per event and the batch's list goes through
    // cf_sampler_flow_diff with the DEVICE edge table edges_dev[n_pT + 1]; decay carries the same table
    int32_t n_pT;
    const double *edges_dev;
};
int sampler_batches(is3d_sampler_plan *P, const is3d::SamplerVariant &v, int64_t n, const double *x_dev, const double *y_dev, int32_t n_events,
                    uint64_t seed, int64_t first_cell, int32_t batch_events, is3d_particle *particles_dev, int64_t capacity, const BinRun *bin,
                    bool fuse, int64_t *n_particles, is3d_sampler_stats *stats, const is3d::DecayMcBinRun *decay = nullptr,
                    double *ms_decay = nullptr, FlowRun *flow = nullptr);
}  // namespace

extern "C" void is3d_sampler_plan_destroy(is3d_sampler_plan *P)
{
    if (!P) return;
    (void)hipSetDevice(P->device);
    for (auto &e : P->ev)
        if (e) (void)hipEventDestroy(e);
    delete P;
}

// cells_dev: DEVICE arrays; x_dev, y_dev: DEVICE arrays or NULL; particles_dev: DEVICE buffer of `capacity` entries or NULL (count only)
extern "C" int is3d_sampler_plan_execute(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev, int32_t n_events,
                                         uint64_t seed, int64_t first_cell, int32_t batch_events, is3d_particle *particles_dev, int64_t capacity,
                                         int64_t *n_particles, is3d_sampler_stats *stats)
{
    using is3d::set_error;
    if (!P || !cells || !n_particles) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_events < 1) return set_error(IS3D_EINVAL, "n_events must be >= 1");
    if (int rc = bind_cells(P, cells, first_cell)) return rc;
    return is3d::sampler_variant_execute(P, P->viscous, cells->n_cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, particles_dev,
                                         capacity, n_particles, stats);
}

namespace {
// the one batch loop of every variant.  bin == NULL fills the caller's list (or only counts); bin != NULL with fuse samples each batch
// straight into P->d_hist (cf_sampler_fused); bin != NULL without it fills each batch into the plan's particle workspace at base 0, bins it
// into P->d_hist (cf_sampler_bins) and drops it -- after, with decay != NULL, the batch's hadrons as primaries base .. of the whole list have
// been decayed and binned into decay->block_dev (cf_decay_mc_bins), whose time is added to *ms_decay
int sampler_batches(is3d_sampler_plan *P, const is3d::SamplerVariant &v, int64_t n, const double *x_dev, const double *y_dev, int32_t n_events,
                    uint64_t seed, int64_t first_cell, int32_t batch_events, is3d_particle *particles_dev, int64_t capacity, const BinRun *bin,
                    bool fuse, int64_t *n_particles, is3d_sampler_stats *stats, const is3d::DecayMcBinRun *decay, double *ms_decay, FlowRun *flow)
{
    using is3d::set_error;
    if (particles_dev == nullptr || bin || flow) capacity = 0;
    if (n > P->max_cells) return set_error(IS3D_EINVAL, "%lld cells, the sampler plan was created for %lld", (long long)n, (long long)P->max_cells);
    HIP_TRY(hipSetDevice(P->device));
    if (n == 0) return IS3D_OK;
    const int ncls = P->ncls;
    is3d::SamplerParams &p = P->p;
    const is3d::SamplerSpecies &sp = P->sp;
    p.x = x_dev; p.y = y_dev;
    p.n_cells = n; p.first_cell = first_cell;
    p.seed = seed;
    p.cdf = nullptr;           // set below, once the workspaces exist
    hipEvent_t *ev = P->ev;
    unsigned long long init[8] = {~0ULL, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(P->d_status.p, init, sizeof init, hipMemcpyHostToDevice, nullptr));
    // ---- workspaces: sized by the largest (cells, event batch) seen so far; a second execute of the same shape allocates nothing ----
    const int64_t max_threads = (int64_t)1 << 25;
    int eb = (int)std::max<int64_t>(1, std::min<int64_t>(n_events, max_threads / n));
    if (batch_events > 0) eb = std::min(eb, batch_events);
    const int64_t bt = (int64_t)eb * n;
    if (n > P->cap_cells) {
        HIP_TRY(P->d_GT.alloc((size_t)n * ncls * sizeof(double)));
        if (P->o.df_mode == 3 && !p.fast) HIP_TRY(P->d_GT2.alloc((size_t)n * ncls * sizeof(double)));
        if (P->o.df_mode == 3 && p.baryon) HIP_TRY(P->d_GT3.alloc((size_t)n * ncls * sizeof(double)));
        HIP_TRY(P->d_rec.alloc((size_t)n * sizeof(is3d::SamplerCell)));
        // running sums of the species weights per cell, one per block of 8 species (312 B per cell for 305 species): df_mode 3's weights may be negative (n_eq + Pi dn_bulk),
        // its sums are not monotone and the species is found by the linear inversion there
        if (P->o.df_mode != 3) HIP_TRY(P->d_cdf.alloc((size_t)n * ((sp.npart + is3d::kCdfBlock - 1) / is3d::kCdfBlock) * sizeof(double)));
        P->cap_cells = n;
    }
    // fused: one pass per batch samples and bins; the counts, the offsets and the scan exist only to put a list in order
    const bool fused = bin && fuse;
    if (bt > P->cap_bt) {
        HIP_TRY(P->d_drawn.alloc((size_t)bt * sizeof(int32_t)));
        HIP_TRY(P->d_emits.alloc((size_t)bt));
        HIP_TRY(P->d_active.alloc((size_t)bt * sizeof(int32_t)));
        HIP_TRY(P->d_nactive.alloc(sizeof(int32_t)));
        HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, P->tmp_select, hipcub::CountingInputIterator<int32_t>(0), P->d_emits.as<uint8_t>(),
                                              P->d_active.as<int32_t>(), P->d_nactive.as<int32_t>(), (int)bt, nullptr));
        P->cap_bt = bt;
    }
    if (!fused && bt > P->cap_list) {
        HIP_TRY(P->d_counts.alloc((size_t)(bt + 1) * sizeof(int64_t)));
        HIP_TRY(P->d_offsets.alloc((size_t)(bt + 1) * sizeof(int64_t)));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, P->tmp_scan, P->d_counts.as<int64_t>(), P->d_offsets.as<int64_t>(), (int)(bt + 1), nullptr));
        P->cap_list = bt;
    }
    if (const size_t need = std::max(P->tmp_select, fused ? (size_t)0 : P->tmp_scan); need > P->tmp_bytes) {
        HIP_TRY(P->d_scan_tmp.alloc(need));
        P->tmp_bytes = need;
    }
    p.cdf = P->d_cdf.as<double>();
    DevMem &d_GT = P->d_GT, &d_rec = P->d_rec, &d_counts = P->d_counts, &d_offsets = P->d_offsets, &d_scan_tmp = P->d_scan_tmp;
    DevMem &d_drawn = P->d_drawn, &d_emits = P->d_emits, &d_active = P->d_active, &d_nactive = P->d_nactive;
    size_t tmp_bytes = P->tmp_bytes;
    HIP_TRY(hipEventRecord(ev[1], nullptr));
    {
        const int64_t tot = n * ncls;
        hipLaunchKernelGGL(is3d::cf_sampler_density, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, nullptr, v.T, v.muB, n, sp, P->d_gl.as<double>(),
                           P->ngla, d_GT.as<double>(), P->d_GT2.as<double>(), P->d_GT3.as<double>());
        HIP_TRY(hipEventRecord(ev[6], nullptr));
        if (int rc = v.cells(v.ctx, p, sp, d_GT.as<double>(), d_rec.as<is3d::SamplerCell>())) return rc;
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[2], nullptr));
    // ---- events in batches of <= 2^25 (event, cell) threads: count, scan, fill ----
    int64_t base = 0;
    double ms_count = 0.0, ms_fill = 0.0, ms_poisson = 0.0, ms_bin = 0.0;
    for (int e0 = 0; e0 < n_events; e0 += eb) {
        const int ne = std::min(eb, n_events - e0);
        const int64_t nt = (int64_t)ne * n;
        HIP_TRY(hipEventRecord(ev[5], nullptr));
        // Poisson numbers of all pairs, then the ordered list of the pairs that emit
        hipLaunchKernelGGL(is3d::cf_sampler_poisson, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, nullptr, p, d_rec.as<is3d::SamplerCell>(), e0, ne,
                           d_drawn.as<int32_t>(), d_emits.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceSelect::Flagged(d_scan_tmp.p, tmp_bytes, hipcub::CountingInputIterator<int32_t>(0), d_emits.as<uint8_t>(),
                                              d_active.as<int32_t>(), d_nactive.as<int32_t>(), (int)nt, nullptr));
        HIP_TRY(hipEventRecord(ev[7], nullptr));
        int32_t n_active = 0;
        HIP_TRY(hipMemcpy(&n_active, d_nactive.p, sizeof(int32_t), hipMemcpyDeviceToHost));
        int64_t batch_total = 0;
        // what every launch of the batch gets; the count pass adds counts, the fill pass offsets and the list
        is3d::SamplerRunArgs a{d_rec.as<is3d::SamplerCell>(), d_GT.as<double>(), e0, d_active.as<int32_t>(), (int64_t)n_active, d_drawn.as<int32_t>(),
                               nullptr, nullptr, 0, nullptr, 0};
        if (fused) {
            HIP_TRY(hipEventRecord(ev[3], nullptr));
            HIP_TRY(hipEventRecord(ev[8], nullptr));
            if (n_active > 0) {
                unsigned long long *hist_dev = P->d_hist.as<unsigned long long>();
                v.fused(v.model, p, sp, a, *bin, hist_dev, hist_dev + bin->layout.total);
                HIP_TRY(hipGetLastError());
            }
        } else if (n_active > 0) {
            HIP_TRY(hipMemsetAsync(d_counts.as<int64_t>() + n_active, 0, sizeof(int64_t), nullptr));
            a.counts = d_counts.as<int64_t>();
            v.run(v.model, false, p, sp, a);
            HIP_TRY(hipGetLastError());
            // element n_active of the scan (counts[n_active] = 0) is the batch total
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_scan_tmp.p, tmp_bytes, d_counts.as<int64_t>(), d_offsets.as<int64_t>(), n_active + 1, nullptr));
            HIP_TRY(hipEventRecord(ev[3], nullptr));
            HIP_TRY(hipMemcpy(&batch_total, d_offsets.as<int64_t>() + n_active, sizeof(int64_t), hipMemcpyDeviceToHost));
            // the list: the caller's buffer at the running base; binned: the plan's workspace, grown to the largest batch seen, at base 0
            a.counts = nullptr; a.offsets = d_offsets.as<int64_t>();
            a.particles = particles_dev; a.base = base; a.capacity = capacity;
            if ((bin || flow) && batch_total > 0) {
                if (batch_total > P->cap_particles) {
                    HIP_TRY(P->d_particles.alloc((size_t)batch_total * sizeof(is3d_particle)));
                    P->cap_particles = batch_total;
                }
                a.particles = P->d_particles.as<is3d_particle>(); a.base = 0; a.capacity = batch_total;
            }
            if (a.capacity > 0 && a.base < a.capacity && batch_total > 0) {
                v.run(v.model, true, p, sp, a);
                HIP_TRY(hipGetLastError());
            }
        } else {
            HIP_TRY(hipEventRecord(ev[3], nullptr));
        }
        if (!fused) HIP_TRY(hipEventRecord(ev[8], nullptr));
        if (bin && batch_total > 0)
            HIP_TRY(is3d::sampler_bins_launch(bin->bins, bin->widths, bin->layout, sp.npart, n_events, P->d_particles.as<is3d_particle>(), batch_total,
                                              P->d_hist.as<unsigned long long>(), P->d_hist.as<unsigned long long>() + bin->layout.total,
                                              bin->bins.kernel_form));
        if (flow && flow->occ_dev && batch_total > 0)
            HIP_TRY(is3d::pair_cells_launch(*flow->pair_bins, *flow->pair_tables, n_events, flow->n_slots, flow->slot_dev, sp.npart,
                                            P->d_particles.as<is3d_particle>(), batch_total, flow->occ_dev));
        if (flow && flow->records_dev && flow->n_pT > 0 && batch_total > 0)
            HIP_TRY(is3d::flow_diff_launch(flow->cuts, flow->thresholds, flow->n_pT, flow->edges_dev, n_events, flow->n_slots, flow->slot_dev, sp.npart,
                                           P->d_particles.as<is3d_particle>(), batch_total, flow->records_dev, flow->cuts.kernel_form));
        else if (flow && flow->records_dev && batch_total > 0)
            HIP_TRY(is3d::flow_launch(flow->cuts, flow->thresholds, n_events, flow->n_slots, flow->slot_dev, sp.npart, P->d_particles.as<is3d_particle>(),
                                      batch_total, flow->records_dev, flow->cuts.kernel_form));
        if (flow && flow->hbt && batch_total > 0)
            if (int rc = is3d::hbt_batch_list(*flow->hbt, flow->slot_dev, sp.npart, P->d_particles.as<is3d_particle>(), batch_total)) return rc;
        HIP_TRY(hipEventRecord(ev[4], nullptr));
        if (flow && flow->hbt_decay && batch_total > 0) {
            if (int rc = is3d::decay_mc_hbt_batch(*flow->hbt_decay, *flow->hbt_decayed, P->d_particles.as<is3d_particle>(), batch_total, base)) return rc;
            HIP_TRY(hipEventRecord(ev[9], nullptr));
            HIP_TRY(hipEventSynchronize(ev[9]));
            float e_ms = 0;
            HIP_TRY(hipEventElapsedTime(&e_ms, ev[4], ev[9]));
            flow->ms_decay += e_ms;
        }
        if (flow && flow->decay && batch_total > 0) {
            HIP_TRY(is3d::decay_mc_flow_launch(*flow->decay, P->d_particles.as<is3d_particle>(), batch_total, base));
            HIP_TRY(hipEventRecord(ev[9], nullptr));
            HIP_TRY(hipEventSynchronize(ev[9]));
            float e_ms = 0;
            HIP_TRY(hipEventElapsedTime(&e_ms, ev[4], ev[9]));
            flow->ms_decay += e_ms;
        }
        if (flow && flow->pair_decay && batch_total > 0) {
            HIP_TRY(is3d::decay_mc_pairs_launch(*flow->pair_decay, P->d_particles.as<is3d_particle>(), batch_total, base));
            HIP_TRY(hipEventRecord(ev[9], nullptr));
            HIP_TRY(hipEventSynchronize(ev[9]));
            float e_ms = 0;
            HIP_TRY(hipEventElapsedTime(&e_ms, ev[4], ev[9]));
            flow->ms_decay += e_ms;
        }
        if (decay && bin && !fused && batch_total > 0) {
            HIP_TRY(is3d::decay_mc_bins_launch(*decay, P->d_particles.as<is3d_particle>(), batch_total, base));
            HIP_TRY(hipEventRecord(ev[9], nullptr));
            HIP_TRY(hipEventSynchronize(ev[9]));
            float e_ms = 0;
            HIP_TRY(hipEventElapsedTime(&e_ms, ev[4], ev[9]));
            *ms_decay += e_ms;
        }
        HIP_TRY(hipEventSynchronize(ev[4]));
        float a_ms = 0, b_ms = 0, c_ms = 0, d_ms = 0;
        HIP_TRY(hipEventElapsedTime(&a_ms, ev[5], ev[3]));
        HIP_TRY(hipEventElapsedTime(&b_ms, ev[3], ev[8]));
        HIP_TRY(hipEventElapsedTime(&c_ms, ev[5], ev[7]));
        HIP_TRY(hipEventElapsedTime(&d_ms, ev[8], ev[4]));
        ms_count += a_ms; ms_fill += b_ms; ms_poisson += c_ms; ms_bin += d_ms;
        base += batch_total;
    }
    unsigned long long h[8];
    HIP_TRY(hipMemcpy(h, P->d_status.p, sizeof h, hipMemcpyDeviceToHost));
    *n_particles = base;
    if (stats) {
        float b = 0, dn = 0;
        (void)hipEventElapsedTime(&b, ev[1], ev[2]);
        (void)hipEventElapsedTime(&dn, ev[1], ev[6]);
        stats->ms_h2d = 0.0;
        stats->ms_prep = b;
        stats->ms_density = dn;
        stats->ms_poisson = ms_poisson;
        stats->n_cells_skipped = (int64_t)h[1];
        stats->n_momentum_samples = (int64_t)h[2];
        stats->n_acceptances = (int64_t)h[3];
        stats->n_hadrons_drawn = (int64_t)h[4];
        stats->n_cells_breakdown = (int64_t)h[5];
        stats->n_classes = ncls;
        stats->ms_count = fused ? 0.0 : ms_count; stats->ms_fill = fused ? 0.0 : ms_fill;
        if (bin || flow) stats->ms_bin = ms_bin;
        if ((bin || flow) && !fused) stats->particle_workspace_bytes = P->cap_particles * (int64_t)sizeof(is3d_particle);
    }
    if (h[0] != ~0ULL) return set_error(IS3D_EDOMAIN, "cell %lld: %s", (long long)h[0], v.domain_text.c_str());
    if (particles_dev && base > capacity)
        return set_error(IS3D_ENOMEM, "%lld particles sampled but the caller's buffer holds %lld (call with particles = NULL for the count)",
                         (long long)base, (long long)capacity);
    return IS3D_OK;
}
}  // namespace

// ---- a sampler variant on this plan and batch loop (cf_sampler_common.h) ----
int is3d::sampler_variant_plan_create(is3d_sampler_plan **out, const is3d_species *species, const is3d_sampler_inputs *in, const is3d_options *opts,
                                      int64_t max_cells)
{
    *out = nullptr;
    if (opts->dimension != 2 && opts->dimension != 3) return set_error(IS3D_EINVAL, "dimension must be 2 or 3 (got %d)", opts->dimension);
    if (int rc = check_species_nodes(species, in)) return rc;
    std::unique_ptr<is3d_sampler_plan> P;
    if (int rc = plan_base(P, species, in, opts, std::max<int64_t>(max_cells, 1), nullptr, false)) return rc;
    P->o.df_mode = 1;              // species_dn: 2 neq_fact g GT; the blocked running sums are kept
    P->o.include_baryon = 0;
    is3d::SamplerParams &p = P->p;
    p.dim3 = P->three_d; p.df_mode = 1;
    p.include_bulk = opts->include_bulk_deltaf != 0; p.include_shear = opts->include_shear_deltaf != 0;
    p.ngl = in->n_gla; p.gl = P->d_gl.as<double>();
    if (int rc = plan_finish(P.get(), in)) return rc;
    *out = P.release();
    return IS3D_OK;
}

int is3d::sampler_variant_execute(is3d_sampler_plan *P, const SamplerVariant &v, int64_t n_cells, const double *x_dev, const double *y_dev,
                                  int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events, is3d_particle *particles_dev,
                                  int64_t capacity, int64_t *n_particles, is3d_sampler_stats *stats)
{
    *n_particles = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_events < 1) return set_error(IS3D_EINVAL, "n_events must be >= 1");
    if (n_cells < 0 || n_cells + first_cell > 0xffffffffLL) return set_error(IS3D_EINVAL, "cell indices must fit 32 bits for the counter-based streams");
    return sampler_batches(P, v, n_cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, particles_dev, capacity, nullptr, false, n_particles,
                           stats);
}

int is3d::sampler_variant_sample_list(is3d_sampler_plan *P, const SamplerVariant &v, int64_t n_cells, const double *x_dev, const double *y_dev,
                                      const is3d_sampler_inputs *in, float ms_h2d, is3d_particle *particles, int64_t capacity,
                                      int64_t *n_particles, is3d_sampler_stats *stats)
{
    if (particles == nullptr) capacity = 0;
    DevMem d_particles;
    if (capacity > 0) HIP_TRY(d_particles.alloc((size_t)capacity * sizeof(is3d_particle)));
    int64_t total = 0;
    const int rc = sampler_variant_execute(P, v, n_cells, x_dev, y_dev, in->n_events, in->seed, in->first_cell, in->batch_events,
                                           d_particles.as<is3d_particle>(), capacity, &total, stats);
    *n_particles = total;
    if (stats) stats->ms_h2d = ms_h2d;
    if (rc && rc != IS3D_ENOMEM && !(rc == IS3D_EDOMAIN && v.edomain_keeps_rest)) return rc;
    const std::string kept = rc ? is3d_last_error() : "";
    const int64_t ncopy = std::min<int64_t>(total, capacity);
    if (ncopy > 0) HIP_TRY(hipMemcpy(particles, d_particles.p, (size_t)ncopy * sizeof(is3d_particle), hipMemcpyDeviceToHost));
    if (rc) return set_error(rc, "%s", kept.c_str());
    return IS3D_OK;
}

namespace {
// what the host-pointer entries share: a plan for this surface, and the needed cell arrays, x and y uploaded in one block
struct StagedRun {
    is3d_sampler_plan *P = nullptr;
    is3d::DevBuf<double> d_cells;   // the needed cell arrays, then x and y
    is3d_cells dc{};
    std::array<const double *, 2> xy{};
    float ms_h2d = 0;
    ~StagedRun() { is3d_sampler_plan_destroy(P); }
};
// an empty surface stages nothing (r.dc.n_cells = 0)
int stage_run(StagedRun &r, const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
              const is3d_options *opts)
{
    if (int rc = is3d_sampler_plan_create(&r.P, species, df, in, opts, std::max<int64_t>(cells->n_cells, 1))) return rc;
    if (int rc = check_cells(cells, opts, in->first_cell)) return rc;
    const int64_t n = cells->n_cells;
    if (n == 0) return IS3D_OK;
    HIP_TRY(r.d_cells.alloc((size_t)n * (is3d::kCellArrays + 2)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evg{e0, e1};
    HIP_TRY(hipEventRecord(e0, nullptr));
    HIP_TRY(is3d::stage_cells(*cells, [opts](int a) { return cell_array_needed(a, opts); }, 0, n, r.d_cells.p, nullptr, &r.dc));
    r.xy = {in->x, in->y};
    HIP_TRY(is3d::stage_arrays(r.xy, 0, n, r.d_cells.p + (size_t)is3d::kCellArrays * n, nullptr));
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&r.ms_h2d, e0, e1);
    return IS3D_OK;
}
}  // namespace

// the host-pointer entry: plan + upload + execute + download (the particle list is the plan's, bit for bit)
extern "C" int is3d_sample_particles(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df,
                                     const is3d_sampler_inputs *in, const is3d_options *opts, is3d_particle *particles,
                                     int64_t capacity, int64_t *n_particles, is3d_sampler_stats *stats)
{
    using is3d::set_error;
    if (!cells || !species || !df || !in || !opts || !n_particles) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (in->n_events < 1) {
        // (argument checks of the plan first, so that a bad option is reported before a bad event count -- as the one-shot entry always did)
        is3d_sampler_plan *chk = nullptr;
        const int rc0 = is3d_sampler_plan_create(&chk, species, df, in, opts, 1);
        is3d_sampler_plan_destroy(chk);
        if (rc0 && rc0 != IS3D_ENODEVICE) return rc0;
        return set_error(IS3D_EINVAL, "n_events must be >= 1");
    }
    StagedRun r;
    if (int rc = stage_run(r, cells, species, df, in, opts)) return rc;
    if (cells->n_cells == 0) return IS3D_OK;
    if (int rc = bind_cells(r.P, &r.dc, in->first_cell)) return rc;
    return is3d::sampler_variant_sample_list(r.P, r.P->viscous, r.dc.n_cells, r.xy[0], r.xy[1], in, r.ms_h2d, particles, capacity, n_particles, stats);
}

// ------------------------------------------------------------------------------------------------
// binned on the device: fused, or the list of each event batch through cf_sampler_bins (cf_sampler_bins.hip) and dropped
// ------------------------------------------------------------------------------------------------
namespace {
int check_bin_args(const is3d_sampler_test_bins *bins, const is3d_sampler_hist *h, int32_t n_events)
{
    using is3d::set_error;
    if (!bins || !h) return set_error(IS3D_EINVAL, "null argument");
    if (n_events < 1) return set_error(IS3D_EINVAL, "n_events must be >= 1");
    if (!is3d::sampler_bins_valid(*bins))
        return set_error(IS3D_EINVAL, "sampler test bins: every bin count must be >= 1, y_cut and eta_cut > 0, pT_upper_cut > pT_lower_cut, tau_max > tau_min, r_max > r_min");
    if (!h->dN_dy || !h->dN_deta || !h->dN_pT || !h->dN_tau || !h->dN_r || !h->vn_re || !h->vn_im || !h->yield) return set_error(IS3D_EINVAL, "null argument");
    if (bins->kernel_form < 0 || bins->kernel_form > 2) return set_error(IS3D_EINVAL, "kernel_form = %d: 0, 1 or 2", bins->kernel_form);
    return IS3D_OK;
}
// ... and kernel_form = 2 on a block that the private form of the kernel that would run cannot hold
int check_bin_args_lds(const is3d_sampler_test_bins *bins, const is3d_sampler_hist *h, int32_t n_events, int32_t n_species, bool fuse)
{
    if (int rc = check_bin_args(bins, h, n_events)) return rc;
    const is3d::SamplerHistLayout l = is3d::sampler_hist_layout(*bins, n_species);
    if (bins->kernel_form == 2 && !(fuse ? is3d::sampler_fused_lds_fits(l) : is3d::sampler_bins_lds_fits(l)))
        return is3d::set_error(IS3D_EINVAL, "kernel_form = 2: %lld histogram words do not fit the LDS", (long long)l.total);
    return IS3D_OK;
}
// the arrays of a histogram set in the order of SamplerHistLayout, with their lengths
struct HistParts {
    int64_t *p[7];
    int64_t n[7];
};
HistParts hist_parts(const is3d_sampler_hist &h, const is3d::SamplerHistLayout &l)
{
    return {{h.dN_dy, h.dN_deta, h.dN_pT, h.dN_tau, h.dN_r, h.vn_re, h.vn_im},
            {l.de - l.dy, l.dp - l.de, l.dt - l.dp, l.dr - l.dt, l.vr - l.dr, l.vi - l.vr, l.total - l.vi}};
}
// a binned run's histograms: the caller's arrays zeroed and, where anything will be binned, the device block d_hist (histograms, then yields)
// grown to `words` on the current device and zeroed ...
int hist_begin(DevMem &d_hist, const HistParts &parts, const is3d_sampler_hist *hist, int32_t n_events, int64_t words, bool device)
{
    for (int a = 0; a < 7; a++) memset(parts.p[a], 0, (size_t)parts.n[a] * sizeof(int64_t));
    memset(hist->yield, 0, (size_t)n_events * sizeof(int64_t));
    if (!device) return IS3D_OK;
    if ((size_t)words * sizeof(int64_t) > d_hist.n) HIP_TRY(d_hist.alloc((size_t)words * sizeof(int64_t)));
    HIP_TRY(hipMemsetAsync(d_hist.p, 0, (size_t)words * sizeof(int64_t), nullptr));
    return IS3D_OK;
}
// ... and after the last batch the one copy to the caller's arrays
int hist_end(const DevMem &d_hist, const HistParts &parts, const is3d_sampler_hist *hist, int32_t n_events, int64_t words)
{
    std::vector<int64_t> h((size_t)words);
    HIP_TRY(hipMemcpy(h.data(), d_hist.p, (size_t)words * sizeof(int64_t), hipMemcpyDeviceToHost));
    const int64_t *src = h.data();
    for (int a = 0; a < 7; a++) {
        memcpy(parts.p[a], src, (size_t)parts.n[a] * sizeof(int64_t));
        src += parts.n[a];
    }
    memcpy(hist->yield, src, (size_t)n_events * sizeof(int64_t));
    return IS3D_OK;
}
int hist_check_counts(const HistParts &parts, const is3d_sampler_hist *hist)
{
    for (int64_t j = 0; j < parts.n[2]; j++)
        if (hist->dN_pT[j] > IS3D_SAMPLER_VN_MAX_COUNT)
            return is3d::set_error(IS3D_EDOMAIN, "dN_pT bin %lld holds %lld hadrons: the fixed-point harmonic sums are exact up to %lld per bin", (long long)j,
                                   (long long)hist->dN_pT[j], (long long)IS3D_SAMPLER_VN_MAX_COUNT);
    return IS3D_OK;
}
}  // namespace

int is3d::sampler_check_bin_args(const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int32_t n_events, int32_t n_species)
{
    return check_bin_args_lds(bins, hist, n_events, n_species, false);
}

int is3d::sampler_check_fused_args(const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int32_t n_events, int32_t n_species)
{
    return check_bin_args_lds(bins, hist, n_events, n_species, true);
}

int is3d::sampler_hist_begin(DevMem &d_hist, const is3d_sampler_hist *hist, const SamplerHistLayout &l, int32_t n_events, int64_t extra_words,
                             bool device)
{
    return hist_begin(d_hist, hist_parts(*hist, l), hist, n_events, l.total + n_events + extra_words, device);
}

int is3d::sampler_hist_end(const DevMem &d_hist, const is3d_sampler_hist *hist, const SamplerHistLayout &l, int32_t n_events)
{
    return hist_end(d_hist, hist_parts(*hist, l), hist, n_events, l.total + n_events);
}

int is3d::sampler_hist_check_counts(const is3d_sampler_hist *hist, const SamplerHistLayout &l) { return hist_check_counts(hist_parts(*hist, l), hist); }

int is3d::sampler_variant_execute_binned(is3d_sampler_plan *P, const SamplerVariant &v, int64_t n_cells, const double *x_dev, const double *y_dev,
                                         int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                         const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, bool fuse, int64_t *n_particles,
                                         is3d_sampler_stats *stats)
{
    *n_particles = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_cells < 0 || n_cells + first_cell > 0xffffffffLL) return set_error(IS3D_EINVAL, "cell indices must fit 32 bits for the counter-based streams");
    const BinRun br{*bins, sampler_bin_widths(*bins), sampler_hist_layout(*bins, P->sp.npart)};
    const HistParts parts = hist_parts(*hist, br.layout);
    const int64_t words = br.layout.total + n_events;
    if (n_cells > 0) HIP_TRY(hipSetDevice(P->device));
    if (int rc = hist_begin(P->d_hist, parts, hist, n_events, words, n_cells > 0)) return rc;
    int64_t listed = 0;
    const int rc = sampler_batches(P, v, n_cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, nullptr, 0, &br, fuse, &listed, stats);
    if (rc && !(rc == IS3D_EDOMAIN && v.edomain_keeps_rest)) return rc;
    if (n_cells == 0) return IS3D_OK;
    const std::string kept = rc ? is3d_last_error() : "";
    if (int rc2 = hist_end(P->d_hist, parts, hist, n_events, words)) return rc2;
    *n_particles = listed;
    if (fuse)   // no list was counted: the hadrons are the sum of the yields
        for (int32_t e = 0; e < n_events; e++) *n_particles += hist->yield[e];
    if (rc) return set_error(rc, "%s", kept.c_str());
    return hist_check_counts(parts, hist);
}

namespace {
// is3d_sampler_plan_execute_binned (fuse = false: the list-and-bin route, the yardstick of the fused one) | is3d_sampler_plan_execute_fused
int plan_execute_binned(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev, int32_t n_events, uint64_t seed,
                        int64_t first_cell, int32_t batch_events, const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist,
                        int64_t *n_particles, is3d_sampler_stats *stats, bool fuse)
{
    using is3d::set_error;
    if (!P || !cells || !n_particles) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (int rc = check_bin_args_lds(bins, hist, n_events, P->sp.npart, fuse)) return rc;
    if (int rc = bind_cells(P, cells, first_cell)) return rc;
    return is3d::sampler_variant_execute_binned(P, P->viscous, cells->n_cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, bins, hist, fuse,
                                                n_particles, stats);
}
}  // namespace

extern "C" int is3d_sampler_plan_execute_binned(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev,
                                                int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                                const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int64_t *n_particles,
                                                is3d_sampler_stats *stats)
{
    return plan_execute_binned(P, cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, bins, hist, n_particles, stats, false);
}

// every hadron binned where it is sampled (cf_sampler_fused): Poisson, select and one launch per event batch
extern "C" int is3d_sampler_plan_execute_fused(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev,
                                               int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                               const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int64_t *n_particles,
                                               is3d_sampler_stats *stats)
{
    return plan_execute_binned(P, cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, bins, hist, n_particles, stats, true);
}

namespace {
// the host-pointer entries: plan + upload + execute_binned | execute_fused
int sample_binned(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                  const is3d_options *opts, const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int64_t *n_particles,
                  is3d_sampler_stats *stats, bool fuse)
{
    using is3d::set_error;
    if (!cells || !species || !df || !in || !opts || !n_particles) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (int rc = check_bin_args(bins, hist, in->n_events)) return rc;
    // (the fused entry refuses a private form that cannot run with the bins, before the plan: no refusal of its own needs a device)
    if (fuse && species->n >= 1)
        if (int rc = is3d::sampler_check_fused_args(bins, hist, in->n_events, species->n)) return rc;
    StagedRun r;
    if (int rc = stage_run(r, cells, species, df, in, opts)) return rc;
    const int rc = plan_execute_binned(r.P, &r.dc, r.xy[0], r.xy[1], in->n_events, in->seed, in->first_cell, in->batch_events, bins, hist,
                                       n_particles, stats, fuse);
    if (stats) stats->ms_h2d = r.ms_h2d;
    return rc;
}
}  // namespace

extern "C" int is3d_sample_binned(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                                  const is3d_options *opts, const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist,
                                  int64_t *n_particles, is3d_sampler_stats *stats)
{
    return sample_binned(cells, species, df, in, opts, bins, hist, n_particles, stats, false);
}

extern "C" int is3d_sample_fused(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                                 const is3d_options *opts, const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist,
                                 int64_t *n_particles, is3d_sampler_stats *stats)
{
    return sample_binned(cells, species, df, in, opts, bins, hist, n_particles, stats, true);
}

// ------------------------------------------------------------------------------------------------
// binned twice: the thermal hadrons of each event batch as above and, from the same workspace, their decay products (cf_decays_mc.hip)
// ------------------------------------------------------------------------------------------------
extern "C" int is3d_sampler_plan_execute_decayed_binned(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev,
                                                        int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                                        const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist,
                                                        const is3d_decay_mc_table *table, const int32_t *slot, int32_t n_slots,
                                                        uint64_t decay_seed, int32_t lifetime, const is3d_sampler_hist *hist_decayed,
                                                        int64_t *n_particles, int64_t *n_final, int64_t *n_unbinned, is3d_sampler_stats *stats,
                                                        is3d_decay_mc_stats *decay_stats)
{
    using is3d::set_error;
    if (!P || !cells || !n_particles || !table || !n_final || !n_unbinned) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = *n_final = *n_unbinned = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (decay_stats) memset(decay_stats, 0, sizeof *decay_stats);
    if (int rc = check_bin_args_lds(bins, hist, n_events, P->sp.npart, false)) return rc;
    if (n_slots < 1) return set_error(IS3D_EINVAL, "n_slots = %d: the decayed histograms hold at least one species", n_slots);
    if (int rc = check_bin_args(bins, hist_decayed, n_events)) return rc;
    if (int rc = is3d::decay_mc_check_slots(is3d::decay_mc_table_entries(table), slot, n_slots, bins)) return rc;
    if (is3d::decay_mc_table_chosen(table) != P->sp.npart)
        return set_error(IS3D_EINVAL, "the decay table was created for %d chosen species, the sampler plan for %d", is3d::decay_mc_table_chosen(table),
                         P->sp.npart);
    if (is3d::decay_mc_table_device(table) != P->device)
        return set_error(IS3D_EINVAL, "the decay table lives on device %d, the sampler plan on device %d", is3d::decay_mc_table_device(table), P->device);
    if (int rc = bind_cells(P, cells, first_cell)) return rc;
    const int64_t n_cells = cells->n_cells;
    const BinRun br{*bins, is3d::sampler_bin_widths(*bins), is3d::sampler_hist_layout(*bins, P->sp.npart)};
    const is3d::SamplerHistLayout ld = is3d::sampler_hist_layout(*bins, n_slots);
    const HistParts parts = hist_parts(*hist, br.layout), parts_d = hist_parts(*hist_decayed, ld);
    const int64_t words = br.layout.total + n_events, words_d = ld.total + n_events;
    const int32_t n_entries = is3d::decay_mc_table_entries(table);
    is3d_decay_mc_stats dst{};
    is3d::decay_mc_table_stats(table, &dst);
    if (n_cells > 0) HIP_TRY(hipSetDevice(P->device));
    // the thermal block as in execute_binned; the decayed block (histograms | yields | tallies) and the slot map sized at first use
    if (int rc = hist_begin(P->d_hist, parts, hist, n_events, words, n_cells > 0)) return rc;
    if (int rc = hist_begin(P->d_hist_decayed, parts_d, hist_decayed, n_events, words_d + is3d::kDecayMcBinTallies, n_cells > 0)) return rc;
    if (n_cells > 0) {
        if ((size_t)n_entries * sizeof(int32_t) > P->d_slot.n) HIP_TRY(P->d_slot.alloc((size_t)n_entries * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(P->d_slot.p, slot, (size_t)n_entries * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    const is3d::DecayMcBinRun run{table, P->d_slot.as<int32_t>(), n_slots, n_events, decay_seed, lifetime, *bins, br.widths, ld,
                                  P->d_hist_decayed.as<unsigned long long>()};
    int64_t listed = 0;
    double ms_decay = 0.0;
    if (int rc = sampler_batches(P, P->viscous, n_cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, nullptr, 0, &br, false, &listed, stats,
                                 &run, &ms_decay))
        return rc;
    dst.n_primaries = listed;
    dst.ms_bin = ms_decay;
    if (n_cells == 0) {
        if (decay_stats) *decay_stats = dst;
        return IS3D_OK;
    }
    if (int rc = hist_end(P->d_hist, parts, hist, n_events, words)) return rc;
    if (int rc = hist_end(P->d_hist_decayed, parts_d, hist_decayed, n_events, words_d)) return rc;
    unsigned long long tally[is3d::kDecayMcBinTallies];
    HIP_TRY(hipMemcpy(tally, run.block_dev + words_d, sizeof tally, hipMemcpyDeviceToHost));
    const int rc_t = is3d::decay_mc_bins_tallies(tally, &dst);
    int64_t binned = 0;
    for (int32_t e = 0; e < n_events; e++) binned += hist_decayed->yield[e];
    *n_particles = listed;
    *n_final = dst.n_final;
    *n_unbinned = dst.n_final - binned;
    if (decay_stats) *decay_stats = dst;
    if (rc_t) return rc_t;
    if (int rc = hist_check_counts(parts, hist)) return rc;
    return hist_check_counts(parts_d, hist_decayed);
}

// host-pointer one-shot: create, upload, execute, destroy (the table included)
extern "C" int is3d_sample_decayed_binned(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                                          const is3d_options *opts, const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist,
                                          const is3d_decay_table *table, const int64_t *chosen_mc_id, const int32_t *slot, int32_t n_slots,
                                          uint64_t decay_seed, int32_t lifetime, const is3d_sampler_hist *hist_decayed, int64_t *n_particles,
                                          int64_t *n_final, int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    using is3d::set_error;
    if (!cells || !species || !df || !in || !opts || !n_particles || !table || !chosen_mc_id || !n_final || !n_unbinned)
        return set_error(IS3D_EINVAL, "null argument");
    *n_particles = *n_final = *n_unbinned = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (decay_stats) memset(decay_stats, 0, sizeof *decay_stats);
    if (int rc = check_bin_args(bins, hist, in->n_events)) return rc;
    if (n_slots < 1) return set_error(IS3D_EINVAL, "n_slots = %d: the decayed histograms hold at least one species", n_slots);
    if (int rc = check_bin_args(bins, hist_decayed, in->n_events)) return rc;
    if (int rc = is3d::decay_mc_check_slots(table->n, slot, n_slots, bins)) return rc;
    // (the table's refusals on the host first, then the plan's: none of them needs a device)
    if (int rc = is3d::decay_mc_table_check(table, species->n, chosen_mc_id)) return rc;
    StagedRun r;
    if (int rc = stage_run(r, cells, species, df, in, opts)) return rc;
    struct TableGuard { is3d_decay_mc_table *t = nullptr; ~TableGuard() { is3d_decay_mc_table_destroy(t); } } tg;
    if (int rc = is3d_decay_mc_table_create(&tg.t, table, species->n, chosen_mc_id, r.P->device)) return rc;
    const int rc = is3d_sampler_plan_execute_decayed_binned(r.P, &r.dc, r.xy[0], r.xy[1], in->n_events, in->seed, in->first_cell, in->batch_events,
                                                            bins, hist, tg.t, slot, n_slots, decay_seed, lifetime, hist_decayed, n_particles, n_final,
                                                            n_unbinned, stats, decay_stats);
    if (stats) stats->ms_h2d = r.ms_h2d;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// per-event flow records: each event batch's list, in the plan's workspace, through cf_sampler_flow and (with a table) cf_decay_mc_flow
// ------------------------------------------------------------------------------------------------
namespace {
// The records of a flow entry, plain or differential: the differential ones on the edge table pT_edges[n_pT + 1] are
// flow records of n_slots * n_pT slots, so one body serves is3d_sampler_plan_execute_flow and is3d_sampler_plan_execute_flow_diff.
struct FlowRecordsArg {
    const is3d_flow_records *plain, *plain_decayed;
    const is3d_flow_diff_records *diff, *diff_decayed;
    int32_t n_pT;                     // 0: plain
    const double *pT_edges;
    bool differential;
    int check(const is3d_flow_cuts *cuts, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species, bool decayed) const
    {
        const int static_words = decayed ? is3d::kDecayMcBinTallies : 0;
        if (differential)
            return is3d::flow_diff_check_args(cuts, n_pT, pT_edges, n_events, n_slots, slot, n_species, decayed ? diff_decayed : diff, static_words);
        return is3d::flow_check_args(cuts, n_events, n_slots, slot, n_species, decayed ? plain_decayed : plain, static_words);
    }
};

int execute_flow(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev, int32_t n_events, uint64_t seed,
                 int64_t first_cell, int32_t batch_events, const is3d_flow_cuts *cuts, const FlowRecordsArg &arg, const int32_t *slot, int32_t n_slots,
                 const is3d_decay_mc_table *table, const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                 int64_t *n_particles, int64_t *n_final, int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    using is3d::set_error;
    if (!P || !cells || !n_particles || (table && (!n_final || !n_unbinned))) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (n_final) *n_final = 0;
    if (n_unbinned) *n_unbinned = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (decay_stats) memset(decay_stats, 0, sizeof *decay_stats);
    if (int rc = arg.check(cuts, n_events, n_slots, slot, P->sp.npart, false)) return rc;
    const int32_t n_entries = table ? is3d::decay_mc_table_entries(table) : 0;
    if (table) {
        if (int rc = arg.check(cuts, n_events, n_slots_decayed, slot_decayed, n_entries, true)) return rc;
        if (is3d::decay_mc_table_chosen(table) != P->sp.npart)
            return set_error(IS3D_EINVAL, "the decay table was created for %d chosen species, the sampler plan for %d", is3d::decay_mc_table_chosen(table),
                             P->sp.npart);
        if (is3d::decay_mc_table_device(table) != P->device)
            return set_error(IS3D_EINVAL, "the decay table lives on device %d, the sampler plan on device %d", is3d::decay_mc_table_device(table), P->device);
    }
    if (int rc = bind_cells(P, cells, first_cell)) return rc;
    const int64_t n_cells = cells->n_cells;
    if (n_cells < 0 || n_cells + first_cell > 0xffffffffLL) return set_error(IS3D_EINVAL, "cell indices must fit 32 bits for the counter-based streams");
    // the blocks hold n_keys = n_slots (* n_pT) records per event
    const int32_t n_pT = arg.differential ? arg.n_pT : 0, n_keys = n_pT ? n_slots * n_pT : n_slots, n_keys_decayed = n_pT ? n_slots_decayed * n_pT : n_slots_decayed;
    const is3d_flow_records view = arg.differential ? is3d::flow_diff_view(*arg.diff) : *arg.plain;
    const is3d_flow_records view_decayed = !table ? is3d_flow_records{} : (arg.differential ? is3d::flow_diff_view(*arg.diff_decayed) : *arg.plain_decayed);
    const is3d_flow_records *records = &view, *records_decayed = &view_decayed;
    const size_t words = (size_t)n_events * n_keys * is3d::kFlowRecordWords;
    const size_t words_d = table ? (size_t)n_events * n_keys_decayed * is3d::kFlowRecordWords : 0;
    is3d_decay_mc_stats dst{};
    if (table) is3d::decay_mc_table_stats(table, &dst);
    is3d::flow_records_zero(records, n_events, n_keys);
    if (table) is3d::flow_records_zero(records_decayed, n_events, n_keys_decayed);
    if (n_cells == 0) {
        if (decay_stats) *decay_stats = dst;
        return IS3D_OK;
    }
    HIP_TRY(hipSetDevice(P->device));
    // the record blocks and slot maps, sized at first use and kept by the plan
    const auto grow = [](DevMem &d, size_t bytes) { return bytes > d.n ? d.alloc(bytes) : hipSuccess; };
    HIP_TRY(grow(P->d_flow, words * sizeof(int64_t)));
    HIP_TRY(hipMemsetAsync(P->d_flow.p, 0, words * sizeof(int64_t), nullptr));
    HIP_TRY(grow(P->d_flow_slot, (size_t)P->sp.npart * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(P->d_flow_slot.p, slot, (size_t)P->sp.npart * sizeof(int32_t), hipMemcpyHostToDevice));
    const is3d::FlowThresholds th = is3d::flow_thresholds(*cuts);
    if (n_pT) {
        HIP_TRY(grow(P->d_flow_edges, ((size_t)n_pT + 1) * sizeof(double)));
        HIP_TRY(hipMemcpy(P->d_flow_edges.p, arg.pT_edges, ((size_t)n_pT + 1) * sizeof(double), hipMemcpyHostToDevice));
    }
    const double *edges_dev = n_pT ? P->d_flow_edges.as<double>() : nullptr;
    is3d::DecayMcFlowRun drun{};
    if (table) {
        HIP_TRY(grow(P->d_flow_decayed, (words_d + is3d::kDecayMcBinTallies) * sizeof(int64_t)));
        HIP_TRY(hipMemsetAsync(P->d_flow_decayed.p, 0, (words_d + is3d::kDecayMcBinTallies) * sizeof(int64_t), nullptr));
        HIP_TRY(grow(P->d_flow_slot_decayed, (size_t)n_entries * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(P->d_flow_slot_decayed.p, slot_decayed, (size_t)n_entries * sizeof(int32_t), hipMemcpyHostToDevice));
        drun = is3d::DecayMcFlowRun{table, P->d_flow_slot_decayed.as<int32_t>(), n_slots_decayed, n_events, decay_seed, lifetime, *cuts, th,
                                    P->d_flow_decayed.as<unsigned long long>(), n_pT, edges_dev};
    }
    FlowRun run{*cuts, th, n_slots, P->d_flow_slot.as<int32_t>(), P->d_flow.as<unsigned long long>(), table ? &drun : nullptr, 0.0, nullptr, nullptr, nullptr, nullptr};
    run.n_pT = n_pT;
    run.edges_dev = edges_dev;
    int64_t listed = 0;
    if (int rc = sampler_batches(P, P->viscous, n_cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, nullptr, 0, nullptr, false, &listed, stats,
                                 nullptr, nullptr, &run))
        return rc;
    *n_particles = listed;
    std::vector<int64_t> h(std::max(words, words_d + is3d::kDecayMcBinTallies));
    HIP_TRY(hipMemcpy(h.data(), P->d_flow.p, words * sizeof(int64_t), hipMemcpyDeviceToHost));
    is3d::flow_records_scatter(h.data(), records, n_events, n_keys);
    int rc_t = IS3D_OK;
    if (table) {
        HIP_TRY(hipMemcpy(h.data(), P->d_flow_decayed.p, (words_d + is3d::kDecayMcBinTallies) * sizeof(int64_t), hipMemcpyDeviceToHost));
        is3d::flow_records_scatter(h.data(), records_decayed, n_events, n_keys_decayed);
        rc_t = is3d::decay_mc_bins_tallies((const unsigned long long *)(h.data() + words_d), &dst);
        int64_t kept = 0;
        for (size_t j = 0; j < (size_t)n_events * n_keys_decayed; j++) kept += records_decayed->M[j * is3d::kFlowRegions];
        dst.n_primaries = listed;
        dst.ms_bin = run.ms_decay;
        *n_final = dst.n_final;
        *n_unbinned = dst.n_final - kept;
        if (decay_stats) *decay_stats = dst;
    }
    if (rc_t) return rc_t;
    if (int rc = is3d::flow_records_check(records, n_events, n_keys)) return rc;
    return table ? is3d::flow_records_check(records_decayed, n_events, n_keys_decayed) : IS3D_OK;
}
}  // namespace

extern "C" int is3d_sampler_plan_execute_flow(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev,
                                              int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                              const is3d_flow_cuts *cuts, const int32_t *slot, int32_t n_slots,
                                              const is3d_flow_records *records, const is3d_decay_mc_table *table, const int32_t *slot_decayed,
                                              int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                                              const is3d_flow_records *records_decayed, int64_t *n_particles, int64_t *n_final,
                                              int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    const FlowRecordsArg arg{records, records_decayed, nullptr, nullptr, 0, nullptr, false};
    return execute_flow(P, cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, cuts, arg, slot, n_slots, table, slot_decayed, n_slots_decayed,
                        decay_seed, lifetime, n_particles, n_final, n_unbinned, stats, decay_stats);
}

extern "C" int is3d_sampler_plan_execute_flow_diff(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev,
                                                   int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                                   const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges, const int32_t *slot,
                                                   int32_t n_slots, const is3d_flow_diff_records *records, const is3d_decay_mc_table *table,
                                                   const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                                                   const is3d_flow_diff_records *records_decayed, int64_t *n_particles, int64_t *n_final,
                                                   int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    const FlowRecordsArg arg{nullptr, nullptr, records, records_decayed, n_pT, pT_edges, true};
    return execute_flow(P, cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, cuts, arg, slot, n_slots, table, slot_decayed, n_slots_decayed,
                        decay_seed, lifetime, n_particles, n_final, n_unbinned, stats, decay_stats);
}

// host-pointer one-shot: create, upload, execute, destroy (the table included)
extern "C" int is3d_sample_flow(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                                const is3d_options *opts, const is3d_flow_cuts *cuts, const int32_t *slot, int32_t n_slots,
                                const is3d_flow_records *records, const is3d_decay_table *table, const int64_t *chosen_mc_id,
                                const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                                const is3d_flow_records *records_decayed, int64_t *n_particles, int64_t *n_final, int64_t *n_unbinned,
                                is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    using is3d::set_error;
    if (!cells || !species || !df || !in || !opts || !n_particles || (table && (!chosen_mc_id || !n_final || !n_unbinned)))
        return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (n_final) *n_final = 0;
    if (n_unbinned) *n_unbinned = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (decay_stats) memset(decay_stats, 0, sizeof *decay_stats);
    if (species->n < 1) return set_error(IS3D_EINVAL, "the species list is empty");
    if (int rc = is3d::flow_check_args(cuts, in->n_events, n_slots, slot, species->n, records, 0)) return rc;
    if (table) {
        if (table->n < 1) return set_error(IS3D_EINVAL, "decay table: n = %d", table->n);
        if (int rc = is3d::flow_check_args(cuts, in->n_events, n_slots_decayed, slot_decayed, table->n, records_decayed, is3d::kDecayMcBinTallies)) return rc;
        if (int rc = is3d::decay_mc_table_check(table, species->n, chosen_mc_id)) return rc;
    }
    StagedRun r;
    if (int rc = stage_run(r, cells, species, df, in, opts)) return rc;
    struct TableGuard { is3d_decay_mc_table *t = nullptr; ~TableGuard() { is3d_decay_mc_table_destroy(t); } } tg;
    if (table)
        if (int rc = is3d_decay_mc_table_create(&tg.t, table, species->n, chosen_mc_id, r.P->device)) return rc;
    const int rc = is3d_sampler_plan_execute_flow(r.P, &r.dc, r.xy[0], r.xy[1], in->n_events, in->seed, in->first_cell, in->batch_events, cuts, slot,
                                                  n_slots, records, tg.t, slot_decayed, n_slots_decayed, decay_seed, lifetime, records_decayed,
                                                  n_particles, n_final, n_unbinned, stats, decay_stats);
    if (stats) stats->ms_h2d = r.ms_h2d;
    return rc;
}

extern "C" int is3d_sample_flow_diff(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                                     const is3d_options *opts, const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges, const int32_t *slot,
                                     int32_t n_slots, const is3d_flow_diff_records *records, const is3d_decay_table *table,
                                     const int64_t *chosen_mc_id, const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed,
                                     int32_t lifetime, const is3d_flow_diff_records *records_decayed, int64_t *n_particles, int64_t *n_final,
                                     int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    using is3d::set_error;
    if (!cells || !species || !df || !in || !opts || !n_particles || (table && (!chosen_mc_id || !n_final || !n_unbinned)))
        return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (n_final) *n_final = 0;
    if (n_unbinned) *n_unbinned = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (decay_stats) memset(decay_stats, 0, sizeof *decay_stats);
    if (species->n < 1) return set_error(IS3D_EINVAL, "the species list is empty");
    if (int rc = is3d::flow_diff_check_args(cuts, n_pT, pT_edges, in->n_events, n_slots, slot, species->n, records, 0)) return rc;
    if (table) {
        if (table->n < 1) return set_error(IS3D_EINVAL, "decay table: n = %d", table->n);
        if (int rc = is3d::flow_diff_check_args(cuts, n_pT, pT_edges, in->n_events, n_slots_decayed, slot_decayed, table->n, records_decayed,
                                                is3d::kDecayMcBinTallies))
            return rc;
        if (int rc = is3d::decay_mc_table_check(table, species->n, chosen_mc_id)) return rc;
    }
    StagedRun r;
    if (int rc = stage_run(r, cells, species, df, in, opts)) return rc;
    struct TableGuard { is3d_decay_mc_table *t = nullptr; ~TableGuard() { is3d_decay_mc_table_destroy(t); } } tg;
    if (table)
        if (int rc = is3d_decay_mc_table_create(&tg.t, table, species->n, chosen_mc_id, r.P->device)) return rc;
    const int rc = is3d_sampler_plan_execute_flow_diff(r.P, &r.dc, r.xy[0], r.xy[1], in->n_events, in->seed, in->first_cell, in->batch_events, cuts, n_pT,
                                                       pT_edges, slot, n_slots, records, tg.t, slot_decayed, n_slots_decayed, decay_seed, lifetime,
                                                       records_decayed, n_particles, n_final, n_unbinned, stats, decay_stats);
    if (stats) stats->ms_h2d = r.ms_h2d;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// two-particle (delta y, delta phi) histograms: each event batch's list, in the plan's workspace, through cf_pair_cells and (with a table)
// cf_decay_mc_pairs into occupancy blocks that live for the whole run; after the last batch cf_pair_correlate for each block
// ------------------------------------------------------------------------------------------------
extern "C" int is3d_sampler_plan_execute_pairs(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev,
                                               int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                               const is3d_pair_bins *bins, const int32_t *slot, int32_t n_slots, const is3d_pair_hist *hist,
                                               const is3d_decay_mc_table *table, const int32_t *slot_decayed, int32_t n_slots_decayed,
                                               uint64_t decay_seed, int32_t lifetime, const is3d_pair_hist *hist_decayed, int64_t *n_particles,
                                               int64_t *n_final, int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    using is3d::set_error;
    if (!P || !cells || !n_particles || (table && (!n_final || !n_unbinned))) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (n_final) *n_final = 0;
    if (n_unbinned) *n_unbinned = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (decay_stats) memset(decay_stats, 0, sizeof *decay_stats);
    if (int rc = is3d::pair_check_args(bins, n_events, n_slots, slot, P->sp.npart, hist)) return rc;
    const int32_t n_entries = table ? is3d::decay_mc_table_entries(table) : 0;
    if (table) {
        if (int rc = is3d::pair_check_args(bins, n_events, n_slots_decayed, slot_decayed, n_entries, hist_decayed)) return rc;
        if (is3d::decay_mc_table_chosen(table) != P->sp.npart)
            return set_error(IS3D_EINVAL, "the decay table was created for %d chosen species, the sampler plan for %d", is3d::decay_mc_table_chosen(table),
                             P->sp.npart);
        if (is3d::decay_mc_table_device(table) != P->device)
            return set_error(IS3D_EINVAL, "the decay table lives on device %d, the sampler plan on device %d", is3d::decay_mc_table_device(table), P->device);
    }
    if (int rc = bind_cells(P, cells, first_cell)) return rc;
    const int64_t n_cells = cells->n_cells;
    if (n_cells < 0 || n_cells + first_cell > 0xffffffffLL) return set_error(IS3D_EINVAL, "cell indices must fit 32 bits for the counter-based streams");
    is3d_decay_mc_stats dst{};
    if (table) is3d::decay_mc_table_stats(table, &dst);
    is3d::pair_hist_zero(*bins, hist, n_events, n_slots);
    if (table) is3d::pair_hist_zero(*bins, hist_decayed, n_events, n_slots_decayed);
    if (n_cells == 0) {
        if (decay_stats) *decay_stats = dst;
        return IS3D_OK;
    }
    HIP_TRY(hipSetDevice(P->device));
    // the occupancy blocks, the histogram block and the slot maps, sized at first use and kept by the plan
    const auto grow = [](DevMem &d, size_t bytes) { return bytes > d.n ? d.alloc(bytes) : hipSuccess; };
    constexpr size_t head = is3d::kDecayMcBinTallies * sizeof(unsigned long long);
    const size_t out_words = is3d::pair_out_words(*bins, n_events, n_slots);
    const size_t out_words_d = table ? is3d::pair_out_words(*bins, n_events, n_slots_decayed) : 0;
    if (int rc = is3d::pair_occ_begin(P->d_pair_occ, 0, is3d::pair_occ_words(*bins, n_events, n_slots))) return rc;
    HIP_TRY(grow(P->d_pair_out, std::max(out_words, out_words_d) * sizeof(int64_t)));
    HIP_TRY(grow(P->d_pair_slot, (size_t)P->sp.npart * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(P->d_pair_slot.p, slot, (size_t)P->sp.npart * sizeof(int32_t), hipMemcpyHostToDevice));
    const is3d::PairTables tables = is3d::pair_tables(*bins);
    is3d::DecayMcPairRun drun{};
    if (table) {
        if (int rc = is3d::pair_occ_begin(P->d_pair_occ_decayed, head, is3d::pair_occ_words(*bins, n_events, n_slots_decayed))) return rc;
        HIP_TRY(grow(P->d_pair_slot_decayed, (size_t)n_entries * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(P->d_pair_slot_decayed.p, slot_decayed, (size_t)n_entries * sizeof(int32_t), hipMemcpyHostToDevice));
        drun = is3d::DecayMcPairRun{table, P->d_pair_slot_decayed.as<int32_t>(), n_slots_decayed, n_events, decay_seed, lifetime, *bins, tables,
                                    P->d_pair_occ_decayed.as<unsigned long long>(), (unsigned *)(P->d_pair_occ_decayed.p + head)};
    }
    FlowRun run{};
    run.n_slots = n_slots;
    run.slot_dev = P->d_pair_slot.as<int32_t>();
    run.pair_bins = bins;
    run.pair_tables = &tables;
    run.occ_dev = P->d_pair_occ.as<unsigned>();
    run.pair_decay = table ? &drun : nullptr;
    int64_t listed = 0;
    if (int rc = sampler_batches(P, P->viscous, n_cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, nullptr, 0, nullptr, false, &listed, stats,
                                 nullptr, nullptr, &run))
        return rc;
    *n_particles = listed;
    std::vector<int64_t> h(std::max(out_words, out_words_d));
    HIP_TRY(is3d::pair_correlate_launch(*bins, n_events, n_slots, run.occ_dev, P->d_pair_out.as<unsigned long long>()));
    HIP_TRY(hipMemcpy(h.data(), P->d_pair_out.p, out_words * sizeof(int64_t), hipMemcpyDeviceToHost));
    is3d::pair_hist_scatter(*bins, h.data(), hist, n_events, n_slots);
    int rc_t = IS3D_OK;
    if (table) {
        HIP_TRY(is3d::pair_correlate_launch(*bins, n_events, n_slots_decayed, drun.occ_dev, P->d_pair_out.as<unsigned long long>()));
        HIP_TRY(hipMemcpy(h.data(), P->d_pair_out.p, out_words_d * sizeof(int64_t), hipMemcpyDeviceToHost));
        is3d::pair_hist_scatter(*bins, h.data(), hist_decayed, n_events, n_slots_decayed);
        unsigned long long tally[is3d::kDecayMcBinTallies];
        HIP_TRY(hipMemcpy(tally, P->d_pair_occ_decayed.p, sizeof tally, hipMemcpyDeviceToHost));
        rc_t = is3d::decay_mc_bins_tallies(tally, &dst);
        int64_t kept = 0;
        for (size_t j = 0; j < (size_t)n_events * n_slots_decayed; j++) kept += hist_decayed->M[j];
        dst.n_primaries = listed;
        dst.ms_bin = run.ms_decay;
        *n_final = dst.n_final;
        *n_unbinned = dst.n_final - kept;
        if (decay_stats) *decay_stats = dst;
    }
    if (rc_t) return rc_t;
    if (int rc = is3d::pair_hist_check(hist, n_events, n_slots)) return rc;
    return table ? is3d::pair_hist_check(hist_decayed, n_events, n_slots_decayed) : IS3D_OK;
}

// host-pointer one-shot: create, upload, execute, destroy (the table included)
extern "C" int is3d_sample_pairs(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                                 const is3d_options *opts, const is3d_pair_bins *bins, const int32_t *slot, int32_t n_slots,
                                 const is3d_pair_hist *hist, const is3d_decay_table *table, const int64_t *chosen_mc_id,
                                 const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                                 const is3d_pair_hist *hist_decayed, int64_t *n_particles, int64_t *n_final, int64_t *n_unbinned,
                                 is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    using is3d::set_error;
    if (!cells || !species || !df || !in || !opts || !n_particles || (table && (!chosen_mc_id || !n_final || !n_unbinned)))
        return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (n_final) *n_final = 0;
    if (n_unbinned) *n_unbinned = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (decay_stats) memset(decay_stats, 0, sizeof *decay_stats);
    if (species->n < 1) return set_error(IS3D_EINVAL, "the species list is empty");
    if (int rc = is3d::pair_check_args(bins, in->n_events, n_slots, slot, species->n, hist)) return rc;
    if (table) {
        if (table->n < 1) return set_error(IS3D_EINVAL, "decay table: n = %d", table->n);
        if (int rc = is3d::pair_check_args(bins, in->n_events, n_slots_decayed, slot_decayed, table->n, hist_decayed)) return rc;
        if (int rc = is3d::decay_mc_table_check(table, species->n, chosen_mc_id)) return rc;
    }
    StagedRun r;
    if (int rc = stage_run(r, cells, species, df, in, opts)) return rc;
    struct TableGuard { is3d_decay_mc_table *t = nullptr; ~TableGuard() { is3d_decay_mc_table_destroy(t); } } tg;
    if (table)
        if (int rc = is3d_decay_mc_table_create(&tg.t, table, species->n, chosen_mc_id, r.P->device)) return rc;
    const int rc = is3d_sampler_plan_execute_pairs(r.P, &r.dc, r.xy[0], r.xy[1], in->n_events, in->seed, in->first_cell, in->batch_events, bins, slot,
                                                   n_slots, hist, tg.t, slot_decayed, n_slots_decayed, decay_seed, lifetime, hist_decayed,
                                                   n_particles, n_final, n_unbinned, stats, decay_stats);
    if (stats) stats->ms_h2d = r.ms_h2d;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// HBT correlation histograms: each event batch's list, in the plan's workspace, is selected into compact records and paired (cf_hbt_select,
// cf_hbt_pairs) and, with a table, decayed twice into records that are paired; an event lies whole in one batch, so the records of a batch
// are discarded after it and only the histograms live for the whole run
// ------------------------------------------------------------------------------------------------
extern "C" int is3d_sampler_plan_execute_hbt(is3d_sampler_plan *P, const is3d_cells *cells, const double *x_dev, const double *y_dev,
                                             int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                             const is3d_hbt_bins *bins, const int32_t *slot, int32_t n_slots, const is3d_hbt_hist *hist,
                                             const is3d_decay_mc_table *table, const int32_t *slot_decayed, int32_t n_slots_decayed,
                                             uint64_t decay_seed, int32_t lifetime, const is3d_hbt_hist *hist_decayed, int64_t *n_particles,
                                             int64_t *n_final, int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    using is3d::set_error;
    if (!P || !cells || !n_particles || (table && (!n_final || !n_unbinned))) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (n_final) *n_final = 0;
    if (n_unbinned) *n_unbinned = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (decay_stats) memset(decay_stats, 0, sizeof *decay_stats);
    if (int rc = is3d::hbt_check_args(bins, n_events, n_slots, slot, P->sp.npart, hist, true)) return rc;
    const int32_t n_entries = table ? is3d::decay_mc_table_entries(table) : 0;
    if (table) {
        if (int rc = is3d::hbt_check_args(bins, n_events, n_slots_decayed, slot_decayed, n_entries, hist_decayed, true)) return rc;
        if (is3d::decay_mc_table_chosen(table) != P->sp.npart)
            return set_error(IS3D_EINVAL, "the decay table was created for %d chosen species, the sampler plan for %d", is3d::decay_mc_table_chosen(table),
                             P->sp.npart);
        if (is3d::decay_mc_table_device(table) != P->device)
            return set_error(IS3D_EINVAL, "the decay table lives on device %d, the sampler plan on device %d", is3d::decay_mc_table_device(table), P->device);
    }
    if (int rc = bind_cells(P, cells, first_cell)) return rc;
    const int64_t n_cells = cells->n_cells;
    if (n_cells < 0 || n_cells + first_cell > 0xffffffffLL) return set_error(IS3D_EINVAL, "cell indices must fit 32 bits for the counter-based streams");
    is3d_decay_mc_stats dst{};
    if (table) is3d::decay_mc_table_stats(table, &dst);
    is3d::hbt_hist_zero(*bins, hist, n_events, n_slots);
    if (table) is3d::hbt_hist_zero(*bins, hist_decayed, n_events, n_slots_decayed);
    if (n_cells == 0) {
        if (decay_stats) *decay_stats = dst;
        return IS3D_OK;
    }
    HIP_TRY(hipSetDevice(P->device));
    // the runs own their blocks for this call; the plan keeps nothing of them
    is3d::HbtRun thermal, decayed;
    is3d::DevBuf<int32_t> d_slot, d_slot_decayed;
    is3d::DevBuf<unsigned long long> d_tally;
    if (int rc = thermal.begin(*bins, n_events, n_slots)) return rc;
    HIP_TRY(d_slot.upload(slot, (size_t)P->sp.npart));
    is3d::DecayMcHbtRun drun{};
    if (table) {
        if (int rc = decayed.begin(*bins, n_events, n_slots_decayed)) return rc;
        HIP_TRY(d_slot_decayed.upload(slot_decayed, (size_t)n_entries));
        HIP_TRY(d_tally.alloc(is3d::kDecayMcBinTallies));
        HIP_TRY(hipMemsetAsync(d_tally.p, 0, is3d::kDecayMcBinTallies * sizeof(unsigned long long), nullptr));
        drun = is3d::DecayMcHbtRun{table, d_slot_decayed.p, decay_seed, lifetime, d_tally.p};
    }
    FlowRun run{};
    run.n_slots = n_slots;
    run.slot_dev = d_slot.p;
    run.hbt = &thermal;
    run.hbt_decayed = table ? &decayed : nullptr;
    run.hbt_decay = table ? &drun : nullptr;
    int64_t listed = 0;
    if (int rc = sampler_batches(P, P->viscous, n_cells, x_dev, y_dev, n_events, seed, first_cell, batch_events, nullptr, 0, nullptr, false, &listed, stats,
                                 nullptr, nullptr, &run))
        return rc;
    *n_particles = listed;
    const int rc_h = thermal.finish(hist);
    int rc_t = IS3D_OK, rc_d = IS3D_OK;
    if (table) {
        rc_d = decayed.finish(hist_decayed);
        unsigned long long tally[is3d::kDecayMcBinTallies];
        HIP_TRY(hipMemcpy(tally, d_tally.p, sizeof tally, hipMemcpyDeviceToHost));
        rc_t = is3d::decay_mc_bins_tallies(tally, &dst);
        int64_t kept = 0;
        for (size_t j = 0; j < (size_t)n_events * n_slots_decayed; j++) kept += hist_decayed->M[j];
        dst.n_primaries = listed;
        dst.ms_bin = run.ms_decay;
        *n_final = dst.n_final;
        *n_unbinned = dst.n_final - kept;
        if (decay_stats) *decay_stats = dst;
    }
    if (rc_t) return rc_t;
    return rc_h ? rc_h : rc_d;
}

// host-pointer one-shot: create, upload, execute, destroy (the table included)
extern "C" int is3d_sample_hbt(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                               const is3d_options *opts, const is3d_hbt_bins *bins, const int32_t *slot, int32_t n_slots,
                               const is3d_hbt_hist *hist, const is3d_decay_table *table, const int64_t *chosen_mc_id,
                               const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                               const is3d_hbt_hist *hist_decayed, int64_t *n_particles, int64_t *n_final, int64_t *n_unbinned,
                               is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats)
{
    using is3d::set_error;
    if (!cells || !species || !df || !in || !opts || !n_particles || (table && (!chosen_mc_id || !n_final || !n_unbinned)))
        return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (n_final) *n_final = 0;
    if (n_unbinned) *n_unbinned = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (decay_stats) memset(decay_stats, 0, sizeof *decay_stats);
    if (species->n < 1) return set_error(IS3D_EINVAL, "the species list is empty");
    if (int rc = is3d::hbt_check_args(bins, in->n_events, n_slots, slot, species->n, hist, true)) return rc;
    if (table) {
        if (table->n < 1) return set_error(IS3D_EINVAL, "decay table: n = %d", table->n);
        if (int rc = is3d::hbt_check_args(bins, in->n_events, n_slots_decayed, slot_decayed, table->n, hist_decayed, true)) return rc;
        if (int rc = is3d::decay_mc_table_check(table, species->n, chosen_mc_id)) return rc;
    }
    StagedRun r;
    if (int rc = stage_run(r, cells, species, df, in, opts)) return rc;
    struct TableGuard { is3d_decay_mc_table *t = nullptr; ~TableGuard() { is3d_decay_mc_table_destroy(t); } } tg;
    if (table)
        if (int rc = is3d_decay_mc_table_create(&tg.t, table, species->n, chosen_mc_id, r.P->device)) return rc;
    const int rc = is3d_sampler_plan_execute_hbt(r.P, &r.dc, r.xy[0], r.xy[1], in->n_events, in->seed, in->first_cell, in->batch_events, bins, slot,
                                                 n_slots, hist, tg.t, slot_decayed, n_slots_decayed, decay_seed, lifetime, hist_decayed,
                                                 n_particles, n_final, n_unbinned, stats, decay_stats);
    if (stats) stats->ms_h2d = r.ms_h2d;
    return rc;
}

// a caller's list through the same kernel: upload, sampler_bins_launch, download as is3d_sampler_plan_execute_binned does
extern "C" int is3d_sampler_bin_list_device(const is3d_sampler_test_bins *bins, int32_t n_events, int32_t n_species, int64_t n_particles,
                                            const is3d_particle *particles, const is3d_sampler_hist *hist, int64_t *n_skipped, int32_t device)
{
    using is3d::set_error;
    if (!n_skipped) return set_error(IS3D_EINVAL, "null argument");
    *n_skipped = 0;
    if (int rc = check_bin_args(bins, hist, n_events)) return rc;
    if (n_species < 1) return set_error(IS3D_EINVAL, "n_species must be >= 1");
    if (n_particles < 0 || (n_particles > 0 && !particles)) return set_error(IS3D_EINVAL, "n_particles must be >= 0 and particles non-null");
    if (int rc = is3d::sampler_check_bin_args(bins, hist, n_events, n_species)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    const is3d::SamplerHistLayout l = is3d::sampler_hist_layout(*bins, n_species);
    const HistParts parts = hist_parts(*hist, l);
    const int64_t words = l.total + n_events;
    DevMem d_list, d_hist;
    if (n_particles > 0 && device >= 0) HIP_TRY(hipSetDevice(device));
    if (int rc = hist_begin(d_hist, parts, hist, n_events, words, n_particles > 0)) return rc;
    if (n_particles == 0) return IS3D_OK;
    HIP_TRY(d_list.upload(particles, (size_t)n_particles));
    HIP_TRY(is3d::sampler_bins_launch(*bins, is3d::sampler_bin_widths(*bins), l, n_species, n_events, d_list.as<is3d_particle>(), n_particles,
                                      d_hist.as<unsigned long long>(), d_hist.as<unsigned long long>() + l.total, bins->kernel_form));
    if (int rc = hist_end(d_hist, parts, hist, n_events, words)) return rc;
    int64_t counted = 0;
    for (int32_t e = 0; e < n_events; e++) counted += hist->yield[e];
    *n_skipped = n_particles - counted;
    return hist_check_counts(parts, hist);
}
