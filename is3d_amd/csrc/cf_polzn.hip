// cf_polzn.hip -- hand-written gfx950 kernels and C ABI entries of the spin polarization from thermal vorticity (mode 5).
//
// Replaces EmissionFunctionArray::calculate_spin_polzn (reference src/cpp/emissionfunction_polzn_kernels.cpp:27-265): for every species,
// pT, phi and y the sums over all cells of w p.dsigma f0 spin_mu and of w p.dsigma f0 (include/is3d_amd.h states the integrand).
// Stages:
//   cf_polzn_cells3 / cf_polzn_cells2   lanes <-> (species class, pT), the cell loop wave-uniform; every workgroup owns a tile of bins
//                   (3+1D 4 phi x 3 y, 2+1D 8 phi with the eta sum inside) and one chunk of the cells, and writes its five partial sums per
//                   bin to the chunk's slab.
//   cf_polzn_reduce the chunk slabs summed in chunk order per (species, pT, bin), the class's -1 / (4 m) applied once.
// Over several devices (is3d_spin_polarization_multi, cf_multi.hip) the second stage is split in two:
//   cf_polzn_class_sums  on each shard's device: its chunk slabs summed in chunk order per (class lane, bin), not expanded, not scaled.
//   cf_polzn_shards      on the first device: the shards' class-lane sums added in shard order per (species, pT, bin), then the -1 / (4 m).
// No floating-point atomics: the results are bitwise the same from run to run.
//
// Factorisation.  With A_k = cosh ut - sinh tau un, B_j = cos(phi) ux + sin(phi) uy and u_perp = sqrt(ux^2 + uy^2):
//   z = exp(-p.u / T) = E1_k E2_j,  E1_k = exp((pT u_perp - mT A_k) / T) <= exp(-m / T),  E2_j = exp(pT (B_j - u_perp) / T) <= 1
// (A_k >= sqrt(1 + u_perp^2) and mT sqrt(1 + u_perp^2) - pT u_perp >= m), so neither factor overflows, and wherever the direct exp(p.u / T) is
// finite (z >= 2^-1022) neither factor underflows.  f0 = z / (1 + sign z), f0 (1 - sign f0) = z / (1 + sign z)^2.  p.dsigma and every
// spin_mu / (2 pref) are a (pT, y) part plus a (pT, phi) part:
//   p.dsigma = mT (cosh dat + sinh / tau dan) + pT (cos dax + sin day)
//   t: mT wxy sinh / tau + pT (wyn cos - wxn sin)          x: mT (wyn cosh + wty sinh / tau) - pT wtn sin
//   y: -mT (wxn cosh + wtx sinh / tau) + pT wtn cos         n: mT wxy cosh + pT (wtx sin - wty cos)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <memory>
#include <utility>
#include <vector>

#include "cf_host.h"
#include "cf_math.h"
#include "cf_plan_geometry.h"
#include "cf_polzn.h"

namespace is3d {

struct PolznLane {
    double mT, pT, sign, mTi, pTi;
};

__device__ __forceinline__ PolznLane polzn_lane(const PolznArgs &a, int l)
{
    PolznLane q;
    q.mT = a.lane_mT[l];
    q.pT = a.lane_pT[l];
    q.sign = a.lane_sign[l];
    q.mTi = q.mT * a.invT;
    q.pTi = q.pT * a.invT;
    return q;
}

// one evaluation: the five running sums of a bin.  E1w = E1 w (2+1D eta weight; E1 in 3+1D)
__device__ __forceinline__ void polzn_eval(double E1, double E1w, double MP, const double (&MA)[4], double E2, double PQ, const double (&PB)[4],
                                           double sign, double (&acc)[5])
{
    const double z = E1 * E2;
    const double inv = rcp_nr1(__builtin_fma(sign, z, 1.0));
    const double g = (E1w * E2) * inv;   // w f0
    const double h = g * inv;            // w f0 (1 - sign f0)
    const double pds = MP + PQ;
    acc[4] = __builtin_fma(pds, g, acc[4]);
    const double q = pds * h;
#pragma unroll
    for (int m = 0; m < 4; m++) acc[m] = __builtin_fma(q, MA[m] + PB[m], acc[m]);
}

// the (pT, phi) side of a cell for one phi node
__device__ __forceinline__ void polzn_phi_side(const PolznLane &q, double cp, double sp, double ux, double uy, double uperp, double dax, double day,
                                               double wtx, double wty, double wtn, double wxn, double wyn, double &E2, double &PQ, double (&PB)[4])
{
    const double B = __builtin_fma(cp, ux, sp * uy);
    E2 = exp_p9_sat(q.pTi * (B - uperp));
    PQ = q.pT * __builtin_fma(cp, dax, sp * day);
    PB[0] = q.pT * __builtin_fma(wyn, cp, -wxn * sp);
    PB[1] = q.pT * (-wtn * sp);
    PB[2] = q.pT * (wtn * cp);
    PB[3] = q.pT * __builtin_fma(wtx, sp, -wty * cp);
}

// the (pT, y) side of a cell for ch = cosh(y - eta), sh = sinh(y - eta)
__device__ __forceinline__ void polzn_y_side(const PolznLane &q, double ch, double sh, double tau, double itau, double ut, double un, double pTu,
                                             double dat, double dan, double wtx, double wty, double wxy, double wxn, double wyn, double &E1,
                                             double &MP, double (&MA)[4])
{
    const double shn = sh * itau;
    const double A = __builtin_fma(ch, ut, -(sh * tau) * un);
    E1 = exp_p9_sat(__builtin_fma(-q.mTi, A, pTu));
    MP = q.mT * __builtin_fma(ch, dat, shn * dan);
    MA[0] = q.mT * (wxy * shn);
    MA[1] = q.mT * __builtin_fma(wyn, ch, wty * shn);
    MA[2] = -q.mT * __builtin_fma(wxn, ch, wtx * shn);
    MA[3] = q.mT * (wxy * ch);
}

__device__ __forceinline__ void polzn_chunk(const PolznArgs &a, int chunk, int &c0, int &c1)
{
    c0 = (int)(((int64_t)chunk * a.n_cells) / a.nch);
    c1 = (int)(((int64_t)(chunk + 1) * a.n_cells) / a.nch);
}

// blockIdx.x = (chunk * ntiles + tile) * G + group; four lane-waves per workgroup share the tile and the chunk
template <int JT, int KT>
__global__ void __launch_bounds__(256) cf_polzn_cells3(const PolznArgs a)
{
    const int G = (a.nlw + 3) / 4, ntiles = a.ntj * a.ntk;
    const int grp = blockIdx.x % G, tile = (blockIdx.x / G) % ntiles, chunk = blockIdx.x / (G * ntiles);
    const int lw = grp * 4 + (threadIdx.x >> 6);
    if (lw >= a.nlw) return;   // no barrier below
    const int l = lw * 64 + (threadIdx.x & 63);
    const PolznLane q = polzn_lane(a, l);
    const int tj = tile % a.ntj, tk = tile / a.ntj;
    double cp[JT], sp[JT], ey[KT], emy[KT];
#pragma unroll
    for (int jj = 0; jj < JT; jj++) { cp[jj] = a.cphi[tj * JT + jj]; sp[jj] = a.sphi[tj * JT + jj]; }
#pragma unroll
    for (int kk = 0; kk < KT; kk++) { ey[kk] = a.ka[tk * KT + kk]; emy[kk] = a.kb[tk * KT + kk]; }
    double acc[KT][JT][5];
#pragma unroll
    for (int kk = 0; kk < KT; kk++)
#pragma unroll
        for (int jj = 0; jj < JT; jj++)
#pragma unroll
            for (int m = 0; m < 5; m++) acc[kk][jj][m] = 0.0;
    int c0, c1;
    polzn_chunk(a, chunk, c0, c1);
    for (int c = c0; c < c1; c++) {
        const double tau = a.tau[c], ux = a.ux[c], uy = a.uy[c], un = a.un[c];
        const double dat = a.dat[c], dax = a.dax[c], day = a.day[c], dan = a.dan[c];
        const double wtx = a.wtx[c], wty = a.wty[c], wtn = a.wtn[c], wxy = a.wxy[c], wxn = a.wxn[c], wyn = a.wyn[c];
        const double eta = a.eta[c];
        const double ut = sqrt(fabs(1.0 + ux * ux + uy * uy + tau * tau * un * un));
        const double uperp = sqrt(ux * ux + uy * uy), itau = 1.0 / tau;
        const double eeta = exp(eta), emeta = exp(-eta);
        const double pTu = q.pTi * uperp;
        double E1[KT], MP[KT], MA[KT][4];
#pragma unroll
        for (int kk = 0; kk < KT; kk++) {
            // e^(y - eta) and e^(eta - y) as products: no cancellation in cosh, none beyond one ulp of cosh in sinh
            const double ep = ey[kk] * emeta, em = emy[kk] * eeta;
            polzn_y_side(q, 0.5 * (ep + em), 0.5 * (ep - em), tau, itau, ut, un, pTu, dat, dan, wtx, wty, wxy, wxn, wyn, E1[kk], MP[kk], MA[kk]);
        }
#pragma unroll
        for (int jj = 0; jj < JT; jj++) {
            double E2, PQ, PB[4];
            polzn_phi_side(q, cp[jj], sp[jj], ux, uy, uperp, dax, day, wtx, wty, wtn, wxn, wyn, E2, PQ, PB);
#pragma unroll
            for (int kk = 0; kk < KT; kk++) polzn_eval(E1[kk], E1[kk], MP[kk], MA[kk], E2, PQ, PB, q.sign, acc[kk][jj]);
        }
    }
    const int64_t Lp = (int64_t)a.nlw * 64;
#pragma unroll
    for (int kk = 0; kk < KT; kk++)
#pragma unroll
        for (int jj = 0; jj < JT; jj++) {
            const int j = tj * JT + jj, k = tk * KT + kk;
            if (j >= a.J || k >= a.K) continue;
            const int64_t bin = j + (int64_t)a.J * k;
#pragma unroll
            for (int m = 0; m < 5; m++) a.slab[(((int64_t)chunk * 5 + m) * a.NB + bin) * Lp + l] = acc[kk][jj][m];
        }
}

// 2+1D: y = 0, every eta node of the table summed inside the bin (tile: JT phi nodes; ntk = 1)
template <int JT>
__global__ void __launch_bounds__(256) cf_polzn_cells2(const PolznArgs a)
{
    const int G = (a.nlw + 3) / 4, ntiles = a.ntj;
    const int grp = blockIdx.x % G, tj = (blockIdx.x / G) % ntiles, chunk = blockIdx.x / (G * ntiles);
    const int lw = grp * 4 + (threadIdx.x >> 6);
    if (lw >= a.nlw) return;
    const int l = lw * 64 + (threadIdx.x & 63);
    const PolznLane q = polzn_lane(a, l);
    double cp[JT], sp[JT];
#pragma unroll
    for (int jj = 0; jj < JT; jj++) { cp[jj] = a.cphi[tj * JT + jj]; sp[jj] = a.sphi[tj * JT + jj]; }
    double acc[JT][5];
#pragma unroll
    for (int jj = 0; jj < JT; jj++)
#pragma unroll
        for (int m = 0; m < 5; m++) acc[jj][m] = 0.0;
    int c0, c1;
    polzn_chunk(a, chunk, c0, c1);
    for (int c = c0; c < c1; c++) {
        const double tau = a.tau[c], ux = a.ux[c], uy = a.uy[c], un = a.un[c];
        const double dat = a.dat[c], dax = a.dax[c], day = a.day[c], dan = a.dan[c];
        const double wtx = a.wtx[c], wty = a.wty[c], wtn = a.wtn[c], wxy = a.wxy[c], wxn = a.wxn[c], wyn = a.wyn[c];
        const double ut = sqrt(fabs(1.0 + ux * ux + uy * uy + tau * tau * un * un));
        const double uperp = sqrt(ux * ux + uy * uy), itau = 1.0 / tau;
        const double pTu = q.pTi * uperp;
        double E2[JT], PQ[JT], PB[JT][4];
#pragma unroll
        for (int jj = 0; jj < JT; jj++) polzn_phi_side(q, cp[jj], sp[jj], ux, uy, uperp, dax, day, wtx, wty, wtn, wxn, wyn, E2[jj], PQ[jj], PB[jj]);
        for (int k = 0; k < a.K; k++) {
            double E1, MP, MA[4];
            polzn_y_side(q, a.ka[k], a.kb[k], tau, itau, ut, un, pTu, dat, dan, wtx, wty, wxy, wxn, wyn, E1, MP, MA);
            const double E1w = E1 * a.kw[k];
#pragma unroll
            for (int jj = 0; jj < JT; jj++) polzn_eval(E1, E1w, MP, MA, E2[jj], PQ[jj], PB[jj], q.sign, acc[jj]);
        }
    }
    const int64_t Lp = (int64_t)a.nlw * 64;
#pragma unroll
    for (int jj = 0; jj < JT; jj++) {
        const int j = tj * JT + jj;
        if (j >= a.J) continue;
#pragma unroll
        for (int m = 0; m < 5; m++) a.slab[(((int64_t)chunk * 5 + m) * a.NB + j) * Lp + l] = acc[jj][m];
    }
}

hipError_t launch_polzn_cells(const PolznArgs &a, int three_d, hipStream_t st)
{
    if (a.n_cells <= 0) return hipSuccess;
    const int G = (a.nlw + 3) / 4;
    const int64_t nblk = (int64_t)G * a.ntj * a.ntk * a.nch;
    if (three_d) hipLaunchKernelGGL((cf_polzn_cells3<kPolznJT3, kPolznKT3>), dim3((unsigned)nblk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((cf_polzn_cells2<kPolznJT2>), dim3((unsigned)nblk), dim3(256), 0, st, a);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256)
cf_polzn_reduce(const double *__restrict__ slab, int nch, int64_t NB, int64_t Lp, const int32_t *__restrict__ cls, const double *__restrict__ scale,
                int S, int npT, int npTp, double *__restrict__ St, double *__restrict__ Sx, double *__restrict__ Sy, double *__restrict__ Sn,
                double *__restrict__ Snorm)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)S * npT * NB) return;
    const int s = (int)(i % S);
    const int64_t r = i / S;
    const int ipT = (int)(r % npT);
    const int64_t bin = r / npT;
    const int64_t l = (int64_t)cls[s] * npTp + ipT;
    double *outs[5] = {St, Sx, Sy, Sn, Snorm};
#pragma unroll
    for (int m = 0; m < 5; m++) {
        double v = 0.0;
        for (int ch = 0; ch < nch; ch++) v += slab[((int64_t)ch * 5 + m) * NB * Lp + bin * Lp + l];
        outs[m][i] = m < 4 ? scale[s] * v : v;
    }
}

hipError_t launch_polzn_reduce(const double *slab, int nch, int64_t NB, int64_t Lp, const int32_t *cls, const double *scale, int S, int npT,
                               int npTp, double *St, double *Sx, double *Sy, double *Sn, double *Snorm, hipStream_t st)
{
    const int64_t n = (int64_t)S * npT * NB;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_polzn_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slab, nch, NB, Lp, cls, scale, S, npT, npTp, St, Sx,
                       Sy, Sn, Snorm);
    return hipGetLastError();
}

// ---- several devices: a shard's class-lane sums, and their sum over the shards (is3d_spin_polarization_multi) ----
// one thread per pair of class-lane elements (per = 5 NB Lp is even: Lp is a multiple of 64); the additions of cf_polzn_reduce, from the same 0.0
__global__ void __launch_bounds__(256) cf_polzn_class_sums(const double *__restrict__ slab, int nch, int64_t per, double *__restrict__ V)
{
    const int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= per) return;
    double2 v = {0.0, 0.0};
    for (int ch = 0; ch < nch; ch++) {
        const double2 a = *(const double2 *)(slab + (int64_t)ch * per + i);
        v.x += a.x;
        v.y += a.y;
    }
    *(double2 *)(V + i) = v;
}

hipError_t launch_polzn_class_sums(const double *slab, int nch, int64_t per, double *V, hipStream_t st)
{
    if (per <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_polzn_class_sums, dim3((unsigned)((per / 2 + 255) / 256)), dim3(256), 0, st, slab, nch, per, V);
    return hipGetLastError();
}

// one thread per output element (species, pT, bin), indexed as cf_polzn_reduce; the shards' sums added left to right in shard order
__global__ void __launch_bounds__(256)
cf_polzn_shards(const double *__restrict__ stage, int n_sh, int64_t NB, int64_t Lp, const int32_t *__restrict__ cls, const double *__restrict__ scale,
                int S, int npT, int npTp, double *__restrict__ St, double *__restrict__ Sx, double *__restrict__ Sy, double *__restrict__ Sn,
                double *__restrict__ Snorm)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)S * npT * NB) return;
    const int s = (int)(i % S);
    const int64_t r = i / S;
    const int ipT = (int)(r % npT);
    const int64_t bin = r / npT;
    const int64_t l = (int64_t)cls[s] * npTp + ipT, per = 5 * NB * Lp;
    double *outs[5] = {St, Sx, Sy, Sn, Snorm};
#pragma unroll
    for (int m = 0; m < 5; m++) {
        const double *p = stage + ((int64_t)m * NB + bin) * Lp + l;
        double v = n_sh > 0 ? p[0] : 0.0;
        for (int k = 1; k < n_sh; k++) v = v + p[(int64_t)k * per];
        outs[m][i] = m < 4 ? scale[s] * v : v;
    }
}

hipError_t launch_polzn_shards(const double *stage, int n_sh, int64_t NB, int64_t Lp, const int32_t *cls, const double *scale, int S, int npT,
                               int npTp, double *St, double *Sx, double *Sy, double *Sn, double *Snorm, hipStream_t st)
{
    const int64_t n = (int64_t)S * npT * NB;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_polzn_shards, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, stage, n_sh, NB, Lp, cls, scale, S, npT, npTp, St, Sx,
                       Sy, Sn, Snorm);
    return hipGetLastError();
}

}  // namespace is3d

// =================================================================================================
// C ABI
// =================================================================================================
using namespace is3d;

struct is3d_polarization_plan {
    int device = 0, dim3 = 1, S = 0, npT = 0, J = 0, K = 0, ncls = 0, npTp = 1, nlw = 0, ntj = 0, ntk = 1;
    int64_t NB = 0, max_cells = 0, ws_cap = 0;
    DevBuf<double> lane_mT, lane_pT, lane_sign, cphi, sphi, ka, kb, kw, scale, slab;
    DevBuf<int32_t> cls;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~is3d_polarization_plan()
    {
        (void)hipSetDevice(device);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

int check_grid_species(const is3d_species *sp, const is3d_grid *g, int dim3)
{
    if (!sp || !g) return set_error(IS3D_EINVAL, "species and grid are required");
    if (sp->n < 1 || !sp->mass || !sp->sign) return set_error(IS3D_EINVAL, "spin polarization needs at least one species with mass and sign");
    for (int s = 0; s < sp->n; s++)
        if (!(sp->mass[s] > 0.0)) return set_error(IS3D_EINVAL, "species %d has mass %g: the spin polarization divides by the mass", s, sp->mass[s]);
    if (g->n_pT < 1 || g->n_phi < 1 || !g->pT || !g->phi) return set_error(IS3D_EINVAL, "the pT and phi grids need at least one node");
    if (dim3 && (g->n_y < 1 || !g->y)) return set_error(IS3D_EINVAL, "3+1D needs the y grid");
    if (!dim3 && (g->n_eta < 2 || !g->eta || !g->eta_w))
        return set_error(IS3D_EINVAL, "2+1D needs at least 2 eta nodes with weights (the reference's delta_eta = eta[1] - eta[0]), %d given", g->n_eta);
    if (g->n_pT > 64) return set_error(IS3D_EINVAL, "spin polarization: at most 64 pT nodes (%d given)", g->n_pT);
    return IS3D_OK;
}

int check_inputs(const is3d_cells *c, const is3d_vorticity *w, double T, int dim3)
{
    if (!c) return set_error(IS3D_EINVAL, "cells are required");
    if (!w || !w->wtx || !w->wty || !w->wtn || !w->wxy || !w->wxn || !w->wyn)
        return set_error(IS3D_EINVAL, "spin polarization needs the six thermal-vorticity arrays (a NULL vorticity pointer was given)");
    if (!(T > 0.0) || !std::isfinite(T)) return set_error(IS3D_EINVAL, "spin polarization needs a finite temperature T > 0 (%g given)", T);
    if (c->n_cells < 0) return set_error(IS3D_EINVAL, "n_cells < 0");
    if (c->n_cells > 0 && (!c->tau || !c->ux || !c->uy || !c->un || !c->dat || !c->dax || !c->day || !c->dan || (dim3 && !c->eta)))
        return set_error(IS3D_EINVAL, "a cell array the spin polarization reads is NULL (tau, ux, uy, un, dat, dax, day, dan%s)", dim3 ? ", eta" : "");
    if (c->n_cells > INT32_MAX) return set_error(IS3D_EINVAL, "at most 2^31 - 1 cells per execute");
    return IS3D_OK;
}

int dim_of(const is3d_options *o, int *dim3)
{
    const int d = o ? o->dimension : 3;
    if (d != 2 && d != 3) return set_error(IS3D_EINVAL, "dimension = %d: 2 or 3", d);
    *dim3 = d == 3;
    return IS3D_OK;
}

// chunks of the cell axis: about 8192 waves in all, at least 256 cells per chunk, and the partial slabs within the workspace cap.  A function
// of the shape only, so that the one-shot and the plan (and every run) sum in the same order.
int polzn_chunks(const is3d_polarization_plan *P, int64_t n)
{
    const int64_t waves = (int64_t)P->nlw * P->ntj * P->ntk;
    int64_t nch = std::max<int64_t>(1, (8192 + waves - 1) / waves);
    nch = std::min<int64_t>(nch, std::max<int64_t>(1, n / 256));
    const int64_t per = 5 * P->NB * (int64_t)P->nlw * 64 * (int64_t)sizeof(double);
    nch = std::min<int64_t>(nch, std::max<int64_t>(1, P->ws_cap / per));
    return (int)std::min<int64_t>(nch, 64);
}

}  // namespace

extern "C" int is3d_polarization_plan_create(is3d_polarization_plan **plan, const is3d_species *species, const is3d_grid *grid,
                                             const is3d_options *opts, int64_t max_cells)
{
    if (!plan) return set_error(IS3D_EINVAL, "plan is NULL");
    *plan = nullptr;
    int dim3;
    if (int rc = dim_of(opts, &dim3)) return rc;
    if (int rc = check_grid_species(species, grid, dim3)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    if (opts && opts->device >= 0) HIP_TRY(hipSetDevice(opts->device));
    std::unique_ptr<is3d_polarization_plan> P(new is3d_polarization_plan);
    count_resource(0);
    HIP_TRY(hipGetDevice(&P->device));
    P->dim3 = dim3;
    P->S = species->n;
    P->npT = grid->n_pT;
    P->J = grid->n_phi;
    P->K = dim3 ? grid->n_y : grid->n_eta;
    P->NB = (int64_t)P->J * (dim3 ? P->K : 1);
    P->max_cells = max_cells;
    P->ws_cap = (opts && opts->workspace_bytes > 0) ? opts->workspace_bytes : ((int64_t)16 << 30);
    // classes: one per distinct (mass, sign), in order of first appearance
    const SpeciesClasses kc = species_classes(species->mass, species->sign, nullptr, P->S, true);
    const std::vector<int32_t> &cls = kc.cls;
    const std::vector<double> &cmass = kc.cmass, &csign = kc.csign;
    std::vector<double> scale((size_t)P->S);
    for (int s = 0; s < P->S; s++) scale[(size_t)s] = -1.0 / (4.0 * species->mass[s]);   // 2 x -(1 / (8 m))
    P->ncls = (int)cmass.size();
    while (P->npTp < P->npT) P->npTp *= 2;
    P->nlw = (int)(((int64_t)P->ncls * P->npTp + 63) / 64);
    const size_t L = (size_t)P->nlw * 64;
    std::vector<double> mT(L, 1.0), pT(L, 0.0), sg(L, 0.0);   // padding lanes: a harmless massive particle at rest
    for (int c = 0; c < P->ncls; c++)
        for (int i = 0; i < P->npT; i++) {
            const size_t l = (size_t)c * P->npTp + i;
            pT[l] = grid->pT[i];
            mT[l] = std::sqrt(cmass[(size_t)c] * cmass[(size_t)c] + grid->pT[i] * grid->pT[i]);
            sg[l] = csign[(size_t)c];
        }
    const int JT = dim3 ? kPolznJT3 : kPolznJT2, KT = dim3 ? kPolznKT3 : 1;
    P->ntj = (P->J + JT - 1) / JT;
    P->ntk = dim3 ? (P->K + KT - 1) / KT : 1;
    std::vector<double> cp((size_t)P->ntj * JT), sp((size_t)P->ntj * JT);
    for (size_t j = 0; j < cp.size(); j++) {
        const int jc = std::min<int>((int)j, P->J - 1);
        cp[j] = std::cos(grid->phi[jc]);
        sp[j] = std::sin(grid->phi[jc]);
    }
    std::vector<double> ka, kb, kw;
    if (dim3) {
        for (int k = 0; k < P->ntk * KT; k++) {
            const double y = grid->y[std::min(k, P->K - 1)];
            ka.push_back(std::exp(y));
            kb.push_back(std::exp(-y));
        }
        kw.assign(1, 1.0);
    } else {
        const double deta = grid->eta[1] - grid->eta[0];   // the reference assumes a uniform grid (polzn_kernels.cpp:60)
        for (int k = 0; k < P->K; k++) {
            ka.push_back(std::cosh(grid->eta[k]));         // y = 0: cosh(y - eta), sinh(y - eta)
            kb.push_back(-std::sinh(grid->eta[k]));
            kw.push_back(grid->eta_w[k] * deta);
        }
    }
    HIP_TRY(P->lane_mT.upload(mT));
    HIP_TRY(P->lane_pT.upload(pT));
    HIP_TRY(P->lane_sign.upload(sg));
    HIP_TRY(P->cphi.upload(cp));
    HIP_TRY(P->sphi.upload(sp));
    HIP_TRY(P->ka.upload(ka));
    HIP_TRY(P->kb.upload(kb));
    HIP_TRY(P->kw.upload(kw));
    HIP_TRY(P->scale.upload(scale));
    HIP_TRY(P->cls.upload(cls));
    for (hipEvent_t &e : P->ev) HIP_TRY(hipEventCreate(&e));
    *plan = P.release();
    return IS3D_OK;
}

extern "C" int is3d_polarization_plan_execute(is3d_polarization_plan *P, const is3d_cells *cells, const is3d_vorticity *w, double T,
                                              const is3d_polarization_out *out, void *hip_stream, is3d_polarization_stats *stats)
{
    if (!P) return set_error(IS3D_EINVAL, "plan is NULL");
    if (int rc = check_inputs(cells, w, T, P->dim3)) return rc;
    if (!out || !out->St || !out->Sx || !out->Sy || !out->Sn || !out->Snorm) return set_error(IS3D_EINVAL, "the five output arrays are required");
    if (P->max_cells > 0 && cells->n_cells > P->max_cells)
        return set_error(IS3D_EINVAL, "%lld cells > the plan's max_cells %lld", (long long)cells->n_cells, (long long)P->max_cells);
    HIP_TRY(hipSetDevice(P->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const int64_t n = cells->n_cells;
    const int nch = polzn_chunks(P, n);
    const int64_t Lp = (int64_t)P->nlw * 64;
    const size_t need = (size_t)nch * 5 * (size_t)P->NB * (size_t)Lp;
    if (n > 0 && P->slab.n < need) {
        hipError_t e = P->slab.alloc(need);
        if (e != hipSuccess) {
            P->slab.release();
            return set_error(IS3D_ENOMEM, "out of device memory for the polarization partial sums (%.2f GB: %d chunks x 5 x %lld bins x %lld lanes)",
                             need * 8.0 / 1e9, nch, (long long)P->NB, (long long)Lp);
        }
    }
    const bool timed = stats != nullptr;
    if (timed) HIP_TRY(hipEventRecord(P->ev[0], st));
    const int64_t nout = (int64_t)P->S * P->npT * P->NB;
    if (n > 0) {
        PolznArgs a{};
        a.tau = cells->tau; a.eta = cells->eta; a.ux = cells->ux; a.uy = cells->uy; a.un = cells->un;
        a.dat = cells->dat; a.dax = cells->dax; a.day = cells->day; a.dan = cells->dan;
        a.wtx = w->wtx; a.wty = w->wty; a.wtn = w->wtn; a.wxy = w->wxy; a.wxn = w->wxn; a.wyn = w->wyn;
        a.n_cells = (int32_t)n; a.nch = nch; a.nlw = P->nlw; a.ntj = P->ntj; a.ntk = P->ntk; a.J = P->J; a.K = P->K;
        a.invT = 1.0 / T;
        a.lane_mT = P->lane_mT.p; a.lane_pT = P->lane_pT.p; a.lane_sign = P->lane_sign.p;
        a.cphi = P->cphi.p; a.sphi = P->sphi.p; a.ka = P->ka.p; a.kb = P->kb.p; a.kw = P->kw.p;
        a.slab = P->slab.p; a.NB = P->NB;
        HIP_TRY(launch_polzn_cells(a, P->dim3, st));
        if (timed) HIP_TRY(hipEventRecord(P->ev[1], st));
        HIP_TRY(launch_polzn_reduce(P->slab.p, nch, P->NB, Lp, P->cls.p, P->scale.p, P->S, P->npT, P->npTp, out->St, out->Sx, out->Sy, out->Sn,
                                    out->Snorm, st));
    } else {
        if (timed) HIP_TRY(hipEventRecord(P->ev[1], st));
        double *o[5] = {out->St, out->Sx, out->Sy, out->Sn, out->Snorm};
        for (double *p : o) HIP_TRY(hipMemsetAsync(p, 0, sizeof(double) * (size_t)nout, st));
    }
    if (timed) {
        HIP_TRY(hipEventRecord(P->ev[2], st));
        HIP_TRY(hipEventSynchronize(P->ev[2]));
        float a = 0.f, b = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, P->ev[0], P->ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, P->ev[1], P->ev[2]));
        stats->code = IS3D_OK;
        stats->n_classes = P->ncls;
        stats->n_chunks = n > 0 ? nch : 0;
        stats->ms_cells = a;
        stats->ms_reduce = b;
    }
    return IS3D_OK;
}

extern "C" void is3d_polarization_plan_destroy(is3d_polarization_plan *P) { delete P; }

extern "C" int is3d_spin_polarization(const is3d_cells *cells, const is3d_vorticity *w, const is3d_species *species, const is3d_grid *grid,
                                      double T, const is3d_options *opts, is3d_polarization_out *out, is3d_polarization_stats *stats)
{
    int dim3;
    if (int rc = dim_of(opts, &dim3)) return rc;
    if (int rc = check_grid_species(species, grid, dim3)) return rc;
    if (int rc = check_inputs(cells, w, T, dim3)) return rc;
    if (!out || !out->St || !out->Sx || !out->Sy || !out->Sn || !out->Snorm) return set_error(IS3D_EINVAL, "the five output arrays are required");
    is3d_polarization_plan *raw = nullptr;
    if (int rc = is3d_polarization_plan_create(&raw, species, grid, opts, std::max<int64_t>(cells->n_cells, 1))) return rc;
    std::unique_ptr<is3d_polarization_plan> P(raw);
    const int64_t n = cells->n_cells;
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<double> blk;
    HIP_TRY(blk.alloc((size_t)std::max<int64_t>(n, 1) * 15));
    is3d_cells dc{};
    HIP_TRY(stage_cells(*cells, [dim3](int i) { return i <= 8 && (i != 1 || dim3); }, 0, n, blk.p, nullptr, &dc));
    std::array<const double *, 6> wa{w->wtx, w->wty, w->wtn, w->wxy, w->wxn, w->wyn};
    HIP_TRY(stage_arrays(wa, 0, n, blk.p + 9 * (size_t)std::max<int64_t>(n, 1), nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    const auto t1 = std::chrono::steady_clock::now();
    is3d_vorticity dw{wa[0], wa[1], wa[2], wa[3], wa[4], wa[5]};
    const size_t nout = (size_t)P->S * P->npT * (size_t)P->NB;
    DevBuf<double> o;
    HIP_TRY(o.alloc(nout * 5));
    is3d_polarization_out dout{o.p, o.p + nout, o.p + 2 * nout, o.p + 3 * nout, o.p + 4 * nout};
    is3d_polarization_stats ps{};
    // n == 0: no cell arrays were staged; the execute writes zeros without reading them
    if (n == 0) dw = is3d_vorticity{o.p, o.p, o.p, o.p, o.p, o.p};
    if (int rc = is3d_polarization_plan_execute(P.get(), n ? &dc : cells, &dw, T, &dout, nullptr, &ps)) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    double *ho[5] = {out->St, out->Sx, out->Sy, out->Sn, out->Snorm};
    for (int m = 0; m < 5; m++) HIP_TRY(hipMemcpy(ho[m], o.p + m * nout, sizeof(double) * nout, hipMemcpyDeviceToHost));
    const auto t3 = std::chrono::steady_clock::now();
    if (stats) {
        *stats = ps;
        stats->ms_h2d = std::chrono::duration<double, std::milli>(t1 - t0).count();
        stats->ms_d2h = std::chrono::duration<double, std::milli>(t3 - t2).count();
    }
    return IS3D_OK;
}

// =================================================================================================
// what is3d_spin_polarization_multi (cf_multi.hip) takes from a plan: the checks, a shard's class-lane sums, the sum over the shards
// =================================================================================================
namespace is3d {

int polzn_check_args(const is3d_cells *cells, const is3d_vorticity *w, const is3d_species *species, const is3d_grid *grid, double T,
                     const is3d_options *opts, const is3d_polarization_out *out)
{
    int dim3;
    if (int rc = dim_of(opts, &dim3)) return rc;
    if (int rc = check_grid_species(species, grid, dim3)) return rc;
    if (int rc = check_inputs(cells, w, T, dim3)) return rc;
    if (!out || !out->St || !out->Sx || !out->Sy || !out->Sn || !out->Snorm) return set_error(IS3D_EINVAL, "the five output arrays are required");
    return IS3D_OK;
}

int polzn_plan_classes(const is3d_polarization_plan *P) { return P->ncls; }
int64_t polzn_plan_output_size(const is3d_polarization_plan *P) { return (int64_t)P->S * P->npT * P->NB; }
int64_t polzn_plan_class_sum_size(const is3d_polarization_plan *P) { return 5 * P->NB * (int64_t)P->nlw * 64; }

int polzn_plan_class_sums(is3d_polarization_plan *P, const is3d_cells *cells, const is3d_vorticity *w, double T, double *V, hipStream_t st,
                          is3d_polarization_stats *stats)
{
    if (!P || !V || !stats) return set_error(IS3D_EINVAL, "plan, class sums or stats is NULL");
    if (int rc = check_inputs(cells, w, T, P->dim3)) return rc;
    const int64_t n = cells->n_cells;
    if (n < 1) return set_error(IS3D_EINVAL, "a shard without cells has no class sums");
    if (P->max_cells > 0 && n > P->max_cells)
        return set_error(IS3D_EINVAL, "%lld cells > the plan's max_cells %lld", (long long)n, (long long)P->max_cells);
    HIP_TRY(hipSetDevice(P->device));
    const int nch = polzn_chunks(P, n);
    const int64_t Lp = (int64_t)P->nlw * 64, per = 5 * P->NB * Lp;
    const size_t need = (size_t)nch * (size_t)per;
    if (P->slab.n < need) {
        hipError_t e = P->slab.alloc(need);
        if (e != hipSuccess) {
            P->slab.release();
            return set_error(IS3D_ENOMEM, "out of device memory for the polarization partial sums (%.2f GB: %d chunks x 5 x %lld bins x %lld lanes)",
                             need * 8.0 / 1e9, nch, (long long)P->NB, (long long)Lp);
        }
    }
    PolznArgs a{};
    a.tau = cells->tau; a.eta = cells->eta; a.ux = cells->ux; a.uy = cells->uy; a.un = cells->un;
    a.dat = cells->dat; a.dax = cells->dax; a.day = cells->day; a.dan = cells->dan;
    a.wtx = w->wtx; a.wty = w->wty; a.wtn = w->wtn; a.wxy = w->wxy; a.wxn = w->wxn; a.wyn = w->wyn;
    a.n_cells = (int32_t)n; a.nch = nch; a.nlw = P->nlw; a.ntj = P->ntj; a.ntk = P->ntk; a.J = P->J; a.K = P->K;
    a.invT = 1.0 / T;
    a.lane_mT = P->lane_mT.p; a.lane_pT = P->lane_pT.p; a.lane_sign = P->lane_sign.p;
    a.cphi = P->cphi.p; a.sphi = P->sphi.p; a.ka = P->ka.p; a.kb = P->kb.p; a.kw = P->kw.p;
    a.slab = P->slab.p; a.NB = P->NB;
    HIP_TRY(hipEventRecord(P->ev[0], st));
    HIP_TRY(launch_polzn_cells(a, P->dim3, st));
    HIP_TRY(hipEventRecord(P->ev[1], st));
    HIP_TRY(launch_polzn_class_sums(P->slab.p, nch, per, V, st));
    HIP_TRY(hipEventRecord(P->ev[2], st));
    HIP_TRY(hipEventSynchronize(P->ev[2]));
    float t_cells = 0.f, t_sums = 0.f;
    HIP_TRY(hipEventElapsedTime(&t_cells, P->ev[0], P->ev[1]));
    HIP_TRY(hipEventElapsedTime(&t_sums, P->ev[1], P->ev[2]));
    stats->code = IS3D_OK;
    stats->n_classes = P->ncls;
    stats->n_chunks = nch;
    stats->ms_cells = t_cells;
    stats->ms_reduce = t_sums;
    return IS3D_OK;
}

int polzn_plan_combine(is3d_polarization_plan *P, const double *stage, int n_sh, const is3d_polarization_out *out, hipStream_t st)
{
    if (!P || !out || n_sh < 0 || (n_sh > 0 && !stage)) return set_error(IS3D_EINVAL, "plan, staging array or outputs missing");
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(launch_polzn_shards(stage, n_sh, P->NB, (int64_t)P->nlw * 64, P->cls.p, P->scale.p, P->S, P->npT, P->npTp, out->St, out->Sx, out->Sy,
                                out->Sn, out->Snorm, st));
    return IS3D_OK;
}

}  // namespace is3d
