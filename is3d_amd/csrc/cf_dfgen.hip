// cf_dfgen.hip -- is3d_df_generate: the ten df-coefficient tables of deltaf_coefficients/vh/<list>/ for any hadron list and (T, mu_B) grid.
//
// Restates the reference's offline generator, generate_delta_f_coefficients/*/df_vh_dimensionless/src/deltaf_table.cpp:137-248 (14-moment
// c0..c4) and :296-395 (Chapman-Enskog F, G, betabulk, betaV, betapi), with the integrands of thermal_integrands.cpp: 20 Gauss-Laguerre
// thermal integrals summed over the massive entries of the list at every grid point.
//
// cf_dfgen_points: one workgroup of 4 waves per grid point; lane <-> quadrature node, wave <-> a contiguous range of list entries.
// With x = exp(Ebar - b alpha_B), q = x + sign, r = 1 / q and the node-only constant ew = w e^pbar, every integrand of a node set is
// a product of powers of pbar and Ebar with one of two kernels
//     nk = ew r              (n_eq, e, p:              w e^pbar / q)
//     K  = nk (x r)          (every J, N, M integral:  w e^(pbar + Ebar - b alpha_B) / q^2)
// so one exponential, one square root and two reciprocals serve all integrals of a node set (exp_full / sqrt_nr / rcp_nr of cf_math.h).
//
// SUM ORDER (fixed by n_gla and the list length n alone, so a point's 30 numbers do not depend on the grid it is computed in):
//   1. lane l of wave w accumulates, for node chunks c = 0, 1, .. (node c * 64 + l < n_gla) in ascending order and inside a chunk for
//      the entries k = floor(n w / 4) .. floor(n (w + 1) / 4) - 1 in ascending order (massless entries skipped), the terms
//      gspin_k [mass_k^2] [b_k | b_k^2] * integrand into 20 accumulators, one plain addition per term;
//   2. the 64 lanes of a wave are summed by a butterfly: v += shfl_xor(v, 32), then 16, 8, 4, 2, 1;
//   3. the four wave sums are added as ((w0 + w1) + w2) + w3, and the result is multiplied by T^k / (2 pi^2 hbarc^3) [/3, /15].
// No floating-point atomics anywhere.  The combinations of the 20 integrals into the ten outputs are evaluated by one thread with IEEE
// division, in the order the reference writes them.
#include <hip/hip_runtime.h>

#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_device.h"
#include "cf_dfgen.h"
#include "cf_host.h"
#include "cf_math.h"
#include "errors.h"

namespace is3d {

// the per-node kernels of one node set for one list entry; returns false where qstat <= 0
struct DfgenNode {
    double Ebar, Ebar2, inv_Ebar, nk, K;
};
__device__ __forceinline__ bool dfgen_node(double pbar2, double ew, double mbar2, double chem, double sign, DfgenNode &o)
{
    o.Ebar2 = pbar2 + mbar2;
    o.Ebar = sqrt_nr(o.Ebar2);
    const double x = exp_full(o.Ebar - chem);
    const double q = x + sign;
    const double r = rcp_nr(q);
    o.inv_Ebar = rcp_nr(o.Ebar);
    // ew == 0 (a lane without a node): exact zeros whatever q is
    o.nk = (ew == 0.0) ? 0.0 : ew * r;
    o.K = (ew == 0.0) ? 0.0 : o.nk * (x * r);
    return q > 0.0;
}

__global__ void __launch_bounds__(kDfgenWaves * 64) cf_dfgen_points(DfgenParams p)
{
    __shared__ double part[kDfgenWaves][kDfgenIntegrals];
    __shared__ double total[kDfgenIntegrals];
    __shared__ int bad_k;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pt = blockIdx.x, iB = pt / p.n_T, iT = pt - iB * p.n_T;
    const double T = p.T[iT], muB = p.muB[iB];
    const double alphaB = muB / T;
    if (tid == 0) bad_k = INT_MAX;
    __syncthreads();
    const int k_lo = (int)(((long long)p.n * wave) / kDfgenWaves), k_hi = (int)(((long long)p.n * (wave + 1)) / kDfgenWaves);

    double J20 = 0.0, J21 = 0.0, J40 = 0.0, J41 = 0.0, N10 = 0.0, N30 = 0.0, N31 = 0.0, M20 = 0.0, M21 = 0.0, A20 = 0.0, A21 = 0.0, B10 = 0.0;
    double nB = 0.0, e = 0.0, pr = 0.0, J30 = 0.0, J32 = 0.0, N20 = 0.0, M10 = 0.0, M11 = 0.0;
    int my_bad = INT_MAX;
    for (int c0 = 0; c0 < p.n_gla; c0 += 64) {
        const int node = c0 + lane;
        const bool valid = node < p.n_gla;
        // node constants of the four sets; a lane without a node carries ew = 0 at pbar = 1: all its terms are exact zeros
        double pb[4], pb2[4], ipb[4], ew[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            pb[s] = valid ? p.root[s][node] : 1.0;
            const double w = valid ? p.weight[s][node] : 0.0;
            pb2[s] = pb[s] * pb[s];
            ipb[s] = rcp_nr(pb[s]);
            ew[s] = w * exp_full(pb[s]);
        }
        for (int k = k_lo; k < k_hi; k++) {
            const double mass = p.mass[k];
            if (mass == 0.0) continue;                                     // the photon, deltaf_table.cpp:176, :327
            const double g = p.gspin[k], b = p.baryon[k], sign = p.sign[k];
            const double mbar = mass / T, mbar2 = mbar * mbar, chem = b * alphaB;
            const double gm2 = g * (mass * mass);
            bool ok = true;
            DfgenNode n;
            // alpha = 2: J20, J21 (A20, A21, M20, M21, N20), e, p (:187-193, :336-339, :346)
            ok &= dfgen_node(pb2[1], ew[1], mbar2, chem, sign, n);
            {
                const double pe = pb2[1] * n.inv_Ebar;
                const double j20 = n.Ebar * n.K, j21 = pe * n.K;
                J20 += g * j20; J21 += g * j21;
                A20 += gm2 * j20; A21 += gm2 * j21;
                e += g * (n.Ebar * n.nk); pr += g * (pe * n.nk);
                if (b != 0.0) {
                    const double gb = g * b, gbb = gb * b;
                    M20 += gbb * j20; M21 += gbb * j21; N20 += gb * j20;
                }
            }
            // alpha = 3: J30, J32 (N30), J31 (N31) (:199-200, :340-341)
            ok &= dfgen_node(pb2[2], ew[2], mbar2, chem, sign, n);
            {
                const double j30 = (n.Ebar2 * ipb[2]) * n.K;
                const double j32 = ((pb2[2] * pb[2]) * (n.inv_Ebar * n.inv_Ebar)) * n.K;
                J30 += g * j30; J32 += g * j32;
                if (b != 0.0) {
                    const double gb = g * b;
                    N30 += gb * j30; N31 += gb * (pb[2] * n.K);
                }
            }
            // alpha = 4: J40, J41 (:192-193)
            ok &= dfgen_node(pb2[3], ew[3], mbar2, chem, sign, n);
            J40 += g * (((n.Ebar * n.Ebar2) * (ipb[3] * ipb[3])) * n.K);
            J41 += g * (n.Ebar * n.K);
            // alpha = 1, baryons only: J10 (N10, B10, M10), J11 (M11), n_eq (nB) (:196-198, :343-348)
            if (b != 0.0) {
                ok &= dfgen_node(pb2[0], ew[0], mbar2, chem, sign, n);
                const double gb = g * b, gbb = gb * b;
                const double j10 = pb[0] * n.K;
                const double j11 = ((pb2[0] * pb[0]) * (n.inv_Ebar * n.inv_Ebar)) * n.K;
                N10 += gb * j10; B10 += (gm2 * b) * j10; M10 += gbb * j10; M11 += gbb * j11;
                nB += gb * (pb[0] * n.nk);
            }
            if (valid && !ok && k < my_bad) my_bad = k;
        }
    }
    if (my_bad != INT_MAX) atomicMin(&bad_k, my_bad);                      // integer, LDS

    double acc[kDfgenIntegrals] = {J20, J21, J40, J41, N10, N30, N31, M20, M21, A20, A21, B10, nB, e, pr, J30, J32, N20, M10, M11};
#pragma unroll
    for (int i = 0; i < kDfgenIntegrals; i++) {
        double v = acc[i];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) part[wave][i] = v;
    }
    __syncthreads();
    if (tid < kDfgenIntegrals) {
        const double T2 = T * T, T3 = T2 * T, T4 = T2 * T2, T5 = T4 * T, T6 = T3 * T3;
        const double c = p.two_pi2_hbarc3;
        // T^k / (2 pi^2 hbarc^3), with the 1/3 and 1/15 of deltaf_table.cpp:145-156, :305-312; the order of kDfgenIntegrals
        const double fact[kDfgenIntegrals] = {T4 / c, T4 / (3.0 * c), T6 / c, T6 / (3.0 * c), T3 / c, T5 / c, T5 / (3.0 * c), T4 / c, T4 / (3.0 * c),
                                              T4 / c, T4 / (3.0 * c), T3 / c, T3 / c, T4 / c, T4 / (3.0 * c), T5 / c, T5 / (15.0 * c), T4 / c,
                                              T3 / c, T3 / (3.0 * c)};
        double s = part[0][tid];
        for (int w = 1; w < kDfgenWaves; w++) s += part[w][tid];
        double f = fact[0];
#pragma unroll
        for (int i = 1; i < kDfgenIntegrals; i++) f = (tid == i) ? fact[i] : f;
        total[tid] = s * f;
    }
    __syncthreads();
    if (tid != 0) return;
    const size_t npt = (size_t)p.n_T * p.n_muB;
    bool finite = true;
    for (int i = 0; i < kDfgenIntegrals; i++) {
        p.integrals[i * npt + pt] = total[i];
        finite = finite && isfinite(total[i]);
    }
    const double I_J20 = total[0], I_J21 = total[1], I_J40 = total[2], I_J41 = total[3], I_N10 = total[4], I_N30 = total[5], I_N31 = total[6];
    const double I_M20 = total[7], I_M21 = total[8], I_A20 = total[9], I_A21 = total[10], I_B10 = total[11], I_nB = total[12], I_e = total[13];
    const double I_p = total[14], I_J30 = total[15], I_J32 = total[16], I_N20 = total[17], I_M10 = total[18], I_M11 = total[19];
    (void)I_J20; (void)I_N10;
    const double T2 = T * T, T3 = T2 * T, T4 = T2 * T2, T5 = T4 * T;
    // 14 moment, deltaf_table.cpp:215-225
    const double bulk0 = (4.0 * I_N30 - I_B10) * I_N30 - I_M20 * (4.0 * I_J40 - I_A20);
    const double bulk1 = (I_B10 - I_N30) * (4.0 * I_J40 - I_A20) - (4.0 * I_N30 - I_B10) * (I_A20 - I_J40);
    const double bulk2 = I_M20 * (I_A20 - I_J40) - (I_B10 - I_N30) * I_N30;
    const double denom = (I_A21 - I_J41) * bulk0 + I_N31 * bulk1 + (4.0 * I_J41 - I_A21) * bulk2;
    const double ddiff = I_N31 * I_N31 - I_M21 * I_J41;
    double out[kDfgenTables];
    out[0] = (bulk0 / denom) * T4;
    out[1] = (bulk1 / denom) * T3;
    out[2] = (bulk2 / denom) * T4;
    out[3] = (I_J41 / ddiff) * T4;
    out[4] = (-I_N31 / ddiff) * T5;
    // Chapman-Enskog, :354-366
    const double ep = I_e + I_p, dce = I_J30 * I_M10 - I_N20 * I_N20;
    const double G = (ep * I_N20 - I_J30 * I_nB) / dce;
    const double F = T * T * (I_N20 * I_nB - ep * I_M10) / dce;
    const double betabulk = G * I_nB * T + F * ep / T + 5.0 * I_J32 / (3.0 * T);
    const double betaV = I_M11 - I_nB * I_nB * T / ep;
    const double betapi = I_J32 / T;
    out[5] = F / T; out[6] = G; out[7] = betabulk / T4; out[8] = betaV / T3; out[9] = betapi / T4;
    for (int i = 0; i < kDfgenTables; i++) {
        p.tables[i * npt + pt] = out[i];
        finite = finite && isfinite(out[i]);
    }
    unsigned cond = 0;
    if (bad_k != INT_MAX) cond |= kDfgenQstat;
    if (I_J21 * bulk0 - I_N31 * bulk1 + I_J41 * bulk2 == 0.0) cond |= kDfgenBulkDenom;   // the test the reference makes, :228
    if (ddiff == 0.0) cond |= kDfgenDiffDenom;                                           // :233
    if (betapi == 0.0) cond |= kDfgenBetapi;                                             // :370
    if (betabulk == 0.0) cond |= kDfgenBetabulk;                                         // :375
    if (betaV == 0.0) cond |= kDfgenBetaV;                                               // :380
    if (!finite) cond |= kDfgenNonFinite;
    if (cond) {
        p.bad_entry[pt] = (bad_k != INT_MAX) ? bad_k : -1;
        atomicMin(p.status, ((unsigned long long)pt << 8) | cond);                       // integer: the first failing point in grid order
    }
}

}  // namespace is3d

namespace {

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

bool all_finite(const double *a, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(a[i])) return false;
    return true;
}

}  // namespace

extern "C" int is3d_df_generate(const is3d_hadron_list *list, int32_t n_gla, const double *const root[4], const double *const weight[4],
                                int32_t n_T, const double *T, int32_t n_muB, const double *muB, int32_t device, double *tables,
                                double *integrals, is3d_dfgen_stats *stats)
{
    using is3d::set_error;
    if (!list || !root || !weight || !T || !muB || !tables) return set_error(IS3D_EINVAL, "null argument");
    const int32_t n = list->n;
    if (n <= 0) return set_error(IS3D_EINVAL, "the hadron list is empty (n = %d)", n);
    if (!list->mass || !list->gspin || !list->baryon || !list->sign) return set_error(IS3D_EINVAL, "a hadron list array is NULL");
    if (n_gla <= 0) return set_error(IS3D_EINVAL, "n_gla = %d: at least one Gauss-Laguerre node", n_gla);
    if (n_T <= 0 || n_muB <= 0) return set_error(IS3D_EINVAL, "n_T = %d, n_muB = %d: at least one of each", n_T, n_muB);
    if ((int64_t)n_T * n_muB > (int64_t)1 << 30) return set_error(IS3D_EINVAL, "n_T * n_muB = %lld grid points: at most 2^30", (long long)n_T * n_muB);
    if (device < -1) return set_error(IS3D_EINVAL, "device = %d: a HIP device ordinal, or -1 for the current device", device);
    for (int s = 0; s < 4; s++) {
        if (!root[s] || !weight[s]) return set_error(IS3D_EINVAL, "the Gauss-Laguerre roots or weights for alpha = %d are NULL", s + 1);
        if (!all_finite(root[s], n_gla) || !all_finite(weight[s], n_gla))
            return set_error(IS3D_EINVAL, "a Gauss-Laguerre root or weight for alpha = %d is not finite", s + 1);
        for (int k = 0; k < n_gla; k++)
            if (!(root[s][k] > 0.0)) return set_error(IS3D_EINVAL, "Gauss-Laguerre root %d for alpha = %d is %g: roots are positive", k, s + 1, root[s][k]);
    }
    if (!all_finite(list->mass, n) || !all_finite(list->gspin, n) || !all_finite(list->baryon, n) || !all_finite(list->sign, n))
        return set_error(IS3D_EINVAL, "a hadron list value is not finite");
    int32_t n_massive = 0;
    for (int k = 0; k < n; k++) {
        if (list->mass[k] < 0.0) return set_error(IS3D_EINVAL, "hadron list entry %d has mass %g", k, list->mass[k]);
        n_massive += list->mass[k] != 0.0;
    }
    for (int i = 0; i < n_T; i++)
        if (!std::isfinite(T[i]) || !(T[i] > 0.0)) return set_error(IS3D_EINVAL, "T[%d] = %g GeV: temperatures are positive and finite", i, T[i]);
    if (!all_finite(muB, n_muB)) return set_error(IS3D_EINVAL, "a baryon chemical potential is not finite");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    if (device >= ndev) return set_error(IS3D_EINVAL, "device = %d: %d HIP device(s) visible", device, ndev);
    if (device >= 0) HIP_TRY(hipSetDevice(device));

    const size_t npt = (size_t)n_T * n_muB;
    // one input block: mass, gspin, baryon, sign [n]; root, weight alpha = 1..4 [n_gla]; T [n_T]; muB [n_muB]
    std::vector<double> h_in;
    h_in.reserve((size_t)4 * n + (size_t)8 * n_gla + n_T + n_muB);
    h_in.insert(h_in.end(), list->mass, list->mass + n);
    h_in.insert(h_in.end(), list->gspin, list->gspin + n);
    h_in.insert(h_in.end(), list->baryon, list->baryon + n);
    h_in.insert(h_in.end(), list->sign, list->sign + n);
    for (int s = 0; s < 4; s++) h_in.insert(h_in.end(), root[s], root[s] + n_gla);
    for (int s = 0; s < 4; s++) h_in.insert(h_in.end(), weight[s], weight[s] + n_gla);
    h_in.insert(h_in.end(), T, T + n_T);
    h_in.insert(h_in.end(), muB, muB + n_muB);

    auto t0 = std::chrono::steady_clock::now();
    is3d::DevBuf<double> d_in, d_out;
    is3d::DevBuf<unsigned long long> d_status;
    is3d::DevBuf<int32_t> d_bad;
    HIP_TRY(d_in.upload(h_in));
    HIP_TRY(d_out.alloc((size_t)(is3d::kDfgenTables + is3d::kDfgenIntegrals) * npt));
    HIP_TRY(d_bad.alloc(npt));
    unsigned long long st = ~0ULL;
    HIP_TRY(d_status.upload(&st, 1));
    HIP_TRY(hipMemset(d_bad.p, 0xff, npt * sizeof(int32_t)));
    HIP_TRY(hipDeviceSynchronize());
    const double ms_h2d = ms_since(t0);

    is3d::DfgenParams p{};
    p.n = n; p.n_gla = n_gla; p.n_T = n_T; p.n_muB = n_muB;
    const double *q = d_in.p;
    p.mass = q; p.gspin = q + n; p.baryon = q + 2 * (size_t)n; p.sign = q + 3 * (size_t)n;
    q += 4 * (size_t)n;
    for (int s = 0; s < 4; s++) p.root[s] = q + (size_t)s * n_gla;
    for (int s = 0; s < 4; s++) p.weight[s] = q + (size_t)(4 + s) * n_gla;
    q += 8 * (size_t)n_gla;
    p.T = q; p.muB = q + n_T;
    p.two_pi2_hbarc3 = 2.0 * std::pow(M_PI, 2) * std::pow(is3d::kHbarC, 3);           // deltaf_table.cpp:18-19
    p.tables = d_out.p; p.integrals = d_out.p + (size_t)is3d::kDfgenTables * npt;
    p.status = d_status.p; p.bad_entry = d_bad.p;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    HIP_TRY(hipEventCreate(&ev0));
    struct EvGuard { hipEvent_t &a, &b; ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev_guard{ev0, ev1};
    HIP_TRY(hipEventCreate(&ev1));
    HIP_TRY(hipEventRecord(ev0, nullptr));
    hipLaunchKernelGGL(is3d::cf_dfgen_points, dim3((unsigned)npt), dim3(is3d::kDfgenWaves * 64), 0, nullptr, p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, nullptr));
    HIP_TRY(hipEventSynchronize(ev1));
    float ms_kernel = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms_kernel, ev0, ev1));

    t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpy(&st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tables, p.tables, (size_t)is3d::kDfgenTables * npt * sizeof(double), hipMemcpyDeviceToHost));
    if (integrals) HIP_TRY(hipMemcpy(integrals, p.integrals, (size_t)is3d::kDfgenIntegrals * npt * sizeof(double), hipMemcpyDeviceToHost));
    const double ms_d2h = ms_since(t0);
    if (stats) { stats->ms_kernel = ms_kernel; stats->ms_h2d = ms_h2d; stats->ms_d2h = ms_d2h; stats->n_massive = n_massive; stats->reserved = 0; }
    if (st != ~0ULL) {
        const size_t pt = (size_t)(st >> 8);
        const unsigned cond = (unsigned)(st & 0xff);
        const double Tp = T[pt % n_T], Bp = muB[pt / n_T];
        if (cond & is3d::kDfgenQstat) {
            int32_t k = -1;
            HIP_TRY(hipMemcpy(&k, d_bad.p + pt, sizeof k, hipMemcpyDeviceToHost));
            return set_error(IS3D_EDOMAIN, "f_eq is negative for T = %.6g, muB = %.6g GeV: list entry %d (mass %.6g GeV, baryon %g, sign %g) has "
                             "exp(E/T - b muB/T) + sign <= 0 at a quadrature node (the reference exits here)", Tp, Bp, k,
                             k >= 0 ? list->mass[k] : 0.0, k >= 0 ? list->baryon[k] : 0.0, k >= 0 ? list->sign[k] : 0.0);
        }
        std::string what;
        const auto add = [&what](const char *s) { if (!what.empty()) what += "; "; what += s; };
        if (cond & is3d::kDfgenBulkDenom) add("14-moment bulk denominator is zero");
        if (cond & is3d::kDfgenDiffDenom) add("14-moment diffusion denominator is zero (no baryons in the list?)");
        if (cond & is3d::kDfgenBetapi) add("shear denominator betapi is zero");
        if (cond & is3d::kDfgenBetabulk) add("bulk denominator betabulk is zero");
        if (cond & is3d::kDfgenBetaV) add("diffusion denominator betaV is zero");
        if (cond & is3d::kDfgenNonFinite) add("a coefficient or an integral is not finite");
        return set_error(IS3D_EDOMAIN, "T = %.6g, muB = %.6g GeV (grid point iT = %d, imuB = %d): %s (the reference exits here)", Tp, Bp,
                         (int)(pt % n_T), (int)(pt / n_T), what.c_str());
    }
    return IS3D_OK;
}
