// cf_yield_vah.hip -- is3d_total_yield_vah: the mean number of hadrons an anisotropic-hydro surface emits, from which an oversampled run of
// the VAH sampler (cf_sampler_vah.hip) takes its number of events; is3d_oversample_events: that rule.
//
// The reference has no VAH yield (calculate_total_yield is viscous-hydro only and works at the surface-average temperature; anisotropic
// hydro has no surface average of (Lambda, alpha_L)), so include/is3d_amd.h is the definition: the momentum integral of
// the smooth VAH integrand with the linear delta-f and no outflow cut over the cells with u.dsigma > 0.  f_a is an equilibrium distribution at
// the stretched momentum p' = (p_x, p_y, p_z / alpha_L), so in the local rest frame the integral is three radial ones per (cell, species):
//
//   N0 = sum_k w_k r_k e^{r_k} / (e^{E_k} + sign)      A0 | A2 = sum_k w_k (r_k | r_k^3) e^{r_k + E_k} / (e^{E_k} + sign)^2      E_k = sqrt(r_k^2 + (m / Lambda)^2)
//   N  = u.dsigma alpha_L g Lambda^3 / (2 pi^2 hbarc^3) (N0 + K_m m^2 A0 + K_p Lambda^2 A2)
//
// on the alpha = 1 Gauss-Laguerre nodes, K_m and K_p from the residual bulk pressure and pi_perp.  The species enter through (m, sign) only:
// the integrals are done per species CLASS, as the sampler's density integrals are.
//
//   cf_yield_vah_cells    thread <-> cell: u.dsigma, the basis, pi_XX + pi_YY + alpha_L^2 pi_ZZ, the coefficients (the cell's own or the ones
//                         cf_vah_coeffs wrote), the skipped and bad tests; four doubles per cell as separate arrays: Lambda, w = u.dsigma alpha_L
//                         Lambda^3, w K_m, w K_p Lambda^2 (skipped or bad: w = 0 and a harmless Lambda)
//   cf_yield_vah_classes  thread <-> (cell, class), grid (cell tile, class): the lanes of a wave are consecutive cells of one class -- the four
//                         loads coalesce, the class constants are wave-uniform.  Node-only factors once per workgroup in LDS; one exp_full,
//                         sqrt_nr and rcp_nr per node shared by the three sums.  w N0 + (w K_m) m^2 A0 + (w K_p Lambda^2) A2 per thread, wave
//                         shuffle, fixed LDS order, partial[class][tile]
//   cf_yield_vah_reduce   one workgroup per class adds its tiles in a fixed order
//
// No floating-point atomics; the tiling depends on n_cells only, so the result is bitwise the same from run to run and device to device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_device.h"
#include "cf_host.h"
#include "cf_math.h"
#include "cf_plan_geometry.h"
#include "cf_vah_coef.h"
#include "errors.h"

namespace is3d {

constexpr int kYvGlMax = 256;                  // n_gla <= 256, as for the samplers
constexpr int kYvBlock = 256;                  // threads of a workgroup
constexpr int kYvCellsPerThread = 4;
constexpr int kYvTile = kYvBlock * kYvCellsPerThread;   // cells of one (tile, class) workgroup

struct YieldVahCells {                         // device arrays
    const double *tau, *ux, *uy, *un, *dat, *dax, *day, *dan;
    const double *pi[10];                      // tt tx ty tn xx xy xn yy yn nn (include_shear)
    const double *bulkPi, *Lambda, *aL;
    const double *c0, *c1, *c2, *c4;           // the cells' own, or the ones cf_vah_coeffs interpolated
    int64_t n_cells, first_cell;
    int32_t include_bulk, include_shear;
    int32_t tables;                            // a cell with Lambda / hbarc or alpha_L not below the last node is a bad cell
    double L_last, aL_last;
    double *Lam, *w, *wKm, *wKp;               // out, [n_cells] each
    unsigned long long *status;                // [0] min bad cell (global index), [1] skipped cells
};

// pi^{mu nu} a_mu a_nu for a contravariant a = (t, x, y, n) in Milne coordinates: a_mu = (a^t, -a^x, -a^y, -tau^2 a^n)
__device__ __forceinline__ double contract_diag(const double (&pi)[10], double at, double ax, double ay, double an, double tau2)
{
    ax = -ax; ay = -ay; an = -tau2 * an;
    return pi[0] * at * at + pi[4] * ax * ax + pi[7] * ay * ay + pi[9] * an * an
         + 2.0 * (pi[1] * at * ax + pi[2] * at * ay + pi[3] * at * an + pi[5] * ax * ay + pi[6] * ax * an + pi[8] * ay * an);
}

__global__ void __launch_bounds__(kYvBlock) cf_yield_vah_cells(YieldVahCells v)
{
    const int64_t ic = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ic >= v.n_cells) return;
    // what a skipped or bad cell leaves: no weight, and a scale with which the class kernel's integrals are finite
    double Lam = 1.0, w = 0.0, wKm = 0.0, wKp = 0.0;
    const double tau = v.tau[ic], tau2 = tau * tau;
    const double dat = v.dat[ic], dax = v.dax[ic], day = v.day[ic], dan = v.dan[ic];
    const double ux = v.ux[ic], uy = v.uy[ic], un = v.un[ic];
    const double ut = sqrt(1.0 + ux * ux + uy * uy + tau2 * un * un);
    const double udsigma = ut * dat + ux * dax + uy * day + un * dan;
    const double Lambda = v.Lambda[ic], aL = v.aL[ic];
    if (udsigma <= 0.0) {
        atomicAdd(&v.status[1], 1ULL);
    } else if (!(Lambda > 0.0 && Lambda < INFINITY && aL > 0.0 && aL < INFINITY) || (v.tables && !(Lambda / kHbarC < v.L_last && aL < v.aL_last))) {
        atomicMin(&v.status[0], (unsigned long long)(v.first_cell + ic));
    } else {
        const double aL2 = aL * aL;
        double Km = 0.0, Kp = 0.0;
        if (v.include_bulk) {
            const double Pi = v.bulkPi[ic], c2 = v.c2[ic];
            Km = Pi * (v.c0[ic] + c2);
            Kp = Pi * (v.c1[ic] * aL2 + c2 * (2.0 + aL2));
        }
        if (v.include_shear) {
            double pi[10];
#pragma unroll
            for (int k = 0; k < 10; k++) pi[k] = v.pi[k][ic];
            // Milne_Basis (viscous_correction.cpp:8-27), as cf_sampler_vah_cells builds it
            const double uperp = sqrt(ux * ux + uy * uy), utperp = sqrt(1.0 + ux * ux + uy * uy);
            const double sinhL = tau * un / utperp, coshL = ut / utperp;
            const double Xt = uperp * coshL, Zt = sinhL, Xn = uperp * sinhL / tau, Zn = coshL / tau;
            double Xx = 1.0, Yx = 0.0, Xy = 0.0, Yy = 1.0;
            if (uperp > 1.e-5) { Xx = utperp * ux / uperp; Yx = -uy / uperp; Xy = utperp * uy / uperp; Yy = ux / uperp; }
            const double piXX = contract_diag(pi, Xt, Xx, Xy, Xn, tau2), piYY = contract_diag(pi, 0.0, Yx, Yy, 0.0, tau2),
                         piZZ = contract_diag(pi, Zt, 0.0, 0.0, Zn, tau2);
            Kp += v.c4[ic] * (piXX + piYY + aL2 * piZZ);
        }
        Kp *= (1.0 / 3.0);
        Lam = Lambda;
        w = udsigma * aL * (Lambda * Lambda * Lambda);
        wKm = w * Km;
        wKp = w * Kp * (Lambda * Lambda);
    }
    v.Lam[ic] = Lam; v.w[ic] = w; v.wKm[ic] = wKm; v.wKp[ic] = wKp;
}

// gl: [2][ngl] root1, weight1; partial: [ncls][n_tiles], n_tiles = gridDim.x
__global__ void __launch_bounds__(kYvBlock)
cf_yield_vah_classes(const double *__restrict__ Lam, const double *__restrict__ w, const double *__restrict__ wKm, const double *__restrict__ wKp,
                     int64_t n_cells, const double *__restrict__ cls_mass, const double *__restrict__ cls_sign, const double *__restrict__ gl, int ngl,
                     double *__restrict__ partial)
{
    __shared__ double l_r2[kYvGlMax], l_c1[kYvGlMax], l_c3[kYvGlMax], l_red[kYvBlock / 64];
    for (int k = threadIdx.x; k < ngl; k += blockDim.x) {
        const double r = gl[k], c1 = gl[ngl + k] * (r * exp(r));
        l_r2[k] = r * r; l_c1[k] = c1; l_c3[k] = c1 * (r * r);
    }
    __syncthreads();
    const int cls = blockIdx.y;                                  // wave-uniform (workgroup-uniform): no workgroup straddles two classes
    const double mass = cls_mass[cls], sign = cls_sign[cls], m2 = mass * mass;
    const int64_t cell0 = (int64_t)blockIdx.x * kYvTile + threadIdx.x;
    double acc = 0.0;
#pragma unroll 1
    for (int j = 0; j < kYvCellsPerThread; j++) {
        const int64_t cell = cell0 + (int64_t)j * kYvBlock;
        if (cell >= n_cells) break;
        const double mbar = mass / Lam[cell];
        const double mb2 = __builtin_fmin(mbar * mbar, 1.0e18);  // E_k <= 1e9: inside exp_full's domain, and its exponential is held below anyway
        double n0 = 0.0, a0 = 0.0, a2 = 0.0;
        for (int k = 0; k < ngl; k++) {
            // an exponential that overflowed is held at 1e300: its node adds < 1e-300 of its weight instead of a division by inf
            const double e = __builtin_fmin(exp_full(sqrt_nr(l_r2[k] + mb2)), 1.0e300), q = rcp_nr(e + sign), t = (e * q) * q;
            n0 = __builtin_fma(l_c1[k], q, n0);
            a0 = __builtin_fma(l_c1[k], t, a0);
            a2 = __builtin_fma(l_c3[k], t, a2);
        }
        acc += w[cell] * n0 + (wKm[cell] * m2) * a0 + wKp[cell] * a2;
    }
    // wave shuffle, then the waves' sums in wave order
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) l_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = l_red[0];
        for (int i = 1; i < kYvBlock / 64; i++) s += l_red[i];
        partial[(int64_t)cls * gridDim.x + blockIdx.x] = s;
    }
}

// class_sum[class] = the tiles of the class: thread t adds tiles t, t + 256, ... in order, then the fixed tree
__global__ void __launch_bounds__(kYvBlock) cf_yield_vah_reduce(const double *__restrict__ partial, int64_t n_tiles, double *__restrict__ class_sum)
{
    __shared__ double red[kYvBlock];
    const double *row = partial + (int64_t)blockIdx.x * n_tiles;
    double acc = 0.0;
    for (int64_t t = threadIdx.x; t < n_tiles; t += kYvBlock) acc += row[t];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = kYvBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) class_sum[blockIdx.x] = red[0];
}

}  // namespace is3d

namespace {

using DevMem = is3d::DevBuf<unsigned char>;

// the arrays of is3d_vah_cells (cf_host.h order) the yield reads: tau, u, dsigma, Lambda, alpha_L; pi_perp and c4 with shear; bulkPi and
// c0..c2 with bulk; the coefficients only without tables; never eta, T, Wx, Wy, c3
bool yield_array_needed(int a, const is3d_options *o, bool tables)
{
    const bool bulk = o->include_bulk_deltaf != 0, shear = o->include_shear_deltaf != 0;
    if (a == 0 || (a >= 2 && a <= 8) || a == 23 || a == 24) return true;
    if (a >= 10 && a <= 19) return shear;
    if (a == 20) return bulk;
    if (a >= 25 && a <= 27) return bulk && !tables;
    if (a == 29) return shear && !tables;
    return false;
}

}  // namespace

extern "C" int is3d_total_yield_vah(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab,
                                    const is3d_sampler_inputs *in, const is3d_options *opts, double *mean_yield, double *yield_by_species,
                                    is3d_yield_vah_stats *stats)
{
    using is3d::set_error;
    if (!cells || !species || !in || !opts || !mean_yield) return set_error(IS3D_EINVAL, "null argument");
    *mean_yield = 0.0;
    if (stats) memset(stats, 0, sizeof *stats);
    // the order of the anisotropic-hydro sampler's refusals (sampler_vah_check), all before any device use
    if (opts->dimension != 2 && opts->dimension != 3) return set_error(IS3D_EINVAL, "dimension must be 2 or 3 (got %d)", opts->dimension);
    if (in->fast != 0) return set_error(IS3D_EINVAL, "the anisotropic-hydro yield has no fast mode (fast = %d)", in->fast);
    if (in->feqmod) return set_error(IS3D_EINVAL, "the anisotropic-hydro yield takes no feqmod tables (in->feqmod must be NULL)");
    if (opts->dimension == 2 && !(in->y_cut > 0.0)) return set_error(IS3D_EINVAL, "2+1D: the yield is multiplied by 2 y_cut, which must be > 0");
    if (species->n < 1 || !species->mass || !species->sign || !species->degeneracy) return set_error(IS3D_EINVAL, "empty species list");
    if (in->n_gla < 1 || in->n_gla > is3d::kYvGlMax || !in->root1 || !in->weight1)
        return set_error(IS3D_EINVAL, "the yield needs the Gauss-Laguerre roots and weights for alpha = 1 (1 to %d nodes)", is3d::kYvGlMax);
    if (tab)
        if (int rc = is3d::vah_tables_check(tab)) return rc;
    const int64_t n = cells->n_cells;
    if (n < 0 || in->first_cell < 0) return set_error(IS3D_EINVAL, "n_cells and first_cell must be >= 0");
    if (n > 0) {
        const auto a = is3d::cell_arrays(*cells);
        for (int i = 0; i < is3d::kVahCellArrays; i++)
            if (!a[i] && yield_array_needed(i, opts, tab != nullptr)) return set_error(IS3D_EINVAL, "a VAH cell array that would be read is NULL (index %d)", i);
    }
    // species classes (mass, sign): the radial integrals are per class
    const int npart = species->n;
    const is3d::SpeciesClasses kc = is3d::species_classes(species->mass, species->sign, nullptr, npart, true);
    const std::vector<int32_t> &cls = kc.cls;
    const std::vector<double> &cmass = kc.cmass, &csign = kc.csign;
    const int ncls = (int)cmass.size();
    if (ncls > 65535) return set_error(IS3D_EINVAL, "%d species classes: the launch grid holds 65535", ncls);
    if (yield_by_species) memset(yield_by_species, 0, sizeof(double) * (size_t)npart);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    if (stats) stats->n_classes = ncls;
    if (n == 0) return IS3D_OK;
    if (opts->device >= 0) HIP_TRY(hipSetDevice(opts->device));

    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 4; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
    // ---- the needed cell arrays, the class constants and the nodes ----
    is3d::DevBuf<double> d_cells, d_work, d_coef, d_const, d_partial;
    DevMem d_status;
    HIP_TRY(d_cells.alloc((size_t)n * is3d::kVahCellArrays));
    HIP_TRY(hipEventRecord(ev[0], nullptr));
    is3d_vah_cells dc{};
    HIP_TRY(is3d::stage_cells(*cells, [&](int a) { return yield_array_needed(a, opts, tab != nullptr); }, 0, n, d_cells.p, nullptr, &dc));
    const int ngl = in->n_gla;
    std::vector<double> consts((size_t)2 * ncls + 2 * ngl);
    for (int c = 0; c < ncls; c++) { consts[c] = cmass[c]; consts[ncls + c] = csign[c]; }
    for (int k = 0; k < ngl; k++) { consts[2 * ncls + k] = in->root1[k]; consts[2 * ncls + ngl + k] = in->weight1[k]; }
    HIP_TRY(d_const.upload(consts));
    const unsigned long long st0[2] = {~0ULL, 0ULL};
    HIP_TRY(d_status.upload(st0, 2));
    HIP_TRY(hipEventRecord(ev[1], nullptr));

    is3d::YieldVahCells v{};
    v.tau = dc.tau; v.ux = dc.ux; v.uy = dc.uy; v.un = dc.un; v.dat = dc.dat; v.dax = dc.dax; v.day = dc.day; v.dan = dc.dan;
    const double *pi[10] = {dc.pitt, dc.pitx, dc.pity, dc.pitn, dc.pixx, dc.pixy, dc.pixn, dc.piyy, dc.piyn, dc.pinn};
    for (int k = 0; k < 10; k++) v.pi[k] = pi[k];
    v.bulkPi = dc.bulkPi; v.Lambda = dc.Lambda; v.aL = dc.aL;
    v.c0 = dc.c0; v.c1 = dc.c1; v.c2 = dc.c2; v.c4 = dc.c4;
    v.n_cells = n; v.first_cell = in->first_cell;
    v.include_bulk = opts->include_bulk_deltaf != 0; v.include_shear = opts->include_shear_deltaf != 0;
    v.tables = tab != nullptr;
    v.status = d_status.as<unsigned long long>();
    if (tab) {
        v.L_last = tab->L[tab->n_L - 1]; v.aL_last = tab->aL[tab->n_aL - 1];
        // as the sampler: a cell off the tables gets zeros from cf_vah_coeffs and goes into the same status word, whatever its u.dsigma
        HIP_TRY(d_coef.alloc((size_t)5 * n));
        double *out[5];
        for (int k = 0; k < 5; k++) out[k] = d_coef.p + (size_t)k * n;
        if (int rc = is3d::vah_coeffs_device(tab, n, in->first_cell, dc.Lambda, dc.aL, out, v.status)) return rc;
        v.c0 = out[0]; v.c1 = out[1]; v.c2 = out[2]; v.c4 = out[4];
    }
    HIP_TRY(d_work.alloc((size_t)4 * n));
    v.Lam = d_work.p; v.w = d_work.p + n; v.wKm = d_work.p + 2 * (size_t)n; v.wKp = d_work.p + 3 * (size_t)n;
    const int64_t n_tiles = (n + is3d::kYvTile - 1) / is3d::kYvTile;
    HIP_TRY(d_partial.alloc((size_t)ncls * n_tiles + ncls));
    double *d_class_sum = d_partial.p + (size_t)ncls * n_tiles;
    hipLaunchKernelGGL(is3d::cf_yield_vah_cells, dim3((unsigned)((n + is3d::kYvBlock - 1) / is3d::kYvBlock)), dim3(is3d::kYvBlock), 0, nullptr, v);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[2], nullptr));
    hipLaunchKernelGGL(is3d::cf_yield_vah_classes, dim3((unsigned)n_tiles, (unsigned)ncls), dim3(is3d::kYvBlock), 0, nullptr, v.Lam, v.w, v.wKm, v.wKp, n,
                       d_const.p, d_const.p + ncls, d_const.p + 2 * ncls, ngl, d_partial.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(is3d::cf_yield_vah_reduce, dim3((unsigned)ncls), dim3(is3d::kYvBlock), 0, nullptr, d_partial.p, n_tiles, d_class_sum);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[3], nullptr));
    std::vector<double> class_sum(ncls);
    unsigned long long st[2] = {~0ULL, 0ULL};
    HIP_TRY(hipMemcpy(class_sum.data(), d_class_sum, sizeof(double) * (size_t)ncls, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
    if (stats) {
        float a = 0, b = 0, c = 0;
        (void)hipEventElapsedTime(&a, ev[0], ev[1]);
        (void)hipEventElapsedTime(&b, ev[1], ev[2]);
        (void)hipEventElapsedTime(&c, ev[2], ev[3]);
        stats->ms_h2d = a; stats->ms_cells = b; stats->ms_classes = c;
        stats->n_cells_skipped = (int64_t)st[1];
    }
    const double two_pi2_hbarC3 = 2.0 * M_PI * M_PI * (is3d::kHbarC * is3d::kHbarC * is3d::kHbarC);
    const double rapidity = opts->dimension == 2 ? 2.0 * in->y_cut : 1.0;
    double total = 0.0;
    for (int s = 0; s < npart; s++) {
        const double ys = species->degeneracy[s] / two_pi2_hbarC3 * class_sum[cls[s]] * rapidity;
        if (yield_by_species) yield_by_species[s] = ys;
        total += ys;
    }
    *mean_yield = total;
    if (st[0] != ~0ULL)
        return set_error(IS3D_EDOMAIN, "cell %llu: Lambda or alpha_L is not finite and > 0, or (Lambda, alpha_L) lies beyond the last node of the VAH "
                         "coefficient tables; the yield holds the sum over the other cells", st[0]);
    return IS3D_OK;
}

extern "C" int is3d_oversample_events(double min_num_hadrons, double mean_yield, int32_t max_num_samples, int32_t *n_events)
{
    using is3d::set_error;
    if (!n_events) return set_error(IS3D_EINVAL, "null argument");
    *n_events = 0;
    if (!(min_num_hadrons > 0.0)) return set_error(IS3D_EINVAL, "min_num_hadrons must be > 0");
    if (max_num_samples < 1) return set_error(IS3D_EINVAL, "max_num_samples must be >= 1 (got %d)", max_num_samples);
    const double N = (double)fabsf((float)mean_yield);                            // "prevent overflow", emissionfunction.cpp:1528
    if (!(N > 0.0 && N < INFINITY)) return set_error(IS3D_EDOMAIN, "a mean yield of %g sizes no run: it must be finite and not 0", mean_yield);
    // Nevents = min((int)ceil(MIN_NUM_HADRONS / Ntotal), MAX_NUM_SAMPLES) (:1531); at least one event
    *n_events = (int32_t)std::fmax(1.0, std::fmin(std::ceil(min_num_hadrons / N), (double)max_num_samples));
    return IS3D_OK;
}
