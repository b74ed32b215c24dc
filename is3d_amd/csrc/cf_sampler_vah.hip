// cf_sampler_vah.hip -- particle sampler for anisotropic hydro (mode 2, operation 2) on the device.
//
// The reference's sample_dN_pTdpTdphidy_VAH_PL is an empty stub, so THIS is the definition (include/is3d_amd.h): the VAH
// analogue of sample_dN_pTdpTdphidy (emissionfunction_sampling_kernels.cpp:833-1225) in regular mode.  The leading-order distribution
// f_a = 1 / (exp(E_a / Lambda) + sign), E_a = sqrt((p.u)^2 + xi_L (p.z)^2), is an equilibrium distribution at the momentum
// p' = (p_x, p_y, p_z / alpha_L) of the local rest frame, so the sampler is the reference's df_mode-4 construction -- sample isotropically, map
// the momentum linearly -- with the residual delta-f of the smooth kernel (smooth_kernels.cpp:2323-2342) as a viscous weight:
//
//   bound density   dn_s = 2 alpha_L g_s Lambda^3 / (2 pi^2 hbarc^3) GaussThermal(neq_int; m_s / Lambda, sign_s)      (2 n_eq with T -> Lambda;
//                   alpha_L is the Jacobian d^3p = alpha_L d^3p'), dn_tot = (sum_s dn_s) 2 y_max ds_max                  (:1077)
//   draws           p' = sample_momentum(m, sign, T = Lambda, chem = 0);  p = (p'_x, p'_y, alpha_L p'_z);  E = sqrt(m^2 + p^2)
//   weights         w_flux = max(0, E dsigma_t - p.dsigma_space) / (E ds_max)
//                   w_visc = (1 + clamp(fbar_a df, -1, 1)) / 2,  fbar_a = 1 - sign f_a with E_a = E' (the energy of p'),
//                   df = c3 (p.z)(W.p) + c4 pi_perp^{mu nu} p_mu p_nu   [include_shear_deltaf]
//                      + (c0 m^2 + c1 (p.z)^2 + c2 (p.u)^2) Pi          [include_bulk_deltaf]
//   keep            u_keep < w_flux w_visc
//
// In the local rest frame p.u = E, p.z = -p_z, W.p = -(W_X p_x + W_Y p_y + W_Z p_z), and pi_perp^{mu nu} p_mu p_nu is the quadratic form of
// the ten tensor components on the basis (u, X, Y, Z) -- all ten are inputs, as for the smooth kernel, so the four components along u are
// carried too and the weight is the smooth kernel's for any input tensor.
//
// Everything else is the viscous sampler's (cf_sampler.hip, through cf_sampler_common.h): cf_sampler_density with Lambda as its temperature
// array, the species weights and their blocked running sums (the record's neq_fact is alpha_L Lambda^3 / (2 pi^2 hbarc^3)), cf_sampler_poisson,
// the hipCUB compaction and scan, the batch loop, the Philox streams keyed by (seed, stream, global cell, event) with their five roles, the
// basis, the dsigma boost, ds_max, the boost to the lab frame and the 2+1D rapidity draw.
//
//   cf_sampler_vah_cells  thread <-> cell: the record (SamplerCell: T = Lambda, pi.. = pi_perp in the LRF, V. = W in the LRF, bulkPi = the residual
//                         bulk pressure, c0..c4; VahCellExtra: alpha_L and the tensor components along u), the running sums, dn_tot
//   cf_sampler_run        thread <-> emitting (event, cell) pair: count pass and fill pass (cf_sampler_common.h, with VahModel)
//   cf_sampler_fused      the same pairs sampled once and binned as cf_sampler_bins does, without a list (is3d_sample_binned_vah)
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_device.h"
#include "cf_host.h"
#include "cf_math.h"
#include "cf_sampler_common.h"
#include "cf_vah_coef.h"
#include "errors.h"

namespace is3d {

struct VahCellExtra {
    double aL;
    double piuu, piux, piuy, piuz;      // pi_perp^{mu nu} u_mu u_nu, u_mu X_nu, u_mu Y_nu, u_mu Z_nu
};

struct VahSamplerCells {                // device arrays
    const double *tau, *eta, *ux, *uy, *un, *dat, *dax, *day, *dan;
    const double *pi[10];               // tt tx ty tn xx xy xn yy yn nn
    const double *bulkPi, *Wx, *Wy, *Lambda, *aL;
    const double *c[5];                 // the cells' own, or the ones cf_vah_coeffs interpolated
    int32_t tables;                     // c[] came from the tables: a cell off them is already in status[0] and has zeros ...
    double L_last, aL_last;             // ... it is one with Lambda / hbarc or alpha_L not below the last node (cf_vah_coeffs)
};

constexpr double kMaxLambdaOverMass = 1.0e4;        // a bad cell above (see cf_sampler_vah_cells)
constexpr double kMaxMeanNumber = 2147483648.0;     // dn_tot of a cell: what cf_sampler_poisson's int32 holds

// pi^{mu nu} a_mu b_nu for contravariant a, b = (t, x, y, n) in Milne coordinates: a_mu = (a^t, -a^x, -a^y, -tau^2 a^n)
__device__ __forceinline__ double contract2(const double (&pi)[10], const double (&a)[4], const double (&b)[4], double tau2)
{
    const double at = a[0], ax = -a[1], ay = -a[2], an = -tau2 * a[3];
    const double bt = b[0], bx = -b[1], by = -b[2], bn = -tau2 * b[3];
    return pi[0] * at * bt + pi[4] * ax * bx + pi[7] * ay * by + pi[9] * an * bn
         + pi[1] * (at * bx + ax * bt) + pi[2] * (at * by + ay * bt) + pi[3] * (at * bn + an * bt)
         + pi[5] * (ax * by + ay * bx) + pi[6] * (ax * bn + an * bx) + pi[8] * (ay * bn + an * by);
}

__global__ void __launch_bounds__(128)
cf_sampler_vah_cells(SamplerParams p, SamplerSpecies sp, VahSamplerCells v, const double *__restrict__ GT, SamplerCell *__restrict__ out,
                     VahCellExtra *__restrict__ extra)
{
    const int64_t ic = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ic >= p.n_cells) return;
    SamplerCell c;
    memset(&c, 0, sizeof c);
    VahCellExtra x = {1.0, 0.0, 0.0, 0.0, 0.0};
    const double tau = v.tau[ic], tau2 = tau * tau;
    const double dat = v.dat[ic], dax = v.dax[ic], day = v.day[ic], dan = v.dan[ic];
    const double ux = v.ux[ic], uy = v.uy[ic], un = v.un[ic];
    const double ut = sqrt(1.0 + ux * ux + uy * uy + tau2 * un * un);
    const double udsigma = ut * dat + ux * dax + uy * day + un * dan;
    if (udsigma <= 0.0) {                                                          // :899
        atomicAdd(&p.status[1], 1ULL);
        out[ic] = c; extra[ic] = x;
        return;
    }
    const double Lambda = v.Lambda[ic], aL = v.aL[ic];
    // a bad cell: a scale that is not finite and > 0 (no rejection loop is ever entered with it: the record stays dead), or one off the tables
    bool bad = !(Lambda > 0.0 && Lambda < INFINITY && aL > 0.0 && aL < INFINITY);
    if (!bad && v.tables) bad = !(Lambda / kHbarC < v.L_last && aL < v.aL_last);
    // ... or a Lambda beyond kMaxLambdaOverMass times a boson's mass: the bound of sample_momentum's light-boson rejection loop
    // (pion_thermal_weight_max) has a pole at m / Lambda = 2.5e-6, below which the loop would never accept
    for (int k = 0; k < sp.ncls && !bad; k++) bad = sp.cls_sign[k] == -1.0 && !(Lambda <= kMaxLambdaOverMass * sp.cls_mass[k]);
    if (bad) {
        atomicMin(&p.status[0], (unsigned long long)(p.first_cell + ic));
        out[ic] = c; extra[ic] = x;
        return;
    }
    // Milne_Basis (viscous_correction.cpp:8-27)
    const double uperp = sqrt(ux * ux + uy * uy), utperp = sqrt(1.0 + ux * ux + uy * uy);
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
    if (p.include_shear) {
        double pi[10];
#pragma unroll
        for (int k = 0; k < 10; k++) pi[k] = v.pi[k][ic];
        const double U[4] = {ut, ux, uy, un}, X[4] = {Xt, Xx, Xy, Xn}, Y[4] = {0.0, Yx, Yy, 0.0}, Z[4] = {Zt, 0.0, 0.0, Zn};
        c.pixx = contract2(pi, X, X, tau2); c.pixy = contract2(pi, X, Y, tau2); c.pixz = contract2(pi, X, Z, tau2);
        c.piyy = contract2(pi, Y, Y, tau2); c.piyz = contract2(pi, Y, Z, tau2); c.pizz = contract2(pi, Z, Z, tau2);
        x.piuu = contract2(pi, U, U, tau2); x.piux = contract2(pi, U, X, tau2); x.piuy = contract2(pi, U, Y, tau2); x.piuz = contract2(pi, U, Z, tau2);
        // W^tau, W^eta as the smooth kernel reconstructs them (smooth_kernels.cpp:2244-2245); LRF components as boost_Vmu_to_lrf
        const double Wx = v.Wx[ic], Wy = v.Wy[ic];
        const double Wt = (ux * Wx + uy * Wy) * ut / (utperp * utperp), Wn = Wt * un / ut;
        c.Vx = -Wt * Xt + Wx * Xx + Wy * Xy + tau2 * Wn * Xn;
        c.Vy = Wx * Yx + Wy * Yy;
        c.Vz = -Wt * Zt + tau2 * Wn * Zn;
    }
    c.bulkPi = p.include_bulk ? v.bulkPi[ic] : 0.0;
    c.c0 = v.c[0][ic]; c.c1 = v.c[1][ic]; c.c2 = v.c[2][ic]; c.c3 = v.c[3][ic]; c.c4 = v.c[4][ic];
    c.tau = tau; c.x = p.x ? p.x[ic] : 0.0; c.y = p.y ? p.y[ic] : 0.0;
    c.eta = p.dim3 ? v.eta[ic] : 0.0;
    c.ut = ut; c.ux = ux; c.uy = uy; c.un = un;
    c.T = Lambda;
    x.aL = aL;
    const double two_pi2_hbarC3 = 2.0 * M_PI * M_PI * (kHbarC * kHbarC * kHbarC);
    c.neq_fact = aL * (Lambda * Lambda * Lambda / two_pi2_hbarC3);
    const double dn = species_running_sums(p, sp, c, GT + ic, nullptr, nullptr, ic);
    c.dn_sum = dn;
    c.dn_tot = dn * (2.0 * p.y_max * c.ds_max);                                    // :1077
    if (!(c.dn_tot < kMaxMeanNumber)) {   // (a NaN too) the Poisson numbers are 32-bit: no cell of a surface comes near
        atomicMin(&p.status[0], (unsigned long long)(p.first_cell + ic));
        memset(&c, 0, sizeof c);
        out[ic] = c; extra[ic] = x;
        return;
    }
    c.live = (c.dn_tot > 0.0) ? 1.0 : 0.0;                                          // :1079
    out[ic] = c; extra[ic] = x;
}

// the anisotropic-hydro route's Model (cf_sampler_common.h): no tables beside GT; per pair the cell's VahCellExtra; per hadron an isotropic
// draw at Lambda stretched by alpha_L along z, with the residual delta-f (smooth_kernels.cpp:2323-2342) as the viscous weight
struct VahModel {
    static constexpr const double *gt2 = nullptr, *gt3 = nullptr;
    const VahCellExtra *extra;
    using Pair = VahCellExtra;
    __device__ __forceinline__ Pair pair(const SamplerParams &, const SamplerCell &, int64_t ic) const { return extra[ic]; }
    __device__ __forceinline__ double draw(const SamplerParams &p, const SamplerSpecies &, const SamplerCell &c, Pair x, int,
                                           double mass, double mass_squared, double sign, Rng &g_momentum, long &acceptances, long &samples,
                                           LrfMom &q) const
    {
        const LrfMom m = sample_momentum(g_momentum, acceptances, samples, mass, sign, c.T, 0.0);
        q.px = m.px; q.py = m.py; q.pz = x.aL * m.pz;
        q.E = sqrt(mass_squared + q.px * q.px + q.py * q.py + q.pz * q.pz);
        // the residual delta-f at this momentum; E_a = m.E
        double df = 0.0;
        if (p.include_shear) {
            const double pimunu_pmu_pnu = q.E * (q.E * x.piuu + 2.0 * (q.px * x.piux + q.py * x.piuy + q.pz * x.piuz))
                                        + q.px * q.px * c.pixx + q.py * q.py * c.piyy + q.pz * q.pz * c.pizz
                                        + 2.0 * (q.px * q.py * c.pixy + q.px * q.pz * c.pixz + q.py * q.pz * c.piyz);
            const double Wmu_pmu_pz = q.pz * (q.px * c.Vx + q.py * c.Vy + q.pz * c.Vz);   // (p.z)(W.p) = (-p_z)(-W_i p_i)
            df = c.c3 * Wmu_pmu_pz + c.c4 * pimunu_pmu_pnu;
        }
        if (p.include_bulk) df += (c.c0 * mass_squared + c.c1 * q.pz * q.pz + c.c2 * q.E * q.E) * c.bulkPi;
        const double fabar = 1.0 - sign / (exp(m.E / c.T) + sign);
        return (1.0 + fmax(-1.0, fmin(fabar * df, 1.0))) / 2.0;
    }
};

}  // namespace is3d

// ------------------------------------------------------------------------------------------------
// host entry
// ------------------------------------------------------------------------------------------------
namespace {

using DevMem = is3d::DevBuf<unsigned char>;

// what the variant's cells hook needs, and the model its launches read
struct VahRun {
    is3d::VahSamplerCells v{};
    const is3d_vah_df_tables *tab = nullptr;
    int64_t n = 0, first_cell = 0;
    DevMem d_coef, d_extra;
    is3d::VahModel model{};
};

int vah_cells_hook(void *ctx, const is3d::SamplerParams &p, const is3d::SamplerSpecies &sp, const double *GT, is3d::SamplerCell *rec)
{
    VahRun &r = *(VahRun *)ctx;
    if (r.tab) {
        double *out[5];
        for (int k = 0; k < 5; k++) { out[k] = r.d_coef.as<double>() + (size_t)k * r.n; r.v.c[k] = out[k]; }
        if (int rc = is3d::vah_coeffs_device(r.tab, r.n, r.first_cell, r.v.Lambda, r.v.aL, out, p.status)) return rc;
    }
    r.model.extra = r.d_extra.as<is3d::VahCellExtra>();
    hipLaunchKernelGGL(is3d::cf_sampler_vah_cells, dim3((unsigned)((r.n + 127) / 128)), dim3(128), 0, nullptr, p, sp, r.v, GT, rec,
                       r.d_extra.as<is3d::VahCellExtra>());
    return IS3D_OK;
}

// the arrays of is3d_vah_cells (cf_host.h order) the sampler reads: not T; eta in 3+1D; pi and W with shear, bulkPi with bulk; c0..c4 without tables
bool vah_array_needed(int a, const is3d_options *o, bool tables)
{
    if (a == 9) return false;
    if (a == 1) return o->dimension == 3;
    if (a >= 10 && a <= 19) return o->include_shear_deltaf != 0;
    if (a == 20) return o->include_bulk_deltaf != 0;
    if (a == 21 || a == 22) return o->include_shear_deltaf != 0;
    if (a >= 25) return !tables;
    return true;
}

}  // namespace

// everything refused before any device use; what is3d_sample_particles_vah_multi checks first too
int is3d::sampler_vah_check(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab, const is3d_sampler_inputs *in,
                            const is3d_options *opts)
{
    if (!cells || !species || !in || !opts) return set_error(IS3D_EINVAL, "null argument");
    if (opts->dimension != 2 && opts->dimension != 3) return set_error(IS3D_EINVAL, "dimension must be 2 or 3 (got %d)", opts->dimension);
    if (in->fast != 0) return set_error(IS3D_EINVAL, "the anisotropic-hydro sampler has no fast mode (fast = %d)", in->fast);
    if (in->feqmod) return set_error(IS3D_EINVAL, "the anisotropic-hydro sampler takes no feqmod tables (in->feqmod must be NULL)");
    if (in->n_events < 1) return set_error(IS3D_EINVAL, "n_events must be >= 1");
    if (species->n < 1 || !species->mass || !species->sign || !species->degeneracy) return set_error(IS3D_EINVAL, "empty species list");
    for (int s = 0; s < species->n; s++)
        if (!(species->mass[s] > 0.0)) return set_error(IS3D_EINVAL, "species %d has mass 0: photons cannot be sampled with this method", s);
    if (in->n_gla < 1 || in->n_gla > kSmpGlMax || !in->root1 || !in->weight1)
        return set_error(IS3D_EINVAL, "the sampler needs the Gauss-Laguerre roots and weights for alpha = 1 (1 to %d nodes)", kSmpGlMax);
    if (tab)
        if (int rc = vah_tables_check(tab)) return rc;
    const int64_t n = cells->n_cells;
    if (n < 0 || in->first_cell < 0 || n + in->first_cell > 0xffffffffLL)
        return set_error(IS3D_EINVAL, "cell indices must fit 32 bits for the counter-based streams");
    if (n > 0) {
        const auto a = cell_arrays(*cells);
        for (int i = 0; i < kVahCellArrays; i++)
            if (!a[i] && vah_array_needed(i, opts, tab != nullptr)) return set_error(IS3D_EINVAL, "a VAH cell array that would be read is NULL (index %d)", i);
    }
    return IS3D_OK;
}

namespace {
// what the host-pointer entries share: a plan for this surface; the needed cell arrays, then x and y, uploaded in one block; the variant
struct VahStaged {
    is3d_sampler_plan *P = nullptr;
    VahRun r;
    is3d::DevBuf<double> d_cells;
    std::array<const double *, 2> xy{};
    float ms_h2d = 0;
    is3d::SamplerVariant var{};
    ~VahStaged() { is3d_sampler_plan_destroy(P); }
};
// an empty surface stages nothing
int vah_stage(VahStaged &s, const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab, const is3d_sampler_inputs *in,
              const is3d_options *opts)
{
    const int64_t n = cells->n_cells;
    if (int rc = is3d::sampler_variant_plan_create(&s.P, species, in, opts, n)) return rc;
    VahRun &r = s.r;
    is3d::SamplerVariant &var = s.var;
    var.domain_text = "Lambda or alpha_L is not finite and > 0 (or Lambda > 1e4 boson masses, or the cell's mean hadron number >= 2^31), or "
                      "(Lambda, alpha_L) lies beyond the last node of the VAH coefficient tables";
    var.edomain_keeps_rest = true;
    var.ctx = &r;
    var.cells = vah_cells_hook;
    var.set_model(&r.model);
    if (n == 0) return IS3D_OK;
    r.tab = tab; r.n = n; r.first_cell = in->first_cell;
    HIP_TRY(s.d_cells.alloc((size_t)n * (is3d::kVahCellArrays + 2)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evg{e0, e1};
    HIP_TRY(hipEventRecord(e0, nullptr));
    is3d_vah_cells dc{};
    HIP_TRY(is3d::stage_cells(*cells, [&](int a) { return vah_array_needed(a, opts, tab != nullptr); }, 0, n, s.d_cells.p, nullptr, &dc));
    s.xy = {in->x, in->y};
    HIP_TRY(is3d::stage_arrays(s.xy, 0, n, s.d_cells.p + (size_t)is3d::kVahCellArrays * n, nullptr));
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&s.ms_h2d, e0, e1);
    is3d::VahSamplerCells &v = r.v;
    v.tau = dc.tau; v.eta = dc.eta; v.ux = dc.ux; v.uy = dc.uy; v.un = dc.un; v.dat = dc.dat; v.dax = dc.dax; v.day = dc.day; v.dan = dc.dan;
    const double *pi[10] = {dc.pitt, dc.pitx, dc.pity, dc.pitn, dc.pixx, dc.pixy, dc.pixn, dc.piyy, dc.piyn, dc.pinn};
    for (int k = 0; k < 10; k++) v.pi[k] = pi[k];
    v.bulkPi = dc.bulkPi; v.Wx = dc.Wx; v.Wy = dc.Wy; v.Lambda = dc.Lambda; v.aL = dc.aL;
    const double *cc[5] = {dc.c0, dc.c1, dc.c2, dc.c3, dc.c4};
    for (int k = 0; k < 5; k++) v.c[k] = cc[k];
    v.tables = tab != nullptr;
    if (tab) { v.L_last = tab->L[tab->n_L - 1]; v.aL_last = tab->aL[tab->n_aL - 1]; }
    if (tab) HIP_TRY(r.d_coef.alloc((size_t)5 * n * sizeof(double)));
    HIP_TRY(r.d_extra.alloc((size_t)n * sizeof(is3d::VahCellExtra)));
    var.T = dc.Lambda;
    return IS3D_OK;
}
}  // namespace

extern "C" int is3d_sample_particles_vah(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab,
                                         const is3d_sampler_inputs *in, const is3d_options *opts, is3d_particle *particles, int64_t capacity,
                                         int64_t *n_particles, is3d_sampler_stats *stats)
{
    using is3d::set_error;
    if (!n_particles) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (int rc = is3d::sampler_vah_check(cells, species, tab, in, opts)) return rc;
    VahStaged s;
    if (int rc = vah_stage(s, cells, species, tab, in, opts)) return rc;
    if (cells->n_cells == 0) return IS3D_OK;
    // (a bad cell, IS3D_EDOMAIN, leaves the other cells' hadrons sampled: the list is returned with the error -- edomain_keeps_rest)
    return is3d::sampler_variant_sample_list(s.P, s.var, cells->n_cells, s.xy[0], s.xy[1], in, s.ms_h2d, particles, capacity, n_particles, stats);
}

// the sampler with every hadron binned where it is sampled (cf_sampler_fused): no list on the device or the host.  kernel_form = 2 needs
// the block and the three tally words beside it in 64 KiB of LDS (sampler_fused_lds_fits: at most 8189 words), as for is3d_sample_fused
extern "C" int is3d_sample_binned_vah(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab,
                                      const is3d_sampler_inputs *in, const is3d_options *opts, const is3d_sampler_test_bins *bins,
                                      const is3d_sampler_hist *hist, int64_t *n_particles, is3d_sampler_stats *stats)
{
    using is3d::set_error;
    if (!n_particles) return set_error(IS3D_EINVAL, "null argument");
    *n_particles = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (int rc = is3d::sampler_vah_check(cells, species, tab, in, opts)) return rc;
    if (int rc = is3d::sampler_check_fused_args(bins, hist, in->n_events, species->n)) return rc;
    VahStaged s;
    if (int rc = vah_stage(s, cells, species, tab, in, opts)) return rc;
    const int rc = is3d::sampler_variant_execute_binned(s.P, s.var, cells->n_cells, s.xy[0], s.xy[1], in->n_events, in->seed, in->first_cell,
                                                        in->batch_events, bins, hist, true, n_particles, stats);
    if (stats) stats->ms_h2d = s.ms_h2d;
    return rc;
}
