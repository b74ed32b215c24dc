// cf_sampler_common.h -- what the particle samplers share (cf_sampler.hip: viscous hydro; cf_sampler_vah.hip: anisotropic hydro): the per-cell
// record, the species and parameter blocks, the Philox streams, the Gauss-Laguerre integrands, the species weights with their blocked
// running sums, the momentum sampler, the per-pair loop and the two kernels that run it (cf_sampler_run, cf_sampler_fused: templates over
// the route's Model) -- device code, instantiated in each file -- and on the host the launch rule of each kernel and the entries through
// which a route runs as a SamplerVariant of the one plan and batch loop (density integrals, Poisson numbers, hipCUB compaction and scan:
// cf_sampler.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/is3d_amd.h"
#include "cf_device.h"
#include "cf_math.h"
#include "cf_sampler_bins.h"

namespace is3d {

struct SamplerCell {
    double live, breakdown;
    double T_mod, shear_mod, bulk_mod, z;          // df_mode 3, 4
    double tau, x, y, eta, ut, ux, uy, un, T;
    double Xt, Xx, Xy, Xn, Yx, Yy, Zt, Zn;
    double dst, dsx, dsy, dsz, ds_max;
    double pixx, pixy, pixz, piyy, piyz, pizz;     // LRF
    double bulkPi, dn_tot, dn_sum, neq_fact;
    double c0, c2, F, betabulk, betapi, shear14;
    // include_baryon: alpha_B (:962), alpha_B,mod (:1022), n_B/(E+P), T/betaV (:1026), V^i in the LRF (boost_Vmu_to_lrf), c1 c3 c4 | G betaV
    double alphaB, alphaB_mod, ber, diff_mod, Vx, Vy, Vz, c1, c3, c4, G, betaV;
};

struct SamplerSpecies {       // device arrays, length npart / ncls
    const double *mass, *sign, *degeneracy;
    const int32_t *cls;
    const double *cls_mass, *cls_sign;
    int32_t npart, ncls;
    const double *baryon, *cls_baryon;   // include_baryon, else NULL (the baryon number is part of the class key then)
};

struct SamplerParams {
    CellPtrs cells;
    const double *x, *y;
    int64_t n_cells, first_cell;
    int32_t dim3, df_mode, include_bulk, include_shear;
    int32_t baryon, baryondiff;  // include_baryon; && include_baryondiff_deltaf: mu_B, n_B, V^mu are read (:953-964)
    BilinearDev bil;             // baryon: c0..c4 (df_mode 1) | F G betabulk betaV betapi (df_mode 2, 3) on the (mu_B, T) grid
    SplineDev spl;              // 14-moment: c0, c2; Chapman-Enskog: F, betabulk, betapi
    int32_t ngl;
    const double *gl;           // [4][ngl]: root1, weight1, root2, weight2 (alpha = 2 only for df_mode 3)
    int32_t fast;               // species densities at the surface-average temperature (host arrays eqd, bkd)
    const double *eqd, *bkd;    // [npart] Equilibrium_Density, Bulk_Density (deltafReader.cpp:536-650)
    double T_sw, F_avg, betabulk_avg;   // fast breakdown test (emissionfunction.cpp:114-119)
    int32_t nj;                 // Jonah tables (df_mode 4): abscissa, lambda^2, z and their spline c's
    const double *jx, *jl2, *jz, *jcl, *jcz;
    double bp_max, detA_min, mass_pion0;
    double y_max;
    uint64_t seed;
    unsigned long long *status; // [0] min bad cell, [1] skipped, [2] momentum samples, [3] acceptances, [4] hadrons drawn, [5] breakdown cells
    double *cdf;                // [ceil(npart / kCdfBlock)][n_cells]: the running sum of a cell's species weights after every kCdfBlock-th species, as
                                // cf_sampler_cells adds them (NULL: df_mode 3)
};

// ---- Philox4x32-10 streams ----
struct Rng {
    uint32_t k0, k1, stream, cell, event, blk, buf[4];
    int pos;
    __device__ void init(uint64_t seed, uint32_t s, uint32_t c, uint32_t e)
    {
        k0 = (uint32_t)seed; k1 = (uint32_t)(seed >> 32);
        stream = s; cell = c; event = e; blk = 0; pos = 4;
    }
    __device__ double uniform()
    {
        if (pos >= 4) {
            uint32_t c0 = blk++, c1 = stream, c2 = cell, c3 = event, a = k0, b = k1;
#pragma unroll
            for (int r = 0; r < 10; r++) {
                const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
                const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
                c0 = hi1 ^ c1 ^ a; c1 = lo1; c2 = hi0 ^ c3 ^ b; c3 = lo0;
                a += 0x9E3779B9u; b += 0xBB67AE85u;
            }
            buf[0] = c0; buf[1] = c1; buf[2] = c2; buf[3] = c3;
            pos = 0;
        }
        const uint32_t a = buf[pos], b = buf[pos + 1];
        pos += 2;
        return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
    }
    __device__ long poisson(double mean)
    {
        long N = 0;
        double remaining = mean;
        while (remaining > 0.0) {
            const double l = remaining < 256.0 ? remaining : 256.0;
            remaining -= l;
            const double u = uniform();
            double p = exp(-l), F = p;
            long k = 0;
            while (u >= F && k < 4096) { k++; p *= l / (double)k; F += p; }
            N += k;
        }
        return N;
    }
};

// GaussThermal(neq_int | J10_int | J20_int, ...) (gaussThermal.cpp); chem = baryon * alpha_B
__device__ __forceinline__ double gt_neq(const double *root, const double *weight, int n, double mbar, double sign, double chem = 0.0)
{
    double s = 0.0;
    for (int k = 0; k < n; k++) {
        const double pbar = root[k], Ebar = sqrt(pbar * pbar + mbar * mbar);
        s += weight[k] * (pbar * exp(pbar) / (exp(Ebar - chem) + sign));
    }
    return s;
}

__device__ __forceinline__ double gt_J10(const double *root, const double *weight, int n, double mbar, double sign, double chem)
{
    double s = 0.0;
    for (int k = 0; k < n; k++) {
        const double pbar = root[k], Ebar = sqrt(pbar * pbar + mbar * mbar);
        const double qstat = exp(Ebar - chem) + sign;
        s += weight[k] * (pbar * exp(pbar + Ebar - chem) / (qstat * qstat));
    }
    return s;
}

__device__ __forceinline__ double gt_J20(const double *root, const double *weight, int n, double mbar, double sign, double chem = 0.0)
{
    double s = 0.0;
    for (int k = 0; k < n; k++) {
        const double pbar = root[k], Ebar = sqrt(pbar * pbar + mbar * mbar);
        const double qstat = exp(Ebar - chem) + sign;
        s += weight[k] * (Ebar * exp(pbar + Ebar - chem) / (qstat * qstat));
    }
    return s;
}

constexpr int kSmpGlMax = 256;   // n_gla <= 256 (is3d_sampler_plan_create checks)

// mean-number weight of species ip in a cell: fast_max_particle_number (:239-280) / max_particle_number (:282-359)
// gt, gt2, gt3: the cell's column of the class-major integral tables (GT + cell), element of class k at [k * p.n_cells]
// The running sums are kept for every kCdfBlock-th species only (round 5: 39 planes instead of 305 -- cf_sampler_cells was bound by these stores, 2.4 GB
// per 1e6 cells): a hadron's species is the bisection of the block sums followed by the producer's own additions inside one block, continued from the stored
// sum in front of it -- the same doubles in the same order, so the same species as the bisection of all 305 sums.
constexpr int kCdfBlock = 8;

__device__ __forceinline__ double species_dn(const SamplerParams &p, const SamplerSpecies &sp, const SamplerCell &c, const double *gt,
                                             const double *gt2, const double *gt3, int ip)
{
    const bool linear = p.df_mode <= 2 || c.breakdown != 0.0;
    if (p.fast) {
        if (linear) return 2.0 * p.eqd[ip];
        if (p.df_mode == 3) return p.eqd[ip] + c.bulkPi * p.bkd[ip];
        return c.z * p.eqd[ip];
    }
    const int64_t kk = (int64_t)sp.cls[ip] * p.n_cells;
    const double equilibrium_density = c.neq_fact * sp.degeneracy[ip] * gt[kk];
    if (linear) return 2.0 * equilibrium_density;
    if (p.df_mode == 3) {
        const double J20 = (c.T * c.neq_fact) * sp.degeneracy[ip] * gt2[kk];
        double bJ10G = 0.0;                                                             // baryon * J10 * G, :319-325
        if (gt3) bJ10G = sp.baryon[ip] * (c.neq_fact * sp.degeneracy[ip] * gt3[kk]) * c.G;
        const double bulk_density = (equilibrium_density + bJ10G + (J20 * c.F / c.T / c.T)) / c.betabulk;
        return equilibrium_density + c.bulkPi * bulk_density;
    }
    return c.z * equilibrium_density;
}

// :172-196
__device__ __forceinline__ double pion_thermal_weight_max(double x)
{
    const double x2 = x * x, x3 = x2 * x, x4 = x3 * x;
    const double max = (143206.88623164667 - 95956.76008684626 * x - 21341.937407169076 * x2 + 14388.446116867359 * x3 - 6083.775788504437 * x4) /
                       (-0.3541350577684533 + 143218.69233952634 * x - 24516.803600065778 * x2 - 115811.59391199696 * x3 + 35814.36403387459 * x4);
    return 1.00001 * max;
}

struct LrfMom { double E, px, py, pz; };

// sample_momentum (:456-617); chem = baryon * alpha_B enters the heavy-hadron weight only (:588)
__device__ inline LrfMom sample_momentum(Rng &g, long &acceptances, long &samples, double mass, double sign, double T, double chem)
{
    const double two_pi = 2.0 * M_PI;
    const double mbar = mass / T, mbar_squared = mbar * mbar;
    double pbar, Ebar, phi_over_2pi, costheta;
    if (mbar < 1.008) {
        double weq_max = 1.0;
        if (mbar < 0.8554 && sign == -1.0) weq_max = pion_thermal_weight_max(mbar);
        for (;;) {
            samples += 1;
            const double r1 = 1.0 - g.uniform(), r2 = 1.0 - g.uniform(), r3 = 1.0 - g.uniform();
            const double l1 = log(r1), l2 = log(r2), l3 = log(r3);
            const double l1_plus_l2 = l1 + l2;
            pbar = -(l1 + l2 + l3);
            Ebar = sqrt(pbar * pbar + mbar_squared);
            phi_over_2pi = l1_plus_l2 * l1_plus_l2 / (pbar * pbar);
            costheta = (l1 - l2) / l1_plus_l2;
            const double weight = 1.0 / (exp(Ebar) + sign) / weq_max / (r1 * r2 * r3);
            if (g.uniform() < weight) break;
        }
    } else {
        const double K0 = mbar_squared, K1 = 2.0 * mbar, K2 = 2.0, Ksum = K0 + K1 + K2;
        double kbar;
        for (;;) {
            samples += 1;
            const double uk = g.uniform() * Ksum;
            if (uk < K0) {
                kbar = -log(1.0 - g.uniform());
                phi_over_2pi = g.uniform();
                costheta = 2.0 * g.uniform() - 1.0;
            } else if (uk < K0 + K1) {
                const double l1 = log(1.0 - g.uniform()), l2 = log(1.0 - g.uniform());
                kbar = -(l1 + l2);
                phi_over_2pi = -l1 / kbar;
                costheta = 2.0 * g.uniform() - 1.0;
            } else {
                const double l1 = log(1.0 - g.uniform()), l2 = log(1.0 - g.uniform()), l3 = log(1.0 - g.uniform());
                const double l1_plus_l2 = l1 + l2;
                kbar = -(l1 + l2 + l3);
                phi_over_2pi = l1_plus_l2 * l1_plus_l2 / (kbar * kbar);
                costheta = (l1 - l2) / l1_plus_l2;
            }
            Ebar = kbar + mbar;
            pbar = sqrt(Ebar * Ebar - mbar_squared);
            const double exponent = exp(Ebar - chem);
            const double weight = pbar / Ebar * exponent / (exponent + sign);
            if (g.uniform() < weight) break;
        }
    }
    acceptances += 1;
    const double E = Ebar * T, pm = pbar * T, phi = phi_over_2pi * two_pi;
    const double sintheta = sqrt(1.0 - costheta * costheta);
    LrfMom q = {E, pm * sintheta * cos(phi), pm * sintheta * sin(phi), pm * costheta};
    return q;
}

// the running sums of a cell's species weights, added in list order (the order the reference adds them in) and stored after every
// kCdfBlock-th species when p.cdf is set; returns the sum over all species
__device__ __forceinline__ double species_running_sums(const SamplerParams &p, const SamplerSpecies &sp, const SamplerCell &c, const double *gt,
                                                       const double *gt2, const double *gt3, int64_t ic)
{
    double dn = 0.0;
    if (p.cdf) {
        // (the stores never alias the tables read: said so, and the loop unrolled, so that four species' loads are in flight per trip)
        double *__restrict__ cdf = p.cdf + ic;
        const double *__restrict__ gtr = gt;
#pragma unroll 4
        for (int ip = 0; ip < sp.npart; ip++) {
            dn += species_dn(p, sp, c, gtr, gt2, gt3, ip);
            if ((ip & (kCdfBlock - 1)) == kCdfBlock - 1 || ip == sp.npart - 1) cdf[(int64_t)(ip / kCdfBlock) * p.n_cells] = dn;
        }
    } else {
        for (int ip = 0; ip < sp.npart; ip++) dn += species_dn(p, sp, c, gt, gt2, gt3, ip);
    }
    return dn;
}

// the species of a hadron: the first one whose running sum exceeds ut_ = u * dn_sum (the last one if none does)
__device__ __forceinline__ int choose_species(const SamplerParams &p, const SamplerSpecies &sp, const SamplerCell &c, const double *gt,
                                              const double *gt2, const double *gt3, int64_t ic, double ut_)
{
    int chosen = sp.npart - 1;
    if (p.cdf) {
        // bisection of the sums species_running_sums stored -- the weights are >= 0 for df_mode 1, 2, 4, so the sums are non-decreasing and this IS
        // the linear inversion below, in 9 reads (round 5) ... of the sums at the block ends: the first block whose end sum exceeds ut_ (the last
        // block if none does), then the producer's additions inside it, continued from the sum stored in front of it
        int lo = 0, hi = (sp.npart + kCdfBlock - 1) / kCdfBlock - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ut_ < p.cdf[(int64_t)mid * p.n_cells + ic]) hi = mid;
            else lo = mid + 1;
        }
        double cum = lo ? p.cdf[(int64_t)(lo - 1) * p.n_cells + ic] : 0.0;
        const int ip1 = min((lo + 1) * kCdfBlock, sp.npart);
        chosen = ip1 - 1;
        for (int ip = lo * kCdfBlock; ip < ip1; ip++) {
            cum += species_dn(p, sp, c, gt, gt2, gt3, ip);
            if (ut_ < cum) { chosen = ip; break; }
        }
    } else {
        double cum = 0.0;
        for (int ip = 0; ip < sp.npart; ip++) {
            cum += species_dn(p, sp, c, gt, gt2, gt3, ip);
            if (ut_ < cum) { chosen = ip; break; }
        }
    }
    return chosen;
}

// the run-wide tallies of a count pass: one global atomic per counter and workgroup instead of three per sampling thread
__device__ __forceinline__ void sampler_tally(const SamplerParams &p, const unsigned long long (&tally)[3])
{
    __shared__ unsigned long long blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0ULL;
    __syncthreads();
    for (int k = 0; k < 3; k++)
        if (tally[k]) atomicAdd(&blk[k], tally[k]);
    __syncthreads();
    if (threadIdx.x < 3 && blk[threadIdx.x]) atomicAdd(&p.status[2 + threadIdx.x], blk[threadIdx.x]);
}

// ---- what a pass does with a kept hadron: the one thing in which count, fill and bin differ (sample_pair) ----
struct SamplerKeepCount {
    __device__ __forceinline__ void operator()(const is3d_particle &) {}
};
struct SamplerKeepFill {
    is3d_particle *__restrict__ particles;
    int64_t slot, capacity;
    __device__ __forceinline__ void operator()(const is3d_particle &o)
    {
        if (slot < capacity) particles[slot] = o;
        slot++;
    }
};
struct SamplerBinArgs {
    is3d_sampler_test_bins b;
    SamplerBinWidths w;
    SamplerHistLayout l;
    int n_species;
};
// the adds of cf_sampler_bins (cf_sampler_bins.hip) for one particle, into the workgroup's LDS block or the global one: 64-bit integer atomics
struct SamplerKeepBin {
    const SamplerBinArgs &a;
    unsigned long long *h;
    __device__ __forceinline__ void operator()(const is3d_particle &q)
    {
        const SamplerBinIndex k = sampler_bin_particle(a.b, a.w, q);
        sampler_bin_add(a.b, a.l, a.n_species, k, q.species, h);
    }
};

// The per-event yields of a fused bin pass.  The pairs are event-major, so the lanes of a wave see runs of equal events: the first lane of
// a run (leader ballot) adds the run's kept hadrons, a segmented sum over an inclusive wave scan -- one add per distinct event per wave.
// Called by EVERY lane of the wave, reconverged, outside any divergent loop; a lane without a pair comes with ev = INT_MAX and kept = 0.
__device__ __forceinline__ void sampler_yield_runs(int ev, long long kept, unsigned long long *__restrict__ yield)
{
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(ev, 1);
    const bool lead = lane == 0 || prev != ev;
    const unsigned long long leaders = __ballot(lead);
    long long incl = kept;                                               // inclusive scan of kept over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const unsigned long long above = lane == 63 ? 0ULL : (leaders >> (lane + 1)) << (lane + 1);
    const int last = (above ? __ffsll((long long)above) - 1 : 64) - 1;  // the last lane of the run that ends at the next leader
    const long long run = __shfl(incl, last) - incl + kept;
    if (lead && ev != INT_MAX && run) atomicAdd(&yield[ev], (unsigned long long)run);
}

// ---- the sampling kernels, written once for every route ----
// A Model is the small struct, passed by value to the kernels, that holds what differs between the routes (ViscousModel of cf_sampler.hip,
// VahModel of cf_sampler_vah.hip):
//   gt2, gt3   the J20 / J10 integral tables choose_species reads beside GT (null where the route has none)
//   Pair       what the route keeps per (event, cell) pair beside the cell record: Pair pair(p, c, ic)
//   draw       one momentum of the chosen species in the LRF with its viscous weight, from the momentum stream:
//              double draw(p, sp, c, pair, chosen, mass, mass_squared, sign, g_momentum, acceptances, samples, q) -> w_visc
//
// one emitting (event, cell) pair: the ONE piece of source the count, the fill and the fused bin pass of every route run.  ic is the pair's
// cell, ievent its event; every kept hadron goes to keep() as the is3d_particle of the list.  Returns the number kept; tally[] gets the
// pair's momentum samples, acceptances and hadrons drawn.
template <class Model, class Keep>
__device__ __forceinline__ long sample_pair(const SamplerParams &p, const SamplerSpecies &sp, const SamplerCell *__restrict__ cellrec,
                                            const double *__restrict__ GT, const Model &model, int ievent, int64_t ic, long N_hadrons,
                                            Keep &keep, unsigned long long (&tally)[3])
{
    const SamplerCell &c = cellrec[ic];
    const typename Model::Pair pair = model.pair(p, c, ic);
    const uint32_t gcell = (uint32_t)(p.first_cell + ic);
    Rng g_type, g_momentum, g_keep, g_rapidity;
    g_type.init(p.seed, 1, gcell, (uint32_t)ievent);
    g_momentum.init(p.seed, 2, gcell, (uint32_t)ievent);
    g_keep.init(p.seed, 3, gcell, (uint32_t)ievent);
    g_rapidity.init(p.seed, 4, gcell, (uint32_t)ievent);
    const double *gt = GT + ic, *gt2 = model.gt2 ? model.gt2 + ic : nullptr, *gt3 = model.gt3 ? model.gt3 + ic : nullptr;
    const double sinheta = sinh(c.eta), cosheta = sqrt(1.0 + sinheta * sinheta);   // :888-889
    long kept = 0, samples = 0, acceptances = 0;
    for (long ih = 0; ih < N_hadrons; ih++) {
        const double ut_ = g_type.uniform() * c.dn_sum;
        const int chosen = choose_species(p, sp, c, gt, gt2, gt3, ic, ut_);
        const double mass = sp.mass[chosen], mass_squared = mass * mass, sign = sp.sign[chosen];
        LrfMom q;
        const double w_visc = model.draw(p, sp, c, pair, chosen, mass, mass_squared, sign, g_momentum, acceptances, samples, q);
        // boost_pLRF_to_lab_frame (emissionfunction.cpp:40-51)
        const double ptau = q.E * c.ut + q.px * c.Xt + q.pz * c.Zt;
        const double plx = q.E * c.ux + q.px * c.Xx + q.py * c.Yx;
        const double ply = q.E * c.uy + q.px * c.Xy + q.py * c.Yy;
        const double pn = q.E * c.un + q.px * c.Xn + q.pz * c.Zn;
        const double w_flux = fmax(0.0, q.E * c.dst - q.px * c.dsx - q.py * c.dsy - q.pz * c.dsz) / (q.E * c.ds_max);   // :1148
        if (!(g_keep.uniform() < (w_flux * w_visc))) continue;
        double Elab, pz, eta = c.eta, sh = sinheta, ch = cosheta;
        if (!p.dim3) {                                                              // :1168-1186
            const double yp = p.y_max * (2.0 * g_rapidity.uniform() - 1.0);
            const double sinhy = sinh(yp), coshy = sqrt(1.0 + sinhy * sinhy);
            const double tau_pn = c.tau * pn, mT = sqrt(mass_squared + plx * plx + ply * ply);
            sh = (ptau * sinhy - tau_pn * coshy) / mT;
            eta = asinh(sh);
            ch = sqrt(1.0 + sh * sh);
            pz = mT * sinhy;
            Elab = mT * coshy;
        } else {
            pz = c.tau * pn * ch + ptau * sh;
            Elab = sqrt(mass_squared + plx * plx + ply * ply + pz * pz);
        }
        is3d_particle o;
        o.cell = p.first_cell + ic; o.event = ievent; o.species = chosen;
        o.tau = c.tau; o.x = c.x; o.y = c.y; o.eta = eta; o.t = c.tau * ch; o.z = c.tau * sh;
        o.E = Elab; o.px = plx; o.py = ply; o.pz = pz;
        keep(o);
        kept++;
    }
    tally[0] += (unsigned long long)samples; tally[1] += (unsigned long long)acceptances; tally[2] += (unsigned long long)N_hadrons;
    return kept;
}

// the geometry of the two kernels
constexpr int kRunThreads = 128;
constexpr int kFusedBinThreads = 256;
constexpr int kFusedBinPrivateBlocks = 768;   // workgroup-private form: at most this many flushes (three 43 KiB blocks per CU of 160 KiB LDS)

// thread <-> emitting (event, cell) pair: the count pass (counts[] and the run-wide tallies) and the fill pass of the list route
template <class Model, bool FILL>
__global__ void __launch_bounds__(kRunThreads)
cf_sampler_run(SamplerParams p, SamplerSpecies sp, const SamplerCell *__restrict__ cellrec, const double *__restrict__ GT, Model model,
               int event0, const int32_t *__restrict__ active, int64_t n_active, const int32_t *__restrict__ n_drawn,
               int64_t *__restrict__ counts, const int64_t *__restrict__ offsets, int64_t base, is3d_particle *__restrict__ particles,
               int64_t capacity)
{
    unsigned long long tally[3] = {0ULL, 0ULL, 0ULL};
    const int64_t ia = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // position in the list of emitting (event, cell) pairs
    if (ia < n_active && !(FILL && offsets[ia + 1] == offsets[ia])) {       // (fill: pass 1 kept nothing here, nothing to replay)
        const int64_t idx = active[ia];                                     // event-major: (event - event0) * n_cells + cell
        const int ievent = event0 + (int)(idx / p.n_cells);
        const int64_t ic = idx % p.n_cells;
        const long N_hadrons = n_drawn[idx];                                // cf_sampler_poisson (stream 0)
        if (FILL) {
            SamplerKeepFill keep{particles, base + offsets[ia], capacity};
            sample_pair(p, sp, cellrec, GT, model, ievent, ic, N_hadrons, keep, tally);
        } else {
            SamplerKeepCount keep;
            counts[ia] = sample_pair(p, sp, cellrec, GT, model, ievent, ic, N_hadrons, keep, tally);
        }
    }
    if (!FILL) sampler_tally(p, tally);
}

// The fused pass of a binned run: the count pass's threads, streams and loop, every kept hadron added straight into the histograms of
// cf_sampler_bins (the same rule, cf_sampler_bins.h, on the same is3d_particle the fill pass would store) -- no list, so no counts,
// offsets, scan or particle workspace.  Every add is a 64-bit integer, so the histograms are those of the list route bit for bit
// whatever the order of arrival.
//   PRIVATE: the whole block lives in dynamic LDS (ds_add_u64), at most kFusedBinPrivateBlocks workgroups walk the pair list grid-stride
//            and each flushes its non-zero words once with global adds
//   else:    every add goes straight to the global block (305 species: 305 x 1800 words)
// Per-event yields: sampler_yield_runs after the rejection loop, with the wave reconverged; lanes past n_active take part with event
// INT_MAX and kept = 0.  The trip count is the same for every thread of a workgroup: the wave operations see whole waves and the barriers
// every thread; none of either sits inside the per-hadron loop.
template <class Model, bool PRIVATE>
__global__ void __launch_bounds__(kFusedBinThreads, 2)
cf_sampler_fused(SamplerParams p, SamplerSpecies sp, const SamplerCell *__restrict__ cellrec, const double *__restrict__ GT, Model model,
                 int event0, const int32_t *__restrict__ active, int64_t n_active, const int32_t *__restrict__ n_drawn, SamplerBinArgs a,
                 unsigned long long *__restrict__ hist, unsigned long long *__restrict__ yield)
{
    extern __shared__ unsigned long long priv[];
    if (PRIVATE) {
        for (int64_t j = threadIdx.x; j < a.l.total; j += kFusedBinThreads) priv[j] = 0ULL;
        __syncthreads();
    }
    SamplerKeepBin keep{a, PRIVATE ? priv : hist};
    unsigned long long tally[3] = {0ULL, 0ULL, 0ULL};
    for (int64_t i0 = (int64_t)blockIdx.x * kFusedBinThreads; i0 < n_active; i0 += (int64_t)gridDim.x * kFusedBinThreads) {
        const int64_t ia = i0 + threadIdx.x;
        int ev = INT_MAX;
        long long kept = 0;
        if (ia < n_active) {
            const int64_t idx = active[ia];
            ev = event0 + (int)(idx / p.n_cells);
            kept = sample_pair(p, sp, cellrec, GT, model, ev, idx % p.n_cells, (long)n_drawn[idx], keep, tally);
        }
        sampler_yield_runs(ev, kept, yield);
    }
    sampler_tally(p, tally);
    if (PRIVATE) {
        __syncthreads();
        for (int64_t j = threadIdx.x; j < a.l.total; j += kFusedBinThreads) {
            const unsigned long long v = priv[j];
            if (v) atomicAdd(&hist[j], v);
        }
    }
}

// ---- host: the launch rule of each kernel, a sampler variant, and the plan and batch loop every variant runs in (cf_sampler.hip) ----
// what one launch gets beside the plan's parameters and species: the arguments of cf_sampler_run; a fused pass reads rec, GT, event0,
// active, n_active and n_drawn only
struct SamplerRunArgs {
    const SamplerCell *rec;
    const double *GT;
    int event0;
    const int32_t *active;
    int64_t n_active;
    const int32_t *n_drawn;
    int64_t *counts;
    const int64_t *offsets;
    int64_t base;
    is3d_particle *particles;
    int64_t capacity;
};
// the bins of a binned run with what follows from them
struct SamplerBinRun {
    is3d_sampler_test_bins bins;
    SamplerBinWidths widths;
    SamplerHistLayout layout;
};

// the count (fill = false) or fill pass: one thread per emitting pair
template <class Model>
void launch_run(const void *model, bool fill, const SamplerParams &p, const SamplerSpecies &sp, const SamplerRunArgs &a)
{
    const dim3 grid((unsigned)((a.n_active + kRunThreads - 1) / kRunThreads)), block(kRunThreads);
    const auto kernel = fill ? cf_sampler_run<Model, true> : cf_sampler_run<Model, false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, nullptr, p, sp, a.rec, a.GT, *(const Model *)model, a.event0, a.active, a.n_active, a.n_drawn,
                       a.counts, a.offsets, a.base, a.particles, a.capacity);
}

// Both forms of cf_sampler_fused keep the three words of sampler_tally in static LDS beside the dynamic block, so a private block fits
// when block + 3 words <= 64 KiB (8189 words): THE rule of every fused entry.  kernel_form 0 takes the global form on a block beyond it,
// kernel_form 2 is refused there (sampler_check_fused_args).
inline bool sampler_fused_lds_fits(const SamplerHistLayout &l) { return l.total + 3 <= (int64_t)(65536 / sizeof(unsigned long long)); }

// the fused pass: one launch per event batch.  Private form: at most kFusedBinPrivateBlocks workgroups, each walking the pair list
// grid-stride; global form: one trip per thread
template <class Model>
void launch_fused(const void *model, const SamplerParams &p, const SamplerSpecies &sp, const SamplerRunArgs &a, const SamplerBinRun &b,
                  unsigned long long *hist_dev, unsigned long long *yield_dev)
{
    const bool priv = b.bins.kernel_form == 2 || (b.bins.kernel_form == 0 && sampler_fused_lds_fits(b.layout));
    const int64_t trips = (a.n_active + kFusedBinThreads - 1) / kFusedBinThreads;
    const dim3 grid((unsigned)(priv ? std::min<int64_t>(trips, kFusedBinPrivateBlocks) : trips)), block(kFusedBinThreads);
    const auto kernel = priv ? cf_sampler_fused<Model, true> : cf_sampler_fused<Model, false>;
    hipLaunchKernelGGL(kernel, grid, block, priv ? (size_t)b.layout.total * sizeof(unsigned long long) : 0, nullptr, p, sp, a.rec, a.GT,
                       *(const Model *)model, a.event0, a.active, a.n_active, a.n_drawn, SamplerBinArgs{b.bins, b.widths, b.layout, sp.npart},
                       hist_dev, yield_dev);
}

// A sampler route inside the plan and batch loop: the viscous sampler is the variant of its own plan (cf_sampler.hip), the anisotropic-hydro
// sampler one on a plan without coefficient tables (cf_sampler_vah.hip).
//   T, muB        the DEVICE arrays the density integrals take as temperature and chemical potential (muB NULL: none)
//   cells         writes the records (live, dn_sum, dn_tot and the running sums as cf_sampler_cells does; status[0], [1]) after the density
//                 kernel and readies *model; returns an IS3D code
//   model         the route's Model with its two launch rules (set_model)
//   domain_text   what IS3D_EDOMAIN says after "cell N: "
//   edomain_keeps_rest   the one difference in behaviour between the families: after IS3D_EDOMAIN the list or the histograms of the good
//                 cells are still returned with the error (anisotropic hydro) or the entry returns at once (viscous hydro)
struct SamplerVariant {
    const double *T = nullptr, *muB = nullptr;
    std::string domain_text;
    bool edomain_keeps_rest = false;
    void *ctx = nullptr;
    int (*cells)(void *ctx, const SamplerParams &p, const SamplerSpecies &sp, const double *GT, SamplerCell *rec) = nullptr;
    const void *model = nullptr;
    void (*run)(const void *model, bool fill, const SamplerParams &p, const SamplerSpecies &sp, const SamplerRunArgs &a) = nullptr;
    void (*fused)(const void *model, const SamplerParams &p, const SamplerSpecies &sp, const SamplerRunArgs &a, const SamplerBinRun &b,
                  unsigned long long *hist_dev, unsigned long long *yield_dev) = nullptr;
    template <class Model>
    void set_model(const Model *m) { model = m; run = launch_run<Model>; fused = launch_fused<Model>; }
};
// a plan with the species classes, the alpha = 1 Gauss-Laguerre nodes and the workspaces, without coefficient tables: df_mode 1 weights
// (2 neq_fact g GT), regular mode.  The argument checks come before any device use.
int sampler_variant_plan_create(is3d_sampler_plan **out, const is3d_species *species, const is3d_sampler_inputs *in, const is3d_options *opts,
                                int64_t max_cells);
// the list of a run (particles_dev: DEVICE buffer of `capacity` entries, or NULL for the count); the caller has checked its cells
int sampler_variant_execute(is3d_sampler_plan *P, const SamplerVariant &v, int64_t n_cells, const double *x_dev, const double *y_dev,
                            int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events, is3d_particle *particles_dev,
                            int64_t capacity, int64_t *n_particles, is3d_sampler_stats *stats);
// ... and the tail of the host-pointer list entries: the device buffer, the run of `in`, and the copy to `particles` (HOST, or NULL for the
// count) -- also after IS3D_ENOMEM and, for a variant with edomain_keeps_rest, IS3D_EDOMAIN, with the error's text kept
int sampler_variant_sample_list(is3d_sampler_plan *P, const SamplerVariant &v, int64_t n_cells, const double *x_dev, const double *y_dev,
                                const is3d_sampler_inputs *in, float ms_h2d, is3d_particle *particles, int64_t capacity, int64_t *n_particles,
                                is3d_sampler_stats *stats);
// A binned run.  fuse: per event batch Poisson, select and ONE launch of cf_sampler_fused -- no counts, offsets, scan or particle workspace
// exist on this path (stats: ms_bin is the time of the fused passes; ms_count, ms_fill and particle_workspace_bytes are 0); else each
// batch's list is counted, scanned, filled into the plan's workspace, binned by cf_sampler_bins and dropped.  The histograms live in the
// plan (zeroed before the first batch) and are copied to hist_host (HOST arrays, overwritten) once after the last batch; *n_particles is
// the number of hadrons binned.  The caller has checked bins and hist (sampler_check_bin_args | sampler_check_fused_args) and its cells.
int sampler_variant_execute_binned(is3d_sampler_plan *P, const SamplerVariant &v, int64_t n_cells, const double *x_dev, const double *y_dev,
                                   int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events, const is3d_sampler_test_bins *bins,
                                   const is3d_sampler_hist *hist_host, bool fuse, int64_t *n_particles, is3d_sampler_stats *stats);
// the bin checks of the list kernel's entries (is3d_sample_binned, is3d_sampler_bin_list_device; IS3D_EINVAL, no device use): null, bad
// bins, kernel_form outside 0..2, and kernel_form = 2 on a histogram block of n_species species beyond sampler_bins_lds_fits (8192 words)
int sampler_check_bin_args(const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int32_t n_events, int32_t n_species);
// the same for every fused entry, viscous and anisotropic: kernel_form = 2 needs sampler_fused_lds_fits
int sampler_check_fused_args(const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int32_t n_events, int32_t n_species);
// A binned run's histograms for an entry outside cf_sampler.hip (is3d_decay_particles_binned).  begin: the caller's arrays (layout l,
// n_events yields) zeroed and, with `device`, the block  histograms | yields | extra_words  grown on the current device and zeroed on the
// null stream; end: the one copy of histograms and yields to the caller's arrays; check_counts: IS3D_EDOMAIN for a dN_pT bin above
// IS3D_SAMPLER_VN_MAX_COUNT.
template <class T> struct DevBuf;
int sampler_hist_begin(DevBuf<unsigned char> &d_hist, const is3d_sampler_hist *hist, const SamplerHistLayout &l, int32_t n_events,
                       int64_t extra_words, bool device);
int sampler_hist_end(const DevBuf<unsigned char> &d_hist, const is3d_sampler_hist *hist, const SamplerHistLayout &l, int32_t n_events);
int sampler_hist_check_counts(const is3d_sampler_hist *hist, const SamplerHistLayout &l);

// is3d_sample_particles_vah's refusals (IS3D_EINVAL), all before any device use: also what is3d_sample_particles_vah_multi checks first
int sampler_vah_check(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab, const is3d_sampler_inputs *in,
                      const is3d_options *opts);

}  // namespace is3d
