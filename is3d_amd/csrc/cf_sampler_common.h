// cf_sampler_common.h -- what the particle samplers share (cf_sampler.hip: viscous hydro; cf_sampler_vah.hip: anisotropic hydro): the per-cell
// record, the species and parameter blocks, the Philox streams, the Gauss-Laguerre integrands, the species weights with their blocked
// running sums, the momentum sampler -- device code, inlined into each file's kernels -- and the host entries through which the
// anisotropic-hydro sampler runs its two kernels inside the viscous sampler's plan and batch loop (density integrals, Poisson numbers,
// hipCUB compaction and scan: cf_sampler.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

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

// ---- what a pass does with a kept hadron: the one thing in which count, fill and bin differ (sample_pair of cf_sampler.hip,
// vah_sample_pair of cf_sampler_vah.hip) ----
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
        const int64_t s = q.species;
        if (k.iyp >= 0) atomicAdd(&h[a.l.dy + s * a.b.y_bins + k.iyp], 1ULL);
        if (k.ieta >= 0) atomicAdd(&h[a.l.de + s * a.b.eta_bins + k.ieta], 1ULL);
        if (k.itau >= 0) atomicAdd(&h[a.l.dt + s * a.b.tau_bins + k.itau], 1ULL);
        if (k.ir >= 0) atomicAdd(&h[a.l.dr + s * a.b.r_bins + k.ir], 1ULL);
        if (k.ipT >= 0) {
            const int64_t j = s * a.b.pT_bins + k.ipT, plane = (int64_t)a.n_species * a.b.pT_bins;
            atomicAdd(&h[a.l.dp + j], 1ULL);
            for (int m = 0; m < IS3D_SAMPLER_VN_HARMONICS; m++) {
                double sn, cs;
                sincos(((double)m + 1.0) * k.phi, &sn, &cs);
                atomicAdd(&h[a.l.vr + m * plane + j], (unsigned long long)sampler_vn_fixed(cs));   // two's complement: signed sums
                atomicAdd(&h[a.l.vi + m * plane + j], (unsigned long long)sampler_vn_fixed(sn));
            }
        }
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

// the geometry of a fused bin pass (cf_sampler_fused, cf_sampler_vah_bin)
constexpr int kFusedBinThreads = 256;
constexpr int kFusedBinPrivateBlocks = 768;   // workgroup-private form: at most this many flushes (three 43 KiB blocks per CU of 160 KiB LDS)

// ---- host: a sampler variant inside the viscous sampler's plan and batch loop (cf_sampler.hip) ----
// what one launch of a variant's run kernel gets: the arguments of cf_sampler_run
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
// the bins of a binned run with what follows from them (is3d_sampler_plan_execute_binned, sampler_variant_execute_binned)
// fused: the viscous route samples and bins in one pass too (cf_sampler_fused) instead of filling and binning a list per batch; a variant
// with a bin hook always does
struct SamplerBinRun {
    is3d_sampler_test_bins bins;
    SamplerBinWidths widths;
    SamplerHistLayout layout;
    int fused;
};
// T: the DEVICE array the density integrals take as temperature; cells: writes the records (live, dn_sum, dn_tot and the running sums as
// cf_sampler_cells does; status[0], [1]) after the density kernel, returns an IS3D code; run: the count (fill = false) or fill pass on `grid`
// workgroups of 128; domain_text: what IS3D_EDOMAIN says after "cell N: ".
// bin (optional): the fused pass of a binned run -- the emitting pairs of a.active sampled once and every kept hadron added straight into
// hist_dev (layout b.layout) and yield_dev (one word per event of the run); of a, only rec, GT, event0, active, n_active and n_drawn are set
struct SamplerVariant {
    const double *T;
    const char *domain_text;
    void *ctx;
    int (*cells)(void *ctx, const SamplerParams &p, const SamplerSpecies &sp, const double *GT, SamplerCell *rec);
    void (*run)(void *ctx, bool fill, unsigned grid, const SamplerParams &p, const SamplerSpecies &sp, const SamplerRunArgs &a);
    void (*bin)(void *ctx, const SamplerParams &p, const SamplerSpecies &sp, const SamplerRunArgs &a, const SamplerBinRun &b,
                unsigned long long *hist_dev, unsigned long long *yield_dev);
};
// a plan with the species classes, the alpha = 1 Gauss-Laguerre nodes and the workspaces, without coefficient tables: df_mode 1 weights
// (2 neq_fact g GT), regular mode.  The argument checks come before any device use.
int sampler_variant_plan_create(is3d_sampler_plan **out, const is3d_species *species, const is3d_sampler_inputs *in, const is3d_options *opts,
                                int64_t max_cells);
// is3d_sampler_plan_execute with the variant's kernels in place of cf_sampler_cells and cf_sampler_run; the caller has checked its cells
int sampler_variant_execute(is3d_sampler_plan *P, const SamplerVariant &v, int64_t n_cells, const double *x_dev, const double *y_dev,
                            int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events, is3d_particle *particles_dev,
                            int64_t capacity, int64_t *n_particles, is3d_sampler_stats *stats);
// a binned run of a variant that has a bin hook: per event batch Poisson, select and ONE launch of the hook -- no counts, offsets, scan or
// particle workspace exist on this path.  The histograms live in the plan (zeroed before the first batch) and are copied to hist_host
// (HOST arrays, overwritten) once after the last batch, also when a bad cell gives IS3D_EDOMAIN; *n_particles is the sum of the yields.
// stats: ms_bin is the time of the fused passes; ms_count, ms_fill and particle_workspace_bytes are 0.  The caller has checked bins and
// hist (sampler_check_bin_args).
int sampler_variant_execute_binned(is3d_sampler_plan *P, const SamplerVariant &v, int64_t n_cells, const double *x_dev, const double *y_dev,
                                   int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events, const is3d_sampler_test_bins *bins,
                                   const is3d_sampler_hist *hist_host, int64_t *n_particles, is3d_sampler_stats *stats);
// the bin checks of is3d_sample_binned (IS3D_EINVAL, no device use): null, bad bins, kernel_form outside 0..2, and kernel_form = 2 on a
// histogram block of n_species species that does not fit the LDS
int sampler_check_bin_args(const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int32_t n_events, int32_t n_species);
// the same for the viscous fused entries (is3d_sample_fused): the private form needs room for the three tally words of sampler_tally beside
// the block
int sampler_check_fused_args(const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int32_t n_events, int32_t n_species);

// is3d_sample_particles_vah's refusals (IS3D_EINVAL), all before any device use: also what is3d_sample_particles_vah_multi checks first
int sampler_vah_check(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab, const is3d_sampler_inputs *in,
                      const is3d_options *opts);

}  // namespace is3d
