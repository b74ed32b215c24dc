// cf_sampler_bins.h -- the per-particle bin rule of the test_sampler = 1 distributions (sample_dN_dy, sample_dN_deta, sample_dN_2pipTdpTdy,
// sample_vn, sample_dN_dX: emissionfunction_sampling_kernels.cpp:31-152), stated ONCE for the host (host_io.cpp: is3d_sampler_bin_list,
// is3d_write_sampler_tests) and the device (cf_sampler_bins.hip).
//
// The arithmetic that decides a bin -- the sums of squares under the square roots, the subtractions, the divisions by the bin width, floor --
// is compiled with floating-point contraction OFF on both sides and with true divisions by widths that the host computes once
// (sampler_bin_widths) and hands to the kernel as bits.  +, -, *, /, sqrt and floor are correctly rounded on both sides, so host and device
// reach the same bin from the same particle bits everywhere except through log, which only yp uses (iyp and the |yp| <= y_cut gate).
// phi goes through atan2 and feeds only the harmonic terms, never a bin.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/is3d_amd.h"

#if defined(__HIP__) || defined(__HIPCC__) || defined(__CUDACC__)
#define IS3D_BINS_HD __host__ __device__ inline
#else
#define IS3D_BINS_HD inline
#endif
#if defined(__clang__)
#define IS3D_BINS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define IS3D_BINS_NO_CONTRACT _Pragma("STDC FP_CONTRACT OFF")
#endif

namespace is3d {

struct SamplerBinWidths { double yw, ew, pw, tw, rw; };

// the bins of one particle: an index is -1 where the particle adds nothing to that histogram (outside the range, or outside |yp| <= y_cut
// for ipT, itau, ir); phi in [0, 2 pi) is meaningful when ipT >= 0
struct SamplerBinIndex {
    int iyp, ieta, ipT, itau, ir;
    double phi;
};

// the element offsets of the arrays of is3d_sampler_hist laid end to end (the device block, and the workgroup's private copy):
// dN_dy | dN_deta | dN_pT | dN_tau | dN_r | vn_re | vn_im; yield is kept apart
struct SamplerHistLayout {
    int64_t dy, de, dp, dt, dr, vr, vi, total;
};

IS3D_BINS_HD SamplerHistLayout sampler_hist_layout(const is3d_sampler_test_bins &b, int n_species)
{
    SamplerHistLayout l;
    const int64_t S = n_species;
    l.dy = 0;
    l.de = l.dy + S * b.y_bins;
    l.dp = l.de + S * b.eta_bins;
    l.dt = l.dp + S * b.pT_bins;
    l.dr = l.dt + S * b.tau_bins;
    l.vr = l.dr + S * b.r_bins;
    l.vi = l.vr + (int64_t)IS3D_SAMPLER_VN_HARMONICS * S * b.pT_bins;
    l.total = l.vi + (int64_t)IS3D_SAMPLER_VN_HARMONICS * S * b.pT_bins;
    return l;
}

// positive bin counts and non-empty ranges (a zero width would divide by zero)
IS3D_BINS_HD bool sampler_bins_valid(const is3d_sampler_test_bins &b)
{
    return b.y_bins >= 1 && b.eta_bins >= 1 && b.pT_bins >= 1 && b.tau_bins >= 1 && b.r_bins >= 1 && b.y_cut > 0.0 && b.eta_cut > 0.0 &&
           b.pT_upper_cut > b.pT_lower_cut && b.tau_max > b.tau_min && b.r_max > b.r_min;
}

IS3D_BINS_HD SamplerBinWidths sampler_bin_widths(const is3d_sampler_test_bins &b)
{
    IS3D_BINS_NO_CONTRACT
    SamplerBinWidths w;
    w.yw = 2.0 * b.y_cut / (double)b.y_bins;
    w.ew = 2.0 * b.eta_cut / (double)b.eta_bins;
    w.pw = (b.pT_upper_cut - b.pT_lower_cut) / (double)b.pT_bins;
    w.tw = (b.tau_max - b.tau_min) / (double)b.tau_bins;
    w.rw = (b.r_max - b.r_min) / (double)b.r_bins;
    return w;
}

// floor((v - lo) / width) as an index of [0, bins), or -1
IS3D_BINS_HD int sampler_bin_of(double v, double lo, double width, int bins)
{
    IS3D_BINS_NO_CONTRACT
    const double d = v - lo;
    const double f = floor(d / width);
    return (f >= 0.0 && f < (double)bins) ? (int)f : -1;   // (NaN compares false: no bin)
}

IS3D_BINS_HD SamplerBinIndex sampler_bin_particle(const is3d_sampler_test_bins &b, const SamplerBinWidths &w, const is3d_particle &q)
{
    IS3D_BINS_NO_CONTRACT
    SamplerBinIndex o;
    const double num = q.E + q.pz, den = q.E - q.pz;
    const double yp = 0.5 * log(num / den);
    o.iyp = sampler_bin_of(yp, -b.y_cut, w.yw, b.y_bins);                          // sample_dN_dy
    o.ieta = sampler_bin_of(q.eta, -b.eta_cut, w.ew, b.eta_bins);                   // sample_dN_deta
    o.ipT = o.itau = o.ir = -1;
    o.phi = 0.0;
    if (fabs(yp) <= b.y_cut) {
        const double px2 = q.px * q.px, py2 = q.py * q.py;
        const double pT = sqrt(px2 + py2);
        o.ipT = sampler_bin_of(pT, b.pT_lower_cut, w.pw, b.pT_bins);                // sample_dN_2pipTdpTdy, sample_vn
        if (o.ipT >= 0) {
            double phi = atan2(q.py, q.px);
            if (phi < 0.0) phi += 2.0 * M_PI;
            o.phi = phi;
        }
        const double x2 = q.x * q.x, y2 = q.y * q.y;
        const double r = sqrt(x2 + y2);                                             // sample_dN_dX
        o.itau = sampler_bin_of(q.tau, b.tau_min, w.tw, b.tau_bins);
        o.ir = sampler_bin_of(r, b.r_min, w.rw, b.r_bins);
    }
    return o;
}

// one harmonic term in fixed point: llrint(term * 2^32), |error| <= 2^-33 of the term's unit
IS3D_BINS_HD long long sampler_vn_fixed(double term) { return llrint(term * IS3D_SAMPLER_VN_SCALE); }

#if defined(__HIP__) || defined(__HIPCC__)
// The adds of one particle with bins k and species s into the block h (layout l; the workgroup's LDS copy or the global block): five counts
// and, in a dN_pT bin, the 14 fixed-point harmonic terms -- 64-bit integer atomics.  THE add sequence of cf_sampler_bins, cf_sampler_fused
// and cf_decay_mc_bins.
__device__ __forceinline__ void sampler_bin_add(const is3d_sampler_test_bins &b, const SamplerHistLayout &l, int n_species, const SamplerBinIndex &k,
                                                int64_t s, unsigned long long *h)
{
    if (k.iyp >= 0) atomicAdd(&h[l.dy + s * b.y_bins + k.iyp], 1ULL);
    if (k.ieta >= 0) atomicAdd(&h[l.de + s * b.eta_bins + k.ieta], 1ULL);
    if (k.itau >= 0) atomicAdd(&h[l.dt + s * b.tau_bins + k.itau], 1ULL);
    if (k.ir >= 0) atomicAdd(&h[l.dr + s * b.r_bins + k.ir], 1ULL);
    if (k.ipT >= 0) {
        const int64_t j = s * b.pT_bins + k.ipT, plane = (int64_t)n_species * b.pT_bins;
        atomicAdd(&h[l.dp + j], 1ULL);
        for (int m = 0; m < IS3D_SAMPLER_VN_HARMONICS; m++) {
            double sn, cs;
            sincos(((double)m + 1.0) * k.phi, &sn, &cs);
            atomicAdd(&h[l.vr + m * plane + j], (unsigned long long)sampler_vn_fixed(cs));   // two's complement: signed sums
            atomicAdd(&h[l.vi + m * plane + j], (unsigned long long)sampler_vn_fixed(sn));
        }
    }
}

// the device side (cf_sampler_bins.hip): one batch of n particles (a DEVICE list, ordered by event as the sampler fills it) added into
// hist_dev (layout l) and yield_dev (n_events) on the null stream.  form: 0 = the measured choice (workgroup-private histograms where
// they fit the LDS, global atomics otherwise), 1 = global atomics, 2 = workgroup-private (needs sampler_bins_lds_fits).
bool sampler_bins_lds_fits(const SamplerHistLayout &l);
hipError_t sampler_bins_launch(const is3d_sampler_test_bins &b, const SamplerBinWidths &w, const SamplerHistLayout &l, int n_species, int n_events,
                               const is3d_particle *particles_dev, int64_t n, unsigned long long *hist_dev, unsigned long long *yield_dev,
                               int form);
#endif

}  // namespace is3d
