// cf_polzn.h -- launch entry points of cf_polzn.hip (spin polarization from thermal vorticity, mode 5).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
namespace is3d {

// per-chunk stage: lanes <-> (class, pT) with npTp (a power of two <= 64) lane slots per class; the workgroup's tile of JT phi x KT y bins
// (2+1D: JT phi, every eta node summed), the loop over the chunk's cells wave-uniform.  slab[((chunk * 5 + mu) * NB + bin) * (nlw * 64) + lane],
// bin = iphi + n_phi * iy, mu = t, x, y, n (without the -1 / (4 m) of the class), norm.
struct PolznArgs {
    const double *tau, *eta, *ux, *uy, *un, *dat, *dax, *day, *dan;
    const double *wtx, *wty, *wtn, *wxy, *wxn, *wyn;
    int32_t n_cells, nch, nlw, ntj, ntk, J, K;   // K: y nodes (3+1D) | eta nodes (2+1D)
    double invT;
    const double *lane_mT, *lane_pT, *lane_sign;  // [nlw * 64]
    const double *cphi, *sphi;                    // [ntj * JT], clamped copies past J
    const double *ka, *kb, *kw;                   // 3+1D: e^y, e^-y [ntk * KT] clamped; 2+1D: cosh(eta_k), -sinh(eta_k), eta_w[k] deta [K]
    double *slab;
    int64_t NB;                                   // n_phi * n_y_eff
};
constexpr int kPolznJT3 = 4, kPolznKT3 = 3, kPolznJT2 = 8;
hipError_t launch_polzn_cells(const PolznArgs &a, int three_d, hipStream_t st);
// out_mu[i] = scale_mu(s) * sum over the nch chunks, in chunk order, of slab[chunk][mu][bin][cls(s) * npTp + ipT], i = s + S (ipT + npT bin);
// scale = -1 / (4 m_s) for t, x, y, n and 1 for norm
hipError_t launch_polzn_reduce(const double *slab, int nch, int64_t NB, int64_t Lp, const int32_t *cls, const double *scale, int S, int npT,
                               int npTp, double *St, double *Sx, double *Sy, double *Sn, double *Snorm, hipStream_t st);
}  // namespace is3d
