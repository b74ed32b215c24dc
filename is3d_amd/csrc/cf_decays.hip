// cf_decays.hip -- resonance decay feed-down on the device: what EmissionFunctionArray::do_resonance_decays
// (src/cpp/emissionfunction_resonance_decays.cpp:124-2158) computes if its exit(-1) at entry (:128-129) is taken away, with the
// divergences of DESIGN.md section 3h.
//
// Parents are the unstable chosen species, chosen-list order from the last to index 1 (:143).  For each parent, in one stream:
//   cf_decay_tables  (one workgroup): log dN of the parent's row as it stands now -- it already holds the feed-down of every parent
//                    before it in the schedule (:157-174) --, per (y, phi) row and per parent mass of its channels the least-squares
//                    fit log dN = c + s M_T (estimate_MT_function_of_dNdypTdpTdphi, :2032-2158), and the M_T switch index: the minimum
//                    over rows of the last pT index before the row's first non-finite log (divergence 2).
//   cf_decay_feed    one wave per (daughter row, bin): the (v, zeta) [x s] quadrature of every channel of the parent that feeds that
//                    daughter, 144 or 1728 points spread over the lanes and summed by a fixed butterfly read at lane 0, added to the bin in
//                    channel order (dN += prefactor * integral, as the reference's sequence of per-channel updates).  One writer per output
//                    and parent, no floating-point atomics: two executions agree bit for bit.
// Species-level setup (schedule, groups, adjusted masses, E*, p*, Q, the s-node tables, M_T nodes per parent mass) is host work at
// plan creation; none of it depends on the spectrum.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_host.h"
#include "errors.h"

namespace {

constexpr int kGauss = 12;
// the reference's 12-point Gauss-Legendre table for v, zeta and s (:467-471, tabulated to 14 significant digits there; kept as tabulated)
__constant__ double c_root[kGauss] = {-0.98156063424672, -0.90411725637048, -0.76990267419431, -0.58731795428662, -0.3678314989982,
                                      -0.12523340851147, 0.12523340851147,  0.36783149899818,  0.58731795428662,  0.76990267419431,
                                      0.90411725637048,  0.98156063424672};
__constant__ double c_weight[kGauss] = {0.04717533638651, 0.1069393259953, 0.16007832854335, 0.20316742672307, 0.23349253653836,
                                        0.2491470458134,  0.2491470458134, 0.23349253653836, 0.20316742672307, 0.1600783285433,
                                        0.10693932599532, 0.04717533638651};
__constant__ double c_coszeta[kGauss];   // cos((pi / 2)(1 + x_k)), formed on the host with the same expression as the reference (:481)

const double h_root[kGauss] = {-0.98156063424672, -0.90411725637048, -0.76990267419431, -0.58731795428662, -0.3678314989982,
                               -0.12523340851147, 0.12523340851147,  0.36783149899818,  0.58731795428662,  0.76990267419431,
                               0.90411725637048,  0.98156063424672};
const double h_weight[kGauss] = {0.04717533638651, 0.1069393259953, 0.16007832854335, 0.20316742672307, 0.23349253653836,
                                 0.2491470458134,  0.2491470458134, 0.23349253653836, 0.20316742672307, 0.1600783285433,
                                 0.10693932599532, 0.04717533638651};

// one channel group feeding one daughter row: 2-body (E[0], p[0]) or 3-body (12 s nodes)
struct Contrib {
    int32_t kind, slot;                  // 2 | 3; parent-mass slot (M_T nodes and fit)
    double pref, M, m2;                  // prefactor, parent mass (adjusted in 2-body), daughter mass^2 (adjusted in 2-body)
    double E[kGauss], p[kGauss], w[kGauss];   // E*, p*, s weight (3-body: w_k sqrt|(s - s-)(s - d)| / s; 2-body: w[0] = 1)
};
struct Target {
    int32_t d, c0, nc, pad;              // daughter chosen index, contributions [c0, c0 + nc) in channel order
};

struct DecayArgs {
    double *dN;
    const double *pT, *phi, *y, *mt;     // mt: [slot][npT + 1], the M_T nodes of the slot's parent mass, then sqrt(2.73) M
    const Contrib *con;
    const Target *tgt;
    double *logtab, *fit;                // [nrows][npT]; [slot - slot0][nrows][2]
    int32_t *kswitch, *err;              // err: {code, parent schedule index, row}
    unsigned long long *clamps;
    int32_t S, npT, nphi, ny, nrows, dim3;
    int32_t p, sched, slot0, nslot, t0, nt;
};

// ---- per parent: log table, fits, switch index --------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cf_decay_tables(const DecayArgs a)
{
    if (a.err[0]) return;   // an earlier parent failed: the run stops there
    __shared__ int s_stop, s_bad;
    if (threadIdx.x == 0) { s_stop = a.npT; s_bad = INT32_MAX; }
    __syncthreads();
    for (int row = threadIdx.x; row < a.nrows; row += blockDim.x) {
        int stop = a.npT;
        for (int i = 0; i < a.npT; i++) {
            const double l = log(a.dN[a.p + (int64_t)a.S * (i + (int64_t)a.npT * row)]);
            a.logtab[(int64_t)row * a.npT + i] = l;
            if (stop == a.npT && !isfinite(l)) stop = i;
        }
        atomicMin(&s_stop, stop);
        for (int k = 0; k < a.nslot; k++) {
            const double *mt = a.mt + (int64_t)(a.slot0 + k) * (a.npT + 1);
            double n = 0.0, sx = 0.0, sxx = 0.0, sy = 0.0, sxy = 0.0;
            const double thr = mt[a.npT];   // slot row holds npT M_T nodes, then sqrt(2.73) M
            for (int i = 0; i < stop; i++) {
                const double m = mt[i];
                if (m > thr) {
                    const double l = a.logtab[(int64_t)row * a.npT + i];
                    n += 1.0; sx += m; sxx += m * m; sy += l; sxy += m * l;
                }
            }
            double c = 0.0, s = 0.0;
            if (n < 2.0) {
                atomicMin(&s_bad, row);
            } else {
                // normal equations [[n, sx], [sx, sxx]] (c, s) = (sy, sxy), Gaussian elimination with partial pivoting
                double a00 = n, a01 = sx, b0 = sy, a10 = sx, a11 = sxx, b1 = sxy;
                if (fabs(a10) > fabs(a00)) { double t; t = a00; a00 = a10; a10 = t; t = a01; a01 = a11; a11 = t; t = b0; b0 = b1; b1 = t; }
                const double f = a10 / a00;
                s = (b1 - f * b0) / (a11 - f * a01);
                c = (b0 - a01 * s) / a00;
            }
            a.fit[((int64_t)k * a.nrows + row) * 2 + 0] = c;
            a.fit[((int64_t)k * a.nrows + row) * 2 + 1] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.kswitch[0] = s_stop - 1;
        if (s_bad != INT32_MAX) { a.err[1] = a.sched; a.err[2] = s_bad; a.err[0] = IS3D_EDOMAIN; }
    }
}

// ---- the interpolated parent distribution exp(log dN) at (M_T, Phi, Y) (dN_dYMTdMTdPhi_boost_invariant / _non_boost_invariant) -------
struct Interp {
    const double *phi, *y, *mt, *L, *fit;
    int npT, nphi, ny, nrows, dim3;
    double MTsw, phimin, phimax;
};

__device__ inline void phi_bracket(const Interp &q, double &P, int &iL, int &iR, double &PL, double &PR)
{
    const double two_pi = 2.0 * M_PI;
    if (P >= q.phimin && P <= q.phimax) {
        iR = 1;
        while (iR < q.nphi - 1 && P > q.phi[iR]) iR++;
        iL = iR - 1;
        PL = q.phi[iL];
        PR = q.phi[iR];
    } else {
        iL = q.nphi - 1;
        iR = 0;
        PL = q.phi[iL] - two_pi;
        PR = q.phi[iR];
        P -= floor(P / M_PI) * two_pi;
    }
}

// one of the two parent azimuths: log dN by (tri/bi)linear interpolation below the switch, the M_T fit above it
__device__ inline double log_parent(const Interp &q, double MT, double P, int iYL, int iYR, double YL, double YR, double Y)
{
    int iL, iR;
    double PL, PR;
    phi_bracket(q, P, iL, iR, PL, PR);
    const double dP = PR - PL;
    if (MT <= q.MTsw) {
        int iMR = 1;
        while (iMR < q.npT - 1 && MT > q.mt[iMR]) iMR++;
        const int iML = iMR - 1;
        const double MTL = q.mt[iML], MTR = q.mt[iMR], dMT = MTR - MTL;
        if (!q.dim3) {
            const double LL = q.L[iML + q.npT * iL], RL = q.L[iML + q.npT * iR];
            const double LR = q.L[iMR + q.npT * iL], RR = q.L[iMR + q.npT * iR];
            return ((LL * (PR - P) + RL * (P - PL)) * (MTR - MT) + (LR * (PR - P) + RR * (P - PL)) * (MT - MTL)) / (dP * dMT);
        }
        auto at = [&](int iM, int iphi, int iy) { return q.L[iM + q.npT * (iphi + q.nphi * iy)]; };
        const double LLL = at(iML, iL, iYL), RLL = at(iML, iL, iYR), LRL = at(iML, iR, iYL), RRL = at(iML, iR, iYR);
        const double LLR = at(iMR, iL, iYL), RLR = at(iMR, iL, iYR), LRR = at(iMR, iR, iYL), RRR = at(iMR, iR, iYR);
        double v = (MTR - MT) * ((LLL * (YR - Y) + RLL * (Y - YL)) * (PR - P) + (LRL * (YR - Y) + RRL * (Y - YL)) * (P - PL))
                   + (MT - MTL) * ((LLR * (YR - Y) + RLR * (Y - YL)) * (PR - P) + (LRR * (YR - Y) + RRR * (Y - YL)) * (P - PL));
        return v / ((YR - YL) * dP * dMT);
    }
    auto lf = [&](int iy, int iphi) {
        const double *f = q.fit + 2 * (iphi + (int64_t)q.nphi * iy);
        return f[0] + f[1] * MT;
    };
    if (!q.dim3) return (lf(0, iL) * (PR - P) + lf(0, iR) * (P - PL)) / dP;
    const double LL = lf(iYL, iL), RL = lf(iYR, iL), LR = lf(iYL, iR), RR = lf(iYR, iR);
    const double v = (LL * (YR - Y) + RL * (Y - YL)) * (PR - P) + (LR * (YR - Y) + RR * (Y - YL)) * (P - PL);
    return v / ((YR - YL) * dP);
}

// ---- per parent: the feed-down into every daughter row --------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cf_decay_feed(const DecayArgs a)
{
    if (a.err[0]) return;
    const int lane = threadIdx.x & 63;
    const int64_t nbins = (int64_t)a.npT * a.nrows;
    const int64_t wid = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wid >= nbins * a.nt) return;   // wave-uniform
    const Target t = a.tgt[a.t0 + wid / nbins];
    const int64_t bin = wid % nbins;
    const int ipT = (int)(bin % a.npT), row = (int)(bin / a.npT);
    const int iphi = row % a.nphi, iy = row / a.nphi;
    const double pT = a.pT[ipT], pT2 = pT * pT, phip = a.phi[iphi], y = a.dim3 ? a.y[iy] : 0.0;
    const double two_pi = 2.0 * M_PI;
    const double Ymax = a.dim3 ? fabs(a.y[a.ny - 1]) : 0.0;
    const int kswitch = max(a.kswitch[0], 0);   // >= 1 whenever every fit had its 2 points (else err is set and this kernel returned)
    const int64_t out = t.d + (int64_t)a.S * bin;
    double acc = a.dN[out];
    unsigned clamps = 0;
    for (int ic = 0; ic < t.nc; ic++) {
        const Contrib &c = a.con[t.c0 + ic];
        Interp q;
        q.phi = a.phi; q.y = a.y; q.mt = a.mt + (int64_t)c.slot * (a.npT + 1); q.L = a.logtab;
        q.fit = a.fit + (int64_t)(c.slot - a.slot0) * a.nrows * 2;
        q.npT = a.npT; q.nphi = a.nphi; q.ny = a.ny; q.nrows = a.nrows; q.dim3 = a.dim3;
        q.MTsw = q.mt[kswitch]; q.phimin = a.phi[0]; q.phimax = a.phi[a.nphi - 1];
        const double M = c.M, M2 = M * M, mT2 = pT2 + c.m2, mT = sqrt(mT2);
        const int np = c.kind == 2 ? kGauss * kGauss : kGauss * kGauss * kGauss;
        double part = 0.0;
        for (int pt = lane; pt < np; pt += 64) {
            const int is = pt / (kGauss * kGauss), iv = (pt / kGauss) % kGauss, iz = pt % kGauss;
            const double Estar = c.E[is], pstar = c.p[is];
            const double DeltaY = log((pstar + sqrt(Estar * Estar + pT2)) / mT);
            const double v = c_root[iv];
            const double coshv = cosh(v * DeltaY);
            const double mT2c2 = mT2 * coshv * coshv;
            const double den = mT2c2 - pT2;
            const double MTbar = Estar * M * mT * coshv / den;
            const double DeltaMT = M * pT * sqrt(fabs(Estar * Estar + pT2 - mT2c2)) / den;
            const double vw = DeltaY * c_weight[iv] / sqrt(fabs(den));
            int iYL = 0, iYR = 0;
            double YL = 0.0, YR = 0.0, Y = 0.0;
            if (a.dim3) {
                Y = y + v * DeltaY;
                if (!(fabs(Y) <= Ymax)) continue;   // parent distribution cut off in Y (:720-744): the point adds 0
                iYR = 1;
                while (iYR < a.ny - 1 && Y > a.y[iYR]) iYR++;
                iYL = iYR - 1;
                YL = a.y[iYL];
                YR = a.y[iYR];
            }
            const double MT = MTbar + DeltaMT * c_coszeta[iz];
            const double PT = sqrt(MT * MT - M2);
            double cphi = (MT * (mT * coshv / pT) - Estar * M / pT) / PT;
            if (cphi > 1.0) { cphi = 1.0; clamps++; }            // divergence 4: in [-1, 1] in exact arithmetic
            else if (cphi < -1.0) { cphi = -1.0; clamps++; }
            const double Pt = acos(cphi);
            double P1 = fmod(Pt + phip, two_pi), P2 = fmod(-Pt + phip, two_pi);
            if (P1 < 0.0) P1 += two_pi;
            if (P2 < 0.0) P2 += two_pi;
            const double f = exp(log_parent(q, MT, P1, iYL, iYR, YL, YR, Y)) + exp(log_parent(q, MT, P2, iYL, iYR, YL, YR, Y));
            part += c.w[is] * vw * (c_weight[iz] * (MT * f));
        }
        // fixed butterfly; lane 0's sum (its association order is fixed) is the integral
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
        part = __shfl(part, 0, 64);
        acc += c.pref * part;
    }
    for (int off = 32; off > 0; off >>= 1) clamps += __shfl_xor(clamps, off, 64);
    if (lane == 0) {
        a.dN[out] = acc;
        if (clamps) atomicAdd(a.clamps, (unsigned long long)clamps);
    }
}

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
using namespace is3d;

namespace {
struct Sched {
    int32_t p, entry, slot0, nslot, t0, nt;
};
}  // namespace

struct is3d_decay_plan {
    int device = 0, dim3 = 1, S = 0, npT = 0, nphi = 0, ny = 1, nrows = 0, max_slot = 1;
    int32_t n_parents = 0, n_channels = 0, n_adjusted = 0;
    int64_t nout = 0, n_points = 0;
    std::vector<Sched> sched;
    std::vector<int64_t> parent_id;      // mc_id per schedule entry
    std::vector<double> y_host;
    DevBuf<double> pT, phi, y, mt, logtab, fit;
    DevBuf<Contrib> con;
    DevBuf<Target> tgt;
    DevBuf<int32_t> flags;               // kswitch, err[3]
    DevBuf<unsigned long long> clamps;
    std::vector<hipEvent_t> ev;
    ~is3d_decay_plan()
    {
        (void)hipSetDevice(device);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

int check_grid(const is3d_grid *g, int dim3)
{
    if (!g || !g->pT || !g->phi) return set_error(IS3D_EINVAL, "the pT and phi grids are required");
    if (g->n_pT < 2 || g->n_phi < 2) return set_error(IS3D_EINVAL, "resonance decays interpolate in pT and phi: at least 2 nodes each (%d, %d given)", g->n_pT, g->n_phi);
    for (int i = 0; i < g->n_pT; i++)
        if (!(g->pT[i] > 0.0) || (i && !(g->pT[i] > g->pT[i - 1])))
            return set_error(IS3D_EDOMAIN, "the pT grid must be positive and ascending (node %d = %g)", i, g->pT[i]);
    for (int i = 1; i < g->n_phi; i++)
        if (!(g->phi[i] > g->phi[i - 1])) return set_error(IS3D_EDOMAIN, "the phi grid must ascend (node %d = %g)", i, g->phi[i]);
    if (dim3) {
        if (g->n_y < 2 || !g->y) return set_error(IS3D_EINVAL, "3+1D resonance decays interpolate in y: at least 2 nodes (%d given)", g->n_y);
        for (int i = 1; i < g->n_y; i++)
            if (!(g->y[i] > g->y[i - 1])) return set_error(IS3D_EDOMAIN, "the y grid must ascend (node %d = %g)", i, g->y[i]);
        if (!(g->y[g->n_y - 1] > 0.0)) return set_error(IS3D_EDOMAIN, "the y grid must end above 0 (its last node is Y_max, :463)");
    }
    return IS3D_OK;
}

int check_table(const is3d_decay_table *t)
{
    if (!t || t->n < 1 || !t->mc_id || !t->mass || !t->width || !t->stable || !t->n_channels || !t->npart || !t->branch_ratio || !t->daughters)
        return set_error(IS3D_EINVAL, "the decay table (is3d_pdg_read_decays) is required, with every array");
    return IS3D_OK;
}

// calculate_Q_factor (:99-121): 24-point Gauss-Legendre, the reference's tabulated nodes
double q_factor(double M, double m1, double m2, double m3)
{
    static const double xr[24] = {-0.99518721999702, -0.97472855597131, -0.93827455200273, -0.8864155270044, -0.8200019859739, -0.74012419157855,
                                  -0.64809365193698, -0.54542147138884, -0.43379350762605, -0.31504267969616, -0.19111886747362, -0.064056892862606,
                                  0.06405689286261,  0.19111886747362,  0.31504267969616,  0.43379350762605,  0.54542147138884,  0.64809365193698,
                                  0.74012419157855,  0.8200019859739,   0.8864155270044,   0.93827455200273,  0.97472855597131,  0.99518721999702};
    static const double xw[24] = {0.01234122979999, 0.02853138862893, 0.0442774388174, 0.059298584915437, 0.0733464814111, 0.08619016153195,
                                  0.0976186521041,  0.107444270116,   0.11550566805373, 0.1216704729278,  0.12583745634683, 0.1279381953468,
                                  0.1279381953468,  0.1258374563468,  0.1216704729278,  0.1155056680537,  0.107444270116,   0.09761865210411,
                                  0.08619016153195, 0.07334648141108, 0.05929858491544, 0.04427743881742, 0.02853138862893, 0.01234122979999};
    const double a = (M + m1) * (M + m1), b = (M - m1) * (M - m1), c = (m2 + m3) * (m2 + m3), d = (m2 - m3) * (m2 - m3);
    double Q = 0.0;
    for (int i = 0; i < 24; i++) {
        const double s = c + (b - c) * (1.0 + xr[i]) / 2.0;
        Q += xw[i] * (b - c) * std::sqrt(std::fabs((a - s) * (b - s) * (s - c) * (s - d))) / (2.0 * s);
    }
    return Q;
}

}  // namespace

extern "C" double is3d_decay_q_factor(double mass_parent, double mass_1, double mass_2, double mass_3)
{
    return q_factor(mass_parent, mass_1, mass_2, mass_3);
}

extern "C" int is3d_decay_plan_create(is3d_decay_plan **plan, const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                                      const is3d_grid *grid, int32_t dimension, int32_t device)
{
    if (!plan) return set_error(IS3D_EINVAL, "plan is NULL");
    *plan = nullptr;
    if (dimension != 2 && dimension != 3) return set_error(IS3D_EINVAL, "dimension = %d: 2 or 3", dimension);
    const int dim3 = dimension == 3;
    if (int rc = check_table(table)) return rc;
    if (n_chosen < 2 || !chosen_mc_id)   // :133-137
        return set_error(IS3D_EINVAL, "need at least two chosen particles for the resonance decay routine (%d given)", n_chosen);
    if (int rc = check_grid(grid, dim3)) return rc;
    std::unique_ptr<is3d_decay_plan> P(new is3d_decay_plan);
    P->dim3 = dim3;
    P->S = n_chosen;
    P->npT = grid->n_pT;
    P->nphi = grid->n_phi;
    P->ny = dim3 ? grid->n_y : 1;
    P->nrows = P->nphi * P->ny;
    P->nout = (int64_t)P->S * P->npT * P->nrows;
    // ---- species-level setup (host) ----
    const is3d_decay_table &T = *table;
    std::vector<int64_t> ch0((size_t)T.n + 1, 0);
    for (int i = 0; i < T.n; i++) {
        if (T.n_channels[i] < 0 || T.n_channels[i] > 50) return set_error(IS3D_EINVAL, "entry %d has %d channels (0 .. 50)", i, T.n_channels[i]);
        ch0[(size_t)i + 1] = ch0[(size_t)i] + T.n_channels[i];
    }
    auto pdg_index = [&](int64_t id) {   // particle_index (:58-79): first match
        for (int i = 0; i < T.n; i++)
            if (T.mc_id[i] == id) return i;
        return -1;
    };
    std::vector<int> chosen_entry((size_t)n_chosen);
    for (int s = 0; s < n_chosen; s++) {
        chosen_entry[(size_t)s] = pdg_index(chosen_mc_id[s]);
        if (chosen_entry[(size_t)s] < 0) return set_error(IS3D_EINVAL, "chosen particle %lld is not in the decay table", (long long)chosen_mc_id[s]);
    }
    auto chosen_of = [&](int entry) {   // particle_chosen_index (:82-97): first match
        for (int s = 0; s < n_chosen; s++)
            if (chosen_entry[(size_t)s] == entry) return s;
        return -1;
    };
    std::vector<double> slot_mass;
    std::vector<Contrib> con;
    std::vector<Target> tgt;
    double cz[kGauss];
    for (int k = 0; k < kGauss; k++) cz[k] = std::cos((M_PI / 2.0) * (1.0 + h_root[k]));
    for (int ip = n_chosen - 1; ip > 0; ip--) {
        const int e = chosen_entry[(size_t)ip];
        if (T.stable[e]) continue;
        P->n_parents++;
        Sched sc{ip, e, (int32_t)slot_mass.size(), 0, (int32_t)tgt.size(), 0};
        // per daughter chosen index: its contributions in channel order
        std::vector<std::pair<int, Contrib>> items;
        for (int j = 0; j < T.n_channels[e]; j++) {
            const int64_t c = ch0[(size_t)e] + j;
            const int np = std::abs(T.npart[c]);
            if (np < 1 || np > 5) return set_error(IS3D_EINVAL, "parent %lld channel %d: %d decay products", (long long)T.mc_id[e], j, T.npart[c]);
            int dd[5];
            for (int k = 0; k < np; k++) {
                const int64_t id = T.daughters[c * 5 + k];
                if (id == 0) return set_error(IS3D_EINVAL, "parent %lld channel %d: daughter mc_id 0 (null particle)", (long long)T.mc_id[e], j);
                dd[k] = pdg_index(id);
                if (dd[k] < 0) return set_error(IS3D_EINVAL, "parent %lld channel %d: daughter %lld is not in the decay table", (long long)T.mc_id[e], j, (long long)id);
            }
            if (np == 1 || np == 4) continue;                 // :194, :282-285
            if (np == 5) return set_error(IS3D_EINVAL, "parent %lld channel %d: 5-body decays are not handled (the reference exits, :286-290)", (long long)T.mc_id[e], j);
            const double br = T.branch_ratio[c];
            double M = T.mass[e], m[3] = {T.mass[dd[0]], T.mass[dd[1]], np == 3 ? T.mass[dd[2]] : 0.0};
            bool adjusted = false;
            if (np == 2) {   // :243-258
                for (int it = 0; m[0] + m[1] > M; it++) {
                    if (it == 0) adjusted = true;
                    if (it > 100000) return set_error(IS3D_EINVAL, "parent %lld channel %d: the mass adjustment does not converge", (long long)T.mc_id[e], j);
                    M += 0.25 * T.width[e];
                    m[0] -= 0.5 * T.width[dd[0]];
                    m[1] -= 0.5 * T.width[dd[1]];
                    if (m[0] < 0.0 || m[1] < 0.0) return set_error(IS3D_EINVAL, "parent %lld channel %d: a daughter mass went negative in the mass adjustment", (long long)T.mc_id[e], j);
                }
            }
            // selected daughters in product order, grouped by type (:311-371)
            std::vector<int> gtype, gmult, gfirst;
            for (int k = 0; k < np; k++) {
                if (chosen_of(dd[k]) < 0) continue;
                auto it = std::find(gtype.begin(), gtype.end(), dd[k]);
                if (it == gtype.end()) { gtype.push_back(dd[k]); gmult.push_back(1); gfirst.push_back(k); }
                else gmult[(size_t)(it - gtype.begin())]++;
            }
            if (gtype.empty()) continue;
            P->n_channels++;
            if (adjusted) P->n_adjusted++;
            int slot = -1;
            for (int k = sc.slot0; k < (int)slot_mass.size(); k++)
                if (slot_mass[(size_t)k] == M) slot = k;
            if (slot < 0) { slot = (int)slot_mass.size(); slot_mass.push_back(M); }
            for (size_t g = 0; g < gtype.size(); g++) {
                Contrib q{};
                q.kind = np;
                q.slot = slot;
                q.M = M;
                const int k1 = gfirst[g];   // the group's particle: the first product of its type; the others, in product order, are the partners
                int rest[2], nr = 0;
                for (int k = 0; k < np; k++)
                    if (k != k1) rest[nr++] = k;
                const double mult = (double)gmult[g];
                if (np == 2) {
                    // divergence 3: W^2 from the partner (:410-412 take particle_2), adjusted masses throughout
                    const double mass = m[k1], W2 = m[rest[0]] * m[rest[0]];
                    const double Estar = (M * M + mass * mass - W2) / (2.0 * M);
                    q.m2 = mass * mass;
                    q.E[0] = Estar;
                    q.p[0] = std::sqrt(Estar * Estar - mass * mass);
                    q.w[0] = 1.0;
                    q.pref = mult * M * br / (8.0 * q.p[0]);
                } else {
                    const double m1 = m[k1], m2 = m[rest[0]], m3 = m[rest[1]];
                    const double sp = (M - m1) * (M - m1), sm = (m2 + m3) * (m2 + m3), d = (m2 - m3) * (m2 - m3);
                    const double Q = q_factor(M, m1, m2, m3);
                    q.m2 = m1 * m1;
                    for (int k = 0; k < kGauss; k++) {
                        const double s = sm + (sp - sm) * (1.0 + h_root[k]) / 2.0;
                        const double Estar = (M * M + m1 * m1 - s) / (2.0 * M);
                        q.E[k] = Estar;
                        q.w[k] = h_weight[k] * std::sqrt(std::fabs((s - sm) * (s - d))) / s;
                        q.p[k] = std::sqrt(Estar * Estar - m1 * m1);
                    }
                    q.pref = mult * (M * M) * (sp - sm) * br / (8.0 * Q);
                }
                items.emplace_back(chosen_of(gtype[g]), q);
            }
        }
        // targets: daughters in order of first appearance, each with its contributions in channel order
        std::vector<int> order;
        for (auto &it : items)
            if (std::find(order.begin(), order.end(), it.first) == order.end()) order.push_back(it.first);
        for (int d : order) {
            Target t{d, (int32_t)con.size(), 0, 0};
            for (auto &it : items)
                if (it.first == d) { con.push_back(it.second); t.nc++; }
            tgt.push_back(t);
            for (int k = t.c0; k < t.c0 + t.nc; k++)
                P->n_points += (int64_t)P->npT * P->nrows * (con[(size_t)k].kind == 2 ? kGauss * kGauss : kGauss * kGauss * kGauss);
        }
        sc.nslot = (int32_t)slot_mass.size() - sc.slot0;
        sc.nt = (int32_t)tgt.size() - sc.t0;
        P->max_slot = std::max(P->max_slot, sc.nslot);
        P->sched.push_back(sc);
        P->parent_id.push_back(T.mc_id[e]);
    }
    // M_T nodes per parent mass (:449-454), then sqrt(2.73) M, the fit's threshold (:2065)
    std::vector<double> mt(slot_mass.size() * (size_t)(P->npT + 1));
    for (size_t k = 0; k < slot_mass.size(); k++) {
        const double M = slot_mass[k];
        for (int i = 0; i < P->npT; i++) mt[k * (P->npT + 1) + i] = std::sqrt(std::fabs(grid->pT[i] * grid->pT[i] + M * M));
        mt[k * (P->npT + 1) + P->npT] = std::sqrt(2.73) * M;
    }
    // ---- device ----
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_error(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    count_resource(0);
    HIP_TRY(hipGetDevice(&P->device));
    HIP_TRY(P->pT.upload(grid->pT, (size_t)P->npT));
    HIP_TRY(P->phi.upload(grid->phi, (size_t)P->nphi));
    if (dim3) HIP_TRY(P->y.upload(grid->y, (size_t)P->ny));
    else HIP_TRY(P->y.upload(std::vector<double>{0.0}));
    if (!mt.empty()) HIP_TRY(P->mt.upload(mt));
    if (!con.empty()) HIP_TRY(P->con.upload(con));
    if (!tgt.empty()) HIP_TRY(P->tgt.upload(tgt));
    HIP_TRY(P->logtab.alloc((size_t)P->nrows * P->npT));
    HIP_TRY(P->fit.alloc((size_t)P->max_slot * P->nrows * 2));
    HIP_TRY(P->flags.alloc(4));
    HIP_TRY(P->clamps.alloc(1));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_coszeta), cz, sizeof cz));
    P->ev.assign(2 * P->sched.size() + 1, nullptr);
    for (hipEvent_t &ev : P->ev) HIP_TRY(hipEventCreate(&ev));
    *plan = P.release();
    return IS3D_OK;
}

extern "C" int64_t is3d_decay_plan_output_size(const is3d_decay_plan *P) { return P ? P->nout : -1; }

extern "C" int is3d_decay_plan_execute(is3d_decay_plan *P, double *dN, void *hip_stream, is3d_decay_stats *stats)
{
    if (!P) return set_error(IS3D_EINVAL, "plan is NULL");
    if (!dN) return set_error(IS3D_EINVAL, "the spectrum is required");
    HIP_TRY(hipSetDevice(P->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const bool timed = stats != nullptr;
    HIP_TRY(hipMemsetAsync(P->flags.p, 0, 4 * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(P->clamps.p, 0, sizeof(unsigned long long), st));
    DecayArgs a{};
    a.dN = dN; a.mt = P->mt.p; a.pT = P->pT.p; a.phi = P->phi.p; a.y = P->y.p; a.con = P->con.p; a.tgt = P->tgt.p;
    a.logtab = P->logtab.p; a.fit = P->fit.p; a.kswitch = P->flags.p; a.err = P->flags.p + 1; a.clamps = P->clamps.p;
    a.S = P->S; a.npT = P->npT; a.nphi = P->nphi; a.ny = P->ny; a.nrows = P->nrows; a.dim3 = P->dim3;
    if (timed) HIP_TRY(hipEventRecord(P->ev[0], st));
    int nev = 1;
    for (size_t i = 0; i < P->sched.size(); i++) {
        const Sched &s = P->sched[i];
        if (s.nt == 0) continue;
        a.p = s.p; a.sched = (int32_t)i; a.slot0 = s.slot0; a.nslot = s.nslot; a.t0 = s.t0; a.nt = s.nt;
        hipLaunchKernelGGL(cf_decay_tables, dim3(1), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
        if (timed) HIP_TRY(hipEventRecord(P->ev[nev++], st));
        const int64_t waves = (int64_t)s.nt * P->npT * P->nrows;
        hipLaunchKernelGGL(cf_decay_feed, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
        if (timed) HIP_TRY(hipEventRecord(P->ev[nev++], st));
    }
    int32_t flags[4];
    unsigned long long clamps = 0;
    HIP_TRY(hipMemcpyAsync(flags, P->flags.p, sizeof flags, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&clamps, P->clamps.p, sizeof clamps, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (flags[1]) {
        const int row = flags[3];
        return set_error(IS3D_EDOMAIN, "not enough points to construct a least squares fit: parent %lld, (y, phi) row iy = %d, iphi = %d "
                         "(fewer than 2 positive values above M_T = sqrt(2.73) M before the first non-positive one)",
                         (long long)P->parent_id[(size_t)flags[2]], row / P->nphi, row % P->nphi);
    }
    if (timed) {
        double mt = 0.0, mf = 0.0;
        for (int k = 1; k < nev; k++) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, P->ev[(size_t)k - 1], P->ev[(size_t)k]));
            (k & 1 ? mt : mf) += ms;
        }
        stats->code = IS3D_OK;
        stats->n_parents = P->n_parents;
        stats->n_channels = P->n_channels;
        stats->n_adjusted = P->n_adjusted;
        stats->n_clamps = (int64_t)clamps;
        stats->n_points = P->n_points;
        stats->ms_tables = mt;
        stats->ms_feed = mf;
    }
    return IS3D_OK;
}

extern "C" void is3d_decay_plan_destroy(is3d_decay_plan *P) { delete P; }

extern "C" int is3d_resonance_decays(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id, const is3d_grid *grid,
                                     int32_t dimension, int32_t device, double *dN_inout, is3d_decay_stats *stats)
{
    if (!dN_inout) return set_error(IS3D_EINVAL, "the spectrum is required");
    is3d_decay_plan *raw = nullptr;
    if (int rc = is3d_decay_plan_create(&raw, table, n_chosen, chosen_mc_id, grid, dimension, device)) return rc;
    std::unique_ptr<is3d_decay_plan> P(raw);
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<double> d;
    HIP_TRY(d.upload(dN_inout, (size_t)P->nout));
    const auto t1 = std::chrono::steady_clock::now();
    is3d_decay_stats ds{};
    if (int rc = is3d_decay_plan_execute(P.get(), d.p, nullptr, &ds)) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpy(dN_inout, d.p, sizeof(double) * (size_t)P->nout, hipMemcpyDeviceToHost));
    const auto t3 = std::chrono::steady_clock::now();
    if (stats) {
        *stats = ds;
        stats->ms_h2d = std::chrono::duration<double, std::milli>(t1 - t0).count();
        stats->ms_d2h = std::chrono::duration<double, std::milli>(t3 - t2).count();
    }
    return IS3D_OK;
}
