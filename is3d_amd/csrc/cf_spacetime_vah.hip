// cf_spacetime_vah.hip -- the per-cell kernel of operation 0 for anisotropic hydro (mode 2, P_L matching).
//
// The reference has no such routine (its calculate_dN_dX knows viscous hydro only); the definition is include/is3d_amd.h: the integrand,
// options and domain rule of the VAH spectra (cf_vah.hip), reduced along the MOMENTUM axis of every cell as cf_spacetime.hip does for
// df_mode 1 / 2.  No outflow cut and no skipped cells: a cell with u.dsigma <= 0 contributes its negative value.  Stages:
//   cf_vah_coeffs, cf_prep_vah   (cf_vah.hip, unchanged) the per-cell "F" unit records of the default variant -- the records the spectra kernel
//                                cf_main_vah3 reads.  They carry no surface-wide scale: D of a cell depends on that cell alone.
//   cf_st_vah_cells              lanes <-> (species class, pT), loop over cells: every lane sums w_phi p.dsigma f over (phi, y | eta) of one cell,
//                                times w_pT, and a fixed xor tree over the pT lanes of a class gives D[class][cell].  2+1D: the same tree per eta
//                                node feeds the class's dN/dy deta partials, kept per workgroup (one lane per class owns its row), reduced in
//                                chunk order by cf_st_eta_reduce.
//   keys, sort, segment sums     cf_spacetime.hip (spacetime_bins_begin / spacetime_bins_add), shared with the viscous-hydro plans.
// No floating-point atomics anywhere: the results are bitwise the same from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cf_math.h"
#include "cf_spacetime.h"

namespace is3d {

// ------------------------------------------------------------------------------------------------
// cf_st_vah_cells.  "F" unit record (cf_prep_vah): header jj < JT {B_j, d_j, gd_j, x}, x of jj = 0, 1, 2 = min_k c_k, min_k e_k over the unit's
// rows and max_j d_j over its phi tile; rows r < R {A_k, c_k, ad_k, e_k [, W_k, 0], bd_jk...}.  For a lane (mT, pT, sign), the arithmetic of
// cf_main_vah3:
//   t = mT c_k - pT d_j;   X = E_a / Lambda = sqrt(t^2 + mT^2 e_k);   z = exp(-X);   fbar = 1 / (1 + sign z)
//   df / (f_a fbar_a) = mT^2 ad_k + mT pT bd_jk + pT^2 gd_j;   f = z fbar (1 + fbar df)   (regulate_deltaf: 1 + fbar df clamped to [0, 2])
//   p.dsigma = pT B_j (W_k) + mT A_k
// Phi entries past J (the last tile's clamped copies) carry w_phi = 0.  Rows past K: in 2+1D cf_prep_vah writes A = W = 0 there (p.dsigma = 0,
// the row adds +-0); in 3+1D W = 1 is not stored and only A is zeroed, so the row loop stops at the y grid's last row.
// The row test is the exact-zero rule of cf_main_vah3 (a lower bound of X^2 above 555400 for the whole wave: exp(-X) == +0, every term of the
// row is +-0 and the sums, which start at +0, keep their bits): zero_skip on or off gives the same D bit for bit.
// ------------------------------------------------------------------------------------------------
template <bool DIM3, bool REG, int JT, int R>
__global__ void __launch_bounds__(256) cf_st_vah_cells(const StVahCellArgs a)
{
    constexpr int HDR = 4 * JT;
    constexpr int RS = DIM3 ? 4 : 6;
    constexpr int RW = RS + JT;
    constexpr int REC = HDR + R * RW;
    constexpr double X2CUT = 555400.0;   // E_a/Lambda > 745.25: exp(-E_a/Lambda) == +0
    static_assert(JT == 8, "one rcp_batch<8> per row of the phi tile; the cull bounds sit in header slots jj = 0, 1, 2");
    extern __shared__ double st_vah_eta[];   // 2+1D: [4 waves][64 / npTp classes][K], each row owned by the head lane of its class

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = blockIdx.x % a.G, chunk = blockIdx.x / a.G;
    const int lw = grp * 4 + wave;
    if (lw >= a.nlw) return;   // no barrier below
    const int l = lw * 64 + lane;
    const double mT = a.lane_mT[l], pT = a.lane_pT[l], sign = a.lane_sign[l], wpT = a.lane_wpT[l];
    const double mT2 = mT * mT;
    const double hs = REG ? 0.5 : 1.0;   // u = (1 + fbar df) * hs, clamped to [0, 1] by the VOP3 clamp modifier when REG
    const double mT2s = hs * mT2, mTpTs = hs * (mT * pT), pT2s = hs * (pT * pT);
    const double unscale = REG ? 2.0 : 1.0;
    const int npTp = a.npTp, K = a.K;
    const int cls = l / npTp, ci = lane / npTp;
    const bool head = (lane & (npTp - 1)) == 0 && cls < a.ncls;
    const int c0 = (int)(((int64_t)chunk * a.nc) / a.nch), c1 = (int)(((int64_t)(chunk + 1) * a.nc) / a.nch);
    double *eta_row = st_vah_eta + ((size_t)wave * (64 / npTp) + ci) * K;
    if (!DIM3 && head)
        for (int k = 0; k < K; k++) eta_row[k] = 0.0;

    for (int c = c0; c < c1; c++) {
        double tot = 0.0;
        for (int jt = 0; jt < a.jtiles; jt++) {
            double accj[JT];
#pragma unroll
            for (int jj = 0; jj < JT; jj++) accj[jj] = 0.0;
            double wph[JT];
#pragma unroll
            for (int jj = 0; jj < JT; jj++) wph[jj] = a.wphi[jt * JT + jj];
            for (int rb = 0; rb < a.rblocks; rb++) {
                const double *__restrict__ U = a.TS + (DIM3 ? ((int64_t)(jt * a.rblocks + rb) * a.nc + c) * REC
                                                            : (((int64_t)jt * a.nc + c) * a.rblocks + rb) * REC);
                const double pTdmax = pT * U[11];
                if (a.zskip) {   // unit-level test: every row of the unit would fail its own test below
                    const double lbu = __builtin_fmax(__builtin_fma(mT, U[3], -pTdmax), 0.0);
                    if (__all(__builtin_fma(lbu, lbu, mT2 * U[7]) > X2CUT)) continue;
                }
                double pTB[JT], pTd[JT], gd[JT];
#pragma unroll
                for (int jj = 0; jj < JT; jj++) {
                    pTB[jj] = pT * U[4 * jj + 0];
                    pTd[jj] = pT * U[4 * jj + 1];
                    gd[jj] = pT2s * U[4 * jj + 2];
                }
                const double *__restrict__ rows = U + HDR;
                for (int r = 0; r < R; r++) {
                    if (DIM3 && rb * R + r >= K) break;   // padding rows: W is not stored in 3+1D, pT B_j f of row K - 1 would be added
                    const double *__restrict__ row = rows + r * RW;
                    const double mTc = mT * row[1], mT2e = mT2 * row[3];
                    if (a.zskip) {
                        const double lb = __builtin_fmax(mTc - pTdmax, 0.0);
                        if (__all(__builtin_fma(lb, lb, mT2e) > X2CUT)) continue;
                    }
                    const double mTA = mT * row[0], ad = mT2s * row[2];
                    double zz[JT], d[JT], inv[JT];
#pragma unroll
                    for (int jj = 0; jj < JT; jj++) {
                        const double t = mTc - pTd[jj];                          // p.u / Lambda
                        const double X = sqrt_g1(__builtin_fma(t, t, mT2e));     // E_a / Lambda
                        zz[jj] = exp_p9(-X);
                        d[jj] = __builtin_fma(sign, zz[jj], 1.0);
                    }
                    rcp_batch<JT>(d, inv);                                       // fbar_a
                    double rv = 0.0;
#pragma unroll
                    for (int jj = 0; jj < JT; jj++) {
                        const double rr = inv[jj];
                        const double br = __builtin_fma(mTpTs, row[RS + jj], ad + gd[jj]);   // hs * df/(f_a fbar_a)
                        const double u = REG ? fma_clamp01_half(rr, br) : __builtin_fma(rr, br, 1.0);
                        const double pds = DIM3 ? pTB[jj] + mTA : __builtin_fma(pTB[jj], row[4], mTA);   // W_k = 1 in 3+1D
                        const double v = pds * ((zz[jj] * rr) * u);
                        if (DIM3) accj[jj] += v;
                        else rv = __builtin_fma(wph[jj], v, rv);
                    }
                    if (!DIM3) {
                        // this eta node's share of the class: w_pT-weighted, summed over the class's pT lanes by a fixed xor tree
                        tot += rv;
                        double e = wpT * rv;
                        for (int o = npTp >> 1; o > 0; o >>= 1) e += __shfl_xor(e, o);
                        const int k = rb * R + r;
                        if (head && k < K) eta_row[k] += e;
                    }
                }
            }
            if (DIM3) {
#pragma unroll
                for (int jj = 0; jj < JT; jj++) tot = __builtin_fma(wph[jj], accj[jj], tot);
            }
        }
        double v = wpT * tot;
        for (int o = npTp >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (head) a.D[(int64_t)cls * a.nc + c] = v * unscale;
    }
    if (!DIM3 && head) {
        double *__restrict__ dst = a.eta_slab + ((int64_t)chunk * a.ncls + cls) * K;
        for (int k = 0; k < K; k++) dst[k] = eta_row[k] * unscale;
    }
}

bool spacetime_vah_shape_supported(int dim3, int JT, int R) { return dim3 ? (JT == 8 && R == 7) : (JT == 8 && R == 31); }

template <bool DIM3, int JT, int R>
static hipError_t launch_vah_cells_t(const StVahCellArgs &a, int regulate, hipStream_t st)
{
    const size_t lds = DIM3 ? 0 : sizeof(double) * 4 * (64 / a.npTp) * (size_t)a.K;
    if (regulate) hipLaunchKernelGGL((cf_st_vah_cells<DIM3, true, JT, R>), dim3((unsigned)(a.G * a.nch)), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((cf_st_vah_cells<DIM3, false, JT, R>), dim3((unsigned)(a.G * a.nch)), dim3(256), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_spacetime_vah_cells(const StVahCellArgs &a, int dim3, int regulate, int JT, int R, hipStream_t st)
{
    if (a.nc <= 0) return hipSuccess;
    if (!spacetime_vah_shape_supported(dim3, JT, R)) return hipErrorInvalidValue;
    return dim3 ? launch_vah_cells_t<true, 8, 7>(a, regulate, st) : launch_vah_cells_t<false, 8, 31>(a, regulate, st);
}

}  // namespace is3d
