// cf_spacetime.hip -- hand-written gfx950 kernels of operation 0: the smooth Cooper-Frye spacetime distributions.
//
// Replaces EmissionFunctionArray::calculate_dN_dX (reference src/cpp/emissionfunction_smooth_kernels.cpp:1000-1446) for df_mode 1, 2.
// The integrand is that of the spectra path; what differs is the reduction: along the MOMENTUM axis of every cell (dN_dy_cell, :1370), then
// over the cells of a (tau | r | tau x r) bin.  Stages ("Operation 0"):
//   cf_prep         (cf_kernels.hip, unchanged) the per-cell unit records of the plan's tile shape: skip / out-of-table neutralisation,
//                   spline or bilinear coefficients, the power-of-two p.dsigma scale -- the same records the spectra kernels read.
//   cf_st_cells     lanes <-> (species class, pT), loop over cells: every lane sums w_phi p.dsigma f over (phi, y | eta) of one cell, times
//                   w_pT, and a fixed xor tree over the pT lanes of a class gives D[class][cell].  2+1D: the same tree per eta node feeds
//                   the class's dN/dy deta partials, kept per workgroup (one lane per class owns its row), reduced in chunk order.
//   cf_st_keys / cf_st_sort_*   bin keys and a stable counting sort of the cells per histogram (ascending cell index inside a bin).
//   cf_st_segsum    lanes <-> species: bin[s][b] = left-to-right sum over the bin's cells of pg[s] * D[class(s)][c] (one rounding each),
//                   the reference's order of additions per bin.
// No floating-point atomics anywhere: the results are bitwise the same from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cf_math.h"
#include "cf_spacetime.h"

namespace is3d {

// 2^e with |p.dsigma| < 2^e over the execute (the records carry p.dsigma 2^-e; cf_kernels.hip::pds_scale)
__device__ __forceinline__ double st_unscale(const unsigned long long *bound_bits)
{
    int e = 0;
    if (bound_bits) {
        const double b = __longlong_as_double((long long)*bound_bits);
        if (b > 0.0) (void)frexp(b, &e);
    }
    return ldexp(1.0, e);
}

// ------------------------------------------------------------------------------------------------
// cf_st_cells.  Unit record (cf_device.h): header jj < JT {B_j, Dp_j, gamma_j, x | L2_j} [+ {alpha_B, Dmax}], rows r < R
// {A_k, Cp_k, alpha_k, W_k [, L_k, c], beta_jk...}.  For a lane (mT, pT, sign, b):
//   p.dsigma = mT A_k + W_k pT B_j;   x = p.u/T = mT Cp_k - pT Dp_j;   z = exp(-x + b alpha_B)
//   br = mT^2 alpha_k + mT pT beta_jk + pT^2 gamma_j [+ b (mT L_k + pT L2_j)]
//   14-moment: df = br / (1 + sign z);  Chapman-Enskog: df = br / ((1 + sign z) x);   f = z / (1 + sign z) (1 + df)
// Phi entries past J (the last tile's clamped copies) carry w_phi = 0; rows past K are neutral padding (A = W = 0) in 2+1D, where W enters
// p.dsigma; in 3+1D (W = 1, not read) the row loop stops at the y grid's last row.
// ------------------------------------------------------------------------------------------------
template <bool CE, bool DIM3, bool BARYON, int JT, int R>
__global__ void __launch_bounds__(256) cf_st_cells(const StCellArgs a)
{
    constexpr int HDR = 4 * JT + (BARYON ? 2 : 0);
    constexpr int RS = BARYON ? 6 : 4;
    constexpr int RW = RS + JT;
    constexpr int REC = HDR + R * RW;
    extern __shared__ double st_eta[];   // 2+1D: [4 waves][64 / npTp classes][K], each row owned by the head lane of its class

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = blockIdx.x % a.G, chunk = blockIdx.x / a.G;
    const int lw = grp * 4 + wave;
    if (lw >= a.nlw) return;   // no barrier below
    const int l = lw * 64 + lane;
    const double mT = a.lane_mT[l], pT = a.lane_pT[l], sign = a.lane_sign[l], wpT = a.lane_wpT[l];
    const double bq = BARYON ? a.lane_b[l] : 0.0;
    const double mT2 = mT * mT, mTpT = mT * pT, pT2 = pT * pT, bmT = bq * mT, bpT = bq * pT;
    const int npTp = a.npTp, K = a.K;
    const int cls = l / npTp, ci = lane / npTp;
    const bool head = (lane & (npTp - 1)) == 0 && cls < a.ncls;
    const double unscale = st_unscale(a.pds_bound);
    const double thr = a.zskip ? -745.2 : -1.0e300;   // exp(earg) == +0 below -745.2 for the whole wave: the row adds exactly +0
    const int c0 = (int)(((int64_t)chunk * a.nc) / a.nch), c1 = (int)(((int64_t)(chunk + 1) * a.nc) / a.nch);
    double *eta_row = st_eta + ((size_t)wave * (64 / npTp) + ci) * K;
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
                double pTB[JT], pTD[JT], pT2g[JT], E2[JT];
                double bmax = -1.0e300;
#pragma unroll
                for (int jj = 0; jj < JT; jj++) {
                    pTB[jj] = pT * U[4 * jj + 0];
                    pTD[jj] = pT * U[4 * jj + 1];
                    pT2g[jj] = pT2 * U[4 * jj + 2];
                    if (BARYON) pT2g[jj] = __builtin_fma(bpT, U[4 * jj + 3], pT2g[jj]);
                    bmax = __builtin_fmax(bmax, pTD[jj]);
                }
#pragma unroll
                for (int jj = 0; jj < JT; jj++) E2[jj] = exp_p9(pTD[jj] - bmax);
                const double baB = BARYON ? bq * U[4 * JT] : 0.0;
                const double *__restrict__ rows = U + HDR;
                for (int r = 0; r < R; r++) {
                    if (DIM3 && rb * R + r >= K) break;   // padding rows: W is not read in 3+1D, pT B_j f of row K - 1 would be added
                    const double *__restrict__ row = rows + r * RW;
                    const double mTC = mT * row[1];
                    const double earg = BARYON ? (bmax - mTC) + baB : bmax - mTC;
                    if (__all(earg < thr)) continue;
                    const double E1 = exp_p9(earg);
                    const double mTA = mT * row[0], W = row[3];
                    const double mT2a = BARYON ? __builtin_fma(bmT, row[4], mT2 * row[2]) : mT2 * row[2];
                    double rv = 0.0;
#pragma unroll
                    for (int jj = 0; jj < JT; jj++) {
                        const double z = E1 * E2[jj];
                        const double d = __builtin_fma(sign, z, 1.0);
                        double inv, rr;
                        if (CE) {
                            const double x = mTC - pTD[jj];
                            inv = rcp_nr(d * x);
                            rr = inv * x;
                        } else {
                            inv = rcp_nr(d);
                            rr = inv;
                        }
                        double pds = DIM3 ? mTA + pTB[jj] : __builtin_fma(pTB[jj], W, mTA);
                        if (a.outflow) pds = __builtin_fmax(pds, 0.0);
                        const double br = __builtin_fma(mTpT, row[RS + jj], mT2a + pT2g[jj]);
                        double df = inv * br;
                        if (a.regulate) df = __builtin_fmax(-1.0, __builtin_fmin(df, 1.0));
                        const double v = pds * ((z * rr) * (1.0 + df));
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

bool spacetime_shape_supported(int dim3, int JT, int R)
{
    return dim3 ? ((JT == 8 || JT == 6) && R == 7) : (JT == 8 && (R == 31 || R == 61));
}

template <bool CE, bool DIM3, bool BARYON, int JT, int R>
static hipError_t launch_cells_t(const StCellArgs &a, hipStream_t st)
{
    const size_t lds = DIM3 ? 0 : sizeof(double) * 4 * (64 / a.npTp) * (size_t)a.K;
    hipLaunchKernelGGL((cf_st_cells<CE, DIM3, BARYON, JT, R>), dim3((unsigned)(a.G * a.nch)), dim3(256), lds, st, a);
    return hipGetLastError();
}

template <bool CE, bool BARYON>
static hipError_t launch_cells_shape(const StCellArgs &a, int dim3, int JT, int R, hipStream_t st)
{
    if (dim3) return JT == 8 ? launch_cells_t<CE, true, BARYON, 8, 7>(a, st) : launch_cells_t<CE, true, BARYON, 6, 7>(a, st);
    return R == 31 ? launch_cells_t<CE, false, BARYON, 8, 31>(a, st) : launch_cells_t<CE, false, BARYON, 8, 61>(a, st);
}

hipError_t launch_spacetime_cells(const StCellArgs &a, int ce, int dim3, int baryon, int JT, int R, hipStream_t st)
{
    if (a.nc <= 0) return hipSuccess;
    if (!spacetime_shape_supported(dim3, JT, R)) return hipErrorInvalidValue;
    if (ce) return baryon ? launch_cells_shape<true, true>(a, dim3, JT, R, st) : launch_cells_shape<true, false>(a, dim3, JT, R, st);
    return baryon ? launch_cells_shape<false, true>(a, dim3, JT, R, st) : launch_cells_shape<false, false>(a, dim3, JT, R, st);
}

// ------------------------------------------------------------------------------------------------
// 2+1D dN/dy deta: chunk partials in chunk order, then the species' values
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
cf_st_eta_reduce(const double *__restrict__ slab, int nch, int64_t n_per_chunk, int first_pass, double *__restrict__ eta_cls)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_per_chunk) return;
    double s = first_pass ? 0.0 : eta_cls[i];
    for (int ch = 0; ch < nch; ch++) s += slab[ch * n_per_chunk + i];
    eta_cls[i] = s;
}

hipError_t launch_spacetime_eta_reduce(const double *eta_slab, int nch, int64_t n_per_chunk, int first_pass, double *eta_cls, hipStream_t st)
{
    if (n_per_chunk <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_st_eta_reduce, dim3((unsigned)((n_per_chunk + 255) / 256)), dim3(256), 0, st, eta_slab, nch, n_per_chunk, first_pass,
                       eta_cls);
    return hipGetLastError();
}

// the multi-device entry: eta_cls[i] = parts[0][i] + parts[1][i] + ... left to right over the shards' class rows (one lane per element, a
// fixed order for a given shard count; one part is copied bit for bit)
__global__ void __launch_bounds__(256)
cf_st_eta_shards(const double *__restrict__ parts, int nparts, int64_t n_per_part, double *__restrict__ eta_cls)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_per_part) return;
    double s = parts[i];
    for (int p = 1; p < nparts; p++) s += parts[p * n_per_part + i];
    eta_cls[i] = s;
}

hipError_t launch_spacetime_eta_shards(const double *parts, int nparts, int64_t n_per_part, double *eta_cls, hipStream_t st)
{
    if (n_per_part <= 0 || nparts <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_st_eta_shards, dim3((unsigned)((n_per_part + 255) / 256)), dim3(256), 0, st, parts, nparts, n_per_part, eta_cls);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256)
cf_st_eta_final(const double *__restrict__ eta_cls, const int32_t *__restrict__ cls, const double *__restrict__ pg, const double *__restrict__ w,
                int S, int K, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)S * K) return;
    const int s = (int)(i / K), k = (int)(i % K);
    out[i] = (pg[s] * eta_cls[(int64_t)cls[s] * K + k]) / w[k];   // :1365, p.dsigma already carries w_k
}

hipError_t launch_spacetime_eta_final(const double *eta_cls, const int32_t *cls, const double *pg, const double *w, int S, int K, double *out,
                                      hipStream_t st)
{
    const int64_t n = (int64_t)S * K;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_st_eta_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, eta_cls, cls, pg, w, S, K, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// bin keys (:1382-1398): itau = floor((tau - tau_min) / dtau), ir = floor((r - r_min) / dr), r = sqrt(x^2 + y^2).  The indices are formed
// in double (the reference's (int) cast of a huge quotient is undefined), a cell counts toward a histogram when its indices are in range.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
cf_st_keys(const double *__restrict__ tau, const double *__restrict__ ux, const double *__restrict__ uy, const double *__restrict__ un,
           const double *__restrict__ dat, const double *__restrict__ dax, const double *__restrict__ day, const double *__restrict__ dan,
           const double *__restrict__ x, const double *__restrict__ y, int64_t n, double tau_min, double dtau,
           int tau_bins, double r_min, double dr, int r_bins, int32_t *__restrict__ key_tau, int32_t *__restrict__ key_r,
           int32_t *__restrict__ key_tr, unsigned long long *__restrict__ counters, int all_cells)
{
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int out_t = 0, out_r = 0, neg_t = 0, neg_r = 0;
    if (c < n) {
        // every operation rounded on its own (contraction off): the bin of a cell on an edge is the host's
        const double r = sqrt(x[c] * x[c] + y[c] * y[c]);
        const double qt = floor((tau[c] - tau_min) / dtau), qr = floor((r - r_min) / dr);
        const bool in_t = qt >= 0.0 && qt < (double)tau_bins, in_r = qr >= 0.0 && qr < (double)r_bins;
        const int it = in_t ? (int)qt : -1, ir = in_r ? (int)qr : -1;
        key_tau[c] = it;
        key_r[c] = ir;
        key_tr[c] = (in_t && in_r) ? it * r_bins + ir : -1;
        // the counts are over the cells the reference bins: it skips u.dsigma <= 0 before binning (:1160-1170, the same expression);
        // a skipped cell is still listed in its bins, where it adds +0.  all_cells: the anisotropic-hydro path skips no cell and counts every one
        const double tau2 = tau[c] * tau[c];
        const double ut = sqrt(1.0 + ux[c] * ux[c] + uy[c] * uy[c] + tau2 * un[c] * un[c]);
        const bool live = all_cells || ut * dat[c] + ux[c] * dax[c] + uy[c] * day[c] + un[c] * dan[c] > 0.0;
        out_t = live && !in_t;
        out_r = live && !in_r;
        neg_t = live && qt < 0.0;
        neg_r = live && qr < 0.0;
    }
    // integer counts: one atomic per wave and counter, the totals do not depend on the order
    const unsigned long long m0 = __ballot(out_t), m1 = __ballot(out_r), m2 = __ballot(neg_t), m3 = __ballot(neg_r);
    if ((threadIdx.x & 63) == 0) {
        if (m0) atomicAdd(counters + 0, (unsigned long long)__popcll(m0));
        if (m1) atomicAdd(counters + 1, (unsigned long long)__popcll(m1));
        if (m2) atomicAdd(counters + 2, (unsigned long long)__popcll(m2));
        if (m3) atomicAdd(counters + 3, (unsigned long long)__popcll(m3));
    }
}

hipError_t launch_spacetime_keys(const double *tau, const double *ux, const double *uy, const double *un, const double *dat, const double *dax,
                                 const double *day, const double *dan, const double *x, const double *y, int64_t n, double tau_min, double dtau, int tau_bins,
                                 double r_min, double dr, int r_bins, int32_t *key_tau, int32_t *key_r, int32_t *key_tr,
                                 unsigned long long *counters, int all_cells, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_st_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tau, ux, uy, un, dat, dax, day, dan, x, y, n, tau_min, dtau, tau_bins, r_min, dr, r_bins,
                       key_tau, key_r, key_tr, counters, all_cells);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// stable counting sort: the cells are cut into ntile tiles; cnt[t][b] = cells of tile t in bin b (integer atomics: exact), then per bin
// the exclusive prefix over tiles, the exclusive prefix over bins, and a scatter that walks every tile in order, 256 cells at a time,
// ranking a cell among the earlier cells of its batch with the same key.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline void st_tile_range(int64_t n, int ntile, int t, int64_t &lo, int64_t &hi)
{
    lo = (n * t) / ntile;
    hi = (n * (t + 1)) / ntile;
}

__global__ void __launch_bounds__(256) cf_st_sort_count(const int32_t *__restrict__ key, int64_t n, int64_t B, int ntile, int32_t *__restrict__ cnt)
{
    int64_t lo, hi;
    st_tile_range(n, ntile, blockIdx.x, lo, hi);
    int32_t *row = cnt + (int64_t)blockIdx.x * B;
    for (int64_t c = lo + threadIdx.x; c < hi; c += blockDim.x) {
        const int k = key[c];
        if (k >= 0) atomicAdd(row + k, 1);
    }
}

__global__ void __launch_bounds__(256) cf_st_sort_cols(int32_t *__restrict__ cnt, int64_t B, int ntile, int32_t *__restrict__ tot)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int32_t run = 0;
    for (int t = 0; t < ntile; t++) {
        const int32_t v = cnt[(int64_t)t * B + b];
        cnt[(int64_t)t * B + b] = run;
        run += v;
    }
    tot[b] = run;
}

// one workgroup: start[b] = sum of tot[b' < b] (start[B] = the total)
__global__ void __launch_bounds__(256) cf_st_sort_scan(const int32_t *__restrict__ tot, int64_t B, int64_t *__restrict__ start)
{
    __shared__ int64_t part[256];
    const int t = threadIdx.x;
    const int64_t per = (B + 255) / 256, lo = std::min<int64_t>(B, t * per), hi = std::min<int64_t>(B, lo + per);
    int64_t s = 0;
    for (int64_t b = lo; b < hi; b++) s += tot[b];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; i++) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
        start[B] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t b = lo; b < hi; b++) {
        start[b] = run;
        run += tot[b];
    }
}

__global__ void __launch_bounds__(256)
cf_st_sort_scatter(const int32_t *__restrict__ key, int64_t n, int64_t B, int ntile, int32_t *__restrict__ cnt, const int64_t *__restrict__ start,
                   int32_t *__restrict__ list)
{
    __shared__ int32_t kb[256];
    int64_t lo, hi;
    st_tile_range(n, ntile, blockIdx.x, lo, hi);
    int32_t *row = cnt + (int64_t)blockIdx.x * B;
    const int t = threadIdx.x;
    for (int64_t base = lo; base < hi; base += 256) {
        const int64_t c = base + t;
        const int k = c < hi ? key[c] : -1;
        kb[t] = k;
        __syncthreads();
        int rank = 0;
        bool last = true;
        if (k >= 0) {
            for (int j = 0; j < 256; j++) {
                const int kj = kb[j];
                rank += (j < t && kj == k) ? 1 : 0;
                last = last && !(j > t && kj == k);
            }
            list[start[k] + row[k] + rank] = (int32_t)c;
        }
        __syncthreads();   // every cell of the batch has read row[k]
        if (k >= 0 && last) row[k] += rank + 1;
        __syncthreads();
    }
}

int spacetime_sort_tiles(int64_t n, int64_t B)
{
    int64_t t = std::min<int64_t>(1024, std::max<int64_t>(1, (n + 2047) / 2048));
    t = std::min<int64_t>(t, std::max<int64_t>(1, ((int64_t)1 << 26) / std::max<int64_t>(B, 1)));
    return (int)t;
}

hipError_t launch_spacetime_sort(const int32_t *key, int64_t n, int64_t B, int ntile, int32_t *cnt, int32_t *tot, int64_t *start, int32_t *list,
                                 hipStream_t st)
{
    hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)ntile * B, st);
    if (e != hipSuccess) return e;
    if (n > 0) hipLaunchKernelGGL(cf_st_sort_count, dim3(ntile), dim3(256), 0, st, key, n, B, ntile, cnt);
    hipLaunchKernelGGL(cf_st_sort_cols, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, cnt, B, ntile, tot);
    hipLaunchKernelGGL(cf_st_sort_scan, dim3(1), dim3(256), 0, st, (const int32_t *)tot, B, start);
    if (n > 0) hipLaunchKernelGGL(cf_st_sort_scatter, dim3(ntile), dim3(256), 0, st, key, n, B, ntile, cnt, (const int64_t *)start, list);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// cf_st_segsum: one wave per (segment, 64 species); the cell loop is wave-uniform, lanes gather their class's D.  Products and sums are
// rounded one at a time (no contraction): bin[s][b] is bitwise the left-to-right sum of pg[s] * D over the bin's cells.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
cf_st_segsum(const double *__restrict__ D, int64_t nc, int64_t c0, const int32_t *__restrict__ cls, const double *__restrict__ pg, int S,
             const int64_t *__restrict__ start, const int32_t *__restrict__ list, int64_t nseg, int first_pass, double *__restrict__ out)
{
#pragma clang fp contract(off)   // one rounding for the product, one for the sum (no fma)
    const int64_t seg = blockIdx.x;
    const int s = blockIdx.y * 64 + threadIdx.x;
    const bool active = s < S;
    const int ss = active ? s : S - 1;
    const double *__restrict__ row = D + (int64_t)cls[ss] * nc - c0;   // row[c] for c in [c0, c0 + nc)
    const double p = pg[ss];
    int64_t lo, hi;
    if (list) {
        // the segment's entries with a cell in [c0, c0 + nc): a contiguous run (ascending cells), found by bisection
        int64_t a = start[seg], b = start[seg + 1];
        int64_t l0 = a, h0 = b;
        while (l0 < h0) { const int64_t m = (l0 + h0) >> 1; if (list[m] < c0) l0 = m + 1; else h0 = m; }
        lo = l0;
        h0 = b;
        while (l0 < h0) { const int64_t m = (l0 + h0) >> 1; if (list[m] < c0 + nc) l0 = m + 1; else h0 = m; }
        hi = l0;
    } else {
        lo = c0;
        hi = c0 + nc;
    }
    double acc = first_pass ? 0.0 : (active ? out[(int64_t)s * nseg + seg] : 0.0);
    int64_t i = lo;
    constexpr int U = 32;   // loads in flight per wave: the all-cells segment is one serial walk per species (latency, not bandwidth)
    for (; i + U <= hi; i += U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = row[list ? (int64_t)list[i + u] : i + u];
#pragma unroll
        for (int u = 0; u < U; u++) acc = acc + p * v[u];
    }
    for (; i < hi; i++) acc = acc + p * row[list ? (int64_t)list[i] : i];
    if (active) out[(int64_t)s * nseg + seg] = acc;
}

hipError_t launch_spacetime_segsum(const double *D, int64_t nc, int64_t c0, const int32_t *cls, const double *pg, int S, const int64_t *start,
                                   const int32_t *list, int64_t nseg, int first_pass, double *out, hipStream_t st)
{
    if (nseg <= 0 || S <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_st_segsum, dim3((unsigned)nseg, (unsigned)((S + 63) / 64)), dim3(64), 0, st, D, nc, c0, cls, pg, S, start, list, nseg,
                       first_pass, out);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256)
cf_st_per_cell(const double *__restrict__ D, int64_t nc, int64_t c0, int64_t n_total, const int32_t *__restrict__ cls, const double *__restrict__ pg,
               int S, double *__restrict__ per_cell)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc * S) return;
    const int s = (int)(i / nc);
    const int64_t c = i % nc;
    per_cell[(int64_t)s * n_total + c0 + c] = pg[s] * D[(int64_t)cls[s] * nc + c];
}

hipError_t launch_spacetime_per_cell(const double *D, int64_t nc, int64_t c0, int64_t n_total, const int32_t *cls, const double *pg, int S,
                                     double *per_cell, hipStream_t st)
{
    const int64_t n = nc * S;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cf_st_per_cell, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, D, nc, c0, n_total, cls, pg, S, per_cell);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// the bin stage over plain device arrays: what is3d_plan_execute_spacetime and is3d_vah_plan_execute_spacetime share
// ------------------------------------------------------------------------------------------------
template <class T>
static hipError_t bins_grow(DevBuf<T> &buf, size_t n)
{
    if (buf.n >= n && buf.p) return hipSuccess;
    return buf.alloc(std::max<size_t>(n, 1));
}

int spacetime_bins_begin(StBinWork &w, StBinStage &s, hipStream_t st)
{
    const int64_t n = s.n, tb = s.bins->tau_bins, rbn = s.bins->r_bins, trb = tb * rbn;
    s.Bs[0] = tb; s.Bs[1] = rbn; s.Bs[2] = trb;
    HIP_TRY(bins_grow(w.keys, (size_t)3 * n));
    HIP_TRY(bins_grow(w.list, (size_t)3 * n));
    HIP_TRY(bins_grow(w.start, (size_t)(tb + 1) + (rbn + 1) + (trb + 1)));
    int ntile[3];
    size_t cnt_need = 1, tot_need = 1;
    for (int h = 0; h < 3; h++) {
        ntile[h] = spacetime_sort_tiles(n, s.Bs[h]);
        cnt_need = std::max(cnt_need, (size_t)ntile[h] * s.Bs[h]);
        tot_need = std::max(tot_need, (size_t)s.Bs[h]);
    }
    HIP_TRY(bins_grow(w.cnt, cnt_need));
    HIP_TRY(bins_grow(w.tot, tot_need));
    int32_t *keys[3];
    for (int h = 0; h < 3; h++) { keys[h] = w.keys.p + h * n; s.lists[h] = w.list.p + h * n; }
    s.starts[0] = w.start.p; s.starts[1] = w.start.p + tb + 1; s.starts[2] = w.start.p + tb + 1 + rbn + 1;
    s.hout[0] = s.out->dN_taudtaudy; s.hout[1] = s.out->dN_twopirdrdy; s.hout[2] = s.out->dN_twopitaurdtaudrdy;
    const double dtau = (s.bins->tau_max - s.bins->tau_min) / (double)s.bins->tau_bins, dr = (s.bins->r_max - s.bins->r_min) / (double)s.bins->r_bins;
    HIP_TRY(launch_spacetime_keys(s.tau, s.ux, s.uy, s.un, s.dat, s.dax, s.day, s.dan, s.x, s.y, n, s.bins->tau_min, dtau, s.bins->tau_bins, s.bins->r_min, dr,
                                  s.bins->r_bins, keys[0], keys[1], keys[2], s.counters, s.all_cells, st));
    for (int h = 0; h < 3; h++) HIP_TRY(launch_spacetime_sort(keys[h], n, s.Bs[h], ntile[h], w.cnt.p, w.tot.p, s.starts[h], s.lists[h], st));
    return IS3D_OK;
}

int spacetime_bins_add(const StBinStage &s, const double *D, int64_t nc, int64_t c0, int first, hipStream_t st)
{
    HIP_TRY(launch_spacetime_segsum(D, nc, c0, s.cls, s.pg, s.S, nullptr, nullptr, 1, first, s.out->dN_dy, st));
    for (int h = 0; h < 3; h++) HIP_TRY(launch_spacetime_segsum(D, nc, c0, s.cls, s.pg, s.S, s.starts[h], s.lists[h], s.Bs[h], first, s.hout[h], st));
    if (s.out->dN_dy_cell) HIP_TRY(launch_spacetime_per_cell(D, nc, c0, s.n, s.cls, s.pg, s.S, s.out->dN_dy_cell, st));
    return IS3D_OK;
}

}  // namespace is3d
