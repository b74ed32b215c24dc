// cf_spacetime_host.cpp -- the host side of operation 0 that does not depend on the plan it serves (cf_spacetime.h): is3d_plan (df_mode 1-4,
// cf_plan.cpp) and is3d_vah_plan (cf_vah.hip) keep one StState each and bring their own records and per-cell launches to spacetime_run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cf_host.h"
#include "cf_launch.h"
#include "cf_spacetime.h"
#include "errors.h"

namespace is3d {

int spacetime_check_bins(const is3d_spacetime_bins *b, const double *x, const double *y)
{
    if (!x || !y) return set_error(IS3D_EINVAL, "operation 0 needs the cells' x and y positions (NULL given)");
    if (!b) return set_error(IS3D_EINVAL, "null spacetime bins");
    if (b->tau_bins < 1 || b->r_bins < 1) return set_error(IS3D_EINVAL, "tau_bins and r_bins must be >= 1 (got %d, %d)", b->tau_bins, b->r_bins);
    if (!(b->tau_max > b->tau_min) || !(b->r_max > b->r_min))
        return set_error(IS3D_EINVAL, "the bin ranges need tau_max > tau_min and r_max > r_min (got [%g, %g], [%g, %g])", b->tau_min, b->tau_max,
                         b->r_min, b->r_max);
    if ((int64_t)b->tau_bins * b->r_bins > ((int64_t)1 << 28)) return set_error(IS3D_EINVAL, "tau_bins x r_bins too large");
    return IS3D_OK;
}

// what the per-cell kernels take of a grid: up to 64 pT values (one wave holds a class), and in 2+1D the workgroup's eta rows in LDS --
// [4 waves][64 / npTp classes][K] doubles within lds_cap_bytes (64 KiB; the feqmod kernel keeps 16 KiB of it for its staged records: 48 KiB).
// A function of the grid alone: the one-shot entries ask it before they create a plan
int spacetime_check_grid(bool dim3, size_t lds_cap_bytes, int npT, int K)
{
    if (npT > 64) return set_error(IS3D_EINVAL, "operation 0 takes pT grids of up to 64 values (got %d)", npT);
    int npTp = 1;
    while (npTp < npT) npTp <<= 1;
    const size_t per_eta = sizeof(double) * 4 * (64 / npTp);
    if (!dim3 && per_eta * (size_t)K > lds_cap_bytes)
        return set_error(IS3D_EINVAL, "operation 0 in 2+1D: %d pT values x %d eta nodes need more LDS than the per-cell kernel has (up to %d eta "
                         "nodes with this pT grid)", npT, K, (int)(lds_cap_bytes / per_eta));
    return IS3D_OK;
}

int spacetime_check_out(const is3d_spacetime_out *out)
{
    if (!out->dN_dy || !out->dN_taudtaudy || !out->dN_twopirdrdy || !out->dN_twopitaurdtaudrdy || !out->dN_dydeta)
        return set_error(IS3D_EINVAL, "a required output array is NULL");
    return IS3D_OK;
}

// the spacetime lane tables and the per-pass workspace of a plan, made once
int spacetime_setup(StState &s, const StSetup &a)
{
    if (s.ready) return IS3D_OK;
    s.ncls = a.ncls; s.npT = a.npT; s.J = a.J; s.K = a.K; s.S = a.npart; s.dim3 = a.dim3; s.nphi = a.jtiles * a.JT;
    int npTp = 1;
    while (npTp < a.npT) npTp <<= 1;
    s.npTp = npTp;
    s.nlw = (a.ncls * npTp + 63) / 64;
    const int nl = s.nlw * 64;
    std::vector<double> mT(nl, 1.0), pT(nl, 0.0), sg(nl, 1.0), b(nl, 0.0), ms(nl, 1.0);
    for (int l = 0; l < nl; l++) {
        int c = l / npTp, i = l % npTp;
        if (c >= a.ncls || i >= a.npT) {   // padded lanes (w_pT = 0), see StPad
            if (a.pad == ST_PAD_UNIT) continue;
            if (c >= a.ncls) c = 0;
            if (i >= a.npT) i = 0;
        }
        const double m = a.cls_mass[c], p = a.pT_grid[i];
        ms[l] = m;
        mT[l] = std::sqrt(m * m + p * p);
        pT[l] = p;
        sg[l] = a.cls_sign[c];
        if (a.cls_bar) b[l] = a.cls_bar[c];
    }
    HIP_TRY(s.d_mT.upload(mT));
    HIP_TRY(s.d_pT.upload(pT));
    HIP_TRY(s.d_sign.upload(sg));
    if (a.b_lanes) HIP_TRY(s.d_b.upload(b));
    if (a.mass_lanes) HIP_TRY(s.d_mass.upload(ms));
    HIP_TRY(s.d_wpT.alloc(nl));
    HIP_TRY(s.d_wphi.alloc((size_t)s.nphi));
    HIP_TRY(s.d_cls.upload(a.sp_cls, (size_t)a.npart));
    std::vector<double> pg(a.npart);
    for (int k = 0; k < a.npart; k++) pg[k] = a.prefactor * a.sp_deg[k];
    HIP_TRY(s.d_pg.upload(pg));
    // passes: the plan's record stream plus D (8 B per class and cell) within the same cap as the spectra path
    const int64_t ws = default_stream_cap_bytes(a.workspace_bytes);
    const int64_t per_cell = a.bytes_per_cell + 8 * (int64_t)a.ncls;
    s.pass = std::max<int64_t>(1, std::min<int64_t>(a.pass_cells, ws / per_cell));
    const hipError_t e = s.d_D.alloc((size_t)a.ncls * s.pass);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return set_error(IS3D_ENOMEM, "out of device memory allocating the per-cell workspace D"); }
    HIP_TRY(e);
    if (!a.dim3) HIP_TRY(s.d_eta.alloc((size_t)a.ncls * a.K));
    HIP_TRY(s.d_counters.alloc(4));
    s.ready = true;
    return IS3D_OK;
}

// pT_tab, phi_tab column 2.  An execute with the same weights does not block the host here
int spacetime_upload_weights(StState &s, const double *pT_w, const double *phi_w, hipStream_t st)
{
    if (s.hwpT.size() == (size_t)s.npT && s.hwphi.size() == (size_t)s.J && std::equal(s.hwpT.begin(), s.hwpT.end(), pT_w) &&
        std::equal(s.hwphi.begin(), s.hwphi.end(), phi_w))
        return IS3D_OK;
    std::vector<double> wl((size_t)s.nlw * 64, 0.0), wp((size_t)s.nphi, 0.0);
    for (size_t l = 0; l < wl.size(); l++) {
        const int c = (int)(l / s.npTp), i = (int)(l % s.npTp);
        if (c < s.ncls && i < s.npT) wl[l] = pT_w[i];
    }
    for (int j = 0; j < s.J; j++) wp[j] = phi_w[j];
    HIP_TRY(hipMemcpyAsync(s.d_wpT.p, wl.data(), wl.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.d_wphi.p, wp.data(), wp.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors go out of scope
    s.hwpT.assign(pT_w, pT_w + s.npT);
    s.hwphi.assign(phi_w, phi_w + s.J);
    return IS3D_OK;
}

template <class T>
static hipError_t st_grow(DevBuf<T> &buf, size_t n)
{
    if (buf.n >= n && buf.p) return hipSuccess;
    return buf.alloc(std::max<size_t>(n, 1));
}

int spacetime_run(StState &s, const StRun &r)
{
    StSplit *split = r.split;
    const bool do_cells = !split || split->role == ST_CELLS, do_bins = !split || split->role == ST_BINS;
    const int64_t n = r.bs.n;
    const is3d_spacetime_out *out = r.bs.out;
    const int S = s.S, K = s.K;
    hipStream_t st = r.stream;
    is3d_spacetime_stats *stats = r.stats;

    std::vector<hipEvent_t> ev;
    struct EvGuard { std::vector<hipEvent_t> &e; ~EvGuard() { for (auto x : e) (void)hipEventDestroy(x); } } evg{ev};
    std::vector<int> stage;   // stage of the interval between events i and i + 1
    const StMark mark = [&](int what) -> hipError_t {
        if (!stats) return hipSuccess;
        hipEvent_t e;
        const hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        if (!ev.empty()) stage.push_back(what);
        ev.push_back(e);
        return hipEventRecord(e, st);
    };
    static const unsigned long long init[8] = {~0ULL, 0ULL, 0ULL, 0ULL, 0ULL, 0ULL, 0ULL, ~0ULL};
    HIP_TRY(hipMemcpyAsync(r.d_status, init, sizeof init, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s.d_counters.p, 0, 4 * sizeof(unsigned long long), st));
    HIP_TRY(mark(0));

    // ---- bin stage, part 1: keys and the stable counting sort of every histogram (once per execute) ----
    StBinStage bs = r.bs;
    if (do_bins) {
        bs.cls = s.d_cls.p; bs.pg = s.d_pg.p; bs.S = S; bs.counters = s.d_counters.p;
        if (int rc = spacetime_bins_begin(s.bins, bs, st)) return rc;
        HIP_TRY(mark(2));
    }
    // ---- bin stage, part 2: a block of D, cells [c0, c0 + nc) in ascending order, onto the running sums ----
    const auto sum_bins = [&](const double *D, int64_t nc, int64_t c0, int first) -> int {
        if (int rc = spacetime_bins_add(bs, D, nc, c0, first, st)) return rc;
        HIP_TRY(mark(2));
        return IS3D_OK;
    };

    if (n == 0) {
        if (do_bins) {
            HIP_TRY(hipMemsetAsync(out->dN_dy, 0, sizeof(double) * S, st));
            for (int h = 0; h < 3; h++) HIP_TRY(hipMemsetAsync(bs.hout[h], 0, sizeof(double) * S * bs.Bs[h], st));
            HIP_TRY(hipMemsetAsync(out->dN_dydeta, 0, sizeof(double) * S * (s.dim3 ? 1 : K), st));
        }
    } else {
        const int64_t pc = s.pass;
        const int G = (s.nlw + 3) / 4;
        int nch = (int)std::min<int64_t>(pc, std::max<int64_t>(1, 16384 / G));
        if (!s.dim3) nch = (int)std::max<int64_t>(1, std::min<int64_t>(nch, ((int64_t)256 << 20) / (8 * (int64_t)s.ncls * K)));
        if (!s.dim3 && do_cells) HIP_TRY(st_grow(s.d_slab, (size_t)(nch + r.linear_slots) * s.ncls * K));
        const int npasses = do_cells ? (int)((n + pc - 1) / pc) : 0;
        for (int pass = 0; pass < npasses; pass++) {
            const int64_t c0 = (int64_t)pass * pc;
            const int32_t nc = (int32_t)std::min<int64_t>(pc, n - c0);
            if (int rc = r.pass(pass, c0, nc, nch, mark)) return rc;
            if (split) {
                // the pass's block [class][nc] into the assembled [class][n_total] at the shard's global cell offset
                double *dst = split->D_full + split->c_off + c0;
                if (split->D_device == r.device)
                    HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double) * (size_t)split->n_total, s.d_D.p, sizeof(double) * (size_t)nc,
                                             sizeof(double) * (size_t)nc, (size_t)s.ncls, hipMemcpyDeviceToDevice, st));
                else
                    for (int c = 0; c < s.ncls; c++)
                        HIP_TRY(hipMemcpyPeerAsync(dst + (int64_t)c * split->n_total, split->D_device, s.d_D.p + (int64_t)c * nc, r.device,
                                                   sizeof(double) * (size_t)nc, st));
                HIP_TRY(mark(5));
            } else if (int rc = sum_bins(s.d_D.p, nc, c0, pass == 0))
                return rc;
        }
        if (do_bins) {
            if (split)   // the whole assembled D at once: the same left-to-right sums as pass after pass
                if (int rc = sum_bins(split->D_full, n, 0, 1)) return rc;
            // dN/dy deta: 2+1D one value per eta node, the node's term over its effective weight; 3+1D the single point of the species' total
            // (quirk 2)
            if (s.dim3) HIP_TRY(hipMemcpyAsync(out->dN_dydeta, out->dN_dy, sizeof(double) * S, hipMemcpyDeviceToDevice, st));
            else HIP_TRY(launch_spacetime_eta_final(s.d_eta.p, s.d_cls.p, s.d_pg.p, r.kweight, S, K, out->dN_dydeta, st));
            HIP_TRY(mark(2));
        }
        if (!stats && r.d_sticky) HIP_TRY(launch_fold_status(r.d_status, r.d_sticky, st));
    }
    if (!stats) return IS3D_OK;
    unsigned long long cn[4];
    HIP_TRY(hipMemcpyAsync(r.status, r.d_status, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cn, s.d_counters.p, sizeof cn, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double unused = 0;
    double *const into[6] = {&stats->ms_prep, &stats->ms_cells, &stats->ms_bins, r.ms_renorm ? r.ms_renorm : &unused,
                             r.ms_linear ? r.ms_linear : &unused, &stats->ms_d2h};
    for (size_t i = 1; i < ev.size(); i++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[i - 1], ev[i]));
        *into[stage[i - 1]] += ms;
    }
    stats->n_classes = s.ncls;
    stats->n_passes = (n == 0 || !do_cells) ? 0 : (int32_t)((n + s.pass - 1) / s.pass);
    stats->n_tau_outside = (int64_t)cn[0];
    stats->n_r_outside = (int64_t)cn[1];
    stats->n_tau_negative = (int64_t)cn[2];
    stats->n_r_negative = (int64_t)cn[3];
    return IS3D_OK;
}

}  // namespace is3d
