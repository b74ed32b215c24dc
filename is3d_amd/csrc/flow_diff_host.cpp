// flow_diff_host.cpp -- the host side of the differential flow records (include/is3d_amd.h): the list route
// is3d_flow_diff_list (THE definition, through the rules of cf_sampler_flow.h and cf_sampler_flow_diff.h), the reference flow vectors, the
// differential Q-cumulants, the writer, and the argument checks the device entries share.  No device use.
#include <charconv>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_sampler_flow_diff.h"
#include "errors.h"

namespace is3d {

int flow_diff_check_args(const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges, int32_t n_events, int32_t n_slots, const int32_t *slot,
                         int32_t n_species, const is3d_flow_diff_records *records, int device_static_words)
{
    if (!records || !pT_edges) return set_error(IS3D_EINVAL, "null argument");
    const is3d_flow_records view = flow_diff_view(*records);
    if (int rc = flow_check_args(cuts, n_events, n_slots, slot, n_species, &view, -1)) return rc;
    if (n_pT < 1 || n_pT > kFlowDiffMaxBins) return set_error(IS3D_EINVAL, "differential flow: n_pT = %d is outside 1..%d", n_pT, kFlowDiffMaxBins);
    if (!flow_diff_edges_valid(n_pT, pT_edges))
        return set_error(IS3D_EINVAL, "differential flow: the %d pT edges must be finite, strictly ascending and start at >= 0", n_pT + 1);
    if (memcmp(&cuts->pT_min, &pT_edges[0], sizeof(double)) != 0 || memcmp(&cuts->pT_max, &pT_edges[n_pT], sizeof(double)) != 0)
        return set_error(IS3D_EINVAL, "differential flow: cuts pT in [%.17g, %.17g) must equal the ends of the edge table [%.17g, %.17g) bit for bit",
                         cuts->pT_min, cuts->pT_max, pT_edges[0], pT_edges[n_pT]);
    if (device_static_words >= 0 && cuts->kernel_form == 2 && flow_diff_window_events(n_events, n_slots, n_pT, device_static_words) < 1)
        return set_error(IS3D_EINVAL,
                         "kernel_form = 2: the records of one event (%d slots x %d bins x %d = %lld words) do not fit the %lld words of the LDS beside %d",
                         n_slots, n_pT, kFlowRecordWords, (long long)n_slots * n_pT * kFlowRecordWords, (long long)kFlowLdsWords,
                         device_static_words + kFlowDiffEdgeWords);
    return IS3D_OK;
}

}  // namespace is3d

using is3d::kFlowRegions;
using is3d::set_error;
constexpr int H = IS3D_FLOW_HARMONICS;

extern "C" int is3d_flow_diff_list(const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges, int32_t n_events, int32_t n_slots,
                                   const int32_t *slot, int32_t n_species, int64_t n_particles, const is3d_particle *particles,
                                   const is3d_flow_diff_records *records)
{
    if (int rc = is3d::flow_diff_check_args(cuts, n_pT, pT_edges, n_events, n_slots, slot, n_species, records, -1)) return rc;
    if (n_particles < 0 || (n_particles > 0 && !particles)) return set_error(IS3D_EINVAL, "n_particles must be >= 0 and particles non-null");
    const is3d_flow_records view = is3d::flow_diff_view(*records);
    is3d::flow_records_zero(&view, n_events, n_slots * n_pT);
    const is3d::FlowThresholds t = is3d::flow_thresholds(*cuts);
    for (int64_t i = 0; i < n_particles; i++) {
        const is3d_particle &q = particles[i];
        if (q.species < 0 || q.species >= n_species || q.event < 0 || q.event >= n_events)
            return set_error(IS3D_EINVAL, "particle %lld: species or event out of range", (long long)i);
        const int s = slot[q.species];
        if (s < 0) continue;
        const int region = is3d::flow_region(*cuts, t, q);
        if (region < 0) continue;
        const int bin = is3d::flow_diff_bin([pT_edges](int k) { return pT_edges[k]; }, n_pT, is3d::flow_diff_pT(q));
        long long re[H], im[H];
        is3d::flow_terms(q, re, im);
        const size_t j0 = (((size_t)q.event * n_slots + (size_t)s) * n_pT + (size_t)bin) * kFlowRegions;
        for (int r = 0; r <= region; r += (region ? region : 1)) {             // region 0, then the particle's sub-event
            const size_t j = j0 + (size_t)r;
            records->m[j] += 1;
            for (int m = 0; m < H; m++) {
                records->p_re[j * H + m] += re[m];
                records->p_im[j * H + m] += im[m];
            }
        }
    }
    return IS3D_OK;
}

namespace {
int check_reference(const is3d_flow_diff_records *records, int32_t n_events, int32_t n_slots, int32_t n_pT, const int32_t *ref_slot, int32_t lo,
                    int32_t hi)
{
    if (!records || !records->m || !records->p_re || !records->p_im || !ref_slot) return set_error(IS3D_EINVAL, "null argument");
    if (n_events < 1 || n_slots < 1) return set_error(IS3D_EINVAL, "differential flow: n_events and n_slots must be >= 1 (got %d, %d)", n_events, n_slots);
    if (n_pT < 1 || n_pT > is3d::kFlowDiffMaxBins)
        return set_error(IS3D_EINVAL, "differential flow: n_pT = %d is outside 1..%d", n_pT, is3d::kFlowDiffMaxBins);
    for (int32_t s = 0; s < n_slots; s++)
        if (ref_slot[s] != 0 && ref_slot[s] != 1) return set_error(IS3D_EINVAL, "ref_slot[%d] = %d: 0 or 1", s, ref_slot[s]);
    if (!(lo >= 0 && lo < hi && hi <= n_pT)) return set_error(IS3D_EINVAL, "reference bins [%d, %d) must lie in [0, %d] and hold a bin", lo, hi, n_pT);
    return IS3D_OK;
}

typedef std::complex<double> cd;
}  // namespace

extern "C" int is3d_flow_diff_reference(const is3d_flow_diff_records *records, int32_t n_events, int32_t n_slots, int32_t n_pT,
                                        const int32_t *ref_slot, int32_t ref_bin_lo, int32_t ref_bin_hi, const is3d_flow_records *out)
{
    if (!out || !out->M || !out->Q_re || !out->Q_im) return set_error(IS3D_EINVAL, "null argument");
    if (int rc = check_reference(records, n_events, n_slots, n_pT, ref_slot, ref_bin_lo, ref_bin_hi)) return rc;
    is3d::flow_records_zero(out, n_events, 1);
    for (int32_t e = 0; e < n_events; e++)
        for (int32_t s = 0; s < n_slots; s++) {
            if (!ref_slot[s]) continue;
            for (int32_t b = ref_bin_lo; b < ref_bin_hi; b++)
                for (int r = 0; r < kFlowRegions; r++) {
                    const size_t a = (((size_t)e * n_slots + (size_t)s) * n_pT + (size_t)b) * kFlowRegions + (size_t)r;
                    const size_t o = (size_t)e * kFlowRegions + (size_t)r;
                    out->M[o] += records->m[a];
                    for (int m = 0; m < H; m++) {
                        out->Q_re[o * H + m] += records->p_re[a * H + m];
                        out->Q_im[o * H + m] += records->p_im[a * H + m];
                    }
                }
        }
    return IS3D_OK;
}

extern "C" int is3d_flow_diff_cumulants(const is3d_flow_diff_records *records, int32_t n_events, int32_t n_slots, int32_t n_pT,
                                        const int32_t *ref_slot, int32_t ref_bin_lo, int32_t ref_bin_hi, is3d_flow_diff_result *out)
{
    if (!out) return set_error(IS3D_EINVAL, "null argument");
    if (int rc = check_reference(records, n_events, n_slots, n_pT, ref_slot, ref_bin_lo, ref_bin_hi)) return rc;
    const size_t nref = (size_t)n_events * kFlowRegions;
    std::vector<int64_t> rM(nref), rRe(nref * H), rIm(nref * H);
    const is3d_flow_records ref{rM.data(), rRe.data(), rIm.data()};
    if (int rc = is3d_flow_diff_reference(records, n_events, n_slots, n_pT, ref_slot, ref_bin_lo, ref_bin_hi, &ref)) return rc;
    is3d_flow_result rc2;
    if (int rc = is3d_flow_cumulants(&ref, n_events, 1, &rc2)) return rc;
    const double unit = 1.0 / IS3D_SAMPLER_VN_SCALE;
    const auto vec = [unit](const int64_t *re, const int64_t *im, size_t j, int m) { return cd((double)re[j * H + m] * unit, (double)im[j * H + m] * unit); };
    for (int32_t s = 0; s < n_slots; s++)
        for (int32_t b = 0; b < n_pT; b++) {
            is3d_flow_diff_result o;
            memset(&o, 0, sizeof o);
            o.n_events = n_events;
            const bool in_ref = ref_slot[s] && b >= ref_bin_lo && b < ref_bin_hi;
            double num2[H] = {}, numg[H] = {}, num4[4] = {}, sum_re[H] = {};
            double w2 = 0.0, w4 = 0.0, wg = 0.0, sum_m = 0.0;
            for (int32_t e = 0; e < n_events; e++) {
                const size_t j = (((size_t)e * n_slots + (size_t)s) * n_pT + (size_t)b) * kFlowRegions, k = (size_t)e * kFlowRegions;
                const double M = (double)rM[k], MA = (double)rM[k + 1], MB = (double)rM[k + 2];
                const double mp = (double)records->m[j], mA = (double)records->m[j + 1], mB = (double)records->m[j + 2];
                const double mq = in_ref ? mp : 0.0;
                cd p[H], Q[H];
                for (int m = 0; m < H; m++) {
                    p[m] = vec(records->p_re, records->p_im, j, m);
                    Q[m] = vec(rRe.data(), rIm.data(), k, m);
                    sum_re[m] += p[m].real();
                }
                sum_m += mp;
                const double e2 = mp * M - mq, e4 = (mp * M - 3.0 * mq) * (M - 1.0) * (M - 2.0), eg = mA * MB + mB * MA;
                if (e2 > 0.0) {
                    o.n_used_2++;
                    w2 += e2;
                    for (int m = 0; m < H; m++) num2[m] += (p[m] * std::conj(Q[m])).real() - mq;
                }
                if (e4 > 0.0 && M >= 4.0) {
                    o.n_used_4++;
                    w4 += e4;
                    for (int m = 0; m < 4; m++) {
                        const cd pn = p[m], Qn = Q[m], Qc = std::conj(Q[m]), Q2c = std::conj(Q[2 * m + 1]);
                        const cd qn = in_ref ? p[m] : cd(0.0), q2n = in_ref ? p[2 * m + 1] : cd(0.0);
                        const cd t = pn * Qn * Qc * Qc - q2n * Qc * Qc - pn * Qn * Q2c - 2.0 * M * pn * Qc - 2.0 * mq * std::norm(Qn) + 7.0 * qn * Qc -
                                     Qn * std::conj(qn) + q2n * Q2c + 2.0 * pn * Qc + 2.0 * mq * M - 6.0 * mq;
                        num4[m] += t.real();
                    }
                }
                if (eg > 0.0) {
                    o.n_used_gap++;
                    wg += eg;
                    for (int m = 0; m < H; m++)
                        numg[m] += (vec(records->p_re, records->p_im, j + 1, m) * std::conj(vec(rRe.data(), rIm.data(), k + 2, m))).real() +
                                   (vec(records->p_re, records->p_im, j + 2, m) * std::conj(vec(rRe.data(), rIm.data(), k + 1, m))).real();
                }
            }
            for (int m = 0; m < H; m++) {
                o.d2[m] = w2 > 0.0 ? num2[m] / w2 : 0.0;
                o.d2_gap[m] = wg > 0.0 ? numg[m] / wg : 0.0;
                o.v2[m] = rc2.c2[m] > 0.0 ? o.d2[m] / std::sqrt(rc2.c2[m]) : 0.0;
                o.v2_gap[m] = rc2.c2_gap[m] > 0.0 ? o.d2_gap[m] / std::sqrt(rc2.c2_gap[m]) : 0.0;
                o.v_rp[m] = sum_m > 0.0 ? sum_re[m] / sum_m : 0.0;
            }
            for (int m = 0; m < 4; m++) {
                o.avg4[m] = w4 > 0.0 ? num4[m] / w4 : 0.0;
                o.d4[m] = w4 > 0.0 ? o.avg4[m] - 2.0 * o.d2[m] * rc2.c2[m] : 0.0;
                o.v4[m] = rc2.c4[m] < 0.0 ? -o.d4[m] / std::pow(-rc2.c4[m], 0.75) : 0.0;
            }
            o.sum_m = sum_m;
            o.mean_m = sum_m / (double)n_events;
            out[(size_t)s * n_pT + (size_t)b] = o;
        }
    return IS3D_OK;
}

// <dir>/flow/differential_<label>.dat per slot; doubles by std::to_chars(scientific, 8) as the other writers' values, integers in full
extern "C" int is3d_write_flow_diff(const char *results_dir, const is3d_flow_diff_records *records, int32_t n_events, int32_t n_slots, int32_t n_pT,
                                    const double *pT_edges, const int32_t *ref_slot, int32_t ref_bin_lo, int32_t ref_bin_hi,
                                    const char *const *labels)
{
    if (!results_dir || !labels || !pT_edges) return set_error(IS3D_EINVAL, "null argument");
    if (int rc = check_reference(records, n_events, n_slots, n_pT, ref_slot, ref_bin_lo, ref_bin_hi)) return rc;
    if (!is3d::flow_diff_edges_valid(n_pT, pT_edges))
        return set_error(IS3D_EINVAL, "differential flow: the %d pT edges must be finite, strictly ascending and start at >= 0", n_pT + 1);
    for (int32_t s = 0; s < n_slots; s++)
        if (!labels[s] || !labels[s][0] || strchr(labels[s], '/'))
            return set_error(IS3D_EINVAL, "differential flow writer: label %d is empty or holds a '/'", s);
    std::vector<is3d_flow_diff_result> res((size_t)n_slots * n_pT);
    if (int rc = is3d_flow_diff_cumulants(records, n_events, n_slots, n_pT, ref_slot, ref_bin_lo, ref_bin_hi, res.data())) return rc;
    const auto num = [](std::string &out, double v) {
        char buf[40];
        const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific, 8);
        out.append(buf, (size_t)(r.ptr - buf));
    };
    for (int32_t s = 0; s < n_slots; s++) {
        std::string c = "# bin\tpT_lo\tpT_hi\tn\td_n{2}\td_n{4}\td_n{2,gap}\tv_n{2}\tv_n{4}\tv_n{2,gap}\tv_n (reaction plane)\tsum m_p; d_n{4} and v_n{4} exist for n <= 4 (0 beyond)\n";
        c += "# events: " + std::to_string((long long)n_events) + ", pT bins: " + std::to_string((long long)n_pT) + ", reference bins: [" +
             std::to_string((long long)ref_bin_lo) + ", " + std::to_string((long long)ref_bin_hi) + "), this slot in the reference: " +
             std::to_string((long long)ref_slot[s]) + "\n";
        for (int32_t b = 0; b < n_pT; b++) {
            const is3d_flow_diff_result &o = res[(size_t)s * n_pT + (size_t)b];
            for (int m = 0; m < H; m++) {
                c += std::to_string(b);
                c.push_back('\t'); num(c, pT_edges[b]);
                c.push_back('\t'); num(c, pT_edges[b + 1]);
                c += "\t" + std::to_string(m + 1);
                const double row[7] = {o.d2[m], m < 4 ? o.d4[m] : 0.0, o.d2_gap[m], o.v2[m], m < 4 ? o.v4[m] : 0.0, o.v2_gap[m], o.v_rp[m]};
                for (double v : row) { c.push_back('\t'); num(c, v); }
                c += "\t" + std::to_string((long long)o.sum_m) + "\n";
            }
        }
        const std::string path = std::string(results_dir) + "/flow/differential_" + labels[s] + ".dat";
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) return set_error(IS3D_EIO, "cannot open %s (the flow/ directory must exist)", path.c_str());
        const bool ok = fwrite(c.data(), 1, c.size(), f) == c.size();
        if (!(fclose(f) == 0 && ok)) return set_error(IS3D_EIO, "cannot write %s", path.c_str());
    }
    return IS3D_OK;
}
