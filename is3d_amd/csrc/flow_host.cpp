// flow_host.cpp -- the host side of the per-event flow records (include/is3d_amd.h): the list route is3d_flow_list
// (THE definition, through the one rule of cf_sampler_flow.h), the integer merge of slots, the Q-cumulants, and the argument checks and
// record plumbing the device entries share.  No device use.
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_sampler_flow.h"
#include "errors.h"

namespace is3d {

int flow_check_args(const is3d_flow_cuts *cuts, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                    const is3d_flow_records *records, int device_static_words)
{
    if (!cuts || !slot || !records || !records->M || !records->Q_re || !records->Q_im) return set_error(IS3D_EINVAL, "null argument");
    if (n_events < 1 || n_slots < 1 || n_species < 1)
        return set_error(IS3D_EINVAL, "flow records: n_events, n_slots and n_species must be >= 1 (got %d, %d, %d)", n_events, n_slots, n_species);
    if (!flow_cuts_valid(*cuts))
        return set_error(IS3D_EINVAL, "flow cuts: y_cut > 0, 0 <= y_gap < 2 y_cut and pT_max > pT_min >= 0 are required (got y_cut = %g, y_gap = %g, pT in [%g, %g))",
                         cuts->y_cut, cuts->y_gap, cuts->pT_min, cuts->pT_max);
    if (cuts->kernel_form < 0 || cuts->kernel_form > 2) return set_error(IS3D_EINVAL, "kernel_form = %d: 0, 1 or 2", cuts->kernel_form);
    for (int32_t s = 0; s < n_species; s++)
        if (slot[s] < -1 || slot[s] >= n_slots) return set_error(IS3D_EINVAL, "slot[%d] = %d is outside [-1, %d)", s, slot[s], n_slots);
    if (device_static_words >= 0 && cuts->kernel_form == 2 && flow_window_events(n_events, n_slots, device_static_words) < 1)
        return set_error(IS3D_EINVAL, "kernel_form = 2: the records of one event (%d slots x %d = %lld words) do not fit the %lld words of the LDS", n_slots,
                         kFlowRecordWords, (long long)n_slots * kFlowRecordWords, (long long)kFlowLdsWords);
    return IS3D_OK;
}

void flow_records_zero(const is3d_flow_records *r, int32_t n_events, int32_t n_slots)
{
    const size_t rec = (size_t)n_events * n_slots * kFlowRegions;
    memset(r->M, 0, rec * sizeof(int64_t));
    memset(r->Q_re, 0, rec * IS3D_FLOW_HARMONICS * sizeof(int64_t));
    memset(r->Q_im, 0, rec * IS3D_FLOW_HARMONICS * sizeof(int64_t));
}

void flow_records_scatter(const int64_t *block, const is3d_flow_records *r, int32_t n_events, int32_t n_slots)
{
    const size_t rec = (size_t)n_events * n_slots * kFlowRegions;
    for (size_t j = 0; j < rec; j++) {
        const int64_t *w = block + j * kFlowRegionWords;
        r->M[j] = w[0];
        memcpy(r->Q_re + j * IS3D_FLOW_HARMONICS, w + 1, IS3D_FLOW_HARMONICS * sizeof(int64_t));
        memcpy(r->Q_im + j * IS3D_FLOW_HARMONICS, w + 1 + IS3D_FLOW_HARMONICS, IS3D_FLOW_HARMONICS * sizeof(int64_t));
    }
}

int flow_records_check(const is3d_flow_records *r, int32_t n_events, int32_t n_slots)
{
    const size_t rec = (size_t)n_events * n_slots * kFlowRegions;
    for (size_t j = 0; j < rec; j++)
        if (r->M[j] > IS3D_SAMPLER_VN_MAX_COUNT)
            return set_error(IS3D_EDOMAIN, "flow record (event %lld, slot %lld, region %d) holds %lld hadrons: the fixed-point flow vectors are exact up to %lld",
                             (long long)(j / ((size_t)n_slots * kFlowRegions)), (long long)(j / kFlowRegions % n_slots), (int)(j % kFlowRegions),
                             (long long)r->M[j], (long long)IS3D_SAMPLER_VN_MAX_COUNT);
    return IS3D_OK;
}

}  // namespace is3d

using is3d::kFlowRegions;
using is3d::set_error;
constexpr int H = IS3D_FLOW_HARMONICS;

extern "C" int is3d_flow_list(const is3d_flow_cuts *cuts, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                              int64_t n_particles, const is3d_particle *particles, const is3d_flow_records *records)
{
    if (int rc = is3d::flow_check_args(cuts, n_events, n_slots, slot, n_species, records, -1)) return rc;
    if (n_particles < 0 || (n_particles > 0 && !particles)) return set_error(IS3D_EINVAL, "n_particles must be >= 0 and particles non-null");
    is3d::flow_records_zero(records, n_events, n_slots);
    const is3d::FlowThresholds t = is3d::flow_thresholds(*cuts);
    for (int64_t i = 0; i < n_particles; i++) {
        const is3d_particle &q = particles[i];
        if (q.species < 0 || q.species >= n_species || q.event < 0 || q.event >= n_events)
            return set_error(IS3D_EINVAL, "particle %lld: species or event out of range", (long long)i);
        const int s = slot[q.species];
        if (s < 0) continue;
        const int region = is3d::flow_region(*cuts, t, q);
        if (region < 0) continue;
        long long re[H], im[H];
        is3d::flow_terms(q, re, im);
        const size_t j0 = ((size_t)q.event * n_slots + (size_t)s) * kFlowRegions;
        for (int r = 0; r <= region; r += (region ? region : 1)) {             // region 0, then the particle's sub-event
            const size_t j = j0 + (size_t)r;
            records->M[j] += 1;
            for (int m = 0; m < H; m++) {
                records->Q_re[j * H + m] += re[m];
                records->Q_im[j * H + m] += im[m];
            }
        }
    }
    return IS3D_OK;
}

extern "C" int is3d_flow_merge(const is3d_flow_records *records, int32_t n_events, int32_t n_slots, const int32_t *group, int32_t n_groups,
                               const is3d_flow_records *out)
{
    if (!records || !records->M || !records->Q_re || !records->Q_im || !group || !out || !out->M || !out->Q_re || !out->Q_im)
        return set_error(IS3D_EINVAL, "null argument");
    if (n_events < 1 || n_slots < 1 || n_groups < 1)
        return set_error(IS3D_EINVAL, "flow merge: n_events, n_slots and n_groups must be >= 1 (got %d, %d, %d)", n_events, n_slots, n_groups);
    for (int32_t s = 0; s < n_slots; s++)
        if (group[s] < -1 || group[s] >= n_groups) return set_error(IS3D_EINVAL, "group[%d] = %d is outside [-1, %d)", s, group[s], n_groups);
    is3d::flow_records_zero(out, n_events, n_groups);
    for (int32_t e = 0; e < n_events; e++)
        for (int32_t s = 0; s < n_slots; s++) {
            if (group[s] < 0) continue;
            for (int r = 0; r < kFlowRegions; r++) {
                const size_t a = ((size_t)e * n_slots + (size_t)s) * kFlowRegions + (size_t)r;
                const size_t b = ((size_t)e * n_groups + (size_t)group[s]) * kFlowRegions + (size_t)r;
                out->M[b] += records->M[a];
                for (int m = 0; m < H; m++) {
                    out->Q_re[b * H + m] += records->Q_re[a * H + m];
                    out->Q_im[b * H + m] += records->Q_im[a * H + m];
                }
            }
        }
    return IS3D_OK;
}

namespace {
double signed_root(double c, double power) { return c == 0.0 ? 0.0 : (c > 0.0 ? 1.0 : -1.0) * std::pow(std::fabs(c), power); }
}  // namespace

extern "C" int is3d_flow_cumulants(const is3d_flow_records *records, int32_t n_events, int32_t n_slots, is3d_flow_result *out)
{
    if (!records || !records->M || !records->Q_re || !records->Q_im || !out) return set_error(IS3D_EINVAL, "null argument");
    if (n_events < 1 || n_slots < 1) return set_error(IS3D_EINVAL, "flow cumulants: n_events and n_slots must be >= 1 (got %d, %d)", n_events, n_slots);
    const double unit = 1.0 / IS3D_SAMPLER_VN_SCALE;
    for (int32_t s = 0; s < n_slots; s++) {
        is3d_flow_result o;
        memset(&o, 0, sizeof o);
        o.n_events = n_events;
        double num2[H] = {}, numg[H] = {}, num4[4] = {}, sum_re[H] = {};
        double w2 = 0.0, w4 = 0.0, wg = 0.0, sum_M = 0.0, sum_M2 = 0.0;
        for (int32_t e = 0; e < n_events; e++) {
            const size_t j = ((size_t)e * n_slots + (size_t)s) * kFlowRegions;
            const double M = (double)records->M[j], MA = (double)records->M[j + 1], MB = (double)records->M[j + 2];
            double qr[H], qi[H];
            for (int m = 0; m < H; m++) {
                qr[m] = (double)records->Q_re[j * H + m] * unit;
                qi[m] = (double)records->Q_im[j * H + m] * unit;
                sum_re[m] += qr[m];
            }
            sum_M += M;
            sum_M2 += M * M;
            const double e2 = M * (M - 1.0), e4 = M * (M - 1.0) * (M - 2.0) * (M - 3.0), eg = MA * MB;
            if (e2 > 0.0) {
                o.n_used_2++;
                w2 += e2;
                for (int m = 0; m < H; m++) num2[m] += qr[m] * qr[m] + qi[m] * qi[m] - M;
            }
            if (e4 > 0.0) {
                o.n_used_4++;
                w4 += e4;
                for (int m = 0; m < 4; m++) {
                    const double q2 = qr[m] * qr[m] + qi[m] * qi[m];
                    const double dr = qr[2 * m + 1], di = qi[2 * m + 1];                     // Q_2n
                    const double sr = qr[m] * qr[m] - qi[m] * qi[m], si = 2.0 * qr[m] * qi[m];   // Q_n^2
                    num4[m] += q2 * q2 + (dr * dr + di * di) - 2.0 * (dr * sr + di * si) - 4.0 * (M - 2.0) * q2 + 2.0 * M * (M - 3.0);
                }
            }
            if (eg > 0.0) {
                o.n_used_gap++;
                wg += eg;
                for (int m = 0; m < H; m++) {
                    const size_t a = (j + 1) * H + m, b = (j + 2) * H + m;
                    numg[m] += ((double)records->Q_re[a] * unit) * ((double)records->Q_re[b] * unit) +
                               ((double)records->Q_im[a] * unit) * ((double)records->Q_im[b] * unit);
                }
            }
        }
        for (int m = 0; m < H; m++) {
            o.c2[m] = w2 > 0.0 ? num2[m] / w2 : 0.0;
            o.c2_gap[m] = wg > 0.0 ? numg[m] / wg : 0.0;
            o.v2[m] = signed_root(o.c2[m], 0.5);
            o.v2_gap[m] = signed_root(o.c2_gap[m], 0.5);
            o.v_rp[m] = sum_M > 0.0 ? sum_re[m] / sum_M : 0.0;
        }
        for (int m = 0; m < 4; m++) {
            o.avg4[m] = w4 > 0.0 ? num4[m] / w4 : 0.0;
            o.c4[m] = w4 > 0.0 ? o.avg4[m] - 2.0 * o.c2[m] * o.c2[m] : 0.0;
            o.v4[m] = signed_root(-o.c4[m], 0.25);
        }
        o.mean_M = sum_M / (double)n_events;
        o.var_M = sum_M2 / (double)n_events - o.mean_M * o.mean_M;
        out[s] = o;
    }
    return IS3D_OK;
}

// <dir>/flow/cumulants_<label>.dat and <dir>/flow/multiplicity_<label>.dat per slot; doubles by std::to_chars(scientific, 8) as the other
// writers' values, integers in full
extern "C" int is3d_write_flow(const char *results_dir, const is3d_flow_records *records, int32_t n_events, int32_t n_slots, const char *const *labels)
{
    if (!results_dir || !labels || !records || !records->M || !records->Q_re || !records->Q_im) return set_error(IS3D_EINVAL, "null argument");
    if (n_events < 1 || n_slots < 1) return set_error(IS3D_EINVAL, "flow writer: n_events and n_slots must be >= 1 (got %d, %d)", n_events, n_slots);
    for (int32_t s = 0; s < n_slots; s++)
        if (!labels[s] || !labels[s][0] || strchr(labels[s], '/')) return set_error(IS3D_EINVAL, "flow writer: label %d is empty or holds a '/'", s);
    std::vector<is3d_flow_result> res((size_t)n_slots);
    if (int rc = is3d_flow_cumulants(records, n_events, n_slots, res.data())) return rc;
    const auto num = [](std::string &out, double v) {
        char buf[40];
        const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific, 8);
        out.append(buf, (size_t)(r.ptr - buf));
    };
    const auto put = [](const std::string &path, const std::string &text) {
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) return set_error(IS3D_EIO, "cannot open %s (the flow/ directory must exist)", path.c_str());
        const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
        return (fclose(f) == 0 && ok) ? IS3D_OK : set_error(IS3D_EIO, "cannot write %s", path.c_str());
    };
    for (int32_t s = 0; s < n_slots; s++) {
        const is3d_flow_result &o = res[(size_t)s];
        std::string c = "# n\tc_n{2}\tc_n{4}\tc_n{2,gap}\tv_n{2}\tv_n{4}\tv_n{2,gap}\tv_n (reaction plane); c_n{4} and v_n{4} exist for n <= 4 (0 beyond)\n";
        c += "# events: " + std::to_string((long long)o.n_events) + ", used for <2>: " + std::to_string((long long)o.n_used_2) + ", <4>: " +
             std::to_string((long long)o.n_used_4) + ", <2>_gap: " + std::to_string((long long)o.n_used_gap) + "\n";
        for (int m = 0; m < H; m++) {
            c += std::to_string(m + 1);
            const double row[7] = {o.c2[m], m < 4 ? o.c4[m] : 0.0, o.c2_gap[m], o.v2[m], m < 4 ? o.v4[m] : 0.0, o.v2_gap[m], o.v_rp[m]};
            for (double v : row) { c.push_back('\t'); num(c, v); }
            c.push_back('\n');
        }
        std::string m = "# mean and variance of M (full acceptance, over all events): ";
        num(m, o.mean_M); m.push_back(' '); num(m, o.var_M);
        m += "\n# event\tM\tM_A\tM_B\n";
        for (int32_t e = 0; e < n_events; e++) {
            const size_t j = ((size_t)e * n_slots + (size_t)s) * kFlowRegions;
            m += std::to_string(e) + "\t" + std::to_string((long long)records->M[j]) + "\t" + std::to_string((long long)records->M[j + 1]) + "\t" +
                 std::to_string((long long)records->M[j + 2]) + "\n";
        }
        const std::string root = std::string(results_dir) + "/flow/";
        if (int rc = put(root + "cumulants_" + labels[s] + ".dat", c)) return rc;
        if (int rc = put(root + "multiplicity_" + labels[s] + ".dat", m)) return rc;
    }
    return IS3D_OK;
}
