// hbt_host.cpp -- the host side of the HBT correlation functions (include/is3d_amd.h): the list route is3d_hbt_list
// (THE definition: the explicit double loop over the ordered pairs of an (event, slot), through the one rule of cf_sampler_hbt.h), the
// radii from the exact integers, the writer, and the argument checks the device entries share.  No device use.
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_sampler_hbt.h"
#include "errors.h"

namespace is3d {

namespace {
int bins_error(const is3d_hbt_bins &b)
{
    return set_error(IS3D_EINVAL, "HBT bins: y_cut > 0, pT_max > pT_min >= 0, kT_max > kT_min >= 0, 1 <= n_kT <= 16, q_max > 0, 2 <= n_q <= 64 and "
                     "finite thresholds and widths are required (got y_cut = %g, pT in [%g, %g), kT in [%g, %g), n_kT = %d, q_max = %g, n_q = %d)",
                     b.y_cut, b.pT_min, b.pT_max, b.kT_min, b.kT_max, b.n_kT, b.q_max, b.n_q);
}
}  // namespace

int hbt_check_args(const is3d_hbt_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                   const is3d_hbt_hist *hist, bool device)
{
    if (!bins || !slot || !hist || !hist->num || !hist->den || !hist->M) return set_error(IS3D_EINVAL, "null argument");
    if (n_events < 1 || n_slots < 1 || n_species < 1)
        return set_error(IS3D_EINVAL, "HBT histograms: n_events, n_slots and n_species must be >= 1 (got %d, %d, %d)", n_events, n_slots, n_species);
    if (!hbt_bins_valid(*bins)) return bins_error(*bins);
    for (int32_t s = 0; s < n_species; s++)
        if (slot[s] < -1 || slot[s] >= n_slots) return set_error(IS3D_EINVAL, "slot[%d] = %d is outside [-1, %d)", s, slot[s], n_slots);
    if (device) {
        if (bins->kernel_form < 0 || bins->kernel_form > 2) return set_error(IS3D_EINVAL, "HBT bins: kernel_form = %d is not 0, 1 or 2", bins->kernel_form);
        if (bins->kernel_form == 2 && !hbt_private_fits(*bins))
            return set_error(IS3D_EINVAL, "HBT bins: kernel_form = 2 keeps one slot's n_kT x n_q^3 = %lld bins in LDS twice (den and num); at most %lld "
                             "64-bit word pairs fit beside the staged tile", (long long)hbt_slot_bins(*bins), (long long)kHbtPrivateWords);
    }
    return IS3D_OK;
}

void hbt_hist_zero(const is3d_hbt_bins &b, const is3d_hbt_hist *h, int32_t n_events, int32_t n_slots)
{
    const size_t words = (size_t)n_slots * (size_t)hbt_slot_bins(b);
    memset(h->num, 0, words * sizeof(int64_t));
    memset(h->den, 0, words * sizeof(int64_t));
    memset(h->M, 0, (size_t)n_events * n_slots * sizeof(int64_t));
}

int hbt_hist_check(const is3d_hbt_bins &b, const is3d_hbt_hist *h, int32_t n_slots)
{
    const size_t words = (size_t)n_slots * (size_t)hbt_slot_bins(b);
    for (size_t j = 0; j < words; j++)
        if (h->den[j] > IS3D_SAMPLER_VN_MAX_COUNT)
            return set_error(IS3D_EDOMAIN, "HBT histograms: bin %lld of slot %lld holds %lld pairs: the fixed-point numerator is exact up to %lld",
                             (long long)(j % (size_t)hbt_slot_bins(b)), (long long)(j / (size_t)hbt_slot_bins(b)), (long long)h->den[j],
                             (long long)IS3D_SAMPLER_VN_MAX_COUNT);
    return IS3D_OK;
}

}  // namespace is3d

using is3d::set_error;

extern "C" int is3d_hbt_list(const is3d_hbt_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                             int64_t n_particles, const is3d_particle *particles, const is3d_hbt_hist *hist)
{
    if (int rc = is3d::hbt_check_args(bins, n_events, n_slots, slot, n_species, hist, false)) return rc;
    if (n_particles < 0 || (n_particles > 0 && !particles)) return set_error(IS3D_EINVAL, "n_particles must be >= 0 and particles non-null");
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].species < 0 || particles[i].species >= n_species || particles[i].event < 0 || particles[i].event >= n_events)
            return set_error(IS3D_EINVAL, "particle %lld: species or event out of range", (long long)i);
    is3d::hbt_hist_zero(*bins, hist, n_events, n_slots);
    const is3d::HbtDerived d = is3d::hbt_derived(*bins);
    const int64_t block = is3d::hbt_slot_bins(*bins);
    // the accepted records per (event, slot), then every ordered pair of a segment
    std::vector<std::vector<is3d::HbtRecord>> seg((size_t)n_events * n_slots);
    for (int64_t i = 0; i < n_particles; i++) {
        const is3d_particle &q = particles[i];
        const int s = slot[q.species];
        if (s < 0 || !is3d::hbt_accept(*bins, d, q.E, q.px, q.py, q.pz)) continue;
        seg[(size_t)q.event * n_slots + (size_t)s].push_back(is3d::HbtRecord{q.E, q.px, q.py, q.pz, q.t, q.x, q.y, q.z});
        hist->M[(size_t)q.event * n_slots + (size_t)s] += 1;
    }
    for (size_t g = 0; g < seg.size(); g++) {
        const std::vector<is3d::HbtRecord> &r = seg[g];
        const int64_t s = (int64_t)(g % (size_t)n_slots);
        for (size_t i = 0; i < r.size(); i++)
            for (size_t j = 0; j < r.size(); j++) {
                if (i == j) continue;
                const int k = is3d::hbt_pair_bin(*bins, d, r[i], r[j]);
                if (k < 0) continue;
                hist->den[s * block + k] += 1;
                hist->num[s * block + k] += is3d::hbt_pair_term(r[i], r[j]);
            }
    }
    return IS3D_OK;
}

namespace {
// A x = b for the 7 unknowns, Gaussian elimination with partial pivoting in long double; false: singular
bool solve7(long double A[7][7], long double b[7], long double x[7])
{
    long double scale = 0.0L;
    for (int r = 0; r < 7; r++)
        for (int c = 0; c < 7; c++) scale = fmaxl(scale, fabsl(A[r][c]));
    if (!(scale > 0.0L) || !std::isfinite((double)scale)) return false;
    for (int k = 0; k < 7; k++) {
        int piv = k;
        for (int r = k + 1; r < 7; r++)
            if (fabsl(A[r][k]) > fabsl(A[piv][k])) piv = r;
        if (!(fabsl(A[piv][k]) > 1e-13L * scale)) return false;
        if (piv != k) {
            for (int c = 0; c < 7; c++) std::swap(A[k][c], A[piv][c]);
            std::swap(b[k], b[piv]);
        }
        for (int r = k + 1; r < 7; r++) {
            const long double f = A[r][k] / A[k][k];
            for (int c = k; c < 7; c++) A[r][c] -= f * A[k][c];
            b[r] -= f * b[k];
        }
    }
    for (int k = 6; k >= 0; k--) {
        long double s = b[k];
        for (int c = k + 1; c < 7; c++) s -= A[k][c] * x[c];
        x[k] = s / A[k][k];
    }
    return true;
}

int radii_check(const is3d_hbt_bins *bins, const is3d_hbt_hist *hist, int32_t n_slots, int64_t min_pairs, double c_min)
{
    if (!bins || !hist || !hist->num || !hist->den) return set_error(IS3D_EINVAL, "null argument");
    if (n_slots < 1) return set_error(IS3D_EINVAL, "HBT radii: n_slots must be >= 1 (got %d)", n_slots);
    if (!is3d::hbt_bins_valid(*bins)) return is3d::bins_error(*bins);
    if (min_pairs < 1 || !(c_min > 0.0)) return set_error(IS3D_EINVAL, "HBT radii: min_pairs >= 1 and c_min > 0 are required (got %lld, %g)", (long long)min_pairs, c_min);
    return IS3D_OK;
}
}  // namespace

extern "C" int is3d_hbt_radii(const is3d_hbt_bins *bins, const is3d_hbt_hist *hist, int32_t n_slots, int64_t min_pairs, double c_min,
                              is3d_hbt_radii_result *out)
{
    if (!out) return set_error(IS3D_EINVAL, "null argument");
    if (int rc = radii_check(bins, hist, n_slots, min_pairs, c_min)) return rc;
    const is3d::HbtDerived d = is3d::hbt_derived(*bins);
    const int nq = bins->n_q;
    const int64_t cube = (int64_t)nq * nq * nq;
    const long double h2 = (long double)is3d::kHbtHbarC * (long double)is3d::kHbtHbarC;
    for (int64_t g = 0; g < (int64_t)n_slots * bins->n_kT; g++) {
        const int64_t *num = hist->num + g * cube, *den = hist->den + g * cube;
        long double A[7][7], rhs[7], x[7];
        memset(A, 0, sizeof A);
        memset(rhs, 0, sizeof rhs);
        memset(x, 0, sizeof x);
        is3d_hbt_radii_result o;
        memset(&o, 0, sizeof o);
        for (int64_t k = 0; k < cube; k++) {
            if (den[k] < min_pairs) continue;
            const long double c = (long double)num[k] / ((long double)den[k] * 4294967296.0L);
            if (!(c >= (long double)c_min)) continue;
            const int io = (int)(k / ((int64_t)nq * nq)), is = (int)(k / nq % nq), il = (int)(k % nq);
            const long double qo = -(long double)bins->q_max + ((long double)io + 0.5L) * (long double)d.dq,
                              qs = -(long double)bins->q_max + ((long double)is + 0.5L) * (long double)d.dq,
                              ql = -(long double)bins->q_max + ((long double)il + 0.5L) * (long double)d.dq;
            const long double row[7] = {1.0L, -qo * qo / h2, -qs * qs / h2, -ql * ql / h2, -2.0L * qo * qs / h2, -2.0L * qo * ql / h2, -2.0L * qs * ql / h2};
            const long double w = (long double)den[k] * c * c, y = logl(c);
            for (int r = 0; r < 7; r++) {
                for (int cc = 0; cc < 7; cc++) A[r][cc] += w * row[r] * row[cc];
                rhs[r] += w * row[r] * y;
            }
            o.n_bins += 1;
        }
        if (o.n_bins >= 7 && solve7(A, rhs, x)) {
            o.lambda = (double)expl(x[0]);
            for (int r = 0; r < 6; r++) o.R2[r] = (double)x[r + 1];
        } else {
            o.singular = 1;
        }
        out[g] = o;
    }
    return IS3D_OK;
}

// <dir>/hbt/correlation_<label>_kT<k>.dat and radii_<label>.dat; doubles by std::to_chars(scientific, 8), integers in full
extern "C" int is3d_write_hbt(const char *results_dir, const is3d_hbt_bins *bins, const is3d_hbt_hist *hist, int32_t n_slots,
                              const char *const *labels, int64_t min_pairs, double c_min)
{
    if (!results_dir || !labels) return set_error(IS3D_EINVAL, "null argument");
    if (int rc = radii_check(bins, hist, n_slots, min_pairs, c_min)) return rc;
    for (int32_t s = 0; s < n_slots; s++)
        if (!labels[s] || !labels[s][0] || strchr(labels[s], '/')) return set_error(IS3D_EINVAL, "HBT writer: label %d is empty or holds a '/'", s);
    std::vector<is3d_hbt_radii_result> res((size_t)n_slots * bins->n_kT);
    if (int rc = is3d_hbt_radii(bins, hist, n_slots, min_pairs, c_min, res.data())) return rc;
    const auto num = [](std::string &out, double v) {
        char buf[40];
        const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific, 8);
        out.append(buf, (size_t)(r.ptr - buf));
    };
    const auto put = [](const std::string &path, const std::string &t) {
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) return set_error(IS3D_EIO, "cannot open %s (the hbt/ directory must exist)", path.c_str());
        const bool ok = fwrite(t.data(), 1, t.size(), f) == t.size();
        if (!(fclose(f) == 0 && ok)) return set_error(IS3D_EIO, "cannot write %s", path.c_str());
        return (int)IS3D_OK;
    };
    const is3d::HbtDerived d = is3d::hbt_derived(*bins);
    const int nq = bins->n_q;
    const int64_t cube = (int64_t)nq * nq * nq;
    const auto centre = [&](int k) { return -bins->q_max + ((double)k + 0.5) * d.dq; };
    for (int32_t s = 0; s < n_slots; s++) {
        std::string rt = "# kT\tlambda\tR2_out\tR2_side\tR2_long\tR2_os\tR2_ol\tR2_sl\tn_bins\tsingular; R2 in fm^2; min_pairs = " +
                         std::to_string((long long)min_pairs) + ", c_min = ";
        num(rt, c_min);
        rt += "\n";
        for (int k = 0; k < bins->n_kT; k++) {
            const int64_t g = (int64_t)s * bins->n_kT + k;
            const int64_t *hn = hist->num + g * cube, *hd = hist->den + g * cube;
            int64_t pairs = 0;
            for (int64_t j = 0; j < cube; j++) pairs += hd[j];
            std::string t = "# q_out\tq_side\tq_long\tden\tC; y_cut = ";
            num(t, bins->y_cut); t += ", pT in ["; num(t, bins->pT_min); t += ", "; num(t, bins->pT_max);
            t += "), q_max = "; num(t, bins->q_max); t += ", n_q = " + std::to_string(nq) + "\n# kT in [";
            num(t, bins->kT_min + (double)k * d.dkT); t += ", "; num(t, bins->kT_min + (double)(k + 1) * d.dkT);
            t += "), pairs: " + std::to_string((long long)pairs) + "\n";
            for (int64_t j = 0; j < cube; j++) {
                num(t, centre((int)(j / ((int64_t)nq * nq)))); t.push_back('\t');
                num(t, centre((int)(j / nq % nq))); t.push_back('\t');
                num(t, centre((int)(j % nq))); t.push_back('\t');
                t += std::to_string((long long)hd[j]) + "\t";
                num(t, hd[j] > 0 ? 1.0 + (double)((long double)hn[j] / ((long double)hd[j] * 4294967296.0L)) : 1.0);
                t.push_back('\n');
            }
            if (int rc = put(std::string(results_dir) + "/hbt/correlation_" + labels[s] + "_kT" + std::to_string(k) + ".dat", t)) return rc;
            const is3d_hbt_radii_result &o = res[(size_t)g];
            num(rt, bins->kT_min + ((double)k + 0.5) * d.dkT); rt.push_back('\t');
            num(rt, o.lambda);
            for (int r = 0; r < 6; r++) { rt.push_back('\t'); num(rt, o.R2[r]); }
            rt += "\t" + std::to_string(o.n_bins) + "\t" + std::to_string(o.singular) + "\n";
        }
        if (int rc = put(std::string(results_dir) + "/hbt/radii_" + labels[s] + ".dat", rt)) return rc;
    }
    return IS3D_OK;
}
