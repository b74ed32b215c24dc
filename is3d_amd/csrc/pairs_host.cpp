// pairs_host.cpp -- the host side of the two-particle (delta y, delta phi) correlations (include/is3d_amd.h): the list
// route is3d_pairs_list (THE definition: the explicit double loop over the pairs of an event, through the one rule of cf_sampler_pairs.h),
// the correlation function from the exact integers, the writer, and the argument checks and plumbing the device entries share.
// No device use.
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_sampler_pairs.h"
#include "errors.h"

namespace is3d {

namespace {
int bins_error(const is3d_pair_bins &b)
{
    return set_error(IS3D_EINVAL, "pair bins: y_cut > 0, pT_max > pT_min >= 0, 1 <= n_y <= 64, n_phi a multiple of 4 in 4..64 and finite, increasing "
                     "rapidity edges are required (got y_cut = %g, pT in [%g, %g), n_y = %d, n_phi = %d)", b.y_cut, b.pT_min, b.pT_max, b.n_y, b.n_phi);
}
}  // namespace

int pair_check_args(const is3d_pair_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                    const is3d_pair_hist *hist)
{
    if (!bins || !slot || !hist || !hist->same || !hist->mixed || !hist->M) return set_error(IS3D_EINVAL, "null argument");
    if (n_events < 1 || n_slots < 1 || n_species < 1)
        return set_error(IS3D_EINVAL, "pair histograms: n_events, n_slots and n_species must be >= 1 (got %d, %d, %d)", n_events, n_slots, n_species);
    if (!pair_bins_valid(*bins)) return bins_error(*bins);
    for (int32_t s = 0; s < n_species; s++)
        if (slot[s] < -1 || slot[s] >= n_slots) return set_error(IS3D_EINVAL, "slot[%d] = %d is outside [-1, %d)", s, slot[s], n_slots);
    return IS3D_OK;
}

void pair_hist_zero(const is3d_pair_bins &b, const is3d_pair_hist *h, int32_t n_events, int32_t n_slots)
{
    const size_t words = (size_t)pair_classes(n_slots) * (size_t)pair_hist_bins(b);
    memset(h->same, 0, words * sizeof(int64_t));
    memset(h->mixed, 0, words * sizeof(int64_t));
    memset(h->M, 0, (size_t)n_events * n_slots * sizeof(int64_t));
}

void pair_hist_scatter(const is3d_pair_bins &b, const int64_t *block, const is3d_pair_hist *h, int32_t n_events, int32_t n_slots)
{
    const size_t words = (size_t)pair_classes(n_slots) * (size_t)pair_hist_bins(b);
    memcpy(h->same, block, words * sizeof(int64_t));
    memcpy(h->mixed, block + words, words * sizeof(int64_t));
    memcpy(h->M, block + 2 * words, (size_t)n_events * n_slots * sizeof(int64_t));
}

int pair_hist_check(const is3d_pair_hist *h, int32_t n_events, int32_t n_slots)
{
    for (size_t j = 0; j < (size_t)n_events * n_slots; j++)
        if (h->M[j] > IS3D_SAMPLER_VN_MAX_COUNT)
            return set_error(IS3D_EDOMAIN, "pair histograms: (event %lld, slot %lld) holds %lld accepted hadrons: the 32-bit occupancies are exact up to %lld",
                             (long long)(j / (size_t)n_slots), (long long)(j % (size_t)n_slots), (long long)h->M[j], (long long)IS3D_SAMPLER_VN_MAX_COUNT);
    return IS3D_OK;
}

}  // namespace is3d

using is3d::set_error;

namespace {
struct Accepted { int32_t slot, iy, iphi; };

// every ordered pair (i of a, j of b), slot_i <= slot_j; same: a and b are one event's list and i != j
void add_pairs(const is3d_pair_bins &bn, int32_t n_slots, const std::vector<Accepted> &a, const std::vector<Accepted> &b, bool same, int64_t *out)
{
    const int64_t bins = is3d::pair_hist_bins(bn);
    for (size_t i = 0; i < a.size(); i++)
        for (size_t j = 0; j < b.size(); j++) {
            if ((same && i == j) || a[i].slot > b[j].slot) continue;
            const int dy = b[j].iy - a[i].iy + bn.n_y - 1;
            int dphi = b[j].iphi - a[i].iphi;
            if (dphi < 0) dphi += bn.n_phi;
            out[is3d::pair_class(a[i].slot, b[j].slot, n_slots) * bins + (int64_t)dy * bn.n_phi + dphi] += 1;
        }
}
}  // namespace

extern "C" int is3d_pairs_list(const is3d_pair_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                               int64_t n_particles, const is3d_particle *particles, const is3d_pair_hist *hist)
{
    if (int rc = is3d::pair_check_args(bins, n_events, n_slots, slot, n_species, hist)) return rc;
    if (n_particles < 0 || (n_particles > 0 && !particles)) return set_error(IS3D_EINVAL, "n_particles must be >= 0 and particles non-null");
    for (int64_t i = 0; i < n_particles; i++)
        if (particles[i].species < 0 || particles[i].species >= n_species || particles[i].event < 0 || particles[i].event >= n_events)
            return set_error(IS3D_EINVAL, "particle %lld: species or event out of range", (long long)i);
    is3d::pair_hist_zero(*bins, hist, n_events, n_slots);
    const is3d::PairTables t = is3d::pair_tables(*bins);
    std::vector<std::vector<Accepted>> ev((size_t)n_events);
    for (int64_t i = 0; i < n_particles; i++) {
        const is3d_particle &q = particles[i];
        const int s = slot[q.species];
        if (s < 0) continue;
        const int cell = is3d::pair_cell(*bins, t, q.E, q.px, q.py, q.pz);
        if (cell < 0) continue;
        ev[(size_t)q.event].push_back(Accepted{s, cell / bins->n_phi, cell % bins->n_phi});
        hist->M[(size_t)q.event * n_slots + (size_t)s] += 1;
    }
    for (int32_t e = 0; e < n_events; e++) {
        add_pairs(*bins, n_slots, ev[(size_t)e], ev[(size_t)e], true, hist->same);
        if (n_events >= 2) add_pairs(*bins, n_slots, ev[(size_t)e], ev[(size_t)((e + 1) % n_events)], false, hist->mixed);
    }
    return IS3D_OK;
}

extern "C" int is3d_pairs_correlation(const is3d_pair_bins *bins, const is3d_pair_hist *hist, int32_t n_slots, int32_t gap_bins, double *C,
                                      double *C_phi, is3d_pair_result *out)
{
    if (!bins || !hist || !hist->same || !hist->mixed || !out) return set_error(IS3D_EINVAL, "null argument");
    if (n_slots < 1) return set_error(IS3D_EINVAL, "pair correlation: n_slots must be >= 1 (got %d)", n_slots);
    if (!is3d::pair_bins_valid(*bins)) return is3d::bins_error(*bins);
    if (gap_bins < 0 || gap_bins >= bins->n_y) return set_error(IS3D_EINVAL, "gap_bins = %d is outside [0, %d)", gap_bins, bins->n_y);
    const int64_t nb = is3d::pair_hist_bins(*bins), n_classes = is3d::pair_classes(n_slots);
    const int n_phi = bins->n_phi, rows = 2 * bins->n_y - 1;
    for (int64_t c = 0; c < n_classes; c++) {
        const int64_t *same = hist->same + c * nb, *mixed = hist->mixed + c * nb;
        is3d_pair_result o;
        memset(&o, 0, sizeof o);
        for (int64_t k = 0; k < nb; k++) { o.n_same += same[k]; o.n_mixed += mixed[k]; }
        const double ns = (double)o.n_same, nm = (double)o.n_mixed;
        if (C)
            for (int64_t k = 0; k < nb; k++)
                C[c * nb + k] = mixed[k] > 0 && o.n_same > 0 ? ((double)same[k] / ns) / ((double)mixed[k] / nm) : 0.0;
        double sum = 0.0, num[4] = {0.0, 0.0, 0.0, 0.0};
        for (int p = 0; p < n_phi; p++) {
            int64_t s = 0, m = 0;
            for (int r = 0; r < rows; r++) {
                const int d = r - (bins->n_y - 1);
                if ((d < 0 ? -d : d) < gap_bins) continue;
                s += same[(int64_t)r * n_phi + p];
                m += mixed[(int64_t)r * n_phi + p];
            }
            const double v = m > 0 && o.n_same > 0 ? ((double)s / ns) / ((double)m / nm) : 0.0;
            if (C_phi) C_phi[c * n_phi + p] = v;
            sum += v;
            for (int n = 1; n <= 4; n++) num[n - 1] += v * cos(2.0 * M_PI * (double)n * (double)p / (double)n_phi);
        }
        for (int n = 0; n < 4; n++) o.V[n] = sum != 0.0 ? num[n] / sum : 0.0;
        out[c] = o;
    }
    return IS3D_OK;
}

// <dir>/pairs/correlation_<A>_<B>.dat per class; doubles by std::to_chars(scientific, 8) as the other writers' values, integers in full
extern "C" int is3d_write_pairs(const char *results_dir, const is3d_pair_bins *bins, const is3d_pair_hist *hist, int32_t n_slots,
                                const char *const *labels)
{
    if (!results_dir || !labels || !bins || !hist || !hist->same || !hist->mixed) return set_error(IS3D_EINVAL, "null argument");
    if (n_slots < 1) return set_error(IS3D_EINVAL, "pair writer: n_slots must be >= 1 (got %d)", n_slots);
    if (!is3d::pair_bins_valid(*bins)) return is3d::bins_error(*bins);
    for (int32_t s = 0; s < n_slots; s++)
        if (!labels[s] || !labels[s][0] || strchr(labels[s], '/')) return set_error(IS3D_EINVAL, "pair writer: label %d is empty or holds a '/'", s);
    const int64_t nb = is3d::pair_hist_bins(*bins), n_classes = is3d::pair_classes(n_slots);
    std::vector<double> C((size_t)(n_classes * nb));
    std::vector<is3d_pair_result> res((size_t)n_classes);
    if (int rc = is3d_pairs_correlation(bins, hist, n_slots, 0, C.data(), nullptr, res.data())) return rc;
    const auto num = [](std::string &out, double v) {
        char buf[40];
        const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific, 8);
        out.append(buf, (size_t)(r.ptr - buf));
    };
    const double yw = 2.0 * bins->y_cut / (double)bins->n_y, pw = 2.0 * M_PI / (double)bins->n_phi;
    for (int32_t a = 0; a < n_slots; a++)
        for (int32_t b = a; b < n_slots; b++) {
            const int64_t c = is3d::pair_class(a, b, n_slots);
            std::string t = "# delta_y\tdelta_phi\tsame\tmixed\tC; y_cut = ";
            num(t, bins->y_cut); t += ", pT in ["; num(t, bins->pT_min); t += ", "; num(t, bins->pT_max);
            t += "), n_y = " + std::to_string(bins->n_y) + ", n_phi = " + std::to_string(bins->n_phi) + "\n";
            t += "# n_same: " + std::to_string((long long)res[(size_t)c].n_same) + ", n_mixed: " + std::to_string((long long)res[(size_t)c].n_mixed) + "\n";
            for (int r = 0; r < 2 * bins->n_y - 1; r++)
                for (int p = 0; p < bins->n_phi; p++) {
                    const int64_t k = c * nb + (int64_t)r * bins->n_phi + p;
                    num(t, (double)(r - (bins->n_y - 1)) * yw); t.push_back('\t');
                    num(t, (double)p * pw); t.push_back('\t');
                    t += std::to_string((long long)hist->same[k]) + "\t" + std::to_string((long long)hist->mixed[k]) + "\t";
                    num(t, C[(size_t)k]);
                    t.push_back('\n');
                }
            const std::string path = std::string(results_dir) + "/pairs/correlation_" + labels[a] + "_" + labels[b] + ".dat";
            FILE *f = fopen(path.c_str(), "wb");
            if (!f) return set_error(IS3D_EIO, "cannot open %s (the pairs/ directory must exist)", path.c_str());
            const bool ok = fwrite(t.data(), 1, t.size(), f) == t.size();
            if (!(fclose(f) == 0 && ok)) return set_error(IS3D_EIO, "cannot write %s", path.c_str());
        }
    return IS3D_OK;
}
