// flow_diff_host_check.cpp -- a stand-alone program for tools/sanitize_flow_diff_host.sh: the host entries of the differential flow
// (flow_diff_host.cpp: is3d_flow_diff_list, is3d_flow_diff_reference, is3d_flow_diff_cumulants, is3d_write_flow_diff) and their refusals under
// AddressSanitizer + UBSan, with no Python, no preloaded runtime and no GPU.
// usage: flow_diff_host_check SCRATCH_DIR   (the directory must exist and be empty)
#include <sys/stat.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/is3d_amd.h"

static int failures = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "line %d: %s -- last error: %s\n", __LINE__, #cond, is3d_last_error()); failures++; } \
    } while (0)

// exactly the words the entries may touch: any step past them is the sanitizer's to find
struct Rec {
    std::vector<int64_t> m, re, im;
    is3d_flow_diff_records view;
    Rec(int events, int slots, int bins)
        : m((size_t)events * slots * bins * 3), re(m.size() * IS3D_FLOW_HARMONICS), im(re.size()), view{m.data(), re.data(), im.data()} {}
};

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s SCRATCH_DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const int n_events = 6, n_species = 7, n_slots = 3;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- a list on both sides of every cut and every edge, an empty event, and momenta no rule should trip over ----
    std::vector<is3d_particle> p;
    unsigned long long state = 88172645463325252ULL;
    const auto uniform = [&state]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0; };
    const int sizes[n_events] = {0, 1, 4, 9, 65, 130};
    for (int e = 0; e < n_events; e++)
        for (int k = 0; k < sizes[e]; k++) {
            is3d_particle q;
            memset(&q, 0, sizeof q);
            const double pT = 0.05 + 3.5 * uniform(), phi = 6.283185307179586 * uniform(), y = 3.0 * (uniform() - 0.5);
            const double mT = std::sqrt(0.0195 + pT * pT);
            q.px = pT * std::cos(phi); q.py = pT * std::sin(phi); q.pz = mT * std::sinh(y); q.E = mT * std::cosh(y);
            q.event = e; q.species = (int)(uniform() * n_species) % n_species;
            p.push_back(q);
        }
    const double edges[6] = {0.2, 0.25, 0.7, 1.0, 2.0, 3.0};
    const int n_pT = 5;
    const double odd[10][4] = {{1, 0.2, 0, 0.1}, {1, 0, 3.0, 0.1}, {1, 0, -1.0, 0.1}, {1, 0, 0, 0.5}, {1, 0, 0, 1}, {1, 0.5, nan, 0}, {inf, 0.3, 0.2, 0.1},
                               {1, 0.3, 0.2, -inf}, {nan, 0.3, 0.2, 0.1}, {1, inf, 0.2, 0.1}};
    for (int k = 0; k < 10; k++) {
        is3d_particle q;
        memset(&q, 0, sizeof q);
        q.E = odd[k][0]; q.px = odd[k][1]; q.py = odd[k][2]; q.pz = odd[k][3];
        q.event = 5; q.species = 1;
        p.push_back(q);
    }
    const int32_t slot[n_species] = {0, 1, 2, -1, 0, 1, 2};
    const is3d_flow_cuts cuts{1.0, 0.5, edges[0], edges[n_pT], 0};
    Rec r(n_events, n_slots, n_pT);
    EXPECT(is3d_flow_diff_list(&cuts, n_pT, edges, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &r.view) == IS3D_OK);
    // the sum rule against is3d_flow_list
    {
        std::vector<int64_t> M((size_t)n_events * n_slots * 3), re(M.size() * IS3D_FLOW_HARMONICS), im(re.size());
        const is3d_flow_records f{M.data(), re.data(), im.data()};
        EXPECT(is3d_flow_list(&cuts, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &f) == IS3D_OK);
        int64_t total = 0;
        for (int e = 0; e < n_events; e++)
            for (int s = 0; s < n_slots; s++)
                for (int g = 0; g < 3; g++) {
                    int64_t sum = 0, sum_re = 0;
                    for (int b = 0; b < n_pT; b++) {
                        const size_t j = (((size_t)e * n_slots + s) * n_pT + b) * 3 + g;
                        sum += r.m[j];
                        sum_re += r.re[j * IS3D_FLOW_HARMONICS + 1];
                    }
                    const size_t k = ((size_t)e * n_slots + s) * 3 + g;
                    EXPECT(sum == M[k] && sum_re == re[k * IS3D_FLOW_HARMONICS + 1]);
                    if (g == 0) total += sum;
                }
        EXPECT(total > 60);
    }
    // the largest and the smallest tables, an empty list
    {
        std::vector<double> e64(IS3D_FLOW_DIFF_MAX_BINS + 1);
        for (int k = 0; k <= IS3D_FLOW_DIFF_MAX_BINS; k++) e64[k] = 0.05 * k;
        const is3d_flow_cuts c64{1.0, 0.5, e64.front(), e64.back(), 0};
        Rec big(n_events, n_slots, IS3D_FLOW_DIFF_MAX_BINS), one(n_events, n_slots, 1);
        EXPECT(is3d_flow_diff_list(&c64, IS3D_FLOW_DIFF_MAX_BINS, e64.data(), n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &big.view) == IS3D_OK);
        const double e1[2] = {0.2, 3.0};
        EXPECT(is3d_flow_diff_list(&cuts, 1, e1, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &one.view) == IS3D_OK);
        EXPECT(is3d_flow_diff_list(&cuts, 1, e1, n_events, n_slots, slot, n_species, 0, nullptr, &one.view) == IS3D_OK);
        std::vector<is3d_flow_diff_result> res((size_t)n_slots * IS3D_FLOW_DIFF_MAX_BINS);
        const int32_t every[n_slots] = {1, 1, 1};
        EXPECT(is3d_flow_diff_cumulants(&big.view, n_events, n_slots, IS3D_FLOW_DIFF_MAX_BINS, every, 0, IS3D_FLOW_DIFF_MAX_BINS, res.data()) == IS3D_OK);
        EXPECT(is3d_flow_diff_cumulants(&one.view, n_events, n_slots, 1, every, 0, 1, res.data()) == IS3D_OK);
    }
    // ---- the reference and the cumulants: all of it, a part of it, one bin of one slot ----
    std::vector<int64_t> M((size_t)n_events * 3), re(M.size() * IS3D_FLOW_HARMONICS), im(re.size());
    const is3d_flow_records ref{M.data(), re.data(), im.data()};
    std::vector<is3d_flow_diff_result> res((size_t)n_slots * n_pT);
    const int32_t refs[3][n_slots] = {{1, 1, 1}, {1, 0, 1}, {0, 1, 0}};
    const int range[3][2] = {{0, n_pT}, {1, 4}, {4, 5}};
    for (int k = 0; k < 3; k++) {
        EXPECT(is3d_flow_diff_reference(&r.view, n_events, n_slots, n_pT, refs[k], range[k][0], range[k][1], &ref) == IS3D_OK);
        EXPECT(is3d_flow_diff_cumulants(&r.view, n_events, n_slots, n_pT, refs[k], range[k][0], range[k][1], res.data()) == IS3D_OK);
        for (const is3d_flow_diff_result &o : res) {
            EXPECT(o.n_events == n_events && o.n_used_2 <= n_events && o.n_used_4 <= o.n_used_2);
            for (int m = 0; m < IS3D_FLOW_HARMONICS; m++)
                EXPECT(std::isfinite(o.d2[m]) && std::isfinite(o.v2[m]) && std::isfinite(o.d2_gap[m]) && std::isfinite(o.v2_gap[m]) && std::isfinite(o.v_rp[m]));
            for (int m = 0; m < 4; m++) EXPECT(std::isfinite(o.avg4[m]) && std::isfinite(o.d4[m]) && std::isfinite(o.v4[m]));
        }
    }
    // ---- the writer ----
    const char *labels[n_slots] = {"211", "321", "other"};
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, n_events, n_slots, n_pT, edges, refs[0], 0, n_pT, labels) == IS3D_EIO);   // no flow/ yet
    mkdir((dir + "/flow").c_str(), 0755);
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, n_events, n_slots, n_pT, edges, refs[0], 0, n_pT, labels) == IS3D_OK);
    for (const char *l : labels) {
        struct stat sb;
        EXPECT(stat((dir + "/flow/differential_" + l + ".dat").c_str(), &sb) == 0 && sb.st_size > 0);
    }
    const char *empty[n_slots] = {"211", "", "x"}, *slash[n_slots] = {"211", "a/b", "x"}, *null_l[n_slots] = {"211", nullptr, "x"};
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, n_events, n_slots, n_pT, edges, refs[0], 0, n_pT, empty) == IS3D_EINVAL);
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, n_events, n_slots, n_pT, edges, refs[0], 0, n_pT, slash) == IS3D_EINVAL);
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, n_events, n_slots, n_pT, edges, refs[0], 0, n_pT, null_l) == IS3D_EINVAL);
    EXPECT(is3d_write_flow_diff(nullptr, &r.view, n_events, n_slots, n_pT, edges, refs[0], 0, n_pT, labels) == IS3D_EINVAL);
    EXPECT(is3d_write_flow_diff(dir.c_str(), nullptr, n_events, n_slots, n_pT, edges, refs[0], 0, n_pT, labels) == IS3D_EINVAL);
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, n_events, n_slots, n_pT, nullptr, refs[0], 0, n_pT, labels) == IS3D_EINVAL);
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, n_events, n_slots, n_pT, edges, nullptr, 0, n_pT, labels) == IS3D_EINVAL);
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, n_events, n_slots, n_pT, edges, refs[0], 0, n_pT, nullptr) == IS3D_EINVAL);
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, 0, n_slots, n_pT, edges, refs[0], 0, n_pT, labels) == IS3D_EINVAL);
    EXPECT(is3d_write_flow_diff(dir.c_str(), &r.view, n_events, n_slots, n_pT, edges, refs[0], 2, 2, labels) == IS3D_EINVAL);
    // ---- every refusal of the list entry ----
    const auto list = [&](const is3d_flow_cuts *c, int32_t nb, const double *e, int32_t ne, int32_t ns, const int32_t *sl, int32_t nsp, int64_t n,
                          const is3d_particle *q, const is3d_flow_diff_records *rec) { return is3d_flow_diff_list(c, nb, e, ne, ns, sl, nsp, n, q, rec); };
    const int64_t N = (int64_t)p.size();
    EXPECT(list(nullptr, n_pT, edges, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, n_pT, nullptr, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, n_pT, edges, n_events, n_slots, nullptr, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, n_pT, edges, n_events, n_slots, slot, n_species, N, nullptr, &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, n_pT, edges, n_events, n_slots, slot, n_species, N, p.data(), nullptr) == IS3D_EINVAL);
    const is3d_flow_diff_records holes[3] = {{nullptr, r.re.data(), r.im.data()}, {r.m.data(), nullptr, r.im.data()}, {r.m.data(), r.re.data(), nullptr}};
    for (const is3d_flow_diff_records &h : holes) EXPECT(list(&cuts, n_pT, edges, n_events, n_slots, slot, n_species, N, p.data(), &h) == IS3D_EINVAL);
    EXPECT(list(&cuts, 0, edges, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, IS3D_FLOW_DIFF_MAX_BINS + 1, edges, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, n_pT, edges, 0, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, n_pT, edges, n_events, 0, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, n_pT, edges, n_events, n_slots, slot, 0, N, p.data(), &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, n_pT, edges, n_events, n_slots, slot, n_species, -1, p.data(), &r.view) == IS3D_EINVAL);
    EXPECT(list(&cuts, n_pT, edges, n_events, 2, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);             // slot 2 of 2
    EXPECT(list(&cuts, n_pT, edges, 5, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);              // a particle of event 5
    EXPECT(list(&cuts, n_pT, edges, n_events, n_slots, slot, 6, N, p.data(), &r.view) == IS3D_EINVAL);               // a particle of species 6
    const double bad_edges[5][6] = {{0.2, 0.25, 0.25, 1.0, 2.0, 3.0}, {0.2, 0.7, 0.25, 1.0, 2.0, 3.0}, {0.2, 0.25, nan, 1.0, 2.0, 3.0},
                                    {-0.1, 0.25, 0.7, 1.0, 2.0, 3.0}, {0.2, 0.25, 0.7, 1.0, 2.0, inf}};
    for (const auto &e : bad_edges) {
        const is3d_flow_cuts c{1.0, 0.5, e[0], e[n_pT], 0};
        EXPECT(list(&c, n_pT, e, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    }
    is3d_flow_cuts c = cuts;
    c.pT_min = std::nextafter(edges[0], 1.0);
    EXPECT(list(&c, n_pT, edges, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    c = cuts; c.pT_max = std::nextafter(edges[n_pT], 0.0);
    EXPECT(list(&c, n_pT, edges, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    c = cuts; c.y_cut = 0.0;
    EXPECT(list(&c, n_pT, edges, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    c = cuts; c.y_gap = 2.0;
    EXPECT(list(&c, n_pT, edges, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    c = cuts; c.kernel_form = 3;
    EXPECT(list(&c, n_pT, edges, n_events, n_slots, slot, n_species, N, p.data(), &r.view) == IS3D_EINVAL);
    // ---- ... of the reference and the cumulants ----
    const int32_t two[n_slots] = {1, 2, 0};
    EXPECT(is3d_flow_diff_reference(nullptr, n_events, n_slots, n_pT, refs[0], 0, n_pT, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, n_events, n_slots, n_pT, nullptr, 0, n_pT, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, n_events, n_slots, n_pT, refs[0], 0, n_pT, nullptr) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, n_events, n_slots, n_pT, two, 0, n_pT, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, n_events, n_slots, n_pT, refs[0], -1, n_pT, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, n_events, n_slots, n_pT, refs[0], 0, n_pT + 1, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, n_events, n_slots, n_pT, refs[0], 3, 3, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, 0, n_slots, n_pT, refs[0], 0, n_pT, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, n_events, 0, n_pT, refs[0], 0, n_pT, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, n_events, n_slots, 0, refs[0], 0, 0, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_reference(&r.view, n_events, n_slots, IS3D_FLOW_DIFF_MAX_BINS + 1, refs[0], 0, 1, &ref) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_cumulants(nullptr, n_events, n_slots, n_pT, refs[0], 0, n_pT, res.data()) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_cumulants(&r.view, n_events, n_slots, n_pT, refs[0], 0, n_pT, nullptr) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_cumulants(&r.view, n_events, n_slots, n_pT, two, 0, n_pT, res.data()) == IS3D_EINVAL);
    EXPECT(is3d_flow_diff_cumulants(&r.view, n_events, n_slots, n_pT, refs[0], 4, 3, res.data()) == IS3D_EINVAL);
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("flow_diff_host_check: all checks passed\n");
    return 0;
}
