// pairs_host_check.cpp -- a stand-alone program for tools/sanitize_pairs_host.sh: the host entries of the pair correlations (pairs_host.cpp:
// is3d_pairs_list, is3d_pairs_correlation, is3d_write_pairs) and their refusals under AddressSanitizer + UBSan, with no Python, no preloaded
// runtime and no GPU.
// usage: pairs_host_check SCRATCH_DIR   (the directory must exist and be empty)
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

struct Hist {
    std::vector<int64_t> same, mixed, M;
    is3d_pair_hist view;
    Hist(const is3d_pair_bins &b, int events, int slots)
        : same((size_t)slots * (slots + 1) / 2 * (2 * b.n_y - 1) * b.n_phi), mixed(same.size()), M((size_t)events * slots),
          view{same.data(), mixed.data(), M.data()} {}
};

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s SCRATCH_DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    // ---- a list on both sides of every cut: the largest grid, the smallest, and an odd one ----
    const int n_events = 5, n_species = 7, n_slots = 3;
    std::vector<is3d_particle> p;
    unsigned long long state = 88172645463325252ULL;
    const auto uniform = [&state]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0; };
    const int sizes[n_events] = {0, 1, 2, 65, 130};
    for (int e = 0; e < n_events; e++)
        for (int k = 0; k < sizes[e]; k++) {
            const double y = -2.4 + 4.8 * uniform(), pT = 0.05 + 3.45 * uniform(), phi = -M_PI + 2.0 * M_PI * uniform(), mT = std::sqrt(0.0195 + pT * pT);
            is3d_particle q;
            memset(&q, 0, sizeof q);
            q.E = mT * std::cosh(y); q.pz = mT * std::sinh(y); q.px = pT * std::cos(phi); q.py = pT * std::sin(phi);
            q.event = e; q.species = (int)(uniform() * n_species) % n_species;
            p.push_back(q);
        }
    // the axes, pT = 0, E = pz, NaN
    for (int k = 0; k < 7; k++) {
        is3d_particle q;
        memset(&q, 0, sizeof q);
        q.E = 1.0; q.event = 4; q.species = 1;
        const double ax[7][3] = {{1, 0, 0}, {0, 1, 0}, {-1, 0, 0}, {0, -1, 0}, {0, 0, 0}, {0.5, 0.5, 1.0}, {0.5, std::numeric_limits<double>::quiet_NaN(), 0}};
        q.px = ax[k][0]; q.py = ax[k][1]; q.pz = ax[k][2];
        p.push_back(q);
    }
    const int32_t slot[n_species] = {0, 1, 2, -1, 0, 1, 2};
    const is3d_pair_bins shapes[3] = {{2.0, 0.2, 3.0, 64, 64}, {2.0, 0.2, 3.0, 1, 4}, {2.0, 0.0, 3.0, 33, 20}};
    for (const is3d_pair_bins &b : shapes) {
        Hist h(b, n_events, n_slots);
        EXPECT(is3d_pairs_list(&b, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_OK);
        for (int a = 0; a < n_slots; a++)
            for (int c = a; c < n_slots; c++) {                          // the sum rules
                const size_t cls = (size_t)(a * n_slots - a * (a - 1) / 2 + (c - a)), nb = (size_t)(2 * b.n_y - 1) * b.n_phi;
                int64_t same = 0, mixed = 0, want_same = 0, want_mixed = 0;
                for (size_t k = 0; k < nb; k++) { same += h.same[cls * nb + k]; mixed += h.mixed[cls * nb + k]; }
                for (int e = 0; e < n_events; e++) {
                    want_same += h.M[e * n_slots + a] * h.M[e * n_slots + c] - (a == c ? h.M[e * n_slots + a] : 0);
                    want_mixed += h.M[e * n_slots + a] * h.M[((e + 1) % n_events) * n_slots + c];
                }
                EXPECT(same == want_same && mixed == want_mixed && same > 0);
            }
        const size_t n_classes = n_slots * (n_slots + 1) / 2;
        std::vector<double> C(h.same.size()), C_phi(n_classes * b.n_phi);
        std::vector<is3d_pair_result> res(n_classes);
        for (int gap = 0; gap < b.n_y; gap += 7)
            EXPECT(is3d_pairs_correlation(&b, &h.view, n_slots, gap, C.data(), C_phi.data(), res.data()) == IS3D_OK);
        EXPECT(is3d_pairs_correlation(&b, &h.view, n_slots, 0, nullptr, nullptr, res.data()) == IS3D_OK);
        EXPECT(is3d_pairs_correlation(&b, &h.view, n_slots, b.n_y, C.data(), C_phi.data(), res.data()) == IS3D_EINVAL);
        EXPECT(is3d_pairs_correlation(&b, &h.view, n_slots, -1, C.data(), C_phi.data(), res.data()) == IS3D_EINVAL);
        // the writer: no directory, then every class
        const char *labels[n_slots] = {"211", "-211", "other"};
        const std::string root = dir + "/" + std::to_string(b.n_y);
        EXPECT(mkdir(root.c_str(), 0777) == 0);
        EXPECT(is3d_write_pairs(root.c_str(), &b, &h.view, n_slots, labels) == IS3D_EIO);
        EXPECT(mkdir((root + "/pairs").c_str(), 0777) == 0);
        EXPECT(is3d_write_pairs(root.c_str(), &b, &h.view, n_slots, labels) == IS3D_OK);
        const char *bad[n_slots] = {"211", "", "a/b"};
        EXPECT(is3d_write_pairs(root.c_str(), &b, &h.view, n_slots, bad) == IS3D_EINVAL);
        EXPECT(is3d_write_pairs(nullptr, &b, &h.view, n_slots, labels) == IS3D_EINVAL);
        EXPECT(is3d_write_pairs(root.c_str(), &b, &h.view, 0, labels) == IS3D_EINVAL);
        // one event: no mixed pairs
        Hist one(b, 1, n_slots);
        std::vector<is3d_particle> first(p.begin() + 3, p.begin() + 68);
        for (is3d_particle &q : first) q.event = 0;
        EXPECT(is3d_pairs_list(&b, 1, n_slots, slot, n_species, (int64_t)first.size(), first.data(), &one.view) == IS3D_OK);
        int64_t m = 0;
        for (int64_t v : one.mixed) m += v;
        EXPECT(m == 0);
    }
    // ---- refusals ----
    const is3d_pair_bins good = shapes[2];
    Hist h(good, n_events, n_slots);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const is3d_pair_bins bad_bins[] = {{0.0, 0.2, 3.0, 8, 8}, {nan, 0.2, 3.0, 8, 8}, {2.0, -0.1, 3.0, 8, 8}, {2.0, 0.2, 0.2, 8, 8}, {2.0, 0.2, nan, 8, 8},
                                       {2.0, 0.2, 3.0, 0, 8}, {2.0, 0.2, 3.0, 65, 8}, {2.0, 0.2, 3.0, 8, 0}, {2.0, 0.2, 3.0, 8, 6}, {2.0, 0.2, 3.0, 8, 68},
                                       {2.0, 0.2, 3.0, -2147483647 - 1, 2147483647}, {400.0, 0.2, 3.0, 8, 8}, {1e-300, 0.2, 3.0, 64, 8}};
    for (const is3d_pair_bins &b : bad_bins) {
        EXPECT(is3d_pairs_list(&b, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
        is3d_pair_result r;
        EXPECT(is3d_pairs_correlation(&b, &h.view, 1, 0, nullptr, nullptr, &r) == IS3D_EINVAL);
        const char *l[1] = {"x"};
        EXPECT(is3d_write_pairs(dir.c_str(), &b, &h.view, 1, l) == IS3D_EINVAL);
    }
    EXPECT(is3d_pairs_list(nullptr, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
    EXPECT(is3d_pairs_list(&good, n_events, n_slots, nullptr, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
    EXPECT(is3d_pairs_list(&good, n_events, n_slots, slot, n_species, (int64_t)p.size(), nullptr, &h.view) == IS3D_EINVAL);
    EXPECT(is3d_pairs_list(&good, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), nullptr) == IS3D_EINVAL);
    EXPECT(is3d_pairs_list(&good, 0, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
    EXPECT(is3d_pairs_list(&good, n_events, 0, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
    EXPECT(is3d_pairs_list(&good, n_events, 2, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);     // slot 2 of 2
    EXPECT(is3d_pairs_list(&good, n_events, n_slots, slot, n_species, -1, p.data(), &h.view) == IS3D_EINVAL);
    EXPECT(is3d_pairs_list(&good, n_events, n_slots, slot, 3, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);       // species 3.. out of range
    EXPECT(is3d_pairs_list(&good, 4, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);       // event 4 out of range
    EXPECT(is3d_pairs_list(&good, n_events, n_slots, slot, n_species, 0, nullptr, &h.view) == IS3D_OK);                     // an empty list
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("pairs_host_check: ok\n");
    return 0;
}
