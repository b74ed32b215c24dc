// hbt_host_check.cpp -- a stand-alone program for tools/sanitize_hbt_host.sh: the host entries of the HBT correlation functions (hbt_host.cpp:
// is3d_hbt_list, is3d_hbt_radii, is3d_write_hbt) and their refusals under AddressSanitizer + UBSan, with no Python, no preloaded runtime and
// no GPU.
// usage: hbt_host_check SCRATCH_DIR   (the directory must exist and be empty)
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
    std::vector<int64_t> num, den, M;
    is3d_hbt_hist view;
    Hist(const is3d_hbt_bins &b, int events, int slots)
        : num((size_t)slots * b.n_kT * b.n_q * b.n_q * b.n_q), den(num.size()), M((size_t)events * slots), view{num.data(), den.data(), M.data()} {}
};

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s SCRATCH_DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    // ---- a list on both sides of every cut, clustered so that pairs land inside the q cube ----
    const int n_events = 5, n_species = 7, n_slots = 3;
    std::vector<is3d_particle> p;
    unsigned long long state = 88172645463325252ULL;
    const auto uniform = [&state]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0; };
    const int sizes[n_events] = {0, 1, 2, 65, 130};
    for (int e = 0; e < n_events; e++)
        for (int k = 0; k < sizes[e]; k++) {
            is3d_particle q;
            memset(&q, 0, sizeof q);
            q.px = 0.3 + 0.2 * (uniform() - 0.5); q.py = 0.1 + 0.2 * (uniform() - 0.5); q.pz = 1.2 * (uniform() - 0.5);
            q.E = std::sqrt(0.0195 + q.px * q.px + q.py * q.py + q.pz * q.pz);
            q.t = 5.0 * uniform(); q.x = 6.0 * (uniform() - 0.5); q.y = 6.0 * (uniform() - 0.5); q.z = 6.0 * (uniform() - 0.5);
            q.event = e; q.species = (int)(uniform() * n_species) % n_species;
            p.push_back(q);
        }
    // equal momenta (q = 0), back to back (KT = 0), pT = 0, E = pz (massless along z), NaN, infinity
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double odd[8][4] = {{1, 0.3, 0.2, 0.1}, {1, 0.3, 0.2, 0.1}, {1, -0.3, -0.2, 0.1}, {1, 0, 0, 0.5}, {1, 0, 0, 1}, {1, 0.5, nan, 0}, {inf, 0.3, 0.2, 0.1}, {1, 0.3, 0.2, -inf}};
    for (int k = 0; k < 8; k++) {
        is3d_particle q;
        memset(&q, 0, sizeof q);
        q.E = odd[k][0]; q.px = odd[k][1]; q.py = odd[k][2]; q.pz = odd[k][3];
        q.x = k; q.event = 4; q.species = 1;
        p.push_back(q);
    }
    const int32_t slot[n_species] = {0, 1, 2, -1, 0, 1, 2};
    const is3d_hbt_bins shapes[3] = {{1.0, 0.05, 2.0, 0.0, 1.0, 16, 0.3, 64, 0}, {1.0, 0.05, 2.0, 0.1, 1.0, 1, 0.3, 2, 0}, {2.0, 0.0, 3.0, 0.0, 2.0, 3, 0.25, 7, 2}};
    for (const is3d_hbt_bins &b : shapes) {
        Hist h(b, n_events, n_slots);
        EXPECT(is3d_hbt_list(&b, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_OK);
        int64_t pairs = 0, most = 0, kept = 0;
        for (size_t j = 0; j < h.den.size(); j++) {
            pairs += h.den[j];
            EXPECT(h.num[j] <= h.den[j] * 4294967296LL && h.num[j] >= -h.den[j] * 4294967296LL);
        }
        for (size_t j = 0; j < h.M.size(); j++) { most += h.M[j] * (h.M[j] - 1); kept += h.M[j]; }
        EXPECT(pairs > 0 && pairs <= most && kept > 100 && kept < (int64_t)p.size());
        std::vector<is3d_hbt_radii_result> res((size_t)n_slots * b.n_kT);
        EXPECT(is3d_hbt_radii(&b, &h.view, n_slots, 1, 1e-3, res.data()) == IS3D_OK);
        for (const is3d_hbt_radii_result &r : res) EXPECT(r.n_bins >= 0 && (r.singular == 0 || (r.lambda == 0.0 && r.R2[0] == 0.0)));
        EXPECT(is3d_hbt_radii(&b, &h.view, n_slots, 1000000, 0.5, res.data()) == IS3D_OK && res[0].singular == 1);
        // the empty list
        EXPECT(is3d_hbt_list(&b, n_events, n_slots, slot, n_species, 0, nullptr, &h.view) == IS3D_OK && h.M[0] == 0 && h.den[0] == 0);
    }
    // ---- the writer ----
    {
        const is3d_hbt_bins b = shapes[2];
        Hist h(b, n_events, n_slots);
        EXPECT(is3d_hbt_list(&b, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_OK);
        const char *labels[n_slots] = {"211", "-211", "321"};
        EXPECT(is3d_write_hbt(dir.c_str(), &b, &h.view, n_slots, labels, 5, 0.05) == IS3D_EIO);       // no hbt/ yet
        EXPECT(mkdir((dir + "/hbt").c_str(), 0755) == 0);
        EXPECT(is3d_write_hbt(dir.c_str(), &b, &h.view, n_slots, labels, 5, 0.05) == IS3D_OK);
        struct stat sb;
        EXPECT(stat((dir + "/hbt/correlation_-211_kT2.dat").c_str(), &sb) == 0 && sb.st_size > 1000);
        EXPECT(stat((dir + "/hbt/radii_321.dat").c_str(), &sb) == 0 && sb.st_size > 100);
        const char *bad[n_slots] = {"211", "a/b", "321"}, *empty[n_slots] = {"211", "", "321"}, *null[n_slots] = {"211", nullptr, "321"};
        EXPECT(is3d_write_hbt(dir.c_str(), &b, &h.view, n_slots, bad, 5, 0.05) == IS3D_EINVAL);
        EXPECT(is3d_write_hbt(dir.c_str(), &b, &h.view, n_slots, empty, 5, 0.05) == IS3D_EINVAL);
        EXPECT(is3d_write_hbt(dir.c_str(), &b, &h.view, n_slots, null, 5, 0.05) == IS3D_EINVAL);
        EXPECT(is3d_write_hbt(nullptr, &b, &h.view, n_slots, labels, 5, 0.05) == IS3D_EINVAL);
        EXPECT(is3d_write_hbt(dir.c_str(), &b, &h.view, n_slots, nullptr, 5, 0.05) == IS3D_EINVAL);
        EXPECT(is3d_write_hbt(dir.c_str(), &b, &h.view, 0, labels, 5, 0.05) == IS3D_EINVAL);
        EXPECT(is3d_write_hbt(dir.c_str(), &b, &h.view, n_slots, labels, 0, 0.05) == IS3D_EINVAL);
        EXPECT(is3d_write_hbt(dir.c_str(), &b, &h.view, n_slots, labels, 5, 0.0) == IS3D_EINVAL);
    }
    // ---- refusals ----
    {
        const is3d_hbt_bins good = shapes[1];
        Hist h(good, n_events, n_slots);
        const is3d_hbt_bins bad[] = {{0.0, 0.05, 2.0, 0.1, 1.0, 1, 0.3, 2, 0}, {nan, 0.05, 2.0, 0.1, 1.0, 1, 0.3, 2, 0}, {1.0, -0.1, 2.0, 0.1, 1.0, 1, 0.3, 2, 0},
                                     {1.0, 0.05, 0.05, 0.1, 1.0, 1, 0.3, 2, 0}, {1.0, 0.05, 2.0, -0.1, 1.0, 1, 0.3, 2, 0}, {1.0, 0.05, 2.0, 1.0, 1.0, 1, 0.3, 2, 0},
                                     {1.0, 0.05, 2.0, 0.1, 1.0, 0, 0.3, 2, 0}, {1.0, 0.05, 2.0, 0.1, 1.0, 17, 0.3, 2, 0}, {1.0, 0.05, 2.0, 0.1, 1.0, 1, 0.0, 2, 0},
                                     {1.0, 0.05, 2.0, 0.1, 1.0, 1, inf, 2, 0}, {1.0, 0.05, 2.0, 0.1, 1.0, 1, 0.3, 1, 0}, {1.0, 0.05, 2.0, 0.1, 1.0, 1, 0.3, 65, 0},
                                     {400.0, 0.05, 2.0, 0.1, 1.0, 1, 0.3, 2, 0}, {1.0, 0.05, 2.0, 0.1, inf, 1, 0.3, 2, 0}};
        for (const is3d_hbt_bins &b : bad) {
            EXPECT(is3d_hbt_list(&b, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
            is3d_hbt_radii_result r;
            EXPECT(is3d_hbt_radii(&b, &h.view, 1, 1, 0.1, &r) == IS3D_EINVAL);
        }
        EXPECT(is3d_hbt_list(nullptr, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
        EXPECT(is3d_hbt_list(&good, 0, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
        EXPECT(is3d_hbt_list(&good, n_events, 0, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
        EXPECT(is3d_hbt_list(&good, n_events, n_slots, nullptr, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
        EXPECT(is3d_hbt_list(&good, n_events, n_slots, slot, 0, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);
        EXPECT(is3d_hbt_list(&good, n_events, n_slots, slot, n_species, -1, p.data(), &h.view) == IS3D_EINVAL);
        EXPECT(is3d_hbt_list(&good, n_events, n_slots, slot, n_species, (int64_t)p.size(), nullptr, &h.view) == IS3D_EINVAL);
        EXPECT(is3d_hbt_list(&good, n_events, n_slots, slot, n_species, (int64_t)p.size(), p.data(), nullptr) == IS3D_EINVAL);
        EXPECT(is3d_hbt_list(&good, n_events, 2, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);          // slot 2 of 2
        EXPECT(is3d_hbt_list(&good, 4, n_slots, slot, n_species, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);          // event 4 of 4
        EXPECT(is3d_hbt_list(&good, n_events, n_slots, slot, 6, (int64_t)p.size(), p.data(), &h.view) == IS3D_EINVAL);           // species 6 of 6
    }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("hbt_host_check: ok\n");
    return 0;
}
