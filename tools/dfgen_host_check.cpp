// dfgen_host_check.cpp -- a stand-alone program for tools/sanitize_dfgen_host.sh: the host code of the coefficient generator (the writer of
// host_io.cpp, the two readers, the argument checks of is3d_df_generate in cf_dfgen.hip) under AddressSanitizer + UBSan, with no Python and no
// preloaded runtime.  It needs no GPU: every is3d_df_generate call here returns before the device is touched, except the last one, which is
// IS3D_ENODEVICE on a machine without a device and IS3D_OK with one.
// usage: dfgen_host_check SCRATCH_DIR   (the directory must exist and be empty)
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

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s SCRATCH_DIR\n", argv[0]); return 2; }
    const std::string dir = std::string(argv[1]) + "/tables";
    // ---- the writer and both readers on an off-shape grid ----
    const int nT = 3, nB = 2;
    const double T[nT] = {0.3, 0.1234, 0.05}, B[nB] = {0.0, 0.4567};
    std::vector<double> tab((size_t)10 * nT * nB);
    for (size_t i = 0; i < tab.size(); i++) tab[i] = std::sin(1.0 + (double)i) * (i % 7 == 0 ? 1744.0 : 0.25);
    EXPECT(is3d_df_tables_write(dir.c_str(), nT, T, nB, B, tab.data()) == IS3D_OK);
    EXPECT(is3d_df_tables_write(dir.c_str(), nT, T, nB, B, tab.data()) == IS3D_EINVAL);          // never overwritten
    EXPECT(is3d_df_tables_write(nullptr, nT, T, nB, B, tab.data()) == IS3D_EINVAL);
    EXPECT(is3d_df_tables_write(dir.c_str(), 0, T, nB, B, tab.data()) == IS3D_EINVAL);
    {
        std::vector<double> bad(tab);
        bad[17] = std::numeric_limits<double>::quiet_NaN();
        EXPECT(is3d_df_tables_write((dir + "_nan").c_str(), nT, T, nB, B, bad.data()) == IS3D_EINVAL);
    }
    static const char *const names[10] = {"c0", "c1", "c2", "c3", "c4", "F", "G", "betabulk", "betaV", "betapi"};
    for (int t = 0; t < 10; t++) {
        const std::string path = dir + "/" + names[t] + ".dat";
        int32_t a = 0, b = 0;
        EXPECT(is3d_df_table_read_full(path.c_str(), &a, &b, nullptr, nullptr, nullptr, 0) == IS3D_OK && a == nT && b == nB);
        std::vector<double> Tr(a), Br(b), v((size_t)a * b), T1(a), v1(a);
        EXPECT(is3d_df_table_read_full(path.c_str(), &a, &b, Tr.data(), Br.data(), v.data(), (int64_t)v.size()) == IS3D_OK);
        EXPECT(is3d_df_table_read(path.c_str(), &a, T1.data(), v1.data(), a) == IS3D_OK);
        for (int i = 0; i < nT * nB; i++) {
            char buf[64];
            snprintf(buf, sizeof buf, "%.6f", tab[(size_t)t * nT * nB + i]);
            EXPECT(v[i] == strtod(buf, nullptr));
        }
        for (int i = 0; i < nT; i++) EXPECT(v1[i] == v[i] && T1[i] == Tr[i]);
    }
    // ---- is3d_df_generate: every refusal returns before the device is used ----
    const int n = 5, ng = 3;
    double mass[n] = {0.0, 0.138, 0.938, 0.938, 1.232}, g[n] = {2, 1, 2, 2, 4}, b[n] = {0, 0, 1, -1, 1}, s[n] = {-1, -1, 1, 1, 1};
    double r[4][ng] = {{0.5, 2.0, 6.0}, {0.7, 2.5, 7.0}, {0.9, 3.0, 8.0}, {1.1, 3.5, 9.0}}, w[4][ng] = {{0.6, 0.3, 0.01}, {0.9, 0.9, 0.05}, {1.5, 3.0, 0.3}, {3.0, 12.0, 2.0}};
    const double *r4[4] = {r[0], r[1], r[2], r[3]}, *w4[4] = {w[0], w[1], w[2], w[3]};
    is3d_hadron_list list = {n, mass, g, b, s};
    double Tg[2] = {0.15, 0.12}, Bg[1] = {0.2};
    std::vector<double> out(10 * 2), integ(20 * 2);
    int64_t p0 = 0, a0 = 0, p1 = 0, a1 = 0;
    is3d_resource_counters(&p0, &a0);
    EXPECT(is3d_df_generate(nullptr, ng, r4, w4, 2, Tg, 1, Bg, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL);
    EXPECT(is3d_df_generate(&list, 0, r4, w4, 2, Tg, 1, Bg, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL);
    EXPECT(is3d_df_generate(&list, ng, nullptr, w4, 2, Tg, 1, Bg, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL);
    EXPECT(is3d_df_generate(&list, ng, r4, w4, 0, Tg, 1, Bg, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL);
    EXPECT(is3d_df_generate(&list, ng, r4, w4, 2, Tg, 1, Bg, -1, nullptr, nullptr, nullptr) == IS3D_EINVAL);
    EXPECT(is3d_df_generate(&list, ng, r4, w4, 2, Tg, 1, Bg, -7, out.data(), nullptr, nullptr) == IS3D_EINVAL);
    { is3d_hadron_list e = list; e.n = 0; EXPECT(is3d_df_generate(&e, ng, r4, w4, 2, Tg, 1, Bg, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL); }
    { is3d_hadron_list e = list; e.sign = nullptr; EXPECT(is3d_df_generate(&e, ng, r4, w4, 2, Tg, 1, Bg, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL); }
    { double Tb[2] = {0.15, 0.0}; EXPECT(is3d_df_generate(&list, ng, r4, w4, 2, Tb, 1, Bg, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL); }
    { double Bb[1] = {std::numeric_limits<double>::infinity()}; EXPECT(is3d_df_generate(&list, ng, r4, w4, 2, Tg, 1, Bb, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL); }
    { const double keep = mass[4]; mass[4] = std::nan(""); EXPECT(is3d_df_generate(&list, ng, r4, w4, 2, Tg, 1, Bg, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL); mass[4] = keep; }
    { const double keep = r[3][2]; r[3][2] = 0.0; EXPECT(is3d_df_generate(&list, ng, r4, w4, 2, Tg, 1, Bg, -1, out.data(), nullptr, nullptr) == IS3D_EINVAL); r[3][2] = keep; }
    is3d_resource_counters(&p1, &a1);
    EXPECT(p0 == p1 && a0 == a1);
    // ---- a good call: no CPU path ----
    is3d_dfgen_stats st;
    const int rc = is3d_df_generate(&list, ng, r4, w4, 2, Tg, 1, Bg, -1, out.data(), integ.data(), &st);
    if (rc == IS3D_OK) EXPECT(st.n_massive == 4);
    else EXPECT(rc == IS3D_ENODEVICE && strstr(is3d_last_error(), "no CPU path"));
    printf("dfgen_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
