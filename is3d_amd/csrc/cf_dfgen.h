// cf_dfgen.h -- the df-coefficient generator's kernel parameters and condition bits (cf_dfgen.hip).
#pragma once
#include <cstdint>

namespace is3d {

constexpr int kDfgenWaves = 4;       // waves per workgroup: wave w sums the list entries [n w / 4, n (w + 1) / 4)
constexpr int kDfgenIntegrals = 20;  // J20 J21 J40 J41 N10 N30 N31 M20 M21 A20 A21 B10 nB e p J30 J32 N20 M10 M11
constexpr int kDfgenTables = 10;     // c0 T^4, c1 T^3, c2 T^4, c3 T^4, c4 T^5, F / T, G, betabulk / T^4, betaV / T^3, betapi / T^4

// what a grid point failed on (the reference prints and calls exit(-1) in each case)
enum DfgenCondition : unsigned {
    kDfgenQstat = 1u,        // exp(Ebar - b alpha_B) + sign <= 0 at a node (thermal_integrands.cpp:18-23)
    kDfgenBulkDenom = 2u,    // 14-moment bulk denominator is zero (deltaf_table.cpp:228-232)
    kDfgenDiffDenom = 4u,    // 14-moment diffusion denominator is zero (:233-237)
    kDfgenBetapi = 8u,       // betapi == 0 (:370-374)
    kDfgenBetabulk = 16u,    // betabulk == 0 (:375-379)
    kDfgenBetaV = 32u,       // betaV == 0 (:380-384)
    kDfgenNonFinite = 64u,   // an output or an integral is inf or NaN
};

struct DfgenParams {
    int32_t n, n_gla, n_T, n_muB;
    const double *mass, *gspin, *baryon, *sign;   // [n], every entry of the list
    const double *root[4], *weight[4];            // alpha = 1..4, [n_gla] each
    const double *T, *muB;                        // [n_T], [n_muB]
    double two_pi2_hbarc3;
    double *tables;                               // [10][n_muB][n_T]
    double *integrals;                            // [20][n_muB][n_T]
    unsigned long long *status;                   // [0]: min over the failing points of (point << 8 | condition bits); ~0 when none fails
    int32_t *bad_entry;                           // [n_muB * n_T]: the first list entry with qstat <= 0 at that point (written by failing points only)
};

}  // namespace is3d
