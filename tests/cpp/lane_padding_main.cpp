// Host-only driver of is3d::lane_arrays (is3d_amd/csrc/cf_plan_geometry.h) for tests/test_lane_padding.py: prints the lane table and the per-lane
// arrays a plan uploads of it, one named array per line; doubles as hexadecimal floats, so that the comparison is one of bits.
//   lane_padding_main FILE      FILE as for plan_geometry_main lanes: "n n_pT split interleave use_baryon collapse", n x "mass sign baryon", n_pT x pT
#include <cstdio>

#include "../../is3d_amd/csrc/cf_plan_geometry.h"

template <class V>
static void line(const char *name, const V &v, const char *fmt)
{
    printf("%s", name);
    for (auto x : v) { printf(" "); printf(fmt, x); }
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0, n_pT = 0, split = 0, inter = 0, use_b = 0, collapse = 0;
    if (fscanf(f, "%d %d %d %d %d %d", &n, &n_pT, &split, &inter, &use_b, &collapse) != 6 || n < 1 || n_pT < 1 || split < 1) { fclose(f); return 2; }
    std::vector<double> mass(n), sign(n), bar(n), pT(n_pT);
    bool ok = true;
    for (int s = 0; s < n; s++) ok = ok && fscanf(f, "%lf %lf %lf", &mass[s], &sign[s], &bar[s]) == 3;
    for (int i = 0; i < n_pT; i++) ok = ok && fscanf(f, "%lf", &pT[i]) == 1;
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    const is3d::SpeciesClasses k = is3d::species_classes(mass.data(), sign.data(), use_b ? bar.data() : nullptr, n, collapse != 0);
    const is3d::LaneTable t = is3d::lane_table(k, pT.data(), n_pT, split, inter != 0);
    const is3d::LaneArrays a = is3d::lane_arrays(t, k, n_pT);
    printf("sizes %d %d %d %d\n", t.Lbins, t.L, t.Lpad, a.Lpad);
    line("cmass", k.cmass, "%a");
    line("order", t.order, "%d");
    line("t.mT", t.mT, "%a");
    line("t.pT", t.pT, "%a");
    line("t.sign", t.sign, "%a");
    line("t.b", t.b, "%a");
    line("t.sub", t.sub, "%d");
    line("a.mT", a.mT, "%a");
    line("a.pT", a.pT, "%a");
    line("a.sign", a.sign, "%a");
    line("a.b", a.b, "%a");
    line("a.mass", a.mass, "%a");
    line("a.sub", a.sub, "%d");
    line("a.ipT", a.ipT, "%d");
    line("a.pe", a.pe, "%d");
    line("a.cls", a.cls, "%d");
    printf("max %a %a\n", a.mTmax, a.pTmax);
    return 0;
}
