// Host-only driver of is3d_amd/csrc/cf_plan_geometry.h for tests/test_plan_geometry.py: prints what the plans' geometry functions return.
//   plan_geometry_main variants        every (dimension, feqmod, baryon, fits, requested -1..15, build): "v dim fq bar fits req dev variant e2tab"
//   plan_geometry_main sizing          "w lane_waves requested wpb", "c rounds tasks pass_cells cell_chunks slab_bytes nch", "s bins rblocks S"
//   plan_geometry_main lanes FILE      FILE: "n n_pT split interleave use_baryon collapse", n x "mass sign baryon", n_pT x pT;
//                                      prints the species classes and the lane table, one named array per line
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../is3d_amd/csrc/cf_plan_geometry.h"

template <class V>
static void line(const char *name, const V &v, const char *fmt)
{
    printf("%s", name);
    for (auto x : v) { printf(" "); printf(fmt, x); }
    printf("\n");
}

static int variants()
{
    for (int dim : {2, 3})
        for (int fq : {0, 1})
            for (int bar : {0, 1})
                for (int fits : {0, 1})
                    for (int req = -1; req <= 15; req++)
                        for (int dev : {0, 1}) {
                            const is3d::VariantChoice c = is3d::choose_variant(dim, fq != 0, bar != 0, fits != 0, req, dev != 0);
                            printf("v %d %d %d %d %d %d %d %d\n", dim, fq, bar, fits, req, dev, c.variant, c.e2tab ? 1 : 0);
                        }
    return 0;
}

static int sizing()
{
    for (int lw = 1; lw <= 64; lw++)
        for (int req : {0, 1, 2, 4, 8}) printf("w %d %d %d\n", lw, req, is3d::waves_per_group(lw, req));
    const int64_t tasks[] = {1, 6, 48, 150, 1000, 98304, 200000};
    const int64_t cells[] = {1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000, 1151, 1152, 1153, 4096, 20000, 125000, 1000000};
    // slabs: tiny; 9.8 MB (config 3); 1 GiB (12 / 32 slabs under the caps); 5 GiB (2 / 6); 40 GiB (none fits: one chunk all the same)
    const int64_t slabs[] = {512, 9800000, (int64_t)1 << 30, (int64_t)5 << 30, (int64_t)40 << 30};
    for (int64_t rounds : {12, 24})
        for (int64_t t : tasks)
            for (int64_t pc : cells)
                for (int64_t cc : {0, 1, 7, 5000})
                    for (int64_t sb : slabs)
                        printf("c %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d\n", rounds, t, pc, cc, sb, is3d::chunk_count(rounds, t, pc, cc, sb));
    for (int bins = 1; bins <= 512; bins++)
        for (int rb = 1; rb <= 8; rb++) printf("s %d %d %d\n", bins, rb, is3d::lane_split(bins, rb));
    return 0;
}

static int lanes(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
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
    printf("ncls %zu\n", k.cmass.size());
    line("cls", k.cls, "%d");
    line("cmass", k.cmass, "%.17g");
    line("csign", k.csign, "%.17g");
    line("cbar", k.cbar, "%.17g");
    printf("sizes %d %d %d\n", t.Lbins, t.L, t.Lpad);
    line("order", t.order, "%d");
    line("slot_of", t.slot_of, "%d");
    line("mT", t.mT, "%.17g");
    line("pT", t.pT, "%.17g");
    line("sign", t.sign, "%.17g");
    line("b", t.b, "%.17g");
    line("sub", t.sub, "%d");
    line("lane_of", t.lane_of, "%d");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "variants")) return variants();
    if (argc == 2 && !strcmp(argv[1], "sizing")) return sizing();
    if (argc == 3 && !strcmp(argv[1], "lanes")) return lanes(argv[2]);
    fprintf(stderr, "usage: %s variants | sizing | lanes FILE\n", argv[0]);
    return 2;
}
