// tools/bilu4_order_asan.cpp — dev tool: bilu4_order.hpp (the multicolour ordering behind an ordered block ILU handle) under the host
// address and undefined-behaviour sanitizers, with the two places of bilu4_plan.hpp that read the caller's values through its src table.
// On 300 seeded random patterns (1 to 200 block rows, unsymmetric, densities 4-23 %), by brute force: the ordering passes its own check;
// the permuted pattern is a legal pattern (columns ascending, a diagonal block per row) and src names, for every block of it, the block of
// the caller's row that carries the renamed column; at fill 0 both sweeps have at most ncolours levels; the host factorisation through src
// (4 threads, both layouts) refuses no pivot of a dominated matrix; the device plan's gather table stays inside the caller's blocks:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -Inavierstokes_amd/csrc -o /tmp/bilu4_order_asan tools/bilu4_order_asan.cpp && /tmp/bilu4_order_asan
#include "bilu4_plan.hpp"
#include "bilu4_order.hpp"
#include <cstdio>
#include <random>
using namespace mi355;
int main()
{
    std::mt19937 rng(7);
    for (int t = 0; t < 300; t++) {
        const int nb = 1 + (int)(rng() % 200);
        std::vector<int> ptr(1, 0), col;
        for (int i = 0; i < nb; i++) {
            for (int j = 0; j < nb; j++)
                if (j == i || rng() % 100 < 4 + t % 20) col.push_back(j);
            ptr.push_back((int)col.size());
        }
        if (!bilu4_check_pattern(nb, ptr.data(), col.data()).empty()) { printf("pattern %d: generated pattern refused\n", t); return 1; }
        Bilu4Order O;
        bilu4_colour(nb, ptr.data(), col.data(), &O);
        const std::string bad = bilu4_order_check(nb, ptr.data(), col.data(), O);
        if (!bad.empty()) { printf("%s\n", bad.c_str()); return 2; }
        std::vector<int> bp, bc;
        bilu4_permute_pattern(nb, ptr.data(), col.data(), &O, &bp, &bc);
        if (!bilu4_check_pattern(nb, bp.data(), bc.data()).empty()) { printf("pattern %d: permuted pattern is not legal\n", t); return 3; }
        for (int n = 0; n < nb; n++)
            for (int k = bp[n]; k < bp[n + 1]; k++) {
                const int a = O.src[k];
                const int i = O.iperm[n];
                if (a < ptr[i] || a >= ptr[i + 1] || O.perm[col[a]] != bc[k]) { printf("pattern %d: src does not name the caller's block\n", t); return 4; }
            }
        Bilu4Schedule S;
        bilu4_schedule(nb, bp.data(), bc.data(), 0, &S);
        if (S.sweep[0].nlev() > O.ncolours || S.sweep[1].nlev() > O.ncolours) { printf("pattern %d: more levels than colours at fill 0\n", t); return 5; }
        std::vector<double> coef(16 * col.size(), 0.01), val(16 * (size_t)S.pat.nblocks());
        for (int i = 0; i < nb; i++)
            for (int k = ptr[i]; k < ptr[i + 1]; k++)
                if (col[k] == i) for (int d = 0; d < 4; d++) coef[16 * (size_t)k + 5 * d] = 10.0 + i;
        if (bilu4_factor(S.pat, S.sweep[0], bp.data(), bc.data(), coef.data(), t & 1, 4, val.data(), O.src.data()) != -1) { printf("pattern %d: a pivot was refused\n", t); return 6; }
        Bilu4DevPlan D;
        bilu4dev_plan(S, bp.data(), bc.data(), &D, O.src.data());
        for (int g : D.gather) if (g < -1 || g >= (int)col.size()) { printf("pattern %d: gather leaves the caller's blocks\n", t); return 7; }
    }
    puts("bad 0");
    return 0;
}
