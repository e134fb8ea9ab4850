// tools/sell_plan_asan.hip — dev tool: the host planner of the blocked sliced stream (spmv_bcsr_sell.hpp: build_sell_plan,
// build_sell_wave_ranges, SellPlanHost) under the HOST address and undefined-behaviour sanitizers, every table checked by brute force.
// The header holds kernels, so this is a HIP file built by hipcc; nothing here launches one (GPU sanitizers are not available on this pool).
// Patterns, by block-row lengths (the families of tests/bsell_cases.py, the smallest of each, generated here): ragged rows at every
// row count around the slice of 16 and around a wave's 64 quads, slices of one step at both sides of each wave-count rule, one heavy
// slice in front of light ones (with and without empty slices), 32 equal slices, empty slices at the front, middle and end, no block
// at all, the heavy slice last, one slice of 257 blocks, a full last step, and random patterns with empty block rows and one long row.
// Each with nwaves_max in {1, 7, 1024, 2048}, and the wave ranges again over the first three slices only (the pool form).
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize -Inavierstokes_amd/csrc -Iinclude -o /tmp/sell_plan_asan tools/sell_plan_asan.hip
//   ASAN_OPTIONS=detect_leaks=0 /tmp/sell_plan_asan
#include "spmv_bcsr_sell.hpp"
#include <cstdio>
#include <random>
#include <string>
using namespace mi355;

static int bad = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            printf("%s: ", what.c_str()); \
            printf(__VA_ARGS__);          \
            printf("\n");                 \
            bad++;                        \
            return;                       \
        }                                 \
    } while (0)

using Lens = std::vector<int>;

// slice s has one row (a varying one) of slice_lens[s] blocks, the others at most `fill`; the last `cut` rows are left out
static Lens rows_of_slices(const Lens& slice_lens, std::mt19937& rng, int fill, int cut = 0)
{
    const int ns = (int)slice_lens.size();
    Lens lens((size_t)ns * kSellRows);
    for (int s = 0; s < ns; s++) {
        for (int r = 0; r < kSellRows; r++) lens[(size_t)s * kSellRows + r] = std::min((int)(rng() % (fill + 1)), slice_lens[s]);
        lens[(size_t)s * kSellRows + (s + 1 < ns || !cut ? (7 * s) % kSellRows : 0)] = slice_lens[s];
    }
    lens.resize(lens.size() - cut);
    return lens;
}

static Lens ragged(int nbrows, int maxlen, int empty_pct, std::mt19937& rng)
{
    Lens lens((size_t)nbrows);
    for (int& l : lens) l = (int)(rng() % 100) < empty_pct ? 0 : (int)(rng() % (maxlen + 1));
    return lens;
}

static int cases = 0;

// the wave ranges of the first NS slices: a partition into `want` contiguous ranges, range w starting at the first slice whose first
// step lies at or behind w / want of the steps
static void check_ranges(const std::string& what, const SellPlanHost& P, const std::vector<int>& wrng, int nwaves, int want, int NS)
{
    EXPECT(nwaves == want && (int)wrng.size() == want + 1, "nwaves %d, table of %zu, a direct count says %d", nwaves, wrng.size(), want);
    EXPECT(wrng[0] == 0 && wrng[want] == NS, "the ranges run from slice %d to %d of %d", wrng[0], wrng[want], NS);
    const long long steps = P.sptr[NS];
    for (int w = 1; w <= want; w++) {
        EXPECT(wrng[w] >= wrng[w - 1] && wrng[w] <= NS, "range %d ends before it starts, or outside the slices", w - 1);
        if (w == want) break;
        int s = 0;
        while (s < NS && ((long long)P.sptr[s] + 1) * want <= steps * w) s++; // sptr[s] < floor(steps w / want), without the division
        EXPECT(wrng[w] == s, "range %d starts at slice %d, its share of the steps starts at slice %d", w, wrng[w], s);
    }
}

static void check(const std::string& name, const Lens& lens, int nbcols, std::mt19937& rng)
{
    const int nbrows = (int)lens.size();
    std::vector<int> ptrow(1, 0), indcol;
    for (int i = 0; i < nbrows; i++) { // ascending, distinct block columns, never column 0
        const int L = lens[i], m = nbcols - 1;
        if (L > m) {
            printf("%s: the harness asked for %d blocks in %d columns\n", name.c_str(), L, m);
            bad++;
            return;
        }
        const int start = L < m ? (int)(rng() % (m - L + 1)) : 0, stride = L ? std::max(1, (m - start) / L) : 1;
        for (int j = 0; j < L; j++) indcol.push_back(1 + start + j * stride);
        ptrow.push_back((int)indcol.size());
    }
    for (int nwaves_max : {1, 7, 1024, 2048}) {
        const std::string what = name + ", at most " + std::to_string(nwaves_max) + " waves";
        cases++;
        SellPlanHost P;
        build_sell_plan(nbrows, ptrow.data(), indcol.data(), nwaves_max, P);
        // slices and steps by a direct count
        const int ns = (nbrows + kSellRows - 1) / kSellRows;
        std::vector<int> len((size_t)ns, 1);
        long long nsteps = 0;
        for (int s = 0; s < ns; s++) {
            for (int i = kSellRows * s; i < std::min(nbrows, kSellRows * (s + 1)); i++) len[s] = std::max(len[s], lens[i]);
            nsteps += len[s];
        }
        EXPECT(P.nslices == ns && P.nsteps == nsteps, "%d slices of %lld steps, a direct count says %d of %lld", P.nslices, P.nsteps, ns, nsteps);
        EXPECT((int)P.sptr.size() == ns + 3 && (long long)P.col.size() == (nsteps + kSellPadSteps) * kSellRows, "table lengths");
        long long at = 0, placed = 0;
        for (int s = 0; s < ns; s++) {
            EXPECT(P.sptr[s] == at, "slice %d starts at step %d, not %lld", s, P.sptr[s], at);
            for (int j = 0; j < len[s]; j++)
                for (int r = 0; r < kSellRows; r++) {
                    const unsigned e = P.col[(size_t)(at + j) * kSellRows + r];
                    const int i = kSellRows * s + r;
                    const bool there = i < nbrows && j < lens[i];
                    EXPECT(((e & kSellFirstCol) != 0) == (j == 0), "slice %d step %d row %d: the first-step mark", s, j, r);
                    if (there) {
                        EXPECT(!(e & kSellPadCol) && (int)(e & kSellColMask) == indcol[ptrow[i] + j], "slice %d step %d row %d: not the row's block %d", s, j, r, j);
                        EXPECT(j == 0 || (P.col[(size_t)(at + j - 1) * kSellRows + r] & kSellColMask) < (e & kSellColMask), "slice %d row %d: columns do not ascend at step %d", s, r, j);
                        placed++;
                    } else
                        EXPECT((e & kSellPadCol) && (e & kSellColMask) == 0, "slice %d step %d row %d: a padding place is not marked (or names a column)", s, j, r);
                }
            at += len[s];
        }
        EXPECT(placed == (long long)indcol.size(), "%lld blocks placed of %zu", placed, indcol.size());
        for (int t = 0; t < 3; t++) EXPECT(P.sptr[ns + t] == nsteps, "terminator %d of sptr", t);
        for (int j = 0; j < kSellPadSteps; j++) // behind the stream: padding places, the first of them marked as a slice's first step
            for (int r = 0; r < kSellRows; r++)
                EXPECT(P.col[(size_t)(nsteps + j) * kSellRows + r] == (kSellPadCol | (j == 0 ? kSellFirstCol : 0u)), "padding step %d row %d", j, r);
        const int want = std::min(nwaves_max, std::max(32, (ns / 2 + 31) / 32 * 32));
        check_ranges(what, P, P.wrng, P.nwaves, want, ns);
        for (int nstatic : {-1, 3}) { // -1 again through the public door; 3: the ranges of the first three slices (the rest is a pool)
            cases++;
            std::vector<int> wrng(5, -7);
            int nwaves = -1;
            build_sell_wave_ranges(P, nwaves_max, wrng, nwaves, nstatic);
            check_ranges(what + ", static slices " + std::to_string(nstatic), P, wrng, nwaves, want, nstatic < 0 ? ns : std::min(nstatic, ns));
        }
    }
}

int main()
{
    std::mt19937 rng(19);
    int patterns = 0;
    auto run = [&](const std::string& name, const Lens& lens, int nbcols = 0) {
        int need = 2;
        for (int l : lens) need = std::max(need, l + 1);
        check(name, lens, std::max(nbcols, need), rng);
        patterns++;
    };
    // the row count against the slice of 16 and a wave's 64 quads
    for (int nbrows : {0, 1, 15, 16, 17, 63, 64, 65, 1023, 1025, 4096}) {
        Lens lens = ragged(nbrows, 6, 20, rng);
        if (nbrows) lens[0] = 3;
        run("rows " + std::to_string(nbrows), lens, std::max(nbrows, 8));
    }
    // the wave-count rule: 32 waves up to 65 slices, nslices / 2 rounded up to 32 beyond, capped at 1024 and at 2048
    for (int ns : {65, 66, 1985, 1986, 2049, 2050, 4033, 4034, 4097}) run("slices " + std::to_string(ns), rows_of_slices(Lens((size_t)ns, 1), rng, 1, 5), 64);
    // one heavy slice in front of light ones: the waves under its steps own nothing
    for (int ns : {9, 35, 100}) {
        Lens sl((size_t)ns, 1);
        sl[0] = 32 * (ns / 4 + 1) - (ns - 1);
        if (ns == 35)
            for (int s = 2; s < ns - 1; s += 4) sl[s] = 0;
        run("one heavy slice of " + std::to_string(ns), rows_of_slices(sl, rng, 1));
    }
    for (int L : {3, 13}) run("32 slices of " + std::to_string(L), rows_of_slices(Lens(32, L), rng, L));
    {
        Lens sl(64, 1);
        for (int s : {0, 1, 10, 11, 62, 63}) sl[s] = 0;
        run("empty slices", rows_of_slices(sl, rng, 1), 32);
        run("no blocks", Lens(100, 0), 8);
        Lens hl(40, 1);
        hl[39] = 2000; // one long row, last
        run("heavy slice last", rows_of_slices(hl, rng, 1));
        Lens tier = ragged(300 * kSellRows, 2, 30, rng);
        for (int r = 0; r < kSellRows; r++) tier[(size_t)290 * kSellRows + r] = r == 4 ? 77 : 12; // 257 blocks in one slice
        run("one slice of 257 blocks", tier);
        Lens tail = ragged(80, 5, 20, rng);
        tail[79] = 9;
        run("full last step", tail);
    }
    for (int it = 0; it < 40; it++) { // random: empty block rows, and in every other one a long row
        Lens lens = ragged((int)(rng() % 3000), 1 + (int)(rng() % 20), (int)(rng() % 60), rng);
        if (it % 2 && !lens.empty()) lens[rng() % lens.size()] = 100 + (int)(rng() % 2400);
        run("random " + std::to_string(it), lens);
    }
    printf("patterns %d\n", patterns);
    printf("sliced block plans: cases %d bad %d\n", cases, bad);
    return bad != 0;
}
