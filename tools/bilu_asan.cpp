// tools/bilu_asan.cpp — dev tool: bilu4_plan.hpp (the schedule of the block ILU, its host factorisation, the device refactor's plan, the
// one-launch solve's plan) and dilu4_plan.hpp (the block DILU's pivots) under the host address and undefined-behaviour sanitizers,
// every table checked by brute force on the empty matrix, a diagonal one, a chain, random banded and random unsymmetric patterns at
// fill 0 to 3, and layered patterns whose levels have 1, 63, 64, 65 and 129 rows (either side of the folding rule).  The level loop
// the factorisation and the pivots share (bilu4_for_level_rows) through both: the same bits at 1, 3, 4 and 16 threads, and of several
// refused pivots planted in one wide and in one narrow level the lowest block row is the one returned.  The device refactor's plan of the
// DILU pivots (dilu4dev_plan, dilu4dev_check) at fill 0 on all of these, on patterns that lost some of their (j, i) blocks and on a
// strictly lower one (no U block at all), without and with a src table: the index stream of dilu4f_row replayed, and corruptions planted
// that dilu4dev_check must report.  Address and undefined behaviour, then (a second binary) threads:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -Inavierstokes_amd/csrc -o /tmp/bilu_tsan tools/bilu_asan.cpp && /tmp/bilu_tsan
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -Inavierstokes_amd/csrc -o /tmp/bilu_asan tools/bilu_asan.cpp && /tmp/bilu_asan
#include "bilu4_plan.hpp"
#include "dilu4_plan.hpp"
#include <cstdio>
#include <random>
using namespace mi355;

static int bad = 0;
#define EXPECT(cond, ...)                  \
    do {                                   \
        if (!(cond)) {                     \
            printf("%s fill %d: ", name, fill); \
            printf(__VA_ARGS__);           \
            printf("\n");                  \
            bad++;                         \
            return;                        \
        }                                  \
    } while (0)

using Rows = std::vector<std::vector<int>>;

// the layered patterns of tests/bilu4_cases.py: layer l holds widths[l] consecutive rows, every row is linked (both ways) to one row
// of the layer before and is named by one of the layer after, so at fill 0 the forward levels are the layers, the backward ones the layers reversed
static Rows layered(const std::vector<int>& widths, int extra, std::mt19937& rng)
{
    std::vector<int> first(1, 0);
    for (int w : widths) first.push_back(first.back() + w);
    Rows rows(first.back());
    auto link = [&](int i, int j) { rows[i].push_back(j), rows[j].push_back(i); };
    for (size_t l = 0; l + 1 < widths.size(); l++) {
        for (int r = 0; r < widths[l + 1]; r++) link(first[l + 1] + r, first[l] + r % widths[l]);
        for (int r = 0; r < widths[l]; r++) link(first[l] + r, first[l + 1] + r % widths[l + 1]);
    }
    for (size_t l = 2; l < widths.size(); l++)
        for (int r = 0; r < widths[l]; r++)
            for (int e = 0; e < extra; e++) link(first[l] + r, (int)(rng() % first[l - 1]));
    return rows;
}

// fill 0, where the factor's pattern is the matrix's own: the DILU pivots with the same bits whatever the thread count, and a refused
// pivot — every block of a block row zeroed, so that nothing is subtracted from its zero diagonal block — planted in two rows of a
// level: both users of the shared level loop return the lower one.  widths: as for check (the levels of a layered pattern)
static void check_dilu(const char* name, const Bilu4Schedule& S, const std::vector<int>& ptr, const std::vector<int>& col, const std::vector<double>& coef,
                       const std::vector<int>& widths)
{
    const int fill = 0;
    const Bilu4Pattern& P = S.pat;
    const Bilu4Sweep& F = S.sweep[0];
    const int nb = P.nb;
    EXPECT(P.col == col && (int)P.ptr.size() == (int)ptr.size(), "the pattern at fill 0 is not the matrix's");
    const size_t nv = 16 * (size_t)P.nblocks(), nd = 16 * (size_t)nb;
    std::vector<double> val(nv, -1.0), e1(nd, -1.0), k1(nd, -1.0), et(nd), kt(nd);
    dilu4_values(P.nblocks(), coef.data(), false, nullptr, val.data());
    EXPECT(nv == 0 || !memcmp(val.data(), coef.data(), sizeof(double) * nv), "dilu4_values without a src table is not a copy");
    const int r1 = dilu4_pivots(P, F, val.data(), 1, e1.data(), k1.data());
    EXPECT(r1 == -1, "a DILU pivot was refused (row %d)", r1);
    for (int threads : {3, 16}) {
        std::fill(et.begin(), et.end(), -2.0), std::fill(kt.begin(), kt.end(), -2.0);
        const int rt = dilu4_pivots(P, F, val.data(), threads, et.data(), kt.data());
        EXPECT(rt == -1, "a DILU pivot was refused with %d threads (row %d)", threads, rt);
        EXPECT(nd == 0 || (!memcmp(e1.data(), et.data(), sizeof(double) * nd) && !memcmp(k1.data(), kt.data(), sizeof(double) * nd)), "the DILU pivots differ between 1 and %d threads", threads);
    }
    if (widths.empty()) return;
    for (bool wide : {true, false}) {
        int l = 0; // the first level of that kind
        while (l < F.nlev() && (F.lev_ptr[l + 1] - F.lev_ptr[l] >= kBiluRowsPerWG) != wide) l++;
        if (l == F.nlev()) continue;
        const int p0 = F.lev_ptr[l], p1 = F.lev_ptr[l + 1];
        const int rows[2] = {F.perm[p1 - 1], F.perm[p0 + (p1 - p0) / 2]}; // the last share's last row, and a lower one from the middle (the same one in a level of one row)
        const int want = std::min(rows[0], rows[1]);
        std::vector<double> cz(coef);
        for (int i : rows) std::fill(cz.begin() + 16 * (size_t)ptr[i], cz.begin() + 16 * (size_t)ptr[i + 1], 0.0);
        dilu4_values(P.nblocks(), cz.data(), false, nullptr, val.data());
        for (int threads : {1, 3, 16}) {
            std::vector<double> v(nv, -3.0);
            const int rf = bilu4_factor(P, F, ptr.data(), col.data(), cz.data(), false, threads, v.data());
            const int rd = dilu4_pivots(P, F, val.data(), threads, et.data(), kt.data());
            EXPECT(rf == want && rd == want, "%s level %d, %d threads: refused rows %d and %d planted, factor says %d, pivots say %d", wide ? "wide" : "narrow", l, threads, rows[0], rows[1], rf, rd);
        }
    }
}

// The device plan of the DILU pivots at fill 0, without a src table and with one (a random permutation of the caller's blocks:
// the caller then stores block k of the pattern at src[k]).  The index stream of dilu4f_row (dilu4_factor.hpp), which reads
//     m = V.mate[k0];  V.fcol[k0];  kn = min(k0 + 1, last): V.fcol[kn], V.mate[kn];  in the loop kn = min(lk + 2, last): V.fcol[kn], V.mate[kn]
//     load: V.L[16 lk + e], V.einv + 16 j + c, V.U + 16 max(m, 0) + c
// over fptr / fcol, the forward sweep's level-major row starts and columns, replayed for every forward position.
static int dilu_plans = 0, planted = 0, caught = 0;
static void check_dilu_dev(const char* name, const Bilu4Schedule& S, const std::vector<int>& ptr, const std::vector<int>& col, std::mt19937& rng)
{
    const int fill = 0;
    const Bilu4Pattern& P = S.pat;
    const int nb = P.nb;
    const long long total = P.nblocks();
    std::vector<int> perm((size_t)total);
    for (long long k = 0; k < total; k++) perm[k] = (int)k;
    std::shuffle(perm.begin(), perm.end(), rng);
    for (const int* src : {(const int*)nullptr, (const int*)perm.data()}) {
        dilu_plans++;
        Dilu4DevPlan D;
        dilu4dev_plan(S, ptr.data(), col.data(), &D, src);
        const std::string why = dilu4dev_check(S, D, src);
        EXPECT(why.empty(), "%s src: %s", src ? "with" : "without", why.c_str());
        std::vector<int> fptr(1, 0), fcol;
        for (int q = 0; q < nb; q++) {
            const auto [k0, k1] = P.offdiag(S.sweep[0].perm[q], false);
            for (int k = k0; k < k1; k++) fcol.push_back(P.col[k]);
            fptr.push_back((int)fcol.size());
        }
        const long long nL = D.nL, nU = D.nU;
        EXPECT((long long)fcol.size() == nL && (long long)D.mate.size() == nL && (long long)D.gather.size() == nL + nU + nb, "table lengths");
        long long pairs = 0;
        for (int q = 0; q < nb; q++) {
            const int k0 = fptr[q], k1 = fptr[q + 1];
            if (k0 >= k1) continue;
            const int last = k1 - 1;
            auto touch = [&](long long at) { // one read of fcol[at] and mate[at], and the loads they lead to
                if (at < 0 || at >= nL) return false;
                const int j = fcol[at], m = D.mate[at];
                return j >= 0 && j < nb && m >= -1 && std::max(m, 0) < std::max<long long>(nU, 1);
            };
            EXPECT(touch(k0) && touch(std::min(k0 + 1, last)), "position %d: the reads ahead of the loop leave the tables", q);
            for (int lk = k0; lk < k1; lk++) {
                EXPECT(touch(std::min(lk + 2, last)), "position %d: the read two blocks ahead of block %d leaves the tables", q, lk);
                pairs += D.mate[lk] >= 0;
            }
        }
        EXPECT(pairs == D.pivot_pairs, "pivot_pairs");
        std::vector<char> seen((size_t)total, 0);
        for (int h : D.gather) EXPECT(h >= 0 && h < total && !seen[h]++, "gather names block %d twice, or no block of the caller's", h);
        // teeth
        long long km = -1;
        for (long long k = 0; k < nL && km < 0; k++)
            if (D.mate[k] >= 0) km = k;
        if (km >= 0 && nU >= 2) {
            Dilu4DevPlan C(D);
            C.mate[km] += C.mate[km] + 1 < nU ? 1 : -1;
            planted++, caught += !dilu4dev_check(S, C, src).empty();
        }
        if (total >= 2) {
            Dilu4DevPlan C(D);
            C.gather[total - 1] = C.gather[0];
            planted++, caught += !dilu4dev_check(S, C, src).empty();
        }
        if (nb >= 2) {
            Dilu4DevPlan C(D);
            std::swap(C.fpos[0], C.fpos[nb - 1]);
            planted++, caught += !dilu4dev_check(S, C, src).empty();
        }
    }
}

// widths: the level sizes the pattern must have at fill 0 (forward; reversed backward), or empty
static void check(const char* name, Rows rows, int fill, const std::vector<int>& widths = {})
{
    const int nb = (int)rows.size();
    std::vector<int> ptr(1, 0), col;
    for (int i = 0; i < nb; i++) {
        rows[i].push_back(i);
        std::sort(rows[i].begin(), rows[i].end());
        rows[i].erase(std::unique(rows[i].begin(), rows[i].end()), rows[i].end());
        col.insert(col.end(), rows[i].begin(), rows[i].end());
        ptr.push_back((int)col.size());
    }
    EXPECT(bilu4_check_pattern(nb, ptr.data(), col.data()).empty(), "the harness made a bad pattern");
    Bilu4Schedule S;
    bilu4_schedule(nb, ptr.data(), col.data(), fill, &S);
    const Bilu4Pattern& P = S.pat;

    // the two off-diagonal ranges and the diagonal partition every row; where[i * nb + j]: the place of block (i, j), found by walking the row
    std::vector<int> where((size_t)nb * nb, -1);
    EXPECT(P.nb == nb && (int)P.ptr.size() == nb + 1 && P.nblocks() == (long long)P.col.size(), "pattern sizes");
    for (int i = 0; i < nb; i++) {
        const auto [l0, l1] = P.offdiag(i, false);
        const auto [u0, u1] = P.offdiag(i, true);
        EXPECT(l0 == P.ptr[i] && l0 <= l1 && l1 == P.diag[i] && u0 == l1 + 1 && u0 <= u1 && u1 == P.ptr[i + 1], "row %d is not L | diagonal | U", i);
        for (int k = P.ptr[i]; k < P.ptr[i + 1]; k++) {
            EXPECT(k < l1 ? P.col[k] < i : k == l1 ? P.col[k] == i : P.col[k] > i, "row %d: block %d on the wrong side of the diagonal", i, k);
            where[(size_t)i * nb + P.col[k]] = k;
        }
    }

    // the launches partition the levels, and a launch is folded exactly when the rule says so
    for (int b = 0; b < 2; b++) {
        const Bilu4Sweep& W = S.sweep[b];
        std::vector<int> level(nb, -1);
        for (int l = 0; l < W.nlev(); l++)
            for (int q = W.lev_ptr[l]; q < W.lev_ptr[l + 1]; q++) level[W.perm[q]] = l;
        for (int i = 0; i < nb; i++) {
            EXPECT(level[i] >= 0, "sweep %d: row %d has no position", b, i);
            const auto [k0, k1] = P.offdiag(i, b == 1);
            for (int k = k0; k < k1; k++) EXPECT(level[P.col[k]] < level[i], "sweep %d: row %d is not above the level of row %d", b, i, P.col[k]);
        }
        if (!widths.empty() && fill == 0) {
            EXPECT(W.nlev() == (int)widths.size(), "sweep %d: %d levels, %zu layers", b, W.nlev(), widths.size());
            for (int l = 0; l < W.nlev(); l++)
                EXPECT(W.lev_ptr[l + 1] - W.lev_ptr[l] == widths[b ? widths.size() - 1 - l : l], "sweep %d: level %d is not its layer", b, l);
        }
        int lev = 0, pos = 0;
        bool last_folded = false;
        for (int a = 0; a < W.nlaunch(); a++) {
            const Bilu4Launch L = W.launch(a);
            EXPECT(L.l0 == lev && L.l1 > L.l0 && L.l1 <= W.nlev() && L.p0 == pos && L.p0 == W.lev_ptr[L.l0] && L.p1 == W.lev_ptr[L.l1], "sweep %d: launch %d does not continue the one before", b, a);
            int narrow = 0;
            for (int l = L.l0; l < L.l1; l++) narrow += W.lev_ptr[l + 1] - W.lev_ptr[l] < 64;
            const bool rule = L.l1 - L.l0 > 1 || L.p1 - L.p0 < 64; // more than one level, or fewer block rows than one workgroup serves
            EXPECT(L.folded() == rule, "sweep %d: launch %d: folded() is %d, the rule says %d", b, a, (int)L.folded(), (int)rule);
            EXPECT(rule ? narrow == L.l1 - L.l0 && !last_folded : narrow == 0, "sweep %d: launch %d mixes wide and narrow levels, or splits a run", b, a);
            lev = L.l1, pos = L.p1, last_folded = rule;
        }
        EXPECT(lev == W.nlev() && pos == nb, "sweep %d: the launches end at level %d, position %d", b, lev, pos);
    }

    // the factorisation: the same bits whatever the thread count
    std::mt19937 rng(7 + nb);
    std::vector<double> coef(16 * col.size());
    for (int i = 0; i < nb; i++)
        for (int k = ptr[i]; k < ptr[i + 1]; k++)
            for (int e = 0; e < 16; e++)
                coef[16 * (size_t)k + e] = ((int)(rng() % 2001) - 1000) / (col[k] == i ? 20000.0 : 4000.0 * (ptr[i + 1] - ptr[i])) + (col[k] == i && e % 5 == 0 ? 4.0 : 0.0);
    std::vector<double> v1(16 * (size_t)P.nblocks(), -1.0), vt(v1.size());
    const int r1 = bilu4_factor(P, S.sweep[0], ptr.data(), col.data(), coef.data(), false, 1, v1.data());
    EXPECT(r1 == -1, "a pivot was refused (row %d)", r1);
    for (int threads : {3, 4, 16}) {
        std::fill(vt.begin(), vt.end(), -2.0);
        const int rt = bilu4_factor(P, S.sweep[0], ptr.data(), col.data(), coef.data(), false, threads, vt.data());
        EXPECT(rt == -1, "a pivot was refused with %d threads (row %d)", threads, rt);
        EXPECT(v1.empty() || !memcmp(v1.data(), vt.data(), sizeof(double) * v1.size()), "the factor differs between 1 and %d threads", threads);
    }
    if (fill == 0) check_dilu(name, S, ptr, col, coef, widths);
    if (fill == 0) check_dilu_dev(name, S, ptr, col, rng);

    // the device refactor's plan
    Bilu4DevPlan D;
    bilu4dev_plan(S, ptr.data(), col.data(), &D);
    std::vector<long long> start[2] = {std::vector<long long>(nb + 1, 0), std::vector<long long>(nb + 1, 0)}; // by position: blocks of the rows before it
    for (int b = 0; b < 2; b++)
        for (int q = 0; q < nb; q++) {
            EXPECT((b ? D.bpos : D.fpos)[S.sweep[b].perm[q]] == q, "sweep %d: the position table does not invert perm at %d", b, q);
            const auto [k0, k1] = P.offdiag(S.sweep[b].perm[q], b == 1);
            start[b][q + 1] = start[b][q] + (k1 - k0);
        }
    EXPECT(D.nL == start[0][nb] && D.nU == start[1][nb] && D.nL + D.nU + nb == P.nblocks() && (long long)D.gather.size() == P.nblocks(), "the plan's block counts");
    auto home = [&](int i, int j) -> long long { // of block (i, j) in L | U | D, or -1
        const int k = where[(size_t)i * nb + j];
        if (k < 0) return -1;
        if (k < P.diag[i]) return start[0][D.fpos[i]] + (k - P.ptr[i]);
        return k == P.diag[i] ? D.nL + D.nU + D.bpos[i] : D.nL + start[1][D.bpos[i]] + (k - P.diag[i] - 1);
    };
    long long hits = 0;
    for (int h : D.gather) hits += h >= 0;
    EXPECT(hits == (long long)col.size(), "gather names %lld blocks of the matrix, which has %zu", hits, col.size());
    for (int i = 0; i < nb; i++)
        for (int k = ptr[i]; k < ptr[i + 1]; k++) EXPECT(home(i, col[k]) >= 0 && D.gather[home(i, col[k])] == k, "block %d of the matrix does not land on its home", k);
    EXPECT((long long)D.upd_ptr.size() == D.nL + 1 && D.upd_ptr[0] == 0 && D.upd_ptr.back() == (long long)D.upd.size(), "upd_ptr");
    long long e = 0, at = 0, pairs = 0;
    for (int q = 0; q < nb; q++) {
        const int i = S.sweep[0].perm[q];
        for (int k = P.ptr[i]; k < P.diag[i]; k++, e++) {
            const int p = P.col[k];
            EXPECT(D.upd_ptr[e] == at && D.upd_ptr[e + 1] - at == P.ptr[p + 1] - P.diag[p] - 1, "upd_ptr of L block (%d, %d)", i, p);
            for (int kk = P.diag[p] + 1; kk < P.ptr[p + 1]; kk++, at++) {
                EXPECT(D.upd[at] == home(i, P.col[kk]), "upd of (%d, %d) x (%d, %d) is %d, the home of (%d, %d) is %lld", i, p, p, P.col[kk], D.upd[at], i, P.col[kk], home(i, P.col[kk]));
                pairs += D.upd[at] >= 0;
            }
        }
    }
    EXPECT(pairs == D.update_pairs, "update_pairs");

    // the one-launch solve's plan, replayed
    Bilu4OnePlan O;
    bilu4one_plan(S, &O);
    for (int G : {1, 2, 7, 256})
        for (int b = 0; b < 2; b++) {
            const std::string why = bilu4one_check(S, b, O.sweep[b], G);
            EXPECT(why.empty(), "G = %d: %s", G, why.c_str());
        }
}

int main()
{
    std::mt19937 rng(23);
    int patterns = 0;
    for (int fill = 0; fill <= 3; fill++) {
        check("empty", Rows(), fill);
        check("diagonal", Rows(150), fill);
        Rows chain(150);
        for (int i = 1; i < 150; i++) chain[i].push_back(i - 1), chain[i - 1].push_back(i);
        check("chain", chain, fill);
        patterns += 3;
        for (int it = 0; it < 12; it++, patterns++) {
            const bool banded = it % 2 == 0;
            const int nb = 1 + (int)(rng() % 300), band = 1 + (int)(rng() % 12), per_row = (int)(rng() % 4);
            Rows rows(nb);
            for (int i = 0; i < nb; i++)
                for (int e = 0; e < per_row; e++) {
                    const int j = banded ? i - band + (int)(rng() % (2 * band + 1)) : (int)(rng() % nb);
                    if (j >= 0 && j < nb) rows[i].push_back(j);
                }
            check(banded ? "random banded" : "random unsymmetric", rows, fill);
        }
    }
    const std::vector<std::vector<int>> layers = {{1}, {63}, {64}, {65}, {129}, {1, 63, 64, 65, 1, 1, 128, 129, 2, 63, 64, 200, 1}, {63, 64, 63, 64, 65, 63}, {129, 1, 129}};
    for (const std::vector<int>& w : layers)
        for (int extra : {0, 3}) check("layered", layered(w, extra, rng), 0, w), patterns++;
    // fill 0 only, for the DILU device plan: a strictly lower pattern (L blocks, no U block), and symmetric patterns that lost a fifth of
    // their off-diagonal blocks one by one, so that some (i, j) have no (j, i)
    Rows lower(150);
    for (int i = 1; i < 150; i++)
        for (int e = 0; e < 3; e++) lower[i].push_back((int)(rng() % i));
    check("lower only", lower, 0), patterns++;
    for (int it = 0; it < 12; it++, patterns++) {
        const int nb = 2 + (int)(rng() % 300), band = 1 + (int)(rng() % 12);
        std::vector<std::pair<int, int>> blocks;
        for (int i = 0; i < nb; i++)
            for (int e = 0; e < 3; e++) {
                const int j = i - band + (int)(rng() % (2 * band + 1));
                if (j >= 0 && j < nb && j != i) blocks.push_back({i, j}), blocks.push_back({j, i});
            }
        Rows rows(nb);
        for (const auto& b : blocks)
            if (rng() % 5) rows[b.first].push_back(b.second);
        check("dropped mates", rows, 0);
    }
    if (planted != caught) bad++;
    printf("DILU device plans %d teeth planted %d caught %d\n", dilu_plans, planted, caught);
    printf("block ILU plans: patterns %d bad %d\n", patterns, bad);
    return bad != 0;
}
