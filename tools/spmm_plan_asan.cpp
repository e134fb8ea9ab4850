// tools/spmm_plan_asan.cpp — dev tool: spmm_tile_plan.hpp (the tile plan of the multi-vector product's forms 1-3) under the host address
// and undefined-behaviour sanitizers.  The pattern families of tests/spmm_tile_cases.py are regenerated here and every plan — 128 and 64
// rows per tile, the default caps and small ones, rows sorted and in growth order — is checked by brute force: every block row once, shadows
// naming a live row of their own tile, lists strictly ascending and equal to the set of their rows' columns, every slot naming its block's
// column, umax the longest list, over-cap lists on single rows only, the 16-bit refusal and the empty matrices.  Also here: the x-tile
// lists of the single-vector blocked kernel (bcsr4_tile_plan.hpp) and the row-block table with its census (partition.hpp,
// rowblock_census.hpp) on random patterns:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Inavierstokes_amd/csrc -o /tmp/spmm_plan_asan tools/spmm_plan_asan.cpp && /tmp/spmm_plan_asan
#include "spmm_tile_plan.hpp"
#include "bcsr4_tile_plan.hpp"
#include "rowblock_census.hpp"
#include <cstdio>
#include <random>
#include <set>
#include <string>
using namespace mi355;

static int bad = 0, plans = 0;
#define EXPECT(cond, ...)                                            \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("%s per %d cap %d sort %d: ", name, per, ucap, (int)sorted); \
            printf(__VA_ARGS__);                                     \
            printf("\n");                                            \
            bad++;                                                   \
            return;                                                  \
        }                                                            \
    } while (0)

using Rows = std::vector<std::vector<int>>;

static Rows band(int n, int half, int lo, int hi)
{
    Rows rows;
    for (int r = lo; r < hi; r++) {
        rows.emplace_back();
        for (int c = std::max(lo, r - half); c < std::min(hi, r + half + 1); c++) rows.back().push_back(c);
    }
    (void)n;
    return rows;
}

static void append(Rows& a, const Rows& b) { a.insert(a.end(), b.begin(), b.end()); }

static void check_one(const char* name, const Rows& rows, int per, int ucap, bool sorted, int want_refused)
{
    const int nbr = (int)rows.size();
    std::vector<int> ptr(1, 0), col;
    for (const auto& r : rows) {
        col.insert(col.end(), r.begin(), r.end());
        ptr.push_back((int)col.size());
    }
    // exactly-sized arrays: a read past the pattern is an error the sanitizer sees
    SpmmTilePlanHost P;
    const int rc = build_spmm_tile_plan_host(nbr, ptr.data(), col.data(), per, ucap, sorted, P);
    plans++;
    if (want_refused) {
        EXPECT(rc == -1 && P.ntiles == 0 && P.umax == 0 && P.wg_ptr.empty() && P.rows.empty(), "expected a refusal, got %d", rc);
        return;
    }
    EXPECT(rc == 1, "refused");
    const int nt = P.ntiles;
    EXPECT(nt >= 1 && (int)P.wg_ptr.size() == nt + 1 && (int)P.rows.size() == nt * per && P.per == per, "sizes");
    EXPECT(P.slots.size() == col.size() + 1 && P.slots.back() == 0, "slots: size or pad entry");
    EXPECT((int)P.nodes.size() == P.wg_ptr[nt] + 1 && P.nodes.back() == 0 && P.wg_ptr[0] == 0, "nodes: size or pad entry");
    std::vector<int> tile_of((size_t)nbr, -1);
    int umax = 0;
    for (int t = 0; t < nt; t++) {
        const int u0 = P.wg_ptr[t], u1 = P.wg_ptr[t + 1];
        EXPECT(u0 <= u1, "tile %d: wg_ptr descends", t);
        umax = std::max(umax, u1 - u0);
        std::set<int> live, cols;
        int prev = -1;
        for (int i = 0; i < per; i++) {
            const int r = P.rows[(size_t)t * per + i];
            if (r < 0) continue;
            EXPECT(r < nbr && tile_of[r] == -1, "tile %d: row %d out of range or listed twice", t, r);
            EXPECT(!sorted || r > prev, "tile %d: rows not ascending", t);
            prev = r;
            tile_of[r] = t;
            live.insert(r);
            cols.insert(rows[r].begin(), rows[r].end());
        }
        EXPECT(!live.empty(), "tile %d has no live row", t);
        for (int i = 0; i < per; i++) {
            const int r = P.rows[(size_t)t * per + i];
            EXPECT(r >= 0 || live.count(-1 - r), "tile %d: place %d shadows row %d, not a live row of the tile", t, i, -1 - r);
        }
        EXPECT((int)cols.size() == u1 - u0, "tile %d: list of %d for %d distinct columns", t, u1 - u0, (int)cols.size());
        int k = u0;
        for (int c : cols) { // std::set iterates ascending: the list must be exactly this sequence
            EXPECT(P.nodes[k] == (unsigned)c, "tile %d: list entry %d is %u, not %d", t, k - u0, P.nodes[k], c);
            k++;
        }
        EXPECT(u1 - u0 <= ucap || live.size() == 1, "tile %d: list of %d over the cap with %d rows", t, u1 - u0, (int)live.size());
    }
    EXPECT(umax == P.umax, "umax %d, longest list %d", P.umax, umax);
    for (int r = 0; r < nbr; r++) {
        EXPECT(tile_of[r] >= 0, "row %d in no tile", r);
        const int t = tile_of[r];
        for (int k = ptr[r]; k < ptr[r + 1]; k++) {
            EXPECT(P.slots[k] < P.wg_ptr[t + 1] - P.wg_ptr[t], "block %d: slot beyond the list", k);
            EXPECT(P.nodes[P.wg_ptr[t] + P.slots[k]] == (unsigned)col[k], "block %d: slot names column %u, not %d", k, P.nodes[P.wg_ptr[t] + P.slots[k]], col[k]);
        }
    }
}

static void check(const std::string& nm, const Rows& rows, bool small_caps = false, int want_refused = 0)
{
    const char* name = nm.c_str();
    for (int per : {128, 64}) {
        check_one(name, rows, per, per == 128 ? 368 : 256, true, want_refused);
        check_one(name, rows, per, per == 128 ? 368 : 256, false, want_refused);
        if (small_caps) {
            check_one(name, rows, per, per == 128 ? 40 : 24, true, want_refused);
            check_one(name, rows, per, 12, true, want_refused);
            check_one(name, rows, per, 12, false, want_refused);
            check_one(name, rows, per, 1, true, want_refused);
        }
    }
}

// The x-tile lists of the single-vector blocked kernel (bcsr4_tile_plan.hpp) and the row-block table with its census
// (partition.hpp: build_row_blocks, rowblock_census.hpp), on exactly-sized arrays, against brute force.
static void check_bcsr4_tile_lists(std::mt19937& rng, int nbr, int width, int cap)
{
    std::vector<int> ptr(1, 0), col;
    for (int r = 0; r < nbr; r++) {
        const int len = rng() % 5 == 0 ? 0 : 10 + (int)(rng() % 12);
        for (int j = 0; j < len; j++) col.push_back((int)((r / 64 * 64 + rng() % width) % (nbr + 50)));
        ptr.push_back((int)col.size());
    }
    Bcsr4TileListsHost H;
    build_bcsr4_tile_lists(nbr, ptr.data(), col.data(), 64, cap, H);
    plans++;
    const int groups = (nbr + 63) / 64;
    int longest = 0, at_cap = 0;
    bool fits = true;
    for (int g = 0; g < groups && fits; g++) {
        std::set<int> cols(col.begin() + ptr[64 * g], col.begin() + ptr[std::min(nbr, 64 * g + 64)]);
        longest = std::max(longest, (int)cols.size());
        at_cap += (int)cols.size() == cap;
        fits = (int)cols.size() <= cap;
        if (!fits || (long long)col.size() < kBtileMinBlocks) continue;
        int k = H.wg_ptr[g];
        for (int c : cols) bad += H.nodes[k++] != (unsigned)c;
        bad += k != H.wg_ptr[g + 1];
        for (int b = ptr[64 * g]; b < ptr[std::min(nbr, 64 * g + 64)]; b++) bad += H.nodes[H.wg_ptr[g] + H.slots[b]] != (unsigned)col[b];
    }
    const bool listed = (long long)col.size() >= kBtileMinBlocks;
    if (H.groups != groups || H.built != (listed && fits) || H.max_nodes != (listed ? longest : 0) || H.groups_at_cap != (listed ? at_cap : 0) ||
        (H.built && (H.slots.size() != col.size() + 1 || (int)H.nodes.size() != H.wg_ptr[groups] + 1))) {
        printf("bcsr4 tile lists: %d block rows, width %d, cap %d: wrong answer\n", nbr, width, cap);
        bad++;
    }
}

static void check_row_blocks(std::mt19937& rng, int n, int nnzb, int max_rows, int align)
{
    std::vector<int> ptr(1, 0);
    for (int r = 0; r < n; r++) {
        const unsigned kind = rng() % 16;
        ptr.push_back(ptr.back() + (kind == 0 ? nnzb + (int)(rng() % (2 * nnzb + 2)) : kind < 4 ? 0 : (int)(rng() % 9)));
    }
    std::vector<int> rows, ptrs;
    std::vector<char> why;
    build_row_blocks(n, ptr.data(), nnzb, max_rows, rows, ptrs, align, kRowBlockKeepEighths, &why);
    plans++;
    const int nblk = (int)rows.size() - 1;
    bool ok = (int)why.size() == nblk && rows[0] == 0 && rows[nblk] == n && ptrs[nblk] == (n ? ptr[n] : 0);
    for (int b = 0; b < nblk && ok; b++) {
        const int r0 = rows[b], r1 = rows[b + 1], nn = ptr[r1] - ptr[r0];
        ok = r1 > r0 && r1 - r0 <= max_rows && ptrs[b] == ptr[r0] && (nn <= nnzb || r1 == r0 + 1);
        // a block that was not pulled back could not have taken its next row; one that was ends on a multiple of `align`
        if (ok && !(why[b] & kBlockEndPulledBack) && r1 < n) ok = r1 - r0 == max_rows || ptr[r1 + 1] - ptr[r0] > nnzb;
        if (ok && (why[b] & kBlockEndPulledBack)) ok = r1 % align == 0;
    }
    std::vector<long long> c((size_t)kRowblockCensusLen);
    rowblock_census(n, ptr.data(), nnzb, max_rows / 4, align, rows, ptrs, why, nullptr, false, c.data());
    long long empty = 0, longs = 0;
    for (int b = 0; b < nblk; b++) {
        empty += ptrs[b + 1] == ptrs[b];
        longs += ptrs[b + 1] - ptrs[b] > nnzb;
    }
    if (!ok || c[kRbBlocks] != nblk || c[kRbEmpty] != empty || c[kRbLong] != longs || c[kRbIdleWgs] != 8LL * ((nblk + 7) / 8) - nblk) {
        printf("row blocks: n %d nnzb %d cap %d align %d: wrong table or census\n", n, nnzb, max_rows, align);
        bad++;
    }
}

int main()
{
    {
        std::mt19937 rng(777);
        for (int nbr : {0, 1, 63, 64, 65, 300, 401}) {
            check_bcsr4_tile_lists(rng, nbr, 20, 1024);
            check_bcsr4_tile_lists(rng, nbr, 200, 64);
            check_bcsr4_tile_lists(rng, nbr, 65, 65);
        }
        for (int trial = 0; trial < 60; trial++) {
            const int n = (int)(rng() % 3000);
            check_row_blocks(rng, n, trial % 2 ? 1024 : 2048, 1024, trial % 3 ? 64 : 1);
            check_row_blocks(rng, n, 16, 8, 4);
        }
    }
    { // grid: 3-D 7-point, 11 x 10 x 9
        const int nx = 11, ny = 10, nz = 9;
        Rows rows;
        for (int k = 0; k < nz; k++)
            for (int j = 0; j < ny; j++)
                for (int i = 0; i < nx; i++) {
                    const int me = (k * ny + j) * nx + i;
                    std::vector<int> nb{me};
                    if (i > 0) nb.push_back(me - 1);
                    if (i < nx - 1) nb.push_back(me + 1);
                    if (j > 0) nb.push_back(me - nx);
                    if (j < ny - 1) nb.push_back(me + nx);
                    if (k > 0) nb.push_back(me - nx * ny);
                    if (k < nz - 1) nb.push_back(me + nx * ny);
                    std::sort(nb.begin(), nb.end());
                    rows.push_back(nb);
                }
        check("grid", rows, true);
    }
    for (int n : {127, 128, 129, 63, 64, 65}) { // the block-row count against `per`: one band; diagonal rows with four dense ones
        const int w = (4096 + n - 1) / n + 1;
        Rows rows(n);
        for (int r = 0; r < n; r++)
            for (int c = r; c < r + w; c++) rows[r].push_back(c);
        check("rows:" + std::to_string(n), rows);
        Rows diag(n);
        for (int r = 0; r < n; r++) diag[r].push_back(r);
        const int dense[4] = {1, n / 2, n - 2, n - 3};
        for (int i = 0; i < 4; i++)
            for (int c = 0; c < 1010; c++) diag[dense[i]].push_back(n + 37 * i + c);
        check("rowsdiag:" + std::to_string(n), diag);
    }
    for (int rev = 0; rev < 2; rev++) { // disconnected pieces
        std::vector<int> sizes{1, 2, 63, 64, 65, 127, 128, 129, 300};
        if (rev) std::reverse(sizes.begin(), sizes.end());
        Rows rows;
        int lo = 0;
        for (int m : sizes) {
            append(rows, band(0, 2, lo, lo + m));
            lo += m;
        }
        check(rev ? "components:rev" : "components:fwd", rows, true);
    }
    { // empty rows: first, a run of 128 named by nobody, interleaved, the last three
        Rows rows(1);
        append(rows, band(0, 2, 1, 256));
        rows.resize(384);
        for (int r = 384; r < 584; r++) rows.push_back(r % 2 ? std::vector<int>{r} : std::vector<int>{});
        append(rows, band(0, 3, 584, 584 + 520));
        rows.resize(rows.size() + 3);
        check("empty", rows, true);
    }
    { // row lengths around the pipeline depths
        const int lens[9] = {1, 2, 3, 4, 5, 7, 8, 9, 13};
        Rows rows(801);
        for (int r = 0; r < 801; r++)
            for (int c = r; c < r + lens[r % 9]; c++) rows[r].push_back(c);
        check("lengths", rows, true);
    }
    { // repeated and descending block columns
        Rows rows = band(0, 3, 0, 700);
        rows[10] = {12, 10, 10, 11, 12, 300, 10};
        rows[20] = {24, 23, 22, 21, 20, 5};
        rows[699] = {699, 699};
        check("repeated", rows, true);
    }
    { // rectangular: columns beyond the rows are never seeds; fewer columns than rows
        Rows rows = band(0, 2, 0, 900);
        for (int r = 0; r < 900; r++) rows[r].push_back(900 + (7 * r) % 500);
        check("rect_wide", rows, true);
        Rows tall(1300);
        for (int r = 0; r < 1300; r++) {
            std::set<int> c;
            for (int j = 0; j < 4; j++) c.insert((r + j) % 800);
            tall[r].assign(c.begin(), c.end());
        }
        check("rect_tall", tall);
    }
    for (int L : {602, 603, 1138, 2049, 3414}) { // one long row: halved down to a tile of its own
        Rows rows = band(0, 2, 0, 900);
        rows[450].clear();
        for (int c = 50; c < 50 + L; c++) rows[450].push_back(c);
        check("long:" + std::to_string(L), rows);
    }
    for (int n : {4095, 4096}) {
        Rows rows(n);
        for (int r = 0; r < n; r++) rows[r].push_back(r);
        check("below:" + std::to_string(n), rows);
    }
    { // random patterns: unsymmetric, repeated columns, empty rows, columns beyond the rows
        std::mt19937 rng(12345);
        for (int trial = 0; trial < 40; trial++) {
            const int n = 1 + (int)(rng() % 700), nc = n + (int)(rng() % 300);
            Rows rows(n);
            long long blocks = 0;
            for (int r = 0; r < n; r++) {
                const int len = rng() % 4 == 0 ? 0 : (int)(rng() % 9);
                for (int j = 0; j < len; j++) rows[r].push_back(rng() % 3 ? std::min(nc - 1, r + (int)(rng() % 7)) : (int)(rng() % nc));
                blocks += len;
            }
            check("random " + std::to_string(trial), rows, true, blocks == 0);
        }
    }
    { // the 16-bit refusal, and nothing to list
        for (int L : {65535, 65536}) {
            Rows rows(3);
            rows[0] = {0};
            for (int c = 0; c < L; c++) rows[1].push_back(c);
            rows[2] = {2};
            check("slots " + std::to_string(L), rows, false, L == 65536);
        }
        check("all empty", Rows(300), true, 1);
        check("no rows", Rows(), true, 1);
    }
    printf("plans %d bad %d\n", plans, bad);
    return bad != 0;
}
