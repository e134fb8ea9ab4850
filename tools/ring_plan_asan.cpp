// tools/ring_plan_asan.cpp — dev tool: the planners of the ring, multi-ring and tile kernels (ring_plan.hpp, mring_plan.hpp, tile_plan.hpp)
// under the host sanitizers, every table checked by brute force WITHOUT the builders' intermediates.  Patterns: ten families (narrow
// band, multi-band, band with far couplings, a scattered row every few hundred, one row longer than a block, rows that outspan the
// 5 120- and the 11 264-entry ring, empty rows at the front, middle and end, all rows empty, ghost columns, random) at n in {0, 1, 2,
// 63, 64, 65, 255, 256, 257, 1 000, 20 000}.
//   ring:   every kRingConfigs entry as it is and with 8 and 1 workgroups per unit (the same planner with runs of many blocks at these
//           sizes: a 20 000-row matrix has ~100 blocks, the real grids start at 256 runs), row alignment 0 / 1 / 64, without and with a
//           ghost range; one pattern of three million nonzeros with the real grids at the default alignment (a prefix and a suffix of the columns): build_ring_plan, build_ring_slots, ring_plan_census, build_run_deps
//           (configuration 4, square, every run of kind 1), the invariants mi_ring_plan_probe and mi_spmk_plan_probe state, restated,
//           and the over-read contract of spmv_ring.hpp (ring_overread below quotes the index expressions);
//   mring:  row alignment 0 / 1 / 64, skew 0 / 30: check_mring_plan, mring_plan_census, the table lengths the kernel's grid indexes;
//   tile:   0, 1, 3 and 16 threads, row alignment 1 / 64: check_tile_plan, the same arrays whatever the thread count, the padding;
//   teeth:  corruptions planted in built plans (a base off by one, a slot changed, a block's new_cnt reduced, run ranges swapped or
//           overlapping, a list entry duplicated, ...), each of which its checker must report.
// Address and undefined behaviour, then (a second binary) threads — the tile planner's pool:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -Inavierstokes_amd/csrc -o /tmp/ring_plan_asan tools/ring_plan_asan.cpp && /tmp/ring_plan_asan
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -Inavierstokes_amd/csrc -o /tmp/ring_plan_tsan tools/ring_plan_asan.cpp && /tmp/ring_plan_tsan
#include "mring_plan.hpp"
#include "ring_plan.hpp"
#include "tile_plan.hpp"
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
using namespace mi355;

static int bad = 0;
#define EXPECT(cond, ...)                     \
    do {                                      \
        if (!(cond)) {                        \
            printf("%s: ", what.c_str());     \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
            bad++;                            \
            return;                           \
        }                                     \
    } while (0)

struct Pattern {
    std::string name;
    int n = 0, ncols = 0;
    std::vector<int> ptr, col;
    long long nnz() const { return (long long)col.size(); }
    bool square() const { return ncols == n; }
};

constexpr int kFamilies = 10;
static const int kSizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 20000};
constexpr int kNumSizes = (int)(sizeof(kSizes) / sizeof(kSizes[0]));

// family f at n rows.  Families that need columns a small matrix does not have (a row longer than a block, a span beyond a ring)
// take them as ghost columns: ncols = max(n, what the family needs)
static Pattern make_pattern(int f, int n, std::mt19937& rng)
{
    static const char* names[kFamilies] = {"narrow", "multi-band", "far couplings", "scattered rows", "wide row", "span 5121", "span 11265",
                                           "empty rows", "all empty", "ghost columns"};
    Pattern A;
    A.n = n;
    A.ncols = std::max(n, 1);
    std::vector<std::vector<int>> rows((size_t)n);
    auto put = [&](int i, long long j) { if (j >= 0 && j < A.ncols) rows[i].push_back((int)j); };
    auto band = [&](int i, int half) { for (int d = -half; d <= half; d++) put(i, (long long)i + d); };
    switch (f) {
    case 0: for (int i = 0; i < n; i++) band(i, 2); break;
    case 1: {
        const int gap = n / 7 + 3;
        for (int i = 0; i < n; i++)
            for (int b = -2; b <= 2; b++)
                for (int d = -1; d <= 1; d++) put(i, (long long)i + (long long)b * gap + d);
        break;
    }
    case 2:
        for (int i = 0; i < n; i++) {
            band(i, 4);
            if (i % 50 == 7) put(i, rng() % A.ncols), put(i, rng() % A.ncols);
        }
        break;
    case 3:
        for (int i = 0; i < n; i++) {
            band(i, 3);
            if (i % 300 == 1)
                for (int e = 0; e < 24; e++) put(i, rng() % A.ncols);
        }
        break;
    case 4: // one row of 4 500 nonzeros (more than either nnzb) in the middle of a band; its columns 3 apart (a span beyond both rings)
        A.ncols = std::max(n, 13600);
        for (int i = 0; i < n; i++) {
            band(i, 5);
            if (i == n / 2)
                for (int e = 0; e < 4500; e++) put(i, 3LL * e + (e & 1));
        }
        break;
    case 5:
    case 6: { // every 97th row reaches one column further than the ring holds
        const int reach = f == 5 ? 5120 : 11264;
        A.ncols = std::max(n, reach + 400);
        for (int i = 0; i < n; i++) {
            band(i, 3);
            if (i % 97 == 3) put(i, i + reach < A.ncols ? (long long)i + reach : (long long)i - reach);
        }
        break;
    }
    case 7: // empty rows at the front, in the middle and at the end
        for (int i = 0; i < n; i++) {
            const int e = n / 8 + 1;
            if (i < e || (i >= n / 2 && i < n / 2 + e) || i >= n - e) continue;
            band(i, 6);
        }
        break;
    case 8: break;
    case 9: // a banded partition's piece: the first and last rows reach into ghost columns behind the owned ones
        A.ncols = n + n / 4 + 3;
        for (int i = 0; i < n; i++) {
            band(i, 4);
            if (i < n / 10 + 1) put(i, n + i % (n / 8 + 1));
            if (i >= n - n / 10 - 1) put(i, n + n / 8 + 1 + (n - 1 - i) % (n / 8 + 1));
        }
        break;
    }
    A.name = std::string(names[f]) + " n " + std::to_string(n);
    A.ptr.assign(1, 0);
    for (int i = 0; i < n; i++) {
        std::sort(rows[i].begin(), rows[i].end());
        rows[i].erase(std::unique(rows[i].begin(), rows[i].end()), rows[i].end());
        A.col.insert(A.col.end(), rows[i].begin(), rows[i].end());
        A.ptr.push_back((int)A.col.size());
    }
    return A;
}

// random: rows of 0 to 40 nonzeros (columns in CSR order NOT sorted, now and then repeated), near the diagonal or anywhere
static Pattern random_pattern(int it, std::mt19937& rng)
{
    Pattern A;
    A.n = (int)(rng() % 3000);
    A.ncols = A.n + (it % 3 == 0 ? (int)(rng() % 500) : 0);
    if (A.ncols == 0) A.ncols = 1;
    const int maxlen = 1 + (int)(rng() % 40), reach = 1 + (int)(rng() % 2000), far_pct = (int)(rng() % 12), empty_pct = (int)(rng() % 30);
    A.ptr.assign(1, 0);
    for (int i = 0; i < A.n; i++) {
        const int len = (int)(rng() % 100) < empty_pct ? 0 : (int)(rng() % (maxlen + 1));
        for (int e = 0; e < len; e++) {
            long long j = (int)(rng() % 100) < far_pct ? (long long)(rng() % A.ncols) : (long long)i - reach + (long long)(rng() % (2 * reach + 1));
            j = std::min<long long>(std::max<long long>(j, 0), A.ncols - 1);
            A.col.push_back((int)j);
        }
        A.ptr.push_back((int)A.col.size());
    }
    A.name = "random " + std::to_string(it) + " n " + std::to_string(A.n);
    return A;
}

// ---------------------------------------------------------------- ring
// Over-read contract.  The ring loop of spmv_ring.hpp issues, for the blocks lb = 0 .. (nb rounded up to D) + D - 1 of its run (blocks
// behind the run are sentinels {r0 + rows, p0 + nnz, 0, 0} {0, 0, 0, 0} of the run's last record), with m0 = {r0, p0, rows, nnz},
// m1 = {new_lo, new_cnt, base, flags}:
//     ring_load_coefs(c[s], A.coef + m0.y, tid & ((m1.w & 1) ? -1 : 0))  — cb = base + lane; cb[i * T], i < PER (8-byte form), or
//                                                                          RingCoef2 cb[i * T], i < PER / 2 (pairs: 2 doubles each)
//     sl[s] = (slotv + min(b_begin + lb, bslot_last) * T)[tid]           — SlotVec = PER 16-bit entries
//     rp = A.ptrow + m0.x + tid;  pr[s] = {rp[0], rp[1]}
//     rm[s] = (A.rowmap + m0.x)[tid]
// and the plain path and the second row pass address rows < r0 + rows and nonzeros < p0 + nnz of their own block only.
// Returns the largest index formed into each array over the whole plan, for depth D.
struct RingReach { long long val = -1, slot = -1, ptrow = -1, rowmap = -1; };
static RingReach ring_overread(const RingPlanHost& P, int D)
{
    const int T = P.cfg.threads, per = P.cfg.nnzb / T;
    const bool pair = ring_pairs(T);
    RingReach R;
    for (int g = 0; g < P.wgs; g++) {
        const int b0 = P.run_rng[2 * g], nb = P.run_rng[2 * g + 1] - b0;
        if (nb <= 0 || !(P.run_ok[g] & 1)) continue;
        const int* last = &P.plan[(size_t)8 * (b0 + nb - 1)];
        const int issued = (nb + D - 1) / D * D + D;
        for (int lb = 0; lb < issued; lb++) {
            const int* Q = &P.plan[(size_t)8 * (b0 + std::min(lb, nb - 1))];
            const long long r0 = lb < nb ? Q[0] : last[0] + last[2], p0 = lb < nb ? Q[1] : (long long)last[1] + last[3];
            const int flags = lb < nb ? Q[7] : 0;
            const long long lane = (flags & 1) ? T - 1 : 0;
            R.val = std::max(R.val, p0 + (pair ? 2 * (lane + (long long)(per / 2 - 1) * T) + 1 : lane + (long long)(per - 1) * T));
            R.slot = std::max(R.slot, ((long long)std::min(b0 + lb, P.nblk - 1) * T + (T - 1)) * per + per - 1);
            R.ptrow = std::max(R.ptrow, r0 + T - 1 + 1);
            R.rowmap = std::max(R.rowmap, r0 + T - 1);
        }
    }
    return R;
}

// the invariants of a ring plan, by brute force; nullptr or the first violation
static const char* ring_check(const Pattern& A, const RingPlanHost& P, const std::vector<unsigned short>& slots, int ghost_lo, int ghost_hi)
{
    const RingConfig& c = P.cfg;
    const int T = c.threads, per = c.nnzb / T, ring = c.ring, nblk = P.nblk, max_rows = c.id == 4 ? T : 2 * T;
    if (nblk == 0) return A.n == 0 ? nullptr : "no blocks for a matrix with rows";
    if ((long long)P.plan.size() != 8LL * nblk || (int)P.run_ok.size() != P.wgs || (int)P.run_rng.size() != 2 * P.wgs || (int)P.run_halo.size() != P.wgs ||
        (long long)slots.size() != (long long)nblk * c.nnzb)
        return "table sizes";
    if (P.wgs < c.wg_unit || P.wgs % c.wg_unit != 0 || P.bpw != (nblk + P.wgs - 1) / P.wgs) return "grid is not whole units, or bpw is not blocks / runs rounded up";
    std::vector<int> run_of((size_t)nblk, -1);
    for (int g = 0; g < P.wgs; g++) {
        const int b0 = P.run_rng[2 * g], b1 = P.run_rng[2 * g + 1];
        if (b0 < 0 || b1 < b0 || b1 > nblk) return "run range out of bounds";
        if (b1 - b0 > kRingMaxB) return "a run longer than kRingMaxB";
        for (int b = b0; b < b1; b++) {
            if (run_of[b] >= 0) return "a block belongs to two runs";
            run_of[b] = g;
        }
    }
    // blocks cover rows and nonzeros once and in order
    long long next_row = 0, next_nz = 0;
    for (int b = 0; b < nblk; b++) {
        const int* Q = &P.plan[(size_t)8 * b];
        if (run_of[b] < 0) return "a block belongs to no run";
        const int rows = Q[7] == 2 ? Q[4] : Q[2];
        if (Q[0] != next_row || Q[1] != next_nz || rows < 1 || Q[0] + (long long)rows > A.n) return "blocks do not cover the rows / nonzeros in order";
        if (Q[3] != A.ptr[Q[0] + rows] - A.ptr[Q[0]]) return "a block's nonzero count disagrees with ptrow";
        next_row += rows;
        next_nz += Q[3];
    }
    if (next_row != A.n || next_nz != A.nnz()) return "blocks do not cover the matrix";
    // the window of every run, replayed: content[s] = the column slot s holds (stamp[s]: of which run)
    std::vector<int> content((size_t)ring, -1), stamp((size_t)ring, -1);
    int bad_runs = 0;
    long long bad_nnz = 0;
    for (int g = 0; g < P.wgs; g++) {
        const int b0 = P.run_rng[2 * g], b1 = P.run_rng[2 * g + 1], kind = P.run_ok[g];
        if (kind != 0 && kind != 1 && kind != 3) return "run kind";
        int nplain = 0, halo = 0;
        long long run_nnz = 0;
        for (int b = b0; b < b1; b++) {
            const int* Q = &P.plan[(size_t)8 * b];
            const int p0 = Q[1], nn = Q[3], base = Q[6], flags = Q[7];
            run_nnz += nn;
            for (int k = p0; k < p0 + nn; k++) halo |= ghost_lo < ghost_hi && (A.col[k] < ghost_lo || A.col[k] >= ghost_hi);
            if (kind == 0) {
                if (flags == 2 || (flags && nn == 0)) return "a block of a plain run is PLAIN, or empty with a flag"; // (the plain path reads {r0, p0, rows, nnz} only)
                continue;
            }
            if (P.lean && (flags == 2 ? Q[4] : Q[2]) > T) return "a LEAN plan holds a block of more than T rows";
            if (nn == 0) {
                if (flags != 0 || Q[5] != 0) return "an empty block carries a flag or brings columns";
                continue;
            }
            if (flags == 2) {
                if (Q[2] != 0 || Q[5] != 0) return "a PLAIN block is visible to the ring loop";
                nplain++;
                bad_nnz += nn;
                continue;
            }
            if (flags != 1) return "a block with nonzeros in a served run is neither served nor PLAIN";
            if (nn > c.nnzb || Q[2] > max_rows) return "a served block over the kernel's limits";
            int cmin = 0x7fffffff, cmax = -1;
            for (int k = p0; k < p0 + nn; k++) cmin = std::min(cmin, A.col[k]), cmax = std::max(cmax, A.col[k]);
            if (cmax - cmin + 1 > ring) return "a served block's columns do not fit one window";
            if (Q[4] < 0 || Q[5] < 0 || Q[5] > ring || (long long)Q[4] + Q[5] > A.ncols) return "new columns out of range";
            if (base < 0 || base % ring != 0) return "a ring base that is no multiple of the ring";
            if (P.lean && Q[5] > T && b != b0) return "a LEAN plan brings more than T new columns into a block inside a run";
            for (int col = Q[4]; col < Q[4] + Q[5]; col++) { // ring_slot: col - base, less the ring once
                int s = col - base;
                if (s >= ring) s -= ring;
                if (s < 0 || s >= ring) return "a new column falls outside the ring";
                content[s] = col, stamp[s] = g;
            }
            for (int k = 0; k < nn; k++) {
                const int col = A.col[p0 + k];
                int s = col - base;
                if (s >= ring) s -= ring;
                if (s < 0 || s >= ring) return "a nonzero's column has no slot under the block's base";
                if (stamp[s] != g || content[s] != col) return "a nonzero's column is not in the window when its block runs";
            }
            // the 16-bit stream in the kernel's thread order: thread t, element i is nonzero t + i T (pairs: 2 (t + (i / 2) T) + (i & 1)),
            // the block's last nonzero again beyond its end
            const unsigned short* o = &slots[(size_t)b * c.nnzb];
            for (int t = 0; t < T; t++)
                for (int i = 0; i < per; i++) {
                    const int k = std::min(ring_pairs(T) ? 2 * (t + (i / 2) * T) + (i & 1) : t + i * T, nn - 1);
                    int want = A.col[p0 + k] - base;
                    if (want >= ring) want -= ring;
                    if (o[t * per + i] != want || o[t * per + i] >= ring) return "a 16-bit slot is not its column less the base";
                }
        }
        if (b1 > b0 && kind != 0 && (nplain > kRingMaxPlain || (kind == 3) != (nplain > 0))) return "a run's kind disagrees with its PLAIN blocks";
        if (kind == 0) bad_runs++, bad_nnz += run_nnz;
        if (P.run_halo[g] != halo) return "run_halo disagrees with the run's columns";
    }
    if (bad_runs != P.bad_runs || bad_nnz != P.bad_nnz) return "bad_runs / bad_nnz disagree with a direct count";
    return nullptr;
}

// a run's dependency list against the matrix (square, every run of kind 1): every column its rows name and every column its
// lanes load lies in the rows of a run on the list
static const char* deps_check(const Pattern& A, const RingPlanHost& P, const std::vector<int>& dp, const std::vector<int>& dr)
{
    const int W = P.wgs, T = P.cfg.threads, n = A.n;
    if ((int)dp.size() != W + 1 || dp[0] != 0 || dp[W] != (int)dr.size()) return "dep_ptr";
    std::vector<int> owner((size_t)n, -1);
    for (int g = 0; g < W; g++)
        for (int b = P.run_rng[2 * g]; b < P.run_rng[2 * g + 1]; b++)
            for (int r = P.plan[(size_t)8 * b]; r < P.plan[(size_t)8 * b] + P.plan[(size_t)8 * b + 2]; r++) owner[r] = g;
    std::vector<int> on((size_t)W, -1);
    for (int g = 0; g < W; g++) {
        if (dp[g + 1] < dp[g]) return "dep_ptr descends";
        for (int j = dp[g]; j < dp[g + 1]; j++) {
            if (dr[j] < 0 || dr[j] >= W || on[dr[j]] == g) return "a dependency out of range or listed twice";
            on[dr[j]] = g;
        }
        for (int b = P.run_rng[2 * g]; b < P.run_rng[2 * g + 1]; b++) {
            const int* Q = &P.plan[(size_t)8 * b];
            for (int k = Q[1]; k < Q[1] + Q[3]; k++)
                if (on[owner[A.col[k]]] != g) return "a run names a column of a run that is not on its list";
            for (int col = Q[4]; col <= std::min(n - 1, Q[4] + std::max(Q[5], T) - 1); col++)
                if (on[owner[col]] != g) return "a run loads a column of a run that is not on its list";
        }
    }
    return nullptr;
}

static int ring_plans = 0, ring_deps = 0, planted = 0, caught = 0;

static void plant(const std::string& what, const char* kind, const char* verdict)
{
    planted++;
    if (verdict) caught++;
    else printf("%s: planted and not reported: %s\n", what.c_str(), kind), bad++;
}

static void ring_case(const Pattern& A, const std::vector<int>& row_min, const std::vector<int>& row_max, const RingConfig& cfg, int row_align, bool ghost, bool teeth)
{
    const std::string what = A.name + ", ring config " + std::to_string(cfg.id) + " unit " + std::to_string(cfg.wg_unit) + " align " + std::to_string(row_align) + (ghost ? " ghosts" : "");
    ring_plans++;
    const int ghost_lo = ghost ? A.ncols / 10 : 0, ghost_hi = ghost ? A.ncols - A.ncols / 10 : 0;
    RingPlanHost P;
    build_ring_plan(cfg, A.n, A.ptr.data(), row_min.data(), row_max.data(), P, ghost_lo, ghost_hi, row_align);
    std::vector<unsigned short> slots;
    if (P.nblk > 0) build_ring_slots(P, A.col.data(), slots);
    const char* why = ring_check(A, P, slots, ghost_lo, ghost_hi);
    EXPECT(!why, "%s", why);
    if (P.nblk == 0) return;
    // the census against direct counts
    long long cen[kRingCensusLen];
    ring_plan_census(P, A.col.data(), cen);
    long long served = 0, plain = 0, empty = 0, kind0 = 0, nonempty = 0, longest = 0;
    bool uniform = true;
    for (int g = 0; g < P.wgs; g++) {
        const int b0 = P.run_rng[2 * g], b1 = P.run_rng[2 * g + 1];
        uniform = uniform && b0 == std::min(P.nblk, g * P.bpw) && b1 == std::min(P.nblk, (g + 1) * P.bpw);
        nonempty += b1 > b0;
        kind0 += b1 > b0 && P.run_ok[g] == 0;
        longest = std::max<long long>(longest, b1 - b0);
        for (int b = b0; b < b1; b++) {
            const int* Q = &P.plan[(size_t)8 * b];
            empty += Q[3] == 0;
            served += Q[7] == 1 && P.run_ok[g] != 0;
            plain += Q[7] == 2;
        }
    }
    EXPECT(cen[kRcBlocks] == P.nblk && cen[kRcTableLen] == P.wgs && cen[kRcBpw] == P.bpw && cen[kRcServed] == served && cen[kRcPlain] == plain && cen[kRcEmpty] == empty &&
               cen[kRcRunsKind0] == kind0 && cen[kRcRunsNonEmpty] == nonempty && cen[kRcRunsIdle] == P.wgs - nonempty && cen[kRcRunMax] == longest &&
               cen[kRcUniform] == (uniform ? 1 : 0) && cen[kRcLean] == (P.lean && cfg.id == 4 ? 1 : 0),
           "the census disagrees with a direct count");
    // the over-read contract, at every depth the kernel is built with
    for (int D : {2, 3, 4}) {
        const RingReach R = ring_overread(P, D);
        EXPECT(R.val < A.nnz() + kRingPadNnz, "depth %d: a lane forms value index %lld, the padded stream ends at %lld", D, R.val, A.nnz() + kRingPadNnz);
        EXPECT(R.slot < (long long)slots.size(), "depth %d: a lane forms slot index %lld of %zu", D, R.slot, slots.size());
        EXPECT(R.ptrow < (long long)A.n + 1 + kRingPadRows && R.rowmap < (long long)A.n + kRingPadRows, "depth %d: ptrow index %lld / row map index %lld past the padding", D, R.ptrow, R.rowmap);
    }
    bool all_kind1 = true;
    for (int g = 0; g < P.wgs; g++) all_kind1 = all_kind1 && P.run_ok[g] == 1;
    if (cfg.id == 4 && A.square() && all_kind1) {
        std::vector<int> dp, dr;
        build_run_deps(P, A.n, dp, dr);
        why = deps_check(A, P, dp, dr);
        EXPECT(!why, "%s", why);
        ring_deps++;
        if (teeth) { // a list without a run that one of the run's nonzeros names a row of
            std::vector<int> owner((size_t)A.n, -1);
            for (int g = 0; g < P.wgs; g++)
                for (int b = P.run_rng[2 * g]; b < P.run_rng[2 * g + 1]; b++)
                    for (int r = P.plan[(size_t)8 * b]; r < P.plan[(size_t)8 * b] + P.plan[(size_t)8 * b + 2]; r++) owner[r] = g;
            int g = -1, lost = -1;
            for (int v = 0; v < P.wgs && g < 0; v++)
                for (int b = P.run_rng[2 * v]; b < P.run_rng[2 * v + 1] && g < 0; b++)
                    for (int k = P.plan[(size_t)8 * b + 1]; k < P.plan[(size_t)8 * b + 1] + P.plan[(size_t)8 * b + 3]; k++)
                        if (owner[A.col[k]] != v) { g = v, lost = owner[A.col[k]]; break; }
            EXPECT(g >= 0, "no run names another's rows");
            std::vector<int> dp2(dp), dr2;
            for (int v = 0; v < P.wgs; v++) {
                dp2[v] = (int)dr2.size();
                for (int j = dp[v]; j < dp[v + 1]; j++)
                    if (v != g || dr[j] != lost) dr2.push_back(dr[j]);
            }
            dp2[P.wgs] = (int)dr2.size();
            plant(what, "a dependency dropped", deps_check(A, P, dp2, dr2));
        }
    }
    if (!teeth) return;
    // teeth, planted in a served block that brings new columns up to its own largest column
    int tb = -1;
    for (int b = 0; b < P.nblk && tb < 0; b++) {
        const int* Q = &P.plan[(size_t)8 * b];
        if (Q[7] != 1 || Q[5] <= 0) continue;
        int cmax = -1;
        for (int k = Q[1]; k < Q[1] + Q[3]; k++) cmax = std::max(cmax, A.col[k]);
        if (cmax == Q[4] + Q[5] - 1) tb = b;
    }
    EXPECT(tb >= 0, "no block to plant a corruption in");
    {
        RingPlanHost C(P);
        C.plan[(size_t)8 * tb + 6] += 1;
        plant(what, "a base off by one", ring_check(A, C, slots, ghost_lo, ghost_hi));
    }
    {
        RingPlanHost C(P);
        C.plan[(size_t)8 * tb + 5] -= 1;
        plant(what, "new_cnt reduced by one", ring_check(A, C, slots, ghost_lo, ghost_hi));
    }
    {
        std::vector<unsigned short> S(slots);
        S[(size_t)tb * cfg.nnzb] ^= 1;
        plant(what, "one slot changed", ring_check(A, P, S, ghost_lo, ghost_hi));
    }
    {
        RingPlanHost C(P);
        C.plan[(size_t)8 * tb + 2] -= 1;
        plant(what, "a block's row count reduced by one", ring_check(A, C, slots, ghost_lo, ghost_hi));
    }
    int g1 = -1, g2 = -1; // two runs with blocks, the second behind the first
    for (int g = 0; g < P.wgs; g++)
        if (P.run_rng[2 * g] < P.run_rng[2 * g + 1]) {
            if (g1 < 0) g1 = g;
            else if (g2 < 0 && P.run_rng[2 * g] == P.run_rng[2 * g1 + 1]) g2 = g;
        }
    if (g2 >= 0) {
        RingPlanHost C(P);
        C.run_rng[2 * g1 + 1] += 1; // the next run's first block in both
        plant(what, "a run range one block too long", ring_check(A, C, slots, ghost_lo, ghost_hi));
        // (two whole ranges swapped are no corruption here: a run's window starts cold, and runs need not be in order)
    }
}

// ---------------------------------------------------------------- multi-ring
static int mring_plans = 0;

static void mring_case(const Pattern& A, int row_align, int skew, bool teeth)
{
    const std::string what = A.name + ", mring align " + std::to_string(row_align) + " skew " + std::to_string(skew);
    mring_plans++;
    const int n = A.n;
    MringPlanHost P;
    build_mring_plan(n, A.ptr.data(), A.col.data(), P, row_align, skew);
    const char* why = check_mring_plan(P, n, A.ptr.data(), A.col.data());
    EXPECT(!why, "%s", why);
    if (P.nblk == 0) {
        EXPECT(n == 0, "no blocks");
        return;
    }
    // what the kernel's grid (wgs workgroups, eight XCD shares) indexes
    EXPECT(P.wgs > 0 && P.wgs % kMringXcds == 0 && (long long)P.run_rng.size() == 2LL * P.wgs && (long long)P.run_ok.size() == P.wgs &&
               (long long)P.first.size() == (long long)kMringFirst * P.wgs && (long long)P.plan.size() == (long long)kMringRec * P.nblk &&
               (long long)P.slots.size() == (long long)P.nblk * kMringNnzb,
           "table lengths: wgs %d, run_rng %zu, run_ok %zu, first %zu, plan %zu, slots %zu", P.wgs, P.run_rng.size(), P.run_ok.size(), P.first.size(), P.plan.size(), P.slots.size());
    long long cen[kMringCensusLen];
    mring_plan_census(P, n, A.col.data(), cen);
    long long nonempty = 0, served = 0, plain = 0, empty = 0, kind0 = 0, longest = 0, bad_nnz = 0;
    for (int g = 0; g < P.wgs; g++) {
        const int b0 = P.run_rng[2 * g], b1 = P.run_rng[2 * g + 1];
        nonempty += b1 > b0;
        kind0 += b1 > b0 && P.run_ok[g] == 0;
        longest = std::max<long long>(longest, b1 - b0);
        for (int b = b0; b < b1; b++) {
            const int* Q = &P.plan[(size_t)kMringRec * b];
            empty += Q[3] == 0;
            served += Q[4] == 1 && Q[3] > 0;
            plain += Q[4] == 2;
            bad_nnz += P.run_ok[g] == 0 || Q[4] == 2 ? Q[3] : 0;
            for (int q = 0; q < kMringGroups; q++) // a wave loads x[min(group + lane, ncols - 1)]: clamped above, not below
                EXPECT(Q[8 + q] >= 0, "block %d: group %d starts at column %d", b, q, Q[8 + q]);
        }
    }
    EXPECT(nonempty == P.nruns && cen[kMcBlocks] == P.nblk && cen[kMcTableLen] == P.wgs && cen[kMcRuns] == P.nruns && cen[kMcTablePadded] == P.wgs - nonempty &&
               cen[kMcServed] == served && cen[kMcPlain] == plain && cen[kMcEmpty] == empty && cen[kMcRunsKind0] == kind0 && cen[kMcRunMax] == longest && bad_nnz == P.bad_nnz &&
               P.bad_runs == kind0,
           "the census or the plan's own counts disagree with a direct count");
    if (!teeth) return;
    const int T = kMringThreads, per = kMringNnzb / T;
    // an inner block with a group that one of its own nonzeros reads, and that nonzero
    int tb = -1, tg = -1, tk = -1;
    for (int b = 0; b < P.nblk && tb < 0; b++) {
        const int* Q = &P.plan[(size_t)kMringRec * b];
        if (Q[4] != 1 || Q[5] <= 0) continue;
        for (int q = 0; q < Q[5] && tb < 0; q++)
            for (int k = 0; k < Q[3]; k++)
                if (A.col[Q[1] + k] >= Q[8 + q] && A.col[Q[1] + k] < Q[8 + q] + 64) { tb = b, tg = q, tk = k; break; }
    }
    EXPECT(tb >= 0, "no block to plant a corruption in");
    {
        MringPlanHost C(P);
        C.plan[(size_t)kMringRec * tb + 8 + tg] += 1;
        plant(what, "a group's first column off by one", check_mring_plan(C, n, A.ptr.data(), A.col.data()));
    }
    {
        MringPlanHost C(P);
        C.slots[(size_t)tb * kMringNnzb + ring_slot_pos(T, per, tk)] ^= 1;
        plant(what, "one slot changed", check_mring_plan(C, n, A.ptr.data(), A.col.data()));
    }
    {
        MringPlanHost C(P);
        C.plan[(size_t)kMringRec * tb + 5] -= 1;
        plant(what, "a block's group count reduced by one", check_mring_plan(C, n, A.ptr.data(), A.col.data()));
    }
    {   // the first record of the run that holds tb: the base of a window its first block reads
        int g = 0;
        while (!(P.run_rng[2 * g] <= tb && tb < P.run_rng[2 * g + 1])) g++;
        const int* Q = &P.plan[(size_t)kMringRec * P.run_rng[2 * g]];
        const int* F = &P.first[(size_t)kMringFirst * g];
        int w = -1;
        for (int v = 0; v < kMringK && w < 0; v++)
            for (int k = 0; k < Q[3] && F[5 + v] > 0; k++)
                if (A.col[Q[1] + k] >= F[v] && A.col[Q[1] + k] < F[v] + F[5 + v]) { w = v; break; }
        if (w >= 0 && Q[4] == 1) {
            MringPlanHost C(P);
            C.first[(size_t)kMringFirst * g + w] += 1;
            plant(what, "a run's first window off by one", check_mring_plan(C, n, A.ptr.data(), A.col.data()));
        }
    }
    {   // two runs swapped in the table, their first records left behind: the first and the last run with a served first block
        int g1 = -1, g2 = -1;
        for (int g = 0; g < P.wgs; g++) {
            if (P.run_rng[2 * g] >= P.run_rng[2 * g + 1] || P.plan[(size_t)kMringRec * P.run_rng[2 * g] + 4] != 1) continue;
            if (g1 < 0 || P.run_rng[2 * g] < P.run_rng[2 * g1]) g1 = g;
            if (g2 < 0 || P.run_rng[2 * g] > P.run_rng[2 * g2]) g2 = g;
        }
        if (g1 >= 0 && g1 != g2 && memcmp(&P.first[(size_t)kMringFirst * g1], &P.first[(size_t)kMringFirst * g2], sizeof(int) * kMringFirst)) {
            MringPlanHost C(P);
            std::swap(C.run_rng[2 * g1], C.run_rng[2 * g2]);
            std::swap(C.run_rng[2 * g1 + 1], C.run_rng[2 * g2 + 1]);
            plant(what, "two run ranges swapped", check_mring_plan(C, n, A.ptr.data(), A.col.data()));
        }
    }
}

// ---------------------------------------------------------------- tile
static int tile_plans = 0;

static void tile_case(const Pattern& A, int row_align, bool teeth)
{
    const std::string what = A.name + ", tile align " + std::to_string(row_align);
    TilePlanHost P0;
    bool have = false;
    for (int threads : {0, 1, 3, 16}) {
        tile_plans++;
        TilePlanHost P;
        build_tile_plan(A.n, A.ptr.data(), A.col.data(), P, kTileNnzb, threads, row_align);
        const char* why = check_tile_plan(P, A.n, A.ptr.data(), A.col.data());
        EXPECT(!why, "%d threads: %s", threads, why);
        // what spmv_tile.hpp forms: desc[b], desc[b + 1] for b < nblk; ul[min(tid + i T, U - 1)] inside the block's list; one 16-byte
        // load of 8 slots at slots + s0 + 8 tid, tid < kTileThreads, whatever the block's length; values at p0 + tid + i T < p0 + nnzb
        EXPECT((long long)P.desc.size() == 4LL * (P.nblk + 1), "%d threads: descriptor table", threads);
        if (P.nblk > 0) {
            const int* E = &P.desc[(size_t)4 * P.nblk];
            EXPECT(E[0] == A.n && E[1] == A.nnz() && (long long)P.ulist.size() == (long long)E[2] + kTileThreads && (long long)P.slots.size() == (long long)E[3] + kTilePadNnz,
                   "%d threads: the closing descriptor and the padded lengths", threads);
            long long reach = -1, listed = 0;
            int max_unique = 0;
            for (int b = 0; b < P.nblk; b++) {
                const int* D = &P.desc[(size_t)4 * b];
                const int nn = D[5] - D[1], U = D[6] - D[2];
                if (nn == 0 || nn > P.nnzb) continue;
                reach = std::max(reach, (long long)D[3] + 8 * (kTileThreads - 1) + 7);
                listed += nn;
                max_unique = std::max(max_unique, U);
            }
            EXPECT(reach < (long long)P.slots.size() && kTileNnzb <= kTilePadNnz && kTilePadNnz <= kRingPadNnz, "%d threads: a lane forms slot index %lld of %zu", threads, reach, P.slots.size());
            EXPECT(listed == P.listed && max_unique == P.max_unique, "%d threads: listed / max_unique", threads);
        }
        if (!have) P0 = P, have = true;
        else
            EXPECT(P.nblk == P0.nblk && P.desc == P0.desc && P.ulist == P0.ulist && P.slots == P0.slots && P.listed == P0.listed && P.max_unique == P0.max_unique,
                   "the plan of %d threads differs from the first", threads);
    }
    long long mult8 = 0;
    for (int i = 0; i < A.n; i++) mult8 += A.ptr[i + 1] > A.ptr[i] && (A.ptr[i + 1] - A.ptr[i]) % 8 == 0;
    EXPECT(tile_wants_skew(A.n, A.ptr.data()) == (10 * mult8 > A.n), "tile_wants_skew");
    if (!teeth) return;
    int tb = -1; // a listed block behind the first, of at least two distinct columns
    for (int b = 1; b < P0.nblk && tb < 0; b++)
        if (P0.desc[(size_t)4 * b + 6] - P0.desc[(size_t)4 * b + 2] >= 2) tb = b;
    EXPECT(tb >= 0, "no block to plant a corruption in");
    const int u0 = P0.desc[(size_t)4 * tb + 2], s0 = P0.desc[(size_t)4 * tb + 3];
    auto verdict = [&](const TilePlanHost& C) { return check_tile_plan(C, A.n, A.ptr.data(), A.col.data()); };
    {
        TilePlanHost C(P0);
        C.desc[(size_t)4 * tb + 2] += 1;
        plant(what, "a block's list base off by one", verdict(C));
    }
    {
        TilePlanHost C(P0);
        C.slots[(size_t)s0] ^= 1;
        plant(what, "one slot changed", verdict(C));
    }
    {
        TilePlanHost C(P0);
        C.ulist[(size_t)u0 + 1] = C.ulist[(size_t)u0];
        plant(what, "a list entry duplicated", verdict(C));
    }
    {
        TilePlanHost C(P0);
        for (int j = 0; j < 4; j++) std::swap(C.desc[(size_t)4 * tb + j], C.desc[(size_t)4 * (tb - 1) + j]);
        plant(what, "two descriptors swapped", verdict(C));
    }
    {
        TilePlanHost C(P0);
        C.desc[(size_t)4 * tb + 1] -= 1;
        plant(what, "a block's first nonzero off by one", verdict(C));
    }
}

// ---------------------------------------------------------------- all of it on one pattern
static int patterns = 0;

// the large pattern: the multi-ring planner cuts runs of more than one block only beyond kMringWgUnit = 512 blocks (a million
// nonzeros), the real ring grids likewise, and the tile planner sizes its own pool only from two million nonzeros on.
// 27-point stencil on 48^3 cells: three clusters of columns a plane (2 304) apart, 3 M nonzeros, multi-ring runs of three blocks
static Pattern large_pattern()
{
    Pattern A;
    const int m = 48;
    A.n = A.ncols = m * m * m;
    A.name = "27-point mesh n " + std::to_string(A.n);
    A.ptr.assign(1, 0);
    for (int z = 0; z < m; z++)
        for (int y = 0; y < m; y++)
            for (int x = 0; x < m; x++) {
                for (int dz = -1; dz <= 1; dz++)
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dx = -1; dx <= 1; dx++)
                            if (z + dz >= 0 && z + dz < m && y + dy >= 0 && y + dy < m && x + dx >= 0 && x + dx < m) A.col.push_back(((z + dz) * m + y + dy) * m + x + dx);
                A.ptr.push_back((int)A.col.size());
            }
    return A;
}

// units: the workgroups per unit to plan every ring configuration with (0: the configuration's own), aligns: the row alignments of the
// ring plans; teeth_*: plant corruptions
static void run_pattern(const Pattern& A, std::initializer_list<int> units, std::initializer_list<int> aligns, bool teeth_ring, bool teeth_mring, bool teeth_tile)
{
    patterns++;
    std::vector<int> row_min((size_t)A.n, 0x7fffffff), row_max((size_t)A.n, -1);
    for (int i = 0; i < A.n; i++)
        for (int k = A.ptr[i]; k < A.ptr[i + 1]; k++) row_min[i] = std::min(row_min[i], A.col[k]), row_max[i] = std::max(row_max[i], A.col[k]);
    for (int ci = 0; ci < kNumRingConfigs; ci++)
        for (int unit : units) {
            RingConfig cfg = kRingConfigs[ci];
            if (unit) cfg.wg_unit = unit;
            for (int row_align : aligns)
                for (bool ghost : {false, true}) ring_case(A, row_min, row_max, cfg, row_align, ghost, teeth_ring && unit == *(units.end() - 1) && row_align == 0 && !ghost);
        }
    for (int row_align : {0, 1, 64})
        for (int skew : {0, 30}) mring_case(A, row_align, skew, teeth_mring && row_align == 0);
    for (int row_align : {1, 64}) tile_case(A, row_align, teeth_tile && row_align == 64);
}

int main()
{
    unsetenv("MI355_RING_ROW_ALIGN"); // (the planners' A/B switches: this run is about their defaults)
    unsetenv("MI355_MRING_DEAL");
    std::mt19937 rng(41);
    for (int f = 0; f < kFamilies; f++)
        for (int s = 0; s < kNumSizes; s++) {
            const Pattern A = make_pattern(f, kSizes[s], rng);
            // teeth where the checker has something to bite on, at the largest size: the ring's in the narrow band and beside the empty
            // rows (runs of ten blocks with 8 workgroups per unit), the tile plan's in the multi-band and the far-coupled matrix
            const bool big = kSizes[s] == 20000;
            run_pattern(A, {0, 1, 8}, {0, 1, 64}, big && (f == 0 || f == 7), false, big && (f == 1 || f == 2));
        }
    for (int it = 0; it < 30; it++) run_pattern(random_pattern(it, rng), {0, 1, 8}, {0, 1, 64}, false, false, false);
    run_pattern(large_pattern(), {0}, {0}, true, true, true);
    printf("ring plans %d run-dependency lists %d multi-ring plans %d tile plans %d\n", ring_plans, ring_deps, mring_plans, tile_plans);
    printf("teeth planted %d caught %d\n", planted, caught);
    printf("ring, multi-ring and tile plans: patterns %d bad %d\n", patterns, bad);
    return bad != 0;
}
