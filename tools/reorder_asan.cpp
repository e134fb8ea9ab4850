// tools/reorder_asan.cpp — dev tool: reorder.hpp (build_node_graph, cuthill_mckee, rcm_reorder, permute_csr, mean_column_distance) under the
// host address and undefined-behaviour sanitizers, every result checked by brute force, on the pattern families of tests/reorder_cases.py
// (generated here: paths, block paths, scrambled bands, a node-blocked 3-D stencil standing in for the FE matrix, components with isolated
// nodes and empty rows, a strictly upper band, unsorted and repeated columns, a hub, one very long row) and on random patterns with empty rows,
// duplicates and a 300-entry row — each as a scalar matrix (block = 1) and expanded to 4x4 node blocks (block = 4):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Inavierstokes_amd/csrc -o /tmp/reorder_asan tools/reorder_asan.cpp && /tmp/reorder_asan
#include "partition.hpp"
#include "reorder.hpp"
#include <cstdio>
#include <random>
#include <set>
using namespace mi355;

typedef std::vector<std::vector<int>> Rows;
static int bad = 0, patterns = 0;

static void fail(const char* what, const char* name, int block)
{
    printf("%s (block %d): %s\n", name, block, what);
    bad++;
}

// the rows under a seeded random numbering: every row's terms keep their order
static Rows scrambled(const Rows& rows, std::mt19937& rng)
{
    const int n = (int)rows.size();
    std::vector<int> perm((size_t)n);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    Rows out((size_t)n);
    for (int i = 0; i < n; i++)
        for (int c : rows[i]) out[perm[i]].push_back(perm[c]);
    return out;
}

static void check(const Rows& nodes, int block, const char* name)
{
    patterns++;
    const int nn = (int)nodes.size(), n = nn * block;
    std::vector<int> P(1, 0), C;
    std::vector<double> V;
    for (int i = 0; i < nn; i++)
        for (int q = 0; q < block; q++) {
            for (int c : nodes[i])
                for (int k = 0; k < block; k++) {
                    C.push_back(block * c + k);
                    V.push_back(1.0 + (double)C.size());
                }
            P.push_back((int)C.size());
        }
    if (block == 4 && n > 0 && !csr_has_block4_pattern(n, P.data(), C.data())) return fail("the expanded pattern is not 4x4-blocked", name, block);
    // 1. the node graph: symmetric, sorted, no self loops, no duplicates, and exactly the symmetrised pattern
    std::vector<long long> gptr;
    std::vector<int> gadj;
    build_node_graph(n, P.data(), C.data(), block, gptr, gadj);
    std::set<std::pair<int, int>> edges;
    for (int i = 0; i < nn; i++)
        for (int c : nodes[i])
            if (c != i) edges.insert({i, c}), edges.insert({c, i});
    if ((int)gptr.size() != nn + 1 || gptr[0] != 0 || gptr[nn] != (long long)gadj.size() || gadj.size() != edges.size()) return fail("graph: sizes", name, block);
    for (int b = 0; b < nn; b++) {
        if (gptr[b + 1] < gptr[b]) return fail("graph: pointers decrease", name, block);
        for (long long e = gptr[b]; e < gptr[b + 1]; e++) {
            if (gadj[e] == b) return fail("graph: self loop", name, block);
            if (e > gptr[b] && gadj[e] <= gadj[e - 1]) return fail("graph: list not strictly ascending", name, block);
            if (!edges.count({b, gadj[e]})) return fail("graph: edge the pattern does not have", name, block);
            const int w = gadj[e];
            if (!std::binary_search(gadj.begin() + gptr[w], gadj.begin() + gptr[w + 1], b)) return fail("graph: not symmetric", name, block);
        }
    }
    // 2. Cuthill-McKee visits every node once
    std::vector<int> order;
    cuthill_mckee(nn, gptr, gadj, order);
    std::vector<int> seen((size_t)nn, 0);
    if ((int)order.size() != nn) return fail("cuthill_mckee: wrong number of nodes", name, block);
    for (int v : order) {
        if (v < 0 || v >= nn || seen[v]++) return fail("cuthill_mckee: a node twice or out of range", name, block);
    }
    // 3. perm and iperm are inverse; a node's rows stay together and aligned
    Reorder R;
    rcm_reorder(n, P.data(), C.data(), block, R);
    if ((int)R.perm.size() != n || (int)R.iperm.size() != n || R.block != block) return fail("rcm_reorder: sizes", name, block);
    for (int i = 0; i < n; i++) {
        if (R.perm[i] < 0 || R.perm[i] >= n || R.iperm[R.perm[i]] != i) return fail("perm and iperm are not inverse", name, block);
        if (R.perm[i] % block != i % block || R.perm[i] / block != R.perm[i - i % block] / block) return fail("a node's rows do not stay together", name, block);
    }
    // 4. permute_csr round-trips
    std::vector<int> p2, c2, src;
    std::vector<double> v2;
    permute_csr(n, P.data(), C.data(), V.data(), R, p2, c2, v2, src);
    if ((int)p2.size() != n + 1 || (int)src.size() != n || c2.size() != C.size() || v2.size() != V.size() || p2[0] != 0 || p2[n] != P[n])
        return fail("permute_csr: sizes", name, block);
    for (int ro = 0; ro < n; ro++) {
        const int rn = R.perm[ro], len = P[ro + 1] - P[ro];
        if (p2[rn + 1] - p2[rn] != len || src[rn] != P[ro]) return fail("permute_csr: row length or src_start", name, block);
        for (int k = 0; k < len; k++)
            if (c2[p2[rn] + k] != R.perm[C[P[ro] + k]] || v2[p2[rn] + k] != V[P[ro] + k]) return fail("permute_csr: a (column, value) pair moved", name, block);
    }
    // 5. the spread figures against a direct sum over every nonzero
    long double s0 = 0, s1 = 0;
    for (int r = 0; r < n; r++)
        for (int k = P[r]; k < P[r + 1]; k++) s0 += std::abs(C[k] / block - r / block);
    for (int r = 0; r < n; r++)
        for (int k = p2[r]; k < p2[r + 1]; k++) s1 += std::abs(c2[k] / block - r / block);
    const double d0 = P[n] ? (double)(s0 / P[n]) : 0.0, d1 = P[n] ? (double)(s1 / P[n]) : 0.0;
    if (R.spread_before != d0 || mean_column_distance(n, P.data(), C.data(), block) != d0) return fail("spread_before is not the direct sum", name, block);
    if (R.spread_after != d1 || mean_column_distance(n, p2.data(), c2.data(), block) != d1) return fail("spread_after is not that of the permuted matrix", name, block);
}

static void both(const Rows& nodes, const char* name)
{
    check(nodes, 1, name);
    check(nodes, 4, name);
}

static Rows path(int n, int half = 1)
{
    Rows r((size_t)n);
    for (int i = 0; i < n; i++)
        for (int c = i - half; c <= i + half; c++)
            if (c >= 0 && c < n) r[i].push_back(c);
    return r;
}

int main()
{
    std::mt19937 rng(29);
    both(Rows(), "empty matrix");
    both(Rows(5), "five empty rows");
    for (int n : {1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200}) {
        const Rows t = path(n);
        both(t, "tridiag");
        Reorder R; // the identity: what makes the twin's row map contiguous
        std::vector<int> P(1, 0), C;
        for (auto& r : t) { C.insert(C.end(), r.begin(), r.end()); P.push_back((int)C.size()); }
        rcm_reorder(n, P.data(), C.data(), 1, R);
        for (int i = 0; i < n; i++)
            if (R.perm[i] != i) { fail("RCM of a path is not the identity", "tridiag", 1); break; }
    }
    for (int n : {8, 65, 129, 1000, 1001, 1002}) { // narrow bands, scrambled
        Rows b = path(n, std::min(12, n / 4));
        for (auto& r : b) { // thin out, keep the diagonal
            std::vector<int> k;
            for (int c : r)
                if (c == (int)(&r - &b[0]) || rng() % 10 < 6) k.push_back(c);
            r = k;
        }
        both(scrambled(b, rng), "band");
    }
    for (int m : {3, 4}) { // 27-point stencil on an (m+1)^3 grid, scrambled: the FE matrix's node graph
        const int g = m + 1;
        Rows s((size_t)g * g * g);
        for (int z = 0; z < g; z++) for (int y = 0; y < g; y++) for (int x = 0; x < g; x++)
            for (int dz = -1; dz <= 1; dz++) for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
                const int X = x + dx, Y = y + dy, Z = z + dz;
                if (X >= 0 && X < g && Y >= 0 && Y < g && Z >= 0 && Z < g) s[(size_t)(z * g + y) * g + x].push_back((Z * g + Y) * g + X);
            }
        both(scrambled(s, rng), "stencil");
    }
    { // components: a band, a path, a star, diagonal-only rows, empty rows (named and unnamed), one column nobody names
        Rows r(200);
        for (int i = 0; i < 90; i++) { for (int c = i - 2; c <= i + 2; c++) if (c >= 0 && c < 90) r[i].push_back(c); r[i].push_back(170 + i % 20); }
        for (int i = 90; i < 130; i++) { for (int c = i - 1; c <= i + 1; c++) if (c >= 90 && c < 130) r[i].push_back(c); if (i < 99) r[i].push_back(100 + i); }
        for (int i = 130; i < 150; i++) { r[i].push_back(130); if (i > 130) r[i].push_back(i), r[130].push_back(i); }
        for (int i = 150; i < 170; i++) r[i].push_back(i);
        both(scrambled(r, rng), "components");
    }
    { // strictly upper band, the last rows empty
        Rows r(300);
        for (int i = 0; i < 295; i++) for (int c = i + 1; c < std::min(i + 6, 300); c++) r[i].push_back(c);
        both(scrambled(r, rng), "upper");
    }
    { // unsorted and repeated columns
        Rows r(400);
        for (int i = 0; i < 400; i++) {
            for (int k = 0; k < 10; k++) r[i].push_back(std::min(399, std::max(0, i + (int)(rng() % 17) - 8)));
            r[i].push_back(r[i][0]);
            r[i].push_back(i);
        }
        both(scrambled(r, rng), "unsorted");
    }
    { // hub: row 0 and column 0 dense, plus a band
        Rows r(600);
        for (int c = 0; c < 600; c++) r[0].push_back(c);
        for (int i = 1; i < 600; i++) { r[i].push_back(0); for (int c = i - 1; c <= i + 1; c++) if (c >= 1 && c < 600) r[i].push_back(c); }
        both(scrambled(r, rng), "hub");
    }
    { // one row of 2500 nonzeros, one of 257
        Rows r = path(3000);
        r[17].clear(), r[1000].clear();
        for (int k = 0; k < 2500; k++) r[17].push_back(250 + k);
        for (int k = 0; k < 257; k++) r[1000].push_back(872 + k);
        both(scrambled(r, rng), "long");
    }
    for (int it = 0; it < 220; it++) { // random: empty rows, duplicates, unsymmetric, a 300-entry row, columns near and far
        const int n = 1 + (int)(rng() % 700);
        const int band = 1 + (int)(rng() % (it % 4 == 0 ? n : 20));
        Rows r((size_t)n);
        for (int i = 0; i < n; i++) {
            const int len = rng() % 5 == 0 ? 0 : (int)(rng() % 9);
            for (int k = 0; k < len; k++) r[i].push_back(std::min(n - 1, std::max(0, i + (int)(rng() % (2 * band + 1)) - band)));
            if (len > 1 && rng() % 3 == 0) r[i].push_back(r[i][0]); // a repeated column
        }
        const int big = (int)(rng() % n);
        r[big].clear();
        for (int k = 0; k < 300; k++) r[big].push_back((int)(rng() % n));
        both(it % 2 ? scrambled(r, rng) : r, "random");
    }
    printf("reorder patterns %d bad %d\n", patterns, bad);
    return bad != 0;
}
