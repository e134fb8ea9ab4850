// bilu4_plan.hpp — host side of the 4x4-block ILU(k) preconditioner (mi_bilu4_*, include/mi355_spmv.h): symbolic
// factorisation, numeric factorisation, dependency levels, the launch schedule of the level-scheduled solve, and the
// pattern-only plan of the numeric factorisation on the device (Bilu4DevPlan, at the end; kernels in bilu4_factor.hpp).
// Plain C++ (no HIP), like ring_plan.hpp / partition.hpp, so that it can be probed and tested without a GPU.
//
// What it stands for in the reference: PCILU on the BAIJ-4 Jacobian (src/solve_newton.c:1156-1164; 4 levels of fill, natural
// ordering) with the hand-written numeric factorisation src/kernels/baij4_factor_avx2.c:114-170 — row by row, IKJ, the
// INVERSE of every diagonal block kept.
//
// ARITHMETIC (part of the interface, restated by tests/bilu4_model.py):
//   * a 4x4 product entry is ONE chain from a rounded product: p = fma(a3,b3, fma(a2,b2, fma(a1,b1, a0*b0))), a = a row of
//     the left block, b = a column of the right block;
//   * an update is one rounded subtraction w - p;
//   * the diagonal block is inverted in place by Gauss-Jordan without pivoting, for k = 0..3: d = a[k][k], refused when
//     |d| < 1e-12; piv = 1/d; a[k][k] = 1; row k is multiplied by piv (one rounded product per entry); then for every other
//     row i in ascending order: f = a[i][k], a[i][k] = 0, a[i][j] = a[i][j] - f*a[k][j] for j = 0..3 (a rounded product, then a
//     rounded subtraction: never an fma).
// The functions below are compiled with floating-point contraction OFF (pragma here, -ffp-contract=off in the Makefile):
// every fma is written out, nothing else may be fused or reassociated.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace mi355 {

constexpr int kBiluRowsPerWG = 64;      // block rows one workgroup of the solve kernels serves (four lanes per block row)
constexpr double kBiluPivotMin = 1e-12; // the reference's zero-pivot threshold (baij4_factor_avx2.c)

// the factor's block pattern: row i holds its L blocks (columns < i), the diagonal block, its U blocks, columns ascending
struct Bilu4Pattern {
    int nb = 0;
    std::vector<int> ptr, col, diag; // diag[i]: position of block (i, i)
    long long nblocks() const { return ptr.empty() ? 0 : ptr.back(); }
    // [first, second): the off-diagonal blocks of row i that a sweep reads — its L blocks forward, its U blocks backward
    std::pair<int, int> offdiag(int i, bool backward) const
    {
        return backward ? std::make_pair(diag[i] + 1, ptr[i + 1]) : std::make_pair(ptr[i], diag[i]);
    }
};

// one launch of a sweep: the levels [l0, l1), which are the positions [p0, p1).  THE FOLDING RULE, stated here and nowhere else:
// a launch is a folded run — one workgroup that steps through its levels with workgroup barriers — iff it has more than one
// level or fewer block rows than one workgroup serves; any other launch is one wide level, kBiluRowsPerWG positions per workgroup.
// The solve's kernels, the factor's kernels and the one-launch form's chunks all follow it.
struct Bilu4Launch {
    int l0, l1, p0, p1;
    bool folded() const { return l1 - l0 > 1 || p1 - p0 < kBiluRowsPerWG; }
};

// one sweep's schedule: rows in level-major order (ascending row number inside a level) and the launches after folding
struct Bilu4Sweep {
    std::vector<int> perm;       // [nb] position -> block row
    std::vector<int> lev_ptr;    // [nlev + 1] first position of each level
    std::vector<int> launch_ptr; // [nlaunch + 1] first level of each launch
    int nlev() const { return (int)lev_ptr.size() - 1; }
    int nlaunch() const { return (int)launch_ptr.size() - 1; }
    Bilu4Launch launch(int a) const { return Bilu4Launch{launch_ptr[a], launch_ptr[a + 1], lev_ptr[launch_ptr[a]], lev_ptr[launch_ptr[a + 1]]}; }
};

// what a pattern and a fill fix: the factor's pattern and both sweeps.  Index 0 is the forward sweep, 1 the backward one, everywhere.
struct Bilu4Schedule {
    Bilu4Pattern pat;
    Bilu4Sweep sweep[2];
};

// MI_ERR_ARG conditions of a square block pattern; empty string = fine
inline std::string bilu4_check_pattern(int nb, const int* ptrow, const int* indcol)
{
    if (ptrow[0] != 0) return "ptrow[0] must be 0";
    for (int i = 0; i < nb; i++) {
        if (ptrow[i + 1] < ptrow[i]) return "ptrow decreases at block row " + std::to_string(i);
        bool diag = false;
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++) {
            const int j = indcol[k];
            if (j < 0 || j >= nb) return "block column out of range (the matrix must be square) in block row " + std::to_string(i);
            if (k > ptrow[i] && j <= indcol[k - 1])
                return std::string(j == indcol[k - 1] ? "duplicate" : "unsorted") + " block columns in block row " + std::to_string(i);
            diag |= j == i;
        }
        if (!diag) return "missing diagonal block in block row " + std::to_string(i);
    }
    return std::string();
}

// Symbolic ILU(fill), natural ordering.  Level-of-fill rule: an original block has level 0; block (i, j) reached through pivot p
// gets lev(i, p) + lev(p, j) + 1, the MINIMUM over all pivots that reach it, and is kept when that is <= fill.  The pivots of
// row i are its blocks left of the diagonal in ascending column order, fill blocks included.
inline void bilu4_symbolic(int nb, const int* ptrow, const int* indcol, int fill, Bilu4Pattern* P)
{
    P->nb = nb;
    P->ptr.assign(1, 0);
    P->col.clear();
    P->diag.assign(nb, 0);
    std::vector<int> lev; // level of every kept block, beside P->col
    std::vector<int> rc, rl, mc, ml;
    for (int i = 0; i < nb; i++) {
        rc.assign(indcol + ptrow[i], indcol + ptrow[i + 1]);
        rl.assign(rc.size(), 0);
        if (fill > 0) {
            for (size_t a = 0; a < rc.size() && rc[a] < i; a++) {
                const int p = rc[a], lp = rl[a];
                // merge the U part of row p (columns > p) into the rest of row i
                mc.assign(rc.begin(), rc.begin() + a + 1);
                ml.assign(rl.begin(), rl.begin() + a + 1);
                size_t b = a + 1;
                int k = P->diag[p] + 1;
                const int ke = P->ptr[p + 1];
                while (b < rc.size() || k < ke) {
                    const int cb = b < rc.size() ? rc[b] : nb, ck = k < ke ? P->col[k] : nb;
                    if (ck < cb) {
                        const int nl = lp + lev[k] + 1;
                        if (nl <= fill) {
                            mc.push_back(ck);
                            ml.push_back(nl);
                        }
                        k++;
                    } else if (cb < ck) {
                        mc.push_back(cb);
                        ml.push_back(rl[b]);
                        b++;
                    } else {
                        mc.push_back(cb);
                        ml.push_back(std::min(rl[b], lp + lev[k] + 1));
                        b++;
                        k++;
                    }
                }
                rc.swap(mc);
                rl.swap(ml);
            }
        }
        for (size_t a = 0; a < rc.size(); a++) {
            if (rc[a] == i) P->diag[i] = (int)P->col.size();
            P->col.push_back(rc[a]);
            lev.push_back(rl[a]);
        }
        P->ptr.push_back((int)P->col.size());
    }
}

// dependency levels: forward, level(i) = 1 + max level of the L columns of row i (0 without any); backward the same over the
// U columns, rows taken from the last to the first
inline void bilu4_levels(const Bilu4Pattern& P, bool backward, std::vector<int>* level, int* nlev)
{
    level->assign(P.nb, 0);
    int top = 0;
    for (int t = 0; t < P.nb; t++) {
        const int i = backward ? P.nb - 1 - t : t;
        const auto [k0, k1] = P.offdiag(i, backward);
        int l = 0;
        for (int k = k0; k < k1; k++) l = std::max(l, (*level)[P.col[k]] + 1);
        (*level)[i] = l;
        top = std::max(top, l + 1);
    }
    *nlev = P.nb ? top : 0;
}

// level-major order and launches: one launch per level, except that a run of consecutive NARROW levels (fewer block rows than
// one workgroup serves) is one launch of one workgroup that steps through the run with workgroup barriers
inline void bilu4_sweep(const Bilu4Pattern& P, bool backward, Bilu4Sweep* S)
{
    std::vector<int> level;
    int nlev = 0;
    bilu4_levels(P, backward, &level, &nlev);
    S->lev_ptr.assign(nlev + 1, 0);
    for (int i = 0; i < P.nb; i++) S->lev_ptr[level[i] + 1]++;
    for (int l = 0; l < nlev; l++) S->lev_ptr[l + 1] += S->lev_ptr[l];
    S->perm.assign(P.nb, 0);
    std::vector<int> fill_at(S->lev_ptr.begin(), S->lev_ptr.end() - (nlev ? 1 : 0));
    for (int i = 0; i < P.nb; i++) S->perm[fill_at[level[i]]++] = i; // ascending row number inside a level
    S->launch_ptr.assign(1, 0);
    for (int l = 0; l < nlev;) {
        int e = l + 1;
        if (S->lev_ptr[l + 1] - S->lev_ptr[l] < kBiluRowsPerWG)
            while (e < nlev && S->lev_ptr[e + 1] - S->lev_ptr[e] < kBiluRowsPerWG) e++;
        S->launch_ptr.push_back(e);
        l = e;
    }
}

inline void bilu4_schedule(int nb, const int* ptrow, const int* indcol, int fill, Bilu4Schedule* S)
{
    bilu4_symbolic(nb, ptrow, indcol, fill, &S->pat);
    for (int b = 0; b < 2; b++) bilu4_sweep(S->pat, b == 1, &S->sweep[b]);
}

// ---------------------------------------------------------------- numeric
// c = a . b, every entry one chain from a rounded product
static inline void bilu4_matmul(const double* a, const double* b, double* c)
{
    for (int r = 0; r < 4; r++)
        for (int q = 0; q < 4; q++) {
            double p = a[4 * r] * b[q];
            p = std::fma(a[4 * r + 1], b[4 + q], p);
            p = std::fma(a[4 * r + 2], b[8 + q], p);
            p = std::fma(a[4 * r + 3], b[12 + q], p);
            c[4 * r + q] = p;
        }
}

// in-place Gauss-Jordan inverse without pivoting, the order fixed at the top of this file; false: a pivot below the threshold
static inline bool bilu4_invert(double* a)
{
    for (int k = 0; k < 4; k++) {
        const double d = a[5 * k];
        if (std::fabs(d) < kBiluPivotMin) return false;
        const double piv = 1.0 / d;
        a[5 * k] = 1.0;
        for (int j = 0; j < 4; j++) a[4 * k + j] = a[4 * k + j] * piv;
        for (int i = 0; i < 4; i++) {
            if (i == k) continue;
            const double f = a[4 * i + k];
            a[4 * i + k] = 0.0;
            for (int j = 0; j < 4; j++) {
                const double t = f * a[4 * k + j];
                a[4 * i + j] = a[4 * i + j] - t;
            }
        }
    }
    return true;
}

// one block of the caller's into row-major: transposed where the caller's blocks are column-major
static inline void bilu4_block_in(const double* from, bool colmajor, double* dst)
{
    if (colmajor)
        for (int r = 0; r < 4; r++)
            for (int q = 0; q < 4; q++) dst[4 * r + q] = from[4 * q + r];
    else
        std::memcpy(dst, from, sizeof(double) * 16);
}

// one row of the IKJ factorisation (baij4_factor_avx2.c:114-170) into val; pos: a per-thread map block column -> place in the
// row, all -1 on entry and on return.  false: zero pivot in this row.  src: null, or the caller's index of every block of
// (ptrow, indcol) — an ordered handle's pattern is the permuted one (bilu4_order.hpp), coef stays the caller's.
static inline bool bilu4_factor_row(const Bilu4Pattern& P, int i, const int* ptrow, const int* indcol, const double* coef, bool colmajor,
                                    double* val, int* pos, const int* src = nullptr)
{
    const int k0 = P.ptr[i], k1 = P.ptr[i + 1];
    double* w = val + 16 * (size_t)k0;
    std::memset(w, 0, sizeof(double) * 16 * (size_t)(k1 - k0));
    for (int k = k0; k < k1; k++) pos[P.col[k]] = k - k0;
    for (int k = ptrow[i]; k < ptrow[i + 1]; k++) bilu4_block_in(coef + 16 * (size_t)(src ? src[k] : k), colmajor, w + 16 * (size_t)pos[indcol[k]]);
    double m[16], pr[16];
    for (int k = k0; k < P.diag[i]; k++) {
        double* wk = w + 16 * (size_t)(k - k0);
        bool zero = true;
        for (int e = 0; e < 16; e++) zero &= wk[e] == 0.0;
        if (zero) continue;
        const int p = P.col[k];
        bilu4_matmul(wk, val + 16 * (size_t)P.diag[p], m);
        std::memcpy(wk, m, sizeof(m));
        for (int kk = P.diag[p] + 1; kk < P.ptr[p + 1]; kk++) {
            const int at = pos[P.col[kk]];
            if (at < 0) continue;
            bilu4_matmul(m, val + 16 * (size_t)kk, pr);
            double* wj = w + 16 * (size_t)at;
            for (int e = 0; e < 16; e++) wj[e] = wj[e] - pr[e];
        }
    }
    for (int k = k0; k < k1; k++) pos[P.col[k]] = -1;
    return bilu4_invert(val + 16 * (size_t)P.diag[i]);
}

// THE LEVEL LOOP of the host numerics (the factorisation below, the DILU pivots of dilu4_plan.hpp): over the forward schedule F,
// level by level.  The rows of a level are independent, so a level of at least kBiluRowsPerWG rows is dealt to the threads in
// contiguous shares; every row is computed by one thread in one fixed order — row_fn(block row, thread index), false: its pivot
// was refused — so the bits do not depend on the thread count.  Returns -1, or the lowest block row that was refused; the loop
// stops behind the first level with a refusal (later rows would use what was refused), and rows behind it are not meaningful.
inline int bilu4_level_threads(int threads) { return std::max(1, std::min(threads, 64)); }

template <class RowFn>
inline int bilu4_for_level_rows(const Bilu4Sweep& F, int threads, RowFn&& row_fn)
{
    const int nb = (int)F.perm.size();
    threads = bilu4_level_threads(threads);
    std::atomic<int> bad(nb);
    auto note = [&](int i) {
        int cur = bad.load();
        while (i < cur && !bad.compare_exchange_weak(cur, i)) {}
    };
    for (int l = 0; l < F.nlev(); l++) {
        const int p0 = F.lev_ptr[l], p1 = F.lev_ptr[l + 1];
        const int T = (p1 - p0 >= kBiluRowsPerWG) ? threads : 1; // a row costs ~10 us, a thread ~20 us to start
        auto share = [&](int t) {
            const int a = p0 + (int)((long long)(p1 - p0) * t / T), b = p0 + (int)((long long)(p1 - p0) * (t + 1) / T);
            for (int q = a; q < b; q++)
                if (!row_fn(F.perm[q], t)) note(F.perm[q]);
        };
        if (T == 1) {
            share(0);
        } else {
            std::vector<std::thread> th;
            for (int t = 1; t < T; t++) th.emplace_back(share, t);
            share(0);
            for (auto& x : th) x.join();
        }
        if (bad.load() < nb) break;
    }
    return bad.load() < nb ? bad.load() : -1;
}

// The numeric factorisation over the forward schedule F (bilu4_for_level_rows; a per-thread pos table for bilu4_factor_row).
// Returns -1, or the lowest block row whose pivot was refused (rows behind it are then not meaningful).
inline int bilu4_factor(const Bilu4Pattern& P, const Bilu4Sweep& F, const int* ptrow, const int* indcol, const double* coef, bool colmajor,
                        int threads, double* val, const int* src = nullptr)
{
    std::vector<std::vector<int>> pos(bilu4_level_threads(threads), std::vector<int>(P.nb, -1));
    return bilu4_for_level_rows(F, threads, [&](int i, int t) { return bilu4_factor_row(P, i, ptrow, indcol, coef, colmajor, val, pos[t].data(), src); });
}

// ---------------------------------------------------------------- the device refactor's plan (mi_bilu4dev_*)
// Pattern-only tables of the numeric factorisation on the GPU (bilu4_factor.hpp), built once per handle.  The device factor is
// three arrays: the L blocks in the forward sweep's order, the U blocks in the backward sweep's order, and the inverted diagonal
// blocks by backward position.  A block of the factor is named by ONE index into their concatenation L | U | D ("home").
constexpr int kBiluDevFixedLaunches = 1; // launches of a device refactor besides the forward sweep's: the one that clears and scatters

struct Bilu4DevPlan {
    long long nL = 0, nU = 0;       // blocks of the L and of the U array (the D array has nb)
    std::vector<int> fpos, bpos;    // [nb] block row -> its position in the forward / backward order
    std::vector<int> gather;        // [nL + nU + nb] by home: the block of the caller's matrix that lands there, or -1 (a fill
                                    // block: it starts every refactor as zeros).  The scatter map, stored by destination, so that
                                    // clearing and scattering are one launch that writes every block of the factor exactly once.
    std::vector<long long> upd_ptr; // [nL + 1] by L block (i, p): its first entry in upd
    std::vector<int> upd;           // per U block (p, j) of the pivot row, in row p's order: the home of block (i, j), or -1
    long long update_pairs = 0;     // entries of upd that are not -1
    long long bytes() const
    {
        return (long long)sizeof(int) * (long long)(fpos.size() + bpos.size() + gather.size() + upd.size() + 1) // + the refusal word
               + (long long)sizeof(long long) * (long long)upd_ptr.size();
    }
};

// (src: as in bilu4_factor_row)
inline void bilu4dev_plan(const Bilu4Schedule& S, const int* ptrow, const int* indcol, Bilu4DevPlan* D, const int* src = nullptr)
{
    const Bilu4Pattern& P = S.pat;
    const Bilu4Sweep& F = S.sweep[0];
    const int nb = P.nb;
    D->fpos.assign(nb, 0);
    D->bpos.assign(nb, 0);
    for (int q = 0; q < nb; q++) D->fpos[F.perm[q]] = q, D->bpos[S.sweep[1].perm[q]] = q;
    // home of every block of the pattern: the level-major copies list a row's blocks in the pattern's order
    std::vector<int> home((size_t)P.nblocks());
    long long n = 0;
    for (int b = 0; b < 2; b++) {
        for (int q = 0; q < nb; q++) {
            const auto [k0, k1] = P.offdiag(S.sweep[b].perm[q], b == 1);
            for (int k = k0; k < k1; k++) home[k] = (int)n++;
        }
        (b ? D->nU : D->nL) = n - (b ? D->nL : 0);
    }
    for (int i = 0; i < nb; i++) home[P.diag[i]] = (int)(n + D->bpos[i]);
    D->gather.assign((size_t)P.nblocks(), -1);
    for (int i = 0; i < nb; i++) {
        int k = P.ptr[i]; // both column lists ascend, and the matrix's is a subset of the factor's
        for (int a = ptrow[i]; a < ptrow[i + 1]; a++) {
            while (P.col[k] != indcol[a]) k++;
            D->gather[home[k]] = src ? src[a] : a;
        }
    }
    D->upd_ptr.assign(1, 0);
    D->upd.clear();
    D->update_pairs = 0;
    for (int q = 0; q < nb; q++) {
        const int i = F.perm[q];
        for (int k = P.ptr[i]; k < P.diag[i]; k++) {
            const int p = P.col[k];
            int at = k + 1; // row p's U columns are > p: merge them with the rest of row i
            for (int kk = P.diag[p] + 1; kk < P.ptr[p + 1]; kk++) {
                while (at < P.ptr[i + 1] && P.col[at] < P.col[kk]) at++;
                const bool hit = at < P.ptr[i + 1] && P.col[at] == P.col[kk];
                D->upd.push_back(hit ? home[at] : -1);
                D->update_pairs += hit;
            }
            D->upd_ptr.push_back((long long)D->upd.size());
        }
    }
}

// ---------------------------------------------------------------- the one-launch solve's plan (mi_bilu4one_*)
// Pattern-only tables of the one-launch form of the solve (bilu4_solve_one.hpp).  The unit of work is a CHUNK of one sweep's
// positions: a wide level (>= kBiluRowsPerWG block rows) is cut into chunks of kBiluRowsPerWG consecutive positions (the last may
// be shorter), a folded run of narrow levels is ONE chunk.  Chunks are numbered in position order; chunk c goes to workgroup
// c mod G and every workgroup takes its chunks in ascending order.  A chunk's dependencies are the distinct chunks of the SAME
// sweep that hold a block row one of its off-diagonal block columns names (itself excepted: a folded chunk orders its own levels
// with workgroup barriers), ascending; all of them have a smaller index, so with all G workgroups resident the lowest unfinished
// chunk always has finished dependencies and an owner with nothing earlier left: the dealing cannot stall (bilu4one_check replays it).
constexpr int kBiluOneMaxDeps = 256;   // one polling lane per dependency: the lanes of a workgroup
constexpr int kBiluOnePlanFor = 256;   // workgroups the probe replays when the caller names none (one per CU of an MI355X)
constexpr int kBiluOneFlagBytes = 64;  // every chunk's flag on a line of its own

struct Bilu4OneSweep {
    std::vector<int> chunk_pos; // [nchunks + 1] first position of each chunk
    std::vector<int> chunk_lev; // [nchunks + 1] first level of each chunk
    std::vector<int> dep_ptr;   // [nchunks + 1]
    std::vector<int> dep;       // chunk numbers, ascending per chunk
    int max_deps = 0;
    int nchunks() const { return (int)chunk_pos.size() - 1; }
    // the levels chunk c walks: a chunk of a wide level that the next chunk continues starts and ends in that level
    int lev_end(int c) const { return chunk_lev[c + 1] == chunk_lev[c] ? chunk_lev[c] + 1 : chunk_lev[c + 1]; }
};

struct Bilu4OnePlan {
    Bilu4OneSweep sweep[2]; // forward, backward
    bool eligible() const { return sweep[0].max_deps <= kBiluOneMaxDeps && sweep[1].max_deps <= kBiluOneMaxDeps; }
    std::string why_not() const
    {
        for (int b = 0; b < 2; b++)
            if (sweep[b].max_deps > kBiluOneMaxDeps)
                return std::string("a chunk of the ") + (b ? "backward" : "forward") + " sweep waits for " + std::to_string(sweep[b].max_deps) +
                       " chunks; the one-launch form polls with one lane per dependency, at most " + std::to_string(kBiluOneMaxDeps);
        return std::string();
    }
    long long bytes() const // tables, flags, the counter between the sweeps
    {
        long long n = 0;
        for (const Bilu4OneSweep& s : sweep)
            n += (long long)sizeof(int) * (long long)(s.chunk_pos.size() + s.chunk_lev.size() + s.dep_ptr.size() + s.dep.size()) +
                 (long long)kBiluOneFlagBytes * s.nchunks();
        return n + kBiluOneFlagBytes;
    }
};

// block row -> chunk of sweep S
inline std::vector<int> bilu4one_chunk_of_row(const Bilu4Sweep& S, const Bilu4OneSweep& O)
{
    std::vector<int> of(S.perm.size(), -1);
    for (int c = 0; c < O.nchunks(); c++)
        for (int q = O.chunk_pos[c]; q < O.chunk_pos[c + 1]; q++) of[S.perm[q]] = c;
    return of;
}

inline void bilu4one_sweep(const Bilu4Schedule& Sch, int b, Bilu4OneSweep* O)
{
    const Bilu4Pattern& P = Sch.pat;
    const Bilu4Sweep& S = Sch.sweep[b];
    O->chunk_pos.clear(), O->chunk_lev.clear(), O->dep.clear();
    for (int a = 0; a < S.nlaunch(); a++) {
        const Bilu4Launch L = S.launch(a);
        for (int p = L.p0; p < L.p1; p += L.folded() ? L.p1 - L.p0 : kBiluRowsPerWG) {
            O->chunk_pos.push_back(p);
            O->chunk_lev.push_back(L.l0);
        }
    }
    O->chunk_pos.push_back(P.nb);
    O->chunk_lev.push_back(S.nlev());
    const std::vector<int> of = bilu4one_chunk_of_row(S, *O);
    std::vector<int> seen(O->nchunks(), -1);
    O->dep_ptr.assign(1, 0);
    O->max_deps = 0;
    for (int c = 0; c < O->nchunks(); c++) {
        const size_t first = O->dep.size();
        for (int q = O->chunk_pos[c]; q < O->chunk_pos[c + 1]; q++) {
            const auto [k0, k1] = P.offdiag(S.perm[q], b == 1);
            for (int k = k0; k < k1; k++) {
                const int d = of[P.col[k]];
                if (d != c && seen[d] != c) seen[d] = c, O->dep.push_back(d);
            }
        }
        std::sort(O->dep.begin() + first, O->dep.end());
        O->dep_ptr.push_back((int)O->dep.size());
        O->max_deps = std::max(O->max_deps, (int)(O->dep.size() - first));
    }
}

inline void bilu4one_plan(const Bilu4Schedule& S, Bilu4OnePlan* O)
{
    for (int b = 0; b < 2; b++) bilu4one_sweep(S, b, &O->sweep[b]);
}

// What the kernel relies on, checked against the pattern and the schedule, and the dealing REPLAYED for G workgroups: every
// workgroup steps through its chunks in order and takes the next one only when all its dependencies are finished.  Empty string,
// or the first violation (of sweep b's tables O).
inline std::string bilu4one_check(const Bilu4Schedule& Sch, int b, const Bilu4OneSweep& O, int G)
{
    const Bilu4Pattern& P = Sch.pat;
    const Bilu4Sweep& S = Sch.sweep[b];
    const std::string sw = b ? "backward" : "forward";
    const int nch = O.nchunks(), nb = P.nb;
    if (nch < 0 || (int)O.chunk_lev.size() != nch + 1 || (int)O.dep_ptr.size() != nch + 1) return sw + ": table sizes disagree";
    std::vector<int> cover(nb, 0);
    for (int c = 0; c < nch; c++) {
        if (O.chunk_pos[c] < 0 || O.chunk_pos[c + 1] > nb || O.chunk_pos[c] >= O.chunk_pos[c + 1]) return sw + ": chunk " + std::to_string(c) + " is empty or out of range";
        for (int q = O.chunk_pos[c]; q < O.chunk_pos[c + 1]; q++) cover[q]++;
    }
    for (int q = 0; q < nb; q++)
        if (cover[q] != 1) return sw + ": position " + std::to_string(q) + (cover[q] ? " is in two chunks" : " is in no chunk");
    for (int c = 0; c < nch; c++) {
        const int l0 = O.chunk_lev[c], l1 = O.lev_end(c);
        if (l0 < 0 || l1 > S.nlev() || O.chunk_pos[c] < S.lev_ptr[l0] || O.chunk_pos[c + 1] > S.lev_ptr[l1])
            return sw + ": chunk " + std::to_string(c) + " does not lie in the levels it names";
        int wide = 0;
        for (int l = l0; l < l1; l++) wide += S.lev_ptr[l + 1] - S.lev_ptr[l] >= kBiluRowsPerWG;
        if (wide > 1 || (wide == 1 && l1 - l0 > 1)) return sw + ": chunk " + std::to_string(c) + " spans a wide level and another level";
        if (wide == 1 && O.chunk_pos[c + 1] - O.chunk_pos[c] > kBiluRowsPerWG) return sw + ": chunk " + std::to_string(c) + " of a wide level has more rows than a workgroup serves";
    }
    const std::vector<int> of = bilu4one_chunk_of_row(S, O);
    for (int c = 0; c < nch; c++) {
        const int* d0 = O.dep.data() + O.dep_ptr[c];
        const int* d1 = O.dep.data() + O.dep_ptr[c + 1];
        for (const int* d = d0; d < d1; d++)
            if (*d < 0 || *d >= c || (d > d0 && *d <= d[-1]))
                return sw + ": chunk " + std::to_string(c) + " lists dependency " + std::to_string(*d) + (*d >= c ? ", not a smaller index" : ", out of order");
        for (int q = O.chunk_pos[c]; q < O.chunk_pos[c + 1]; q++) {
            const int i = S.perm[q];
            const auto [k0, k1] = P.offdiag(i, b == 1);
            for (int k = k0; k < k1; k++)
                if (of[P.col[k]] != c && !std::binary_search(d0, d1, of[P.col[k]]))
                    return sw + ": block row " + std::to_string(i) + " names block row " + std::to_string(P.col[k]) + ", whose chunk " +
                           std::to_string(of[P.col[k]]) + " is not on the list of chunk " + std::to_string(c);
        }
    }
    // the replay: rounds over the workgroups until nobody moves
    std::vector<char> done(nch, 0);
    std::vector<int> next(G);
    for (int g = 0; g < G; g++) next[g] = g;
    int left = nch;
    for (bool moved = true; moved && left > 0;) {
        moved = false;
        for (int g = 0; g < G; g++)
            while (next[g] < nch) {
                const int c = next[g];
                bool ready = true;
                for (int d = O.dep_ptr[c]; d < O.dep_ptr[c + 1] && ready; d++) ready = done[O.dep[d]] != 0;
                if (!ready) break;
                done[c] = 1, next[g] += G, left--, moved = true;
            }
    }
    if (left > 0) {
        int c = 0;
        while (done[c]) c++;
        return sw + ": the dealing stalls for " + std::to_string(G) + " workgroups at chunk " + std::to_string(c);
    }
    return std::string();
}

} // namespace mi355
