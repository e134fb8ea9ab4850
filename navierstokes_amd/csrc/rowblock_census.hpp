// rowblock_census.hpp — host-side (no HIP) census of the row-block table of the stream kernel (spmv_csr_stream<1024>, get_table) and of
// the tile kernel's plan (spmv_csr_tile<2048>, build_tile): which branches of the two kernels the blocks of a matrix reach, so that a
// test can assert that its matrix sits on the limit it is named for (mi_rowblock_census; tests/rowblock_cases.py).
// Counted from the table the handle would run: the same build_row_blocks / build_tile_plan call, the same row_block_align rule.
#pragma once
#include <algorithm>
#include <vector>

#include "partition.hpp"

namespace mi355 {

// order of the counters: include/mi355_spmv.h (MI_ROWBLOCK_CENSUS_LEN) and navierstokes_amd/mpk.py (ROWBLOCK_CENSUS)
enum RowblockCensus {
    kRbBlocks, kRbRowAlign, kRbIdleWgs,
    kRbEmpty, kRbEmptyFirst, kRbEmptyLast, kRbEmptyMiddle,
    kRbFull, kRbFullLess1, kRbNnMod8Is1, kRbNnMod8Is7, kRbNnIs1,
    kRbRows1, kRbRowsT, kRbRowsT1, kRbRowsCap, kRbRowsMax, kRbEndedByCap, kRbPulledBack,
    kRbFirstRowEmpty, kRbLastRowEmpty, kRbRowLen1, kRbRowLen8, kRbRowLen9,
    kRbLong, kRbLongPlus1, kRbLong2x, kRbLong2xPlus1, kRbLongFirstRow, kRbLongLastRow, kRbLongAfterLong,
    kRbR1, kRbR2, kRbR3, kRbR4, kRbR5, kRbR6, kRbR7, kRbR8,
    kRbU1, kRbUMultT, kRbUMultTPlus1, kRbUIsNn, kRbUMax, kRbSkew,
    kRowblockCensusLen
};

// rows / ptrs: the table (blocks + 1 entries each); why: build_row_blocks' reasons; ucount: distinct columns per block (tile) or null
inline void rowblock_census(int n, const int* ptrow, int nnzb, int threads, int row_align, const std::vector<int>& rows,
                            const std::vector<int>& ptrs, const std::vector<char>& why, const int* ucount, bool skew, long long* c)
{
    std::fill(c, c + kRowblockCensusLen, 0LL);
    const int nblk = (int)rows.size() - 1;
    const int T = threads, cap = 4 * threads;
    c[kRbBlocks] = nblk;
    c[kRbRowAlign] = row_align;
    c[kRbIdleWgs] = 8LL * ((nblk + 7) / 8) - nblk;
    c[kRbSkew] = ucount && skew;
    for (int b = 0; b < nblk; b++) {
        const int r0 = rows[b], r1 = rows[b + 1], nn = ptrs[b + 1] - ptrs[b], nr = r1 - r0;
        c[kRbEndedByCap] += (why[b] & kBlockEndRowCap) != 0;
        c[kRbPulledBack] += (why[b] & kBlockEndPulledBack) != 0;
        if (nn == 0) {
            c[kRbEmpty]++;
            if (b == 0) c[kRbEmptyFirst]++;
            if (b == nblk - 1) c[kRbEmptyLast]++;
            if (b != 0 && b != nblk - 1) c[kRbEmptyMiddle]++;
            continue;
        }
        if (nn > nnzb) { // one row longer than a block
            c[kRbLong]++;
            c[kRbLongPlus1] += nn == nnzb + 1;
            c[kRbLong2x] += nn == 2 * nnzb;
            c[kRbLong2xPlus1] += nn == 2 * nnzb + 1;
            c[kRbLongFirstRow] += r0 == 0;
            c[kRbLongLastRow] += r1 == n;
            c[kRbLongAfterLong] += b > 0 && ptrs[b] - ptrs[b - 1] > nnzb;
            continue;
        }
        c[kRbFull] += nn == nnzb;
        c[kRbFullLess1] += nn == nnzb - 1;
        c[kRbNnMod8Is1] += nn % 8 == 1;
        c[kRbNnMod8Is7] += nn % 8 == 7;
        c[kRbNnIs1] += nn == 1;
        c[kRbRows1] += nr == 1;
        c[kRbRowsT] += nr == T;
        c[kRbRowsT1] += nr == T + 1;
        c[kRbRowsCap] += nr == cap;
        c[kRbRowsMax] = std::max<long long>(c[kRbRowsMax], nr);
        c[kRbFirstRowEmpty] += ptrow[r0 + 1] == ptrow[r0];
        c[kRbLastRowEmpty] += ptrow[r1] == ptrow[r1 - 1];
        for (int r = r0; r < r1; r++) {
            const int len = ptrow[r + 1] - ptrow[r];
            c[kRbRowLen1] += len == 1;
            c[kRbRowLen8] += len == 8;
            c[kRbRowLen9] += len == 9;
        }
        if (ucount) {
            const int U = ucount[b], R = (U + T - 1) / T;
            if (R >= 1 && R <= 8) c[kRbR1 + R - 1]++;
            c[kRbU1] += U == 1;
            c[kRbUMultT] += U % T == 0;
            c[kRbUMultTPlus1] += U > 1 && U % T == 1;
            c[kRbUIsNn] += U == nn;
            c[kRbUMax] = std::max<long long>(c[kRbUMax], U);
        }
    }
}

} // namespace mi355
