// bilu4_order.hpp — the opt-in ordering of the block rows behind a block ILU handle (mi_bilu4_create_ordered, include/mi355_spmv.h).
// Plain C++ (no HIP), like bilu4_plan.hpp, so that it can be probed and tested without a GPU.
//
// A handle created with MI_BILU_ORDER_COLOUR factors B = Q A Q^T instead of A, Q a multicolour renumbering of the block rows: the
// rows of one colour have no block between them, so at fill 0 an exact solve has at most as many dependency levels per sweep as
// there are colours, each a wide, contiguous, independent range of rows.  ILU of B is NOT ILU of A: a different, usually weaker
// preconditioner.
//
// THE COLOURING RULE (part of the interface, restated in plain Python by tests/test_bilu4_order.py): greedy colouring of the
// symmetrised block graph — the pattern of A + A^T without the diagonal — block rows taken in ascending natural order, each taking
// the smallest colour that no already-coloured neighbour holds.  New numbering: colour ascending, inside a colour the old row
// number ascending.  perm[old] = new, the convention of mi_csr_perm.
//
// Everything behind the ordering (symbolic ILU, levels, folding, both factorisations, the one-launch plan, the sweeps, the f32
// copy) runs unchanged on B's pattern; what reads the CALLER's values goes through src: src[k] = the caller's index of B's k-th block.
#pragma once
#include <string>
#include <vector>

namespace mi355 {

struct Bilu4Order {
    int ordering = 0;          // MI_BILU_ORDER_*
    int ncolours = 0;          // 0 in natural order
    std::vector<int> perm;     // [nb] old block row -> new; empty in natural order
    std::vector<int> iperm;    // [nb] new -> old
    std::vector<int> colour_ptr; // [ncolours + 1] first new block row of each colour
    std::vector<int> src;      // [nblocks of B] B's k-th block is the caller's block src[k]; empty in natural order
    bool on() const { return ordering != 0; }
    const int* src_or_null() const { return src.empty() ? nullptr : src.data(); }
    // the caller's number of block row i of the factor (what messages and statuses name)
    int caller_row(int i) const { return on() && i >= 0 && i < (int)iperm.size() ? iperm[i] : i; }
};

// the greedy colouring and the numbering it gives; pattern as bilu4_check_pattern accepts it
inline void bilu4_colour(int nb, const int* ptrow, const int* indcol, Bilu4Order* O)
{
    // the symmetrised graph, diagonal excluded, as CSR (neighbours may repeat: harmless to the rule)
    std::vector<int> np((size_t)nb + 1, 0), nbr;
    for (int i = 0; i < nb; i++)
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++)
            if (indcol[k] != i) np[i + 1]++, np[indcol[k] + 1]++;
    for (int i = 0; i < nb; i++) np[i + 1] += np[i];
    nbr.resize((size_t)np[nb]);
    std::vector<int> at(np.begin(), np.end() - 1);
    for (int i = 0; i < nb; i++)
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++)
            if (indcol[k] != i) nbr[at[i]++] = indcol[k], nbr[at[indcol[k]]++] = i;
    std::vector<int> colour((size_t)nb, -1), held; // held[c] == i: colour c is taken by a neighbour of row i
    int nc = 0;
    for (int i = 0; i < nb; i++) {
        for (int k = np[i]; k < np[i + 1]; k++)
            if (colour[nbr[k]] >= 0) held[colour[nbr[k]]] = i;
        int c = 0;
        while (c < nc && held[c] == i) c++;
        if (c == nc) nc++, held.push_back(-1);
        colour[i] = c;
    }
    O->ordering = 1;
    O->ncolours = nc;
    O->colour_ptr.assign((size_t)nc + 1, 0);
    for (int i = 0; i < nb; i++) O->colour_ptr[colour[i] + 1]++;
    for (int c = 0; c < nc; c++) O->colour_ptr[c + 1] += O->colour_ptr[c];
    std::vector<int> next(O->colour_ptr.begin(), O->colour_ptr.end() - 1);
    O->perm.assign((size_t)nb, 0);
    O->iperm.assign((size_t)nb, 0);
    for (int i = 0; i < nb; i++) { // ascending old number inside a colour
        O->perm[i] = next[colour[i]]++;
        O->iperm[O->perm[i]] = i;
    }
}

// B = Q A Q^T: row perm[i] of B is row i of A with its block columns renamed and re-sorted ascending; src as above
inline void bilu4_permute_pattern(int nb, const int* ptrow, const int* indcol, Bilu4Order* O, std::vector<int>* bptr, std::vector<int>* bcol)
{
    bptr->assign((size_t)nb + 1, 0);
    for (int n = 0; n < nb; n++) (*bptr)[n + 1] = (*bptr)[n] + ptrow[O->iperm[n] + 1] - ptrow[O->iperm[n]];
    bcol->assign((size_t)(*bptr)[nb], 0);
    O->src.assign((size_t)(*bptr)[nb], 0);
    // a counting sort by new column over all blocks keeps every row ascending: deal the blocks of new column 0, 1, ... to their rows
    std::vector<int> fill_at(bptr->begin(), bptr->end() - 1);
    std::vector<int> cnt((size_t)nb + 1, 0), byc((size_t)(*bptr)[nb]), rowof((size_t)(*bptr)[nb]);
    for (int i = 0; i < nb; i++)
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++) cnt[O->perm[indcol[k]] + 1]++;
    for (int c = 0; c < nb; c++) cnt[c + 1] += cnt[c];
    for (int i = 0; i < nb; i++)
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++) {
            const int at = cnt[O->perm[indcol[k]]]++;
            byc[at] = k, rowof[at] = O->perm[i];
        }
    for (size_t a = 0; a < byc.size(); a++) {
        const int k = byc[a], to = fill_at[rowof[a]]++;
        (*bcol)[to] = O->perm[indcol[k]];
        O->src[to] = k;
    }
}

// What the ordering promises, checked against the caller's pattern: perm is a permutation, and every colour is an independent
// set of the symmetrised graph.  Empty string, or the first violation.
inline std::string bilu4_order_check(int nb, const int* ptrow, const int* indcol, const Bilu4Order& O)
{
    if ((int)O.perm.size() != nb || (int)O.iperm.size() != nb || (int)O.colour_ptr.size() != O.ncolours + 1) return "table sizes disagree";
    std::vector<char> seen((size_t)nb, 0);
    for (int i = 0; i < nb; i++) {
        const int n = O.perm[i];
        if (n < 0 || n >= nb) return "perm[" + std::to_string(i) + "] is out of range";
        if (seen[n]) return "perm names block row " + std::to_string(n) + " twice (at " + std::to_string(i) + ")";
        seen[n] = 1;
        if (O.iperm[n] != i) return "iperm is not the inverse of perm at block row " + std::to_string(i);
    }
    if (O.colour_ptr[0] != 0 || O.colour_ptr[O.ncolours] != nb) return "the colours do not cover the block rows";
    std::vector<int> colour((size_t)nb, 0);
    for (int c = 0; c < O.ncolours; c++) {
        if (O.colour_ptr[c + 1] <= O.colour_ptr[c]) return "colour " + std::to_string(c) + " is empty";
        for (int n = O.colour_ptr[c]; n < O.colour_ptr[c + 1]; n++) colour[O.iperm[n]] = c;
    }
    for (int i = 0; i < nb; i++)
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++)
            if (indcol[k] != i && colour[indcol[k]] == colour[i])
                return "colour " + std::to_string(colour[i]) + " is not independent: it holds block rows " + std::to_string(i) + " and " + std::to_string(indcol[k]) +
                       ", which share a block";
    return std::string();
}

} // namespace mi355
