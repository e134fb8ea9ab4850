// spmm_tile_plan.hpp — the host-side plan of the multi-vector product's tile forms (spmm_tile.hpp: spmm_bcsr4_tile on tiles of up to
// 128 block rows, spmm_bcsr4_otile on tiles of up to 64).  Host only: no HIP, no device memory — like tile_plan.hpp and mring_plan.hpp.
//
// build_spmm_tile_plan_host is the ONE function that makes these arrays.  The handle (capi_bcsr.hip: build_spmm_tile_plan) uploads what
// it returns, unchanged, and mi_bcsr4_spmm_plan_probe copies the same arrays out to its caller: for a given pattern, `per`, `ucap` and
// row order, the probe's arrays ARE the handle's.  tests/test_spmm_tile_plan.py holds them to their invariants through the probe,
// tools/spmm_plan_asan.cpp runs this header under the host sanitizers.
//
// Tiles of the multi-vector product: groups of at most `per` block rows, the list of distinct block columns each group touches, and
// every block's position in its group's list.  The groups are CLUSTERS of the block graph, not runs of consecutive rows: grown
// breadth-first from the lowest unassigned row over unassigned rows (a "ball" of the mesh), because the tile's cost — its gather, its
// LDS — is the number of distinct columns per row, and a ball of 128 nodes of a 3-D mesh touches ~2.5 per row where 128
// consecutive nodes (1.9 mesh lines) touch 5.1 (FE matrix, 68^3 cells: lists of 321 against 654 entries on average).  A cluster
// whose list would exceed `ucap` entries is cut in halves (in growth order) until it fits: the LDS footprint, hence the
// workgroups per CU, is set by the LONGEST list.  A single row whose list exceeds the cap is a tile of its own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace mi355 {

struct SpmmTilePlanHost {
    int per = 0, umax = 0, ntiles = 0;  // block rows per tile (at most); longest list; tiles
    double mean_list = 0.0;             // list entries per tile
    std::vector<int> wg_ptr;            // [ntiles + 1]: tile t's list is nodes[wg_ptr[t] .. wg_ptr[t + 1])
    std::vector<unsigned> nodes;        // [wg_ptr[ntiles] + 1]: the lists, each strictly ascending; one pad entry (0) behind the last
    std::vector<unsigned short> slots;  // [nblocks + 1]: block k's column is nodes[wg_ptr[tile of k's row] + slots[k]]; one pad entry (0)
    std::vector<int> rows;              // [ntiles * per]: block row of lane group i of tile t, or -1 - (a live row of the tile) for unused
                                        // places (those lanes shadow that row and store nothing)
};

// Returns 1 and fills `out`, or -1 (refused; `out` is left empty): a list of more than 65 535 entries (the slots are 16 bits), or
// nothing to list (no block row, or no block column in any).  sort_rows: a tile's rows ascending (what the handle uploads unless
// MI355_SPMM_TILE_SORT=0), else in the order the cluster grew.
inline int build_spmm_tile_plan_host(int nbr, const int* ptrow, const int* indcol, int per, int ucap, bool sort_rows, SpmmTilePlanHost& out)
{
    out = SpmmTilePlanHost();
    if (nbr < 0 || per < 1) return -1;
    const long long nblocks = nbr > 0 ? ptrow[nbr] : 0;
    std::vector<int> order;           // block rows in cluster growth order
    std::vector<int> cuts;            // first position of every cluster, then cut further below
    order.reserve((size_t)nbr);
    {
        std::vector<char> assigned((size_t)nbr, 0);
        std::vector<int> stamp((size_t)nbr, 0), queue;
        int seed = 0, tid = 0, in_cur = 0;
        while (true) {
            while (seed < nbr && assigned[seed]) seed++;
            if (seed >= nbr) break;
            if (in_cur == 0) {
                tid++;
                cuts.push_back((int)order.size());
            }
            queue.clear();
            queue.push_back(seed);
            stamp[seed] = tid;
            for (size_t qh = 0; qh < queue.size() && in_cur < per; qh++) {
                const int r = queue[qh];
                order.push_back(r);
                assigned[r] = 1;
                in_cur++;
                for (int k = ptrow[r]; k < ptrow[r + 1]; k++) {
                    const int nb = indcol[k];
                    if (nb < nbr && !assigned[nb] && stamp[nb] != tid) { // (columns beyond the rows: a rectangular matrix has no such node)
                        stamp[nb] = tid;
                        queue.push_back(nb);
                    }
                }
            }
            if (in_cur == per) in_cur = 0; // full; else the component ran dry: the next seed continues this cluster
        }
        cuts.push_back((int)order.size());
    }
    // lists; clusters over the cap are halved
    std::vector<int> wg_ptr(1, 0), rows;
    std::vector<unsigned> nodes, u;
    std::vector<unsigned short> slots((size_t)nblocks + 1, 0);
    int umax = 0;
    std::vector<std::pair<int, int>> work; // [first, end) positions in `order`, processed in order (a stack keeps the order)
    for (size_t t = cuts.size() - 1; t-- > 0;) work.push_back({cuts[t], cuts[t + 1]});
    while (!work.empty()) {
        const std::pair<int, int> w = work.back();
        work.pop_back();
        if (w.first >= w.second) continue;
        u.clear();
        for (int i = w.first; i < w.second; i++) u.insert(u.end(), indcol + ptrow[order[i]], indcol + ptrow[order[i] + 1]);
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        if ((int)u.size() > ucap && w.second - w.first > 1) {
            const int mid = (w.first + w.second) / 2;
            work.push_back({mid, w.second});
            work.push_back({w.first, mid});
            continue;
        }
        if (u.size() > 65535) return -1;
        umax = std::max(umax, (int)u.size());
        for (int i = w.first; i < w.second; i++)
            for (int k = ptrow[order[i]]; k < ptrow[order[i] + 1]; k++)
                slots[k] = (unsigned short)(std::lower_bound(u.begin(), u.end(), (unsigned)indcol[k]) - u.begin());
        nodes.insert(nodes.end(), u.begin(), u.end());
        wg_ptr.push_back((int)nodes.size());
        // (round 5) the tile's rows in ASCENDING order, not in the order the cluster grew: neighbouring lane groups then stream
        // neighbouring rows' blocks (one run of the coefficient array per run of consecutive rows) and store neighbouring pieces of Y.
        if (sort_rows) std::sort(order.begin() + w.first, order.begin() + w.second);
        for (int i = 0; i < per; i++) rows.push_back(w.first + i < w.second ? order[w.first + i] : -1 - order[w.first]);
    }
    const int ntiles = (int)wg_ptr.size() - 1;
    if (umax < 1 || ntiles < 1) return -1;
    nodes.push_back(0);
    out.per = per;
    out.umax = umax;
    out.ntiles = ntiles;
    out.mean_list = (double)(nodes.size() - 1) / ntiles;
    out.wg_ptr = std::move(wg_ptr);
    out.nodes = std::move(nodes);
    out.slots = std::move(slots);
    out.rows = std::move(rows);
    return 1;
}

} // namespace mi355
