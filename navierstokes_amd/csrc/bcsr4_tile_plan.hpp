// bcsr4_tile_plan.hpp — host-side (no HIP) lists of the blocked kernel's x tile (spmv_bcsr4_tile, spmv_kernels.hpp): the distinct
// block columns of each group of `per` block rows (one workgroup), ascending, and every block's position in its group's list.
// Built for matrices of at least kBtileMinBlocks blocks, and only when no group needs more nodes than the tile holds (`cap`).
// One builder for the handle (build_bcsr4_tile, capi_bcsr.hip) and the host-only probe (mi_bcsr4_tile_probe).
#pragma once
#include <algorithm>
#include <vector>

namespace mi355 {

constexpr long long kBtileMinBlocks = 4096; // below: the plain kernel (a launch of a few workgroups gains nothing from the tile)

struct Bcsr4TileListsHost {
    bool built = false;                // false: too few blocks, or a group over the cap — the arrays below are then not for use
    int groups = 0;                    // groups of `per` block rows = workgroups of the kernel
    int max_nodes = 0;                 // longest list among the groups looked at (all of them when built)
    int groups_at_cap = 0;             // groups whose list holds exactly `cap` nodes
    std::vector<int> wg_ptr;           // [groups + 1] first list entry of each group
    std::vector<unsigned> nodes;       // the lists, one padding entry behind them
    std::vector<unsigned short> slots; // [blocks + 1] per block: position of its column in its group's list (one padding entry)
};

inline void build_bcsr4_tile_lists(int nbrows, const int* ptrow, const int* indcol, int per, int cap, Bcsr4TileListsHost& out)
{
    out = Bcsr4TileListsHost();
    const long long nb = nbrows > 0 ? ptrow[nbrows] : 0;
    const int nwg = (nbrows + per - 1) / per;
    out.groups = nwg;
    if (nb < kBtileMinBlocks) return; // (nothing listed: max_nodes and groups_at_cap stay 0)
    out.wg_ptr.assign((size_t)nwg + 1, 0);
    out.slots.assign((size_t)nb + 1, 0);
    std::vector<unsigned> u;
    bool fits = true;
    for (int w = 0; w < nwg && fits; w++) {
        const int b0 = ptrow[(size_t)w * per], b1 = ptrow[std::min<long long>((long long)(w + 1) * per, nbrows)];
        u.assign(indcol + b0, indcol + b1);
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        fits = (int)u.size() <= cap;
        out.max_nodes = std::max(out.max_nodes, (int)u.size());
        out.groups_at_cap += (int)u.size() == cap;
        for (int k = b0; k < b1 && fits; k++) out.slots[k] = (unsigned short)(std::lower_bound(u.begin(), u.end(), (unsigned)indcol[k]) - u.begin());
        out.nodes.insert(out.nodes.end(), u.begin(), u.end());
        out.wg_ptr[w + 1] = (int)out.nodes.size();
    }
    out.nodes.push_back(0);
    out.built = fits;
}

} // namespace mi355
