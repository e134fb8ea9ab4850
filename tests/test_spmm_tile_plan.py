"""The tile plan of the multi-vector product's forms 1-3 (navierstokes_amd/csrc/spmm_tile_plan.hpp) without a GPU.

mi_bcsr4_spmm_plan_probe returns the arrays the handle uploads (one function builds both).  For every pattern of tests/spmm_tile_cases.py,
for per = 128 and per = 64, under the default caps and the small ones, the arrays are held to the invariants the kernels of
spmm_tile.hpp rely on, and the plan is REPLAYED: Y computed from wg_ptr / nodes / slots / rows alone, on integer-valued doubles (every
sum exact, so the order of a row's blocks cannot matter), must equal the oracle's product column by column."""
import numpy as np
import pytest

import spmm_tile_cases as TC
from navierstokes_amd import mpk
from oracle import oracle as O

PERS = (128, 64)
RUNS = [(name, caps) for caps in (None,) + TC.SMALL_CAPS for name in TC.NAMES]


def probe(C, per, ucap_env=None):
    cap = TC.caps_of(ucap_env)[0 if per == 128 else 1]
    return mpk.bcsr4_spmm_plan_probe(C.nbrows, C.bp, C.bc, per, cap), cap


def check_invariants(C, P, per, cap):
    what = f"{C.name} per {per} cap {cap}"
    wg, nodes, slots, rows = P["wg_ptr"], P["nodes"], P["slots"], P["rows"]
    nt = P["ntiles"]
    assert nt == len(wg) - 1 == rows.shape[0] and rows.shape[1] == per and wg[0] == 0 and (np.diff(wg) >= 0).all(), what
    assert slots.dtype == np.uint16 and len(slots) == C.nblocks and len(nodes) == wg[-1], what
    live = rows[rows >= 0]
    assert np.array_equal(np.sort(live), np.arange(C.nbrows)), f"{what}: every block row exactly once"
    lists = np.diff(wg)
    assert P["umax"] == lists.max(), what
    assert abs(P["mean_list"] - wg[-1] / nt) <= 1e-12 * max(1.0, wg[-1] / nt), what
    tile_of = np.full(C.nbrows, -1)
    for t in range(nt):
        r = rows[t]
        lv = r[r >= 0]
        assert 1 <= len(lv) <= per, f"{what}: tile {t} holds {len(lv)} live rows"
        assert (np.diff(lv) > 0).all(), f"{what}: tile {t}: live rows not ascending"
        assert (r[:len(lv)] >= 0).all(), f"{what}: tile {t}: a shadow in front of a live row"
        sh = -1 - r[r < 0]
        assert np.isin(sh, lv).all(), f"{what}: tile {t}: a shadow names a row of another tile"
        tile_of[lv] = t
        lst = nodes[wg[t]:wg[t + 1]].astype(np.int64)
        assert (np.diff(lst) > 0).all(), f"{what}: tile {t}: list not strictly ascending"
        cols = np.unique(np.concatenate([C.row_cols(i) for i in lv])) if len(lv) else np.zeros(0, np.int64)
        assert np.array_equal(lst, cols), f"{what}: tile {t}: the list is not the set of its rows' block columns"
        if len(lst) > cap:
            assert len(lv) == 1, f"{what}: tile {t}: list of {len(lst)} > cap with {len(lv)} rows"
    row_of_block = np.repeat(np.arange(C.nbrows), np.diff(C.bp))
    base = wg[tile_of[row_of_block]]
    assert (slots < lists[tile_of[row_of_block]]).all(), f"{what}: a slot beyond its tile's list"
    assert np.array_equal(nodes[base + slots], C.bc.astype(np.uint32)), f"{what}: a slot names another column"
    return tile_of


def replay(C, P, X):
    """Y from the plan alone, as the kernels walk it: per tile, gather the list's nodes of X; per live row, its blocks in stored order, x from
    the gathered records by slot."""
    wg, nodes, slots, rows = P["wg_ptr"], P["nodes"], P["slots"], P["rows"]
    s = X.shape[0]
    Y = np.full((s, 4 * C.nbrows), np.nan)
    B = C.bv_int.reshape(-1, 4, 4)
    for t in range(P["ntiles"]):
        lst = nodes[wg[t]:wg[t + 1]].astype(np.int64)
        G = X[:, (4 * lst[:, None] + np.arange(4)[None, :])] if len(lst) else np.zeros((s, 0, 4))   # (s, U, 4)
        for r in rows[t][rows[t] >= 0]:
            k0, k1 = C.bp[r], C.bp[r + 1]
            acc = np.zeros((s, 4))
            if k1 > k0:
                acc = np.einsum("kqc,skc->sq", B[k0:k1], G[:, slots[k0:k1].astype(np.int64), :])
            assert np.isnan(Y[:, 4 * r:4 * r + 4]).all(), f"row {r} stored twice"
            Y[:, 4 * r:4 * r + 4] = acc
    return Y


@pytest.mark.parametrize("name,ucap", RUNS, ids=[f"{n}{'' if u is None else '-ucap' + u}" for n, u in RUNS])
def test_plan_invariants_and_replay(name, ucap):
    C = TC.case(name)
    rng = np.random.default_rng(C.seed)
    if not hasattr(C, "bv_int"):
        C.bv_int = rng.integers(-8, 9, 16 * C.nblocks).astype(np.float64)
        C.X_int = rng.integers(-8, 9, (2, 4 * C.nbcols)).astype(np.float64)
        C.Y_int = np.stack([O.spmv_bcsr4(C.bp, C.bc, C.bv_int, x) for x in C.X_int])
    for per in PERS:
        P, cap = probe(C, per, ucap)
        assert not P["refused"], (name, per)
        check_invariants(C, P, per, cap)
        Y = replay(C, P, C.X_int)
        assert np.array_equal(Y, C.Y_int), f"{name} per {per} cap {cap}: the replayed plan computes another product"


def test_each_pattern_reaches_what_it_is_for():
    """What a pattern's name promises, read off the probe's arrays."""
    def tiles(name, per, ucap=None):
        P, _ = probe(TC.case(name), per, ucap)
        return P, (P["rows"] >= 0).sum(axis=1), np.diff(P["wg_ptr"])
    # rows:N — the last tile of the band: one shadow, none, or one live row and per - 1 shadows
    for per, counts in ((128, (127, 128, 129)), (64, (63, 64, 65))):
        for n, last in zip(counts, (per - 1, per, 1)):
            for kind in ("rows", "rowsdiag"):
                P, live, _ = tiles(f"{kind}:{n}", per)
                assert live.sum() == n and (kind == "rowsdiag" or (live[-1] == last and P["ntiles"] == -(-n // per))), (kind, n, per, live)
    # components: a cluster continues across a component that ran dry (no tile under `per` rows but the last), and full clusters do not
    # (1 + 2 + 63 + 64 = 130: the first tile ends inside the fourth piece)
    for name in ("components:fwd", "components:rev"):
        for per in PERS:
            P, live, _ = tiles(name, per)
            assert (live[:-1] == per).all() and P["ntiles"] == -(-sum(TC.COMPONENT_SIZES) // per), (name, per, live)
    # empty: a tile whose list is empty, in both plans; the trailing rows' ptrow equals nblocks
    C = TC.case("empty")
    assert C.bp[1] == 0 and (C.bp[-4:] == C.nblocks).all()
    for per in PERS:
        P, live, lists = tiles("empty", per)
        assert ((lists == 0) & (live == per)).sum() == 128 // per, (per, lists)
    # long:L — umax == L in both plans, the long row alone in its tile; the band's tiles stay under the caps
    for L in TC.LONG:
        for per in PERS:
            P, live, lists = tiles(f"long:{L}", per)
            t = int(np.argmax(lists))
            assert P["umax"] == L and live[t] == 1 and P["rows"][t, 0] == 450 and (np.sort(lists)[:-1] <= TC.DEFAULT_CAPS[per == 64]).all(), (L, per)
    # the boundaries the list is named for: L fits at s columns, L + 1 does not
    for s, L in ((8, 602), (6, 787), (4, 1137), (3, 1462), (2, 2048), (1, 3413)):
        assert TC.lds_bytes(L, s) <= TC.LDS_BYTES < TC.lds_bytes(L + 1, s) and L in TC.LONG and L + 1 in TC.LONG
    assert [TC.lds_bytes(L, s) for s, L in ((4, 1137), (3, 1462), (8, 602), (6, 787))] == [163728, 163744, 163744, 163696]
    # small caps: "40,24" halves, "12,12" halves again and again, "1,1" leaves single rows, each above its cap and accepted
    G = TC.case("grid")
    for per in PERS:
        n0 = tiles("grid", per)[0]["ntiles"]
        n1, live1, _ = tiles("grid", per, "40,24")
        n2, live2, _ = tiles("grid", per, "12,12")
        n3, live3, lists3 = tiles("grid", per, "1,1")
        assert n0 < n1["ntiles"] < n2["ntiles"] < n3["ntiles"] == G.nbrows and (live3 == 1).all() and (lists3 > 1).all()
        assert (live2 % 2 == 1).any() and live2.max() < per // 4
    # rect_wide: the extra columns are no seeds and are listed; repeated: blocks of one row share a slot
    W = TC.case("rect_wide")
    P, _ = probe(W, 128)
    assert (P["nodes"] >= W.nbrows).sum() >= 500
    R = TC.case("repeated")
    P, _ = probe(R, 128)
    sl = P["slots"][R.bp[10]:R.bp[11]]
    assert sl[1] == sl[2] == sl[6] and sl[0] == sl[4] and len(set(sl.tolist())) == 4


def test_clusters_beat_consecutive_rows_on_the_grid():
    """The documented reason for clustering: a breadth-first ball touches fewer distinct columns than as many consecutive rows."""
    C = TC.case("grid")
    for per in PERS:
        P, _ = probe(C, per)
        consecutive = [len(np.unique(C.bc[C.bp[r0]:C.bp[min(r0 + per, C.nbrows)]])) for r0 in range(0, C.nbrows, per)]
        assert P["mean_list"] < np.mean(consecutive), (per, P["mean_list"], np.mean(consecutive))


def test_refusals():
    """65 536 distinct columns in one row cannot be named by 16-bit slots: refused; 65 535 can.  Nothing to list: refused, no crash."""
    for L, refused in ((65536, True), (65535, False)):
        bp = np.array([0, 1, 1 + L, 2 + L], np.int32)
        bc = np.concatenate([[0], np.arange(L), [2]]).astype(np.int32)
        P = mpk.bcsr4_spmm_plan_probe(3, bp, bc, 128)
        assert P["refused"] == refused, L
        if refused:
            assert (P["ntiles"], P["umax"]) == (0, 0)
        else:
            assert P["umax"] == L and P["ntiles"] == 3 and P["slots"][L] == L - 1
    assert mpk.bcsr4_spmm_plan_probe(300, np.zeros(301, np.int32), np.zeros(0, np.int32), 128)["refused"]
    assert mpk.bcsr4_spmm_plan_probe(300, np.zeros(301, np.int32), np.zeros(0, np.int32), 64)["refused"]
    assert mpk.bcsr4_spmm_plan_probe(0, np.zeros(1, np.int32), np.zeros(0, np.int32), 128)["refused"]


def test_probe_checks_its_buffers_and_arguments():
    import ctypes
    C = TC.case("grid")
    L = mpk.lib()
    ref, nt, um = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    small = np.zeros(4, np.int32)
    args = (C.nbrows, C.bp.ctypes.data, C.bc.ctypes.data)
    out = (ctypes.byref(ref), ctypes.byref(nt), ctypes.byref(um), None)
    assert L.mi_bcsr4_spmm_plan_probe(*args, 128, 368, *out, None, 0, None, 0, None, 0, None, 0) == 0 and nt.value > 0 and not ref.value
    for which in range(4):
        bufs = [None, 0] * 4
        bufs[2 * which], bufs[2 * which + 1] = small.ctypes.data, 4
        assert L.mi_bcsr4_spmm_plan_probe(*args, 128, 368, *out, *bufs) == 1, which
        assert b"too small" in L.mi_last_error()
    assert L.mi_bcsr4_spmm_plan_probe(*args, 96, 368, *out, None, 0, None, 0, None, 0, None, 0) == 1
    assert L.mi_bcsr4_spmm_plan_probe(*args, 64, 0, *out, None, 0, None, 0, None, 0, None, 0) == 1
