"""Model of the one-launch solve's plan (mi_bilu4one_*), restated in plain numpy from the description in include/mi355_spmv.h:
chunks, dependency lists and the replay of the dealing.  Pattern and level schedule come from tests/bilu4_model.py.

Chunks, per sweep: the schedule's launches in order; a launch that is one level of at least 64 block rows is cut into chunks of 64
consecutive positions (the last may be shorter), every other launch (a folded run of narrow levels) is one chunk.  A chunk's
dependencies: the distinct chunks of the same sweep that hold a block row named by an off-diagonal block column of one of its rows,
itself excepted, ascending.  Dealing: chunk c belongs to workgroup c mod G, every workgroup takes its chunks in ascending order."""
import numpy as np

import bilu4_model as M

CHUNK = M.ROWS_PER_WG
MAX_DEPS = 256


def chunks(S):
    """(chunk_pos, chunk_lev), nchunks + 1 entries each, of a schedule S of bilu4_model.schedule."""
    pos, lev = [], []
    lp, sizes = S["lev_ptr"], S["sizes"]
    for a in range(S["launches"]):
        l0, l1 = S["launch_ptr"][a], S["launch_ptr"][a + 1]
        p0, p1 = int(lp[l0]), int(lp[l1])
        if l1 - l0 == 1 and sizes[l0] >= CHUNK:
            for p in range(p0, p1, CHUNK):
                pos.append(p)
                lev.append(l0)
        else:
            pos.append(p0)
            lev.append(l0)
    pos.append(int(lp[-1]) if len(lp) else 0)
    lev.append(S["nlev"])
    return np.array(pos, np.int32), np.array(lev, np.int32)


def dependencies(nb, ptr, col, diag, S, chunk_pos, backward):
    """(dep_ptr, dep) of one sweep."""
    nch = len(chunk_pos) - 1
    chunk_of_pos = np.repeat(np.arange(nch), np.diff(chunk_pos))
    chunk_of_row = np.zeros(nb, np.int64)
    chunk_of_row[S["perm"]] = chunk_of_pos
    k0 = (diag + 1) if backward else ptr[:-1]
    k1 = ptr[1:] if backward else diag
    dep_ptr, dep = [0], []
    for c in range(nch):
        rows = S["perm"][chunk_pos[c]:chunk_pos[c + 1]]
        named = np.concatenate([col[k0[i]:k1[i]] for i in rows]) if len(rows) else np.zeros(0, np.int64)
        d = np.unique(chunk_of_row[named]) if len(named) else np.zeros(0, np.int64)
        d = d[d != c]
        dep.extend(int(x) for x in d)
        dep_ptr.append(len(dep))
    return np.array(dep_ptr, np.int32), np.array(dep, np.int32)


def replay(dep_ptr, dep, G):
    """G workgroups step through their chunks (c mod G) in order; a chunk starts only when all its dependencies are finished.
    Returns the order in which the chunks finished; raises when nobody can move while chunks are left."""
    nch = len(dep_ptr) - 1
    done = np.zeros(nch, bool)
    nxt = list(range(G))
    order = []
    while len(order) < nch:
        moved = False
        for g in range(G):
            while nxt[g] < nch and done[dep[dep_ptr[nxt[g]]:dep_ptr[nxt[g] + 1]]].all():
                done[nxt[g]] = True
                order.append(nxt[g])
                nxt[g] += G
                moved = True
        if not moved:
            raise AssertionError(f"the dealing stalls for {G} workgroups after {len(order)} of {nch} chunks")
    return order


def plan(nb, ptrow, indcol, fill):
    """dict(chunk_pos, chunk_lev, dep_ptr, dep, nchunks, max_deps: (forward, backward) pairs; eligible) of a matrix's pattern."""
    ptr, col, diag = M.symbolic(nb, ptrow, indcol, fill)
    out = dict(chunk_pos=[], chunk_lev=[], dep_ptr=[], dep=[], nchunks=[], max_deps=[])
    for backward in (False, True):
        S = M.schedule(nb, ptr, col, diag, backward)
        cp, cl = chunks(S)
        dp, d = dependencies(nb, ptr, col, diag, S, cp, backward)
        out["chunk_pos"].append(cp), out["chunk_lev"].append(cl), out["dep_ptr"].append(dp), out["dep"].append(d)
        out["nchunks"].append(len(cp) - 1)
        out["max_deps"].append(int(np.diff(dp).max()) if len(dp) > 1 else 0)
    out["eligible"] = max(out["max_deps"]) <= MAX_DEPS
    return out
