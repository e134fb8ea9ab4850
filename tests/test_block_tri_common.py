"""What the block ILU and block DILU handles have in common (capi_bilu_common.hpp), through the three host create entry points
mi_bilu4_create_host, mi_bilu4_create_host_ordered and mi_dilu4_create_host.  No GPU: host-only handles.

  refusals   one table of bad inputs, in the order the create functions check them, gives every entry point the same status and
             the message recorded here IN FULL (tests/test_bilu4_abi.py, tests/test_bilu4_order.py and tests/test_dilu4.py look
             for a word of some of these lines; none of them pins a whole text, so none is repeated here).  Every fault is
             presented alone and together with all the faults behind it: the first one is what is reported.
  pivot      a zero pivot is reported by the caller's block row, under both orderings, on a 3-block-row chain and on fe_matrix(3)
  schedule   on one pattern both families report the same ordering (perm, ncolours), the same fill-0 levels and the same launch
             count, which is the plan's plus the two boundary launches exactly when the handle is ordered: fe_matrix(3), a
             layered pattern with levels of 1, 63, 64, 65 and 129 block rows (either side of the folding rule), the empty matrix"""
import ctypes

import numpy as np
import pytest

import bilu4_cases as C

MI_OK, MI_ERR_ARG = 0, 1
ORDERS = ("natural", "colour")
WIDTHS = (1, 63, 64, 65, 129)


class _Entry:
    """One host create entry point: its symbol, the family prefix of its messages, the orderings it can be asked for."""

    def __init__(self, symbol, prefix, orderings, call):
        self.symbol, self.prefix, self.orderings, self._call = symbol, prefix, orderings, call

    def create(self, a):
        """(status, message, handle) of the call with the arguments a (a dict; arrays or None)."""
        from navierstokes_amd import mpk
        L = mpk.lib()
        h = ctypes.c_void_p()
        ptr = lambda v: None if v is None else v.ctypes.data  # noqa: E731
        status = self._call(getattr(L, self.symbol), a["nbrows"], ptr(a["ptrow"]), ptr(a["indcol"]), ptr(a["coef"]), a["layout"], a["ordering"],
                            ctypes.byref(h) if a["out"] else None)
        return status, L.mi_last_error().decode() if status else "", h

    def destroy(self, h):
        from navierstokes_amd import mpk
        getattr(mpk.lib(), self.symbol.split("_create")[0] + "_destroy")(h)


ENTRIES = [
    _Entry("mi_bilu4_create_host", "mi_bilu4: ", (0,), lambda f, n, p, c, v, lay, o, out: f(n, p, c, v, lay, 0, out)),
    _Entry("mi_bilu4_create_host_ordered", "mi_bilu4: ", (0, 1), lambda f, n, p, c, v, lay, o, out: f(n, p, c, v, lay, 0, o, out)),
    _Entry("mi_dilu4_create_host", "mi_dilu4: ", (0, 1), lambda f, n, p, c, v, lay, o, out: f(n, p, c, v, lay, o, out)),
]
ZERO_PIVOT = {"mi_bilu4: ": "mi_bilu4: zero pivot (|d| < 1e-12) in the diagonal block of block row {}",
              "mi_dilu4: ": "mi_dilu4: zero pivot (|d| < 1e-12) in the pivot block E of block row {}"}


def _chain3():
    nb, bp, bc, bv = C.chain(3)
    return nb, np.ascontiguousarray(bp, np.int32), np.ascontiguousarray(bc, np.int32), np.ascontiguousarray(bv, np.float64)


def _good(ordering):
    nb, bp, bc, bv = _chain3()
    return dict(out=True, layout=0, ordering=ordering, nbrows=nb, ptrow=bp, indcol=bc, coef=bv)


def _no_diagonal(a):
    """The chain with block row 1 naming columns (0, 2): its diagonal block is missing, everything else is in order."""
    a["ptrow"], a["indcol"] = np.array([0, 2, 4, 6], np.int32), np.array([0, 1, 0, 2, 1, 2], np.int32)


# in the order of the create functions' checks: (what, the fault put into the arguments, message; {} is the family prefix)
FAULTS = [
    ("null output handle", lambda a: a.update(out=False), "null output handle"),
    ("unknown layout", lambda a: a.update(layout=2), "unknown block layout"),
    ("unknown ordering", lambda a: a.update(ordering=7), "unknown ordering (0: natural, 1: multicolour)"),
    ("negative nbrows", lambda a: a.update(nbrows=-1), "negative nbrows"),
    ("null ptrow", lambda a: a.update(ptrow=None), "null ptrow"),
    ("null indcol", lambda a: a.update(indcol=None), "null indcol"),
    ("refused pattern", _no_diagonal, "{}missing diagonal block in block row 1"),
    ("null coef", lambda a: a.update(coef=None), "null coef"),
]
# later faults that cannot be presented together with an earlier one: the refused pattern brings its own two arrays
EXCLUDES = {"null ptrow": ("refused pattern",), "null indcol": ("refused pattern",)}


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.symbol)
@pytest.mark.parametrize("first", range(len(FAULTS)), ids=lambda k: FAULTS[k][0].replace(" ", "_"))
def test_a_bad_input_is_refused_with_its_status_and_text(entry, first):
    what, fault, text = FAULTS[first]
    if what == "unknown ordering" and len(entry.orderings) == 1:
        assert entry.symbol == "mi_bilu4_create_host"  # (no ordering argument: nothing to refuse)
        return
    for together in (False, True):  # alone, then with every fault behind it that can be presented with it
        a = _good(entry.orderings[-1])
        fault(a)
        for later, later_fault, _ in FAULTS[first + 1:] if together else ():
            if later not in EXCLUDES.get(what, ()):
                later_fault(a)
        status, msg, h = entry.create(a)
        assert (status, msg) == (MI_ERR_ARG, text.format(entry.prefix)), (entry.symbol, what, together, status, msg)
        assert not h.value


def _zeroed_row(nb, bp, bc, bv, row):
    """The values with every block of block row `row` zeroed: under any ordering nothing is subtracted from its (zero) diagonal
    block, and only rows of later levels read it, so that row is the lowest one refused."""
    v = np.array(bv, np.float64).reshape(-1, 4, 4)
    v[bp[row]:bp[row + 1]] = 0.0
    return v.reshape(-1)


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.symbol)
@pytest.mark.parametrize("name", ["chain:3", "fe:3"])
def test_a_zero_pivot_names_the_callers_block_row_under_both_orderings(entry, name):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = _chain3() if name == "chain:3" else C.matrix(name)
    bp, bc, bv = np.ascontiguousarray(bp, np.int32), np.ascontiguousarray(bc, np.int32), np.ascontiguousarray(bv, np.float64)
    perm = mpk.bilu4_order_probe(nb, bp, bc, "colour")["perm"]
    row = nb - 1
    assert perm[row] != row  # the caller's number is not the factor's
    for ordering in entry.orderings:
        a = dict(out=True, layout=0, ordering=ordering, nbrows=nb, ptrow=bp, indcol=bc, coef=_zeroed_row(nb, bp, bc, bv, row))
        status, msg, h = entry.create(a)
        assert (status, msg) == (MI_ERR_ARG, ZERO_PIVOT[entry.prefix].format(row)), (entry.symbol, ordering, status, msg)
        assert not h.value
        a["coef"] = bv
        status, msg, h = entry.create(a)
        assert status == MI_OK and h.value, (entry.symbol, ordering, msg)
        entry.destroy(h)


# ---------------------------------------------------------------- one ordering, one schedule

def _pattern(name):
    if name == "empty":
        return 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)
    if name == "layered":
        return C.layered(WIDTHS, 0, 36)
    return C.matrix(name)


def _permuted(nb, bp, bc, perm):
    """The pattern of the matrix renumbered by perm[old] = new."""
    rows = [None] * nb
    for i in range(nb):
        rows[perm[i]] = sorted(int(perm[j]) for j in bc[bp[i]:bp[i + 1]])
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return ptr, np.array([c for r in rows for c in r], np.int32)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["fe:3", "layered", "empty"])
def test_both_families_report_one_ordering_and_one_schedule(name, order):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = _pattern(name)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0, host_only=True, order=order)
    E = mpk.dilu4(nb, bp, bc, bv, host_only=True, order=order)
    fi, fo, ei = F.info(), F.order_info(), E.info()
    F.close()
    E.close()
    assert fo["order"] == ei["order"] == order
    assert np.array_equal(fo["perm"], ei["perm"]) and fo["ncolours"] == ei["ncolours"], name
    assert (fi["fwd_levels"], fi["bwd_levels"]) == (ei["fwd_levels"], ei["bwd_levels"]), (fi, ei)
    assert fi["form"] == 0 and fi["launches"] == ei["launches"], (fi, ei)
    boundary = 2 if order == "colour" else 0
    if nb == 0:
        assert fi["launches"] == boundary and fi["fwd_levels"] == 0 and fo["ncolours"] == 0
        return
    assert (order == "colour") == (not np.array_equal(fo["perm"], np.arange(nb))) and (order == "colour") == (fo["ncolours"] > 0)
    plan = mpk.bilu4_plan_probe(nb, *_permuted(nb, bp, bc, fo["perm"]), 0)
    assert (plan["fwd_levels"], plan["bwd_levels"]) == (fi["fwd_levels"], fi["bwd_levels"])
    assert fi["launches"] == plan["fwd_launches"] + plan["bwd_launches"] + boundary
    if name == "layered" and order == "natural":  # the levels the pattern was made for: 1 and 63 fold, 64, 65 and 129 do not
        assert list(plan["fwd_sizes"]) == list(WIDTHS) and list(plan["bwd_sizes"]) == list(WIDTHS[::-1])
        assert plan["fwd_launches"] == 4 and plan["bwd_launches"] == 4
