"""Shared by tests/test_gpu_link_slice.py: where the links of pepsgpu_link_exchange_slice sit, the candidate table of its sqrt5 kinds in
numpy, and the per-call reference sequences of both orientations (ReplaceNNNSiteTrace / ReplaceSqrt5DistTwoSiteTrace per link between
the BTen2 window shifts of the triangular J1-J2 model's row-pair and column-pair loops)."""
import numpy as np

from nnn_slice_ref import rect_state, walkers  # noqa: F401  (the state and the walkers of the diagonal-slice test)

HOR, VER = 0, 1
# kind -> (row, col) offsets of the left end (ten_left of the per-call trace) and of the right end from the window's upper-left site
ENDS = {
    HOR: {0: ((0, 0), (1, 1)), 1: ((1, 0), (0, 1)), 2: ((0, 0), (1, 2)), 3: ((1, 0), (0, 2))},
    VER: {2: ((0, 0), (2, 1)), 3: ((2, 0), (0, 1))},
}


def link_ends(cfgs, orient, slice1, j, kind):
    """states [n] of the left and of the right end of link `kind` of the window at position j of the pair, or None where the lattice
    has no such link"""
    r, c = (slice1, j) if orient == HOR else (j, slice1)
    if kind not in ENDS[orient]:
        return None
    (r1, c1), (r2, c2) = ENDS[orient][kind]
    rows, cols = cfgs.shape[1:]
    if r + max(r1, r2) >= rows or c + max(c1, c2) >= cols:
        return None
    return cfgs[:, r + r1, c + c1], cfgs[:, r + r2, c + c2]


def differ_table(cfgs, orient, slice1):
    """[n][N - 1][4] bool: the link exists and its two end states differ"""
    n, rows, cols = cfgs.shape
    N = cols if orient == HOR else rows
    out = np.zeros((n, N - 1, 4), dtype=bool)
    for j in range(N - 1):
        for kind in range(4):
            ends = link_ends(cfgs, orient, slice1, j, kind)
            if ends is not None:
                out[:, j, kind] = ends[0] != ends[1]
    return out


def exists_table(cfgs, orient, slice1):
    """[N - 1][4] bool: the lattice has link `kind` at position j"""
    n, rows, cols = cfgs.shape
    N = cols if orient == HOR else rows
    return np.array([[link_ends(cfgs, orient, slice1, j, kind) is not None for kind in range(4)] for j in range(N - 1)])


def sqrt5_candidates(cfgs, orient, row1, col1):
    """(cand [n][2][4], flag [n][2]) of the 2 x 3 (HOR) / 3 x 2 (VER) window at (row1, col1): the corner states (upper-left, lower-left,
    lower-right, upper-right) with the ends of kind 2 (upper-left <-> lower-right) and of kind 3 (lower-left <-> upper-right) exchanged;
    flag -1 where the end states differ, else 1"""
    dr, dc = (1, 2) if orient == HOR else (2, 1)
    c0, c1 = cfgs[:, row1, col1], cfgs[:, row1 + dr, col1]
    c2, c3 = cfgs[:, row1 + dr, col1 + dc], cfgs[:, row1, col1 + dc]
    cand = np.stack([np.stack([c2, c1, c0, c3], axis=-1), np.stack([c0, c3, c2, c1], axis=-1)], axis=1).astype(np.int32)
    flag = np.stack([np.where(c0 == c2, 1, -1), np.where(c1 == c3, 1, -1)], axis=-1).astype(np.int32)
    return cand, flag


def _exchanged(ends):
    left, right = ends
    return np.stack([right, left], axis=-1)[:, None, :]


def per_call_reference(ctx, cfgs, orient, slice1):
    """[n][N - 1][4] exchanged amplitudes of every link of the pair through the per-call traces (zeros where there is no link), and the
    BTen2 stack sizes (LEFT, RIGHT) / (UP, DOWN) the sequence leaves"""
    from peps_amd import capi
    n, rows, cols = cfgs.shape
    N = cols if orient == HOR else rows
    out = np.zeros((n, N - 1, 4), dtype=ctx._ot)
    if orient == HOR:
        row = slice1
        ctx.init_bten2(capi.LEFT, row)
        ctx.grow_full_bten2(capi.RIGHT, row, 2, True)
        for col in range(cols - 1):
            for kind in (0, 1):
                out[:, col, kind] = ctx.replace_nnn_trace(row, col, kind, capi.HORIZONTAL, _exchanged(link_ends(cfgs, HOR, row, col, kind)))[:, 0]
            for kind in (2, 3):
                ends = link_ends(cfgs, HOR, row, col, kind)
                if ends is not None:
                    out[:, col, kind] = ctx.replace_sqrt5_trace(row, col, kind - 2, capi.HORIZONTAL, _exchanged(ends))[:, 0]
            ctx.shift_bten2_window(capi.RIGHT, row)
        return out, (ctx.bten2_stack_size(capi.LEFT), ctx.bten2_stack_size(capi.RIGHT))
    col = slice1
    ctx.init_bten2(capi.UP, col)
    ctx.grow_full_bten2(capi.DOWN, col, 3, True)
    for row in range(rows - 2):
        for kind in (2, 3):
            out[:, row, kind] = ctx.replace_sqrt5_trace(row, col, kind - 2, capi.VERTICAL, _exchanged(link_ends(cfgs, VER, col, row, kind)))[:, 0]
        if row + 3 < rows:
            ctx.shift_bten2_window(capi.DOWN, col)
    return out, (ctx.bten2_stack_size(capi.UP), ctx.bten2_stack_size(capi.DOWN))
