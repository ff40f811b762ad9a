"""
The numpy mirror of csrc/ehm_reach.hip: the reach tube, the limit set and the step
sets of a may-reach relation given as CSR, straight from the definitions.  Seeds (``level == 0``) are
absorbing: ``post`` never reads their rows.  The boxes are numpy's min / max over the vertices of the
cells the caller hands in (``certify_cpu.cells`` or ``invariance_cpu`` vertices; NaN rows: no cell),
plus 0.0 so that a zero bound is +0 whatever order the device met its zeros in.
"""

from types import SimpleNamespace

import numpy as np


def post(mask, indptr, indices, level):
    """bool [n]: the union of the rows of the non-seed leaves of ``mask``."""
    n = mask.size
    active = mask & (level != 0)
    out = np.zeros(n, dtype=bool)
    out[indices[np.repeat(active, np.diff(indptr))]] = True
    return out


def leaf_boxes(V):
    """[n, 2, p]: lo and hi per coordinate of the cells V [n, p+1, p]; NaN without a cell."""
    V = np.asarray(V, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.stack([V.min(axis=1), V.max(axis=1)], axis=1)


def set_box(mask, boxes):
    """[2, p]: the box of the leaves of ``mask`` that have a cell; NaN when there is none."""
    p = boxes.shape[2]
    sel = boxes[mask & ~np.isnan(boxes).any(axis=(1, 2))]
    if sel.shape[0] == 0:
        return np.full((2, p), np.nan)
    return np.stack([sel[:, 0].min(axis=0), sel[:, 1].max(axis=0)]) + 0.


def reach(indptr, indices, level, start, V=None, horizon=0, max_sweeps=None):
    """``start``: bool [n].  ``V`` [n, p+1, p] (None: no leaf has a cell, p = 1).  The fields are
    those of ``invariance.ReachResult``; ``D`` is the list of the sets D_j that were made and
    ``steps`` always there."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int32)
    level = np.asarray(level, dtype=np.int32)
    start = np.asarray(start, dtype=bool)
    n = level.size
    assert indptr.size == n + 1 and start.shape == (n,) and start.any()
    boxes = leaf_boxes(np.full((n, 2, 1), np.nan) if V is None else V)
    max_sweeps = n if max_sweeps is None else int(max_sweeps)
    cap = min(max_sweeps, n)
    # A: arrival
    arrival = np.where(start, 0, -1).astype(np.int32)
    reached = start.copy()
    tube_box, tube_count = [set_box(reached, boxes)], [int(reached.sum())]
    a_done, sweeps_a = False, 0
    for k in range(1, cap + 1):
        sweeps_a = k
        new = post(arrival == k - 1, indptr, indices, level) & (arrival < 0)
        if not new.any():
            a_done = True
            break
        arrival[new] = k
        reached |= new
        tube_box.append(set_box(reached, boxes))
        tube_count.append(int(reached.sum()))
    closure = arrival >= 0
    n_arrival = int(arrival.max())
    seeds = closure & (level == 0)
    leak = int(arrival[seeds].min()) if seeds.any() else -1
    # B: the limit set
    depart = np.full(n, -1, dtype=np.int32)
    limit = limit_outer = settle = settle_box = settle_count = None
    D = []
    b_done = False
    if a_done and leak < 0:
        cur = closure.copy()
        D, settle_box, settle_count = [cur], [set_box(cur, boxes)], [int(cur.sum())]
        settle = cap
        for j in range(1, cap + 1):
            nxt = post(cur, indptr, indices, level)
            assert not (nxt & ~cur).any()           # post(closure) lies in the closure
            gone = cur & ~nxt
            if not gone.any():
                b_done, settle = True, j - 1
                break
            depart[gone] = j
            cur = nxt
            D.append(cur)
            settle_box.append(set_box(cur, boxes))
            settle_count.append(int(cur.sum()))
            if not cur.any():
                b_done, settle = True, j
                break
        if b_done:
            limit = cur
        else:
            limit_outer = cur
        settle_box = np.array(settle_box)
        settle_count = np.array(settle_count, dtype=np.int64)
    # C: the step sets
    last = int(horizon)
    if leak >= 0:
        last = min(last, leak)
    if not a_done:
        last = min(last, max_sweeps)
    R = [start.copy()]
    for k in range(last):
        R.append(post(R[-1], indptr, indices, level))
    return SimpleNamespace(
        arrival=arrival, closure=closure, n_arrival=n_arrival, leak_step=leak, safe=leak < 0,
        limit=limit, limit_outer=limit_outer, depart=depart, settle=settle,
        tube_box=np.array(tube_box), tube_count=np.array(tube_count, dtype=np.int64),
        settle_box=settle_box, settle_count=settle_count,
        limit_box=None if settle_box is None else settle_box[-1],
        step_box=np.array([set_box(r, boxes) for r in R]),
        step_count=np.array([int(r.sum()) for r in R], dtype=np.int64),
        steps=np.array(R).astype(np.uint8), D=D, leaf_box=boxes,
        converged=a_done and (b_done or leak >= 0), sweeps_arrival=sweeps_a)
