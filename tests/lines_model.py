"""The model of cz_search_lines (TEST INFRASTRUCTURE): principal variations restated in NumPy over one tree's pre-order dump.

A dump (SearchEngine.tree_dump / oracle.Search.tree_dump) is an int32 array of records {depth, label, N, bits(W), bits(Q),
bits(P), child_count or -1}: the root's children are the records of depth 0, in generation order, and the children of record
k are the records of depth[k] + 1 between k and the next record of depth <= depth[k], again in generation order.

Rules (include/cchess_hip.h: cz_search_lines): the candidates are the root's children whose label is allowed, in generation
order; line j starts at the candidate of rank j under "more visits first, earlier first among equals"; below it the line takes the
first maximum of N over the children of the node just appended, and stops without appending when that child has N <= 0, when
the node is not expanded, or at max_len."""
import numpy as np

DEPTH, LABEL, N, W, Q, P, COUNT = range(7)


def children_of(rec):
    """-> (root children, kids): the record indices of the root's children and, per record, of its children, generation order."""
    rec = np.asarray(rec)
    kids = [[] for _ in range(len(rec))]
    roots, path = [], []   # path[d] = the last record seen at depth d
    for k in range(len(rec)):
        d = int(rec[k, DEPTH])
        del path[d:]
        (kids[path[d - 1]] if d else roots).append(k)
        path.append(k)
    return roots, kids


def first_max(values):
    """Index of the first maximum (Python max() over a list in generation order; wave_most_visited)."""
    best = 0
    for i, x in enumerate(values):
        if x > values[best]:
            best = i
    return best


def lines_from_dump(rec, allowed, n_lines, max_len):
    """-> (moves uint16 [n_lines, max_len], visits int32, q float32 (the dump's bits), len uint16 [n_lines]) of one tree.
    allowed: None, or the labels a line may start with (any iterable)."""
    rec = np.asarray(rec, np.int32).reshape(-1, 7)
    moves = np.full((n_lines, max_len), 0xFFFF, np.uint16)
    visits = np.zeros((n_lines, max_len), np.int32)
    qbits = np.zeros((n_lines, max_len), np.int32)
    length = np.zeros(n_lines, np.uint16)
    roots, kids = children_of(rec)
    if allowed is not None:
        allowed = {int(x) for x in allowed}
        roots = [k for k in roots if int(rec[k, LABEL]) in allowed]
    order = sorted(range(len(roots)), key=lambda i: (-int(rec[roots[i], N]), i))
    for j in range(min(n_lines, len(order))):
        k, i = roots[order[j]], 0
        while True:
            moves[j, i], visits[j, i], qbits[j, i] = rec[k, LABEL], rec[k, N], rec[k, Q]
            i += 1
            if i >= max_len or rec[k, COUNT] <= 0 or not kids[k]:
                break
            best = kids[k][first_max([int(rec[c, N]) for c in kids[k]])]
            if rec[best, N] <= 0:
                break
            k = best
        length[j] = i
    return moves, visits, qbits.view(np.float32), length


def mask_labels(mask):
    """The labels whose bit is set in one [66] move-set mask (uint32 or int32 words)."""
    words = np.asarray(mask).astype(np.int64) & 0xFFFFFFFF
    return [w * 32 + b for w in range(len(words)) for b in range(32) if (int(words[w]) >> b) & 1]
