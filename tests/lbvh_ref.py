"""What the device BVH build (go-raytracing_amd/csrc/build.hip) must produce,
restated from its definition in numpy and plain Python: no Karras searches,
no magic-multiply bit spreading, no atomics, no node slots.

  * Morton code of a triangle: the centroid 0.5f * (lo + hi) of its fp32 box,
    scaled into the mesh box by 1024 / extent (0 for a flat axis), clamped to
    [0, 1023], truncated; the three 10-bit numbers interleaved x, y, z from
    the top.  All in float32, one rounding per operation (the product is
    built with -ffp-contract=off).
  * Order: a stable sort of the codes.
  * Hierarchy: over the sorted 64-bit keys (code << 32 | position), a range
    splits after the last key that has 0 in the highest bit in which the
    range's first and last key differ.
  * Box of a subtree: min / max over its triangles' fp32 boxes (exact).
  * BVH4 collapse (build.hip's header): a node starts from its
    two children; while it has fewer than four, the child with the largest
    float32 dx*dy + dy*dz + dz*dx among the internal children of more than
    four triangles (first wins ties) is replaced, in place, by its two
    children.  A subtree of at most four triangles is one leaf over its
    contiguous sorted range.

The result is slot-free: `canon` lists the nodes in pre-order, each as a
tuple of children (box as six uint32 bit patterns, "N" or "L", first sorted
position, count); plus the node count, the leaf count and need4, the largest
sum over a root-to-leaf path of (children - 1)."""
import numpy as np

MAX_LEAF = 4
F = np.float32


def morton_codes(lo, hi, flo, fhi):
    """lo, hi: (n, 3) float32 box corners; flo, fhi: (3,) float32 frame."""
    lo, hi, flo, fhi = (np.asarray(a, F) for a in (lo, hi, flo, fhi))
    ext = fhi - flo
    sc = np.zeros(3, F)
    for a in range(3):
        if ext[a] > 0:
            sc[a] = F(1024.0) / ext[a]
    c = F(0.5) * (lo + hi)
    q = (c - flo[None, :]) * sc[None, :]
    assert q.dtype == F and not np.isnan(q).any()
    q = np.where(q < 0, F(0), np.where(q > 1023, F(1023), q))
    cell = np.trunc(q).astype(np.uint32)
    code = np.zeros(len(lo), np.uint32)
    for bit in range(10):
        for a in range(3):   # x above y above z
            code |= ((cell[:, a] >> np.uint32(bit)) & np.uint32(1)) << np.uint32(3 * bit + 2 - a)
    return code


def _area(box):
    dx, dy, dz = box[3] - box[0], box[4] - box[1], box[5] - box[2]   # float32 scalars
    return (dx * dy + dy * dz) + dz * dx


class Ref:
    pass


def build(lo, hi, flo, fhi):
    """Reference build of one mesh: .codes (per triangle), .perm (sorted
    position -> triangle), .canon, .nodes, .leaves, .need4, .depth2 (depth of
    the binary tree)."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    n = len(lo)
    assert n > MAX_LEAF
    r = Ref()
    r.codes = morton_codes(lo, hi, flo, fhi)
    r.perm = np.argsort(r.codes, kind="stable").astype(np.uint32)
    keys = (r.codes[r.perm].astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    assert (keys[1:] > keys[:-1]).all()
    slo, shi = lo[r.perm], hi[r.perm]

    # binary tree by the definition; node = [first, last, left, right], leaves are ranges of one
    first, last, left, right = [], [], [], []

    def new(a, b):
        first.append(a); last.append(b); left.append(-1); right.append(-1)
        return len(first) - 1

    root = new(0, n - 1)
    todo, depth = [(root, 1)], 1
    while todo:
        i, d = todo.pop()
        depth = max(depth, d)
        a, b = first[i], last[i]
        if a == b:
            continue
        top = int(keys[a] ^ keys[b]).bit_length() - 1
        zero = ((keys[a:b + 1] >> np.uint64(top)) & np.uint64(1)) == 0
        split = a + int(np.flatnonzero(zero)[-1])          # the last key with 0 in that bit
        assert a <= split < b and zero[:split - a + 1].all() and not zero[split - a + 1:].any()
        left[i], right[i] = new(a, split), new(split + 1, b)
        todo += [(left[i], d + 1), (right[i], d + 1)]
    r.depth2 = depth

    def box(i):
        a, b = first[i], last[i] + 1
        return np.concatenate([slo[a:b].min(axis=0), shi[a:b].max(axis=0)])

    def count(i):
        return last[i] - first[i] + 1

    r.canon, r.leaves, r.need4 = [], 0, 0
    todo = [(root, 0)]
    while todo:   # pre-order: children pushed in reverse
        i, need = todo.pop()
        kids = [left[i], right[i]]
        while len(kids) < 4:
            best, best_area = -1, F(-1.0)
            for q, k in enumerate(kids):
                if count(k) <= MAX_LEAF:
                    continue
                a = _area(box(k))
                if a > best_area:
                    best, best_area = q, a
            if best < 0:
                break
            k = kids[best]
            kids[best:best + 1] = [left[k], right[k]]
        need += len(kids) - 1
        rec, inner = [], []
        for k in kids:
            leaf = count(k) <= MAX_LEAF
            rec.append((tuple(box(k).view(np.uint32).tolist()), "L" if leaf else "N", first[k], count(k)))
            if leaf:
                r.leaves += 1
                r.need4 = max(r.need4, need)
            else:
                inner.append((k, need))
        r.canon.append(tuple(rec))
        todo += reversed(inner)
    r.nodes = len(r.canon)
    return r
