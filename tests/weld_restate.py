"""The rules of weld_vertices (include/pb3d.h: EQUALITY, CLASSES, FACES, ATTRIBUTES) restated in NumPy, a plain dictionary loop that the
restatement itself is held to, and the constructed inputs of tests/test_weld_vertices.py.

restate(): np.unique(axis=0) on the rows with -0.0 replaced by +0.0 (for finite rows, equal rows are then equal bytes and the other way
round), renumbered by first appearance.  loop() keys a dictionary with the tuple of Python floats, which compares as IEEE numbers do
(-0.0 == 0.0 and they hash alike)."""
import numpy as np


def _arrays(vertices, faces):
    V = np.asarray(vertices)
    V = np.ascontiguousarray(V if V.dtype == np.float32 else V.astype(np.float64)).reshape(-1, 3)
    assert np.isfinite(V).all()
    F = None if faces is None else np.asarray(faces).reshape(-1, 3)
    if F is not None and F.size and (int(F.min()) < -len(V) or int(F.max()) >= len(V)):
        raise IndexError(f"index out of bounds for {len(V)} entries")
    return V, F


def _pack(V, F, colors, index, inverse, counts):
    faces = None
    if F is not None:
        wrapped = np.where(F < 0, F.astype(np.int64) + len(V), F.astype(np.int64))
        faces = inverse[wrapped].astype(F.dtype).reshape(-1, 3)
    return dict(vertices=V[index].copy(), faces=faces, colors=None if colors is None else np.asarray(colors)[index].copy(),
                index=index.astype(np.int32), inverse=inverse.astype(np.int32), counts=counts.astype(np.int64))


def restate(vertices, faces=None, colors=None):
    """dict(vertices, faces or None, colors or None, index int32, inverse int32, counts int64)"""
    V, F = _arrays(vertices, faces)
    n = len(V)
    if n == 0:
        return _pack(V, F, colors, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    rows = V + V.dtype.type(0.0)                                               # -0.0 + 0.0 = +0.0, everything else unchanged
    _, first, inv, counts = np.unique(rows, axis=0, return_index=True, return_inverse=True, return_counts=True)   # first: smallest position
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")                                   # classes by first appearance
    number = np.empty(len(first), np.int64)
    number[order] = np.arange(len(first))
    return _pack(V, F, colors, first[order], number[inv], counts[order])


def loop(vertices, faces=None, colors=None):
    """the same result vertex by vertex"""
    V, F = _arrays(vertices, faces)
    seen, index, inverse, counts = {}, [], [], []
    for i, row in enumerate(V.tolist()):
        k = seen.setdefault(tuple(row), len(index))
        if k == len(index):
            index.append(i)
            counts.append(0)
        inverse.append(k)
        counts[k] += 1
    return _pack(V, F, colors, np.array(index, np.int64), np.array(inverse, np.int64), np.array(counts, np.int64))


def same(x, y):
    """two results equal in every output, vertices by their bytes"""
    for k in x:
        p, q = x[k], y[k]
        if (p is None) != (q is None):
            return False
        if p is not None and (p.dtype != q.dtype or p.shape != q.shape or p.tobytes() != q.tobytes()):
            return False
    return True


def soup(V, F):
    """every face three vertices of its own: (vertices, faces)"""
    V, F = np.asarray(V), np.asarray(F)
    return V[np.where(F < 0, F + len(V), F)].reshape(-1, 3).copy(), np.arange(3 * len(F), dtype=np.int32).reshape(-1, 3)


# ---- constructed inputs ------------------------------------------------------------------------------------------------------------------
def distinct(n, dtype=np.float32):
    i = np.arange(n, dtype=np.float64)
    return np.stack([np.sin(1.3 * i) + i, np.cos(0.7 * i), 0.25 * i], 1).astype(dtype)


def all_equal(n, dtype=np.float32):
    return np.tile(np.array([[0.1, -2.5, 3.0]], dtype), (n, 1))


def zero_pair():
    """rows 0 and 2 are one vertex (-0.0 == +0.0), and the representative keeps its sign bits"""
    return np.array([[-0.0, 1.0, 0.0], [0.5, 1.0, 0.0], [0.0, 1.0, -0.0], [-0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], np.float32)


def subnormals(dtype):
    t = np.finfo(dtype).smallest_subnormal
    return np.array([[t, 0.0, 0.0], [0.0, 0.0, 0.0], [t, 0.0, 0.0], [2 * t, 0.0, 0.0], [-t, 0.0, 0.0], [-0.0, 0.0, 0.0], [t, 0.0, -t]], dtype)


def word_neighbours():
    """float64 rows that differ from row 0 only in the low 32 bits of one coordinate, or only in the high 32 bits; then repeats"""
    base = np.array([1.0 + 2.0 ** -20, -3.0 - 2.0 ** -21, 0.75 + 2.0 ** -22])
    rows = [base.copy()]
    for a in range(3):
        for bit in (0, 31, 32, 51, 63):          # bits 0 .. 31 the low word, 32 .. 63 the high one
            r = base.copy()
            r[a:a + 1] = (r[a:a + 1].view(np.uint64) ^ np.uint64(1 << bit)).view(np.float64)
            rows.append(r)
    rows = np.array(rows)
    assert np.isfinite(rows).all()
    return np.concatenate([rows, rows[::-1], rows[::3]])
