"""numpy restatement of mvx_views_reduce: rows of a selection summed back onto the shared atoms,

    out[n, j] = sum over the views b that hold atom n of rows[slot(b, n), j]

as a float64 sum per atom in ascending view order, with the bound sum |terms| the tolerance rule of tests/tolerance.py wants
(|got - ref| <= REL * bound + ABS). `index` / `offsets` are a selection as mvx_select_views returns it: segment b, ascending,
holds the atoms of view b. Run as a script, it checks itself against a dense B x N scatter.
"""
import numpy as np


def _rows2d(rows, total):
    r = np.asarray(rows, np.float64)
    return r.reshape(total, 1 if r.ndim == 1 else r.shape[1])


def reduce_reference(index, offsets, N, rows):
    """(out (N, W) float64, bound (N, W) float64) for rows (total,) or (total, W); views are added in ascending order."""
    index = np.asarray(index, np.int64)
    offsets = np.asarray(offsets, np.int64)
    r = _rows2d(rows, len(index))
    out = np.zeros((N, r.shape[1]))
    bound = np.zeros((N, r.shape[1]))
    for b in range(len(offsets) - 1):  # (atoms are distinct inside a segment: one term per atom and view)
        seg = slice(offsets[b], offsets[b + 1])
        out[index[seg]] += r[seg]
        bound[index[seg]] += np.abs(r[seg])
    return out, bound


def dense_reference(index, offsets, N, rows):
    """The same sum through a dense (B, N, W) scatter (small shapes only)."""
    index = np.asarray(index, np.int64)
    r = _rows2d(rows, len(index))
    B = len(offsets) - 1
    dense = np.zeros((B, N, r.shape[1]))
    view = np.repeat(np.arange(B), np.diff(offsets))
    dense[view, index] = r
    return dense.sum(0)


def random_selection(rng, B, N, keep=0.5, full=(), empty=(), never=()):
    """(index, offsets): every view keeps each atom with probability `keep`; views in `full` keep the whole cloud, views in
    `empty` nothing; atoms in `never` are in no view but the full ones."""
    segs = []
    for b in range(B):
        if b in full:
            m = np.ones(N, bool)
        elif b in empty:
            m = np.zeros(N, bool)
        else:
            m = rng.random(N) < keep
            m[list(never)] = False
        segs.append(np.flatnonzero(m).astype(np.int64))
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    return (np.concatenate(segs) if segs else np.zeros(0, np.int64)).astype(np.int64), offsets


def self_check():
    rng = np.random.default_rng(0)
    for B, N, W in ((1, 1, 1), (5, 7, 3), (65, 33, 4), (3, 40, 33)):
        index, offsets = random_selection(rng, B, N, full=(0,), empty=(B - 1,) if B > 1 else ())
        rows = rng.integers(-8, 9, (len(index), W)).astype(np.float64)  # small integers: every order of addition is exact
        out, bound = reduce_reference(index, offsets, N, rows)
        assert np.array_equal(out, dense_reference(index, offsets, N, rows))
        assert np.array_equal(bound, dense_reference(index, offsets, N, np.abs(rows)))
        rows = rng.standard_normal((len(index), W))
        out, bound = reduce_reference(index, offsets, N, rows)
        assert np.all(np.abs(out - dense_reference(index, offsets, N, rows)) <= 1e-15 * bound)
    out, bound = reduce_reference(np.zeros(0, np.int64), np.zeros(4, np.int64), 3, np.zeros((0, 2)))
    assert out.shape == (3, 2) and not out.any() and not bound.any()
    return True


if __name__ == "__main__":
    self_check()
    print("views_reduce_reference: ok")
