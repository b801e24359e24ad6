"""Host buffers for the leading-dimension contract of every column loader (no device needed): a matrix on top of rows that must never
be read, the C contract's short form of the same, and the host-side checks that a test built on them is not vacuous."""
import numpy as np

PAD = 43


def padded(V, fill_rows=PAD):
    """V on top of `fill_rows` rows that must never be read as genotypes: NaN and inf (255 for codes)."""
    big = np.empty((V.shape[0] + fill_rows, V.shape[1]), dtype=V.dtype, order="F")
    big[:V.shape[0]] = V
    if V.dtype == np.uint8:
        big[V.shape[0]:] = 255
    else:
        big[V.shape[0]::2] = np.nan
        big[V.shape[0] + 1::2] = np.inf
    view = big[:V.shape[0]]
    assert view.strides == (V.itemsize, (V.shape[0] + fill_rows) * V.itemsize) and not view.flags.f_contiguous
    return view


def short_buffer(V, ld):
    """The C contract's short form: ncol - 1 columns of ld elements and a last one of N, not an element more; NaN (255) between."""
    n, ncol = V.shape
    flat = np.full((ncol - 1) * ld + n, 255 if V.dtype == np.uint8 else np.nan, dtype=V.dtype)
    for j in range(ncol):
        flat[j * ld:j * ld + n] = V[:, j]
    return flat


def leading_dimension(view):
    """Elements between two columns of a column-major view."""
    assert (view.shape[0] == 1 or view.strides[0] == view.itemsize) and view.strides[1] % view.itemsize == 0   # (one row: numpy's stride of it is free)
    return view.strides[1] // view.itemsize


def assert_poisoned(view):
    """What makes a test on padded(V) bite: the view is no copy (its parent is taller), every row below it holds a non-finite value
    (255 for codes), and the mean of every column over the parent's ld rows differs from the mean over the view's N rows -- a loader that
    read into the padding could not have produced the statistics of the N rows.  Returns the leading dimension."""
    big = view.base
    n, ld = view.shape[0], leading_dimension(view)
    assert big is not None and big.shape == (ld, view.shape[1]) and ld > n and np.shares_memory(big, view) and big.ctypes.data == view.ctypes.data
    below = big[n:]
    assert np.all(below == 255) if view.dtype == np.uint8 else not np.isfinite(below).any()
    with np.errstate(invalid="ignore"):
        over_ld, over_n = big.astype(np.float64).sum(axis=0) / ld, view.astype(np.float64).sum(axis=0) / n
    assert np.all(over_ld != over_n)   # (NaN differs from everything)
    return ld


def assert_short(flat, V, ld):
    """short_buffer's product: exactly (ncol - 1) ld + N elements, V's columns at their places and NaN (255) in every gap."""
    n, ncol = V.shape
    assert flat.ndim == 1 and flat.size == (ncol - 1) * ld + n and flat.dtype == V.dtype and ld > n
    gap = np.ones(flat.size, dtype=bool)
    for j in range(ncol):
        assert np.array_equal(flat[j * ld:j * ld + n], V[:, j])
        gap[j * ld:j * ld + n] = False
    assert gap.sum() == (ncol - 1) * (ld - n)
    assert np.all(flat[gap] == 255) if V.dtype == np.uint8 else np.isnan(flat[gap]).all()
