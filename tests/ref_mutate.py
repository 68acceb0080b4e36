"""The numpy statement of adding rows to and removing rows from a resident index (include/vqhip.h, "adding and removing
rows"): an index is a sequence of rows R[0 .. n), an add appends, a removal drops a set of rows and keeps the order of
the rest.  After any sequence of the two, every call on the index equals the same call on a fresh index over
``apply(rows, ops)``."""
from __future__ import annotations

import numpy as np


def remove_mask(n: int, mask_or_ids) -> np.ndarray:
    """bool (n,), True: removed -- from a bool mask (n,) or from row ids in [0, n), in any order, repeats welcome"""
    a = np.asarray(mask_or_ids)
    if a.dtype == np.bool_:
        assert a.shape == (n,), (a.shape, n)
        return a.copy()
    m = np.zeros(n, np.bool_)
    if a.size:
        ids = a.astype(np.int64)
        assert ids.min() >= 0 and ids.max() < n, (int(ids.min()), int(ids.max()), n)
        m[ids] = True
    return m


def kept(n: int, mask_or_ids) -> np.ndarray:
    """uint32: the old ids of the rows a removal leaves, in their new order (``kept[new id] = old id``)"""
    return np.flatnonzero(~remove_mask(n, mask_or_ids)).astype(np.uint32)


def new_id(n: int, mask_or_ids, i: int) -> int:
    """the id of surviving old row i behind the removal: i minus the removed rows below it"""
    m = remove_mask(n, mask_or_ids)
    assert not m[i], i
    return int(i - np.count_nonzero(m[:i]))


def mask_words(n: int, mask_or_ids) -> np.ndarray:
    """the removal as the C ABI takes it: uint32 (ceil(n / 32),), row i removed iff bit i & 31 of word i >> 5 is set"""
    m = remove_mask(n, mask_or_ids)
    words = np.zeros((n + 31) // 32, np.uint32)
    for i in np.flatnonzero(m).tolist():
        words[i >> 5] |= np.uint32(1 << (i & 31))
    return words


def apply(rows: np.ndarray, ops) -> np.ndarray:
    """`rows` (n, w) behind `ops`, a list of ("add", array (b, w)) and ("remove", mask_or_ids over the rows then in the
    index); a removal of every row is not a legal op"""
    r = np.ascontiguousarray(rows)
    for op, arg in ops:
        if op == "add":
            b = np.asarray(arg)
            assert b.ndim == 2 and b.shape[1] == r.shape[1] and b.dtype == r.dtype, (b.shape, b.dtype, r.shape, r.dtype)
            r = np.concatenate([r, b], axis=0)
        elif op == "remove":
            keep = ~remove_mask(r.shape[0], arg)
            assert keep.any(), "a removal leaves at least one row"
            r = r[keep]
        else:
            raise ValueError(op)
    return np.ascontiguousarray(r)
