"""Removing rows from the four inverted-file indexes without a GPU (include/vqhip.h, "removing rows from an inverted
file"): every argument error leaves the index unchanged, an empty removal and a removal of every row, and -- with the
handle absent and with it present -- the calls that need no device against a fresh index given ref_mutate's rows in one
add.  No device is touched: ``uploads`` stays 0."""
import ctypes as C

import numpy as np
import pytest

import ivf_mutate_cases as IC
import ref_mutate as RM
from vq_amd import DimensionMismatch, InvalidParameter, _lib

N = 200
HOST_KINDS = ["flat32_d21", "flat16_d21_cos", "sq_d1", "sq_d21_cos", "bin_d20", "bin_d1024", "pq_m2_k16", "pq_m3_k300_res"]


def built(kind, handle, seed=0, n=N):
    lists, rows = IC.gen(kind, seed, n)
    ix = IC.make(kind)
    if handle:
        ix._handle()  # (host only: the device state is built by the first probe or search)
    IC.add(ix, kind, lists, rows)
    return ix, lists, rows


@pytest.mark.parametrize("handle", [False, True])
@pytest.mark.parametrize("kind", IC.ONE_PER_INDEX)
def test_argument_errors_leave_the_index_unchanged(kind, handle):
    ix, lists, rows = built(kind, handle)
    for bad, err in (([N], InvalidParameter), ([-1], InvalidParameter), (np.zeros(N + 1, bool), DimensionMismatch),
                     (np.zeros(N, np.float32), InvalidParameter), (np.zeros((2, N), bool), InvalidParameter)):
        with pytest.raises(err):
            ix.remove_rows(bad)
    IC.same_host_state(kind, ix, lists, rows, f"{kind}: behind five refused removals")
    assert (ix._ix is not None) == handle


@pytest.mark.parametrize("handle", [False, True])
@pytest.mark.parametrize("kind", IC.ONE_PER_INDEX)
def test_an_empty_removal_and_a_removal_of_every_row(kind, handle):
    ix, lists, rows = built(kind, handle)
    for nothing in ([], np.zeros(N, bool), np.empty(0, np.int64)):
        kept = ix.remove_rows(nothing)
        assert kept.dtype == np.uint32 and np.array_equal(kept, np.arange(N))
    IC.same_host_state(kind, ix, lists, rows, f"{kind}: behind empty removals")
    kept = ix.remove_rows(np.ones(N, bool))
    assert kept.dtype == np.uint32 and kept.shape == (0,)
    IC.same_host_state(kind, ix, lists[:0], rows[:0], f"{kind}: every row removed")
    # an empty index accepts only an empty removal
    assert ix.remove_rows([]).shape == (0,) and ix.remove_rows(np.zeros(0, bool)).shape == (0,)
    for bad in ([0], np.zeros(1, bool), np.zeros(1, np.float32), np.zeros((1, 0), bool)):
        with pytest.raises((InvalidParameter, DimensionMismatch)):
            ix.remove_rows(bad)
    l2, r2 = IC.gen(kind, 5, 40)  # and later adds work
    assert np.array_equal(IC.add(ix, kind, l2, r2), np.arange(40))
    IC.same_host_state(kind, ix, l2, r2, f"{kind}: 40 rows added to the emptied index")


@pytest.mark.parametrize("handle", [False, True])
@pytest.mark.parametrize("kind", HOST_KINDS)
def test_add_remove_add_remove_equals_a_fresh_index(kind, handle, tmp_path):
    ix, lists, rows = built(kind, handle, seed=1)
    rng = np.random.default_rng(2)
    removals = [rng.random(N) < 0.3, np.concatenate([[0], np.arange(64, 130), [N + 69]])]  # (N + 69: the last row then)
    for j, m in enumerate(removals):
        n = lists.shape[0]
        kept = ix.remove_rows(m)
        want = RM.kept(n, m)
        assert kept.dtype == np.uint32 and np.array_equal(kept, want), f"{kind}: kept differs"
        lists, rows = lists[want], rows[want]
        IC.same_host_state(kind, ix, lists, rows, f"{kind}, removal {j}", tmp_path)
        if j == 0:
            l2, r2 = IC.gen(kind, 3, N + 70 - lists.shape[0])  # up to N + 70 rows
            IC.add(ix, kind, l2, r2)
            lists, rows = np.concatenate([lists, l2]), np.concatenate([rows, r2])
            IC.same_host_state(kind, ix, lists, rows, f"{kind}, add behind removal {j}", tmp_path)
    if handle:
        assert ix._ix.uploads() == 0  # no device was touched


def test_a_removal_of_a_whole_list_and_of_partial_words():
    """list sizes follow, and the mask's last word is partial at n = 200 and whole at n = 192"""
    kind = "sq_d21"
    for n in (200, 192, 33, 32, 31, 1):
        ix, lists, rows = built(kind, True, seed=4, n=n)
        for which in ("the last row", "a whole list"):
            if lists.shape[0] == 0:
                continue
            m = np.array([lists.shape[0] - 1]) if which == "the last row" else lists == lists[0]
            keep = RM.kept(lists.shape[0], m)
            assert np.array_equal(ix.remove_rows(m), keep)
            lists, rows = lists[keep], rows[keep]
            IC.same_host_state(kind, ix, lists, rows, f"n = {n}")
            assert np.array_equal(ix._ix.codes(), rows)


PREFIXES = ("vqhip_ivfpq", "vqhip_ivfflat", "vqhip_ivfsq", "vqhip_ivfbin")


def test_every_new_entry_point_refuses_null_arguments():
    lib = _lib.load()
    words = np.zeros(1, np.uint32)
    out = C.c_uint64(7)
    handles = {IC.make(k)._handle()._prefix: IC.make(k) for k in IC.ONE_PER_INDEX}
    assert set(handles) == set(PREFIXES)
    for prefix, ix in handles.items():
        raw = ix._handle().raw
        remove, uploads = getattr(lib, prefix + "_remove"), getattr(lib, prefix + "_uploads")
        assert prefix + "_remove" in _lib.SIGNATURES and prefix + "_uploads" in _lib.SIGNATURES
        assert remove(None, _lib.ptr(words, _lib._u32p), C.byref(out)) == -1   # VQHIP_ERR_NULL_PTR
        assert remove(raw, None, C.byref(out)) == -1
        assert remove(raw, _lib.ptr(words, _lib._u32p), None) == -1
        assert uploads(None, C.byref(out)) == -1
        assert uploads(raw, None) == -1
        assert uploads(raw, C.byref(out)) == 0 and out.value == 0
        assert remove(raw, _lib.ptr(words, _lib._u32p), C.byref(out)) == 0 and out.value == 0  # (no rows: nothing removed)


def test_the_handle_counts_what_it_removes():
    ix, lists, rows = built("bin_d96", True, seed=6)
    m = np.random.default_rng(7).random(N) < 0.4
    assert ix._ix.remove(RM.mask_words(N, m)) == int(m.sum())
    assert ix._ix.info()[0] == N - int(m.sum())
    assert np.array_equal(ix._ix.packed(), rows[~m])
    assert np.array_equal(ix._ix.list_sizes(), np.bincount(lists[~m], minlength=IC.NLIST))


def test_ivfpq_gains_no_filtered_or_range_method():
    from vq_amd import IVFPQIndex

    assert hasattr(IVFPQIndex, "remove_rows")
    assert not [n for n in dir(IVFPQIndex) if n.startswith("filtered_") or "range" in n]
