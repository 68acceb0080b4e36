"""Adding and removing rows without a GPU: every argument error is raised with the index unchanged, the zero-row add and
the empty removal need no device, a real mutation fails loudly (ERR_NO_DEVICE), the C entry points check their handle,
and ref_mutate against hand-written cases."""
import ctypes as C

import numpy as np
import pytest

import ref_mutate as RM
from vq_amd import (BinaryIndex, BinaryQuantizer, DimensionMismatch, Distance, FfiError, FlatIndex, InvalidParameter,
                    ScalarIndex, ScalarQuantizer, _lib)

F = np.float32
SQ = ScalarQuantizer(-3.0, 3.0, 256)
N, D = 40, 20


def rows(n=N, d=D, dtype=F, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(dtype)


def indexes():
    return {
        "flat": FlatIndex(rows()),
        "flat16": FlatIndex(rows(dtype=np.float16), Distance.cosine()),
        "sq": ScalarIndex(rows(), SQ),
        "sq_codes": ScalarIndex.from_codes(np.zeros((N, D), np.uint8), SQ),
        "bin": BinaryIndex(rows()),
        "bin_packed": BinaryIndex.from_packed(np.zeros((N, 1), np.uint32), D),
    }


def no_device():
    return _lib.device_count() == 0


def unchanged(ix):
    assert len(ix) == N and ix._ix is None, "an argument error touched the index"


@pytest.mark.parametrize("name", list(indexes()))
def test_argument_errors_leave_the_index_unchanged(name):
    ix = indexes()[name]
    own = np.float16 if name == "flat16" else F
    other = F if name == "flat16" else np.float64
    with pytest.raises(InvalidParameter):
        ix.add(rows(3, dtype=other))          # the dtype is the index's own
    with pytest.raises(DimensionMismatch):
        ix.add(rows(3, D + 1, own))
    with pytest.raises(ValueError):
        ix.add(rows(3, dtype=own)[0])             # 1D
    with pytest.raises(InvalidParameter):
        ix.add_device(0x1000, -1)
    with pytest.raises(InvalidParameter):
        ix.add_device(0x1000, 1.5)
    with pytest.raises(InvalidParameter):
        ix.add_device(0x1000, (1 << 32) - N)      # n + b must stay below 2^32
    with pytest.raises(InvalidParameter):
        ix.remove_rows([N])                       # id range
    with pytest.raises(InvalidParameter):
        ix.remove_rows([-1])
    with pytest.raises(DimensionMismatch):
        ix.remove_rows(np.zeros(N + 1, bool))     # mask length
    with pytest.raises(InvalidParameter):
        ix.remove_rows(np.zeros(N, F))            # neither a mask nor ids
    with pytest.raises(InvalidParameter):
        ix.remove_rows(np.zeros((2, N), bool))
    with pytest.raises(InvalidParameter, match="would leave no row"):
        ix.remove_rows(np.ones(N, bool))
    with pytest.raises(InvalidParameter, match="would leave no row"):
        ix.remove_rows(np.arange(N)[::-1])
    unchanged(ix)


def test_the_forms_of_one_index_check_their_own_arguments():
    ix = indexes()
    with pytest.raises(InvalidParameter):
        ix["sq"].add_codes(rows(2))               # codes are uint8
    with pytest.raises(DimensionMismatch):
        ix["sq"].add_codes(np.zeros((2, D - 1), np.uint8))
    with pytest.raises(InvalidParameter):
        ix["sq"].add_codes_device(0x1000, -3)
    with pytest.raises(InvalidParameter):
        ix["bin"].add_codes(rows(2))
    with pytest.raises(InvalidParameter):
        ix["bin"].add_packed(np.zeros((2, 1), np.int32))
    with pytest.raises(DimensionMismatch):
        ix["bin"].add_packed(np.zeros((2, 2), np.uint32))     # W = 1 at d = 20
    with pytest.raises(InvalidParameter, match="pad bit"):
        ix["bin"].add_packed(np.array([[1], [1 << 20]], np.uint32))
    with pytest.raises(InvalidParameter):
        ix["bin"].add_packed_device(0x1000, -1)
    for x in ix.values():
        unchanged(x)


@pytest.mark.parametrize("name", list(indexes()))
def test_adding_nothing_and_removing_nothing_need_no_device(name):
    ix = indexes()[name]
    own = np.float16 if name == "flat16" else F
    ids = ix.add(np.empty((0, D), own))
    assert ids.dtype == np.uint32 and ids.shape == (0,)
    assert ix.add_device(0, 0).shape == (0,)
    for nothing in ([], np.zeros(N, bool), np.empty(0, np.int64)):
        kept = ix.remove_rows(nothing)
        assert kept.dtype == np.uint32 and np.array_equal(kept, np.arange(N))
    if name.startswith("sq"):
        assert ix.add_codes(np.empty((0, D), np.uint8)).shape == (0,) and ix.add_codes_device(0, 0).shape == (0,)
    if name.startswith("bin"):
        assert ix.add_codes(np.empty((0, D), np.uint8)).shape == (0,)
        assert ix.add_packed(np.empty((0, 1), np.uint32)).shape == (0,) and ix.add_packed_device(0, 0).shape == (0,)
    unchanged(ix)


@pytest.mark.parametrize("name", list(indexes()))
def test_a_real_mutation_fails_loudly_without_a_gpu(name):
    ix = indexes()[name]
    own = np.float16 if name == "flat16" else F
    if not no_device():  # with a GPU the same two host calls go through (tests/test_gpu_mutate.py holds them to the statement)
        assert np.array_equal(ix.add(rows(2, dtype=own)), [N, N + 1]) and len(ix) == N + 2
        assert np.array_equal(ix.remove_rows([1]), np.delete(np.arange(N + 2), 1)) and len(ix) == N + 1
        return
    for call in (lambda: ix.add(rows(2, dtype=own)), lambda: ix.remove_rows([1]), lambda: ix.remove_rows_device(0x1000)):
        with pytest.raises(FfiError) as e:
            call()
        assert e.value.status == -4  # VQHIP_ERR_NO_DEVICE
        assert len(ix) == N


ENTRY_POINTS = {
    "vqhip_flat_add": (None, 1), "vqhip_flat_add_device": (None, 1),
    "vqhip_sqindex_add_codes": (None, 1), "vqhip_sqindex_add_codes_device": (None, 1),
    "vqhip_sqindex_add_rows": (None, 1), "vqhip_sqindex_add_rows_device": (None, 1),
    "vqhip_binary_add": (None, 0, 1), "vqhip_binary_add_device": (None, 0, 1),
}
REMOVALS = ("vqhip_flat_remove", "vqhip_flat_remove_device", "vqhip_sqindex_remove", "vqhip_sqindex_remove_device",
            "vqhip_binary_remove", "vqhip_binary_remove_device")


def test_every_new_entry_point_refuses_a_null_handle():
    lib = _lib.load()
    words = np.zeros(1, np.uint32)
    removed = C.c_uint64(7)
    for name, args in ENTRY_POINTS.items():
        assert name in _lib.SIGNATURES
        assert getattr(lib, name)(None, *args) == -1, name              # VQHIP_ERR_NULL_PTR
        assert getattr(lib, name)(None, *args[:-1], 0) == -1, name      # the handle is checked before n_add == 0
    for name in REMOVALS:
        assert name in _lib.SIGNATURES
        src = C.c_void_p(words.ctypes.data) if name.endswith("_device") else _lib.ptr(words, _lib._u32p)
        assert getattr(lib, name)(None, src, C.byref(removed)) == -1, name


# -- ref_mutate against hand-written cases ------------------------------------------------------------------------------
def test_ref_mutate_by_hand():
    r = np.arange(12, dtype=F).reshape(6, 2)  # rows 0 .. 5: row i is (2 i, 2 i + 1)
    assert np.array_equal(RM.kept(6, [4, 1, 1]), [0, 2, 3, 5])
    assert np.array_equal(RM.kept(6, np.array([True, False, False, False, False, True])), [1, 2, 3, 4])
    assert np.array_equal(RM.kept(6, []), np.arange(6)) and RM.kept(6, []).dtype == np.uint32
    assert RM.new_id(6, [4, 1], 0) == 0 and RM.new_id(6, [4, 1], 3) == 2 and RM.new_id(6, [4, 1], 5) == 3
    out = RM.apply(r, [("remove", [4, 1])])
    assert np.array_equal(out[:, 0], [0, 4, 6, 10])
    b = np.array([[100, 101]], F)
    out = RM.apply(r, [("add", b), ("remove", [0, 6]), ("add", b), ("remove", np.array([False] * 5 + [True]))])
    assert np.array_equal(out[:, 0], [2, 4, 6, 8, 10])
    assert np.array_equal(RM.apply(r, []), r)
    with pytest.raises(AssertionError):
        RM.apply(r, [("remove", np.ones(6, bool))])
    # the C ABI's layout: row i is bit i & 31 of word i >> 5
    w = RM.mask_words(70, [0, 31, 32, 69])
    assert w.dtype == np.uint32 and w.tolist() == [0x80000001, 1, 1 << 5]


def test_remove_words_are_the_row_mask_layout():
    from vq_amd import pack_row_mask

    m = np.random.default_rng(1).random(1501) < 0.3
    assert np.array_equal(RM.mask_words(1501, m), pack_row_mask(m, 1501))
    assert np.array_equal(RM.mask_words(1501, np.flatnonzero(m)), pack_row_mask(np.flatnonzero(m), 1501))
