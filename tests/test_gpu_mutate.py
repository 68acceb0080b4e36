"""Adding rows to and removing rows from FlatIndex, ScalarIndex and BinaryIndex (include/vqhip.h, "adding and removing
rows") against the one statement there is: after any sequence of adds and removals, every call on
the index returns bit for bit what a fresh index over ref_mutate's rows returns.  Distances are compared as uint32 bits."""
import ctypes as C

import numpy as np
import pytest

import ref_mutate as RM
from vq_amd import (BinaryIndex, BinaryQuantizer, DimensionMismatch, Distance, FfiError, FlatIndex, InvalidParameter,
                    ScalarIndex, ScalarQuantizer, _lib)
from vq_amd.binary import pack_bits

pytestmark = pytest.mark.gpu
F = np.float32
SQ = ScalarQuantizer(-3.0, 3.0, 256)
BQ = BinaryQuantizer(0.0)
NQ = 5
N0 = 1501  # the removal shapes: not a multiple of 64 (a group) or of 1024 (a block)

# name -> (family, dtype of the rows, d, metric)
KINDS = {
    "flat32_d21": ("flat", np.float32, 21, "euclidean"),            # rb 84: 4-byte units
    "flat32_d128": ("flat", np.float32, 128, "euclidean"),          # rb 512: 16-byte units
    "flat32_d21_cos": ("flat", np.float32, 21, "cosine"),           # rnorm moves too
    "flat32_d128_cos": ("flat", np.float32, 128, "cosine"),
    "flat16_d21": ("flat", np.float16, 21, "squared_euclidean"),    # rb 42: byte units
    "sq_d1": ("sq", np.float32, 1, "manhattan"),                    # rb 1
    "sq_d21": ("sq", np.float32, 21, "euclidean"),                  # rb 21
    "sq_d21_cos": ("sq", np.float32, 21, "cosine"),
    "bin_d20": ("bin", np.float32, 20, "manhattan"),                # W 1, pad bits
    "bin_d96": ("bin", np.float32, 96, "manhattan"),                # W 3
    "bin_d1024": ("bin", np.float32, 1024, "manhattan"),            # W 32: rb 128, 16-byte units
}


def gen(kind, seed, b):
    """b rows of the kind, as its constructor and its ``add`` take them"""
    _, dtype, d, _ = KINDS[kind]
    return np.random.default_rng(seed).standard_normal((b, d)).astype(dtype)


def make(kind, rows):
    fam, _, _, metric = KINDS[kind]
    if fam == "flat":
        return FlatIndex(rows, Distance(metric))
    if fam == "sq":
        return ScalarIndex(rows, SQ, Distance(metric))
    return BinaryIndex(rows, BQ, Distance(metric))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_pair(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: indices differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: distance bits differ"


def same_csr(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: lims differ"
    assert np.array_equal(got[1], want[1]), f"{what}: indices differ"
    assert np.array_equal(bits(got[2]), bits(want[2])), f"{what}: distance bits differ"


def info_n(ix):
    """n as the handle's info entry point reports it"""
    h = ix._index()
    n = C.c_uint64(0)
    rest = {"vqhip_flat": 3, "vqhip_sqindex": 5, "vqhip_binary": 5}[h._prefix]
    _lib.check(getattr(_lib.load(), h._prefix + "_info")(h.raw, C.byref(n), *([None] * rest)))
    return int(n.value)


def file_bytes(ix, tmp_path, name):
    p = tmp_path / name
    ix.save(p)
    return p.read_bytes()


def check_invariant(kind, ix, rows, what, tmp_path=None, seed=7):
    """every call of the invariant on `ix` against a fresh index over `rows`, on NQ queries and a mask over the new n"""
    fam, _, d, _ = KINDS[kind]
    n = rows.shape[0]
    fresh = make(kind, rows)
    rng = np.random.default_rng(seed + n)
    Q = rng.standard_normal((NQ, d)).astype(F)
    mask = rng.random(n) < 0.5
    mask[int(rng.integers(n))] = True
    k = min(n, 10)
    assert len(ix) == n and info_n(ix) == n, f"{what}: len {len(ix)}, info {info_n(ix)}, want {n}"
    want = fresh.search(Q, k)
    same_pair(ix.search(Q, k), want, f"{what}: search")
    if n < 1024:  # the bounds follow the current n
        with pytest.raises(InvalidParameter):
            ix.search(Q, n + 1)
    with pytest.raises(DimensionMismatch):
        (ix.search(Q, k, allowed=np.ones(n + 1, bool)) if fam != "bin" else ix.filtered_search(Q, np.ones(n + 1, bool), k))
    if fam == "bin":
        same_pair(ix.filtered_search(Q, mask, k), fresh.filtered_search(Q, mask, k), f"{what}: filtered search")
        r = max(1, d // 2 - 2)
        same_csr(ix.hamming_range_search(Q, r), fresh.hamming_range_search(Q, r), f"{what}: range")
        same_csr(ix.filtered_hamming_range_search(Q, r, mask), fresh.filtered_hamming_range_search(Q, r, mask),
                 f"{what}: filtered range")
        assert np.array_equal(ix.packed(), fresh.packed()), f"{what}: packed() differs"
    else:
        same_pair(ix.search(Q, k, allowed=mask), fresh.search(Q, k, allowed=mask), f"{what}: masked search")
        radii = want[1][:, min(k - 1, 4)].copy()  # a handful of hits per query
        same_csr(ix.range_search(Q, radii), fresh.range_search(Q, radii), f"{what}: range")
        same_csr(ix.range_search(Q, radii, allowed=mask), fresh.range_search(Q, radii, allowed=mask), f"{what}: masked range")
        c = min(n, 16)
        cand = np.stack([rng.choice(n, c, replace=False) for _ in range(NQ)]).astype(np.uint32)
        same_pair(ix.rerank(Q, cand, min(c, 5)), fresh.rerank(Q, cand, min(c, 5)), f"{what}: rerank")
        if fam == "sq":
            assert np.array_equal(ix.codes(), fresh.codes()), f"{what}: codes() differs"
    if tmp_path is not None and fam != "flat":
        assert file_bytes(ix, tmp_path, "got") == file_bytes(fresh, tmp_path, "want"), f"{what}: the saved files differ"


def to_device(a):
    """a host array on the device: (tensor to keep alive, its pointer)"""
    import torch

    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.float16): np.float16}.get(a.dtype, a.dtype)
    t = torch.from_numpy(a.view(view).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr()


# -- removal ------------------------------------------------------------------------------------------------------------
def removal_masks(n):
    rng = np.random.default_rng(11)
    one = np.ones(n, bool)
    one[700] = False
    return {
        "random 20 %": rng.random(n) < 0.2,
        "rows 128..447 (whole groups and the best part of a block)": np.arange(128, 448),
        "row 0": np.array([0]),
        "row n - 1": np.array([n - 1], dtype=np.uint32),
        "all but one": one,
    }


@pytest.mark.parametrize("kind", list(KINDS))
def test_removal_equals_a_fresh_index(kind, tmp_path):
    rows = gen(kind, 1, N0)
    for name, m in removal_masks(N0).items():
        ix = make(kind, rows)
        got = ix.remove_rows(m)
        assert np.array_equal(got, RM.kept(N0, m)) and got.dtype == np.uint32, f"{kind}, {name}: kept differs"
        check_invariant(kind, ix, RM.apply(rows, [("remove", m)]), f"{kind}, {name}", tmp_path)


@pytest.mark.parametrize("kind", ["flat32_d128_cos", "sq_d21", "bin_d20"])
def test_removal_device_form(kind):
    rows = gen(kind, 2, N0)
    m = np.random.default_rng(12).random(N0) < 0.2
    ix = make(kind, rows)
    keep, ptr = to_device(RM.mask_words(N0, m))
    assert ix.remove_rows_device(ptr) == int(m.sum())
    check_invariant(kind, ix, rows[~m], f"{kind}, device form")
    none, ptr = to_device(np.zeros((len(ix) + 31) // 32, np.uint32))
    assert ix.remove_rows_device(ptr) == 0
    every, ptr = to_device(np.full((len(ix) + 31) // 32, 0xFFFFFFFF, np.uint32))
    with pytest.raises(FfiError) as e:
        ix.remove_rows_device(ptr)
    assert e.value.status == -3
    check_invariant(kind, ix, rows[~m], f"{kind}, behind a refused removal of every row")
    del keep, none, every


def test_scan_carry_more_blocks_than_one_pass():
    """1 Mi + 1500 rows are 1026 blocks of 1024 rows: the scan takes 1024 block counts per pass and carries into a second"""
    n = (1 << 20) + 1500
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 256, (n, 1), dtype=np.uint8)
    m = rng.random(n) < 0.5
    ix = ScalarIndex.from_codes(codes, SQ, Distance.manhattan())
    got = ix.remove_rows(m)
    assert np.array_equal(got, np.flatnonzero(~m).astype(np.uint32))
    assert len(ix) == int((~m).sum())
    assert np.array_equal(ix.codes(), codes[~m])


# -- append -------------------------------------------------------------------------------------------------------------
ADDS = (1, 63, 64, 1000)  # onto 300 rows: the capacity grows at the first (300 -> 450 rows) and at the last


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("kind", ["flat32_d21_cos", "flat32_d128", "flat16_d21", "sq_d21_cos", "bin_d20", "bin_d1024"])
def test_appends_across_capacity_growths(kind, form):
    rows = gen(kind, 4, 300)
    ix = make(kind, rows)
    for j, b in enumerate(ADDS):
        B = gen(kind, 40 + j, b)
        if form == "host":
            ids = ix.add(B)
        else:
            keep, ptr = to_device(B)
            ids = ix.add_device(ptr, b)
            del keep
        assert ids.dtype == np.uint32 and np.array_equal(ids, np.arange(rows.shape[0], rows.shape[0] + b))
        rows = RM.apply(rows, [("add", B)])
        check_invariant(kind, ix, rows, f"{kind}, {form} add of {b}")


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_scalar_add_equals_add_codes_of_the_quantizer(metric):
    rows, B = gen("sq_d21", 5, 300), gen("sq_d21", 6, 500)
    want = ScalarIndex(np.concatenate([rows, B]), SQ, Distance(metric))
    a = ScalarIndex(rows, SQ, Distance(metric))
    a.add(B)
    b = ScalarIndex(rows, SQ, Distance(metric))
    assert np.array_equal(b.add_codes(SQ.quantize_batch(B)), np.arange(300, 800))
    c = ScalarIndex(rows, SQ, Distance(metric))
    keep, ptr = to_device(SQ.quantize_batch(B))
    c.add_codes_device(ptr, 500)
    Q = gen("sq_d21", 7, NQ)
    for name, ix in (("add", a), ("add_codes", b), ("add_codes_device", c)):
        assert np.array_equal(ix.codes(), want.codes()), name
        same_pair(ix.search(Q, 10), want.search(Q, 10), name)


@pytest.mark.parametrize("d", [20, 96])
def test_binary_adds_of_the_three_kinds(d):
    kind = f"bin_d{d}"
    rows, B = gen(kind, 8, 300), gen(kind, 9, 500)
    want = BinaryIndex(np.concatenate([rows, B]), BQ).packed()
    forms = {
        "add": lambda ix: ix.add(B),
        "add_codes": lambda ix: ix.add_codes(BQ.quantize_batch(B)),
        "add_packed": lambda ix: ix.add_packed(pack_bits(B >= F(0.0))),
        "add_packed_device": lambda ix: ix.add_packed_device(to_device(pack_bits(B >= F(0.0)))[1], 500),
    }
    for name, add in forms.items():
        ix = BinaryIndex(rows, BQ)
        assert np.array_equal(add(ix), np.arange(300, 800)), name
        assert np.array_equal(ix.packed(), want), f"{name}: packed() differs"


@pytest.mark.parametrize("slack", [False, True])
def test_a_pad_bit_is_refused_and_the_index_unchanged(slack):
    """d = 20: bit 20 of a row's only word is a pad bit.  Host form (the package's check, then the library's own) and
    device form; with the buffer full (the add would have grown it) and with room behind the rows."""
    rows = gen("bin_d20", 10, 300)
    ix = BinaryIndex(rows, BQ)
    if slack:
        B = gen("bin_d20", 11, 1)
        ix.add(B)
        rows = np.concatenate([rows, B])
    before = ix.packed()
    bad = pack_bits(gen("bin_d20", 12, 3) >= F(0.0))
    bad[1, 0] |= np.uint32(1 << 20)
    with pytest.raises(InvalidParameter):
        ix.add_packed(bad)
    with pytest.raises(FfiError) as e:
        ix._index().add("add", bad, 3, _lib.BINARY_PACKED)
    assert e.value.status == -3
    keep, ptr = to_device(bad)
    with pytest.raises(FfiError) as e:
        ix.add_packed_device(ptr, 3)
    assert e.value.status == -3
    assert len(ix) == rows.shape[0] and info_n(ix) == rows.shape[0]
    assert np.array_equal(ix.packed(), before)
    check_invariant("bin_d20", ix, rows, "behind three refused adds")


# -- sequences ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat32_d21_cos", "flat16_d21", "sq_d21_cos", "bin_d96"])
def test_a_sequence_of_twelve_ops(kind, tmp_path):
    """12 ops: the first two take n from 1501 to 1 and up to about 3000, the other ten are drawn -- add, remove, and the
    read calls, which must change nothing.  The invariant is checked behind each."""
    rng = np.random.default_rng(sum(map(ord, kind)))  # (a seed per kind that is the same in every process)
    rows = gen(kind, 13, N0)
    ix = make(kind, rows)
    ops = ["remove_to_one", "add_many"] + [str(o) for o in rng.choice(["add", "remove", "search", "range", "filtered"], 10)]
    for j, op in enumerate(ops):
        n = rows.shape[0]
        if op == "remove_to_one":
            m = np.ones(n, bool)
            m[n // 3] = False
        elif op == "remove":
            m = rng.random(n) < float(rng.choice([0.1, 0.6]))
            m[int(rng.integers(n))] = False
        if op in ("remove_to_one", "remove"):
            assert np.array_equal(ix.remove_rows(m), RM.kept(n, m))
            rows = RM.apply(rows, [("remove", m)])
        elif op in ("add_many", "add"):
            B = gen(kind, 100 + j, 2999 - n if op == "add_many" else int(rng.choice([1, 70, 700])))
            ix.add(B)
            rows = RM.apply(rows, [("add", B)])
        # (the read ops are what check_invariant does anyway: search, range search and their filtered forms)
        check_invariant(kind, ix, rows, f"{kind}, op {j} ({op})", tmp_path if j in (0, 1, 11) else None, seed=j)


# -- pairing, file, stream order ----------------------------------------------------------------------------------------
def test_binary_search_with_a_flat_reranker_follows_both():
    d = 96
    rows = np.random.default_rng(14).standard_normal((N0, d)).astype(F)
    B = np.random.default_rng(15).standard_normal((700, d)).astype(F)
    m = np.random.default_rng(16).random(N0 + 700) < 0.3
    b, f = BinaryIndex(rows, BQ), FlatIndex(rows, Distance.cosine())
    for ix in (b, f):
        ix.add(B)
        ix.remove_rows(m)
    R = RM.apply(rows, [("add", B), ("remove", m)])
    Q = np.random.default_rng(17).standard_normal((NQ, d)).astype(F)
    want = BinaryIndex(R, BQ).search(Q, 10, rerank=FlatIndex(R, Distance.cosine()), candidates=64)
    same_pair(b.search(Q, 10, rerank=f, candidates=64), want, "binary search, flat rerank")


@pytest.mark.parametrize("kind", ["sq_d21_cos", "bin_d20"])
def test_save_and_load_behind_mutations(kind, tmp_path):
    rows, B = gen(kind, 18, 500), gen(kind, 19, 333)
    m = np.random.default_rng(20).random(833) < 0.4
    ix = make(kind, rows)
    ix.add(B)
    ix.remove_rows(m)
    R = RM.apply(rows, [("add", B), ("remove", m)])
    fresh = make(kind, R)
    assert file_bytes(ix, tmp_path, "got") == file_bytes(fresh, tmp_path, "want")
    back = type(ix).load(tmp_path / "got")
    Q = gen(kind, 21, NQ)
    assert len(back) == R.shape[0]
    same_pair(back.search(Q, 10), fresh.search(Q, 10), f"{kind}: the loaded index")


def test_a_queued_device_search_completes_on_the_old_rows():
    """A search_device is queued on stream A behind a blocker; an add that grows the buffer, and so frees the old one, then
    runs on stream B.  A's result is the statement for the old rows, the next search the statement for the new.  One pass."""
    import torch

    kind = "flat32_d21_cos"
    rows, B = gen(kind, 22, 300), gen(kind, 23, 1000)
    Q = gen(kind, 24, NQ)
    ix = make(kind, rows)
    want_old = ix.search(Q, 10)  # (the rows are on the device and the workspaces of this search exist)
    qd = torch.from_numpy(Q).to("cuda:0")
    idx = torch.zeros((NQ, 10), dtype=torch.int32, device="cuda:0")
    dist = torch.zeros((NQ, 10), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        _lib.set_stream(a.cuda_stream)
        with torch.cuda.stream(a):
            torch.cuda._sleep(12_000_000)  # about 5 ms: the search is still queued when the add enters
        ix.search_device(qd.data_ptr(), NQ, 10, idx.data_ptr(), dist.data_ptr())
        busy = not a.query()
        _lib.set_stream(b.cuda_stream)
        ix.add(B)
    finally:
        _lib.set_stream(None)
    torch.cuda.synchronize()
    assert busy, "no overlap achieved: the search had run before the add entered"
    same_pair((idx.cpu().numpy().view(np.uint32), dist.cpu().numpy()), want_old, "the queued search")
    check_invariant(kind, ix, np.concatenate([rows, B]), "behind the add")
