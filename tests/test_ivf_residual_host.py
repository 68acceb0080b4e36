"""CPU checks of the residual inverted-file PQ index (vq_amd.IVFPQIndex(..., residual=True), VQHIP_IVF_RESIDUAL): the
numpy statement (tests/ref_ivf_residual.py) against its brute-force restatement -- all metrics, one- and two-byte codes,
NaN / inf queries, ties, padding --, the zero-centroid identity with the non-residual statement, the Python checks, the
VQIVFRP1 file, and vqhip_ivfpq_create_ex / vqhip_ivfpq_flags, all without a device."""
import ctypes as C
import struct

import numpy as np
import pytest

import ref_ivf as R
import ref_ivf_residual as RR
import ref_knn as K

F = np.float32
METRICS = (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN)


@pytest.fixture(scope="module")
def orc():
    import oracle as O

    return O.get()


def _case(rng, n, nlist, m, k, sd, nq=6):
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = (rng.standard_normal((m, k, sd)) * 0.5).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8 if k <= 256 else np.uint16)
    codes[n // 2:n // 2 + 5] = codes[:5]  # duplicate codes: ties by row id within a list
    Q = rng.standard_normal((nq, m * sd)).astype(F)
    return coarse, cb, lists, codes, Q


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", [(300, 7, 4, 16, 3), (200, 1, 2, 300, 2), (400, 16, 8, 8, 1)])
@pytest.mark.parametrize("nprobe", [1, 3, "all"])
def test_statement_equals_brute_force(orc, metric, shape, nprobe):
    n, nlist, m, k, sd = shape
    rng = np.random.default_rng(n + nlist + 10 * metric + 1)
    coarse, cb, lists, codes, Q = _case(rng, n, nlist, m, k, sd)
    p = nlist if nprobe == "all" else min(nprobe, nlist)
    for topk in (1, 10, 64):
        _same(RR.search(orc, metric, coarse, cb, lists, codes, Q, p, topk),
              RR.brute_search(metric, coarse, cb, lists, codes, Q, p, topk))


@pytest.mark.parametrize("metric", METRICS)
def test_statement_nan_queries_ties_and_padding(orc, metric):
    rng = np.random.default_rng(5 + metric)
    coarse, cb, lists, codes, Q = _case(rng, 120, 9, 4, 16, 2, nq=4)
    lists[lists == 3] = 4  # an empty list
    Q[1, 0] = np.nan
    Q[2, -1] = np.inf
    Q[3, 2] = -np.inf
    codes[:] = codes[0]  # all rows one code: ties within a list
    sizes = np.bincount(lists, minlength=9)
    for p in (1, 2, 9):
        got = RR.search(orc, metric, coarse, cb, lists, codes, Q, p, 30)
        _same(got, RR.brute_search(metric, coarse, cb, lists, codes, Q, p, 30))
        P = R.probe(metric, coarse, Q, p)
        for j in range(Q.shape[0]):
            s = int(sizes[P[j]].sum())
            if s < 30:
                assert np.all(got[0][j, s:] == R.PAD_ID) and np.all(got[1][j, s:].view(np.uint32) == R.INF_BITS)
                assert np.all(got[0][j, :s] != R.PAD_ID)


@pytest.mark.parametrize("metric", METRICS)
def test_zero_centroids_equal_non_residual_statement(orc, metric):
    rng = np.random.default_rng(30 + metric)
    coarse, cb, lists, codes, Q = _case(rng, 500, 8, 4, 32, 2, nq=5)
    zero = np.zeros_like(coarse)
    Q[1, 0] = -0.0
    Q[2, 1] = np.nan
    Q[3, 0] = np.inf
    for p in (1, 3, 8):
        for topk in (1, 25, 200):
            _same(RR.search(orc, metric, zero, cb, lists, codes, Q, p, topk),
                  R.search(orc, metric, zero, cb, lists, codes, Q, p, topk))


def test_residual_is_exact_per_element():
    q = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, 1.0, 1e-45], F)
    z = np.zeros_like(q)
    assert np.array_equal(RR.residual(q, z).view(np.uint32), q.view(np.uint32))
    a = np.array([1.0, 3.0], F)
    b = np.array([1e-8, 1.0], F)
    assert np.array_equal(RR.residual(a, b), np.array([F(1.0) - F(1e-8), F(2.0)], F))


# ---- the Python class: checks before any device ------------------------------------------------

def _index(rng=None, nlist=5, m=2, k=16, sd=3, metric="euclidean", residual=True):
    import vq_amd

    rng = rng or np.random.default_rng(0)
    return vq_amd.IVFPQIndex(rng.standard_normal((nlist, m * sd)).astype(F), rng.standard_normal((m, k, sd)).astype(F),
                             vq_amd.Distance(metric), residual=residual)


def test_python_residual_flag_and_checks():
    import vq_amd
    from vq_amd import InvalidParameter

    cb = np.zeros((2, 16, 3), F)
    plain = vq_amd.IVFPQIndex(np.zeros((4, 6), F), cb)
    assert plain.residual is False
    assert repr(plain) == "IVFPQIndex(n=0, nlist=4, dim=6, m=2, k=16, distance=" + repr(plain.distance) + ")"
    res = vq_amd.IVFPQIndex(np.zeros((4, 6), F), cb, residual=True)
    assert res.residual is True and repr(res).endswith(", residual=True)")
    for bad in (1, "yes", None):
        with pytest.raises(InvalidParameter):
            vq_amd.IVFPQIndex(np.zeros((4, 6), F), cb, residual=bad)
    with pytest.raises(TypeError):  # keyword only
        vq_amd.IVFPQIndex(np.zeros((4, 6), F), cb, None, True)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFPQIndex(np.zeros((4, 6), F), cb, vq_amd.Distance("cosine"), residual=True)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFPQIndex.train(np.zeros((64, 6), F), 2, 2, 4, residual="no")
    ix = _index()
    ix.add_codes([1, 1, 4], np.array([[0, 1], [2, 3], [15, 15]]))
    with pytest.raises(InvalidParameter):
        ix.add_codes([0, 5], np.zeros((2, 2), np.uint8))
    q = np.zeros((2, 6), F)
    for bad in (0, 6, 1025):
        with pytest.raises(InvalidParameter):
            ix.search(q, topk=1, nprobe=bad)
    with pytest.raises(InvalidParameter):
        ix.search(q, topk=4, nprobe=2)
    i, d = ix.search(np.zeros((0, 6), F), topk=2, nprobe=2)
    assert i.shape == (0, 2) and d.shape == (0, 2)


def test_python_save_load_round_trip(tmp_path):
    import vq_amd

    rng = np.random.default_rng(4)
    for k in (16, 300):
        lists = rng.integers(0, 7, 50)
        codes = rng.integers(0, k, (50, 3))
        files = {}
        for residual in (False, True):
            ix = _index(np.random.default_rng(k), nlist=7, m=3, k=k, sd=2, metric="manhattan", residual=residual)
            ix.add_codes(lists, codes)
            p = tmp_path / f"ix{k}_{int(residual)}.bin"
            ix.save(p)
            back = vq_amd.IVFPQIndex.load(p)
            assert back.residual == residual and back.distance.metric == ix.distance.metric and len(back) == 50
            assert np.array_equal(back.coarse_centroids, ix.coarse_centroids)
            assert np.array_equal(back.codebooks, ix.codebooks)
            assert np.array_equal(back.list_ids, lists.astype(np.uint32)) and np.array_equal(back.codes, codes)
            files[residual] = p.read_bytes()
        # the same layout under another magic; the non-residual file is VQIVFPQ1 with reserved 0, as before
        assert files[False][:8] == b"VQIVFPQ1" and files[True][:8] == b"VQIVFRP1"
        assert files[False][8:] == files[True][8:]
        assert struct.unpack_from("<I", files[False], 28)[0] == 0
        assert len(files[False]) == 40 + 4 * (7 * 6 + 3 * k * 2 + 50) + 50 * 3 * (1 if k <= 256 else 2)


def _corrupt(tmp_path, mutate):
    import vq_amd

    ix = _index(np.random.default_rng(9), nlist=4)
    ix.add_codes([0, 3, 2], np.array([[1, 2], [3, 4], [5, 6]]))
    p = tmp_path / "c.bin"
    ix.save(p)
    raw = bytearray(p.read_bytes())
    assert raw[:8] == b"VQIVFRP1"
    p.write_bytes(bytes(mutate(raw)))
    with pytest.raises(ValueError):
        vq_amd.IVFPQIndex.load(p)


def _field(off, fmt, value):
    def f(raw):
        struct.pack_into(fmt, raw, off, value)
        return raw
    return f


@pytest.mark.parametrize("mutate", [
    lambda r: r[:20],                   # truncated header
    lambda r: b"VQIVFRP2" + r[8:],      # another magic
    _field(8, "<I", 3),                 # cosine
    _field(12, "<I", 7),                # dim not a multiple of m
    _field(16, "<I", 0),                # nlist 0
    _field(16, "<I", 70000),            # nlist too large
    _field(20, "<I", 0),                # m 0
    _field(24, "<I", 70000),            # k too large
    _field(28, "<I", 1),                # reserved
    _field(32, "<Q", 4),                # more rows than the file holds
    _field(32, "<Q", 1 << 40),          # n beyond 2^32
    lambda r: r[:-1],                   # truncated codes
    lambda r: r + b"\0",                # trailing bytes
    _field(40 + 4 * (4 * 6 + 2 * 16 * 3) + 4, "<I", 4),  # list id 4 of nlist 4
    lambda r: r[:-1] + bytes([16]),     # code 16 of k 16
])
def test_python_load_rejects_corrupt_residual_files(tmp_path, mutate):
    _corrupt(tmp_path, mutate)


# ---- the C ABI: create_ex and flags, host-only -------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from vq_amd import _lib

    return _lib


def _create_ex(lib, flags, nlist=4, m=2, k=16, sd=3, metric=1):
    coarse = np.zeros((max(nlist, 1), m * sd), F)
    cb = np.zeros((m, max(k, 1), sd), F)
    h = C.c_void_p()
    rc = lib.load().vqhip_ivfpq_create_ex(coarse.ctypes.data_as(lib._f32p), nlist, cb.ctypes.data_as(lib._f32p), m, k, sd,
                                          metric, flags, C.byref(h))
    return rc, h


def test_cabi_create_ex_and_flags(lib):
    L = lib.load()
    for bad in (2, 3, 0x80000000, 0xFFFFFFFF):
        rc, h = _create_ex(lib, bad)
        assert rc == lib.ERR_INVALID_INPUT and not h.value
    assert _create_ex(lib, 1, nlist=0)[0] == lib.ERR_INVALID_INPUT
    assert _create_ex(lib, 1, metric=lib.COSINE)[0] == lib.ERR_UNSUPPORTED
    assert _create_ex(lib, 1, m=151, k=256, sd=1)[0] == lib.ERR_UNSUPPORTED
    h = C.c_void_p()
    assert L.vqhip_ivfpq_create_ex(None, 4, None, 2, 16, 3, 1, 1, C.byref(h)) == lib.ERR_NULL_PTR
    f = C.c_uint32(7)
    assert L.vqhip_ivfpq_flags(None, C.byref(f)) == lib.ERR_NULL_PTR
    for flags in (0, lib.IVF_RESIDUAL):
        rc, h = _create_ex(lib, flags, k=300)
        assert rc == lib.OK
        try:
            assert L.vqhip_ivfpq_flags(h, None) == lib.ERR_NULL_PTR
            assert L.vqhip_ivfpq_flags(h, C.byref(f)) == lib.OK and f.value == flags
            lid = np.array([0, 3, 3], np.uint32)
            codes = np.array([[1, 299], [0, 0], [5, 7]], np.uint16)
            assert L.vqhip_ivfpq_add(h, lid.ctypes.data_as(lib._u32p), codes.ctypes.data_as(lib._vp), 3) == lib.OK
            sizes = np.zeros(4, np.uint64)
            assert L.vqhip_ivfpq_list_sizes(h, sizes.ctypes.data_as(lib._u64p)) == lib.OK and sizes.tolist() == [1, 0, 0, 2]
            q = np.zeros((2, 6), F)
            idx = np.zeros((2, 8), np.uint32)
            dist = np.zeros((2, 8), F)
            qp, ip, dp = q.ctypes.data_as(lib._f32p), idx.ctypes.data_as(lib._u32p), dist.ctypes.data_as(lib._f32p)
            for nprobe, topk in ((0, 1), (5, 1), (1, 0), (1, 4)):
                assert L.vqhip_ivfpq_search(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
            assert L.vqhip_ivfpq_search(h, qp, 0, 2, 2, ip, dp) == lib.OK
        finally:
            L.vqhip_ivfpq_destroy(h)
    # the Python handle passes the flag through
    ix = lib.IVFPQ(np.zeros((4, 6), F), np.zeros((2, 16, 3), F), lib.EUCLIDEAN, lib.IVF_RESIDUAL)
    assert ix.flags() == lib.IVF_RESIDUAL
    ix.close()
    ix = lib.IVFPQ(np.zeros((4, 6), F), np.zeros((2, 16, 3), F), lib.EUCLIDEAN)
    assert ix.flags() == 0
    ix.close()
