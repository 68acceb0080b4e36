"""Every kernel family held to its reference on rows that sit on both sides of a 32-bit boundary.

The rest of the suite stays below 2^31 elements and 2^31 bytes of any array, so a kernel that formed `row * d`, `i * m` or
`g * 8` in 32 bits would pass it.  Here the inputs are large enough that an offset product crosses byte 2^31, byte 2^32,
element 2^31, element 2^32 and, where the API allows that many rows, row 2^31 -- of the input and of the output.  Only
windows of rows are compared (tests/big_offsets.py: 2048 rows on each side of each boundary row, the first and the last
2048 rows), against the same references the small tests use: the C oracle, tests/ref_*.py and numpy.

The f32 input X (2^25 + 4099 rows x 128, 17 GB) is generated on the device by Dataset.synthetic; synth_uniform_host
regenerates any window of it on the host bit for bit.  Its boundary rows are 2^22 (byte 2^31), 2^23 (byte 2^32), 2^24
(element 2^31) and 2^25 (element 2^32); 4099 rows past the last, the end is ragged against every tile size.

Each test states its device memory need and skips with both numbers where the device has less free.  A run that
counts as evidence shows no skips here."""
import ctypes as C

import numpy as np
import pytest

import big_offsets as BO
import ref_centroids as RC
import ref_knn as RK
import ref_sqbq as RS
from vq_amd import _lib
from vq_amd import tsvq as TS
from vq_amd.bq import BinaryQuantizer
from vq_amd.errors import FfiError
from vq_amd.sq import ScalarQuantizer

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GiB = 1 << 30
D = 128
NX = (1 << 25) + 4099
SEED = 7
X_ROWS = BO.boundary_rows(NX, D, 4)  # (the codes and f16 rows of X's cases have their boundaries at these rows too)
X_SPANS = BO.windows(NX, X_ROWS.values())
N31 = (1 << 31) + 4099  # past row 2^31


def _need(nbytes, what):
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes / GiB:.1f} GiB of device memory; {free / GiB:.1f} GiB of {total / GiB:.1f} free")


def _sync():
    torch.cuda.synchronize()
    _lib.synchronize()


@pytest.fixture(scope="module")
def X():
    _need(NX * D * 4 + GiB, "X")
    _lib.set_device(0)
    ds = _lib.Dataset.synthetic(NX, D, seed=SEED)
    _sync()
    yield ds
    ds.close()
    _sync()
    torch.cuda.empty_cache()


_OWNED = []


def _own(h):
    """a library object (Dataset, PQEncoder, Flat, ...) closed when the test ends, passed or failed"""
    _OWNED.append(h)
    return h


@pytest.fixture(autouse=True)
def _free_after():
    yield
    _sync()
    while _OWNED:
        _OWNED.pop().close()
    torch.cuda.empty_cache()


def _host_rows(r0, r1):
    return _lib.synth_uniform_host(r1 - r0, D, SEED, r0)


def _codebooks_from_rows(m, k, first_row):
    """k rows of X (from first_row on) split into m sub-vectors: [m][k][D/m]"""
    rows = _lib.synth_uniform_host(k, D, SEED, first_row)
    return np.ascontiguousarray(rows.reshape(k, m, D // m).transpose(1, 0, 2))


# ---- PQ encode, device form ----

@pytest.mark.parametrize("m,k,metric", [
    (16, 256, _lib.SQUARED_EUCLIDEAN),  # bf16 screen (pipelined at this n)
    (16, 256, _lib.COSINE),
    (1, 256, _lib.SQUARED_EUCLIDEAN),   # sub_dim 128: the chunked variant
    (128, 256, _lib.SQUARED_EUCLIDEAN), # sub_dim 1: the exact engine; codes 4.3 GB, past byte 2^32
    (16, 256, _lib.MANHATTAN),
], ids=["m16-l2", "m16-cos", "m1-l2", "m128-l2", "m16-l1"])
def test_pq_encode_device_past_2e32(X, oracle, m, k, metric):
    """Crosses: X bytes 2^31 / 2^32 and elements 2^31 / 2^32 (rows 2^22 .. 2^25); the f16 output's bytes 2^31 / 2^32
    and elements 2^31 / 2^32; at m = 128 the codes' bytes 2^31 / 2^32."""
    _need(NX * (m + 2 * D) + GiB, "encode outputs")
    cb = _codebooks_from_rows(m, k, (1 << 24) + 11)
    enc = _own(_lib.PQEncoder(cb, metric))
    codes = torch.empty((NX, m), dtype=torch.uint8, device="cuda")
    f16 = torch.empty((NX, D), dtype=torch.float16, device="cuda")
    _sync()
    enc.encode_device(X.device_ptr, NX, codes.data_ptr(), f16.data_ptr())
    _sync()
    bad = []
    for r0, r1 in X_SPANS:
        want, want16 = oracle.pq_encode(metric, _host_rows(r0, r1), cb, want_f16=True, threads=0)
        got = codes[r0:r1].cpu().numpy().astype(np.uint32)
        got16 = f16[r0:r1].cpu().numpy().view(np.uint16)
        rows = np.nonzero((got != want).any(1) | (got16 != want16).any(1))[0]
        bad += [r0 + int(r) for r in rows[:4]]
    assert not bad, f"rows whose codes / f16 differ from the oracle: {bad} (boundaries {X_ROWS})"


def test_pq_encode_device_past_row_2e31(oracle):
    """d = 2, m = 1, k = 300 (two-byte codes), n = 2^31 + 4099.  Crosses: X bytes 2^31 / 2^32 and elements 2^31 / 2^32,
    codes bytes 2^31 / 2^32, f16 bytes 2^31 / 2^32, row 2^31."""
    d, m, k = 2, 1, 300
    _need(N31 * (4 * d + 2 * m + 2 * d) + GiB, "d = 2 encode")
    bounds = {}
    for name, (re, eb) in {"X": (d, 4), "codes": (m, 2), "f16": (d, 2)}.items():
        bounds.update({f"{name} {b}": r for b, r in BO.boundary_rows(N31, re, eb).items()})
    spans = BO.windows(N31, bounds.values())
    ds = _own(_lib.Dataset.synthetic(N31, d, seed=SEED))
    cb = _lib.synth_uniform_host(k, d, SEED + 1).reshape(1, k, d)
    enc = _own(_lib.PQEncoder(cb, _lib.SQUARED_EUCLIDEAN))
    codes = torch.empty((N31, m), dtype=torch.int16, device="cuda")
    f16 = torch.empty((N31, d), dtype=torch.float16, device="cuda")
    _sync()
    enc.encode_device(ds.device_ptr, N31, codes.data_ptr(), f16.data_ptr())
    _sync()
    bad = []
    for r0, r1 in spans:
        want, want16 = oracle.pq_encode(_lib.SQUARED_EUCLIDEAN, _lib.synth_uniform_host(r1 - r0, d, SEED, r0), cb,
                                        want_f16=True, threads=0)
        got = codes[r0:r1].cpu().numpy().view(np.uint16).astype(np.uint32)
        got16 = f16[r0:r1].cpu().numpy().view(np.uint16)
        rows = np.nonzero((got != want).any(1) | (got16 != want16).any(1))[0]
        bad += [r0 + int(r) for r in rows[:4]]
    assert not bad, f"rows whose codes / f16 differ from the oracle: {bad} (boundaries {bounds})"


# ---- decode and dequantize ----

@pytest.mark.parametrize("m,k", [(16, 256), (16, 300), (128, 256), (128, 300)],
                         ids=["lds", "global-u16", "m128-scalar", "m128-u16"])
def test_pq_decode_device_past_2e32(m, k):
    """Random codes made on the device, NX rows x D = 2^32 + 524672 output floats.  (16, 256): the codebooks in LDS;
    (16, 300): two-byte codes, the global gather; (128, 256) / (128, 300): sub_dim 1, codes past byte 2^32 (8.6 GB of
    two-byte codes at k = 300).  Crosses: the output's bytes 2^31 / 2^32 and elements 2^31 / 2^32 (rows 2^22 .. 2^25); at
    m = 128 the codes' bytes 2^31 / 2^32 (and their elements 2^31 / 2^32 at k = 300)."""
    cbytes = 1 if k <= 256 else 2
    _need(NX * (m * cbytes + 4 * D) + GiB, "decode")
    sd = D // m
    cb = np.random.default_rng(5).standard_normal((m, k, sd)).astype(np.float32)
    enc = _own(_lib.PQEncoder(cb, _lib.SQUARED_EUCLIDEAN))
    gen = torch.Generator(device="cuda").manual_seed(m * 1000 + k)
    codes = torch.randint(0, k, (NX, m), dtype=torch.uint8 if k <= 256 else torch.int16, device="cuda", generator=gen)
    out = torch.empty((NX, D), dtype=torch.float32, device="cuda")
    _sync()
    enc.decode_device(codes.data_ptr(), NX, out.data_ptr())
    _sync()
    bad = []
    for r0, r1 in X_SPANS:
        c = codes[r0:r1].cpu().numpy()
        c = (c.view(np.uint16) if k > 256 else c).astype(np.int64)
        want = np.concatenate([cb[s][c[:, s]] for s in range(m)], axis=1)
        got = out[r0:r1].cpu().numpy()
        rows = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
        bad += [r0 + int(r) for r in rows[:4]]
    assert not bad, f"decoded rows that differ from codebook[s][code]: {bad} (boundaries {X_ROWS})"


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd"])
def test_dequantize_f16_device_past_2e32(offset):
    """f16 -> f32 over 2^32 + 4099 elements of random bits; at offset 1 neither pointer is 16-byte aligned and the
    scalar loop runs the whole way.  Crosses: input bytes 2^31 / 2^32, elements 2^31 / 2^32 of both arrays, output bytes
    2^31 / 2^32."""
    count = (1 << 32) + 4099
    _need((count + 8) * 6 + GiB, "dequantize")
    gen = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randint(-32768, 32768, (count + 8,), dtype=torch.int16, device="cuda", generator=gen)
    out = torch.zeros(count + 8, dtype=torch.float32, device="cuda")
    _sync()
    _lib.dequantize_f16_device(src.data_ptr() + 2 * offset, count, out.data_ptr() + 4 * offset)
    _sync()
    bounds = {}
    for name, eb in (("in", 2), ("out", 4)):
        bounds.update({f"{name} {b}": e for b, e in BO.boundary_rows(count, 1, eb, rows=False).items()})
    bad = []
    for e0, e1 in BO.windows(count, bounds.values()):
        h = src[offset + e0:offset + e1].cpu().numpy().view(np.float16)
        want = h.astype(np.float32)
        got = out[offset + e0:offset + e1].cpu().numpy()
        nan = np.isnan(want)
        wrong = np.nonzero(((got.view(np.uint32) != want.view(np.uint32)) & ~nan) | (nan != np.isnan(got)))[0]
        bad += [e0 + int(e) for e in wrong[:4]]
    assert not bad, f"elements that differ from numpy's f16 -> f32: {bad} (boundaries {bounds})"
    # nothing written before or after the output
    assert not out[:offset].any().item() and not out[offset + count:].any().item()


# ---- SQ / BQ device forms ----

def test_sqbq_device_past_2e32(X):
    """Encode and decode of the first 2^32 + 4099 floats of X (values in [0, 1)) with a ScalarQuantizer that clamps at
    both ends and a BinaryQuantizer.  Crosses: input bytes 2^31 / 2^32 and elements 2^31 / 2^32, code bytes 2^31 / 2^32,
    output bytes and elements 2^31 / 2^32."""
    count = (1 << 32) + 4099
    _need(count * (1 + 4) + GiB, "SQ / BQ")
    codes = torch.empty(count, dtype=torch.uint8, device="cuda")
    out = torch.empty(count, dtype=torch.float32, device="cuda")
    bounds = {}
    for name, eb in (("in", 4), ("codes", 1)):
        bounds.update({f"{name} {b}": e for b, e in BO.boundary_rows(count, 1, eb, rows=False).items()})
    spans = BO.windows(count, bounds.values())
    sq = ScalarQuantizer(0.1, 0.9, 200)
    bq = BinaryQuantizer(0.5, 3, 7)
    for name, q, enc_ref, dec_ref in (
            ("sq", sq, lambda x: RS.sq_encode(0.1, 0.9, 200, x), lambda c: RS.sq_decode(0.1, 0.9, 200, c)),
            ("bq", bq, lambda x: RS.bq_encode(0.5, 3, 7, x), lambda c: RS.bq_decode(0.5, 3, 7, c))):
        _sync()
        q.quantize_device(X.device_ptr, count, codes.data_ptr())
        _sync()
        q.dequantize_device(codes.data_ptr(), count, out.data_ptr())
        _sync()
        bad = []
        for e0, e1 in spans:
            r0, r1 = e0 // D, (e1 + D - 1) // D
            x = _host_rows(r0, r1).reshape(-1)[e0 - r0 * D:e1 - r0 * D]
            c = codes[e0:e1].cpu().numpy()
            wrong = np.nonzero((c != enc_ref(x)) | (out[e0:e1].cpu().numpy().view(np.uint32) != dec_ref(c).view(np.uint32)))[0]
            bad += [e0 + int(e) for e in wrong[:4]]
        assert not bad, f"{name}: elements that differ from tests/ref_sqbq.py: {bad} (boundaries {bounds})"


# ---- ADC search, device form ----

def _adc_case(n, m, k, topk, seed):
    """codes [n][m] on the device (random in [1, k) with the planted rows written in), the planted rows nearest first, the
    boundaries crossed"""
    cbytes = 1 if k <= 256 else 2
    bounds = {f"codes {b}": r for b, r in BO.boundary_rows(n, m, cbytes).items()}
    # the full pass's distance row: row i's distance sits at byte 4 i of it
    bounds.update({f"distances {b}": r for b, r in BO.boundary_rows(n, 1, 4, rows=False).items()})
    planted = BO.adc_planted_rows(n, bounds.values())
    gen = torch.Generator(device="cuda").manual_seed(seed)
    codes = torch.randint(1, k, (n, m), dtype=torch.uint8 if cbytes == 1 else torch.int16, device="cuda", generator=gen)
    pc = torch.from_numpy(BO.adc_planted_codes(m, len(planted))).to(codes.dtype).cuda()
    codes[torch.tensor(planted, dtype=torch.int64, device="cuda")] = pc
    return codes, planted, bounds


def _adc_rows(codes, rows, k):
    c = codes[torch.from_numpy(np.asarray(rows, np.int64)).cuda()].cpu().numpy()
    return (c.view(np.uint16) if k > 256 else c).astype(np.int64)


@pytest.mark.parametrize("m,k,n", [
    (8, 256, (1 << 29) + 4099),  # rows of whole 8-byte words; codes past byte 2^32
    (2, 256, N31),               # the byte path, rows past 2^31
    (4, 300, (1 << 29) + 4099),  # two-byte codes past byte 2^32
], ids=["m8-words", "m2-row2e31", "m4-u16"])
def test_adc_search_device_past_2e32(m, k, n):
    """Both schedules: topk 10 (one scan against a sampled threshold) and topk 300 (the full pass, which writes one
    row of n distances per query: 8.6 GB at n = 2^31 + 4099).  Crosses: the codes' bytes 2^31 / 2^32 and elements
    2^31 / 2^32 and, at n > 2^31, row 2^31 (and the full pass's distance row past byte 2^32).  Two queries: at n > 2^25 the full pass takes fewer than a scan batch of them per
    group (one at n = 2^31 + 4099), so it runs several groups."""
    cbytes = 1 if k <= 256 else 2
    _need(n * m * cbytes + 4 * n + 2 * GiB, "ADC search")
    sd = 2
    cb = BO.adc_codebooks(m, k, sd)
    table = BO.adc_table(cb)
    codes, planted, bounds = _adc_case(n, m, k, 300, seed=m)
    enc = _own(_lib.PQEncoder(cb, _lib.SQUARED_EUCLIDEAN))
    q = np.zeros((2, m * sd), np.float32)
    spans = BO.windows(n, bounds.values())
    win = BO.window_index(spans)
    samp = BO.sample_rows(n, 1_000_000, seed=3)
    check_rows = np.unique(np.concatenate([win, samp]))
    check_d = BO.adc_distances(table, _adc_rows(codes, check_rows, k))
    _sync()
    for topk in (10, 300):
        idx3, dist3 = enc.adc_search((codes.data_ptr(), n), q, topk)
        assert np.array_equal(idx3[1:], idx3[:-1]) and np.array_equal(dist3[1:].view(np.uint32), dist3[:-1].view(np.uint32)), \
            f"topk {topk}: equal queries, different results"
        idx, dist = idx3[0].astype(np.int64), dist3[0]
        lead = min(topk, len(planted))
        assert list(idx[:lead]) == planted[:lead], f"topk {topk}: planted rows {planted[:lead]}, got {list(idx[:lead])}"
        want = BO.adc_distances(table, _adc_rows(codes, idx, k))
        assert np.array_equal(dist.view(np.uint32), want.view(np.uint32)), f"topk {topk}: distances differ from numpy"
        order = np.lexsort((idx, dist))
        assert np.array_equal(order, np.arange(topk)), f"topk {topk}: results not in (distance, row) order"
        ahead = BO.beats(check_d, check_rows, dist[-1], idx[-1], idx)
        assert ahead.size == 0, f"topk {topk}: rows {ahead[:8]} beat the k-th result (boundaries {bounds})"


# ---- FlatIndex ----

def test_flat_f32_past_2e32(X):
    """Exact k-NN over X (f32, d = 128); queries are the rows just past each boundary and the last row.  Crosses: X bytes
    2^31 / 2^32 and elements 2^31 / 2^32.  Then rerank with candidates past 2^25."""
    _need(NX * D * 4 + 8 * NX * 4 + GiB, "flat search (the index's copy of X, distance rows)")
    flat = _own(_lib.Flat(np.empty((0, D), np.float32), _lib.SQUARED_EUCLIDEAN, dev_rows=X.device_ptr, shape=(NX, D)))
    qrows = [r + 1 for r in X_ROWS.values()] + [NX - 1]
    Q = np.concatenate([_host_rows(r, r + 1) for r in qrows])
    topk = 10
    idx, dist = flat.search(Q, topk)
    win = BO.window_index(X_SPANS)
    samp = np.unique(np.concatenate([np.arange(b, b + 4096) for b in BO.sample_rows(NX - 4096, 244, seed=4)]))
    rows = np.unique(np.concatenate([win, samp]))
    XR = np.concatenate([_host_rows(a, b) for a, b in _runs(rows)])
    for j, r in enumerate(qrows):
        got_i, got_d = idx[j].astype(np.int64), dist[j]
        assert got_i[0] == r, f"query = row {r}: first result {got_i[0]}"
        want = RK.distances(RK.SQUARED_EUCLIDEAN, Q[j], np.concatenate([_host_rows(i, i + 1) for i in got_i]))
        assert np.array_equal(got_d.view(np.uint32), want.view(np.uint32)), f"query = row {r}: distances differ from ref_knn"
        ahead = BO.beats(RK.distances(RK.SQUARED_EUCLIDEAN, Q[j], XR), rows, got_d[-1], got_i[-1], got_i)
        assert ahead.size == 0, f"query = row {r}: rows {ahead[:8]} beat the k-th result"
    # rerank: candidates on both sides of every boundary and the end, brute force over them
    cand = np.array([sorted({c for b in X_ROWS.values() for c in (b - 2, b - 1, b, b + 1)} | {NX - 2, NX - 1})] * len(qrows),
                    np.uint32)
    ridx, rdist = flat.rerank(Q, cand, 5)
    XC = np.concatenate([_host_rows(int(i), int(i) + 1) for i in cand[0]])
    for j in range(len(qrows)):
        wi, wd = RK.topk_of(RK.distances(RK.SQUARED_EUCLIDEAN, Q[j], XC), cand[0], 5)
        assert np.array_equal(ridx[j], wi) and np.array_equal(rdist[j].view(np.uint32), wd.view(np.uint32)), \
            f"rerank of query {j}: got {ridx[j]}, want {wi}"


def _runs(rows):
    """sorted row ids -> [r0, r1) runs of consecutive ids"""
    rows = np.asarray(rows, np.int64)
    cut = np.nonzero(np.diff(rows) != 1)[0] + 1
    return [(int(s[0]), int(s[-1]) + 1) for s in np.split(rows, cut)]


def test_flat_f16_past_row_2e31():
    """Exact k-NN over f16 rows, d = 2, n = 2^31 + 4099; the query rows (just past each boundary, and the last row) are
    written with values no other row holds, so each is its own unique nearest.  Crosses: rows bytes 2^31 / 2^32 and
    elements 2^31 / 2^32, row 2^31.  Then rerank with candidates past 2^31."""
    d, n = 2, N31
    _need(n * (2 * 2 * d + 4) + GiB, "f16 flat search (rows, the index's copy, one distance row)")
    bounds = BO.boundary_rows(n, d, 2)
    gen = torch.Generator(device="cuda").manual_seed(9)
    rows_t = torch.rand((n, d), dtype=torch.float16, device="cuda", generator=gen)
    qrows = sorted({r + 1 for r in bounds.values() if r + 1 < n} | {n - 1})
    qv = torch.tensor([[-1.0 - j / 8, 2.0 + j / 8] for j in range(len(qrows))], dtype=torch.float16, device="cuda")
    rows_t[torch.tensor(qrows, device="cuda")] = qv
    Q = qv.float().cpu().numpy()
    flat = _own(_lib.Flat(np.empty((0, d), np.float16), _lib.SQUARED_EUCLIDEAN, dev_rows=rows_t.data_ptr(), shape=(n, d)))
    _sync()
    topk = 10
    idx, dist = flat.search(Q, topk)
    check = np.unique(np.concatenate([BO.window_index(BO.windows(n, bounds.values())), BO.sample_rows(n, 1_000_000, 6)]))
    XR = rows_t[torch.from_numpy(check).cuda()].float().cpu().numpy()
    for j, r in enumerate(qrows):
        got_i, got_d = idx[j].astype(np.int64), dist[j]
        assert got_i[0] == r, f"query = row {r}: first result {got_i[0]}"
        XI = rows_t[torch.from_numpy(got_i).cuda()].float().cpu().numpy()
        want = RK.distances(RK.SQUARED_EUCLIDEAN, Q[j], XI)
        assert np.array_equal(got_d.view(np.uint32), want.view(np.uint32)), f"query = row {r}: distances differ from ref_knn"
        ahead = BO.beats(RK.distances(RK.SQUARED_EUCLIDEAN, Q[j], XR), check, got_d[-1], got_i[-1], got_i)
        assert ahead.size == 0, f"query = row {r}: rows {ahead[:8]} beat the k-th result"
    cand = np.array([sorted({c for b in bounds.values() for c in (b - 1, b, b + 1) if c < n} | {n - 1})] * len(qrows), np.uint32)
    ridx, rdist = flat.rerank(Q, cand, 3)
    XC = rows_t[torch.from_numpy(cand[0].astype(np.int64)).cuda()].float().cpu().numpy()
    for j in range(len(qrows)):
        wi, wd = RK.topk_of(RK.distances(RK.SQUARED_EUCLIDEAN, Q[j], XC), cand[0], 3)
        assert np.array_equal(ridx[j], wi) and np.array_equal(rdist[j].view(np.uint32), wd.view(np.uint32)), \
            f"rerank of query {j}: got {ridx[j]}, want {wi}"


# ---- Lloyd step ----

def _lloyd_init(m, k):
    """init rows [m][k]: even centroids from rows past 2^24, odd ones from rows past 2^25, all distinct"""
    j = np.arange(k, dtype=np.uint64)[None, :]
    s = np.arange(m, dtype=np.uint64)[:, None]
    base = np.where(j % 2 == 0, np.uint64((1 << 24) + 1), np.uint64((1 << 25) + 1))
    return (base + 8 * j + s).astype(np.uint64)


def test_lloyd_step_past_2e32(X, oracle):
    """One Lloyd step over X, m = 16, k = 256, from rows past 2^24 and 2^25, one centroid patched from row NX - 7; the same
    step again under exact_update.  Window codes against the oracle, counts against a bincount of every code, subspaces
    0 and 15 against the f64 bound summed over every row (exact in f64: the values are multiples of 2^-24 in [0, 1)), and
    under exact_update bit-identical to the sequential f32 sums in row order.  Crosses: X bytes 2^31 / 2^32 and elements
    2^31 / 2^32 (rows 2^22 .. 2^25) in the assignment and the update."""
    m, k = 16, 256
    sd = D // m
    _need(2 * NX * m + 4 * GiB, "Lloyd step (codes and slabs)")
    init = _lloyd_init(m, k)
    patch = (3, 5, NX - 7)
    results = []
    for exact in (False, True):
        km = _own(_lib.KMeans(X, m, k))
        km.set_exact_update(exact)
        km.init_from_rows(init)
        km.patch_from_row(*patch)
        c0 = km.get_centroids()
        want0 = np.stack([np.concatenate([_host_rows(int(r), int(r) + 1)[:, s * sd:(s + 1) * sd] for r in init[s]])
                          for s in range(m)])
        want0[patch[0], patch[1]] = _host_rows(patch[2], patch[2] + 1)[0, patch[0] * sd:(patch[0] + 1) * sd]
        assert np.array_equal(c0.view(np.uint32), want0.view(np.uint32)), "initial centroids differ from the host rows"
        counts, _ = km.step()
        results.append((counts, km.get_assignments(), km.get_centroids()))
        km.close()
    (counts, assign, c1), (counts_e, assign_e, c1_e) = results
    assert np.array_equal(assign, assign_e) and np.array_equal(counts, counts_e), "exact_update changed the assignment"
    for r0, r1 in X_SPANS:
        want, _ = oracle.pq_encode(_lib.SQUARED_EUCLIDEAN, _host_rows(r0, r1), want0, want_f16=False, threads=0)
        bad = np.nonzero((assign[r0:r1].astype(np.uint32) != want).any(1))[0]
        assert bad.size == 0, f"rows {[r0 + int(b) for b in bad[:4]]}: codes differ from the oracle (boundaries {X_ROWS})"
    for s in range(m):
        assert np.array_equal(np.bincount(assign[:, s], minlength=k), counts[s]), f"subspace {s}: counts != bincount"
    # every row's columns of subspaces 0 and 15, read back in chunks
    subs = (0, m - 1)
    cols = {s: np.empty((NX, sd), np.float32) for s in subs}
    for r0 in range(0, NX, 1 << 21):
        r1 = min(NX, r0 + (1 << 21))
        Xc = X.read(r0, r1 - r0)
        for s in subs:
            cols[s][r0:r1] = Xc[:, s * sd:(s + 1) * sd]
        del Xc
    for s in subs:
        c, S = BO.f64_sums(assign[:, s], cols[s], k)
        mu = S / np.maximum(c, 1)[:, None]
        B = RC.bound(c, mu, S)  # A = S: every value is >= 0
        err = np.abs(c1[s].astype(np.float64) - mu)
        bad = np.argwhere((c > 0)[:, None] & ~(err <= B))
        assert bad.size == 0, f"subspace {s}: {len(bad)} centroid components outside the f64 bound, first {bad[0]}"
        want = BO.sequential_f32_means(assign[:, s], cols[s], k)  # exact_update: row order in f32, divided in f32
        ne = c > 0
        assert np.array_equal(c1_e[s][ne].view(np.uint32), want[ne].view(np.uint32)), \
            f"subspace {s}: exact_update centroids differ from the sequential f32 sums"


# ---- TSVQ ----

def _tsvq_tree(d, depth):
    """a tree built on 65536 rows of the synthetic matrix of width d (rows spread over the first 2^24)"""
    rows = np.concatenate([_lib.synth_uniform_host(256, d, SEED, r) for r in range(0, 1 << 24, 1 << 16)])
    ds = _own(_lib.Dataset.from_host(rows))
    cent, left, right = TS.build_tree(ds, depth)
    return dict(centroids=cent, left=left, right=right)


def _tsvq_encoder(tree, d, metric):
    h = C.c_void_p()
    _lib.check(_lib.load().vqhip_tsvq_create(_lib.ptr(tree["centroids"], _lib._f32p), _lib.ptr(tree["left"], _lib._i32p),
                                             _lib.ptr(tree["right"], _lib._i32p), tree["centroids"].shape[0], d, metric,
                                             C.byref(h)))
    return _own(TS._TsvqHandle(h))


def _tsvq_encode_windows(oracle, tree, t, dev_rows, n, d, metric, spans, host_rows):
    leaf = torch.empty(n, dtype=torch.int32, device="cuda")
    f16 = torch.empty((n, d), dtype=torch.float16, device="cuda")
    _sync()
    _lib.check(_lib.load().vqhip_tsvq_encode_device(t.raw, dev_rows, n, leaf.data_ptr(), f16.data_ptr()))
    _sync()
    bad = []
    for r0, r1 in spans:
        want, want16 = oracle.tsvq_encode(metric, host_rows(r0, r1), tree, want_f16=True, threads=0)
        got = leaf[r0:r1].cpu().numpy()
        got16 = f16[r0:r1].cpu().numpy().view(np.uint16)
        rows = np.nonzero((got != want) | (got16 != want16).any(1))[0]
        bad += [r0 + int(r) for r in rows[:4]]
    return bad


@pytest.mark.parametrize("metric", [_lib.SQUARED_EUCLIDEAN, _lib.EUCLIDEAN, _lib.MANHATTAN, _lib.COSINE],
                         ids=["l2sq", "l2", "l1", "cos"])
def test_tsvq_encode_device_past_2e32(X, oracle, metric):
    """Depth-8 tree on a sample; leaves and f16 rows of all of X.  Crosses: X bytes 2^31 / 2^32 and elements 2^31 / 2^32,
    the f16 output's bytes 2^31 / 2^32 and elements 2^31 / 2^32 (rows 2^22 .. 2^25)."""
    _need(NX * (4 + 2 * D) + GiB, "TSVQ encode outputs")
    tree = _tsvq_tree(D, 8)
    t = _tsvq_encoder(tree, D, metric)
    bad = _tsvq_encode_windows(oracle, tree, t, X.device_ptr, NX, D, metric, X_SPANS, _host_rows)
    assert not bad, f"rows whose leaf / f16 differ from the oracle: {bad} (boundaries {X_ROWS})"


def test_tsvq_encode_device_past_row_2e31(oracle):
    """d = 2, n = 2^31 + 4099 (the exact descent: d is not a multiple of 4).  Crosses: rows bytes 2^31 / 2^32 and
    elements 2^31 / 2^32, leaves bytes 2^31 / 2^32 and elements 2^31, f16 bytes 2^31 / 2^32, row 2^31."""
    d, n = 2, N31
    _need(n * (4 * d + 4 + 2 * d) + GiB, "d = 2 TSVQ encode")
    bounds = {}
    for name, (re, eb) in {"X": (d, 4), "leaf": (1, 4), "f16": (d, 2)}.items():
        bounds.update({f"{name} {b}": r for b, r in BO.boundary_rows(n, re, eb).items()})
    ds = _own(_lib.Dataset.synthetic(n, d, seed=SEED))
    tree = _tsvq_tree(d, 8)
    t = _tsvq_encoder(tree, d, _lib.SQUARED_EUCLIDEAN)
    bad = _tsvq_encode_windows(oracle, tree, t, ds.device_ptr, n, d, _lib.SQUARED_EUCLIDEAN, BO.windows(n, bounds.values()),
                               lambda r0, r1: _lib.synth_uniform_host(r1 - r0, d, SEED, r0))
    assert not bad, f"rows whose leaf / f16 differ from the oracle: {bad} (boundaries {bounds})"


def test_tsvq_build_refuses_2e31_rows():
    """The build takes fewer than 2^31 rows: n = 2^31 (d = 1) is refused with VQHIP_ERR_UNSUPPORTED before any work."""
    _need((1 << 31) * 4 + GiB, "2^31 x 1 rows")
    ds = _own(_lib.Dataset.synthetic(1 << 31, 1, seed=SEED))
    with pytest.raises(FfiError) as e:
        TS.build_tree(ds, 2)
    assert e.value.status == _lib.ERR_UNSUPPORTED, str(e.value)


# ---- host form past 2^32 elements (the transfer driver's lanes) ----

def test_sq_quantize_batch_host_past_2e32():
    """ScalarQuantizer.quantize_batch on a host array of 2^32 + 4099 floats (17 GB in, 4.3 GB out).  Only the windows hold
    data (synthetic rows); the rest is zero.  Crosses: host and device bytes 2^31 / 2^32 and elements 2^31 / 2^32 of the
    input and of the codes."""
    count = (1 << 32) + 4099
    _need(2 * GiB, "host-form SQ staging")
    bounds = {}
    for name, eb in (("in", 4), ("codes", 1)):
        bounds.update({f"{name} {b}": e for b, e in BO.boundary_rows(count, 1, eb, rows=False).items()})
    spans = BO.windows(count, bounds.values())
    x = np.zeros(count, np.float32)
    for e0, e1 in spans:
        r0, r1 = e0 // D, (e1 + D - 1) // D
        x[e0:e1] = _host_rows(r0, r1).reshape(-1)[e0 - r0 * D:e1 - r0 * D]
    codes = ScalarQuantizer(0.1, 0.9, 200).quantize_batch(x)
    bad = []
    for e0, e1 in spans:
        wrong = np.nonzero(codes[e0:e1] != RS.sq_encode(0.1, 0.9, 200, x[e0:e1]))[0]
        bad += [e0 + int(e) for e in wrong[:4]]
    assert not bad, f"elements that differ from tests/ref_sqbq.py: {bad} (boundaries {bounds})"
