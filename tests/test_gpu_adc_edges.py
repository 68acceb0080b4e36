"""ADC search at the edges of its LDS plan (k_adc.hip): every batch size `qb` of both schedules, the largest table, the
row / topk switch between the schedules, the env switches, the three entry points and a PQIndex whose store changes.

The one-scan schedule (n >= 32768, topk <= 256) batches 8, 4, 2 or 1 queries by m*k (edges 4800, 9600, 19200); the
full pass batches min(8, 150 KiB / ((m*k + 512) * 4)) of them.  Both take tables up to m*k = 38400 and refuse larger
ones with VQHIP_ERR_UNSUPPORTED.  Every case holds a query equal to a stored row whose code is repeated across the
k-th place (D = 0 ties by row), a query with a NaN component (no row passes any threshold: the full pass repeats it at
this table size), and more queries than one batch, not a multiple of it.  Results are compared with the oracle,
indices exactly and distances bit for bit."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle as O

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = [O.SQUARED_EUCLIDEAN, O.EUCLIDEAN, O.MANHATTAN]


def _data(n, m, k, sd, nq, topk, seed, dense=0):
    """codebooks, codes and queries of one case: Q[0] is the reconstruction of row `src`, whose code also fills a block
    of topk + 7 rows (or `dense` rows); Q[1] has a NaN component"""
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8 if k <= 256 else np.uint16)
    src = 12345 % n
    block = dense if dense else topk + 7
    r0 = n // 3
    codes[r0:r0 + block] = codes[src]
    Q = rng.standard_normal((nq, m * sd)).astype(F)
    Q[0] = cb[np.arange(m), codes[src].astype(np.int64)].reshape(-1)
    Q[1, 0] = np.nan
    return cb, codes, Q


def _same(idx, dist, want_i, want_d):
    np.testing.assert_array_equal(idx, want_i)
    nan = np.isnan(want_d)
    np.testing.assert_array_equal(np.isnan(dist), nan)
    np.testing.assert_array_equal(np.where(nan, 0, dist.view(np.uint32)), np.where(nan, 0, want_d.view(np.uint32)))


def _check_redone(redone, n, m, k, nq, topk, one_scan, extra=0):
    if not one_scan:
        assert redone == nq, redone
    elif k ** m > 100 * n and topk <= 64:
        # the threshold is placed for >= 16 topk candidates: on random codes only the NaN query (and `extra` ones with
        # more than 8192 rows tied at the threshold) need the full pass
        assert redone == 1 + extra, redone
    else:
        assert 1 + extra <= redone <= nq, redone


def _run(oracle, metric, n, m, k, sd, nq, topk, seed, one_scan, dense=0, extra=0):
    from vq_amd import _lib

    cb, codes, Q = _data(n, m, k, sd, nq, topk, seed, dense)
    enc = _lib.PQEncoder(cb, metric)
    try:
        idx, dist = enc.adc_search(codes, Q, topk)
        redone = enc.adc_last_redone()
    finally:
        enc.close()
    want_i, want_d = oracle.adc_search(metric, cb, codes, Q, topk)
    _same(idx, dist, want_i, want_d)
    _check_redone(redone, n, m, k, nq, topk, one_scan, extra)
    return idx, dist, redone


# ---- the one-scan schedule: qb = 8 / 4 / 2 / 1 at m*k <= 4800 / 9600 / 19200 / 38400 ------------------------------------
# (name, n, m, k, sd, nq, topk); nq > qb and not a multiple of it
ONE_SCAN = [
    ("4799-u16-m1", 36_000, 1, 4799, 2, 11, 10),    # qb 8 (4799 is prime: one subspace, two-byte codes)
    ("4800-u8-m75", 36_000, 75, 64, 1, 11, 20),     # qb 8 at the edge; m not a multiple of 8: the byte-load path
    ("4800-u8-m24", 36_000, 24, 200, 1, 11, 64),    # qb 8 at the edge; rows of whole 8-byte words
    ("4800-u16-m16", 36_000, 16, 300, 1, 11, 65),   # qb 8 at the edge, two-byte codes
    ("4801-u16-m1", 36_000, 1, 4801, 1, 7, 10),     # qb 4
    ("9600-u8-m150", 36_000, 150, 64, 1, 7, 30),    # qb 4 at the edge, byte loads
    ("9600-u16-m32", 36_000, 32, 300, 1, 7, 256),   # qb 4 at the edge, the largest topk of the schedule
    ("9601-u16-m1", 36_000, 1, 9601, 2, 5, 10),     # qb 2
    ("19200-u8-m75", 36_000, 75, 256, 1, 5, 10),    # qb 2 at the edge
    ("19201-u8-m91", 36_000, 91, 211, 1, 3, 40),    # qb 1
    ("19201-u16-m7", 36_000, 7, 2743, 1, 3, 10),    # qb 1, two-byte codes
    ("38400-u8-m150", 36_000, 150, 256, 1, 3, 10),  # qb 1, the largest table (above the full pass's old 37888)
    ("38400-u16-m128", 36_000, 128, 300, 1, 3, 10),  # the largest table, two-byte codes
]


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", ONE_SCAN, ids=[s[0] for s in ONE_SCAN])
def test_gpu_adc_one_scan_batch_edges(oracle, metric, shape):
    _, n, m, k, sd, nq, topk = shape
    _run(oracle, metric, n, m, k, sd, nq, topk, seed=n + m * k + metric, one_scan=True)


# ---- the full pass: qb = min(8, 150 KiB / ((m*k + 512) * 4)), one shape inside each range --------------------------------
# forced by n < 32768 or topk > 256
FULL_PASS = [
    ("qb8", 30_000, 8, 256, 2, 11, 10),
    ("qb7", 33_000, 18, 256, 1, 9, 300),    # m*k 4608
    ("qb6", 30_000, 22, 256, 1, 8, 10),     # 5632
    ("qb5", 33_000, 27, 256, 1, 7, 257),    # 6912
    ("qb4", 30_000, 35, 256, 1, 6, 100),    # 8960
    ("qb3", 30_000, 40, 288, 1, 5, 10),     # 11520, two-byte codes
    ("qb2", 30_000, 70, 256, 1, 3, 10),     # 17920
    ("qb1", 30_000, 100, 256, 1, 3, 10),    # 25600
    ("qb1-38144", 30_000, 149, 256, 1, 3, 10),  # inside (37888, 38400]: refused before the plan took the CU's whole LDS
    ("qb1-38400", 30_000, 150, 256, 1, 3, 33),  # the largest table
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FULL_PASS, ids=[s[0] for s in FULL_PASS])
def test_gpu_adc_full_pass_batch_sizes(oracle, shape):
    name, n, m, k, sd, nq, topk = shape
    metric = METRICS[FULL_PASS.index(shape) % 3]
    _run(oracle, metric, n, m, k, sd, nq, topk, seed=n + m * k, one_scan=False)


@pytest.mark.gpu
def test_gpu_adc_largest_table_dense_ties(oracle):
    """m*k = 38400 under the one-scan schedule with 8200 rows tied at D = 0 for Q[0]: its threshold lets more than 8192
    rows pass, so Q[0] is repeated through the full pass as well as the NaN query"""
    _run(oracle, O.SQUARED_EUCLIDEAN, 36_000, 150, 256, 1, 3, 10, seed=5, one_scan=True, dense=8200, extra=1)


@pytest.mark.gpu
@pytest.mark.parametrize("n,topk", [(33_000, 10), (33_000, 300), (1000, 10)])
def test_gpu_adc_table_above_the_limit_is_refused(n, topk):
    """m*k = 38401 = 11 x 3491: both schedules refuse it with VQHIP_ERR_UNSUPPORTED and a message naming the table"""
    import vq_amd as pyvq
    from vq_amd import _lib
    from vq_amd.store import PQIndex

    rng = np.random.default_rng(1)
    m, k, sd = 11, 3491, 1
    cb = rng.standard_normal((m, k, sd)).astype(F)
    codes = rng.integers(0, k, (n, m)).astype(np.uint16)
    Q = rng.standard_normal((3, m * sd)).astype(F)
    enc = _lib.PQEncoder(cb, O.SQUARED_EUCLIDEAN)
    try:
        with pytest.raises(_lib.FfiError, match=r"m=11, k=3491") as e:
            enc.adc_search(codes, Q, topk)
        assert e.value.status == _lib.ERR_UNSUPPORTED
    finally:
        enc.close()
    index = PQIndex(cb, codes, pyvq.Distance.manhattan())
    with pytest.raises(pyvq.FfiError, match=r"m=11, k=3491") as e:
        index.search(Q, topk)
    assert e.value.status == _lib.ERR_UNSUPPORTED


# ---- where the schedules switch: n = 32767 / 32768, topk = 256 / 257, at a qb = 4 and a qb = 2 table -----------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [32_767, 32_768])
@pytest.mark.parametrize("topk", [256, 257])
@pytest.mark.parametrize("table", [(32, 256, 6), (64, 256, 3)], ids=["qb4", "qb2"])
def test_gpu_adc_schedule_switch_edges(oracle, n, topk, table):
    m, k, nq = table
    one_scan = n >= 32_768 and topk <= 256
    metric = METRICS[(n + topk + m) % 3]
    _run(oracle, metric, n, m, k, 1, nq, topk, seed=n + topk + m, one_scan=one_scan)


# ---- env switches, each in a fresh process (the library reads them once) ----------------------------------------------
_CHILD = textwrap.dedent("""
    import json, sys
    sys.path[:0] = [".", "oracle", "tests"]
    import numpy as np
    from test_gpu_adc_edges import _data
    from vq_amd import _lib
    a = json.loads(sys.argv[1])
    cb, codes, Q = _data(a["n"], a["m"], a["k"], a["sd"], a["nq"], a["topk"], a["seed"])
    enc = _lib.PQEncoder(cb, a["metric"])
    idx, dist = enc.adc_search(codes, Q, a["topk"])
    np.savez(a["out"], idx=idx, dist=dist, redone=enc.adc_last_redone())
    enc.close()
    print("ok")
""")


@pytest.mark.gpu
@pytest.mark.parametrize("env,shape,all_redone", [
    ({"VQHIP_ADC_FAST": "0"}, (40_000, 32, 256, 1, 6, 10), True),    # qb 4 table, n >= 32768: the full pass
    ({"VQHIP_ADC_FAST": "0"}, (40_000, 64, 256, 1, 3, 10), True),    # qb 2 table
    ({"VQHIP_TEST_ADC_REDO": "1"}, (40_000, 32, 256, 1, 6, 10), True),   # every query of a qb 4 one-scan repeated
    ({"VQHIP_TEST_ADC_REDO": "1"}, (40_000, 64, 256, 1, 3, 10), True),   # qb 2
    ({"VQHIP_TEST_ADC_REDO": "1"}, (40_000, 100, 256, 1, 3, 10), True),  # qb 1
], ids=["fast0-qb4", "fast0-qb2", "redo-qb4", "redo-qb2", "redo-qb1"])
def test_gpu_adc_env_switches_give_the_same_bits(oracle, tmp_path, env, shape, all_redone):
    n, m, k, sd, nq, topk = shape
    metric = O.EUCLIDEAN
    seed = n + m * k
    out = str(tmp_path / "r.npz")
    args = dict(n=n, m=m, k=k, sd=sd, nq=nq, topk=topk, seed=seed, metric=metric, out=out)
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(args)], env=dict(os.environ, **env), capture_output=True,
                       text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    got = np.load(out)
    idx, dist, redone = _run(oracle, metric, n, m, k, sd, nq, topk, seed=seed, one_scan=True)
    _same(got["idx"], got["dist"], idx, dist)
    assert int(got["redone"]) == (nq if all_redone else redone)


# ---- entry points: host codes, device codes, resident codes ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(36_000, 32, 256, 1, 6, 12), (36_000, 64, 256, 1, 3, 12), (36_000, 16, 300, 1, 6, 12)],
                         ids=["qb4", "qb2", "qb4-u16"])
def test_gpu_adc_entry_points_agree(oracle, shape):
    import torch
    import vq_amd as pyvq
    from vq_amd import _lib
    from vq_amd.store import PQIndex

    n, m, k, sd, nq, topk = shape
    cb, codes, Q = _data(n, m, k, sd, nq, topk, seed=n + m)
    want_i, want_d = oracle.adc_search(O.MANHATTAN, cb, codes, Q, topk)
    enc = _lib.PQEncoder(cb, O.MANHATTAN)
    try:
        _same(*enc.adc_search(codes, Q, topk), want_i, want_d)
        dev = torch.from_numpy(codes.view(np.int16) if codes.dtype == np.uint16 else codes).to("cuda")
        torch.cuda.synchronize()
        _same(*enc.adc_search((dev.data_ptr(), n), Q, topk), want_i, want_d)
        enc.adc_set_codes(codes)
        _same(*enc.adc_search(None, Q, topk), want_i, want_d)
    finally:
        enc.close()
    index = PQIndex(cb, codes, pyvq.Distance.manhattan())
    _same(*index.search(Q, topk), want_i, want_d)


# ---- a PQIndex answers for its current store ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_pq_index_follows_reassigned_store(oracle):
    import vq_amd as pyvq
    from vq_amd.store import PQIndex

    n, m, k, sd, nq, topk = 40_000, 8, 64, 4, 5, 9
    cb, codes, Q = _data(n, m, k, sd, nq, topk, seed=17)
    index = PQIndex(cb, codes, pyvq.Distance.squared_euclidean())
    _same(*index.search(Q, topk), *oracle.adc_search(O.SQUARED_EUCLIDEAN, cb, codes, Q, topk))

    codes2 = np.ascontiguousarray(codes[::-1][: n - 1000])
    index.codes = codes2
    _same(*index.search(Q, topk), *oracle.adc_search(O.SQUARED_EUCLIDEAN, cb, codes2, Q, topk))

    index.distance = pyvq.Distance.manhattan()
    _same(*index.search(Q, topk), *oracle.adc_search(O.MANHATTAN, cb, codes2, Q, topk))

    cb2 = (cb * F(2) + F(0.5)).astype(F)
    index.codebooks = cb2
    _same(*index.search(Q, topk), *oracle.adc_search(O.MANHATTAN, cb2, codes2, Q, topk))
