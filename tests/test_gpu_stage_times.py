"""Stage times of a profiled pass come from the kernels' own dispatches.

With the hooks on (`vqhip_set_profiling`) a pass's first kernel carries a start event and the last kernel of each
stage a stop event, all taken from the library's event pool; nothing is recorded on the stream.  For every launch
sequence of `run_assign` this checks the contract of `vqhip_profile_collect` -- one record per pass, a positive
screen-stage time, a re-check time that is zero exactly when there is no re-check stage, both together no longer
than the passes took on the wall clock -- and that the hooks change no code.  The pool must not grow with the number
of profiled passes: at any time it holds three events per pass not collected yet and one per handle."""
import time

import numpy as np
import pytest
import torch

from vq_amd import _lib

pytestmark = pytest.mark.gpu
PASSES = 5

# (n, d, m, k, engine): every launch sequence of an encode pass
ENCODE_CASES = {
    "pipelined_ragged": (40007, 128, 8, 256, None),      # three-product pipelined screen, ragged last step
    "x32_short": (256, 128, 8, 256, "bf16"),             # too short to pipeline: the plain X32 kernel (AUTO would scan)
    "transposed_m16": (40007, 128, 16, 256, None),       # screen + k_codes_transpose in the first stage
    "grouped_merge": (4096, 128, 4, 512, None),          # grouped screen + k_merge_partials_x32
    "exact": (10000, 64, 4, 16, None),                   # one kernel, no re-check stage
}


def _timed_passes(fn, count):
    _lib.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    _lib.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _check_record(record, wall_ms, calls, recheck_stage):
    got_calls, primary_ms, recheck_ms = record
    print(f"calls {got_calls} primary_ms {primary_ms:.4f} recheck_ms {recheck_ms:.4f} wall_ms {wall_ms:.4f}")
    assert got_calls == calls
    assert primary_ms > 0
    assert recheck_ms >= 0
    if not recheck_stage:
        assert recheck_ms == 0
    assert primary_ms + recheck_ms <= wall_ms
    assert _lib.profile_collect()[0] == 0  # the record is cleared


@pytest.mark.parametrize("case", list(ENCODE_CASES))
def test_encode_stage_times(case):
    n, d, m, k, engine = ENCODE_CASES[case]
    _lib.load()
    _lib.set_stream(None)
    rng = np.random.default_rng(5)
    ds = _lib.Dataset.synthetic(n, d, 21, 0)
    enc = _lib.PQEncoder(rng.random((m, k, d // m), dtype=np.float32), _lib.SQUARED_EUCLIDEAN)
    if engine == "bf16":
        enc.set_engine(_lib.ENGINE_MFMA_BF16)
    width = 1 if k <= 256 else 2
    plain = torch.zeros((n, m * width), dtype=torch.uint8, device="cuda")
    hooked = torch.zeros((n, m * width), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        _lib.set_profiling(False)
        enc.encode_device(ds.device_ptr, n, plain.data_ptr(), None)
        _lib.synchronize()
        _, used_engine = _lib.last_assign_stats()
        assert (used_engine == _lib.ENGINE_EXACT) == (case == "exact")
        _lib.set_profiling(True)
        _lib.profile_collect()
        wall_ms = _timed_passes(lambda: enc.encode_device(ds.device_ptr, n, hooked.data_ptr(), None), PASSES)
        _check_record(_lib.profile_collect(), wall_ms, PASSES, recheck_stage=case != "exact")
        assert torch.equal(plain, hooked)
    finally:
        _lib.set_profiling(False)
        enc.close()
        ds.close()


def test_kmeans_run_stage_times():
    """`KMeans.run(2)` with the hooks on is two host-driven iterations, one assignment pass each: the fused update, with
    `launch_accumulate_listed` behind the re-check in the second stage."""
    n, d, m, k = 40007, 64, 8, 256
    _lib.load()
    _lib.set_stream(None)
    ds = _lib.Dataset.synthetic(n, d, 22, 0)
    init = np.array([[(j * (n // k) + s) % n for j in range(k)] for s in range(m)], np.uint64)
    results = []
    try:
        for hooks in (False, True):
            km = _lib.KMeans(ds, m, k)
            km.init_from_rows(init)
            _lib.set_profiling(hooks)
            _lib.profile_collect()
            _lib.synchronize()
            t0 = time.perf_counter()
            iters, counts, _, paused = km.run(2)
            wall_ms = (time.perf_counter() - t0) * 1e3
            assert not paused and int(iters.min()) == int(iters.max()) == 2
            if hooks:
                _check_record(_lib.profile_collect(), wall_ms, 2, recheck_stage=True)
            results.append((km.get_centroids(), km.get_assignments(), counts))
            km.close()
    finally:
        _lib.set_profiling(False)
        ds.close()
    for plain, hooked in zip(*results):
        assert plain.tobytes() == hooked.tobytes()


def test_event_pool_stays_bounded():
    """200 toggles of the hooks with one pass each: the pool ends with at most the three events of one profiled pass and
    the one the encoder's last kernel carries more than it began with."""
    n, d, m, k = 4096, 128, 8, 256
    _lib.load()
    _lib.set_stream(None)
    rng = np.random.default_rng(6)
    ds = _lib.Dataset.synthetic(n, d, 23, 0)
    enc = _lib.PQEncoder(rng.random((m, k, d // m), dtype=np.float32), _lib.SQUARED_EUCLIDEAN)
    enc.set_engine(_lib.ENGINE_MFMA_BF16)
    codes = torch.zeros((n, m), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        _lib.set_profiling(False)
        _lib.profile_collect()
        before = _lib.event_pool_count()
        profiled = 0
        for toggle in range(200):
            hooks = toggle % 2 == 0
            _lib.set_profiling(hooks)
            enc.encode_device(ds.device_ptr, n, codes.data_ptr(), None)
            if hooks:
                calls, primary_ms, _ = _lib.profile_collect()
                assert calls == 1 and primary_ms > 0
                profiled += 1
        _lib.synchronize()
        after = _lib.event_pool_count()
        print(f"pool events before {before} after {after} profiled passes {profiled}")
        assert profiled == 100
        assert after <= before + 4
    finally:
        _lib.set_profiling(False)
        enc.close()
        ds.close()
