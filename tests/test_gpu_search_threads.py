"""The search handles under threads and streams: what include/vqhip.h ("Threading") promises, for vqhip_flat, vqhip_sqindex,
vqhip_binary, the ADC search of vqhip_pq_encoder, vqhip_ivfpq, vqhip_ivfflat, vqhip_ivfsq, vqhip_ivfbin and vqhip_range.

Every call goes through the handle classes of vq_amd._lib (ctypes releases the GIL: the calls really overlap), and every
result is compared bit for bit with the numpy statement tests/search_thread_cases.py computed for it before the threads
start: indices equal, distances equal as uint32, lims equal.  No tolerance.

The threads are plain daemon threads released by a barrier and joined with a time limit: a thread still inside the library
after it is a failure ("deadlock on handle ..."), never a hang.  Each thread stops at its first exception, which the main
thread re-raises with the kind, the variant, the thread and the iteration.  Nothing is tried twice."""
import threading
import time

import numpy as np
import pytest

import ref_filter as RF
import search_thread_cases as T
from vq_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
JOIN_S = 120.0
ALTERNATIONS = 10
# torch.cuda._sleep(cycles) of the blocker a thread queues in front of its `_device` call.  Measured on the MI355X with two
# events around it on the same stream: 48_000_000 cycles last 19.94 ms (21.03 ms on another card; 2_000_000: 0.84 ms,
# 4_000_000: 1.68 ms: the counter runs at about 2.4 GHz).  The ten alternations of two threads queue 0.4 s of blockers in all, and a case takes 0.2 s: the two
# threads' blockers run side by side.
SLEEP_CYCLES = 48_000_000
IVF_KINDS = tuple(k for k in T.KINDS if T.KINDS[k][0] in T.IVF)


class Stuck(AssertionError):
    """threads are still inside the library: the handle must not be destroyed under them"""


def run_threads(n, body, what, on_error=None):
    """body(t) on n daemon threads released together.  The first exception of a thread stops that thread (on_error() then
    frees the others from whatever they wait for); it is re-raised here.  A thread alive JOIN_S later is a failure."""
    start = threading.Barrier(n)
    errors = [None] * n

    def run(t):
        try:
            start.wait(JOIN_S)
            body(t)
        except BaseException as e:  # noqa: BLE001 - carried to the main thread
            errors[t] = e
            if on_error is not None:
                on_error()

    threads = [threading.Thread(target=run, args=(t,), daemon=True, name=f"{what}-{t}") for t in range(n)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + JOIN_S
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
    alive = [th.name for th in threads if th.is_alive()]
    for t, e in enumerate(errors):
        if e is not None and not alive:
            raise AssertionError(f"{what}: thread {t}: {e}") from e
    if alive:
        first = next((f"; thread {t} had failed: {e}" for t, e in enumerate(errors) if e is not None), "")
        raise Stuck(f"deadlock on handle {what}: {alive} still running after {JOIN_S:.0f} s{first}")


def guarded(handles, fn):
    """fn(), then close the handles -- unless threads are stuck inside them: then they are leaked"""
    try:
        fn()
    except Stuck:
        for h in handles:
            h.raw = None
        raise
    finally:
        for h in handles:
            h.close()


# -- a case's handle and its calls ----------------------------------------------------------------------------------------
def open_empty(c):
    d, o = c.data, c.opts
    if c.family == "ivfpq":
        return _lib.IVFPQ(d["coarse"], d["codebooks"], c.metric, _lib.IVF_RESIDUAL if o["residual"] else 0)
    if c.family == "ivfflat":
        return _lib.IVFFlat(d["coarse"], c.metric, np.dtype(o["dtype"]))
    if c.family == "ivfsq":
        return _lib.IVFSQ(d["coarse"], T.SQ[0], T.SQ[1], T.SQ[2], c.metric)
    if c.family == "ivfbin":
        thr, low, high = o["bq"]
        return _lib.IVFBin(d["coarse"], thr, low, high, c.metric, o["coarse_metric"])
    raise ValueError(c.family)


def add_rows(c, ix, lo, hi, encode=False):
    """rows lo .. hi - 1 into an inverted-file handle; encode: as f32 rows the index encodes on the device, where it can"""
    d = c.data
    lists = d["lists"][lo:hi]
    if c.family == "ivfpq":
        ix.add(lists, d["pq_codes"][lo:hi])
    elif c.family == "ivfflat":
        ix.add(lists, d["stored"][lo:hi])
    elif c.family == "ivfsq":
        ix.add_rows(lists, d["rows"][lo:hi]) if encode else ix.add_codes(lists, d["sq_codes"][lo:hi])
    else:
        ix.add_rows(lists, d["rows"][lo:hi]) if encode else ix.add_packed(lists, d["words"][lo:hi])


def open_handle(c):
    d, o = c.data, c.opts
    if c.family == "flat":
        return _lib.Flat(np.ascontiguousarray(d["stored"]), c.metric)
    if c.family == "sqindex":
        return _lib.SQIndex(np.ascontiguousarray(d["sq_codes"]), False, T.N, T.D, T.SQ[0], T.SQ[1], T.SQ[2], c.metric)
    if c.family == "binary":
        thr, low, high = o["bq"]
        return _lib.Binary(np.ascontiguousarray(d["words"]), _lib.BINARY_PACKED, T.N, T.D, thr, low, high, c.metric)
    if c.family == "pq":
        enc = _lib.PQEncoder(d["codebooks"], c.metric)
        enc.adc_set_codes(d["pq_codes"])
        return enc
    ix = open_empty(c)
    add_rows(c, ix, 0, T.N)
    return ix


def mask_words(variants):
    """variant name -> the uint32 words of its row mask over all N rows (made before the threads start)"""
    return {v.name: RF.pack(v.mask) for v in variants if v.masked}


def read(r):
    try:
        return r.read()
    finally:
        r.close()


def call(c, h, v, words):
    """variant v through the host form of handle h: the arrays of its result"""
    q = c.queries(v)
    p = (v.nprobe,) if c.ivf else ()
    if v.op == "search":
        return h.adc_search(None, q, v.topk) if c.family == "pq" else h.search(q, *p, v.topk)
    if v.op == "search_codes":
        return h.adc_search(c.data["pq_codes"], q, v.topk)
    if v.op == "search_masked":
        return h.search_masked(q, *p, v.topk, words[v.name])
    if v.op == "range_search":
        return read(h.range_search(q, *p, v.radii, T.MAX_RESULTS))
    if v.op == "range_search_masked":
        return read(h.range_search_masked(q, *p, v.radii, T.MAX_RESULTS, words[v.name]))
    if v.op == "hamming_range_search":
        return read(h.hamming_range_search(q, *p, v.radii, T.MAX_RESULTS))
    if v.op == "rerank":
        return h.rerank(q, np.ascontiguousarray(v.cand), v.topk)
    if v.op == "probe":
        return (h.probe(q, v.nprobe),)
    raise ValueError(v.op)


def differs(got, want):
    """None, or where two results of one call first differ"""
    if len(got) != len(want):
        return f"{len(got)} arrays, not {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"array {k}: {g.dtype}{g.shape}, not {w.dtype}{w.shape}"
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == F else (g, w)
        bad = np.argwhere(gb != wb)
        if bad.size:
            at = tuple(bad[0])
            return f"array {k} at {at}: {gb[at]:#x}, not {wb[at]:#x} ({bad.shape[0]} elements differ)"
    return None


def check(got, want, what):
    bad = differs(got, want)
    assert bad is None, f"{what}: {bad}"


def checked_call(c, h, v, words, what):
    try:
        got = call(c, h, v, words)
    except Exception as e:  # noqa: BLE001 - an error return of a valid call is a finding
        raise AssertionError(f"{what}: {type(e).__name__}: {e}") from e
    check(got, v.want, what)


# -- 1. many threads, host forms, one handle ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(T.KINDS))
def test_eight_threads_on_one_handle(kind):
    """eight threads, thirty host-form calls each on ONE handle, neighbouring threads always in different variants (other
    queries, topk, nprobe, a mask or none, a range search, a rerank, a probe): every result is its statement's"""
    c = T.case(kind)
    words = mask_words(c.variants)
    sched = T.schedule(len(c.variants))
    h = open_handle(c)

    def body(t):
        for i, j in enumerate(sched[t]):
            v = c.variants[j]
            checked_call(c, h, v, words, f"{kind} {v.describe()} thread {t} iteration {i}")

    def run():
        checked_call(c, h, c.variants[0], words, f"{kind} warm call")  # the device state exists before the threads start
        run_threads(T.THREADS, body, kind)

    guarded([h], run)


# -- 2. the `_device` forms across streams ----------------------------------------------------------------------------------
class DeviceSide:
    """the two threads' queries, masks and one pair of zeroed output tensors per alternation, on the device"""

    def __init__(self, c, variants, rounds):
        import torch

        self.c, self.vs = c, variants
        dev = torch.device("cuda:0")
        self.q = [torch.from_numpy(c.queries(v).copy()).to(dev) for v in variants]
        self.mask = [torch.from_numpy(RF.pack(v.mask).view(np.int32).copy()).to(dev) if v.masked else None for v in variants]
        self.idx = [[torch.zeros((v.nq, v.topk), dtype=torch.int32, device=dev) for _ in range(rounds)] for v in variants]
        self.dist = [[torch.zeros((v.nq, v.topk), dtype=torch.float32, device=dev) for _ in range(rounds)] for v in variants]
        torch.cuda.synchronize()

    def call(self, h, t, j):
        v = self.vs[t]
        p = (v.nprobe,) if self.c.ivf else ()
        out = (self.idx[t][j].data_ptr(), self.dist[t][j].data_ptr())
        if v.masked:
            h.search_masked_device(self.q[t].data_ptr(), v.nq, *p, v.topk, self.mask[t].data_ptr(), *out)
        else:
            h.search_device(self.q[t].data_ptr(), v.nq, *p, v.topk, *out)

    def result(self, t, j):
        return self.idx[t][j].cpu().numpy().view(np.uint32), self.dist[t][j].cpu().numpy()


def alternate(kind, h, side, streams, rounds):
    """two threads in strict alternation on handle h, `rounds` `_device` calls each.  streams: each thread's own
    torch.cuda.Stream, set through vqhip_set_stream, with a blocker queued in front of every call -- or None: the
    library's per-thread streams.  Returns [thread][round] -> was the OTHER thread's stream still busy right after this
    thread's call returned (None where nothing had been queued there yet)."""
    import torch

    turn = [threading.Semaphore(1), threading.Semaphore(0)]
    stop = threading.Event()
    busy = [[None] * rounds for _ in range(2)]

    def body(t):
        if streams is not None:
            _lib.set_stream(streams[t].cuda_stream)
        for j in range(rounds):
            if not turn[t].acquire(timeout=JOIN_S / 2) or stop.is_set():
                if stop.is_set():
                    return
                raise AssertionError(f"{kind} thread {t} round {j}: the other thread never handed over")
            if streams is not None:
                with torch.cuda.stream(streams[t]):
                    torch.cuda._sleep(SLEEP_CYCLES)  # this thread's search is certainly still queued when the other enters
            try:
                side.call(h, t, j)
            except Exception as e:  # noqa: BLE001
                raise AssertionError(f"{kind} {side.vs[t].describe()} thread {t} round {j}: {type(e).__name__}: {e}") from e
            if streams is not None and (t, j) != (0, 0):
                busy[t][j] = not streams[1 - t].query()
            turn[1 - t].release()
        _lib.synchronize()

    def on_error():
        stop.set()
        for s in turn:
            s.release()

    run_threads(2, body, kind, on_error)
    torch.cuda.synchronize()
    return busy


def check_alternations(kind, side, rounds):
    for t, v in enumerate(side.vs):
        for j in range(rounds):
            check(side.result(t, j), v.want, f"{kind} {v.describe()} thread {t} round {j}")


DEVICE_PARAMS = [(k, False) for k in T.DEVICE_KINDS] + [("ivfflat_f16_cosine", True)]


@pytest.mark.parametrize("kind,masked", DEVICE_PARAMS, ids=[k + ("_masked" if m else "") for k, m in DEVICE_PARAMS])
def test_device_calls_on_the_callers_streams(kind, masked):
    """A `_device` search returns with its kernels queued on the calling thread's stream; the next call on the handle comes
    from another thread on another stream and reuses every workspace.  Each thread queues a blocker in front of its call,
    so its search has certainly not run when the other thread enters -- and the test verifies that premise: right after a
    thread's call returns, the other thread's stream must still be busy, else the case fails with "no overlap achieved".
    What keeps the results right is the wait the library queues (HandleSync::order, the event recorded when a call on a
    caller's stream leaves)."""
    import torch

    c = T.case(kind)
    side = DeviceSide(c, T.device_case(kind, masked), ALTERNATIONS + 1)
    h = open_handle(c)

    def run():
        for t in range(2):  # both shapes once: no call below allocates (an allocation waits for the device: no overlap)
            side.call(h, t, ALTERNATIONS)
        _lib.synchronize()
        torch.cuda.synchronize()
        for t, v in enumerate(side.vs):
            check(side.result(t, ALTERNATIONS), v.want, f"{kind} {v.describe()} warm call")
        streams = [torch.cuda.Stream() for _ in range(2)]
        busy = alternate(kind, h, side, streams, ALTERNATIONS)
        for t in range(2):
            for j in range(ALTERNATIONS):
                assert busy[t][j] is not False, f"{kind}: no overlap achieved (thread {t} round {j}: the other stream was idle)"
        assert sum(b is True for row in busy for b in row) == 2 * ALTERNATIONS - 1
        check_alternations(kind, side, ALTERNATIONS)

    guarded([h], run)


def test_device_calls_on_the_librarys_own_streams():
    """The same alternation without vqhip_set_stream: each thread's calls run on the stream the library made for it, and the
    event that orders the next thread behind them is recorded only when that thread shows up (HandleSync: tail_lazy).  No
    blocker can be queued on these streams and they cannot be queried from outside, so the overlap is by construction of
    the size and is NOT asserted: 100 000 rows of 64 dimensions and 4096 queries a call, which measured on the MI355X
    (events around the call on one stream) are 4.9 ms of device work behind a call that returns after 0.09 ms, against the
    tens of microseconds of the hand-over.  The 4096 queries of a thread are its 32 distinct ones 128 times over, so the
    statement is computed for 32 and tiled.  What is asserted: every output of every round is its statement's."""
    import ref_knn as K

    rng = np.random.default_rng(77)
    n, d, distinct, tiles, topks = 100_000, 64, 32, 128, (10, 33)
    nq = distinct * tiles
    X = rng.standard_normal((n, d)).astype(F)
    X[n - 5:] = X[:5]
    Q = rng.standard_normal((2 * distinct, d)).astype(F)
    Q[0], Q[distinct] = X[0], X[1]
    tiled = np.concatenate([np.tile(Q[t * distinct:(t + 1) * distinct], (tiles, 1)) for t in range(2)])
    c = T.Case("flat_100000x64", "flat", K.SQUARED_EUCLIDEAN, {"dtype": "float32"}, {"queries": tiled, "stored": X}, [])
    vs = [T.Variant(f"thread{t}", "search", nq, topks[t], q0=t * nq) for t in range(2)]
    for t, v in enumerate(vs):
        v.want = tuple(np.tile(a, (tiles, 1)) for a in K.search(c.metric, Q[t * distinct:(t + 1) * distinct], X, v.topk))
    side = DeviceSide(c, vs, ALTERNATIONS)
    h = _lib.Flat(X, c.metric)

    def run():
        alternate(c.kind, h, side, None, ALTERNATIONS)
        check_alternations(c.kind, side, ALTERNATIONS)

    guarded([h], run)


@pytest.mark.parametrize("kind", T.REGROW_KINDS)
def test_workspaces_regrown_behind_a_queued_device_search(kind):
    """Thread A queues a small `_device` search behind a blocker on its stream; thread B then makes a host call that is
    larger in every workspace the two share (130 queries, topk 1024, every list, a mask), so the handle frees and
    reallocates them while A's kernels have not run.  A's output is still A's statement, and B's result B's.  The premise
    -- A's stream busy when B enters -- is checked right before B's call (B's call ends the overlap itself: it waits)."""
    import torch

    c = T.case(kind)
    small, big = T.regrow_case(kind)
    words = mask_words([big])
    side = DeviceSide(c, [small], 2)
    stream = torch.cuda.Stream()
    h = open_handle(c)
    turn = [threading.Semaphore(1), threading.Semaphore(0)]
    seen = {}

    def body(t):
        if not turn[t].acquire(timeout=JOIN_S / 2):
            raise AssertionError(f"{kind}: thread {t} never got its turn")
        if t == 0:
            _lib.set_stream(stream.cuda_stream)
            with torch.cuda.stream(stream):
                torch.cuda._sleep(SLEEP_CYCLES)
            side.call(h, 0, 1)
            turn[1].release()
        else:
            seen["busy"] = not stream.query()
            checked_call(c, h, big, words, f"{kind} {big.describe()} behind the queued {small.describe()}")

    def run():
        side.call(h, 0, 0)  # the device state and the small call's workspaces exist; the big call's do not
        _lib.synchronize()
        torch.cuda.synchronize()
        check(side.result(0, 0), small.want, f"{kind} {small.describe()} warm call")
        run_threads(2, body, kind, lambda: [s.release() for s in turn])
        torch.cuda.synchronize()
        assert seen.get("busy") is True, f"{kind}: no overlap achieved (the small search had run before the large call entered)"
        check(side.result(0, 1), small.want, f"{kind} {small.describe()} with its workspaces regrown under it")

    guarded([h], run)


# -- 3. adds while searching ------------------------------------------------------------------------------------------------
SEARCHERS = 6


@pytest.mark.parametrize("kind", IVF_KINDS)
def test_adds_while_searching(kind):
    """One thread appends three uneven slices to an inverted-file handle while six threads search it without pause (the
    exact families: also a range search and a search under a mask of all N rows, whose bits past the index's current n
    the library ignores).  Every result equals the statement over ONE of the four prefixes; within a thread the prefix
    never goes back, and it is at least the one whose add had returned before the call started; list_sizes() is one of
    the four prefixes' too.  The adder starts a slice only after every searcher has made two more calls, and the
    searchers go on for two calls behind the last add: so the calls certainly spread over more than one prefix, which
    the test asserts."""
    a = T.add_case(kind)
    c = a.case
    words = mask_words(a.variants)
    nv = len(a.variants)
    mine = [a.variants[t % nv] for t in range(SEARCHERS)]
    ix = open_empty(c)
    cond = threading.Condition()
    calls = [0] * SEARCHERS
    state = {"adds": 0, "failed": False}
    matched = [[] for _ in range(SEARCHERS)]
    in_flight = [0]  # calls that saw an add return while they ran
    deadline = time.monotonic() + JOIN_S

    def adder():
        for s in range(3):
            with cond:
                target = [n + 2 for n in calls]
                ok = cond.wait_for(lambda: state["failed"] or all(n >= t for n, t in zip(calls, target)), timeout=JOIN_S / 2)
                if state["failed"]:
                    return
                assert ok, f"{kind}: the searchers made no progress before add {s}"
            add_rows(c, ix, T.PREFIXES[s], T.PREFIXES[s + 1], encode=(s == 1))
            with cond:
                state["adds"] = s + 1
                cond.notify_all()

    def searcher(t):
        v = mine[t]
        last, last_size, behind = 0, 0, 0
        i = 0
        while behind < 2:
            assert time.monotonic() < deadline, f"{kind} thread {t}: still searching after {JOIN_S:.0f} s"
            with cond:
                if state["failed"]:
                    return
                before = state["adds"]
            what = f"{kind} {v.describe()} thread {t} iteration {i}"
            try:
                got = call(c, ix, v, words)
                sizes = ix.list_sizes()
            except Exception as e:  # noqa: BLE001
                raise AssertionError(f"{what}: {type(e).__name__}: {e}") from e
            hit = [p for p in range(len(T.PREFIXES)) if T.same(got, v.want[p])]
            assert len(hit) == 1, f"{what}: equals the statement of {len(hit)} prefixes ({differs(got, v.want[max(before, last)])})"
            assert hit[0] >= last, f"{what}: prefix {hit[0]} behind prefix {last}"
            assert hit[0] >= before, f"{what}: prefix {hit[0]}, but add {before} had returned before the call"
            size = [p for p in range(len(T.PREFIXES)) if np.array_equal(sizes, a.sizes[p])]
            assert len(size) == 1 and int(sizes.sum()) == T.PREFIXES[size[0]], f"{what}: list_sizes() sums to {int(sizes.sum())}"
            assert size[0] >= max(last_size, hit[0]), f"{what}: list_sizes() of prefix {size[0]} behind a search of prefix {hit[0]}"
            last, last_size = hit[0], size[0]
            matched[t].append(last)
            with cond:
                calls[t] += 1
                if state["adds"] != before:
                    in_flight[0] += 1
                if before == 3:
                    behind += 1
                cond.notify_all()
            i += 1

    def body(t):
        adder() if t == SEARCHERS else searcher(t)

    def on_error():
        with cond:
            state["failed"] = True
            cond.notify_all()

    def run():
        add_rows(c, ix, 0, T.PREFIXES[0])
        check(call(c, ix, mine[0], words), mine[0].want[0], f"{kind} warm call")
        run_threads(SEARCHERS + 1, body, kind, on_error)
        every = [p for m in matched for p in m]
        spread = f"{len(every)} searches, per prefix {np.bincount(every, minlength=4).tolist()}, {in_flight[0]} beside an add"
        assert len(set(every)) > 1 and not all(p == 0 for p in every) and not all(p == 3 for p in every), f"no interleaving: {spread}"
        for t in range(SEARCHERS):
            assert matched[t][0] == 0 and matched[t][-1] == 3, f"{kind} thread {t}: prefixes {sorted(set(matched[t]))}"
        for v in a.variants:  # and with nothing beside it, the whole index
            check(call(c, ix, v, words), v.want[3], f"{kind} {v.describe()} after the threads")

    guarded([ix], run)


# -- 4. shared results and independent handles --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,variant", [("flat_f32_euclidean", "range"), ("binary_euclidean", "hamming_range")])
def test_one_range_result_read_by_eight_threads(kind, variant):
    """one vqhip_range from a `_device` range search, read by eight threads at once: lims, read() and the device pointers
    (copied down by each thread on its own stream) all give the statement"""
    import torch

    c = T.case(kind)
    v = next(x for x in c.variants if x.name == variant)
    qd = torch.from_numpy(c.queries(v).copy()).to("cuda:0")
    torch.cuda.synchronize()
    total = int(v.want[0][-1])
    handles = []  # the range result, then the index: whatever was made is closed

    def body(t):
        r = handles[0]
        for i in range(5):
            what = f"{kind} {v.describe()} thread {t} iteration {i}"
            assert (r.nq, r.total) == (v.nq, total), what
            assert np.array_equal(r.lims, v.want[0]), f"{what}: lims"
            check(r.read(), v.want, what)
            p_lims, p_idx, p_dist = r.device_pointers()
            assert p_lims and p_idx and p_dist, what
            lims = torch.zeros(v.nq + 1, dtype=torch.int64, device="cuda:0")
            idx = torch.zeros(total, dtype=torch.int32, device="cuda:0")
            dist = torch.zeros(total, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()  # (the zeros are torch's work, on torch's stream)
            _lib.memcpy_device(lims.data_ptr(), p_lims, 8 * (v.nq + 1))
            _lib.memcpy_device(idx.data_ptr(), p_idx, 4 * total)
            _lib.memcpy_device(dist.data_ptr(), p_dist, 4 * total)
            _lib.synchronize()
            got = (lims.cpu().numpy().view(np.uint64), idx.cpu().numpy().view(np.uint32), dist.cpu().numpy())
            check(got, v.want, f"{what}: through the device pointers")

    def run():
        h = open_handle(c)
        handles.append(h)
        fn = h.range_search_device if c.family == "flat" else h.hamming_range_search_device
        handles.insert(0, fn(qd.data_ptr(), v.nq, v.radii, T.MAX_RESULTS))
        run_threads(T.THREADS, body, kind)

    guarded(handles, run)


@pytest.mark.parametrize("kind", ["flat_f16_cosine", "ivfflat_f32_squared", "binary_euclidean"])
def test_eight_handles_on_eight_threads(kind):
    """distinct handles share nothing mutable: eight of one family, each created, searched (the inverted-file ones under
    masks too) and closed on its own thread over the same host arrays -- no launcher keeps a process-wide static"""
    c = T.case(kind)
    words = mask_words(c.variants)
    nv = len(c.variants)

    def body(t):
        h = open_handle(c)
        try:
            for i in range(nv):
                v = c.variants[(i + t) % nv]
                checked_call(c, h, v, words, f"{kind} {v.describe()} thread {t} call {i}")
        finally:
            h.close()

    run_threads(T.THREADS, body, kind)
