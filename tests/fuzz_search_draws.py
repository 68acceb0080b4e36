"""The draws of the search fuzz (tests/test_gpu_fuzz_search.py) and the statement each draw is held to.  No GPU here.

`draw(family, seed)` builds one case from np.random.default_rng seeded by (family, seed): the index kind and its constructor
arguments, the data, the queries and a list of operations to run in order.  The kind and the metric come from the seed
round-robin (every supported pair appears by construction); everything else is drawn.  A draw that would be an invalid call
(topk > rows so far, nprobe > nlist, ...) is clamped here, so a case is a valid call by construction.

`draw_filtered(family, seed)` is the same case under other ops, drawn from a generator of its own (draw's stream is
untouched; tests/golden/fuzz_search_draws_digests.json holds it): at least half of its query ops are the filtered searches,
range searches and reranks and the Hamming-radius range searches (NEW_OPS), every filtered op with a row mask over the rows
present at that op -- its kind one of MASK_KINDS, handed over in one of FORMS -- and some directly after close() or
save / load.

`statement_search`, `statement_range`, `statement_rerank` and `dense_statement`, and for the new ops
`statement_filtered_search`, `statement_filtered_range`, `statement_hamming_range` and their dense forms, dispatch a case to
the numpy statements of tests/ref_*.py.  They make no arithmetic of their own.
"""
import zlib
from dataclasses import dataclass

import numpy as np

import ref_binary as B
import ref_binary_filter as BF
import ref_binary_range as BR
import ref_filter as RF
import ref_ivf as I
import ref_ivf_filter as RIF
import ref_ivf_range as IRG
import ref_ivf_residual as IRES
import ref_ivfbin as IB
import ref_ivfflat as IFL
import ref_ivfsq as ISQ
import ref_knn as K
import ref_pq_filter as RPF
import ref_range as RG
import ref_sqbq as S
import ref_sqindex as SI
from test_gpu_fuzz import KINDS, _draw_data

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
ALL5 = (0, 1, 2, 3, 4)
SUMS = (0, 1, 2)  # the metrics with an ADC / Hamming form: no cosine

# seeds per family at VQ_FUZZ_SCALE=1 (tests/test_fuzz_search_draws.py holds the coverage these give)
N_FAMILY = {"flat": 24, "scalar": 16, "binary": 16, "pq": 16, "ivfpq": 16, "ivfflat": 24, "ivfsq": 16, "ivfbin": 16}
FAMILIES = tuple(N_FAMILY)
DENSE = ("flat", "scalar", "binary", "pq")  # every row is a candidate of every query
IVF = ("ivfpq", "ivfflat", "ivfsq", "ivfbin")
PAIRS = {
    "flat": [(k, m) for m in ALL5 for k in ("flat_f32", "flat_f16")],
    "scalar": [("scalar", m) for m in ALL5],
    "binary": [("binary", m) for m in SUMS],
    "pq": [("pq", m) for m in SUMS],
    "ivfpq": [(k, m) for m in SUMS for k in ("ivfpq", "ivfpq_residual")],
    "ivfflat": [(k, m) for m in ALL5 for k in ("ivfflat_f32", "ivfflat_f16")],
    "ivfsq": [("ivfsq", m) for m in ALL5],
    "ivfbin": [("ivfbin", m) for m in SUMS],
}
# the operations after the rows are in (an IVF family also draws "add")
QUERY_OPS = {
    "flat": ("search", "range_search"),
    "scalar": ("search", "range_search", "save_load_search"),
    "binary": ("search", "rerank_search", "save_load_search"),
    "pq": ("search", "rerank_search", "save_load_search"),
    "ivfpq": ("search", "close_search", "save_load_search", "rerank_search"),
    "ivfflat": ("search", "range_search", "close_search", "save_load_search"),
    "ivfsq": ("search", "range_search", "close_search", "save_load_search"),
    "ivfbin": ("search", "close_search", "save_load_search", "rerank_search"),
}
NQ = (1, 3, 17, 40, 130)
FLAT_DIMS = (1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 36, 64, 100, 127, 128, 129, 200)
BINARY_DIMS = (1, 31, 32, 33, 64, 65, 96, 128, 192, 1056)
RESIDUAL_TABLE_BUDGET = 150_000  # nq * probed lists with rows * dim: the residual statement builds one table per pair


@dataclass
class Case:
    family: str
    seed: int
    kind: str
    metric: int
    coarse_metric: int  # the metric lists are probed under (IVFBinaryIndex: drawn; the other IVF kinds: `metric`)
    data_kind: str
    dense_cut: bool     # every row equal but a few: the cut of the selection holds more than 8192 positions
    n: int
    dim: int
    nlist: int
    nprobe: int
    topk: int
    nq: int
    ctor: dict          # constructor arguments beyond the metric: dtype, sq, bq, residual, source
    data: dict          # the arrays: rows as drawn, as stored, list ids, coarse centroids, codebooks, codes, words
    queries: np.ndarray
    ops: list           # dicts {"op": name, "n": rows in the index after it, ...}, run in order

    def describe(self, upto=None) -> str:
        """the whole case in one line: a red seed replays from it"""
        ops = self.ops if upto is None else self.ops[:upto + 1]
        c = " ".join(f"{k}={v}" for k, v in sorted(self.ctor.items()))
        return (f"family={self.family} seed={self.seed} kind={self.kind} metric={NAMES[self.metric]} "
                f"coarse_metric={NAMES[self.coarse_metric]} data={self.data_kind} dense_cut={self.dense_cut} n={self.n} "
                f"dim={self.dim} nlist={self.nlist} nprobe={self.nprobe} topk={self.topk} nq={self.nq} {c} "
                f"ops=[{', '.join(_op_text(o) for o in ops)}]")


def _op_text(o) -> str:
    if o["op"] == "add":
        return f"{o['how']}[{o['lo']}:{o['n']}]"
    extra = "".join(f" {k}={o[k]}" for k in ("candidates", "flat_metric") if k in o)
    if "mask" in o:  # a filtered op: the mask's kind, the form it is handed over in and the number of allowed rows
        extra += f" mask={o['mask_kind']} form={o['form']} allowed={o['allowed']}"
    extra += "".join(f" {k}" for k in ("after_close", "after_load") if o.get(k))
    return f"{o['op']}(n={o['n']} topk={o['topk']}{extra})" if "topk" in o else f"{o['op']}(n={o['n']}{extra})"


def seeds(family, scale=1):
    return range(N_FAMILY[family] * scale)


# -- pieces of a draw -------------------------------------------------------------------------------------------------------
def _draw_n(rng) -> int:
    return int(rng.choice([1, int(rng.integers(2, 70)), int(rng.integers(70, 1100)), int(rng.integers(1100, 3000))],
                          p=[0.06, 0.22, 0.36, 0.36]))


def _plant(rng, X, lists=None):
    """the special rows of ref_knn.special_rows, and duplicates (in the same list: ties go to the lower row id)"""
    n, d = X.shape
    if n >= 16 and rng.random() < 0.5:
        X[7:15] = K.special_rows(d, rng)
    if n >= 14:
        X[n - 7:] = X[:7]
        if lists is not None:
            lists[n - 7:] = lists[:7]
    elif n >= 2:
        X[n - 1] = X[0]
        if lists is not None:
            lists[n - 1] = lists[0]


def _draw_lists(rng, n, nlist, max_live):
    """list ids in an order unrelated to the rows'; with nlist >= 2 mostly at least one list without rows"""
    if nlist >= 2 and rng.random() < 0.75:
        nlive = int(rng.integers(1, nlist))
    else:
        nlive = nlist
    live = rng.permutation(nlist)[:min(nlive, max_live)]
    return live[rng.integers(0, live.size, n)].astype(np.uint32)


def _draw_queries(rng, nq, dim, kind, row, coarse=None, lists=None):
    Q = _draw_data(rng, nq, dim, kind if rng.random() < 0.7 else "normal")
    Q[0] = row                       # equal to a row (one with a duplicate)
    if nq >= 3:
        Q[1] = 0.0                   # the zero vector
        Q[2, dim // 2] = np.nan      # a NaN element
    if nq >= 17 and coarse is not None:
        empty = np.flatnonzero(np.bincount(lists, minlength=coarse.shape[0]) == 0)
        if empty.size:
            Q[3] = coarse[empty[int(rng.integers(0, empty.size))]]  # the centroid of a list without rows
    return np.ascontiguousarray(Q, F)


def _query_op(rng, case, qops, n_now):
    o = {"op": str(rng.choice(qops)), "n": n_now, "topk": min(case.topk, n_now)}
    if o["op"] == "range_search":
        del o["topk"]
        o["radius"] = _draw_radius(rng, case, n_now)
    if o["op"] == "rerank_search":
        _draw_rerank(rng, o, n_now)
    return o


def _draw_rerank(rng, o, n_now):
    t = o["topk"]
    cap = min(n_now, 1024)
    o["candidates"] = int(rng.choice([t, min(4 * t, cap), int(rng.integers(t, cap + 1))]))
    o["flat_metric"] = int(rng.integers(0, 5))


def _draw_ops(rng, case):
    """3 to 7 operations; an IVF family adds its rows in 1 to 3 uneven slices with queries between"""
    fam, n = case.family, case.n
    qops = QUERY_OPS[fam]
    ops = []

    if fam in IVF:
        pieces = min(n, int(rng.choice([1, 2, 3])))
        cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, n), pieces - 1, replace=False)) + [n]
        for i in range(pieces):
            ops.append({"op": "add", "lo": cuts[i], "n": cuts[i + 1], "how": str(rng.choice(case.ctor["adds"]))})
            if i + 1 < pieces and rng.random() < 0.7:
                ops.append(_query_op(rng, case, qops, cuts[i + 1]))
        room = 7 - len(ops)
        for _ in range(max(3 - len(ops), int(rng.integers(1, room + 1)))):
            ops.append(_query_op(rng, case, qops, n))
    else:
        for _ in range(int(rng.integers(3, 8))):
            ops.append(_query_op(rng, case, qops, n))
    return ops


def _draw_radius(rng, case, n_now):
    """per-query radii from the case's own k-th distances (ref_range.kth_distance), so that the hits are neither none nor
    all; query 0 (equal to a duplicated row) gets its 2nd distance: an exact tie on the boundary; the last query -1; with
    17 queries or more, the one before it +inf"""
    X = decoded(case)[:n_now]
    nq = case.nq
    k = int(rng.integers(1, min(n_now, 40) + 1))
    r = RG.kth_distance(case.metric, case.queries, X, k)
    r[0] = RG.kth_distance(case.metric, case.queries[:1], X, min(2, n_now))[0]
    r[np.isnan(r)] = F(1.0)  # (a NaN radius is refused)
    if nq >= 2:
        r[-1] = F(-1.0)
    if nq >= 17:
        r[-2] = np.inf
    return r.astype(F)


def decoded(case) -> np.ndarray:
    """the f32 rows the exact statements see: f16 rows widened, SQ codes decoded"""
    d = case.data
    if case.family in ("flat", "ivfflat"):
        return d["stored"].astype(F)
    if case.family in ("scalar", "ivfsq"):
        return SI.decode(case.ctor["sq"], d["codes"])
    raise ValueError(case.family)


# -- the draw ---------------------------------------------------------------------------------------------------------------
def draw(family: str, seed: int) -> Case:
    rng = np.random.default_rng([zlib.crc32(family.encode()), int(seed)])
    pairs = PAIRS[family]
    kind, metric = pairs[seed % len(pairs)]
    nfam = N_FAMILY[family]
    dense_cut = family in DENSE and seed % nfam >= nfam - 2
    ivf = family in IVF
    data_kind = KINDS[int(rng.integers(0, len(KINDS)))]
    nq = int(rng.choice(NQ))
    n = _draw_n(rng)
    ctor, data = {}, {}

    # dimensions
    if family in ("pq", "ivfpq"):
        m = int(rng.choice([1, 2, 3, 4, 8, 16]))
        sd = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 32]))
        k = int(rng.choice([1, 2, 16, 64, 100, 255, 256, 300, 300]))
        if rng.random() < 0.08:
            m, k, sd = 128, 300, 1  # m * k = 38400: the ADC table limit
        if dense_cut:
            k = max(k, 2)
        dim = m * sd
        ctor.update(m=m, k=k, sub_dim=sd)
    elif family in ("binary", "ivfbin"):
        dim = int(rng.choice(BINARY_DIMS)) if rng.random() < 0.5 else int(rng.integers(1, 1101))
    else:
        dim = int(rng.choice(FLAT_DIMS)) if rng.random() < 0.5 else int(rng.integers(1, 201))
    if dense_cut:
        n = int(rng.integers(8193, 9001))
        nq = int(rng.choice([1, 3]))
        if family not in ("pq",):
            dim = min(dim, 130)

    # lists
    nlist, nprobe, coarse_metric = 1, 1, metric
    if ivf:
        nlist = int(rng.choice([1, 2, 7, int(rng.integers(2, 40)), int(rng.integers(40, 301)),
                                min(300, n + int(rng.integers(1, 50)))]))
        nprobe = min(int(rng.choice([1, int(rng.integers(1, min(nlist, 8) + 1)), nlist])), nlist, 1024)
        if family == "ivfbin":
            coarse_metric = int(rng.integers(0, 5))
        max_live = nlist
        if kind == "ivfpq_residual":
            max_live = max(1, RESIDUAL_TABLE_BUDGET // (nq * dim))
        lists = _draw_lists(rng, n, nlist, max_live)
        data["lists"] = lists
    topk = min(int(rng.choice([1, 10, int(rng.integers(1, 301)), min(n, 1024)])), n, 1024)
    if dense_cut:
        topk = int(rng.choice([1, 10, 1024]))

    # rows
    if family in ("pq", "ivfpq"):
        cb = _draw_data(rng, m * k, sd, data_kind).reshape(m, k, sd)
        if rng.random() < 0.3 and k > 3:
            cb[:, k - 1] = cb[:, 0]  # duplicate centroid: equal distances
        codes = rng.integers(0, k, (n, m)).astype(np.uint8 if k <= 256 else np.uint16)
        if dense_cut:
            codes[:] = 0
            cb[0, k - 1, 0] = np.nan  # "NaN rows": a few rows hold a code whose centroid has a NaN
            codes[rng.integers(0, n, 3), 0] = k - 1
        elif n >= 14:
            codes[n - 7:] = codes[:7]
            if ivf:
                lists[n - 7:] = lists[:7]
        elif n >= 2:
            codes[n - 1] = codes[0]
            if ivf:
                lists[n - 1] = lists[0]
        data["codebooks"] = np.ascontiguousarray(cb, F)
        data["codes"] = codes
        data["rerank_rows"] = _draw_data(rng, n, dim, "normal")  # the exact index of rerank=: any rows of the same shape
        row0 = np.concatenate([cb[s][codes[0, s]] for s in range(m)])
        if ivf:
            data["coarse"] = np.ascontiguousarray(_draw_data(rng, nlist, dim, data_kind), F)
            ctor.update(residual=kind == "ivfpq_residual", adds=("add_codes",))
    else:
        X = _draw_data(rng, n, dim, data_kind)
        if dense_cut:
            X[:] = X[0]
            X[rng.integers(0, n, 3)] = np.nan
        else:
            _plant(rng, X, data.get("lists"))
        X = np.ascontiguousarray(X, F)
        data["rows"] = X
        row0 = X[0]
        if ivf:
            if n >= nlist and rng.random() < 0.5:
                coarse = X[rng.choice(n, nlist, replace=False)].copy()  # centroids drawn from the rows: zero distances
            else:
                coarse = _draw_data(rng, nlist, dim, data_kind)
            data["coarse"] = np.ascontiguousarray(coarse, F)
        if family in ("flat", "ivfflat"):
            dtype = np.float16 if kind.endswith("f16") else np.float32
            with np.errstate(over="ignore"):
                data["stored"] = X.astype(dtype)
            ctor.update(dtype=np.dtype(dtype).name)
            if ivf:
                ctor.update(adds=("add_rows",))
            row0 = data["stored"][0].astype(F)
        elif family in ("scalar", "ivfsq"):
            sq = SI.QUANTIZERS[int(rng.integers(0, len(SI.QUANTIZERS)))]
            source = str(rng.choice(["rows", "codes"]))
            codes = S.sq_encode(sq[0], sq[1], sq[2], X)
            if source == "codes" and not dense_cut and n >= 16:
                at = rng.integers(7, n - 7, 5)
                codes[at] = rng.integers(0, 256, (5, dim)).astype(np.uint8)  # every byte value is legal (codes >= levels too)
            data["codes"] = codes
            ctor.update(sq=sq, source=source)
            if ivf:
                ctor.update(adds=("add_codes",) if source == "codes" else ("add_rows", "add_codes"))
        else:  # binary, ivfbin
            low, high = IB.LOW_HIGH[int(rng.integers(0, len(IB.LOW_HIGH)))]
            thr = float(rng.choice([0.0, -0.5, 0.25, float(X[int(rng.integers(0, n)), int(rng.integers(0, dim))])]))
            thr = float(F(thr)) if np.isfinite(thr) else 0.0
            data["words"] = B.pack(B.bits_f32(X, thr))
            data["bq_codes"] = S.bq_encode(thr, low, high, X)
            ctor.update(bq=(thr, low, high))
            if ivf:
                ctor.update(adds=("add_packed", "add_codes", "add_rows"))
            else:
                ctor.update(source=str(rng.choice(["rows", "codes", "packed"])))

    Q = _draw_queries(rng, nq, dim, data_kind, row0, data.get("coarse"), data.get("lists"))
    case = Case(family, int(seed), kind, metric, coarse_metric, data_kind, dense_cut, n, dim, nlist, nprobe, topk, nq, ctor,
                data, Q, [])
    case.ops = _draw_ops(rng, case)
    return case


# -- the statement a case is held to ------------------------------------------------------------------------------------------
def statement_search(case: Case, n: int, topk: int):
    """(idx uint32 (nq, topk), dist f32 (nq, topk)) of case.queries over the first n rows at the case's nprobe"""
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    fam = case.family
    if fam == "flat":
        return K.search(metric, Q, d["stored"][:n].astype(F), topk)
    if fam == "scalar":
        return SI.search(metric, Q, c["sq"], d["codes"][:n], topk)
    if fam == "binary":
        thr, low, high = c["bq"]
        return B.search(B.pack(B.bits_f32(Q, thr)), d["words"][:n], case.dim, low, high, metric, topk)
    if fam == "pq":  # the ADC full pass: the inverted-file statement with one list, probed
        return I.brute_search(metric, np.zeros((1, case.dim), F), d["codebooks"], np.zeros(n, np.uint32), d["codes"][:n], Q, 1, topk)
    if fam == "ivfpq":
        ref = IRES if c["residual"] else I
        return ref.brute_search(metric, d["coarse"], d["codebooks"], d["lists"][:n], d["codes"][:n], Q, case.nprobe, topk)
    if fam == "ivfflat":
        return IFL.search(metric, d["coarse"], d["lists"][:n], d["stored"][:n], Q, case.nprobe, topk)
    if fam == "ivfsq":
        return ISQ.search(metric, d["coarse"], d["lists"][:n], c["sq"], d["codes"][:n], Q, case.nprobe, topk)
    if fam == "ivfbin":
        return IB.search(metric, case.coarse_metric, d["coarse"], d["lists"][:n], c["bq"], d["words"][:n], case.dim, Q,
                         case.nprobe, topk)
    raise ValueError(fam)


def dense_statement(case: Case, n: int, topk: int):
    """the statement of the resident index over the same first n rows: an IVF case's own at nprobe == nlist"""
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    if case.family == "ivfflat":
        return K.search(metric, Q, d["stored"][:n].astype(F), topk)
    if case.family == "ivfsq":
        return SI.search(metric, Q, c["sq"], d["codes"][:n], topk)
    if case.family == "ivfbin":
        thr, low, high = c["bq"]
        return B.search(B.pack(B.bits_f32(Q, thr)), d["words"][:n], case.dim, low, high, metric, topk)
    raise ValueError(case.family)


def statement_range(case: Case, n: int, radius):
    """(lims, idx, dist) of a range search over the first n rows at the case's nprobe"""
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    if case.family == "flat":
        return RG.search(metric, Q, d["stored"][:n].astype(F), radius)
    if case.family == "scalar":
        return RG.sq_search(metric, Q, c["sq"], d["codes"][:n], radius)
    if case.family == "ivfflat":
        return IRG.search(metric, d["coarse"], d["lists"][:n], d["stored"][:n], Q, case.nprobe, radius)
    if case.family == "ivfsq":
        return IRG.sq_search(metric, d["coarse"], d["lists"][:n], c["sq"], d["codes"][:n], Q, case.nprobe, radius)
    raise ValueError(case.family)


def dense_statement_range(case: Case, n: int, radius):
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    if case.family == "ivfflat":
        return RG.search(metric, Q, d["stored"][:n].astype(F), radius)
    if case.family == "ivfsq":
        return RG.sq_search(metric, Q, c["sq"], d["codes"][:n], radius)
    raise ValueError(case.family)


def rerank_rows(case: Case, n: int) -> np.ndarray:
    """the f32 rows of the exact index a rerank_search goes through"""
    return (case.data["rows"] if case.family in ("binary", "ivfbin", "ivfsq") else case.data["rerank_rows"])[:n]


def statement_rerank(case: Case, n: int, hits, topk: int, flat_metric: int):
    """the exact rerank (ref_knn.rerank) of each query's real hits, padded as the index pads"""
    X = rerank_rows(case, n)
    Q = case.queries
    idx = np.full((Q.shape[0], topk), I.PAD_ID, np.uint32)
    dist = np.full((Q.shape[0], topk), np.inf, F)
    for j in range(Q.shape[0]):
        real = hits[j][hits[j] != I.PAD_ID]
        t = min(topk, real.size)
        if t:
            ii, dd = K.rerank(flat_metric, Q[j:j + 1], X, real[None, :], t)
            idx[j, :t], dist[j, :t] = ii[0], dd[0]
    return idx, dist


def probed_rows(case: Case, n: int) -> np.ndarray:
    """(nq,) the number of rows in each query's probed lists, over the first n rows"""
    lists = case.data["lists"][:n]
    P = I.probe(case.coarse_metric, case.data["coarse"], case.queries, case.nprobe)
    sizes = np.bincount(lists, minlength=case.nlist)
    return sizes[P.astype(np.int64)].sum(axis=1)


# -- the second draw: the filtered and the Hamming-range calls ----------------------------------------------------------------
FILTER_WORD = 0x46494C54  # the third seed word of draw_filtered's generator: draw()'s own stream never sees it
NEW_OPS = {
    "flat": ("filtered_search", "filtered_range_search"),
    "scalar": ("filtered_search", "filtered_range_search"),
    "binary": ("hamming_range_search", "filtered_search", "filtered_hamming_range_search", "filtered_rerank_search"),
    "pq": ("filtered_search", "filtered_rerank_search"),
    "ivfpq": ("filtered_search", "filtered_rerank_search"),
    "ivfflat": ("filtered_search", "filtered_range_search"),
    "ivfsq": ("filtered_search", "filtered_range_search", "filtered_rerank_search"),
    "ivfbin": ("hamming_range_search", "filtered_search", "filtered_hamming_range_search", "filtered_rerank_search"),
}
FILTERED = ("filtered_search", "filtered_range_search", "filtered_hamming_range_search", "filtered_rerank_search")
MASK_KINDS = ("ones", "zeros", "one_row", "random", "block64", "block", "all_but_few", "fewer_than_topk", "without_winners",
              "higher_twins")
RARE_KINDS = ("fewer_than_topk", "higher_twins", "one_list")  # not on every op: topk >= 2, the whole set, an IVF family
FORMS = ("bool", "words", "ids", "words_tail")
HAS_SAVE = tuple(f for f in FAMILIES if "save_load_search" in QUERY_OPS[f])


def mask_kinds(family):
    return MASK_KINDS + (("one_list",) if family in IVF else ())


def _applies(case, kind, n_now, topk) -> bool:
    if kind == "fewer_than_topk":
        return topk >= 2
    if kind == "higher_twins":  # the duplicates _plant / the code rows make sit at the end of the whole set
        return n_now == case.n >= 2 and not case.dense_cut
    return True


def _draw_mask(rng, case, kind, n_now, topk) -> np.ndarray:
    """bool (n_now,): the allowed rows of one filtered op"""
    m = np.zeros(n_now, np.bool_)
    if kind == "ones":
        m[:] = True
    elif kind == "one_row":
        m[int(rng.choice([0, n_now - 1, int(rng.integers(0, n_now))]))] = True
    elif kind == "random":
        m = rng.random(n_now) < min(1.0, float(rng.choice([0.5, 0.03, 3 / n_now])))
    elif kind == "block64":  # a run of whole 64-row groups (the last one as far as the rows go)
        groups = (n_now + 63) // 64
        a = int(rng.integers(0, groups))
        m[64 * a:min(64 * int(rng.integers(a + 1, groups + 1)), n_now)] = True
    elif kind == "block":
        lo = int(rng.integers(0, n_now))
        m[lo:int(rng.integers(lo + 1, n_now + 1))] = True
    elif kind == "all_but_few":
        few = int(rng.integers(1, 6))
        if case.dense_cut:  # all but three rows are tied: more than 8192 of them stay allowed
            few = min(few, max(1, case.n - 3 - 8193))
        m[:] = True
        m[rng.choice(n_now, min(few, n_now), replace=False)] = False
    elif kind == "fewer_than_topk":
        m[rng.choice(n_now, int(rng.integers(1, topk)), replace=False)] = True
    elif kind == "without_winners":  # a kernel that ignored the mask would return exactly the rows left out
        winners = statement_search(case, n_now, min(topk, 4))[0]
        m[:] = True
        m[winners[winners != I.PAD_ID].astype(np.int64)] = False
    elif kind == "higher_twins":  # of every duplicate pair only the higher id: the distance bits stay, the id changes
        m[:] = True
        m[:7 if n_now >= 14 else 1] = False
    elif kind == "one_list":
        lists = case.data["lists"][:n_now]
        live = np.unique(lists)
        P = I.probe(case.coarse_metric, case.data["coarse"], case.queries, case.nprobe)
        probing = np.array([int((P == l).any(axis=1).sum()) for l in live])  # the queries that probe each list with rows
        some = live[(probing > 0) & (probing < case.nq)]
        if some.size and rng.random() < 0.75:  # probed by some queries only: the others come back all padding
            live = some
        m = lists == live[int(rng.integers(0, live.size))]
    elif kind != "zeros":
        raise ValueError(kind)
    return m


def _draw_hamming_radius(rng, case, n_now):
    """per-query integer radii from the case's own k-th Hamming distances; query 0 (equal to a duplicated row) gets 0: the
    exact bit match and its duplicate; the last query `dim`: every row; with 17 queries or more, the one before it dim + 7"""
    H = B.hamming(B.pack(B.bits_f32(case.queries, case.ctor["bq"][0])), case.data["words"][:n_now])
    k = int(rng.integers(1, min(n_now, 40) + 1))
    r = np.sort(H, axis=1)[:, k - 1].astype(np.int64)
    r[0] = 0
    if case.nq >= 2:
        r[-1] = case.dim
    if case.nq >= 17:
        r[-2] = case.dim + 7
    return r


def _new_op(rng, case, name, n_now, nth):
    """one of NEW_OPS over the first n_now rows; nth: how many filtered ops the case holds already -- the first two take
    their mask kind round-robin from the seed, a dense-cut case the two kinds that reach the dense cut"""
    fam, seed = case.family, case.seed
    topk = min(case.topk, n_now)
    o = {"op": name, "n": n_now}
    if name in ("filtered_search", "filtered_rerank_search"):
        o["topk"] = topk
    if name == "filtered_rerank_search":
        _draw_rerank(rng, o, n_now)
    if name == "filtered_range_search":
        o["radius"] = _draw_radius(rng, case, n_now)
    if name.endswith("hamming_range_search"):
        o["hradius"] = _draw_hamming_radius(rng, case, n_now)
    if name not in FILTERED:
        return o
    kinds = mask_kinds(fam)
    if case.dense_cut and nth < 2:
        kind = ("all_but_few", ("without_winners", "random")[seed % 2])[nth]
    elif nth < 2:
        kind = kinds[(2 * seed + nth) % len(kinds)]
    else:  # (the kinds that do not always apply are drawn more often where they do)
        w = np.array([3.0 if k in RARE_KINDS else 1.0 for k in kinds])
        kind = str(rng.choice(kinds, p=w / w.sum()))
    if not _applies(case, kind, n_now, topk):
        rare = [k for k in RARE_KINDS if k in kinds]
        rare = rare[seed % len(rare):] + rare[:seed % len(rare)]
        kind = next(k for k in rare + ["ones"] if _applies(case, k, n_now, topk))
    mask = _draw_mask(rng, case, kind, n_now, topk)
    o.update(mask_kind=kind, form=str(rng.choice(FORMS)), mask=mask, allowed=int(mask.sum()))
    if o["form"] == "ids":
        o["ids"] = rng.permutation(np.flatnonzero(mask)).astype(np.int64)
    close = fam in IVF and (rng.random() < 0.12 or (nth == 0 and seed % 4 == 1))
    load = fam in HAS_SAVE and (rng.random() < 0.12 or (nth == 0 and seed % 4 == 3))
    if close:
        o["after_close"] = True  # close() directly before: the filtered call is the first the fresh handle sees
    elif load:
        o["after_load"] = True   # save / load directly before: the filtered call goes to the loaded index, its first
    return o


def _draw_filtered_ops(rng, case):
    """the length rules of _draw_ops; at least half of the query ops are NEW_OPS, the others the family's QUERY_OPS"""
    fam, n, seed = case.family, case.n, case.seed
    shape = []  # an add, or the number of rows a query op sees
    if fam in IVF:
        pieces = min(n, int(rng.choice([1, 2, 3])))
        cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, n), pieces - 1, replace=False)) + [n]
        for i in range(pieces):
            shape.append({"op": "add", "lo": cuts[i], "n": cuts[i + 1], "how": str(rng.choice(case.ctor["adds"]))})
            if i + 1 < pieces and rng.random() < 0.7:
                shape.append(cuts[i + 1])
        room = 7 - len(shape)
        shape += [n] * max(3 - len(shape), int(rng.integers(1, room + 1)))
    else:
        shape = [n] * int(rng.integers(3, 8))
    slots = [i for i, s in enumerate(shape) if not isinstance(s, dict)]
    new = {int(i) for i in rng.choice(slots, int(rng.integers((len(slots) + 1) // 2, len(slots) + 1)), replace=False)}
    ops, nth_new, nth_filtered = [], 0, 0
    for i, s in enumerate(shape):
        if isinstance(s, dict):
            ops.append(s)
        elif i not in new:
            ops.append(_query_op(rng, case, QUERY_OPS[fam], s))
        else:
            names = NEW_OPS[fam]
            name = names[seed % len(names)] if nth_new == 0 else str(rng.choice(names))
            if case.dense_cut and nth_filtered < 2 and name not in FILTERED:
                name = "filtered_search"
            ops.append(_new_op(rng, case, name, s, nth_filtered))
            nth_new += 1
            nth_filtered += name in FILTERED
    return ops


def draw_filtered(family: str, seed: int) -> Case:
    """draw(family, seed) with its ops replaced: the same index, rows and queries under the filtered and the Hamming-range
    calls, every filtered op with a mask of its own over the rows present at that op"""
    case = draw(family, seed)
    rng = np.random.default_rng([zlib.crc32(family.encode()), int(seed), FILTER_WORD])
    case.ops = _draw_filtered_ops(rng, case)
    return case


# -- the statement a filtered op is held to -----------------------------------------------------------------------------------
def _qwords(case):
    return B.pack(B.bits_f32(case.queries, case.ctor["bq"][0]))


def statement_filtered_search(case: Case, n: int, topk: int, mask):
    """statement_search among the allowed rows: mask bool (n,)"""
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    fam = case.family
    if fam == "flat":
        return RF.search(metric, Q, d["stored"][:n].astype(F), topk, mask)
    if fam == "scalar":
        return RF.sq_search(metric, Q, c["sq"], d["codes"][:n], topk, mask)
    if fam == "binary":
        thr, low, high = c["bq"]
        return BF.search(_qwords(case), d["words"][:n], case.dim, low, high, metric, topk, mask)
    if fam == "pq":
        return RPF.brute_dense_search(metric, d["codebooks"], d["codes"][:n], Q, topk, mask)
    if fam == "ivfpq":
        ref = RPF.brute_residual_search if c["residual"] else RPF.brute_search
        return ref(metric, d["coarse"], d["codebooks"], d["lists"][:n], d["codes"][:n], Q, case.nprobe, topk, mask)
    if fam == "ivfflat":
        return RIF.search(metric, d["coarse"], d["lists"][:n], d["stored"][:n], Q, case.nprobe, topk, mask)
    if fam == "ivfsq":
        return RIF.sq_search(metric, d["coarse"], d["lists"][:n], c["sq"], d["codes"][:n], Q, case.nprobe, topk, mask)
    if fam == "ivfbin":
        return BF.ivf_search(metric, case.coarse_metric, d["coarse"], d["lists"][:n], c["bq"], d["words"][:n], case.dim, Q,
                             case.nprobe, topk, mask)
    raise ValueError(fam)


def dense_statement_filtered(case: Case, n: int, topk: int, mask):
    """the filtered statement of the resident index over the same first n rows: an IVF case's own at nprobe == nlist
    (None for the residual IVFPQ index, which has no resident twin)"""
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    if case.family == "ivfflat":
        return RF.search(metric, Q, d["stored"][:n].astype(F), topk, mask)
    if case.family == "ivfsq":
        return RF.sq_search(metric, Q, c["sq"], d["codes"][:n], topk, mask)
    if case.family == "ivfbin":
        thr, low, high = c["bq"]
        return BF.search(_qwords(case), d["words"][:n], case.dim, low, high, metric, topk, mask)
    if case.family == "ivfpq":
        return None if c["residual"] else RPF.brute_dense_search(metric, d["codebooks"], d["codes"][:n], Q, topk, mask)
    raise ValueError(case.family)


def statement_filtered_range(case: Case, n: int, radius, mask):
    """statement_range in which only allowed rows hit"""
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    if case.family == "flat":
        return RF.range_search(metric, Q, d["stored"][:n].astype(F), radius, mask)
    if case.family == "scalar":
        return RF.sq_range_search(metric, Q, c["sq"], d["codes"][:n], radius, mask)
    if case.family == "ivfflat":
        return RIF.range_search(metric, d["coarse"], d["lists"][:n], d["stored"][:n], Q, case.nprobe, radius, mask)
    if case.family == "ivfsq":
        return RIF.sq_range_search(metric, d["coarse"], d["lists"][:n], c["sq"], d["codes"][:n], Q, case.nprobe, radius, mask)
    raise ValueError(case.family)


def dense_statement_filtered_range(case: Case, n: int, radius, mask):
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    if case.family == "ivfflat":
        return RF.range_search(metric, Q, d["stored"][:n].astype(F), radius, mask)
    if case.family == "ivfsq":
        return RF.sq_range_search(metric, Q, c["sq"], d["codes"][:n], radius, mask)
    raise ValueError(case.family)


def statement_hamming_range(case: Case, n: int, hradius, mask=None, dense=False):
    """(lims, idx, dist) of a Hamming-radius range search over the first n rows, among the allowed rows with a mask;
    dense: the resident index's statement for an IVFBinaryIndex case"""
    c, d = case.ctor, case.data
    thr, low, high = c["bq"]
    if case.family == "binary" or (dense and case.family == "ivfbin"):
        if mask is None:
            return BR.search(_qwords(case), d["words"][:n], case.dim, low, high, case.metric, hradius)
        return BF.range_search(_qwords(case), d["words"][:n], case.dim, low, high, case.metric, hradius, mask)
    if case.family == "ivfbin":
        front = (case.metric, case.coarse_metric, d["coarse"], d["lists"][:n], c["bq"], d["words"][:n], case.dim, case.queries,
                 case.nprobe, hradius)
        return BR.ivf_search(*front) if mask is None else BF.ivf_range_search(*front, mask)
    raise ValueError(case.family)


def allowed_in_reach(case: Case, n: int, mask) -> np.ndarray:
    """(nq,) the number of allowed rows a query can return: those of its probed lists (ref_ivf_filter.allowed_members), of a
    resident index all of them"""
    if case.family in DENSE:
        return np.full(case.nq, int(np.count_nonzero(mask)), np.int64)
    lists = case.data["lists"][:n]
    P = I.probe(case.coarse_metric, case.data["coarse"], case.queries, case.nprobe)
    return np.array([RIF.allowed_members(lists, P[j], mask).size for j in range(case.nq)], np.int64)
