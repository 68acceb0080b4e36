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

`draw_mutated(family, seed)` is the same case again under adds, removes and the family's query ops between them, from a
third generator (neither other stream moves), for the ten families whose index has `remove_rows` (MUTABLE).  A resident
family is built over a prefix of its rows and adds the rest; a remove op has one of REMOVE_KINDS, handed over as a bool
mask or as shuffled ids with repeats, some directly before close() or save / load.  Every op carries `present`, the
original ids of the rows in the index behind it; a query op is held to the family's statement over
`gathered(case, case.n, present)`, so row ids are positions in `present`.

`statement_search`, `statement_range`, `statement_rerank` and `dense_statement`, and for the new ops
`statement_filtered_search`, `statement_filtered_range`, `statement_hamming_range` and their dense forms, dispatch a case to
the numpy statements of tests/ref_*.py.  They make no arithmetic of their own.
"""
import dataclasses
import zlib
from dataclasses import dataclass, field

import numpy as np

import ref_abin as A
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
import ref_ivfsq4 as IS4
import ref_knn as K
import ref_pq_filter as RPF
import ref_mutate as M
import ref_range as RG
import ref_sq4 as S4
import ref_sqbq as S
import ref_sqindex as SI
from test_gpu_fuzz import KINDS, _draw_data

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
ALL5 = (0, 1, 2, 3, 4)
SUMS = (0, 1, 2)  # the metrics with an ADC / Hamming form: no cosine

# seeds per family at VQ_FUZZ_SCALE=1 (tests/test_fuzz_search_draws.py holds the coverage these give)
N_FAMILY = {"flat": 24, "scalar": 16, "binary": 16, "pq": 16, "ivfpq": 16, "ivfflat": 24, "ivfsq": 16, "ivfbin": 16,
            "abin": 16, "sq4": 16, "ivfsq4": 16}
FAMILIES = tuple(N_FAMILY)
DENSE = ("flat", "scalar", "binary", "pq", "abin", "sq4")  # every row is a candidate of every query
IVF = ("ivfpq", "ivfflat", "ivfsq", "ivfbin", "ivfsq4")
PACKED = ("abin", "sq4", "ivfsq4")  # exact f32 queries over packed words: the statements share one distance matrix a case
PAIRS = {
    "flat": [(k, m) for m in ALL5 for k in ("flat_f32", "flat_f16")],
    "scalar": [("scalar", m) for m in ALL5],
    "binary": [("binary", m) for m in SUMS],
    "pq": [("pq", m) for m in SUMS],
    "ivfpq": [(k, m) for m in SUMS for k in ("ivfpq", "ivfpq_residual")],
    "ivfflat": [(k, m) for m in ALL5 for k in ("ivfflat_f32", "ivfflat_f16")],
    "ivfsq": [("ivfsq", m) for m in ALL5],
    "ivfbin": [("ivfbin", m) for m in SUMS],
    "abin": [("abin", m) for m in ALL5],
    "sq4": [("sq4", m) for m in ALL5],
    "ivfsq4": [("ivfsq4", m) for m in ALL5],
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
    "abin": ("search", "range_search", "save_load_search"),
    "sq4": ("search", "range_search", "save_load_search"),
    "ivfsq4": ("search", "range_search", "close_search", "save_load_search", "rerank_search"),
}
NQ = (1, 3, 17, 40, 130)
FLAT_DIMS = (1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 36, 64, 100, 127, 128, 129, 200)
BINARY_DIMS = (1, 31, 32, 33, 64, 65, 96, 128, 192, 1056)
SQ4_DIMS = (1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 39, 40, 41, 63, 64, 65, 100, 129, 200)  # 8 to a word, 32 to a chunk
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
    gathered: bool = False  # a case over some of another's rows (`gathered`): the planted duplicates are not at its end
    cache: dict = field(default_factory=dict, repr=False, compare=False)  # a PACKED case's distance matrix, computed once

    def describe(self, upto=None) -> str:
        """the whole case in one line: a red seed replays from it"""
        ops = self.ops if upto is None else self.ops[:upto + 1]
        c = " ".join(f"{k}={v}" for k, v in sorted(self.ctor.items()))
        return (f"family={self.family} seed={self.seed} kind={self.kind} metric={NAMES[self.metric]} "
                f"coarse_metric={NAMES[self.coarse_metric]} data={self.data_kind} dense_cut={self.dense_cut} n={self.n} "
                f"dim={self.dim} nlist={self.nlist} nprobe={self.nprobe} topk={self.topk} nq={self.nq} {c} "
                f"ops=[{', '.join(_op_text(o) for o in ops)}]")


def _op_text(o) -> str:
    if o["op"] == "add" and "hi" in o:  # a mutated case's add: the original rows lo .. hi - 1 arrive as ids at .. n - 1
        return f"{o['how']}[{o['lo']}:{o['hi']}]@{o['at']}"
    if o["op"] == "add":
        return f"{o['how']}[{o['lo']}:{o['n']}]"
    if o["op"] == "remove":
        flags = "".join(f" {k}" for k in ("then_close", "then_load") if o.get(k))
        return f"remove(n={o['n_before']}->{o['n']} kind={o['kind']} form={o['form']} removed={o['removed']}{flags})"
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
    if fam in PACKED:  # (their first two query ops go round-robin from the seed: every op often enough by construction)
        return _draw_ops_in_turn(rng, case)

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


def _draw_ops_in_turn(rng, case):
    """_draw_ops with the first two query ops taken in turn from the seed"""
    fam, n, seed = case.family, case.n, case.seed
    qops = QUERY_OPS[fam]
    ops, nth = [], 0

    def query(n_now):
        nonlocal nth
        ops.append(_query_op(rng, case, qops if nth >= 2 else (qops[(2 * seed + nth) % len(qops)],), n_now))
        nth += 1

    if fam in IVF:
        pieces = min(n, int(rng.choice([1, 2, 3])))
        cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, n), pieces - 1, replace=False)) + [n]
        for i in range(pieces):
            ops.append({"op": "add", "lo": cuts[i], "n": cuts[i + 1], "how": str(rng.choice(case.ctor["adds"]))})
            if i + 1 < pieces and rng.random() < 0.7:
                query(cuts[i + 1])
        room = 7 - len(ops)
        for _ in range(max(3 - len(ops), int(rng.integers(1, room + 1)))):
            query(n)
    else:
        for _ in range(int(rng.integers(3, 8))):
            query(n)
    return ops


def _draw_radius(rng, case, n_now):
    """per-query radii from the case's own k-th distances (ref_range.kth_distance), so that the hits are neither none nor
    all; query 0 (equal to a duplicated row) gets its 2nd distance: an exact tie on the boundary; the last query -1; with
    17 queries or more, the one before it +inf"""
    nq = case.nq
    if case.family in PACKED:  # (the same k-th distances, off the case's one distance matrix)
        k = int(rng.integers(1, min(n_now, 40) + 1))
        r = A.topk(_matrix(case, n_now), k)[1][:, k - 1].copy()
        r[0] = A.topk(_matrix(case, n_now)[:1], min(2, n_now))[1][0, -1]
    else:
        X = decoded(case)[:n_now]
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
    if case.family in ("sq4", "ivfsq4"):
        return S4.decode(d["words"], case.dim, *case.ctor["sq"])
    if case.family == "abin":
        return A.decode(d["words"], case.dim, *case.ctor["bq"][1:])
    raise ValueError(case.family)


def _matrix(case, n: int) -> np.ndarray:
    """D(q, i) float32 (nq, n) of a PACKED case over its first n rows, every row a candidate: ref_abin / ref_sq4's
    distance_matrix, computed once a case (a row's distance does not depend on the other rows)"""
    if "D" not in case.cache:
        if case.family == "abin":
            case.cache["D"] = A.distance_matrix(case.metric, case.queries, case.data["words"], case.dim, *case.ctor["bq"][1:])
        else:
            case.cache["D"] = S4.distance_matrix(case.metric, case.queries, case.data["words"], case.dim, *case.ctor["sq"])
    return case.cache["D"][:, :n]


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
    elif family in ("binary", "ivfbin", "abin"):
        dim = int(rng.choice(BINARY_DIMS)) if rng.random() < 0.5 else int(rng.integers(1, 1101))
    elif family in ("sq4", "ivfsq4"):
        dim = int(rng.choice(SQ4_DIMS)) if rng.random() < 0.5 else int(rng.integers(1, 201))
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
        if family == "ivfsq4" and seed % 8 == 3:  # more lists than rows by construction (elsewhere the seed count sees to it)
            n = int(rng.integers(1, 40))
            nlist = n + int(rng.integers(1, 50))
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
            odd = rng.integers(0, n, 3)
            if family not in PACKED:  # (sq_encode sends NaN to code 0 and a bit is a bit: those get stored words of their own)
                X[odd] = np.nan
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
        elif family in ("sq4", "ivfsq4"):
            sq = S4.QUANTIZERS[int(rng.integers(0, len(S4.QUANTIZERS)))]
            source = str(rng.choice(["codes", "packed"] if dense_cut else ["rows", "codes", "packed"]))
            codes = S.sq_encode(sq[0], sq[1], sq[2], X)
            if source != "rows" and not dense_cut and n >= 16:
                at = rng.integers(7, n - 7, 5)
                codes[at] = rng.integers(0, 16, (5, dim)).astype(np.uint8)  # every nibble is legal (codes >= levels too)
            if dense_cut:  # the three odd rows: all nibbles 15 (all 0 where the tied rows are all 15 themselves)
                codes[odd] = 0 if bool((codes[0] == 15).all()) else 15
            data["codes"] = codes
            data["words"] = S4.pack4(codes)
            ctor.update(sq=sq, source=source)
            if ivf:
                ctor.update(adds=("add_codes", "add_packed") if source != "rows" else ("add_rows", "add_codes", "add_packed"))
            row0 = S4.decode(data["words"][:1], dim, *sq)[0]
        elif family == "abin":
            low, high = A.LOW_HIGH[int(rng.integers(0, len(A.LOW_HIGH)))]
            thr = float(rng.choice([0.0, -0.5, 0.25, float(X[int(rng.integers(0, n)), int(rng.integers(0, dim))])]))
            thr = float(F(thr)) if np.isfinite(thr) else 0.0
            bits = B.bits_f32(X, thr)
            data["bq_codes"] = S.bq_encode(thr, low, high, X)
            if dense_cut:  # the three odd rows: every bit of the tied rows inverted
                bits[odd] = ~bits[0]
                data["bq_codes"][odd] = S.bq_encode(0.5, low, high, bits[odd])  # (True is 1.0: the code of a set bit)
            data["words"] = B.pack(bits)
            ctor.update(bq=(thr, low, high), source=str(rng.choice(["codes", "packed"] if dense_cut else ["rows", "codes", "packed"])))
            row0 = A.decode(data["words"][:1], dim, low, high)[0]
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
    if fam in ("abin", "sq4"):
        return A.topk(_matrix(case, n), topk)
    if fam == "ivfsq4":
        return IS4.search(metric, d["coarse"], d["lists"][:n], c["sq"], d["codes"][:n], Q, case.nprobe, topk)
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
    if case.family == "ivfsq4":  # ref_sq4 over the packed words
        return A.topk(_matrix(case, n), topk)
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
    if case.family in ("abin", "sq4"):
        return A.ranged(_matrix(case, n), radius)
    if case.family == "ivfsq4":
        return IS4.range_search(metric, d["coarse"], d["lists"][:n], c["sq"], d["codes"][:n], Q, case.nprobe, radius)
    raise ValueError(case.family)


def dense_statement_range(case: Case, n: int, radius):
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    if case.family == "ivfflat":
        return RG.search(metric, Q, d["stored"][:n].astype(F), radius)
    if case.family == "ivfsq":
        return RG.sq_search(metric, Q, c["sq"], d["codes"][:n], radius)
    if case.family == "ivfsq4":
        return A.ranged(_matrix(case, n), radius)
    raise ValueError(case.family)


def rerank_rows(case: Case, n: int) -> np.ndarray:
    """the f32 rows of the exact index a rerank_search goes through"""
    return (case.data["rows"] if case.family in ("binary", "ivfbin", "ivfsq", "ivfsq4") else case.data["rerank_rows"])[:n]


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
    "abin": ("filtered_search", "filtered_range_search"),
    "sq4": ("filtered_search", "filtered_range_search"),
    "ivfsq4": ("filtered_search", "filtered_range_search", "filtered_rerank_search"),
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
        return n_now == case.n >= 2 and not case.dense_cut and not case.gathered
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
    if fam in ("abin", "sq4"):
        return A.topk(_matrix(case, n), topk, mask)
    if fam == "ivfsq4":
        return IS4.search_masked(metric, d["coarse"], d["lists"][:n], c["sq"], d["codes"][:n], Q, case.nprobe, topk, mask)
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
    if case.family == "ivfsq4":
        return A.topk(_matrix(case, n), topk, mask)
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
    if case.family in ("abin", "sq4"):
        return A.ranged(_matrix(case, n), radius, mask)
    if case.family == "ivfsq4":
        return IS4.range_search_masked(metric, d["coarse"], d["lists"][:n], c["sq"], d["codes"][:n], Q, case.nprobe, radius, mask)
    raise ValueError(case.family)


def dense_statement_filtered_range(case: Case, n: int, radius, mask):
    c, d, Q, metric = case.ctor, case.data, case.queries, case.metric
    if case.family == "ivfflat":
        return RF.range_search(metric, Q, d["stored"][:n].astype(F), radius, mask)
    if case.family == "ivfsq":
        return RF.sq_range_search(metric, Q, c["sq"], d["codes"][:n], radius, mask)
    if case.family == "ivfsq4":
        return A.ranged(_matrix(case, n), radius, mask)
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


# -- the third draw: rows added and removed -----------------------------------------------------------------------------------
MUTATE_WORD = 0x4D555441  # the third seed word of draw_mutated's generator: neither draw() nor draw_filtered() sees it
MUTABLE = tuple(f for f in FAMILIES if f != "pq")  # (PQIndex searches the caller's own codes: it has no remove_rows)
N_MUTATED = {f: 24 for f in MUTABLE}  # seeds per family at VQ_FUZZ_SCALE=1: every remove kind twice a family takes these
REMOVE_KINDS = ("one_row", "block", "block64", "word_straddle", "random", "all_but_one", "winners", "lower_twins", "nothing")
IVF_REMOVE_KINDS = ("one_list", "everything")  # a resident index refuses a removal of every row
REMOVES_P = (0.1, 0.3, 0.6)  # 1, 2 or 3 remove ops a case
REMOVE_ORDER = {"nothing": 0, "one_row": 0, "lower_twins": 0, "word_straddle": 0, "winners": 1, "block64": 1, "one_list": 1,
                "random": 2, "block": 2, "all_but_one": 3, "everything": 3}  # within a case: how few rows a kind leaves
REMOVE_FORMS = ("bool", "ids")
PER_ROW = ("rows", "stored", "codes", "words", "bq_codes", "rerank_rows", "lists")
SEARCH_LIKE = ("search", "close_search", "save_load_search", "rerank_search")


def mutated_seeds(family, scale=1):
    return range(N_MUTATED[family] * scale)


def remove_kinds(family):
    return REMOVE_KINDS + (IVF_REMOVE_KINDS if family in IVF else ())


def gathered(case: Case, n: int, rows) -> Case:
    """the case over `rows` of its first n rows alone: every per-row array gathered (a PACKED case's distance matrix too:
    a row's distances are its own), the rest as it is; row ids of the new case are positions in `rows`"""
    rows = np.asarray(rows, np.int64)
    data = {k: (v[:n][rows] if k in PER_ROW else v) for k, v in case.data.items()}
    cache = {"D": _matrix(case, n)[:, rows]} if case.family in PACKED else {}
    return dataclasses.replace(case, n=int(rows.size), data=data, gathered=True, cache=cache)


def every_row(case: Case) -> Case:
    """the case with every list probed: a range search at radius +inf (a Hamming radius past `dim`; for IVFPQIndex a
    search at topk = n) then returns every row whose distance is not NaN, so every id shows"""
    return dataclasses.replace(case, nprobe=case.nlist)


def resident_adds(case: Case):
    """the add methods of a resident case that store what the constructor stored (planted codes and the dense cut's odd
    words exist as codes and words only)"""
    fam, source = case.family, case.ctor.get("source")
    if fam == "flat":
        return ("add",)
    if fam == "scalar":
        return ("add", "add_codes") if source == "rows" else ("add_codes",)
    if fam == "binary":
        return ("add", "add_codes", "add_packed")
    if fam in ("abin", "sq4"):
        return ("add", "add_codes", "add_packed") if source == "rows" else ("add_codes", "add_packed")
    raise ValueError(fam)


def _twin_pairs(case: Case, present):
    """positions in `present` of the lower row of every planted duplicate pair (_plant, the code rows) still whole"""
    n = case.n
    pairs = [(i, n - 7 + i) for i in range(7)] if n >= 14 else [(0, n - 1)] if n >= 2 else []
    where = {int(r): p for p, r in enumerate(present.tolist())}
    return np.array([where[a] for a, b in pairs if a in where and b in where], np.int64)


def _remove_applies(case, G, kind, present, adds_left) -> bool:
    n_now, ivf = int(present.size), case.family in IVF
    if kind == "nothing":
        return True
    if n_now < 2 and not (ivf and adds_left):
        return False  # (its one row stays: a query op follows)
    if kind == "block64":
        return n_now > 64
    if kind == "word_straddle":
        return n_now >= 34
    if kind == "winners":
        return ivf or n_now > 4
    if kind == "lower_twins":
        return not case.dense_cut and _twin_pairs(case, present).size > 0
    if kind == "everything":
        return adds_left > 0
    return True


def _draw_removal(rng, case, G, kind, present, adds_left) -> np.ndarray:
    """bool (n_now,): the rows one remove op takes out -- all of them only from an IVF index with an add to come"""
    n_now, ivf = int(present.size), case.family in IVF
    m = np.zeros(n_now, np.bool_)
    if kind == "one_row":
        m[int(rng.choice([0, n_now - 1, int(rng.integers(0, n_now))]))] = True
    elif kind == "block":
        lo = int(rng.integers(0, n_now))
        m[lo:int(rng.integers(lo + 1, n_now + 1))] = True
    elif kind == "block64":  # a run of whole 64-row groups (the last one as far as the rows go), never all of them
        groups = (n_now + 63) // 64
        a = int(rng.integers(0, groups))
        b = int(rng.integers(a + 1, groups + 1))
        if a == 0 and b == groups:
            a = 1
        m[64 * a:min(64 * b, n_now)] = True
    elif kind == "word_straddle":  # the last two rows of one 32-row mask word and the first two of the next
        g = int(rng.integers(0, (n_now - 34) // 32 + 1))
        m[32 * g + 30:32 * g + 34] = True
    elif kind == "random":
        m = rng.random(n_now) < float(rng.choice([0.5, 0.03]))
    elif kind == "all_but_one":
        m[:] = True
        m[int(rng.choice([0, n_now - 1, int(rng.integers(0, n_now))]))] = False
    elif kind == "winners":  # a removal that is ignored returns exactly these rows again
        winners = statement_search(G, n_now, min(G.topk, n_now, 4))[0]
        m[winners[winners != I.PAD_ID].astype(np.int64)] = True
    elif kind == "lower_twins":  # the distance bits of the next search stay, the ids change
        m[_twin_pairs(case, present)] = True
    elif kind == "one_list":  # every row of one list with rows, mostly one that some query probes
        lists = G.data["lists"]
        live = np.unique(lists)
        P = I.probe(case.coarse_metric, case.data["coarse"], case.queries, case.nprobe)
        probed = live[np.isin(live, P)]
        if probed.size and rng.random() < 0.75:
            live = probed
        m = lists == live[int(rng.integers(0, live.size))]
    elif kind == "everything":
        m[:] = True
    elif kind != "nothing":
        raise ValueError(kind)
    if m.all() and not (ivf and adds_left):  # (block, random, the one row, the one list ...: a query op follows)
        m[int(rng.integers(0, n_now))] = False
    return m


def _draw_mutated_ops(rng, case):
    """4 to 9 ops: the adds (an IVF family's 1 to 3 slices; a resident family is built over a prefix and adds the rest in 0
    to 2 slices), 1 to 3 removes and 3 or more of the family's QUERY_OPS + NEW_OPS between and behind them, the last op a
    query.  Every op carries `present`: the original ids of the rows in the index behind it, in order."""
    fam, n, seed = case.family, case.n, case.seed
    ivf = fam in IVF
    if ivf:
        pieces = min(n, int(rng.choice([1, 2, 3])))
        if seed % 8 == 2:
            pieces = min(n, max(pieces, 2))  # (a removal of every row needs an add behind it)
        hows = case.ctor["adds"]
    else:
        pieces = min(n - 1, int(rng.integers(0, 3))) + 1  # (the first piece is the constructor's)
        hows = resident_adds(case)
    cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, n), pieces - 1, replace=False)) + [n]
    adds = [{"op": "add", "lo": cuts[i], "hi": cuts[i + 1], "how": str(rng.choice(hows))} for i in range(pieces)]
    present = np.empty(0, np.int64)
    ops = []

    def add():
        nonlocal present
        o = adds.pop(0)
        o["at"] = int(present.size)  # the ids an add returns start at the current length
        present = np.concatenate([present, np.arange(o["lo"], o["hi"], dtype=np.int64)])
        o.update(n=int(present.size), present=present.copy())
        ops.append(o)

    if ivf:
        add()
    else:
        present = np.arange(adds.pop(0)["hi"], dtype=np.int64)
    removes = int(rng.choice([1, 2, 3], p=REMOVES_P))
    queries = int(rng.integers(3, max(3, 9 - len(ops) - len(adds) - removes) + 1))
    names = QUERY_OPS[fam] + NEW_OPS[fam]
    # the kinds of the case's removes: the next ones of the round that goes through the seeds, those that leave few rows
    # last.  The two kinds that need the case's help come by construction, one seed in eight each.
    turn = remove_kinds(fam)
    forced = "everything" if ivf and seed % 8 == 2 else "lower_twins" if seed % 8 == 5 else None
    window = [turn[(4 * seed + i) % len(turn)] for i in range(removes)]
    if forced:
        window[0] = forced
    window.sort(key=lambda k: -1 if k == forced else REMOVE_ORDER[k])
    nth_remove = nth_query = nth_filtered = 0
    while adds or removes or queries:
        n_now = int(present.size)
        tokens = (["add"] if adds else []) + (["remove"] if removes and n_now else []) + (["query"] if queries > 1 and n_now else [])
        tok = str(rng.choice(tokens)) if tokens else "query"  # (the last query closes the case)
        if forced == "everything" and nth_remove == 0 and removes and n_now:
            tok = "remove"   # (while an add is still to come)
        if forced == "lower_twins" and nth_remove == 0 and adds:
            tok = "add"      # (both rows of a pair are in only behind the last add)
        if tok == "add":
            add()
            continue
        G = gathered(case, n, present)
        if tok == "remove":
            kind = window[nth_remove]
            at = turn.index(kind)
            if not _remove_applies(case, G, kind, present, len(adds)):  # (the next kind in turn that does)
                ok = [k for k in turn[at:] + turn[:at] if k != "nothing" and _remove_applies(case, G, k, present, len(adds))]
                kind = ok[0] if ok else "nothing"
            gone = _draw_removal(rng, case, G, kind, present, len(adds))
            o = {"op": "remove", "kind": kind, "form": str(rng.choice(REMOVE_FORMS)), "n_before": n_now,
                 "removed": int(gone.sum())}
            if o["form"] == "bool":
                o["arg"] = gone
            else:  # the ids shuffled, some of them twice
                ids = np.flatnonzero(gone)
                twice = rng.choice(ids, int(rng.integers(0, min(ids.size, 5) + 1))) if ids.size else ids
                o["arg"] = rng.permutation(np.concatenate([ids, twice])).astype(np.int64)
            present = present[M.kept(n_now, o["arg"]).astype(np.int64)]
            o.update(n=int(present.size), present=present.copy())
            close = ivf and (rng.random() < 0.15 or (nth_remove == 0 and seed % 4 == 1))
            load = fam in HAS_SAVE and (rng.random() < 0.15 or (nth_remove == 0 and seed % 4 == 3))
            if present.size and close:
                o["then_close"] = True  # close() directly behind the remove: the next call rebuilds the handle
            elif present.size and load:
                o["then_load"] = True   # save / load directly behind: the run goes on with the loaded index
            ops.append(o)
            removes -= 1
            nth_remove += 1
            continue
        name = names[(3 * seed + nth_query) % len(names)] if nth_query < 3 else str(rng.choice(names))
        if name in NEW_OPS[fam]:
            o = _new_op(rng, G, name, n_now, nth_filtered)
            nth_filtered += name in FILTERED
        else:
            o = _query_op(rng, G, (name,), n_now)
        o["present"] = present.copy()
        ops.append(o)
        queries -= 1
        nth_query += 1
    reranks = [o for o in ops if "flat_metric" in o]
    for o in reranks:  # one flat metric a case: the reranker is one FlatIndex that follows the adds and removes
        o["flat_metric"] = reranks[0]["flat_metric"]
    return ops


def draw_mutated(family: str, seed: int) -> Case:
    """draw(family, seed) with its ops replaced: the same index, rows and queries under adds, removes and the family's query
    ops, every query op held to its statement over `gathered(case, case.n, op["present"])`"""
    case = draw(family, seed)
    rng = np.random.default_rng([zlib.crc32(family.encode()), int(seed), MUTATE_WORD])
    case.ops = _draw_mutated_ops(rng, case)
    return case


def built_over(case: Case) -> int:
    """the rows a mutated resident case is built over: the prefix its first add starts behind (all rows without an add)"""
    first = next((o for o in case.ops if o["op"] == "add"), None)
    return case.n if first is None else first["lo"]
