"""The cases of the threaded search tests (tests/test_gpu_search_threads.py) and the statement each call is held to.  No GPU
here; tests/test_search_thread_cases.py holds what the cases claim.

One data set serves every kind of index: N rows of D dimensions (past one 1024-position view block, past the 64-row
tiles, no multiple of 32), NLIST lists of which a few stay empty, NQ queries with a row's twin, the zero vector, a NaN
element and the centroid of an empty list among them.  A KIND is a family of handle with its metric and storage; `case(kind)`
gives its VARIANTS: calls that differ in exactly what the handle's workspaces are sized by (queries, topk, nprobe, a row
mask, radii, candidates), each with the result the numpy statements of tests/ref_*.py give for it.  `add_case(kind)` gives
an inverted-file kind's calls with their results over each of the four PREFIXES of the rows, `device_case(kind)` the two
threads' calls of the cross-stream tests.  Nothing here makes arithmetic of its own."""
import functools
from dataclasses import dataclass

import numpy as np

import ref_binary as B
import ref_binary_range as BR
import ref_filter as RF
import ref_ivf as I
import ref_ivf_filter as IVFF
import ref_ivf_range as IRG
import ref_ivf_residual as IRES
import ref_ivfbin as IB
import ref_ivfflat as IFL
import ref_knn as K
import ref_range as RG
import ref_sqbq as S
import ref_sqindex as SI

F = np.float32
N, D, NLIST, NQ = 2100, 33, 37, 130
EMPTY_LISTS = 4
PREFIXES = (400, 900, 1300, 2100)  # the rows before the adder starts and behind each of its three uneven slices
THREADS, ITERS = 8, 30
SHAPES = ((1, 1, 1), (17, 10, 5), (130, 300, NLIST))  # (nq, topk, nprobe) of the three plain searches
NQ_MID, TOPK_MID, NPROBE_MID = SHAPES[1]
FEW = 6            # allowed rows of the mask with fewer than TOPK_MID of them
RERANK_C = 40      # candidates per query of the rerank variant
KTH = 25           # the radii are the KTH-th distances
MAX_RESULTS = 1 << 28
SQ = (-3.0, 5.0, 17)   # ref_sqindex.QUANTIZERS[2]: few levels, so equal distances and ties on the radius
PQ_M, PQ_K, PQ_SD = 3, 16, 11

# kind -> (family, metric, options)
KINDS = {
    "flat_f32_euclidean": ("flat", K.EUCLIDEAN, {"dtype": "float32"}),
    "flat_f16_cosine": ("flat", K.COSINE, {"dtype": "float16"}),
    "sqindex_manhattan": ("sqindex", K.MANHATTAN, {}),
    "sqindex_cosine_unclamped": ("sqindex", K.COSINE_UNCLAMPED, {}),
    "binary_euclidean": ("binary", K.EUCLIDEAN, {"bq": (0.0, 0, 1)}),
    "pq_adc_euclidean": ("pq", K.EUCLIDEAN, {}),
    "ivfpq_manhattan": ("ivfpq", K.MANHATTAN, {"residual": False}),
    "ivfpq_residual_squared": ("ivfpq", K.SQUARED_EUCLIDEAN, {"residual": True}),
    "ivfflat_f32_squared": ("ivfflat", K.SQUARED_EUCLIDEAN, {"dtype": "float32"}),
    "ivfflat_f16_cosine": ("ivfflat", K.COSINE, {"dtype": "float16"}),
    "ivfsq_euclidean": ("ivfsq", K.EUCLIDEAN, {}),
    "ivfsq_cosine": ("ivfsq", K.COSINE, {}),
    "ivfbin_manhattan": ("ivfbin", K.MANHATTAN, {"bq": (0.25, 3, 200), "coarse_metric": K.COSINE}),
}
EXACT = ("flat", "sqindex", "ivfflat", "ivfsq")  # the families with masks, range search (and, resident, rerank)
IVF = ("ivfpq", "ivfflat", "ivfsq", "ivfbin")
DEVICE_KINDS = ("flat_f16_cosine", "sqindex_manhattan", "binary_euclidean", "ivfflat_f16_cosine", "ivfsq_euclidean",
                "ivfpq_residual_squared", "ivfbin_manhattan")  # the kinds of the cross-stream tests
REGROW_KINDS = ("flat_f16_cosine", "ivfflat_f16_cosine")


@dataclass
class Variant:
    name: str
    op: str                 # search, search_masked, range_search, range_search_masked, rerank, hamming_range_search, probe,
                            # search_codes (the ADC search over host codes)
    nq: int
    topk: int = 0
    nprobe: int = 0
    mask: np.ndarray = None   # bool (rows,): the allowed rows
    radii: np.ndarray = None  # f32 (nq,), or the uint32 Hamming radii
    cand: np.ndarray = None   # uint32 (nq, RERANK_C)
    q0: int = 0               # the first query
    want: tuple = None        # (idx, dist), (lims, idx, dist) or (lists,)

    @property
    def masked(self) -> bool:
        return self.mask is not None

    def describe(self) -> str:
        extra = "".join(f" {k}={getattr(self, k)}" for k in ("topk", "nprobe") if getattr(self, k))
        return f"{self.name}: {self.op}(nq={self.nq}{extra}{' mask=' + str(int(self.mask.sum())) + ' rows' if self.masked else ''})"


@dataclass
class Case:
    kind: str
    family: str
    metric: int
    opts: dict
    data: dict
    variants: list

    @property
    def ivf(self) -> bool:
        return self.family in IVF

    def queries(self, v: Variant) -> np.ndarray:
        return np.ascontiguousarray(self.data["queries"][v.q0:v.q0 + v.nq])


# -- the data ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base() -> dict:
    rng = np.random.default_rng(20241)
    X = rng.standard_normal((N, D)).astype(F)
    X[11] = 0.0
    live = rng.permutation(NLIST)[:NLIST - EMPTY_LISTS]
    lists = live[rng.integers(0, live.size, N)].astype(np.uint32)
    for p in PREFIXES:  # a twin of a row of the first prefix ends every prefix, in its list: ties go to the lower row id
        X[p - 3:p] = X[:3]
        lists[p - 3:p] = lists[:3]
    coarse = rng.standard_normal((NLIST, D)).astype(F)
    empty = np.setdiff1d(np.arange(NLIST), live)
    Q = rng.standard_normal((NQ, D)).astype(F)
    Q[0] = X[0]
    Q[1] = 0.0
    Q[2, D // 2] = np.nan
    Q[3] = coarse[empty[0]]
    Q[60] = X[1]
    cb = rng.standard_normal((PQ_M, PQ_K, PQ_SD)).astype(F)
    cb[:, PQ_K - 1] = cb[:, 0]  # a duplicate centroid: equal distances
    pq_codes = rng.integers(0, PQ_K, (N, PQ_M)).astype(np.uint8)
    for p in PREFIXES:
        pq_codes[p - 3:p] = pq_codes[:3]
    sparse = rng.random(N) < 0.01
    sparse[128:448] = False                # whole 64-row tiles without an allowed row
    sparse[[5, N - 1]] = True
    half = rng.random(N) < 0.5
    few = np.zeros(N, np.bool_)
    few[rng.choice(N, FEW, replace=False)] = True
    cand = np.stack([rng.choice(N, RERANK_C, replace=False) for _ in range(NQ_MID)]).astype(np.uint32)
    sq_codes = S.sq_encode(SQ[0], SQ[1], SQ[2], X)
    d = {"rows": X, "lists": lists, "coarse": coarse, "queries": np.ascontiguousarray(Q), "codebooks": cb, "pq_codes": pq_codes,
         "masks": {"sparse": sparse, "half": half, "few": few}, "cand": cand, "sq_codes": sq_codes, "empty": empty}
    for a in (X, lists, coarse, Q, cb, pq_codes, sparse, half, few, cand, sq_codes):
        a.setflags(write=False)  # shared by every case and every thread: left unchanged
    return d


def _kind_data(kind: str) -> dict:
    family, _, opts = KINDS[kind]
    d = dict(base())
    X = d["rows"]
    if family in ("flat", "ivfflat"):
        d["stored"] = X.astype(np.dtype(opts["dtype"]))
        d["decoded"] = d["stored"].astype(F)
    elif family in ("sqindex", "ivfsq"):
        d["decoded"] = SI.decode(SQ, d["sq_codes"])
    elif family in ("binary", "ivfbin"):
        d["words"] = B.pack(B.bits_f32(X, opts["bq"][0]))
    return d


# -- the statements -----------------------------------------------------------------------------------------------------------
def statement(case: Case, v: Variant, n: int = N):
    """the result of variant v over the first n rows, by the numpy statements"""
    fam, metric, d, o = case.family, case.metric, case.data, case.opts
    Q = case.queries(v)
    lists, coarse = d["lists"][:n], d["coarse"]
    mask = None if v.mask is None else v.mask[:n]
    if v.op == "probe":
        return (I.probe(o.get("coarse_metric", metric), coarse, Q, v.nprobe),)
    if fam in ("flat", "sqindex"):
        X = d["decoded"][:n]
        if v.op == "search":
            return K.search(metric, Q, X, v.topk)
        if v.op == "search_masked":
            return RF.search(metric, Q, X, v.topk, mask)
        if v.op == "range_search":
            return RG.search(metric, Q, X, v.radii)
        if v.op == "range_search_masked":
            return RF.range_search(metric, Q, X, v.radii, mask)
        if v.op == "rerank":
            return K.rerank(metric, Q, X, v.cand, v.topk)
    if fam in ("ivfflat", "ivfsq"):  # (the scalar statement is the flat one over the decoded rows: ref_ivfsq, ref_ivf_filter)
        X = d["decoded"][:n]
        if v.op == "search":
            return IFL.search(metric, coarse, lists, X, Q, v.nprobe, v.topk)
        if v.op == "search_masked":
            return IVFF.search(metric, coarse, lists, X, Q, v.nprobe, v.topk, mask)
        if v.op == "range_search":
            return IRG.search(metric, coarse, lists, X, Q, v.nprobe, v.radii)
        if v.op == "range_search_masked":
            return IVFF.range_search(metric, coarse, lists, X, Q, v.nprobe, v.radii, mask)
    if fam == "binary":
        thr, low, high = o["bq"]
        qw = B.pack(B.bits_f32(Q, thr))
        if v.op == "search":
            return B.search(qw, d["words"][:n], D, low, high, metric, v.topk)
        if v.op == "hamming_range_search":
            return BR.search(qw, d["words"][:n], D, low, high, metric, v.radii)
    if fam == "ivfbin":
        if v.op == "search":
            return IB.search(metric, o["coarse_metric"], coarse, lists, o["bq"], d["words"][:n], D, Q, v.nprobe, v.topk)
        if v.op == "hamming_range_search":
            return BR.ivf_search(metric, o["coarse_metric"], coarse, lists, o["bq"], d["words"][:n], D, Q, v.nprobe, v.radii)
    if fam == "pq" and v.op in ("search", "search_codes"):  # the ADC full pass: the inverted-file statement with one list
        return I.brute_search(metric, np.zeros((1, D), F), d["codebooks"], np.zeros(n, np.uint32), d["pq_codes"][:n], Q, 1, v.topk)
    if fam == "ivfpq" and v.op == "search":
        ref = IRES if o["residual"] else I
        return ref.brute_search(metric, coarse, d["codebooks"], lists, d["pq_codes"][:n], Q, v.nprobe, v.topk)
    raise ValueError(f"{case.kind}: no statement for {v.op}")


def _radii(case: Case, q0: int, nq: int) -> np.ndarray:
    """per-query radii from the case's own KTH-th distances (ref_range.kth_distance), as the search fuzz draws them: query
    0 (a row's twin) gets its 2nd distance, an exact tie on the boundary; the last query -1, the one before it +inf"""
    Q = case.data["queries"][q0:q0 + nq]
    X = case.data["decoded"]
    r = RG.kth_distance(case.metric, Q, X, KTH)
    r[0] = RG.kth_distance(case.metric, Q[:1], X, 2)[0]
    r[np.isnan(r)] = F(1.0)  # (a NaN radius is refused)
    r[-1] = F(-1.0)
    r[-2] = np.inf
    return r.astype(F)


def _hradii(case: Case, q0: int, nq: int) -> np.ndarray:
    """Hamming radii the same way: the KTH-th Hamming distance, 0 for the row's twin, the dimension (every row) for the
    last query and 2^32 - 1 for the one before it"""
    Q = case.data["queries"][q0:q0 + nq]
    H = np.sort(B.hamming(B.pack(B.bits_f32(Q, case.opts["bq"][0])), case.data["words"]), axis=1)
    h = H[:, KTH - 1].astype(np.uint32)
    h[0] = 0
    h[-1] = D
    h[-2] = 0xFFFFFFFF
    return h


def big_nprobe(case: Case) -> int:
    """nprobe of the largest search: every list -- but 11 in the residual index, whose statement builds a table per pair"""
    return 11 if case.opts.get("residual") else NLIST


def _variants(case: Case) -> list:
    fam, d = case.family, case.data
    ivf = case.ivf
    m = d["masks"]
    plain = []
    for nq, topk, nprobe in SHAPES:
        nprobe = min(nprobe, big_nprobe(case)) if ivf else 0
        plain.append(Variant(f"search_{nq}x{topk}", "search", nq, topk, nprobe))
    np_mid = NPROBE_MID if ivf else 0
    out = []
    if fam in EXACT:  # a masked call next to an unmasked one, all the way down
        r = _radii(case, 0, NQ_MID)
        out += [plain[0],
                Variant("masked_sparse", "search_masked", NQ_MID, TOPK_MID, np_mid, mask=m["sparse"]),
                plain[1],
                Variant("masked_half", "search_masked", NQ_MID, TOPK_MID, np_mid, mask=m["half"]),
                plain[2],
                Variant("masked_few", "search_masked", NQ_MID, TOPK_MID, np_mid, mask=m["few"]),
                Variant("range", "range_search", NQ_MID, nprobe=np_mid, radii=r),
                Variant("range_masked_half", "range_search_masked", NQ_MID, nprobe=np_mid, radii=r, mask=m["half"])]
        if not ivf:
            out.append(Variant("rerank", "rerank", NQ_MID, TOPK_MID, cand=d["cand"]))
        out.append(Variant("range_masked_sparse", "range_search_masked", NQ_MID, nprobe=np_mid, radii=r, mask=m["sparse"]))
    else:
        out += plain
        if fam in ("binary", "ivfbin"):
            out.append(Variant("hamming_range", "hamming_range_search", NQ_MID, nprobe=np_mid, radii=_hradii(case, 0, NQ_MID)))
            out.append(Variant("hamming_range_40", "hamming_range_search", 40, nprobe=np_mid, radii=_hradii(case, 60, 40), q0=60))
        if fam == "pq":
            out.append(Variant("search_codes_17x10", "search_codes", NQ_MID, TOPK_MID))
    if ivf:
        out.insert(1, Variant("probe_1", "probe", NQ_MID, nprobe=1))
        out.append(Variant("probe_all", "probe", NQ, nprobe=NLIST))
    return out


@functools.lru_cache(maxsize=None)
def case(kind: str) -> Case:
    """the kind's data and its variants, each with its statement over all N rows (computed once, shared, left unchanged)"""
    family, metric, opts = KINDS[kind]
    c = Case(kind, family, metric, opts, _kind_data(kind), [])
    c.variants = _variants(c)
    for v in c.variants:
        v.want = statement(c, v)
    return c


def schedule(nvariants: int, threads: int = THREADS, iters: int = ITERS) -> list:
    """[thread][iteration] -> variant: every thread walks the variants in their order, thread t starting t places on, so that
    at every step neighbouring threads are in different variants (and with eight variants or more, all eight threads)"""
    return [[(i + t) % nvariants for i in range(iters)] for t in range(threads)]


# -- adds while searching -------------------------------------------------------------------------------------------------------
@dataclass
class AddCase:
    case: Case
    variants: list   # Variant.want: a list of the four prefixes' statements
    sizes: list      # list_sizes() at the four prefixes


@functools.lru_cache(maxsize=None)
def add_case(kind: str) -> AddCase:
    """an inverted-file kind's calls beside an adder: two plain searches for every family, and for the two exact ones a
    range search and a search under a mask that covers all N rows (include/vqhip.h: the mask is read as ceil(n / 32) words
    for the n rows of the index at the time of the call and the bits at or past n are ignored, so a longer mask is a valid
    argument at every prefix, and the statement over n rows takes its first n bits)"""
    c0 = case(kind)
    assert c0.ivf
    c = Case(c0.kind, c0.family, c0.metric, c0.opts, c0.data, [])
    big = (NQ, 300, big_nprobe(c)) if not c.opts.get("residual") else (40, 300, big_nprobe(c))
    vs = [Variant("search_17x10", "search", NQ_MID, TOPK_MID, NPROBE_MID), Variant(f"search_{big[0]}x300", "search", *big)]
    if c.family in EXACT:
        vs.append(Variant("range", "range_search", NQ_MID, nprobe=NPROBE_MID, radii=_radii(c, 0, NQ_MID)))
        vs.append(Variant("masked_half", "search_masked", NQ_MID, TOPK_MID, NPROBE_MID, mask=c.data["masks"]["half"]))
    for v in vs:
        v.want = [statement(c, v, n) for n in PREFIXES]
    c.variants = vs
    sizes = [np.bincount(c.data["lists"][:n], minlength=NLIST).astype(np.uint64) for n in PREFIXES]
    return AddCase(c, vs, sizes)


def same(a, b) -> bool:
    """two results of one call equal bit for bit: every array, the float ones as uint32"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if not np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y):
            return False
    return True


# -- the device forms across streams ----------------------------------------------------------------------------------------------
DEVICE_SHAPES = ((17, 10, 5, 0), (40, 33, 11, 60))  # (nq, topk, nprobe, first query) of the two threads


@functools.lru_cache(maxsize=None)
def device_case(kind: str, masked: bool = False) -> list:
    """the two threads' `_device` searches of one handle: their own queries, another (nq, topk, nprobe) each and, masked,
    another row mask each"""
    c = case(kind)
    out = []
    for t, (nq, topk, nprobe, q0) in enumerate(DEVICE_SHAPES):
        mask = c.data["masks"]["half" if t == 0 else "sparse"] if masked else None
        v = Variant(f"thread{t}", "search_masked" if masked else "search", nq, topk, nprobe if c.ivf else 0, mask=mask, q0=q0)
        v.want = statement(c, v)
        out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def regrow_case(kind: str) -> tuple:
    """(small, big): a `_device` search of 3 queries and, for the host call that enters behind it, a filtered search that
    is larger in every workspace the two share: 130 queries, topk 1024, every list, a mask"""
    c = case(kind)
    small = Variant("small", "search", 3, 5, 1 if c.ivf else 0, q0=60)
    big = Variant("big", "search_masked", NQ, 1024, NLIST if c.ivf else 0, mask=c.data["masks"]["half"])
    for v in (small, big):
        v.want = statement(c, v)
    return small, big
