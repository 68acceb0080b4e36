"""Expected-answer helpers for the 32-bit boundary tests (tests/test_gpu_big_offsets.py), checked at small scale by
tests/test_big_offsets_host.py.  Every helper takes the boundaries as parameters, so the host tests run the same code with
2^31 / 2^32 scaled down.

A boundary is a byte offset or an element index at which a product formed in 32 bits would wrap (2^31 for a signed
int, 2^32 for an unsigned one); it falls in the row that holds that byte or element.  A window is `half` rows on each
side of such a row, plus the first and last `half` rows of the array."""
import numpy as np

F = np.float32
B31, B32 = 1 << 31, 1 << 32


def boundary_rows(n, row_elems, elem_bytes, lo=B31, hi=B32, rows=True):
    """{name: row} of the rows < n that hold byte lo / hi, element lo / hi and (rows=True) row lo of an array of n rows
    of row_elems elements of elem_bytes bytes each"""
    out = {}
    for name, e in ((f"byte {lo:#x}", lo // elem_bytes), (f"byte {hi:#x}", hi // elem_bytes),
                    (f"element {lo:#x}", lo), (f"element {hi:#x}", hi)):
        if e // row_elems < n:
            out[name] = e // row_elems
    if rows and lo < n:
        out[f"row {lo:#x}"] = lo
    return out


def windows(n, rows, half=2048):
    """merged, sorted [r0, r1) ranges: half rows on each side of every row in `rows`, the first and the last half rows"""
    spans = [(0, min(n, half)), (max(0, n - half), n)] + [(max(0, r - half), min(n, r + half)) for r in rows]
    spans.sort()
    out = []
    for a, b in spans:
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def window_index(spans):
    """the row ids of every window, in order (int64)"""
    return np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in spans])


def sample_rows(n, count, seed):
    """a seeded, sorted sample of distinct row ids (int64)"""
    rng = np.random.default_rng(seed)
    if count >= n:
        return np.arange(n, dtype=np.int64)
    return np.unique(rng.integers(0, n, size=int(count * 1.05) + 16, dtype=np.int64))[:count]


# ---- ADC search with planted rows ----
# Codebook of subspace s, centroid j: (v_j, 0, ..., 0), v_0 = 0, v_j = 1 + j / 1024.  Against the zero query the squared-L2
# table is t[s][j] = v_j^2 (exact in f32 for the j used here).  Every row that is not planted has all its codes >= 1: its
# distance is >= m >= 2.  Planted row p (p = 0, 1, ...) has code 0 everywhere except code 1 + p in the last subspace: its
# distance is v_{1+p}^2 < 2, increasing in p.  So the planted rows come first, in the order they were given.

def adc_codebooks(m, k, sd):
    cb = np.zeros((m, k, sd), F)
    cb[:, 1:, 0] = (F(1) + np.arange(1, k, dtype=F) / F(1024)).astype(F)
    return cb


def adc_table(cb):
    """t[s][j] for the zero query, squared L2: sum over the sub-vector of (0 - c)^2, sequential from t = 0"""
    m, k, sd = cb.shape
    t = np.zeros((m, k), F)
    for c in range(sd):
        d = (F(0) - cb[:, :, c]).astype(F)
        t = (t + d * d).astype(F) if c else (d * d).astype(F)
    return t


def adc_planted_codes(m, count):
    """the codes [count][m] of planted rows 0 .. count-1"""
    c = np.zeros((count, m), np.int64)
    c[:, m - 1] = 1 + np.arange(count)
    return c


def adc_planted_rows(n, rows, half_last=True):
    """the rows to plant, nearest first: the last row, then each boundary row and the row before it, highest first --
    so a search that dropped the rows past a boundary would lose its best answers"""
    out = [n - 1] if half_last else []
    for r in sorted(rows, reverse=True):
        for x in (r, r - 1):
            if 0 <= x < n and x not in out:
                out.append(x)
    return out


def adc_distances(table, codes):
    """D(q, i) = t[0][c_0] + t[1][c_1] + ... in f32, subspace 0 first (the scans' order); codes [r][m]"""
    codes = np.asarray(codes, np.int64)
    acc = table[0][codes[:, 0]].astype(F)
    for s in range(1, codes.shape[1]):
        acc = (acc + table[s][codes[:, s]]).astype(F)
    return acc


def beats(dist, rows, kth_dist, kth_row, exclude):
    """rows (with their distances) that are strictly ahead of the k-th result by (distance, row) and not in the result"""
    dist = np.asarray(dist, F)
    rows = np.asarray(rows, np.int64)
    ahead = (dist < kth_dist) | ((dist == kth_dist) & (rows < kth_row))
    ahead &= ~np.isin(rows, np.asarray(list(exclude), np.int64))
    return rows[ahead]


# ---- centroid statements over a column subset ----

def f64_sums(assign, cols, k):
    """(counts [k], f64 sums [k][cols]) of the rows of each cluster; exact in any order when every value is a multiple of
    2^-24 in [0, 1) and there are fewer than 2^29 rows"""
    a = np.asarray(assign).astype(np.int64)
    c = np.bincount(a, minlength=k)
    S = np.stack([np.bincount(a, weights=cols[:, t].astype(np.float64), minlength=k) for t in range(cols.shape[1])], 1)
    return c, S


def sequential_f32_means(assign, cols, k):
    """per non-empty cluster: its rows added in row order in f32, then divided by the count in f32 (the reference's mean,
    exact_update); empty clusters 0"""
    a = np.asarray(assign).astype(np.int64)
    c = np.bincount(a, minlength=k)
    xs = np.asarray(cols, F)[np.argsort(a, kind="stable")]
    ends = np.cumsum(c)
    out = np.zeros((k, cols.shape[1]), F)
    for j in np.nonzero(c)[0]:
        out[j] = np.cumsum(xs[ends[j] - c[j]:ends[j]], axis=0, dtype=F)[-1] / F(c[j])
    return out
