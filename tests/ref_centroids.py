"""An f64 reference for the centroids of one Lloyd step, and the bound every update path must meet.

The reference's mean (src/core/vector.rs:368-384) adds a cluster's members in row order in f32 and divides in f32.
`exact_update` reproduces those bits and is tested for bit equality.  The default update sums the rows in chunks and
combines the chunk partials in f64, so its bits differ.  This module says how far they may differ: given the rows of
one subspace, the final assignment (already asserted equal to the oracle's) and the library's centroids, it computes
per (cluster j, dimension t), in extended precision,

    c  = members of j,   mu = (sum of x over the members) / c,   A = sum of |x| over the members

and checks

    |c_gpu - mu| <= (1 + 2^-20) * u * (L * A / c + |mu|) + 2^-35 * A / c + F,      u = 2^-24,
    F = r * 2^-150 / c + 2^-150.

Why the bound holds (in the manner of DESIGN "Screen soundness")
------------------------------------------------------------------
1. Every path splits a cluster's members into chunk partials.  A partial is either an f32 chain (rows added one at a
   time, or in any tree, inside one chunk of at most R rows) or an f64 sum rounded to f32 once.  An f32 sum of l terms,
   in any order, is off by at most gamma_{l-1} * (sum of |x| over those terms), gamma_n = n*u / (1 - n*u) [Higham,
   Accuracy and Stability of Numerical Algorithms, Th. 4.2 and (4.6)].  An f64 sum rounded once is off by at most
   u * |partial| + (2^-53 terms).  So every partial j_p with member mass A_p is off by at most gamma_{L-1} * A_p with
   L = min(c, R), or u * A_p when L = 1.  Summed over the partials: gamma_{L-1} * A.  For L <= 4096, gamma_{L-1} <= L * u;
   beyond, the code uses gamma_{L-1} itself.
2. The partials are added in f64: P partials cost at most P * 2^-53 * A, under 2^-36 * A for P < 2^17.  The reference
   here sums in 80-bit long double: c * 2^-64 * A, under 2^-47 * A.  Together, after the division by c, under
   2^-35 * A / c.
3. The mean is formed as (float)(sum / count) (one f64 divide, one rounding to f32) or, on the exact paths, as an f32
   divide of an f32 sum: either way at most u * |mu| (1 + 2^-29) plus what item 1 left, times 1 + u.  The factor
   1 + 2^-20 holds those second-order terms.
4. Subnormals: an f32 ADDITION whose result is subnormal is exact, but rounding an f64 partial or quotient to f32 in
   the subnormal range costs up to half the spacing, 2^-150, absolutely and not relative to the value.  A cluster has
   at most r such roundings of its partial sums (r <= c: each partial holds at least one member), each divided by c in
   the mean, and the mean itself is rounded once more: F.

L per path
----------
  * L = 1: each chunk partial is an f64 sum rounded to f32 once (the fused screen's `ds_add_f64` slabs);
  * L = min(c, R) for f32 chains of at most R rows (the `rows_per_*` functions below say where R comes from);
  * L = c (no chunk bound can be stated; the reference's own gamma_{c-1}): `R=None`.
A path that also adds re-checked rows in an f32 chain of their own (k_accumulate_listed) has L = max(its own L, the
rows that chain can hold): the caller passes R accordingly.

A centroid outside the bound means a member was lost, added twice, flushed, or divided in the wrong precision -- not
that the rows were merely added in another order.

`changed` (vector.rs:232-240: some |new - old| >= 1e-6 in a non-empty cluster) must equal the oracle's flag unless
some coordinate could fall on either side of the threshold: the library's value anywhere within this bound of mu (plus
the f32 rounding of the difference), the oracle's where it is.  Then either answer is right and `changed_expected`
says "ambiguous" -- unless another coordinate has moved past the threshold beyond doubt.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
SUB = 2.0 ** -150
EPSILON = float(F(1e-6))  # vector.rs:439, as the f32 the comparison uses


# ---- rows per chunk of each update path (how R follows from the launch geometry) ------------------------------------

def rows_per_owned_slab(n, m, k, sd, num_cus):
    """k_accumulate_owned (P4; the one-wave form too): plan_update's wave-owned branch (vq_amd/csrc/k_update.hip,
    plan_update, `owned_waves` / `owned_row_split` / `n_row_chunks = rc2 * split`) and launch_owned
    (`rows_per_chunk = ceil(n / chunks)`, each of `split` waves taking ceil(rows_per_chunk / split) of them)."""
    budget = 38912  # kLdsBudgetWords
    per_wave = (k * (sd + 1) + 3) & ~3
    w = min(budget // per_wave, 8)
    w_fit = w
    w = min(w, m)
    if w > 0:
        g = (m + w - 1) // w
        w = (m + g - 1) // g
    split = max(1, w_fit // w) if w > 0 else 1
    if w * split < 2:
        return None  # no owned plan: not this path
    sub_groups = (m + w - 1) // w
    per_cu = max(1, min(4, budget // (per_wave * w * split)))
    rc2 = max(1, num_cus * per_cu // sub_groups)
    max_rc = max(1, (n + 511) // 512)
    rc2 = max(1, min(rc2, (max_rc + split - 1) // split))
    rows_per_chunk = (n + rc2 - 1) // rc2
    return (rows_per_chunk + split - 1) // split


def rows_per_screen_chunk(n, m, sd, num_cus):
    """The fused screen's row chunk (P1 / P2): launch_one_x32 in vq_amd/csrc/k_screen_bf16.hip with ACC, G = 1, NT32 = 8
    (k in 225..256) or fewer tiles: want_waves = CUs * kWavesPerBlock(4) * (2 if x32_two_waves), capped at
    max(1, n_steps / 8) * m and at least m, rounded up to whole blocks; chunks = blocks * 4 / m; a chunk holds
    ceil(n_steps / chunks) steps of 32 rows.  Computed for one wave per SIMD: fewer, longer chunks than with two, so
    an upper bound whichever the shape gets."""
    n_steps = (n + 31) // 32
    want = num_cus * 4
    want = min(want, max(1, n_steps // 8) * m)
    want = max(want, m)
    blocks = (want + 3) // 4
    while blocks * 4 < m:
        blocks += 1
    chunks = max(1, blocks * 4 // m)
    return 32 * ((n_steps + chunks - 1) // chunks)


SM_ROWS = 64  # kSmRows, vq_amd/csrc/k_lloyd_small.hip: k_sm_assign's f32 partial of 64 consecutive rows (P6)


# ---- the reference and the bound --------------------------------------------------------------------------------------

def exact_means(X, assign, k):
    """X [n][sd] f32 (the subspace's columns), assign [n] -> (c [k] int, mu [k][sd] f64, A [k][sd] f64).  Sums in
    long double; mu of an empty cluster is 0."""
    X = np.asarray(X, dtype=F)
    assign = np.asarray(assign).astype(np.int64)
    n, sd = X.shape
    c = np.bincount(assign, minlength=k)[:k]
    order = np.argsort(assign, kind="stable")
    xs = X[order].astype(np.longdouble)
    starts = np.concatenate([[0], np.cumsum(c)[:-1]])
    S = np.zeros((k, sd), np.longdouble)
    Aa = np.zeros((k, sd), np.longdouble)
    ne = c > 0
    if n:
        S[ne] = np.add.reduceat(xs, starts[ne], axis=0)
        Aa[ne] = np.add.reduceat(np.abs(xs), starts[ne], axis=0)
    cd = np.maximum(c, 1).astype(np.longdouble)[:, None]
    mu = (S / cd).astype(np.float64)
    return c, mu, (Aa.astype(np.float64))


def bound(c, mu, A, R=None, r=None):
    """|c_gpu - mu| allowed per (cluster, dimension).  R: rows per f32 chain (None: L = c; 1: f64 partials rounded
    once); r: f32 roundings of a cluster's partials (default c, the most there can be)."""
    c = np.asarray(c, dtype=np.float64)
    L = c.copy() if R is None else np.minimum(c, float(R))
    L = np.maximum(L, 1.0)
    Lm1 = L - 1.0
    Lf = np.maximum(L, Lm1 / (1.0 - Lm1 * U))  # gamma_{L-1} / u, <= L for L <= 4096
    rr = c if r is None else np.asarray(r, dtype=np.float64)
    cc = np.maximum(c, 1.0)[:, None]
    Ac = A / cc
    return (1.0 + 2.0 ** -20) * U * (Lf[:, None] * Ac + np.abs(mu)) + 2.0 ** -35 * Ac + (rr[:, None] * SUB / cc + SUB)


def centroid_violations(X, assign, got, k, R=None, r=None):
    """Indices (cluster, dimension) of non-empty clusters whose centroid breaks the bound, and the worst ratio
    |got - mu| / bound (inf for a non-finite centroid)."""
    c, mu, A = exact_means(X, assign, k)
    B = bound(c, mu, A, R, r)
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got - mu)
    err = np.where(np.isfinite(err), err, np.inf)
    ne = (c > 0)[:, None] & np.ones_like(err, bool)
    bad = ne & ~(err <= B)
    ratio = np.where(ne, err / B, 0.0)
    return np.argwhere(bad), float(ratio.max()) if ratio.size else 0.0


def assert_centroids(X, assign, got, k, R=None, r=None, what=""):
    bad, worst = centroid_violations(X, assign, got, k, R, r)
    if len(bad):
        c, mu, A = exact_means(X, assign, k)
        j, t = bad[0]
        B = bound(c, mu, A, R, r)[j, t]
        raise AssertionError(f"{what}: {len(bad)} centroid components outside the f64 bound (worst |err|/bound = {worst:.3g}); "
                             f"first: cluster {j} dim {t}: got {float(np.asarray(got)[j, t])!r}, mean {mu[j, t]!r}, "
                             f"members {c[j]}, bound {B:.3g}, L from R={R}")


def changed_expected(X, assign, c_oracle, old, k, ch_oracle, R=None, r=None):
    """-> (expected flag, ambiguous).  Per coordinate of a non-empty cluster, the library's |new - old| lies within
    this path's bound (plus the f32 rounding of the difference) of |mu - old|, and the oracle's is |c_oracle - old|
    exactly.  A coordinate whose interval, joined with the oracle's value, lies wholly at or above the 1e-6 threshold
    sets the flag for both; one whose hull straddles it leaves the flag open: ambiguous, unless another coordinate
    already sets it."""
    c, mu, A = exact_means(X, assign, k)
    Bg = bound(c, mu, A, R, r)
    od = np.asarray(old, dtype=np.float64)
    co = np.asarray(c_oracle, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dm = np.abs(mu - od)
        slack = Bg * (1.0 + 4.0 * U) + 2.0 * U * (dm + Bg) + 2.0 * SUB
        lo = np.minimum(dm - slack, np.abs(co - od) * (1.0 - 2.0 * U))
        hi = np.maximum(dm + slack, np.abs(co - od) * (1.0 + 2.0 * U))
    ne = (c > 0)[:, None]
    moved = ne & (lo >= EPSILON)
    open_ = ne & ~moved & (hi >= EPSILON)
    if moved.any():
        return bool(ch_oracle), False
    return bool(ch_oracle), bool(open_.any())
