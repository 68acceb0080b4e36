"""The grid reduce of the pipelined screen (k_assign_screen_bf16_x32p, reduce_grid / fold_step) stated in numpy for one
row of X and held against the direct (minimum, second minimum, first index) of its 256 values.

A lane half h sees 8 tiles x 16 accumulator elements e of the row; element e of tile t is centroid
32 t + 8 (e >> 2) + 4 h + (e & 3).  Plain minima run on the untagged values -- per column class c = e & 7 over the step,
per row class rt = 2 t + (e >> 3) (or c = e & 3 and rt = 4 t + (e >> 2)) -- and only those 8 + 16 (4 + 32) minima take a tag in their low 6 bits and enter a
(minimum, second minimum) chain.  The lane's result is (row chain's minimum, min of the two chains' second minima,
centroid from the two winners' tags); the two lane halves merge as in the kernel's tail (tie to the lower centroid).

What the screen needs from it: with a clear gap the index is exact and both minima are the true ones up to the 6 masked
bits; without one, second - first stays within the packing budget (two values, each moved by less than 64 ulps), so the
margin test fails and the row goes to the exact re-check."""
import numpy as np
import pytest

F = np.float32
MASK = np.uint32(0xFFFFFFC0)
NCS = [8, 4]  # the kernel's two grid shapes
PINF = F(np.inf)


def _tagged(v, tag):
    return ((v.view(np.uint32) & MASK) | np.uint32(tag)).view(F)


def _snan(x):
    return np.isnan(x) & ((np.ascontiguousarray(x).view(np.uint32) & np.uint32(0x00400000)) == 0)


def _min3(a, b, c):
    """v_min3_f32 in IEEE mode: quiet NaN operands are ignored, a signalling NaN operand (a tagged +inf is one) or
    three NaNs give NaN."""
    nan = [np.isnan(x) for x in (a, b, c)]
    m = np.minimum(np.minimum(np.where(nan[0], PINF, a), np.where(nan[1], PINF, b)), np.where(nan[2], PINF, c))
    bad = _snan(a) | _snan(b) | _snan(c) | (nan[0] & nan[1] & nan[2])
    return np.where(bad, F(np.nan), m).astype(F)


def _med3(a, b, c):  # v_med3_f32: any NaN operand -> min3
    with np.errstate(invalid="ignore"):
        med = np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))
    return np.where(np.isnan(med), _min3(a, b, c), med).astype(F)


def _lane_half(v, h, nc):
    """v: (B, 8, 16) values of lane half h -> (m1, m2, j), the kernel's order of operations (nc column classes)."""
    B = v.shape[0]
    inf = np.full(B, PINF, F)
    cm = [None] * nc
    rq1 = rq2 = ta = None
    for t in range(8):
        fin = v[:, t, :]
        if nc == 8:
            pr = []
            for hf in range(2):
                for c in range(4 * hf, 4 * hf + 4):
                    cm[c] = _min3(fin[:, c], fin[:, c + 8], inf) if t == 0 else _min3(cm[c], fin[:, c], fin[:, c + 8])
                r = _min3(fin[:, 8 * hf], fin[:, 8 * hf + 1], fin[:, 8 * hf + 2])
                r = _min3(r, fin[:, 8 * hf + 3], fin[:, 8 * hf + 4])
                r = _min3(r, fin[:, 8 * hf + 5], fin[:, 8 * hf + 6])
                r = _min3(r, fin[:, 8 * hf + 7], inf)
                pr.append(_tagged(r, 2 * t + hf))
            q = inf if t == 0 else rq1
            tt = _med3(q, pr[0], pr[1])
            rq1 = _min3(q, pr[0], pr[1])
            rq2 = tt if t == 0 else _min3(rq2, tt, inf)
        else:
            for hf in range(2):
                for c in range(4):
                    x, y = fin[:, 8 * hf + c], fin[:, 8 * hf + 4 + c]
                    cm[c] = _min3(x, y, inf) if (t == 0 and hf == 0) else _min3(cm[c], x, y)
                pr = []
                for w in range(2):
                    o = 8 * hf + 4 * w
                    r = _min3(fin[:, o], fin[:, o + 1], fin[:, o + 2])
                    r = _min3(r, fin[:, o + 3], inf)
                    pr.append(_tagged(r, 4 * t + 2 * hf + w))
                q = inf if (t == 0 and hf == 0) else rq1
                tt = _med3(q, pr[0], pr[1])
                rq1 = _min3(q, pr[0], pr[1])
                if hf == 0:
                    ta = tt
                else:
                    rq2 = _min3(inf if t == 0 else rq2, ta, tt)
    pc = [_tagged(cm[c], 8 * (c >> 2) + (c & 3)) for c in range(nc)]
    c1, c2 = _min3(pc[0], pc[1], inf), _med3(pc[0], pc[1], inf)
    t1 = _med3(c1, pc[2], pc[3])
    c1 = _min3(c1, pc[2], pc[3])
    if nc == 8:
        t2 = _med3(c1, pc[4], pc[5])
        c1 = _min3(c1, pc[4], pc[5])
        c2 = _min3(c2, t1, t2)
        t1 = _med3(c1, pc[6], pc[7])
        c1 = _min3(c1, pc[6], pc[7])
    m2 = _min3(c2, t1, rq2)
    rt_mask, rt_shift = (15, 4) if nc == 8 else (31, 3)
    j = ((rq1.view(np.uint32) & np.uint32(rt_mask)) << np.uint32(rt_shift)) | (c1.view(np.uint32) & np.uint32(11)) | np.uint32(4 * h)
    return rq1, m2, j


def grid_reduce(vals, nc):
    """vals: (B, 256) values by centroid -> (m1, m2, j) of the row after the cross-half merge."""
    B = vals.shape[0]
    t, e, h = np.meshgrid(np.arange(8), np.arange(16), np.arange(2), indexing="ij")
    cen = 32 * t + 8 * (e >> 2) + 4 * h + (e & 3)           # (8, 16, 2)
    assert sorted(cen.ravel().tolist()) == list(range(256))
    a1, a2, ja = _lane_half(np.ascontiguousarray(vals[:, cen[:, :, 0]]), 0, nc)
    b1, b2, jb = _lane_half(np.ascontiguousarray(vals[:, cen[:, :, 1]]), 1, nc)
    pinf, ninf = np.full(B, PINF, F), np.full(B, -PINF, F)
    hi = _med3(a1, b1, pinf)
    lo2 = _med3(a2, b2, ninf)
    m2 = _med3(lo2, hi, ninf)
    take = (b1 < a1) | ((b1 == a1) & (jb < ja))
    return np.where(take, b1, a1), m2, np.where(take, jb, ja)


def direct(vals):
    j = np.argmin(vals, axis=1)                              # first index of the minimum
    s = np.sort(vals, axis=1)
    return s[:, 0], s[:, 1], j


def _same_but_tag(got, want):
    return (got.view(np.uint32) & MASK) == (np.ascontiguousarray(want).view(np.uint32) & MASK)


def _ulps(a, b):  # a, b > 0 in one binade here
    return a.view(np.uint32).astype(np.int64) - np.ascontiguousarray(b).view(np.uint32).astype(np.int64)


_W, _R = np.divmod(np.arange(256 * 256), 256)
PAIRS = np.stack([_W[_W != _R], _R[_W != _R]], axis=1)        # every (winner, runner-up) position: 256 x 255
assert PAIRS.shape == (256 * 255, 2)


def _rows(pairs, win, run, rest_lo, rest_hi, seed=0, k=256):
    rng = np.random.default_rng(seed)
    vals = rng.uniform(rest_lo, rest_hi, (len(pairs), 256)).astype(F)
    vals[:, k:] = F(3.0e38)
    idx = np.arange(len(pairs))
    vals[idx, pairs[:, 1]] = run
    vals[idx, pairs[:, 0]] = win
    return vals


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_clear_gap_every_winner_and_runner_up(sign, nc):
    """Every (winner, runner-up) pair of positions with a clear gap: index exact, both minima exact up to the 6 tag bits."""
    if sign > 0:
        vals = _rows(PAIRS, F(0.25), F(0.5), 1.0, 2.0)
    else:
        vals = _rows(PAIRS, F(-2.0), F(-1.5), -1.0, 1.0)
    m1, m2, j = grid_reduce(vals, nc)
    d1, d2, dj = direct(vals)
    assert np.array_equal(dj, PAIRS[:, 0])
    assert np.array_equal(j, dj)
    assert _same_but_tag(m1, d1).all()
    assert _same_but_tag(m2, d2).all()


@pytest.mark.parametrize("k_ulps,nc", [(u, 8) for u in range(0, 65)] + [(u, 4) for u in (0, 1, 2, 33, 63, 64)])
def test_ties_and_near_ties_stay_within_the_packing_budget(k_ulps, nc):
    """Runner-up equal to the winner or 1..64 ulps above it: the chains may name different cells, but second - first is
    at most the true gap plus two tag perturbations (< 64 ulps each) -- far below any margin, the row would be listed.
    The first minimum carries the row chain's tag and the second may carry a smaller column tag, so the difference can be
    negative by less than one perturbation.  Every pair of positions at 0 ulps, every 13th pair above."""
    pairs = PAIRS if k_ulps == 0 else PAIRS[k_ulps % 13::13]
    win = F(1.25)
    run = (np.array([win]).view(np.uint32) + np.uint32(k_ulps)).view(F)[0]
    vals = _rows(pairs, win, run, 4.0, 8.0, seed=k_ulps)
    m1, m2, j = grid_reduce(vals, nc)
    gap = _ulps(m2, m1)
    assert (gap > -64).all()
    assert (gap <= k_ulps + 128).all()
    assert _same_but_tag(m1, np.full(len(pairs), win, F)).all()
    # the named centroid is one of the two candidates whenever both chains agree on the cell; otherwise it is some
    # cell of the winner's row class and the runner-up's column class (or the reverse) -- any centroid index at all
    assert (j < 256).all()


@pytest.mark.parametrize("nc", NCS)
def test_all_nan_rows_are_listed(nc):
    vals = np.full((4, 256), np.nan, F)
    m1, m2, j = grid_reduce(vals, nc)
    # the minima keep the +inf they start from; a tagged +inf is a NaN pattern, so the result is +inf or NaN:
    # |m1| <= 3e38 fails either way and the row is listed
    with np.errstate(invalid="ignore"):
        assert not (np.abs(m1) <= F(3.0e38)).any()
        assert not (m2 - m1 > F(0.0)).any()
    assert (j < 256).all()


@pytest.mark.parametrize("nc", NCS)
def test_padding_centroids_k225(nc):
    """k = 225: centroids 225..255 are padding at 3e38; winner and runner-up at every pair of real positions."""
    pairs = PAIRS[(PAIRS[:, 0] < 225) & (PAIRS[:, 1] < 225)]
    vals = _rows(pairs, F(0.25), F(0.5), 1.0, 2.0, k=225)
    m1, m2, j = grid_reduce(vals, nc)
    d1, d2, dj = direct(vals)
    assert np.array_equal(j, dj) and (j < 225).all()
    assert _same_but_tag(m1, d1).all() and _same_but_tag(m2, d2).all()
    # a single real value next to the padding: second minimum is the padding value itself
    one = np.full((225, 256), F(3.0e38), F)
    one[np.arange(225), np.arange(225)] = F(7.0)
    m1, m2, j = grid_reduce(one, nc)
    assert np.array_equal(j, np.arange(225))
    assert _same_but_tag(m2, np.full(225, F(3.0e38), F)).all()


@pytest.mark.parametrize("nc", NCS)
def test_duplicates_in_three_or_more_cells(nc):
    rng = np.random.default_rng(5)
    B = 20_000
    vals = rng.uniform(4.0, 8.0, (B, 256)).astype(F)
    cnt = rng.integers(3, 9, B)
    for i in range(B):                                       # the minimum sits in 3..8 cells
        vals[i, rng.choice(256, cnt[i], replace=False)] = F(1.25)
    m1, m2, j = grid_reduce(vals, nc)
    assert _same_but_tag(m1, np.full(B, F(1.25), F)).all()
    gap = _ulps(m2, m1)
    assert (gap > -64).all() and (gap <= 128).all()
    # a unique winner over a runner-up value held by 3..8 cells: index and both minima exact
    win = rng.integers(0, 256, B)
    vals[np.arange(B), win] = F(0.25)
    m1, m2, j = grid_reduce(vals, nc)
    d1, d2, dj = direct(vals)
    assert np.array_equal(j, dj) and np.array_equal(j, win)
    assert _same_but_tag(m1, d1).all() and _same_but_tag(m2, d2).all()
