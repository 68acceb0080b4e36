"""numpy restatement of the reference's ScalarQuantizer / BinaryQuantizer arithmetic (src/sq.rs, src/bq.rs), every
operand f32, for the SQ / BQ tests (tests/test_sqbq_host.py, tests/test_gpu_sqbq.py, tools/sqbq_exhaustive.py)."""
import numpy as np

F = np.float32


def sq_step(mn, mx, levels) -> np.float32:
    with np.errstate(over="ignore"):
        return F(F(F(mx) - F(mn)) / F(levels - 1))  # (max - min) / (levels - 1) as f32


def round_half_away(r: np.ndarray) -> np.ndarray:
    """f32::round: half away from zero (floor(r + 0.5) is wrong at 0.49999997); NaN and +-inf pass through"""
    t = np.trunc(r)
    with np.errstate(invalid="ignore"):
        up = np.abs(r - t) >= F(0.5)
    return np.where(up, t + np.sign(r), t).astype(F)


def sq_encode(mn, mx, levels, x) -> np.ndarray:
    mn, mx = F(mn), F(mx)
    step = sq_step(mn, mx, levels)
    x = np.asarray(x, dtype=F)
    c = np.where(x < mn, mn, x)  # f32::clamp; a NaN stays NaN
    c = np.where(c > mx, mx, c).astype(F)
    with np.errstate(all="ignore"):
        r = round_half_away(((c - mn).astype(F) / step).astype(F))
    top = F(levels - 1)
    r = np.where(np.isnan(r), F(0), r)  # `as usize` saturates: NaN -> 0, +inf -> usize::MAX ...
    r = np.where(r >= top, top, r)      # ... then .min(levels - 1)
    return r.astype(np.uint8)


def sq_decode(mn, mx, levels, codes) -> np.ndarray:
    step = sq_step(mn, mx, levels)
    c = np.asarray(codes, dtype=np.uint8).astype(F)
    with np.errstate(all="ignore"):
        t = (c * step).astype(F)  # a multiply, then an add: never fused
        return (F(mn) + t).astype(F)


def bq_encode(threshold, low, high, x) -> np.ndarray:
    x = np.asarray(x, dtype=F)
    return np.where(x >= F(threshold), np.uint8(high), np.uint8(low)).astype(np.uint8)


def bq_decode(threshold, low, high, codes) -> np.ndarray:
    c = np.asarray(codes, dtype=np.uint8)
    return np.where(c >= np.uint8(high), F(high), F(low)).astype(F)


def nextafter32(x, direction) -> np.ndarray:
    return np.nextafter(np.asarray(x, dtype=F), F(direction)).astype(F)


# configurations the tests cover: ordinary ranges, two levels, step = inf, step = 0, subnormal ranges
SQ_CONFIGS = [
    (-1.0, 1.0, 5), (-1.0, 1.0, 256), (0.0, 1.0, 256), (0.0, 100.0, 256), (-1000.0, 1000.0, 256), (0.0, 1.0, 2),
    (-3e38, 3e38, 256),        # max - min overflows: step = inf
    (0.0, 1e-45, 3),           # step underflows to 0
    (1e-40, 3e-40, 256),       # subnormal range, subnormal step
    (-1e-38, 1e-38, 17),
    (0.0, 1.5e-43, 200),       # 1/step overflows: the direct kernel
]
