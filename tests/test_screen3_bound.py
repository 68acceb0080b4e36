"""The three-product form of the sub_dim-16 encode screen (k_assign_screen_bf16_x32p, NPR = 3), restated in numpy:

    v1 = RNE_bf16(v), v2 = RNE_bf16(v - v1)           two rounded slices of x' = x - mu and of a' = -2 (c - mu)
    s^ = MFMA(a1, x1; MFMA(a2, x1; MFMA(a1, x2; |c'|^2)))   ... in the kernel's order: pair 0 first, on C = |c'|^2

with the bit-exact model of v_mfma_f32_32x32x16_bf16 (tests/mfma_model.py; k-slots 0..7 = dimensions 0..7, the lower
lane half, 8..15 = dimensions 8..15).  The value must lie within the E that DESIGN.md "Screen soundness" states for this
form of the f64 value of |c'|^2 - 2 x'.c':

    E3 = (388 + 20 NMF + sd) u B' + 0.5e-35 (|x'| + |c'|) + 0.5e-37,   u = 2^-24, NMF = 3, sd = 16, B' = (|x'| + |c'|)^2

(388: the dropped products a2x2 + a1 rx + a2 rx + ra x, 3.02 * 2^-16 |a||x| per dimension, Cauchy-Schwarz, 2|c'||x'| <=
B'/2; 20 per MFMA: the accumulation bound the margins budget; sd: the sequential f32 |c'|^2; the absolute part: slices
below the normal range).  Nothing here is imported from the library."""
import numpy as np

from mfma_model import mfma_model_one

F = np.float32
U = 2.0 ** -24
SD, NMF = 16, 3
PAIR_A = (0, 1, 0)   # A slice of MFMA f
PAIR_X = (0, 0, 1)   # X slice of MFMA f


def rne_bf16(v):
    """float32 array -> float32 array holding the nearest bf16 (ties to even)"""
    u = np.asarray(v, F).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(F)


def split2(v):
    v = np.asarray(v, F)
    v1 = rne_bf16(v)
    with np.errstate(over="ignore", invalid="ignore"):
        v2 = rne_bf16((v - v1).astype(F))
    return v1, v2


def bf_bits(v):
    return (np.asarray(v, F).view(np.uint32) >> 16).astype(np.uint16)


def screen_value(x, c):
    """one (row, centroid) pair of centred f32 sub-vectors -> the screen's f32 value"""
    a = (F(-2.0) * c).astype(F)  # exact
    a_sl = [bf_bits(s) for s in split2(a)]
    x_sl = [bf_bits(s) for s in split2(x)]
    cn = F(-0.0)
    for t in range(SD):  # the prepare kernel's sequential f32 sum of squares
        cn = F(cn + F(c[t] * c[t]))
    acc = F(cn + F(0.0))
    for f in range(NMF):
        acc = mfma_model_one(a_sl[PAIR_A[f]], x_sl[PAIR_X[f]], acc)
    return acc


def _boundary_values(rng, count, exps):
    """f32 values one ulp either side of (and on) every bf16 rounding boundary, both signs: mantissa (t << 16) | 0x8000
    for each of the 128 kept-bit patterns t, at exponents drawn from `exps`"""
    pats = np.array([(t << 16) | (0x8000 + o) for t in range(128) for o in (-1, 0, 1)], np.uint32)
    idx = np.arange(count) % len(pats)                     # every pattern, in turn
    sign = ((np.arange(count) // len(pats)) & 1).astype(np.uint32)  # ... under both signs
    e = (rng.choice(exps, count) + 127).astype(np.uint32)
    bits = (sign << np.uint32(31)) | (e << np.uint32(23)) | pats[idx]
    return bits.astype(np.uint32).view(F)


def _cases():
    rng = np.random.default_rng(316)
    xs, cs = [], []

    def add(x, c):
        xs.append(np.asarray(x, F).reshape(-1, SD))
        cs.append(np.asarray(c, F).reshape(-1, SD))

    n = 3072  # 8 x 384 patterns x signs per block of 16-vectors
    near = np.arange(-3, 4)
    add(_boundary_values(rng, n * SD, near), rng.standard_normal((n, SD)))                       # boundary rows
    add(rng.standard_normal((n, SD)), _boundary_values(rng, n * SD, near))                       # boundary centroids
    add(_boundary_values(rng, n * SD, near), rng.permutation(_boundary_values(rng, n * SD, near)))  # both
    m = 4096  # magnitudes 2^-60 .. 2^60 within one sub-vector
    add(rng.standard_normal((m, SD)) * np.exp2(rng.integers(-60, 61, (m, SD))),
        rng.standard_normal((m, SD)) * np.exp2(rng.integers(-60, 61, (m, SD))))
    add(_boundary_values(rng, 1024 * SD, np.arange(-60, 61)), rng.standard_normal((1024, SD)) * np.exp2(rng.integers(-60, 61, (1024, SD))))
    t = 2048  # residuals (and whole slices) below the normal range: |v| in 2^-126 .. 2^-112, v - v1 down to 2^-149
    tiny = (rng.standard_normal((t, SD)) * np.exp2(rng.integers(-126, -111, (t, SD)))).astype(F)
    add(tiny, rng.standard_normal((t, SD)))
    add(rng.standard_normal((t, SD)), tiny)
    add(tiny, rng.permutation(tiny))
    add(_boundary_values(rng, 512 * SD, np.arange(-126, -118)), rng.standard_normal((512, SD)) * np.exp2(rng.integers(-20, 21, (512, 1))))
    r = 5120  # random ones: N(0,1), uniform, a row next to its centroid
    add(rng.standard_normal((r, SD)), rng.standard_normal((r, SD)))
    add(rng.random((r // 4, SD)) - 0.5, rng.random((r // 4, SD)) - 0.5)
    c = rng.standard_normal((r // 4, SD)).astype(F)
    add(c + (1e-4 * rng.standard_normal(c.shape)).astype(F), c)
    return np.concatenate(xs), np.concatenate(cs)


def test_two_slices_are_rounded_and_the_residual_is_exact():
    """|v - v1| <= 2^-8 |v| and |v - v1 - v2| <= 2^-16 |v| (+ half a bf16 subnormal ulp), v - v1 exact in f32"""
    rng = np.random.default_rng(5)
    v = np.concatenate([_boundary_values(rng, 384 * 2 * 8, np.arange(-126, 127)),
                        (rng.standard_normal(20000) * np.exp2(rng.integers(-100, 120, 20000))).astype(F)])
    v1, v2 = split2(v)
    d = v.astype(np.float64) - v1.astype(np.float64)
    assert np.all((v - v1).astype(F).astype(np.float64) == d)
    assert np.all(np.abs(d) <= 2.0 ** -8 * np.abs(v.astype(np.float64)))
    assert np.all(np.abs(d - v2.astype(np.float64)) <= 2.0 ** -16 * np.abs(v.astype(np.float64)) + 2.0 ** -134)
    assert np.all((v1.view(np.uint32) & 0xFFFF) == 0) and np.all((v2.view(np.uint32) & 0xFFFF) == 0)


def test_three_product_value_within_the_stated_error():
    X, C = _cases()
    assert len(X) >= 25_000
    x64, c64 = X.astype(np.float64), C.astype(np.float64)
    exact = (c64 * c64).sum(axis=1) - 2.0 * (x64 * c64).sum(axis=1)
    nx, nc = np.sqrt((x64 * x64).sum(axis=1)), np.sqrt((c64 * c64).sum(axis=1))
    E = (388.0 + 20.0 * NMF + SD) * U * (nx + nc) ** 2 + 0.5e-35 * (nx + nc) + 0.5e-37
    got = np.array([float(screen_value(X[i], C[i])) for i in range(len(X))])
    assert np.all(np.isfinite(got))
    err = np.abs(got - exact)
    worst = int(np.argmax(err / E))
    print(f"cases {len(X)}  max err / E = {err[worst] / E[worst]:.4f}  (case {worst})")
    assert np.all(err <= E), (worst, err[worst], E[worst])
