"""The two-operand A image of the three-product encode screen (k_assign_screen_bf16_x32p with NPR = 3): the image holds
the two rounded slices of -2(c - mu) once each and the third product a1.x2 reads operand 0 again.  A wrong operand there
(a2 where a1 belongs) is an error of 2^-8 |a||x| per dimension, far beyond the margin: it shows as wrong codes on the
N(0,1) and clustered rows, and -- deterministically -- in the NUMBER of rows the screen hands to the exact re-check.

Every case encodes seeded rows on the bf16 engine and on the exact engine and asks for equal codes, for three products,
and for the listed count (last_assign_stats()[0]) of the commit BEFORE the two-operand image, PARENT below: the screened
values are the same bits in both, so the counts are equal and not merely close.  (That is why sub_dim 14 stays on the
two tagged chains although the grid reduce now fits its registers: with untagged values the six 40 007-row cases of
each family listed one row more or fewer, profiles/NOTES.md.)
The constants are the output of tools/screen3_image_counts.py against a build of PARENT
(profiles/a_image64/parent_counts.txt); the test passes on PARENT as it stands.

Shapes: the smallest that take the pipelined form and can go wrong -- m = 2 and 3; n = 256 (one chunk of exactly eight
32-row steps), 288 (nine steps: an odd count, so a dummy step), 2 * 256 + 5 (ragged last step), 40 007 (many chunks);
k = 256 and 225 (padding centroids); squared L2 and Euclidean; sub_dim 16 and the padded 13, 14, 15 (row parts of 1, 2
and 1 floats); uniform, N(0,1) and clustered rows (0.05 around 40 centres, codebook of two Lloyd iterations: nearly
every row undecidable)."""
import functools

import numpy as np
import pytest

import oracle as O
from vq_amd import _lib

F = np.float32

PARENT = "69a1d26"
SDS = (16, 13, 14, 15)
FAMILIES = ("uniform", "normal", "clustered")
MS = (2, 3)
NS = (256, 288, 2 * 256 + 5, 40_007)
KS = (256, 225)
METRICS = (O.SQUARED_EUCLIDEAN, O.EUCLIDEAN)
N_MAX, M_MAX, N_TRAIN = max(NS), max(MS), 2048

# listed entries per case on PARENT: [sub_dim][family] -> counts in the order of cases()
PARENT_LISTED = {
    16: {
        "uniform": [0, 0, 3, 3, 0, 0, 3, 3, 3, 3, 5, 5, 229, 229, 207, 207, 1, 1, 3, 3, 1, 1, 3, 3, 5, 5, 7, 7, 333, 333, 308, 308],
        "normal": [3, 3, 2, 2, 3, 3, 2, 2, 4, 4, 4, 4, 328, 328, 262, 262, 3, 3, 3, 3, 3, 3, 3, 3, 6, 6, 6, 6, 486, 486, 423, 423],
        "clustered": [511, 511, 502, 502, 575, 575, 565, 565, 1030, 1030, 1008, 1008, 79991, 79991, 77946, 77946, 753, 753, 744, 744, 847, 847, 837,
                      837, 1515, 1515, 1499, 1499, 118026, 118026, 115957, 115957],
    },
    13: {
        "uniform": [1, 1, 3, 3, 4, 4, 4, 4, 5, 5, 6, 6, 231, 231, 230, 230, 1, 1, 4, 4, 4, 4, 5, 5, 5, 5, 7, 7, 348, 348, 344, 344],
        "normal": [0, 0, 3, 3, 0, 0, 3, 3, 1, 1, 6, 6, 347, 347, 330, 330, 1, 1, 5, 5, 1, 1, 5, 5, 2, 2, 8, 8, 487, 487, 489, 489],
        "clustered": [505, 505, 481, 481, 567, 567, 542, 542, 1013, 1013, 965, 965, 78946, 78946, 73696, 73696, 754, 754, 734, 734, 847, 847, 827,
                      827, 1520, 1520, 1479, 1479, 117938, 117938, 113674, 113674],
    },
    14: {
        "uniform": [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 234, 234, 203, 203, 1, 1, 3, 3, 1, 1, 3, 3, 1, 1, 6, 6, 369, 369, 327, 327],
        "normal": [2, 2, 3, 3, 2, 2, 3, 3, 3, 3, 5, 5, 307, 307, 292, 292, 3, 3, 3, 3, 3, 3, 3, 3, 4, 4, 5, 5, 462, 462, 446, 446],
        "clustered": [496, 496, 502, 502, 557, 557, 564, 564, 992, 992, 1015, 1015, 76923, 76923, 78920, 78920, 744, 744, 754, 754, 836, 836, 848,
                      848, 1494, 1494, 1525, 1525, 115911, 115911, 118896, 118896],
    },
    15: {
        "uniform": [1, 1, 0, 0, 1, 1, 0, 0, 3, 3, 2, 2, 259, 259, 196, 196, 2, 2, 0, 0, 3, 3, 0, 0, 6, 6, 2, 2, 370, 370, 309, 309],
        "normal": [4, 4, 2, 2, 4, 4, 2, 2, 7, 7, 5, 5, 338, 338, 312, 312, 4, 4, 2, 2, 5, 5, 2, 2, 8, 8, 5, 5, 471, 471, 455, 455],
        "clustered": [505, 505, 507, 507, 568, 568, 571, 571, 1024, 1024, 1023, 1023, 79975, 79975, 79961, 79961, 757, 757, 759, 759, 851, 851, 854,
                      854, 1534, 1534, 1532, 1532, 119961, 119961, 119941, 119941],
    },
}


def cases():
    return [(m, n, k, metric) for m in MS for n in NS for k in KS for metric in METRICS]


@functools.lru_cache(maxsize=None)
def _rows(family, sd):
    """(N_MAX, M_MAX * sd) rows of one family; a case takes the first n rows and the first m sub-vectors"""
    rng = np.random.default_rng(1000 * sd + FAMILIES.index(family))
    d = M_MAX * sd
    if family == "uniform":
        X = rng.random((N_MAX, d), dtype=F)
    elif family == "normal":
        X = rng.standard_normal((N_MAX, d), dtype=F)
    else:
        centres = F(3.0) * rng.standard_normal((40, d), dtype=F)
        pick = rng.integers(0, 40, N_MAX)
        X = centres[pick] + F(0.05) * rng.standard_normal((N_MAX, d), dtype=F)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _codebook(family, sd, k):
    """(M_MAX, k, sd): seeded draws of the rows' distribution; clustered: two Lloyd iterations (oracle) from k of the
    first N_TRAIN rows -- the centroids crowd around the 40 centres, so the runner-up is within the margin nearly always"""
    rng = np.random.default_rng(7000 * sd + 10 * k + FAMILIES.index(family))
    if family == "uniform":
        cb = rng.random((M_MAX, k, sd), dtype=F)
    elif family == "normal":
        cb = rng.standard_normal((M_MAX, k, sd), dtype=F)
    else:
        T = _rows(family, sd)[:N_TRAIN]
        cb = np.empty((M_MAX, k, sd), F)
        for s in range(M_MAX):
            sub = np.ascontiguousarray(T[:, s * sd:(s + 1) * sd])
            c = sub[[j * (N_TRAIN // k) + s for j in range(k)]]
            for _ in range(2):
                c = O.get().lloyd_step(sub, c)[0]
            cb[s] = c
    cb.setflags(write=False)
    return cb


def run_family(sd, family):
    """every case of (sub_dim, family): [(case, listed, products, engine, codes equal the exact engine's)]"""
    out = []
    for m in MS:
        for k in KS:
            cb = np.ascontiguousarray(_codebook(family, sd, k)[:m])
            for metric in METRICS:
                enc = _lib.PQEncoder(cb, metric)
                for n in NS:
                    X = np.ascontiguousarray(_rows(family, sd)[:n, :m * sd])
                    enc.set_engine(_lib.ENGINE_EXACT)
                    want, _ = enc.encode(X, want_f16=False)
                    enc.set_engine(_lib.ENGINE_MFMA_BF16)
                    codes, _ = enc.encode(X, want_f16=False)
                    listed, engine = _lib.last_assign_stats()
                    out.append(((m, n, k, metric), listed, _lib.last_screen_products(), engine, bool(np.array_equal(codes, want))))
                enc.close()
    order = {c: i for i, c in enumerate(cases())}
    out.sort(key=lambda r: order[r[0]])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("sd", SDS)
def test_two_operand_image_codes_and_listed_counts(sd, family):
    res = run_family(sd, family)
    listed = [r[1] for r in res]
    print(f"sub_dim {sd} {family}: listed {listed}")
    for case, _, products, engine, equal in res:
        assert engine == _lib.ENGINE_MFMA_BF16 and products == 3, (case, engine, products)
        assert equal, f"codes differ from the exact engine's at (m, n, k, metric) = {case}"
    if family != "uniform":  # the families whose screen has work to hand on: a wrong operand cannot hide in an empty list
        assert sum(listed) > 0
    assert listed == PARENT_LISTED[sd][family]
