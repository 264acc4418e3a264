"""Two independent readings of the brute-force matcher's contract, held against each other on the CPU: the C oracle
(oracle/brisk_oracle_match.c, through oracle_lib) and the NumPy statement (match_plain).  Everything is compared as bytes,
on small shapes of every rule: empty images, masks, the isMaskedOut rule, the top-up entries of a k beyond what exists,
descriptor sizes with and without a truncated tail, and the strict `<` of the radius."""
import numpy as np
import pytest

import match_plain as P
import oracle_lib as O

DIMS = [16, 40, 64, 72, 80, 224]


def same_bytes(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == P.DMATCH
        assert g.tobytes() == w.tobytes(), (i, g, w)


def low(rng, n, dim):
    """low-entropy rows: many equal distances, so the (distance, image, train index) order is on trial"""
    return (rng.integers(0, 4, (n, dim), dtype=np.uint8) * 85).astype(np.uint8)


def both(q, train, ks=(), radii=(), masks=None):
    for k in ks:
        same_bytes(P.match_knn(q, train, k, masks), O.match_knn(q, train, k, masks))
    for r in radii:
        same_bytes(P.match_radius(q, train, r, masks), O.match_radius(q, train, r, masks))


def test_layouts_agree():
    assert P.DMATCH == O.DMATCH and P.DMATCH.itemsize == 16
    assert P.TOP_UP.view(np.uint32) == 0x4F000000


@pytest.mark.parametrize("dim", DIMS)
def test_distance(dim):
    rng = np.random.default_rng(dim)
    q = rng.integers(0, 256, (3, dim), dtype=np.uint8)
    t = rng.integers(0, 256, (37, dim), dtype=np.uint8)
    t[0], t[1] = q[0], ~q[0]
    dim16 = 16 * (dim // 16)
    for i in range(3):
        want = np.unpackbits(q[i, :dim16][None, :] ^ t[:, :dim16], axis=1).sum(axis=1)
        assert np.array_equal(P.hamming_row(q[i], t), want)
        assert np.array_equal(P.hamming_row(q[i], t, table=True), want)
        assert [O.hamming(q[i], t[j]) for j in range(37)] == list(want)
    assert P.hamming_row(q[0], t)[0] == 0 and P.hamming_row(q[0], t)[1] == 8 * dim16     # bytes behind dim16 are ignored


@pytest.mark.parametrize("dim", DIMS)
def test_knn_and_radius_rules(dim):
    rng = np.random.default_rng(100 + dim)
    dim16 = 16 * (dim // 16)
    q = low(rng, 9, dim)
    e = np.zeros((0, dim), np.uint8)
    a, b, c = low(rng, 7, dim), low(rng, 5, dim), low(rng, 1, dim)
    a[3], b[2], b[4], a[6] = q[0], q[0], q[1], b[0]          # distance 0 in two images; one descriptor in two images
    q[8], c[0] = 0, 255                                      # the largest distance there is: 8 * dim16
    some = float(P.hamming_row(q[2], a)[1])                  # exactly a distance that occurs
    radii = (0.0, 0.5, some, some + 0.5, float(8 * dim16), 8 * dim16 + 0.5, -1.0, float("inf"), float("nan"))
    for train in ([a, b, c], [e, a, b, c], [a, e, e, b, c], [a, b, c, e], [e, e, c, e], [a], [e], []):
        nt = sum(len(t) for t in train)
        both(q, train, ks=(0, 1, 2, 3, nt, nt + 1, nt + 4), radii=radii)
    assert [len(r) for r in P.match_radius(q[8:], [c], float(8 * dim16))] == [0]
    assert [len(r) for r in P.match_radius(q[8:], [c], 8 * dim16 + 0.5)] == [1]
    top = P.match_knn(q[:1], [c, e], 3)[0]
    assert list(top["distance"][1:]) == [2147483648.0] * 2 and list(top["imgIdx"]) == [0, 0, 0] and list(top["trainIdx"]) == [0, 0, 0]


@pytest.mark.parametrize("dim", [16, 72])
def test_mask_rules(dim):
    rng = np.random.default_rng(200 + dim)
    q = low(rng, 8, dim)
    e = np.zeros((0, dim), np.uint8)
    a, b = low(rng, 6, dim), low(rng, 9, dim)
    ma = (rng.random((8, 6)) > 0.4).astype(np.uint8)              # value 1
    mb = (rng.random((8, 9)) > 0.4).astype(np.uint8) * 255        # value 255
    ma[2], mb[2] = 0, 0                                           # all-zero row in every image: query 2 is masked out
    ma[5] = 0                                                     # ... in one image only: query 5 stays
    mb[5, 0], mb[5, 1:] = 255, 0
    ma[6], mb[6] = 0, 0
    mb[6, 8] = 7                                                  # one entry (any non-zero value) keeps query 6
    me = np.zeros((8, 0), np.uint8)
    radii = (0.5, float(dim * 2), 1e9)
    for train, masks in (([a, b], [ma, mb]), ([a, b], [ma, None]), ([a, b], [None, mb]), ([a, b], [None, None]),
                         ([a, b, e], [ma, mb, me]), ([e, a, b], [me, ma, mb]), ([a, e, b], [ma, None, mb]),
                         ([a, e, b], [ma, me, mb]), ([a], [ma]), ([e], [me]), ([a, b], None)):
        both(q, train, ks=(0, 1, 3, 15, 16, 20), radii=radii, masks=masks)
    assert [len(r) for r in P.match_knn(q, [a, b], 3, [ma, mb])] == [3, 3, 0, 3, 3, 3, 3, 3]
    assert [len(r) for r in P.match_knn(q, [a, b], 3, [ma, None])] == [3] * 8
    assert [len(r) for r in P.match_knn(q, [a, b, e], 3, [ma, mb, me])] == [3] * 8   # an empty image is not counted
    six = P.match_knn(q, [a, b], 3, [ma, mb])[6]
    assert list(six["trainIdx"]) == [8, 0, 0] and list(six["imgIdx"]) == [1, 1, 1] and list(six["distance"][1:]) == [2147483648.0] * 2


def test_rows_argument():
    rng = np.random.default_rng(7)
    q, a, b = low(rng, 12, 32), low(rng, 70, 32), low(rng, 65, 32)
    m = [None, (rng.random((12, 65)) > 0.5).astype(np.uint8)]
    rows = [0, 11, 5]
    same_bytes(P.match_knn(q, [a, b], 4, m, rows=rows), [O.match_knn(q, [a, b], 4, m)[i] for i in rows])
    same_bytes(P.match_radius(q, [a, b], 70.0, m, rows=rows), [O.match_radius(q, [a, b], 70.0, m)[i] for i in rows])
