"""GPU tests of the drop-in brute-force matcher at the block and tile seams of its two implementations (brisk_match.hip): the
distance-matrix path (k_match_dist, k_match_masked_out, k_match_knn, k_match_radius) and the register-row path
(k_match_knn_fused, k_match_radius_pairs_one), through B.BruteForceMatcher and the four C entry points.

The expectation for whole results is the C oracle (oracle_lib); a sample of rows of every large case is also compared with the NumPy
statement of the contract (match_plain), so that the two cannot share a mistake (tests/test_match_plain.py holds them against each
other on the CPU).  Everything is compared as bytes.  Outputs are pre-filled with a sentinel: the device forms must leave every
entry behind a row's count, behind cap and behind the last query untouched; the host forms copy whole rows back, so there the
sentinel must stand behind the last query (the ABI promises nothing for a row's entries behind its count).

Every shape is a seam, stated as a parameter.  The quantities taken from the code, each derived by the formula beside it:
  qblock = 2^28 / (2 * dist_pitch), at least 64 queries, dist_pitch = nt rounded up to 64, plus 64      (match_host)
  MF_IDX_BITS = 22: a packed key of the register-row path holds train rows below 2^22                    (brisk_launch_match_*_fused)
  MR_BINS = 1 793 = 8 * 224 + 1 histogram bins of k_match_radius; 256 train rows x 32 queries per workgroup of k_match_dist, whose
  <8> / <28> word instantiations switch between 64 and 80 bytes; 64 lanes per query in k_match_knn / k_match_radius; 16 wave
  slices of ceil(nt / 16) rows in k_match_knn_fused."""
import ctypes as C

import numpy as np
import pytest

from gpu_prefill import settled
import match_plain as P
import oracle_lib as O

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 3                      # spare rows behind the last query that must keep the sentinel
MF_IDX_BITS = 22
MF_WAVES = 16
MR_BINS = 8 * 224 + 1
assert MR_BINS == 1793 and MR_BINS - 1 == 1792


def dist_pitch_of(nt):
    return (nt + 63) // 64 * 64 + 64


def qblock_of(nt):
    """queries per pass of match_host's block loop: 2^28 bytes of u16 distances, never fewer than 64 queries"""
    return max((256 << 20) // (2 * dist_pitch_of(nt)), 64)


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    assert P.DMATCH == B.DMATCH == O.DMATCH
    return B


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0)
    yield c
    c.close()


def low(rng, n, dim):
    """low-entropy rows (bytes of {0, 85, 170, 255}): plenty of equal distances, the (distance, image, train index) order decides"""
    return (rng.integers(0, 4, (n, dim), dtype=np.uint8) * 85).astype(np.uint8)


def uni(rng, n, dim):
    return rng.integers(0, 256, (n, dim), dtype=np.uint8)


def same_rows(got, want, rows=None):
    """rows: `want` holds only these queries of `got`"""
    if rows is not None:
        got = [got[int(i)] for i in rows]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (i if rows is None else int(rows[i]), g, w)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_args(q, train, masks):
    q = np.ascontiguousarray(q, np.uint8)
    train = [np.ascontiguousarray(t, np.uint8) for t in train]
    n = len(train)
    tptr = (C.c_void_p * max(n, 1))(*[t.ctypes.data for t in train])
    ntr = np.array([len(t) for t in train] + [0], np.int32)
    tpitch = np.array([t.strides[0] if len(t) else q.shape[1] for t in train] + [0], np.int32)
    mptr, mpitch, keep = None, None, None
    if masks is not None:
        keep = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
        mptr = (C.c_void_p * max(n, 1))(*[None if m is None else m.ctypes.data for m in keep])
        mpitch = np.array([0 if m is None else m.strides[0] for m in keep] + [0], np.int32)
    return q, train, n, tptr, ntr, tpitch, mptr, mpitch, keep


def _host_outputs(nq, width):
    out = np.full((nq + PAD, max(width, 1), 4), SENTINEL, np.uint32)
    cnt = np.full(nq + PAD, SENTINEL, np.uint32)
    return out, cnt


def _host_rows(out, cnt, nq, width):
    assert (cnt[nq:] == SENTINEL).all() and (out[nq:] == SENTINEL).all(), "written behind the last query"
    counts = cnt[:nq].view(np.int32)
    recs = out.view(P.DMATCH).reshape(nq + PAD, -1)
    return counts, [recs[i, :min(int(counts[i]), width)].copy() for i in range(nq)]


def host_knn(ctx, q, train, k, masks=None):
    """brisk_hip_match_knn itself, into sentinel-filled outputs"""
    q, train, n, tptr, ntr, tpitch, mptr, mpitch, keep = _host_args(q, train, masks)
    nq = len(q)
    out, cnt = _host_outputs(nq, k)
    ctx.check(ctx._L.brisk_hip_match_knn(ctx._h, _p(q), nq, q.strides[0], q.shape[1], n, tptr, _p(ntr), _p(tpitch), mptr,
                                         None if mpitch is None else _p(mpitch), k, _p(out), _p(cnt)))
    counts, rows = _host_rows(out, cnt, nq, k)
    assert all(len(r) == c for r, c in zip(rows, counts))
    return rows


def host_radius(ctx, q, train, max_distance, cap, masks=None):
    """brisk_hip_match_radius itself: (counts found, the stored rows); cap = 0 goes with out = NULL"""
    q, train, n, tptr, ntr, tpitch, mptr, mpitch, keep = _host_args(q, train, masks)
    nq = len(q)
    out, cnt = _host_outputs(nq, cap)
    ctx.check(ctx._L.brisk_hip_match_radius(ctx._h, _p(q), nq, q.strides[0], q.shape[1], n, tptr, _p(ntr), _p(tpitch), mptr,
                                            None if mpitch is None else _p(mpitch), float(max_distance), cap,
                                            _p(out) if cap > 0 else None, _p(cnt)))
    if cap == 0:
        assert (out == SENTINEL).all()
    return _host_rows(out, cnt, nq, cap)


def radius_all(ctx, q, train, max_distance, masks=None):
    """every hit: a counting call (cap 0, no output), then one with the cap it asks for"""
    counts, _ = host_radius(ctx, q, train, max_distance, 0, masks)
    counts2, rows = host_radius(ctx, q, train, max_distance, max(int(counts.max()), 1), masks)
    assert np.array_equal(counts, counts2) and all(len(r) == c for r, c in zip(rows, counts))
    return rows


def check_cut(counts, rows, full, cap):
    """the radius contract under a cap: the count FOUND, and the first cap entries of the full order"""
    assert list(counts) == [len(f) for f in full]
    same_rows(rows, [f[:cap] for f in full])


class DevCall:
    """one device-form call: inputs uploaded with the given row pitches, sentinel-filled outputs, checked after the caller's sync"""

    def __init__(self, q, t, k_or_cap, q_pitch=None, t_pitch=None, t_offset=0):
        import torch
        self.nq, self.nt, self.dim, self.width = len(q), len(t), q.shape[1], k_or_cap
        self.q_pitch, self.t_pitch = q_pitch or self.dim, t_pitch or self.dim
        hq = np.full((max(self.nq, 1), self.q_pitch), 0xEE, np.uint8)
        hq[:self.nq, :self.dim] = q
        ht = np.full(t_offset + max(self.nt, 1) * self.t_pitch, 0xEE, np.uint8)
        ht[t_offset:].reshape(-1, self.t_pitch)[:self.nt, :self.dim] = t
        self.dq, self.dt_all = torch.from_numpy(hq).cuda(), torch.from_numpy(ht).cuda()
        self.t_ptr = self.dt_all.data_ptr() + t_offset
        self.out, self.cnt = settled(torch.full((self.nq + PAD, max(k_or_cap, 1), 4), SENTINEL, dtype=torch.int32, device="cuda"),
                                     torch.full((self.nq + PAD,), SENTINEL, dtype=torch.int32, device="cuda"))

    def knn(self, ctx, stream=0):
        ctx.check(ctx._L.brisk_hip_match_knn_device(ctx._h, self.dq.data_ptr(), self.nq, self.q_pitch, self.t_ptr, self.nt, self.t_pitch,
                                                    self.dim, self.width, self.out.data_ptr(), self.cnt.data_ptr(), stream))
        return self

    def radius(self, ctx, max_distance, stream=0):
        ctx.check(ctx._L.brisk_hip_match_radius_device(ctx._h, self.dq.data_ptr(), self.nq, self.q_pitch, self.t_ptr, self.nt,
                                                       self.t_pitch, self.dim, float(max_distance), self.width, self.out.data_ptr(),
                                                       self.cnt.data_ptr(), stream))
        return self

    def result(self):
        """(counts, the whole output as u32 [nq + PAD][width][4]) - call after a synchronise"""
        return self.cnt.cpu().numpy().view(np.uint32), self.out.cpu().numpy().view(np.uint32)

    def check(self, full):
        """full: the uncut rows expected; count = what was found, the first `width` stored, the sentinel everywhere else"""
        cnt, out = self.result()
        nq = self.nq
        assert (cnt[nq:] == SENTINEL).all() and (out[nq:] == SENTINEL).all(), "written behind the last query"
        assert list(cnt[:nq].view(np.int32)) == [len(f) for f in full]
        for i, f in enumerate(full):
            n = min(len(f), self.width)
            assert out[i, :n].tobytes() == f[:n].tobytes(), (i, out[i, :n].view(P.DMATCH), f[:n])
            assert (out[i, n:] == SENTINEL).all(), "query %d: written behind its %d entries" % (i, n)


def sync():
    import torch
    torch.cuda.synchronize()


# ---- tile, lane and word seams of the matrix path (host calls) -----------------------------------------------------------------

SEAM_NQ = [1, 31, 32, 33, 65]                         # the 32-query tile of k_match_dist: below, at, above, two tiles and one
SEAM_NT = [1, 63, 64, 65, 255, 256, 257, 513]         # the 64 lanes of k_match_knn / k_match_radius, the 256 train rows of k_match_dist


@pytest.mark.parametrize("dim", [16, 40, 64, 80, 224])   # 40 truncates to 32 bytes; 64 | 80 is k_match_dist<8> | <28>; 224 the widest
def test_matrix_seams(B, ctx, dim):
    rng = np.random.default_rng(1000 + dim)
    dim16 = 16 * (dim // 16)
    qs, ts = low(rng, max(SEAM_NQ), dim), low(rng, max(SEAM_NT), dim)
    ts[::50] = qs[0]                                  # equal rows (distance 0 for query 0) across lanes, tiles and images
    for nt in SEAM_NT:
        a = nt // 2                                   # two train images: the matrix path for every k
        train = [ts[:a], ts[a:nt]]
        bf = B.BruteForceMatcher(ctx)
        bf.add(train)
        for nq in SEAM_NQ:
            q = qs[:nq]
            # (nt = 1 leaves one image empty, which alone would take the register-row path for k = 1: a mask that allows everything bars it)
            masks = [np.zeros((nq, 0), np.uint8), np.full((nq, 1), 255, np.uint8)] if nt == 1 else None
            for k in (1, 3, nt, nt + 1):
                same_rows(bf.knnMatch(q, k, masks), O.match_knn(q, train, k, masks))
            for r in (0.5, 4.0 * dim16, 8 * dim16 + 0.5):        # 4 * dim16: the mean distance, about half the entries
                same_rows(bf.radiusMatch(q, r, masks), O.match_radius(q, train, r, masks))
        q = qs[:33]
        same_rows(bf.knnMatch(q, 3), P.match_knn(q, train, 3))
        same_rows(bf.radiusMatch(q, 4.0 * dim16), P.match_radius(q, train, 4.0 * dim16))


# ---- image boundaries on the 64-entry chunks ----------------------------------------------------------------------------------

def chunk_images(rng, dim):
    """70 train images whose cumulative offsets fall on 63, 64, 65, 128, 255, 256 and 257; empty ones leading, between and trailing"""
    offsets = [0, 0, 0, 63, 64, 65, 65, 128, 255, 256, 257, 257, 257]
    sizes = list(np.diff(offsets)) + [1, 2, 0, 3, 64, 5, 0, 0, 30, 7, 1] * 5 + [0, 0, 0]
    assert len(sizes) == 70
    train = [low(rng, int(n), dim) for n in sizes]
    cum = np.concatenate([[0], np.cumsum(sizes)])
    assert {63, 64, 65, 128, 255, 256, 257}.issubset(set(cum.tolist()))
    return train, sizes


def test_image_boundaries_on_chunks(B, ctx):
    dim, nq = 32, 40
    rng = np.random.default_rng(70)
    train, sizes = chunk_images(rng, dim)
    nt = int(sum(sizes))
    q = low(rng, nq, dim)
    same = q[3]                                        # one descriptor in several images, at several indices
    for i, j in ((2, 0), (2, 62), (3, 0), (4, 0), (6, 0), (6, 62), (7, 126), (8, 0), (9, 0), (16, 63), (20, 29), (66, 0)):
        assert sizes[i] > j
        train[i][j] = same
    bf = B.BruteForceMatcher(ctx)
    bf.add(train)
    few_hundred = 4.0 * dim                            # the mean distance: about half of the nt entries
    lens = [len(r) for r in O.match_radius(q, train, few_hundred)]
    assert 200 < min(lens) and max(lens) < nt
    rng_m = np.random.default_rng(71)
    full = [(rng_m.random((nq, n)) > 0.4).astype(np.uint8) * (255 if i % 2 else 1) for i, n in enumerate(sizes)]
    for m in full:
        m[7] = 0                                       # query 7 can match nothing: dropped where every image counts - none is empty
    for i in (2, 8, 20):
        full[i][9] = 0                                 # query 9 is barred from some images only
    some = [m if i % 3 else None for i, m in enumerate(full)]    # (an image without a mask keeps every query alive)
    for masks in (None, full, some):
        for k in (5, 1000):                            # 1000 > nt: top-up entries of the last non-empty image (66 - three empty ones trail)
            want = O.match_knn(q, train, k, masks)
            same_rows(bf.knnMatch(q, k, masks), want)
            same_rows(want, P.match_knn(q, train, k, masks))
        want = O.match_radius(q, train, few_hundred, masks)
        same_rows(bf.radiusMatch(q, few_hundred, masks), want)
        same_rows(want, P.match_radius(q, train, few_hundred, masks))
    rows = bf.knnMatch(q, 1000, full)                  # the empty images are not counted: query 7 stays, with top-up entries only
    assert nt < 1000 and len(rows[9]) == 1000 and rows[9][-1]["imgIdx"] == 66
    assert len(rows[7]) == 1000 and (rows[7]["distance"] == 2147483648.0).all() and (rows[7]["imgIdx"] == 66).all()
    assert len(bf.knnMatch(q, 5, some)[7]) == 5
    filled = [i for i, n in enumerate(sizes) if n]     # the same images without the empty ones: now query 7 is masked out
    train2, masks2 = [train[i] for i in filled], [full[i] for i in filled]
    bf2 = B.BruteForceMatcher(ctx)
    bf2.add(train2)
    for k in (5, 1000):
        want = O.match_knn(q, train2, k, masks2)
        same_rows(bf2.knnMatch(q, k, masks2), want)
        same_rows(want, P.match_knn(q, train2, k, masks2))
        assert [len(r) for r in want] == [0 if i == 7 else k for i in range(nq)]
    want = O.match_radius(q, train2, few_hundred, masks2)
    same_rows(bf2.radiusMatch(q, few_hundred, masks2), want)
    assert len(want[7]) == 0 and len(want[9]) > 0
    assert [int(i) for i in bf.knnMatch(q, 5)[3]["imgIdx"]] == [2, 2, 3, 4, 6]     # distance 0: image, then train index


# ---- the extremes of the distance ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [16, 40, 64, 80, 224])
def test_distance_extremes(B, ctx, dim):
    rng = np.random.default_rng(2000 + dim)
    dim16 = 16 * (dim // 16)
    top = 8 * dim16                                    # 224 bytes: 1 792, the last bin k_match_radius owns (MR_BINS - 1)
    if dim == 224:
        assert top == 1792 == MR_BINS - 1
    q = uni(rng, 5, dim)
    q[0] = 0
    a, b = uni(rng, 70, dim), uni(rng, 130, dim)
    a[69], b[64], b[129] = 255, 255, 255
    a[69, dim16:] = 0                                  # bytes behind the last full word do not count
    train = [a, b]
    bf = B.BruteForceMatcher(ctx)
    bf.add(train)
    for r in (float(top), top + 0.5, 1e9, 0.0, -1.0, float("inf"), float("nan")):
        want = O.match_radius(q, train, r)
        same_rows(radius_all(ctx, q, train, r), want)
        same_rows(bf.radiusMatch(q, r), want)
        same_rows(want, P.match_radius(q, train, r))
    far = [(0, 69), (1, 64), (1, 129)]
    at = radius_all(ctx, q, train, float(top))
    assert len(at[0]) == 197 and at[0]["distance"].max() < top               # strict: distance == max_distance is no hit
    for r in (top + 0.5, 1e9, float("inf")):
        row = radius_all(ctx, q, train, r)[0]
        assert len(row) == 200 and [(int(m["imgIdx"]), int(m["trainIdx"])) for m in row[-3:]] == far
        assert (row[-3:]["distance"] == np.float32(top)).all()
    for r in (0.0, -1.0, float("nan")):
        assert all(len(x) == 0 for x in radius_all(ctx, q, train, r))
    ones = [np.full((1, dim), 255, np.uint8), np.full((2, dim), 255, np.uint8)]
    for k in (1, 3):
        got = host_knn(ctx, q[:1], ones, k)
        same_rows(got, O.match_knn(q[:1], ones, k))
        same_rows(got, P.match_knn(q[:1], ones, k))
        assert (got[0]["distance"] == np.float32(top)).all()
    masks = [np.zeros((5, 70), np.uint8), np.ones((5, 130), np.uint8)]       # masked pairs (0xFFFF in the matrix) beside inf
    masks[0][:, 69] = 1
    want = O.match_radius(q, train, float("inf"), masks)
    same_rows(radius_all(ctx, q, train, float("inf"), masks), want)
    same_rows(want, P.match_radius(q, train, float("inf"), masks))
    assert [len(r) for r in want] == [131] * 5


# ---- the cut of the radius at cap ---------------------------------------------------------------------------------------------

CUT_CAP = 8
CUT_RADIUS = 10.0


def flips(base, bits):
    """a copy of `base` with the given bits inverted"""
    r = base.copy()
    for b in bits:
        r[b // 8] ^= 1 << (b % 8)
    return r


def cut_case(dim):
    """five queries against 512 train rows in two images (300 + 212).  Within CUT_RADIUS: query 0 has CUT_CAP - 1 hits, query 1
    CUT_CAP, query 2 CUT_CAP + 1 (scattered rows, distances 0 .. 3); query 3 has 64 hits of one distance that fill the 64-entry
    chunk [128, 192); query 4 has 151 hits of one distance over the three chunks [192, 384) - the running bins[d] of the placement
    loop; every other pair is far (random rows)."""
    rng = np.random.default_rng(3000 + dim)
    q, t = uni(rng, 5, dim), uni(rng, 512, dim)
    scattered = [3, 40, 90, 120, 193, 360, 410, 450, 500]                   # both images, many chunks, none of the rows used below
    for qi, n in ((0, CUT_CAP - 1), (1, CUT_CAP), (2, CUT_CAP + 1)):
        for j in range(n):
            t[scattered[j] + qi] = flips(q[qi], range(j % 4))
    for j in range(64):
        t[128 + j] = flips(q[3], (j, 64 + j))                               # distance 2, all different rows
    for j in range(151):
        t[200 + j] = flips(q[4], (j % 50, 50 + j % 50, 100 + j % 28))       # distance 3
    train = [t[:300], t[300:]]
    full = O.match_radius(q, train, CUT_RADIUS)
    assert [len(f) for f in full] == [CUT_CAP - 1, CUT_CAP, CUT_CAP + 1, 64, 151]
    assert set(full[3]["distance"]) == {2.0} and set(full[4]["distance"]) == {3.0}
    same_rows(full, P.match_radius(q, train, CUT_RADIUS))
    return q, t, train, full


@pytest.mark.parametrize("dim", [16, 64, 96])
def test_radius_cut_host(ctx, dim):
    q, t, train, full = cut_case(dim)
    for cap in (CUT_CAP, 1, 63, 64, 65, 150, 151, 152):
        counts, rows = host_radius(ctx, q, train, CUT_RADIUS, cap)
        check_cut(counts, rows, full, cap)
    counts, rows = host_radius(ctx, q, train, CUT_RADIUS, 0)                 # cap = 0, out = NULL: counts only
    assert list(counts) == [len(f) for f in full] and all(len(r) == 0 for r in rows)
    m = [np.ones((5, 300), np.uint8), np.ones((5, 212), np.uint8)]
    m[0][4, 210:220] = 0                                                      # ten of query 4's equal distances masked
    m[0][3], m[1][3] = 0, 0                                                   # query 3 masked out
    fullm = O.match_radius(q, train, CUT_RADIUS, m)
    assert [len(f) for f in fullm] == [CUT_CAP - 1, CUT_CAP, CUT_CAP + 1, 0, 141]
    for cap in (CUT_CAP, 140, 141):
        counts, rows = host_radius(ctx, q, train, CUT_RADIUS, cap, m)
        check_cut(counts, rows, fullm, cap)


@pytest.mark.parametrize("dim", [96, 224])                                    # the matrix path of the device form: more than 64 bytes
def test_radius_cut_device(ctx, dim):
    q, t, train, _ = cut_case(dim)
    full = O.match_radius(q, [t], CUT_RADIUS)                                 # the device form has one train set
    same_rows(full, P.match_radius(q, [t], CUT_RADIUS))
    calls = [DevCall(q, t, cap, q_pitch=dim + 16, t_pitch=dim + 32) for cap in (CUT_CAP, 1, 64, 150, 151, 152)]
    sync()
    for c in calls:
        c.radius(ctx, CUT_RADIUS)
    sync()
    for c in calls:
        c.check(full)


# ---- query blocks: q0 > 0 in match_host --------------------------------------------------------------------------------------

BLOCK_NT = 32704               # dist_pitch 32 768, so a block is 2^28 / (2 * 32 768) = 4 096 queries
BLOCK_NQ = [4096, 4097, 8193]  # one block; a last block of one query; three blocks
BLOCK_SPLIT = 20000            # rows of the first of the two train images
BLOCK_DEAD = (5, 4095, 4096, 8192)   # all-zero mask rows: inside a block, its last row, the first of the next, the last query
BLOCK_RADIUS = 45.0            # 16-byte random rows lie 64 +- 5.7 bits apart: a handful of the 32 704 is nearer than 45


class Blocks:
    """the data of the query-block tests and their references, each computed once (for the 8 193 queries: a query's row does not
    depend on the others, so the cases of fewer queries take a prefix) and never changed"""

    def __init__(self):
        assert dist_pitch_of(BLOCK_NT) == 32768 and qblock_of(BLOCK_NT) == 4096
        rng = np.random.default_rng(4000)
        self.q = uni(rng, max(BLOCK_NQ), 16)
        t = uni(rng, BLOCK_NT, 16)
        for i in (0, 4095, 4096, 4097, 8191, 8192):
            t[(i * 7) % BLOCK_NT] = self.q[i]                                  # a distance 0 for the rows at the block seams
        self.train = [t[:BLOCK_SPLIT], t[BLOCK_SPLIT:]]
        self._ref, self._masks = {}, None

    def masks(self, nq):
        if self._masks is None:
            m0 = np.full((max(BLOCK_NQ), BLOCK_SPLIT), 255, np.uint8)
            m1 = np.full((max(BLOCK_NQ), BLOCK_NT - BLOCK_SPLIT), 1, np.uint8)
            m0[:, ::7] = 0
            m1[:, 3::5] = 0
            m0[100:200] = 0                                                  # barred from one image only: alive
            m1[4097:4100, 64:] = 0
            for r in BLOCK_DEAD:
                m0[r], m1[r] = 0, 0
            m1[6], m0[6] = 0, 0
            m1[6, 12703] = 1                                                  # one entry, the last column of all, keeps query 6
            self._masks = [m0, m1]
        return [m[:nq] for m in self._masks]

    def ref(self, kind):
        if kind not in self._ref:
            nq = max(BLOCK_NQ)
            self._ref[kind] = {"knn": lambda: O.match_knn(self.q, self.train, 3),
                               "radius": lambda: O.match_radius(self.q, self.train, BLOCK_RADIUS),
                               "masked_knn": lambda: O.match_knn(self.q, self.train, 3, self.masks(nq)),
                               "masked_radius": lambda: O.match_radius(self.q, self.train, BLOCK_RADIUS, self.masks(nq))}[kind]()
        return self._ref[kind]

    def sample(self, nq):
        """at least 32 rows: the first and last of every block, the rows the masks single out, and a seeded draw"""
        qb = qblock_of(BLOCK_NT)
        rows = {q0 for q0 in range(0, nq, qb)} | {min(q0 + qb, nq) - 1 for q0 in range(0, nq, qb)}
        rows |= {r for r in BLOCK_DEAD + (6, 150, 4098) if r < nq}
        rows |= set(np.random.default_rng(nq).integers(0, nq, 32).tolist())
        assert len(rows) >= 32
        return sorted(rows)


@pytest.fixture(scope="module")
def blocks():
    return Blocks()


@pytest.mark.parametrize("nq", BLOCK_NQ)
def test_query_blocks_knn(ctx, blocks, nq):
    got = host_knn(ctx, blocks.q[:nq], blocks.train, 3)
    same_rows(got, blocks.ref("knn")[:nq])
    rows = blocks.sample(nq)
    same_rows(got, P.match_knn(blocks.q, blocks.train, 3, rows=rows), rows)
    assert all(got[i][0]["distance"] == 0 for i in (0, 4095, 4096, 8192) if i < nq)      # the twins planted for the rows at the seams


@pytest.mark.parametrize("nq", BLOCK_NQ)
def test_query_blocks_radius(ctx, blocks, nq):
    got = radius_all(ctx, blocks.q[:nq], blocks.train, BLOCK_RADIUS)
    want = blocks.ref("radius")[:nq]
    same_rows(got, want)
    rows = blocks.sample(nq)
    same_rows(got, P.match_radius(blocks.q, blocks.train, BLOCK_RADIUS, rows=rows), rows)
    hits = sum(len(r) for r in want)
    assert nq < hits < 64 * nq                                                 # a handful per query


@pytest.mark.parametrize("nq", BLOCK_NQ)
def test_query_blocks_masked_knn(ctx, blocks, nq):
    masks = blocks.masks(nq)
    got = host_knn(ctx, blocks.q[:nq], blocks.train, 3, masks)
    same_rows(got, blocks.ref("masked_knn")[:nq])
    rows = blocks.sample(nq)
    same_rows(got, P.match_knn(blocks.q[:nq], blocks.train, 3, masks, rows=rows), rows)
    dead = [r for r in BLOCK_DEAD if r < nq]
    assert nq - 1 in dead and [i for i in range(nq) if len(got[i]) == 0] == dead
    assert [(int(m["imgIdx"]), int(m["trainIdx"])) for m in got[6]] == [(1, 12703), (1, 0), (1, 0)]


def test_query_blocks_masked_radius(ctx, blocks):
    """(an all-zero row has no hit whether or not it is taken for masked out: what shows a wrong row of k_match_masked_out's answer
    here is a query with hits whose row WITHIN its block is a dead one of the first block - 4 096 + 5 and 4 096 + 4 095)"""
    nq = 8193
    masks = blocks.masks(nq)
    got = radius_all(ctx, blocks.q[:nq], blocks.train, BLOCK_RADIUS, masks)
    same_rows(got, blocks.ref("masked_radius")[:nq])
    rows = blocks.sample(nq)
    same_rows(got, P.match_radius(blocks.q[:nq], blocks.train, BLOCK_RADIUS, masks, rows=rows), rows)
    assert all(len(got[r]) == 0 for r in BLOCK_DEAD if r < nq)
    assert len(got[4096 + 5]) > 0 and len(got[4096 + 4095]) > 0


# ---- train sets of 2^22 rows: the clamp of the query block, and the index limit of the register-row path -------------------------

BIG = 1 << MF_IDX_BITS         # 1 << 22: the first row count a packed key cannot index


@pytest.fixture(scope="module")
def big_train():
    """2^22 random 16-byte rows (64 MB), made once and never changed.  The last rows repeat queries: the best match has the largest
    index.  Row 2^22 - 2 is the largest a key of the register-row path holds when nt = 2^22 - 1."""
    rng = np.random.default_rng(22)
    q = uni(rng, 65, 16)
    t = uni(rng, BIG, 16)
    t[BIG - 2] = q[0]
    t[BIG - 1] = q[1]
    t[BIG - 3] = flips(q[0], (5,))
    t[BIG - 4] = flips(q[1], (9, 77))
    t[BIG - 6] = flips(q[1], (3,))
    t[BIG - 5], t[1] = q[64], q[64]                                          # equal rows at both ends: the smaller index first
    t[BIG // 2 + 3] = q[63]
    return q, t


def test_query_block_clamp(ctx, big_train):
    """nt = 2^22: 2^28 / (2 * (2^22 + 64)) = 31 queries, clamped to 64 - blocks of 64 + 1 - and the best matches at the largest indices"""
    q, t = big_train
    nq, k = 65, 3
    assert qblock_of(BIG) == 64 and (256 << 20) // (2 * dist_pitch_of(BIG)) == 31
    train = [t[:5], t[5:]]                                                   # the second image alone has 2^22 - 5 rows
    got = host_knn(ctx, q[:nq], train, k)
    same_rows(got, O.match_knn(q[:nq], train, k))
    rows = [0, 1, 62, 63, 64] + list(range(2, 29))                            # 32 rows with both ends of both blocks
    assert len(set(rows)) == 32
    same_rows(got, P.match_knn(q[:nq], train, k, rows=rows), rows)
    assert [int(x) for x in got[0]["trainIdx"][:2]] == [BIG - 2 - 5, BIG - 3 - 5] and list(got[0]["imgIdx"]) == [1, 1, 1]
    assert [(int(m["imgIdx"]), int(m["trainIdx"])) for m in got[64][:2]] == [(0, 1), (1, BIG - 5 - 5)]


@pytest.mark.parametrize("nt", [BIG - 1, BIG])          # (1 << 22) - 1: the register-row path's last size; 1 << 22: the matrix path
def test_index_limit_knn(ctx, big_train, nt):
    q, t = big_train
    q, t = q[:2], t[:nt]
    want = O.match_knn(q, [t], 2)
    same_rows(want, P.match_knn(q, [t], 2))
    assert [int(x) for x in want[0]["trainIdx"]] == [BIG - 2, BIG - 3]
    assert int(want[1]["trainIdx"][0]) == (BIG - 1 if nt == BIG else BIG - 6)
    same_rows(host_knn(ctx, q, [t], 2), want)
    same_rows(host_knn(ctx, q, [np.zeros((0, 16), np.uint8), t], 2), O.match_knn(q, [np.zeros((0, 16), np.uint8), t], 2))
    call = DevCall(q, t, 2)
    sync()
    call.knn(ctx)
    sync()
    call.check(want)


@pytest.mark.parametrize("nt", [BIG - 1, BIG])
def test_index_limit_radius_device(ctx, big_train, nt):
    q, t = big_train
    q, t = q[:2], t[:nt]
    full = O.match_radius(q, [t], 36.0)                                       # 64 +- 5.7 bits: a few of the 2^22 lie below 36
    same_rows(full, P.match_radius(q, [t], 36.0))
    assert int(full[0]["trainIdx"][0]) == BIG - 2 and min(len(f) for f in full) >= 2
    calls = [DevCall(q, t, cap) for cap in (1, 2, 64)]
    sync()
    for c in calls:
        c.radius(ctx, 36.0)
    sync()
    for c in calls:
        c.check(full)


# ---- seams of the register-row k-NN kernel (k <= 2, one train set) ------------------------------------------------------------

FUSED_NT = [1, 2, 15, 16, 17, 31, 33, 1023, 1025]       # 16 wave slices of ceil(nt / 16) rows: empty slices below 16, a short last one
FUSED_NQ = [1, 63, 64, 65, 129]                         # 64 queries per workgroup: min(q, nq - 1) in the last one


def slice_rows(nt):
    """one row in each non-empty wave slice of k_match_knn_fused (the slice's last row)"""
    per = (nt + MF_WAVES - 1) // MF_WAVES
    return [min(w * per + per - 1, nt - 1) for w in range(MF_WAVES) if w * per < nt]


@pytest.mark.parametrize("dim", [16, 32, 48, 64])
def test_fused_seams(B, ctx, dim):
    rng = np.random.default_rng(5000 + dim)
    qs, ts = low(rng, max(FUSED_NQ), dim), low(rng, max(FUSED_NT), dim)
    e = np.zeros((0, dim), np.uint8)
    for nt in FUSED_NT:
        t = ts[:nt].copy()
        planted = slice_rows(nt)
        t[planted] = qs[0]                             # the same row in every wave slice: the smallest index wins, the next is second
        for nq in FUSED_NQ:
            q = qs[:nq]
            for k in (1, 2):                           # nt = 1, k = 2 leaves the register-row path: a top-up entry
                want = O.match_knn(q, [t], k)
                same_rows(host_knn(ctx, q, [t], k), want)
                if nq == 65:
                    same_rows(host_knn(ctx, q, [e, t, e], k), O.match_knn(q, [e, t, e], k))      # imgIdx 1, patched on the host
                    same_rows(want, P.match_knn(q, [t], k))
            if len(planted) > 1:
                assert [int(x) for x in want[0]["trainIdx"]] == planted[:2] and (want[0]["distance"] == 0).all()
    top = host_knn(ctx, qs[:3], [ts[:1]], 2)
    assert all(r[1]["distance"] == 2147483648.0 and r[1]["trainIdx"] == 0 for r in top)
    bf = B.BruteForceMatcher(ctx)
    bf.add(ts[:1025])
    same_rows(bf.knnMatch(qs, 2), O.match_knn(qs, [ts[:1025]], 2))


@pytest.mark.parametrize("dim", [16, 48, 64])
def test_fused_unaligned_train(ctx, dim):
    """the byte-wise train scan: base + 1 byte and pitch dim + 2 against the aligned layout of the same rows"""
    rng = np.random.default_rng(5100 + dim)
    q, t = low(rng, 129, dim), low(rng, 1025, dim)
    want = O.match_knn(q, [t], 2)
    calls = [DevCall(q, t, 2), DevCall(q, t, 2, q_pitch=dim + 3, t_pitch=dim + 2, t_offset=1), DevCall(q, t, 2, t_pitch=dim + 4)]
    assert calls[1].t_ptr % 4 == 1 and calls[0].t_ptr % 4 == 0
    sync()
    for c in calls:
        c.knn(ctx)
    sync()
    for c in calls:
        c.check(want)
    assert calls[0].result()[1].tobytes() == calls[1].result()[1].tobytes()


# ---- the matrix path of the device forms --------------------------------------------------------------------------------------

def test_device_knn_matrix(ctx):
    import torch
    rng = np.random.default_rng(6000)
    nt = 130
    stream = torch.cuda.Stream()
    cases = []
    q, t = low(rng, 70, 48), low(rng, nt, 48)
    t[::9] = q[2]
    for k in (3, 7, nt, nt + 1):                        # k >= 3; nt + 1: one top-up entry per row
        cases.append((DevCall(q, t, k, q_pitch=64, t_pitch=80), O.match_knn(q, [t], k)))
    for k in (3, 200):                                  # nt < k
        cases.append((DevCall(q, t[:2], k), O.match_knn(q, [t[:2]], k)))
    for k in (1, 2, 3):                                 # nt = 0: no entry, nothing written
        cases.append((DevCall(q, t[:0], k), O.match_knn(q, [t[:0]], k)))
        assert all(len(r) == 0 for r in cases[-1][1])
    cases.append((DevCall(q, t[:1], 2), O.match_knn(q, [t[:1]], 2)))          # nt = 1, k = 2 leaves the register-row path
    for dim in (80, 224):                               # k = 1 at sizes the register-row path is not built for
        qd, td = low(rng, 70, dim), low(rng, 300, dim)
        td[299] = qd[0]
        for k in (1, 2):
            cases.append((DevCall(qd, td, k, t_pitch=dim + 16), O.match_knn(qd, [td], k)))
    sync()
    for i, (c, _) in enumerate(cases):
        c.knn(ctx, stream.cuda_stream if i % 2 else 0)   # a caller's stream, and the context's
    sync()
    for c, want in cases:
        c.check(want)
    same_rows(cases[3][1], P.match_knn(q, [t], nt + 1))
    same_rows(cases[-1][1], P.match_knn(qd, [td], 2))


def test_device_workspace_grows_and_is_reused(B):
    """small -> large -> small on a fresh context and one caller's stream: the context's distance workspace grows (behind a device
    synchronise) and then serves a smaller call with another dist_pitch; nothing is read back before the third call is enqueued"""
    import torch
    rng = np.random.default_rng(6100)
    c = B.Context(0)
    try:
        stream = torch.cuda.Stream()
        shapes = [(40, 100, 3), (300, 2000, 5), (33, 30, 4)]
        assert len({dist_pitch_of(nt) for _, nt, _ in shapes}) == 3
        data = [(low(rng, nq, 32), low(rng, nt, 32), k) for nq, nt, k in shapes]
        knn = [DevCall(q, t, k) for q, t, k in data]
        rad = [DevCall(np.pad(q, ((0, 0), (0, 64))), np.pad(t, ((0, 0), (0, 64))), 40) for q, t, k in data]   # 96 bytes: the matrix path
        sync()
        for call in knn:
            call.knn(c, stream.cuda_stream)
        for call in rad:
            call.radius(c, 100.0, stream.cuda_stream)
        sync()
        for call, (q, t, k) in zip(knn, data):
            call.check(O.match_knn(q, [t], k))
        for call, (q, t, k) in zip(rad, data):
            call.check(O.match_radius(q, [t], 100.0))
    finally:
        c.close()


def test_forced_matrix_path_equals_register_rows(B):
    """debug flag 0x20000 (tuning library only) forces the matrix path for k <= 2: the same bytes from both implementations"""
    L = B.load_library()
    if not hasattr(L, "brisk_hip_debug_set_flags"):
        pytest.skip("debug_set_flags is unavailable: not the tuning library")
    rng = np.random.default_rng(6200)
    q, t = low(rng, 300, 48), low(rng, 1000, 48)
    c = B.Context(0)
    try:
        for k in (1, 2):
            want = O.match_knn(q, [t], k)
            results = []
            for flags in (0, 0x20000, 0):
                c.debug_set_flags(flags)
                host = host_knn(c, q, [t], k)
                same_rows(host, want)
                call = DevCall(q, t, k)
                sync()
                call.knn(c)
                sync()
                call.check(want)
                results.append((np.concatenate(host).tobytes(), call.result()[1].tobytes()))
            assert results[0] == results[1] == results[2]
    finally:
        c.debug_set_flags(0)
        c.close()
