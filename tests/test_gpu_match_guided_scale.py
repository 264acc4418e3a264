"""GPU tests of the six guided pair matchers (centre form, line form; k-NN, radius, mutual) where pair and row indices get wide: more
pairs than one launch holds with a model per pair, train rows beyond 2^16 and at the keys' limit 2^22 - 1 behind a guide, the mutual
forms' backward scan over slices of hundreds of staging blocks, and train keypoints planted on the closed bounds of centres that are
no grid points.  What tests/test_gpu_match_scale.py pins for the plain and gated matchers, for the code the guides add.

The expectation is never another entry point of the engine: a forward call is compared with the C oracle
(oracle/brisk_oracle_match.c) under the NumPy restatement of the guide's mask (test_gpu_match_guided.guide_mask,
test_gpu_match_epiline.epi_mask), a mutual call with test_abi_match_mutual.mutual_under_mask under the same mask.  Whole
sentinel-filled output arrays are compared as bytes - entries behind a count, rows behind pair_rows and bad pairs included: no
tolerance anywhere.

Every input is made by a case builder that needs NumPy alone (torch is imported inside the tests); every "the input reaches the case"
condition is a function of the restatement and is asserted both here and, without a GPU, by tests/test_match_guided_scale_cases.py."""
import itertools

import numpy as np
import pytest

from gpu_prefill import settled
import ethzasl_brisk_amd as B
import oracle_lib as O
from test_abi_match_epiline import RECTIFIED, cross, scaled
from test_abi_match_guided import PAIR_NO_MODEL, restated_centres
from test_abi_match_mutual import CENTRE, LINE, mutual_under_mask
from test_gpu_match_epiline import epi_mask, model_records as line_records
from test_gpu_match_gated import oracle_knn, oracle_radius
from test_gpu_match_guided import Kp, guide_mask, model_records as centre_records, upload_models
from test_gpu_match_mutual import compare as same_mutual
from test_gpu_match_pairs import SENTINEL, SynthSet, sentinel_outputs
from test_gpu_match_scale import BAD, LAUNCH, LIST, MANY_CAP, MANY_CPQ, MANY_RADIUS, NPAIRS, POOL_A, POOL_B, block, drawn_pairs, flipped, same_padded

pytestmark = pytest.mark.gpu

INF = float("inf")
IDX_BITS = 22                       # MF_IDX_BITS
LIMIT = (1 << IDX_BITS) - 1         # the most rows of a frame the keys hold
FAR = 1.0e6                         # where the keypoints lie that nothing may match
FORMS = {CENTRE: "centre", LINE: "line"}


@pytest.fixture(scope="module")
def lib():
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


# ---- what the builders share (NumPy only) -------------------------------------------------------------------------------------------

def keypoints(n, x=FAR, y=FAR, octave=1):
    k = np.zeros(n, B.KEYPOINT)
    k["x"], k["y"], k["octave"] = x, y, octave
    return k


def put(k, i, xy, octave=1):
    k["x"][i], k["y"][i], k["octave"][i] = xy[0], xy[1], octave


def records(form, models):
    return (line_records if form == LINE else centre_records)(B, models)


def mask_of(form, window, band, fallback, rec, kq, kt, step=1 << 18):
    """(M [n_a, n_b] uint8, has [n_a]) of one pair under the model record `rec`: guide_mask / epi_mask, evaluated `step` rows of the
    longer side at a time - their [n_a, n_b] float temporaries stay small"""
    def one(q, t):
        return epi_mask(window, band, fallback, rec, q, t) if form == LINE else guide_mask(window, fallback, rec, q, t)
    if max(len(kq), len(kt)) <= step:
        M, has = one(kq, kt)
        return np.ascontiguousarray(M, np.uint8), np.asarray(has, bool)
    if len(kt) >= len(kq):
        parts = [one(kq, kt[c:c + step]) for c in range(0, len(kt), step)]
        return np.ascontiguousarray(np.concatenate([p[0] for p in parts], axis=1), np.uint8), np.asarray(parts[0][1], bool)
    parts = [one(kq[r:r + step], kt) for r in range(0, len(kq), step)]
    return np.ascontiguousarray(np.concatenate([p[0] for p in parts], axis=0), np.uint8), np.concatenate([np.asarray(p[1], bool) for p in parts])


def mutual_want(M, has, dq, dt, b, rows_cap):
    """what test_gpu_match_mutual.compare takes for one pair: (n_a, train frame, f, distances, kept)"""
    ft, fd, kept, _ = mutual_under_mask(M, has, dq, dt, rows_cap)
    return len(dq), b, ft, fd, kept


def mutual_block(want, rows_cap):
    """the padded arrays of one pair of a mutual call: a kept row holds its record and count 1, a dropped row count 0 and the sentinel"""
    _, b, ft, fd, kept = want
    m, c = np.full((rows_cap, 1, 4), SENTINEL, np.int32), np.full(rows_cap, SENTINEL, np.int32)
    c[:len(kept)] = kept
    rec = m.reshape(-1).view(O.DMATCH)
    for q in np.flatnonzero(kept):
        rec[q] = (q, ft[q], b, np.float32(fd[q]))
    return m, c


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


# ---- the device side ----------------------------------------------------------------------------------------------------------------

class Frame:
    """one frame of descriptor rows and its keypoints in device memory, uploaded as they are"""

    def __init__(self, rows, kps):
        import torch
        rows = np.ascontiguousarray(rows, np.uint8)
        assert len(rows) == len(kps) and kps.dtype == B.KEYPOINT
        self.dim, n = rows.shape[1], len(rows)
        self.t_desc, self.t_cnt = torch.from_numpy(rows.reshape(-1)).cuda(), torch.tensor([n], dtype=torch.int32).cuda()
        self.t_kps = torch.from_numpy(np.ascontiguousarray(kps).view(np.uint8).copy()).cuda()
        self.set = B.DescSet(self.t_desc.data_ptr(), self.t_cnt.data_ptr(), 1, n * self.dim, self.dim, 1)
        self.kp = B.KpSet(self.t_kps.data_ptr(), n * B.KEYPOINT.itemsize)


def guide_of(form, window, band, fallback):
    gate = B.MatchGate(*window)
    return B.MatchEpipolarGuide(gate, band, fallback) if form == LINE else B.MatchGuide(gate, fallback)


def device_call(ctx, form, kind, Q, Qk, T, Tk, spec, npairs, d_models, guide, per, rows_cap, dim, radius=None):
    """one call of the six into sentinel-filled arrays; kind: "knn" (per = k), "radius" (per = cap_per_query), "mutual" (per = 1).
    Returns the device triple"""
    import torch
    out = sentinel_outputs(npairs, rows_cap, per)
    kw = dict(rows_cap=rows_cap, query_kps=Qk, train_kps=Tk, dim_bytes=dim, out=out)
    torch.cuda.synchronize()
    if kind == "knn":
        (ctx.match_knn_pairs_epipolar_guided if form == LINE else ctx.match_knn_pairs_guided)(Q, T, spec, per, d_models, guide, **kw)
    elif kind == "radius":
        (ctx.match_radius_pairs_epipolar_guided if form == LINE else ctx.match_radius_pairs_guided)(Q, T, spec, radius, per, d_models, guide, **kw)
    else:
        assert per == 1
        (ctx.match_mutual_pairs_epipolar_guided if form == LINE else ctx.match_mutual_pairs_guided)(Q, T, spec, d_models, guide, **kw)
    torch.cuda.synchronize()
    return out


def host(out):
    return tuple(t.cpu().numpy() for t in out)


def list_spec(plist):
    """(PairSpec, the tensor that keeps the device list alive)"""
    import torch
    keep = torch.from_numpy(np.ascontiguousarray(np.array(plist, np.int32).reshape(-1, 2))).cuda()
    return B.PairSpec(len(keep), 0, 0, 0, 0, keep.data_ptr()), keep


# ---- 1: more than 65 535 pairs in one call, a model per pair -------------------------------------------------------------------------

TRANSLATION = (1.0, 0.0, 8.0, 0.0, 1.0, -8.0, 0.0, 0.0, 1.0)
PERSPECTIVE = (2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.015625, 0.0, 1.0)          # centre = (2x, 2y) / (1 + x / 64): no grid point for x > 0
MANY_MODELS = {
    CENTRE: [(TRANSLATION, 0, 0), ((1.0, 0.0, -8.0, 0.0, 1.0, 8.0, 0.0, 0.0, 1.0), 7, 0x100), (PERSPECTIVE, 4095, 0x1), ((0.0,) * 9, 2, 0),
             (TRANSLATION, 3, PAIR_NO_MODEL), (TRANSLATION, -1, 0)],
    LINE: [(scaled(RECTIFIED, 0.5), 0, 0), (cross(24.0, 8.0), 7, 0x100), (scaled(RECTIFIED, -4.0), 4095, 0x1), ((0.0,) * 9, 2, 0),
           (scaled(RECTIFIED, 1.0), 3, PAIR_NO_MODEL), (scaled(RECTIFIED, 1.0), -1, 0)]}
USABLE, NMODELS = 3, 6               # ids 0 ... 2 guide; 3: the zero model (guided, no row has a centre or line); 4, 5: unguided
MANY_WINDOW = {CENTRE: (-16.0, 16.0, -8.0, 8.0, 1), LINE: (-24.0, 24.0, -16.0, 16.0, 1)}
MANY_BAND = 4.0
# the pairs at LAUNCH - 1, LAUNCH, LAUNCH + 1: the same frames under three models (the two scales of RECTIFIED give ONE mask, so
# the third is the zero model: rows with count 0)
SEAM_PAIR, SEAM_IDS = (4, 4), (0, 1, 3)
# mode -> (form, kind, entries per row, fallback)
MANY_MODES = {"guided_k2": (CENTRE, "knn", 2, 0), "guided_radius": (CENTRE, "radius", MANY_CPQ, 0), "epi_k2": (LINE, "knn", 2, 0),
              "epi_radius": (LINE, "radius", MANY_CPQ, 0), "mutual_centre": (CENTRE, "mutual", 1, 0), "mutual_line": (LINE, "mutual", 1, 0),
              "mutual_centre_fallback": (CENTRE, "mutual", 1, 1)}
KEY_MODES = {"guided_k1": (CENTRE, "knn", 1, 0), "mutual_line": (LINE, "mutual", 1, 0)}
KEY_FRAMES = (4, 2)                  # the keyframe form's one query frame and one train frame: the pool's frames of 5 rows


class Many:
    """the pool of 6 x 6 tiny frames, the drawn pair list and model ids, and what assembles a call's expected arrays from one restatement
    per distinct (a, b, model id): test_gpu_match_scale.Drawn with a model per pair"""

    def __init__(self):
        rng = np.random.default_rng(1907)
        self.descA = [(rng.integers(0, 4, (n, 16), dtype=np.uint8) * 85).astype(np.uint8) for n in POOL_A]
        self.descB = [(rng.integers(0, 4, (n, 16), dtype=np.uint8) * 85).astype(np.uint8) for n in POOL_B]
        for f in (1, 2, 3, 4, 5):                                    # the same descriptors in several frames: distance 0, ties
            k = min(2, len(self.descB[f]), len(self.descA[4]))
            self.descB[f][:k] = self.descA[4][:k]
        self.kA = [keypoints(n, 8.0 * rng.integers(0, 4, n), 8.0 * rng.integers(0, 3, n), rng.integers(0, 3, n)) for n in POOL_A]
        self.kB = [keypoints(n, 8.0 * rng.integers(0, 4, n), 8.0 * rng.integers(0, 3, n), rng.integers(0, 3, n)) for n in POOL_B]
        self.pairs = drawn_pairs()
        self.ids = rng.integers(0, NMODELS, NPAIRS).astype(np.int64)
        for i, p in enumerate((LAUNCH - 1, LAUNCH, LAUNCH + 1)):
            self.pairs[p], self.ids[p] = SEAM_PAIR, SEAM_IDS[i]
        nA, nB = len(POOL_A), len(POOL_B)
        pa, pb = self.pairs[:, 0].astype(np.int64), self.pairs[:, 1].astype(np.int64)
        self.good = (pa >= 0) & (pa < nA) & (pb >= 0) & (pb < nB)
        self.bad_slot = nA * nB * NMODELS
        self.slot = np.where(self.good, (pa * nB + pb) * NMODELS + self.ids, self.bad_slot)
        self.recs = {form: records(form, MANY_MODELS[form]) for form in (CENTRE, LINE)}
        self.model_list = {form: self.recs[form][self.ids] for form in (CENTRE, LINE)}      # the call's records, one per pair
        self.tables, self.key_tables = {}, {}

    def slot_of(self, a, b, mid):
        return (a * len(POOL_B) + b) * NMODELS + mid

    def one(self, mode, dq, dt, kq, kt, b, mid, modes=MANY_MODES):
        """(matches, counts) of one pair under model `mid`, and how many train rows its mask allows per stored query row"""
        form, kind, per, fallback = modes[mode]
        M, has = mask_of(form, MANY_WINDOW[form], MANY_BAND, fallback, self.recs[form][mid], kq, kt)
        rows = min(len(dq), MANY_CAP)
        allowed = [int(v) for v in M[:rows].sum(axis=1)] if M.size else [0] * rows
        if kind == "mutual":
            want = mutual_want(M, has, dq, dt, b, MANY_CAP)
            return mutual_block(want, MANY_CAP), allowed, [bool(k) for k, f in zip(want[4], want[2]) if f >= 0]
        want = oracle_knn(dq, dt, M, b, per) if kind == "knn" else oracle_radius(dq, dt, M, b, MANY_RADIUS)
        return block(want[:MANY_CAP], MANY_CAP, per), allowed, []

    def table(self, mode):
        """(matches, counts, pair_rows) per slot - every (a, b, model id), and the last slot for a bad entry - with what the masks
        allowed and, for a mutual mode, which rows with a forward match were kept"""
        if mode not in self.tables:
            per = MANY_MODES[mode][2]
            n = self.bad_slot + 1
            tm, tc = np.full((n, MANY_CAP, per, 4), SENTINEL, np.int32), np.full((n, MANY_CAP), SENTINEL, np.int32)
            tr = np.full(n, -1, np.int32)
            allowed, kept = [], []
            for a, b, mid in itertools.product(range(len(POOL_A)), range(len(POOL_B)), range(NMODELS)):
                s = self.slot_of(a, b, mid)
                (tm[s], tc[s]), al, kp = self.one(mode, self.descA[a], self.descB[b], self.kA[a], self.kB[b], b, mid)
                tr[s] = POOL_A[a]
                allowed, kept = allowed + al, kept + kp
            self.tables[mode] = (tm, tc, tr), allowed, kept
        return self.tables[mode]

    def key_table(self, mode):
        """the keyframe form: frame 0 of a one-frame set against frame 0 of another, (matches, counts) per model id"""
        if mode not in self.key_tables:
            a, b = KEY_FRAMES
            blocks = [self.one(mode, self.descA[a], self.descB[b], self.kA[a], self.kB[b], 0, mid, KEY_MODES)[0] for mid in range(NMODELS)]
            self.key_tables[mode] = np.stack([m for m, _ in blocks]), np.stack([c for _, c in blocks])
        return self.key_tables[mode]


def many_checks(many):
    """what the committed seed must give, on the list, the ids and the restatement alone"""
    assert len(many.pairs) == NPAIRS == LAUNCH + 70 and not many.good[list(BAD)].any() and many.good.sum() == NPAIRS - len(BAD)
    assert min(BAD) < LAUNCH - 1 and max(BAD) > LAUNCH + 1           # bad entries in both launches
    seam = [LAUNCH - 1, LAUNCH, LAUNCH + 1]
    assert len({tuple(many.pairs[p]) for p in seam}) == 1 and len({int(many.ids[p]) for p in seam}) == 3 and many.good[seam].all()
    assert sorted(np.unique(many.ids[many.good])) == list(range(NMODELS))
    late = np.flatnonzero(many.good & (np.arange(NPAIRS) >= LAUNCH))
    pa, pb = many.pairs[late, 0].astype(np.int64), many.pairs[late, 1].astype(np.int64)
    relative = (pa * len(POOL_B) + pb) * NMODELS + many.ids[late - LAUNCH]   # the slot a launch-relative model index would give
    assert len(late) == 70 - sum(p >= LAUNCH for p in BAD)
    for mode in MANY_MODES:
        (tm, tc, tr), allowed, kept = many.table(mode)
        blocks = [tm[many.slot[p]].tobytes() + tc[many.slot[p]].tobytes() for p in seam]
        assert len(set(blocks)) == 3, mode                          # the three pairs at the seam: three different expected blocks
        differ = [(tm[s].tobytes(), tc[s].tobytes()) != (tm[r].tobytes(), tc[r].tobytes()) for s, r in zip(many.slot[late], relative)]
        assert 4 * sum(differ) >= len(late), (mode, sum(differ), len(late))
        al = np.array(allowed)
        assert (al == 0).any() and (al == 1).any() and (al > 1).any(), (mode, np.bincount(al))
        if MANY_MODES[mode][1] == "mutual":
            assert 0 < sum(kept) < len(kept), (mode, sum(kept), len(kept))   # the backward scan keeps and drops
        unguided = [many.slot_of(a, b, mid) for a in range(6) for b in range(6) for mid in range(USABLE, NMODELS) if POOL_A[a]]
        written = int((tm[unguided] != SENTINEL).sum())
        assert (written > 0) == (MANY_MODES[mode][3] != 0), (mode, written)   # fallback 0: the unusable records give empty rows
    for mode in KEY_MODES:
        km, kc = many.key_table(mode)
        assert len({km[i].tobytes() + kc[i].tobytes() for i in SEAM_IDS}) == 3, mode     # a model id read wrongly shows
        assert (km[USABLE:] == SENTINEL).all() and (kc[USABLE:, :MANY_CAP] == 0).all()


class ManyDevice:
    def __init__(self, many):
        rng = np.random.default_rng(8)
        self.ctx = B.default_context(0)
        self.A = SynthSet(B, rng, 16, 16, POOL_A, 5, prepared=dict(enumerate(many.descA)))
        self.Bs = SynthSet(B, rng, 16, 20, POOL_B, 5, 4, 2, 8, prepared=dict(enumerate(many.descB)))
        self.Ak, self.Bk = Kp(B, many.kA, 5), Kp(B, many.kB, 5)
        self.spec, self.keep = list_spec(many.pairs)
        self.models = {form: upload_models(many.model_list[form]) for form in (CENTRE, LINE)}
        a, b = KEY_FRAMES
        self.key_q, self.key_t = Frame(many.descA[a], many.kA[a]), Frame(many.descB[b], many.kB[b])


@pytest.fixture(scope="module")
def many(lib):
    m = Many()
    many_checks(m)
    m.dev = ManyDevice(m)
    return m


def same_arrays(got, want, pairs):
    for name, g, w in zip(("pair_rows", "counts", "matches"), got[::-1], want[::-1]):
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
            p = int(bad[0])
            assert False, "%s: %d pairs differ, the first is %d = %s: got %s, want %s" % (name, len(bad), p, pairs[p], g[p].tolist(), w[p].tolist())


@pytest.mark.parametrize("mode", list(MANY_MODES))
def test_more_pairs_than_one_launch_a_model_per_pair(many, mode):
    form, kind, per, fallback = MANY_MODES[mode]
    (tm, tc, tr), _, _ = many.table(mode)
    d = many.dev
    out = device_call(d.ctx, form, kind, d.A.set, d.Ak.set, d.Bs.set, d.Bk.set, d.spec, NPAIRS, d.models[form],
                      guide_of(form, MANY_WINDOW[form], MANY_BAND, fallback), per, MANY_CAP, 16, radius=MANY_RADIUS)
    got = host(out)
    assert got[0].shape == (NPAIRS, MANY_CAP, per, 4)
    same_arrays(got, (tm[many.slot], tc[many.slot], tr[many.slot]), many.pairs)


@pytest.mark.parametrize("mode", list(KEY_MODES))
def test_the_keyframe_form_beyond_one_launch(many, mode):
    """PairSpec(65 605, 0, 0, 0, 0, None): every pair is frame 0 against frame 0, so pair p's arrays depend on models[p] alone"""
    form, kind, per, fallback = KEY_MODES[mode]
    km, kc = many.key_table(mode)
    d = many.dev
    out = device_call(d.ctx, form, kind, d.key_q.set, d.key_q.kp, d.key_t.set, d.key_t.kp, B.PairSpec(NPAIRS, 0, 0, 0, 0, None), NPAIRS,
                      d.models[form], guide_of(form, MANY_WINDOW[form], MANY_BAND, fallback), per, MANY_CAP, 16)
    rows = np.full(NPAIRS, POOL_A[KEY_FRAMES[0]], np.int32)
    same_arrays(host(out), (km[many.ids], kc[many.ids], rows), np.zeros((NPAIRS, 2), np.int32))


# ---- 2 (a): train indices beyond 2^16 behind a guide ---------------------------------------------------------------------------------

WIDE_NB, WIDE_NA = 70000, 65
WIDE_SLICE = 8750                    # ceil(70 000 / 8): a wave's rows; no multiple of MPG_CHUNK = 4, so every slice ends in a clamped chunk
WIDE_LIST_RADIUS, WIDE_DENSE_RADIUS = 46.5, 56.5
WIDE_CAPS = (16, 1024)               # cap_per_query below and above the hits of the crowded rows at WIDE_DENSE_RADIUS
WIDE_WINDOW = {CENTRE: (-16.0, 16.0, -8.0, 8.0, 1), LINE: (-16.0, 16.0, -INF, INF, 1)}
WIDE_BAND = 8.0                      # (RECTIFIED: |dy| <= 8)
WIDE_MODEL = {CENTRE: (TRANSLATION, 5, 0), LINE: (scaled(RECTIFIED, 2.0), 5, 0)}
CROWD_FROM = 30                      # query rows 30 ... 64 share one spot, whose window holds thousands of train keypoints


def image(form, xy):
    """where the model of the wide cases puts the window of a query keypoint at xy"""
    return (xy[0] + 8.0, xy[1] - 8.0) if form == CENTRE else xy


def wide_case(form):
    """65 query rows against 70 000 train rows (16 bytes, random).  Every planted query row has its own spot; the train rows the plan
    wants allowed lie in the window around the model's image of the spot (some exactly on its bounds), everything else far away:
      copy     rows 0 ... 4: an exact copy above index 65 536, allowed
      hidden   rows 5 ... 9: an exact copy above 65 536 that the guide forbids, and an allowed row at distance 3 above 65 536
      tie      rows 10 ... 14: two allowed rows at distance 3, one below and one above 65 536
      seam     rows 15, 16: three allowed rows at distance 4 at the last two rows of wave slice w - 1 and the first of slice w, w = 1, 7
      second   rows 17 ... 21: the best below, the second best above 65 536
      last     row 22: the best is the very last train row
      crowd    rows 30 ... 64 at one spot; every 20th train row lies around its image, some outside the window or octaves away"""
    rng = np.random.default_rng(2301 + form)
    t = rng.integers(0, 256, (WIDE_NB, 16), dtype=np.uint8)
    q = rng.integers(0, 256, (WIDE_NA, 16), dtype=np.uint8)
    kq, kt = keypoints(WIDE_NA), keypoints(WIDE_NB)
    spot = [(300.0 * i, 100.0 + 40.0 * (i % 5)) for i in range(WIDE_NA)]
    crowd_spot = (30000.0, 700.0)
    for i in range(WIDE_NA):
        put(kq, i, spot[i] if i < CROWD_FROM else crowd_spot)
    crowd = np.arange(7, WIDE_NB, 20)
    cx, cy = image(form, crowd_spot)
    kt["x"][crowd], kt["y"][crowd] = cx + rng.integers(-80, 81, len(crowd)) / 4.0, cy + rng.integers(-40, 41, len(crowd)) / 4.0
    kt["octave"][crowd] = rng.integers(0, 4, len(crowd))
    plan = {"copy": {}, "hidden": {}, "tie": {}, "seam": {}, "second": {}, "last": {}}
    corners = [(-16.0, -8.0), (16.0, 8.0), (0.0, 0.0), (16.0, -8.0), (-16.0, 8.0)]       # offsets on the window's closed bounds

    def allow(i, at, rows, n=0):
        c = image(form, spot[i])
        o = corners[(i + n) % len(corners)]
        put(kt, at, (c[0] + o[0], c[1] + o[1]), 1 + (i + n) % 2)
        t[at] = rows

    def forbid(at, rows):
        put(kt, at, (FAR, FAR))
        t[at] = rows

    for i in range(5):
        plan["copy"][i] = 65536 + 700 * i + 3
        allow(i, plan["copy"][i], q[i])
    for i in range(5, 10):
        plan["hidden"][i] = (65536 + 410 * i + 3, 67100 + i)
        forbid(plan["hidden"][i][0], q[i])
        allow(i, plan["hidden"][i][1], flipped(q[i], [4, 5, 6]))
    for i in range(10, 15):
        plan["tie"][i] = (100 + i, 66000 + i)
        allow(i, 100 + i, flipped(q[i], [1, 2, 3]))
        allow(i, 66000 + i, flipped(q[i], [9, 70, 127]), 1)
    for i, w in ((15, 1), (16, 7)):
        plan["seam"][i] = [WIDE_SLICE * w - 2, WIDE_SLICE * w - 1, WIDE_SLICE * w]
        for n, at in enumerate(plan["seam"][i]):
            allow(i, at, flipped(q[i], [8 * n, 8 * n + 1, 100 + n, 120 + n]), n)
    for i in range(17, 22):
        plan["second"][i] = (200 + i, 69000 + i)
        allow(i, 200 + i, flipped(q[i], [5]))
        allow(i, 69000 + i, flipped(q[i], [7, 8]), 1)
    plan["last"][22] = WIDE_NB - 1
    allow(22, WIDE_NB - 1, flipped(q[22], [0]))
    model = records(form, [WIDE_MODEL[form]])[0]
    return {"form": form, "q": q, "t": t, "kq": kq, "kt": kt, "model": model, "plan": plan}


def wide_wants(case):
    """the oracle's rows of every mode under the restated mask, with the assertions that they reach the cases"""
    form, q, t, plan = case["form"], case["q"], case["t"], case["plan"]
    M, has = mask_of(form, WIDE_WINDOW[form], WIDE_BAND, 0, case["model"], case["kq"], case["kt"])
    assert has.all()
    w = {1: oracle_knn(q, t, M, 0, 1), 2: oracle_knn(q, t, M, 0, 2), "list": oracle_radius(q, t, M, 0, WIDE_LIST_RADIUS),
         "dense": oracle_radius(q, t, M, 0, WIDE_DENSE_RADIUS)}
    reported = np.concatenate([r["trainIdx"] for mode in w for r in w[mode]])
    for i, at in plan["copy"].items():
        assert M[i, at] and w[1][i][0]["trainIdx"] == at >= 65536 and w[1][i][0]["distance"] == 0
    for i, (hidden, shown) in plan["hidden"].items():               # the exact copy is forbidden and never reported
        assert not M[i, hidden] and hidden >= 65536 and hidden not in reported and np.array_equal(t[hidden], q[i])
        assert w[1][i][0]["trainIdx"] == shown >= 65536 and w[1][i][0]["distance"] == 3
    for i, (low, high) in plan["tie"].items():                      # the same distance twice: the lower index comes first
        assert list(w[2][i]["trainIdx"]) == [low, high] and list(w[2][i]["distance"]) == [3, 3] and low < 65536 <= high
    assert WIDE_SLICE * 8 == WIDE_NB and WIDE_SLICE % 4 != 0
    for i, at in plan["seam"].items():
        assert list(w[2][i]["trainIdx"]) == at[:2] and list(w["list"][i]["trainIdx"]) == at and list(w["list"][i]["distance"]) == [4, 4, 4]
        assert at[1] % WIDE_SLICE == WIDE_SLICE - 1 and at[2] % WIDE_SLICE == 0
    for i, (low, high) in plan["second"].items():
        assert list(w[2][i]["trainIdx"]) == [low, high] and high >= 65536
    assert w[1][22][0]["trainIdx"] == WIDE_NB - 1
    allowed = M.sum(axis=1)
    assert (allowed[:CROWD_FROM] <= 3).all() and (allowed[CROWD_FROM:] > 1000).all() and (allowed[CROWD_FROM:] < 3500).all()
    n_list, n_dense = np.array([len(r) for r in w["list"]]), np.array([len(r) for r in w["dense"]])
    assert n_list.max() <= LIST and (n_list > 2).any()
    assert (n_dense > LIST).sum() >= 30 and n_dense[CROWD_FROM:].min() > WIDE_CAPS[0] and n_dense.max() < WIDE_CAPS[1] and (n_dense <= 3).any()
    stored = {"k1": (w[1], 1), "k2": (w[2], 2), "list": (w["list"], 8), "dense_cut": (w["dense"], WIDE_CAPS[0]), "dense_all": (w["dense"], WIDE_CAPS[1])}
    for mode, (rows, cap) in stored.items():                         # at least 10 reported train indices of 2^16 and more, in every mode
        assert sum(int((r[:cap]["trainIdx"] >= 65536).sum()) for r in rows) >= 10, mode
    return w


@pytest.fixture(scope="module", params=[CENTRE, LINE], ids=lambda f: FORMS[f])
def wide(lib, request):
    case = wide_case(request.param)
    case["want"] = wide_wants(case)
    case["Q"], case["T"] = Frame(case["q"], case["kq"]), Frame(case["t"], case["kt"])
    case["d_model"] = upload_models(case["model"].reshape(1))
    return case


@pytest.mark.parametrize("mode", ["k1", "k2", "list", "dense_cut", "dense_all"])
def test_train_indices_beyond_16_bits_behind_a_guide(wide, mode):
    form, w = wide["form"], wide["want"]
    kind, per, want, radius, rows_cap = {"k1": ("knn", 1, w[1], None, WIDE_NA + 5), "k2": ("knn", 2, w[2], None, WIDE_NA + 5),
                                         "list": ("radius", 8, w["list"], WIDE_LIST_RADIUS, WIDE_NA + 5),
                                         "dense_cut": ("radius", WIDE_CAPS[0], w["dense"], WIDE_DENSE_RADIUS, WIDE_NA),
                                         "dense_all": ("radius", WIDE_CAPS[1], w["dense"], WIDE_DENSE_RADIUS, WIDE_NA)}[mode]
    Q, T = wide["Q"], wide["T"]
    out = device_call(B.default_context(0), form, kind, Q.set, Q.kp, T.set, T.kp, B.PairSpec(1, 0, 0, 0, 0, None), 1, wide["d_model"],
                      guide_of(form, WIDE_WINDOW[form], WIDE_BAND, 0), per, rows_cap, 16, radius=radius)
    same_padded(host(out), 0, want, WIDE_NA)


# ---- 2 (b): the mutual forms over a long query frame ---------------------------------------------------------------------------------

LONG_NA, LONG_NB, LONG_CAP = 70000, 64, 64
LONG_SLICE = 8750                    # a wave's query rows: 136 staging blocks of 64 and a last block of 46 rows, whose last chunk is clamped
LONG_LAST_BLOCK = 136 * 64
# the y scale makes the image of y = 2e38 overflow fp32: a keypoint there has no centre, whatever the window's bounds on dy
LONG_MODEL = {CENTRE: ((1.0, 0.0, 8.0, 0.0, 2.0, -8.0, 0.0, 0.0, 1.0), 3, 0), LINE: (cross(2000.0, 304.0), 3, 0)}
LONG_WINDOW = {CENTRE: (-8.0, 8.0, -INF, INF, -1), LINE: (-8.0, 8.0, -8.0, 8.0, -1)}
LONG_BAND = 2.0
EPIPOLE = (2000.0, 304.0)
POSITIONS = [(name, w, LONG_SLICE * w + off) for w in (1, 7)
             for name, off in (("first", 0), ("64th", 63), ("65th", 64), ("last block", LONG_LAST_BLOCK), ("last", LONG_SLICE - 1))] + \
            [("beyond 2^16", 7, 66003)]
ABSENT_AT = [LONG_SLICE * 2 + 1, LONG_SLICE * 5 + LONG_SLICE - 2, 67001]       # rivals without a centre / a line
OTHER_AT = [LONG_SLICE * 3 + 65, LONG_SLICE * 4 + LONG_SLICE - 1, 68000]       # rivals outside the band (line), with a NaN coordinate (centre)
LONG_CROWD = 39                      # query and train rows 39 ... 63: low-entropy rows at one spot, all allowed to each other


def long_image(form, xy):
    return (xy[0] + 8.0, 2.0 * xy[1] - 8.0) if form == CENTRE else xy


def long_case(form):
    """n_a = 70 000 against n_b = 64, rows_cap 64.  Rival query row r of each entry of POSITIONS serves three forward rows:
      3g      train row 3g is one bit from r and two from row 3g, and the guide allows (r, 3g): the row is dropped
      3g + 1  the same descriptors, but train row 3g + 1 lies 200 pixels outside r's window: the row is kept (the ungated cross check
              would drop it)
      3g + 2  r ties row 3g + 2 at distance 2 and has the higher index: the row is kept
    rows 33 ... 35: a nearer rival without a centre (its image overflows fp32) / without a line (it is the epipole), inside the window
    otherwise; rows 36 ... 38: a nearer rival with a NaN coordinate (centre), 6 pixels off the line (line): all kept"""
    rng = np.random.default_rng(2310 + form)
    a = rng.integers(0, 256, (LONG_NA, 16), dtype=np.uint8)
    b = rng.integers(0, 256, (LONG_NB, 16), dtype=np.uint8)
    ka, kb = keypoints(LONG_NA), keypoints(LONG_NB)
    img = lambda xy: long_image(form, xy)                            # noqa: E731
    plan = []
    for g, (name, w, r) in enumerate(POSITIONS):
        A, Bsp = (400.0 * g + 40.0, 100.0 + 10.0 * (g % 3)), (400.0 * g + 240.0, 100.0 + 10.0 * (g % 3))
        D = rng.integers(0, 256, 16, dtype=np.uint8)
        a[r] = D
        put(ka, r, A)
        for v, (bits_t, bits_q, at) in enumerate((([10], [10, 20, 21], A), ([11], [11, 22, 23], Bsp), ([12, 13], [12, 13, 24, 25], A))):
            q = 3 * g + v
            b[q], a[q] = flipped(D, bits_t), flipped(D, bits_q)
            put(ka, q, at)
            put(kb, q, img(at))
        plan.append((name, w, r, 3 * g))
    extra = []
    for j in range(3):
        for q, r, kind in ((33 + j, ABSENT_AT[j], "absent"), (36 + j, OTHER_AT[j], "other")):
            D = rng.integers(0, 256, 16, dtype=np.uint8)
            b[q], a[q], a[r] = flipped(D, [30]), flipped(D, [30, 40, 41]), D
            if form == CENTRE:
                at = (6000.0 + 400.0 * (q - 33), 100.0)
                put(ka, r, (at[0], 2.0e38) if kind == "absent" else (np.nan, at[1]))
            elif kind == "absent":
                at = (EPIPOLE[0] + 3.0, EPIPOLE[1])
                put(ka, r, EPIPOLE)
            else:
                at = (8000.0 + 400.0 * j, 100.0)
                put(ka, r, (at[0], at[1] + 6.0))
            put(ka, q, at)
            put(kb, q, img(at))
            extra.append((kind, q, r))
    n = LONG_NB - LONG_CROWD
    a[LONG_CROWD:LONG_NB] = rng.integers(0, 4, (n, 16), dtype=np.uint8) * 85
    b[LONG_CROWD:] = rng.integers(0, 4, (n, 16), dtype=np.uint8) * 85
    Z = (14000.0, 500.0)
    for q in range(LONG_CROWD, LONG_NB):
        put(ka, q, Z)
        put(kb, q, img(Z))
    return {"form": form, "a": a, "b": b, "ka": ka, "kb": kb, "model": records(form, [LONG_MODEL[form]])[0], "plan": plan, "extra": extra}


def long_want(case):
    """mutual_under_mask on the full 70 000 x 64 mask, and on the restatement alone: every variant occurs at every position class"""
    form, a, b = case["form"], case["a"], case["b"]
    M, has = mask_of(form, LONG_WINDOW[form], LONG_BAND, 0, case["model"], case["ka"], case["kb"])
    assert M.shape == (LONG_NA, LONG_NB)
    want = mutual_want(M, has, a, b, 0, LONG_CAP)
    _, _, ft, fd, kept = want
    assert LONG_SLICE * 8 == LONG_NA and LONG_SLICE - LONG_LAST_BLOCK == 46 and 46 % 4 == 2
    seen = {}
    for name, w, r, q in case["plan"]:
        assert r // LONG_SLICE == w and r >= LONG_CAP
        off = r - LONG_SLICE * w
        assert {"first": off == 0, "64th": off == 63, "65th": off == 64, "last block": off == LONG_LAST_BLOCK, "last": off == LONG_SLICE - 1,
                "beyond 2^16": r >= 65536 and 64 < off < LONG_LAST_BLOCK}[name]
        assert [int(ft[q + v]) for v in range(3)] == [q, q + 1, q + 2] and [int(fd[q + v]) for v in range(3)] == [2, 2, 2]
        dropped = M[r, q] and hamming(a[r], b[q]) < 2 and not kept[q]
        forbidden = not M[r, q + 1] and hamming(a[r], b[q + 1]) < 2 and kept[q + 1]      # nearer, as the ungated cross check sees it
        tied = M[r, q + 2] and hamming(a[r], b[q + 2]) == 2 and r > q + 2 and kept[q + 2]
        seen.setdefault(name, []).append((bool(dropped), bool(forbidden), bool(tied)))
    assert len(seen) == 6 and all(all(all(v) for v in vs) for vs in seen.values()), seen
    for kind, q, r in case["extra"]:
        assert ft[q] == q and fd[q] == 2 and kept[q] and hamming(a[r], b[q]) == 1 and not M[r, q], (kind, q)
        assert not has[r] if kind == "absent" or form == CENTRE else has[r]
    crowd = kept[LONG_CROWD:]
    assert (ft[LONG_CROWD:] >= LONG_CROWD).all() and 0 < crowd.sum() < len(crowd)
    return want


@pytest.mark.parametrize("form", [CENTRE, LINE], ids=lambda f: FORMS[f])
def test_the_backward_scan_over_a_long_query_frame(lib, form):
    case = long_case(form)
    want = long_want(case)
    Q, T = Frame(case["a"], case["ka"]), Frame(case["b"], case["kb"])
    out = device_call(B.default_context(0), form, "mutual", Q.set, Q.kp, T.set, T.kp, B.PairSpec(1, 0, 0, 0, 0, None), 1,
                      upload_models(case["model"].reshape(1)), guide_of(form, LONG_WINDOW[form], LONG_BAND, 0), 1, LONG_CAP, 16)
    assert same_mutual(B, out, [want], LONG_CAP) > 20


# ---- 2 (c): the most rows the keys hold ------------------------------------------------------------------------------------------------

LIMIT_NA = 8
LIMIT_SPOT = (500.0, 300.0)
LIMIT_PLANTED = 48                   # the last 48 train rows lie nearer than any random row; every sixth of them is forbidden


def limit_case(form):
    """8 query rows at one spot against 2^22 - 1 train rows from one generator call.  The best and second-best allowed rows of every
    query are the last two (indices 2^22 - 2 and 2^22 - 3); of the 46 near rows in front of them every sixth lies far away, and every
    997th train row lies in the window too.  The model, window and band of the wide cases"""
    rng = np.random.default_rng(2320 + form)
    t = rng.integers(0, 256, (LIMIT, 16), dtype=np.uint8)
    q0 = rng.integers(0, 256, 16, dtype=np.uint8)
    q = np.stack([q0] + [flipped(q0, [127 - i]) for i in range(1, LIMIT_NA)])
    kq, kt = keypoints(LIMIT_NA, *LIMIT_SPOT), keypoints(LIMIT)
    c = image(form, LIMIT_SPOT)
    some = np.arange(500, LIMIT, 997)
    kt["x"][some], kt["y"][some] = c[0] + rng.integers(-64, 65, len(some)) / 4.0, c[1] + rng.integers(-32, 33, len(some)) / 4.0
    t[LIMIT - 1], t[LIMIT - 2] = q0, flipped(q0, [0, 1])
    hidden = []
    for j in range(LIMIT_PLANTED - 2):
        at = LIMIT - 3 - j
        t[at] = flipped(q0, [8] if j % 6 == 0 else [8 + i for i in range(4 + j % 5)])    # (one bit: nearer than row 2^22 - 3)
        hidden += [at] if j % 6 == 0 else []
    near = np.arange(LIMIT - LIMIT_PLANTED, LIMIT)
    kt["x"][near], kt["y"][near] = c[0] + 16.0 * ((near % 3) - 1), c[1] + 8.0 * ((near % 5) // 2 - 1)    # on the window's bounds and inside
    kt["x"][hidden] = FAR
    return {"form": form, "q": q, "t": t, "kq": kq, "kt": kt, "model": records(form, [WIDE_MODEL[form]])[0], "hidden": hidden}


def limit_want(case):
    form, q, t = case["form"], case["q"], case["t"]
    M, has = mask_of(form, WIDE_WINDOW[form], WIDE_BAND, 0, case["model"], case["kq"], case["kt"])
    assert M.shape == (LIMIT_NA, LIMIT) and has.all() and not M[:, case["hidden"]].any() and len(case["hidden"]) == 8
    assert M[:, LIMIT - LIMIT_PLANTED:].sum() == LIMIT_NA * (LIMIT_PLANTED - 8) and 100 < M[0].sum() < 5000
    want = {2: oracle_knn(q, t, M, 0, 2), "list": oracle_radius(q, t, M, 0, 3.5), "dense": oracle_radius(q, t, M, 0, 10.0)}
    for r in want[2]:
        assert list(r["trainIdx"]) == [LIMIT - 1, LIMIT - 2] == [(1 << IDX_BITS) - 2, (1 << IDX_BITS) - 3]
    assert [list(r["trainIdx"]) for r in want["list"]] == [[LIMIT - 1, LIMIT - 2]] * LIMIT_NA
    assert [len(r) for r in want["dense"]] == [LIMIT_PLANTED - 8] * LIMIT_NA and LIMIT_PLANTED - 8 > LIST
    plain = O.match_knn(q, [t], 2, masks=[np.ascontiguousarray(M | (np.arange(LIMIT) == case["hidden"][0])[None, :].astype(np.uint8))])
    assert all(r[1]["trainIdx"] == case["hidden"][0] for r in plain)               # a forbidden row would have come second
    return want


@pytest.fixture(scope="module", params=[CENTRE, LINE], ids=lambda f: FORMS[f])
def limit(lib, request):
    case = limit_case(request.param)
    case["want"] = limit_want(case)
    case["Q"], case["T"] = Frame(case["q"], case["kq"]), Frame(case["t"], case["kt"])
    case["d_model"] = upload_models(case["model"].reshape(1))
    return case


@pytest.mark.parametrize("kind", ["knn", "radius"])
def test_the_most_train_rows_the_keys_hold_behind_a_guide(limit, kind):
    form, w, Q, T = limit["form"], limit["want"], limit["Q"], limit["T"]
    calls = [("knn", 2, w[2], None)] if kind == "knn" else [("radius", 1, w["list"], 3.5), ("radius", 48, w["dense"], 10.0)]
    for kind_, per, want, radius in calls:
        out = device_call(B.default_context(0), form, kind_, Q.set, Q.kp, T.set, T.kp, B.PairSpec(1, 0, 0, 0, 0, None), 1, limit["d_model"],
                          guide_of(form, WIDE_WINDOW[form], WIDE_BAND, 0), per, LIMIT_NA + 1, 16, radius=radius)
        same_padded(host(out), 0, want, LIMIT_NA)


LIMIT_NB, LIMIT_ROWS_CAP = 3, 4


def limit_mutual_case(form):
    """2^22 - 1 query rows against 3 train rows, rows_cap 4: row 0 loses its train row to an allowed rival in the very last query row;
    row 1 keeps its own although row 2^22 - 3 is nearer - 100 pixels outside the window; row 2 is tied by row 2^22 - 4 and kept; row 3
    lies far away and has no forward match.  The model, window and band of the long cases"""
    rng = np.random.default_rng(2330 + form)
    a = rng.integers(0, 256, (LIMIT, 16), dtype=np.uint8)
    D = rng.integers(0, 256, (3, 16), dtype=np.uint8)
    b = np.stack([flipped(D[0], [10]), flipped(D[1], [11]), flipped(D[2], [12, 13])])
    a[0], a[1], a[2] = flipped(D[0], [10, 20, 21]), flipped(D[1], [11, 22, 23]), flipped(D[2], [12, 13, 24, 25])
    rivals = [LIMIT - 1, LIMIT - 2, LIMIT - 3]
    ka, kb = keypoints(LIMIT), keypoints(LIMIT_NB)
    for i, r in enumerate(rivals):
        at = (400.0 * i + 40.0, 100.0)
        a[r] = D[i]
        put(ka, i, at)
        put(kb, i, long_image(form, at))
        put(ka, r, (at[0] + 100.0, at[1]) if i == 1 else at)
    return {"form": form, "a": a, "b": b, "ka": ka, "kb": kb, "model": records(form, [LONG_MODEL[form]])[0], "rivals": rivals}


def limit_mutual_want(case):
    form, a, b, r = case["form"], case["a"], case["b"], case["rivals"]
    M, has = mask_of(form, LONG_WINDOW[form], LONG_BAND, 0, case["model"], case["ka"], case["kb"])
    assert M.shape == (LIMIT, LIMIT_NB) and r[0] == (1 << IDX_BITS) - 2
    want = mutual_want(M, has, a, b, 0, LIMIT_ROWS_CAP)
    _, _, ft, fd, kept = want
    assert list(ft) == [0, 1, 2, -1] and list(fd[:3]) == [2, 2, 2] and list(kept) == [False, True, True, False]
    assert M[r[0], 0] and hamming(a[r[0]], b[0]) == 1
    assert not M[r[1], 1] and hamming(a[r[1]], b[1]) == 1
    assert M[r[2], 2] and hamming(a[r[2]], b[2]) == 2
    assert M.sum() == 5
    return want


@pytest.mark.parametrize("form", [CENTRE, LINE], ids=lambda f: FORMS[f])
def test_the_most_query_rows_the_backward_keys_hold(lib, form):
    case = limit_mutual_case(form)
    want = limit_mutual_want(case)
    Q, T = Frame(case["a"], case["ka"]), Frame(case["b"], case["kb"])
    out = device_call(B.default_context(0), form, "mutual", Q.set, Q.kp, T.set, T.kp, B.PairSpec(1, 0, 0, 0, 0, None), 1,
                      upload_models(case["model"].reshape(1)), guide_of(form, LONG_WINDOW[form], LONG_BAND, 0), 1, LIMIT_ROWS_CAP, 16)
    assert same_mutual(B, out, [want], LIMIT_ROWS_CAP) == 2


CLAIM_ROWS = 64
CLAIM_PAIRS = [(0, 2), (0, 1), (1, 0), (2, 0)]       # frame 1 claims 2^22 rows: as the train frame of pair 1, as the query frame of pair 2


def claim_case():
    """three frames of 64 rows, 64 rows apart in ONE buffer of 2^22 + 192 rows: frame 1 may claim 2^22 rows, and every one of them is
    allocated memory.  The 192 rows the expectations read, with keypoints on the wide cases' grid"""
    rng = np.random.default_rng(2340)
    rows = (rng.integers(0, 4, (3 * CLAIM_ROWS, 16), dtype=np.uint8) * 85).astype(np.uint8)
    kps = keypoints(3 * CLAIM_ROWS, 8.0 * rng.integers(0, 6, 3 * CLAIM_ROWS), 8.0 * rng.integers(0, 4, 3 * CLAIM_ROWS), rng.integers(0, 3, 3 * CLAIM_ROWS))
    return rows, kps


def claim_want(form, kind, per, rows, kps, radius):
    """per pair: what the call must hold when frame 1 claims 2^22 rows (None: the pair is refused), and pair_rows"""
    frame = lambda f: slice(CLAIM_ROWS * f, CLAIM_ROWS * (f + 1))    # noqa: E731
    model = records(form, [WIDE_MODEL[form]])[0]
    out, pair_rows = [], []
    for a, b in CLAIM_PAIRS:
        if b == 1 or (a == 1 and kind == "mutual"):
            out.append(None)
            pair_rows.append(-1)
            continue
        M, has = mask_of(form, WIDE_WINDOW[form], WIDE_BAND, 0, model, kps[frame(a)], kps[frame(b)])
        dq, dt = rows[frame(a)], rows[frame(b)]
        assert 0 < M.sum() < M.size
        if kind == "mutual":
            w = mutual_want(M, has, dq, dt, b, CLAIM_ROWS)
            out.append(((1 << IDX_BITS) if a == 1 else CLAIM_ROWS,) + w[1:])
        else:
            out.append(oracle_knn(dq, dt, M, b, per) if kind == "knn" else oracle_radius(dq, dt, M, b, radius))
        pair_rows.append((1 << IDX_BITS) if a == 1 else CLAIM_ROWS)  # (as a query frame of a forward call: its first rows_cap rows are matched)
    return out, pair_rows


@pytest.mark.parametrize("form", [CENTRE, LINE], ids=lambda f: FORMS[f])
def test_a_count_the_keys_do_not_hold(lib, form):
    """a count of exactly 2^22, backed by 2^22 allocated rows and keypoint records: as a train frame (and as a query frame of a mutual
    call) the pair gets pair_rows -1 and nothing is written; the pairs before and after it are what they are without it"""
    import torch
    rows, kps = claim_case()
    total = (1 << IDX_BITS) + 3 * CLAIM_ROWS
    rec = B.KEYPOINT.itemsize
    d_desc = torch.randint(0, 256, (total * 16,), dtype=torch.uint8, device="cuda")
    d_kps = torch.zeros(total * rec, dtype=torch.uint8, device="cuda")
    d_desc[:rows.size] = torch.from_numpy(rows.reshape(-1)).cuda()
    d_kps[:kps.nbytes] = torch.from_numpy(kps.view(np.uint8).copy()).cuda()
    settled(d_desc, d_kps)
    d_cnt = torch.tensor([CLAIM_ROWS, 1 << IDX_BITS, CLAIM_ROWS], dtype=torch.int32).cuda()
    S = B.DescSet(d_desc.data_ptr(), d_cnt.data_ptr(), 1, CLAIM_ROWS * 16, 16, 3)
    K = B.KpSet(d_kps.data_ptr(), CLAIM_ROWS * rec)
    assert CLAIM_ROWS * 16 + (1 << IDX_BITS) * 16 <= d_desc.numel() and CLAIM_ROWS * rec + (1 << IDX_BITS) * rec <= d_kps.numel()
    spec, keep = list_spec(CLAIM_PAIRS)
    d_models = upload_models(records(form, [WIDE_MODEL[form]] * len(CLAIM_PAIRS)))
    guide = guide_of(form, WIDE_WINDOW[form], WIDE_BAND, 0)
    for kind, per, radius in (("knn", 2, None), ("radius", 3, 40.5), ("mutual", 1, None)):
        want, pair_rows = claim_want(form, kind, per, rows, kps, radius)
        out = device_call(B.default_context(0), form, kind, S, K, S, K, spec, len(CLAIM_PAIRS), d_models, guide, per, CLAIM_ROWS, 16, radius=radius)
        if kind == "mutual":
            assert pair_rows == [CLAIM_ROWS, -1, -1, CLAIM_ROWS] and same_mutual(B, out, want, CLAIM_ROWS) > 10
            continue
        got = host(out)
        assert list(got[2]) == pair_rows == [CLAIM_ROWS, -1, 1 << IDX_BITS, CLAIM_ROWS]
        for p, w in enumerate(want):
            if w is None:
                assert (got[1][p] == SENTINEL).all() and (got[0][p] == SENTINEL).all()
            else:
                same_padded(got, p, w, pair_rows[p])


# ---- 3: closed bounds at fractional centres -------------------------------------------------------------------------------------------

BOUND_H = (1.01, 0.02, 3.0, -0.015, 0.99, -2.0, 1e-5, -2e-5, 1.0)
BOUND_WINDOW = (-6.0, 6.0, -5.5, 5.5, -1)
BOUND_NQ, BOUND_RADIUS = 2000, 40.5


def bound_case():
    """one pair of frames under BOUND_H and under its negation (the guide has no sign test): 2 000 query keypoints with arbitrary
    fractions in a 1920 x 1080 frame, 48-byte rows.  Query row q has two train rows that carry its descriptor: 2q + 1 lies ON one of
    the window's four bounds around the restated centre (in turn from row to row) - T.x = fl32(C.x + 6) where fl32(T.x - C.x) == 6
    holds, and so on -, 2q one fp32 ulp beyond it.  The forbidden row comes first: allowed by mistake, it wins every tie.  Where no
    fp32 number lies exactly on the bound both rows lie at the centre and the row is not counted."""
    rng = np.random.default_rng(2350)
    x, y = rng.uniform(0, 1920, BOUND_NQ).astype(np.float32), rng.uniform(0, 1080, BOUND_NQ).astype(np.float32)
    cx, cy, has = restated_centres(BOUND_H, 0, 0, 0, x, y)
    assert has.all() and cx.dtype == np.float32
    bound = np.arange(BOUND_NQ) % 4
    lim = np.array([BOUND_WINDOW[1], BOUND_WINDOW[0], BOUND_WINDOW[3], BOUND_WINDOW[2]], np.float32)[bound]
    c = np.where(bound < 2, cx, cy)
    on = (c + lim).astype(np.float32)                                # one fp32 addition: fl32(C + bound)
    beyond = np.nextafter(on, np.where(lim > 0, np.float32(INF), np.float32(-INF)).astype(np.float32)).astype(np.float32)
    # (a neighbour finer than the centre's ulp - a small coordinate under a larger centre - may round back onto the bound)
    planted = ((on - c).astype(np.float32) == lim) & ((beyond - c).astype(np.float32) != lim)
    on, beyond = np.where(planted, on, c), np.where(planted, beyond, c)
    kq, kt = keypoints(BOUND_NQ, x, y), keypoints(2 * BOUND_NQ)
    kt["x"][0::2], kt["x"][1::2] = np.where(bound < 2, beyond, cx), np.where(bound < 2, on, cx)
    kt["y"][0::2], kt["y"][1::2] = np.where(bound < 2, cy, beyond), np.where(bound < 2, cy, on)
    dq = rng.integers(0, 256, (BOUND_NQ, 48), dtype=np.uint8)
    dt = np.repeat(dq, 2, axis=0)
    models = centre_records(B, [(BOUND_H, 0, 0), (tuple(-e for e in BOUND_H), 1, 0)])
    return {"dq": dq, "dt": dt, "kq": kq, "kt": kt, "models": models, "planted": planted, "bound": bound, "centres": (cx, cy)}


def bound_want(case):
    """per model: the mask and the expectations of the three calls; the share of rows that keep their plant"""
    dq, dt, planted = case["dq"], case["dt"], case["planted"]
    out = []
    for rec in case["models"]:
        cx, cy, _ = restated_centres(rec["h"], rec["hypothesis"], rec["flags"], 0, case["kq"]["x"], case["kq"]["y"])
        assert cx.tobytes() == case["centres"][0].tobytes() and cy.tobytes() == case["centres"][1].tobytes()   # -H: the same centres
        M, has = mask_of(CENTRE, BOUND_WINDOW, 0.0, 0, rec, case["kq"], case["kt"])
        q = np.arange(BOUND_NQ)
        assert M[q, 2 * q + 1].all() and not M[q[planted], 2 * q[planted]].any() and M[q[~planted], 2 * q[~planted]].all()
        k1, rad = oracle_knn(dq, dt, M, 0, 1), oracle_radius(dq, dt, M, 0, BOUND_RADIUS)
        assert all(r[0]["trainIdx"] == 2 * i + 1 - (not planted[i]) and r[0]["distance"] == 0 for i, r in enumerate(k1))
        assert all(len(r) == 2 - planted[i] for i, r in enumerate(rad))
        out.append({"k1": k1, "radius": rad, "mutual": mutual_want(M, has, dq, dt, 0, BOUND_NQ)})
        assert out[-1]["mutual"][4].all()
    share = planted.mean()
    assert share >= 0.9 and all((planted & (case["bound"] == k)).sum() > 400 for k in range(4)), share
    return out


@pytest.fixture(scope="module")
def bounds(lib):
    case = bound_case()
    case["want"] = bound_want(case)
    case["Q"], case["T"] = Frame(case["dq"], case["kq"]), Frame(case["dt"], case["kt"])
    case["d_models"] = upload_models(case["models"])
    return case


@pytest.mark.parametrize("kind", ["knn", "radius", "mutual"])
def test_closed_bounds_at_fractional_centres(bounds, kind):
    """A train keypoint exactly on a bound of a centre with an arbitrary fraction is allowed, its fp32 neighbour beyond the bound is
    not: a centre that is one fp32 ulp off - an fp32 division, a reciprocal approximation, a contracted multiply-add in fp32 - swaps
    at least one of the two in almost every row.  What this does NOT claim: a one-ulp error of the fp64 quotient moves none of these
    fp32 centres (counted on 100 000 draws of this model: none), so the test detects fp32-level arithmetic in the centre, not
    last-bit differences of the fp64 division."""
    Q, T, want = bounds["Q"], bounds["T"], bounds["want"]
    per, radius = {"knn": (1, None), "radius": (4, BOUND_RADIUS), "mutual": (1, None)}[kind]
    spec, keep = list_spec([(0, 0), (0, 0)])
    out = device_call(B.default_context(0), CENTRE, kind, Q.set, Q.kp, T.set, T.kp, spec, 2, bounds["d_models"],
                      guide_of(CENTRE, BOUND_WINDOW, 0.0, 0), per, BOUND_NQ, 48, radius=radius)
    if kind == "mutual":
        assert same_mutual(B, out, [w["mutual"] for w in want], BOUND_NQ) == 2 * BOUND_NQ
        return
    got = host(out)
    for p, w in enumerate(want):
        same_padded(got, p, w["k1" if kind == "knn" else "radius"], BOUND_NQ)


BAND_NQ, BAND, BAND_SCALES = 48, 3.0, (1.0, 0.25, -4.0)
BAND_WINDOW = (-16.0, 16.0, -INF, INF, -1)
BAND_RADIUS = 20.5


def band_case():
    """the line form, exact cases only: RECTIFIED at three power-of-two scales (three pairs on the same frames), 32-byte rows, y around
    1 900 where an fp32 ulp is 2^-13.  Query row q has four train rows that carry its descriptor: 4q one ulp beyond y + band, 4q + 1 at
    y + band, 4q + 2 one ulp beyond y - band, 4q + 3 at y - band; their x lie on and inside the window's bounds.  Every product and
    sum of the band's rule is exact in fp64 here"""
    rng = np.random.default_rng(2360)
    i = np.arange(BAND_NQ)
    x, y = (40.0 * i + 0.5).astype(np.float32), (1900.25 + 0.5 * i).astype(np.float32)
    up, down = (y + np.float32(BAND)).astype(np.float32), (y - np.float32(BAND)).astype(np.float32)
    assert ((up - y) == BAND).all() and ((y - down) == BAND).all()
    kq, kt = keypoints(BAND_NQ, x, y), keypoints(4 * BAND_NQ)
    for j, (ty, dx) in enumerate(((np.nextafter(up, np.float32(INF)), -16.0), (up, 16.0), (np.nextafter(down, np.float32(-INF)), 0.0), (down, 8.0))):
        kt["x"][j::4], kt["y"][j::4] = x + np.float32(dx), ty
    dq = rng.integers(0, 256, (BAND_NQ, 32), dtype=np.uint8)
    return {"dq": dq, "dt": np.repeat(dq, 4, axis=0), "kq": kq, "kt": kt, "models": line_records(B, [(scaled(RECTIFIED, s), 0, 0) for s in BAND_SCALES])}


def band_want(case):
    dq, dt = case["dq"], case["dt"]
    out = []
    q = np.arange(BAND_NQ)
    for rec in case["models"]:
        M, has = mask_of(LINE, BAND_WINDOW, BAND, 0, rec, case["kq"], case["kt"])
        assert has.all() and M.sum() == 2 * BAND_NQ and M[q, 4 * q + 1].all() and M[q, 4 * q + 3].all()
        k2, rad = oracle_knn(dq, dt, M, 0, 2), oracle_radius(dq, dt, M, 0, BAND_RADIUS)
        assert all(list(r["trainIdx"]) == [4 * i + 1, 4 * i + 3] for i, r in enumerate(k2))
        out.append({"k2": k2, "radius": rad, "mutual": mutual_want(M, has, dq, dt, 0, BAND_NQ)})
        assert out[-1]["mutual"][4].all() and (out[-1]["mutual"][2] == 4 * q + 1).all()
    return out


@pytest.mark.parametrize("kind", ["knn", "radius", "mutual"])
def test_closed_bounds_of_the_band(lib, kind):
    case = band_case()
    want = band_want(case)
    Q, T = Frame(case["dq"], case["kq"]), Frame(case["dt"], case["kt"])
    per, radius = {"knn": (2, None), "radius": (4, BAND_RADIUS), "mutual": (1, None)}[kind]
    n = len(BAND_SCALES)
    spec, keep = list_spec([(0, 0)] * n)
    out = device_call(B.default_context(0), LINE, kind, Q.set, Q.kp, T.set, T.kp, spec, n, upload_models(case["models"]),
                      guide_of(LINE, BAND_WINDOW, BAND, 0), per, BAND_NQ + 3, 32, radius=radius)
    if kind == "mutual":
        assert same_mutual(B, out, [w["mutual"] for w in want], BAND_NQ + 3) == n * BAND_NQ
        return
    got = host(out)
    for p, w in enumerate(want):
        same_padded(got, p, w["k2" if kind == "knn" else "radius"], BAND_NQ)
