"""GPU tests of brisk_hip_match_knn_pairs_guided_device / brisk_hip_match_radius_pairs_guided_device: the gated pair matchers with the
window centred where each pair's model puts the query keypoint.  The guide defines a mask per pair (tests/test_abi_match_guided.py
restates it in NumPy); everything is compared with the CPU oracle matching with that mask, as the gated matchers' tests do - integer
fields equal, distances equal as bit patterns, counts equal: no tolerance."""
import ctypes as C

import numpy as np
import pytest

from test_abi_match_guided import IDENTITY, PAIR_BAD, PAIR_NO_MODEL, restated_centres
from test_abi_tracks import SENT32, restated_link
from test_abi_verify import restated_verify
from test_gpu_match_export import expect as restated_select, host_triple
from test_gpu_match_gated import SynthKp, gate_mask, knn_rows, oracle_knn, oracle_radius, same_cut, sentinel_outputs, spec_of
from test_gpu_match_pairs import CAP, COUNTS_A, COUNTS_B, SENTINEL, SynthSet, batch_frames, oracle_pair, same_rows
from test_gpu_stream_order import begin, env, race, run_batch, sptr  # noqa: F401 (env: the fixture of the held stream)
from test_gpu_verify import chain_frames
from test_oracle_golden import H_1TO2

pytestmark = pytest.mark.gpu

COUNTS_T = [0, 1, 3, 4, 5, 8, 9, 33]        # train rows around the waves' chunks of four and their eight slices
GRID_WINDOW = (-16.0, 16.0, -8.0, 8.0, 1)   # on SynthKp's grid of 8 pixels: differences hit the bounds exactly
NARROW = (-8.0, 8.0, -8.0, 8.0, 0)          # nine grid positions and one octave: dense frames keep rows with 0, 1 and many allowed
LIST = 32                                   # MRP_LIST: radius rows with more hits take the kernel's dense path
NAN = float("nan")
# (h, hypothesis, flags): one of each kind.  SynthKp's keypoints lie on x = 0, 8 ... 56, y = 0, 8 ... 40
MODELS = [((1.0, 0.0, 8.0, 0.0, 1.0, -8.0, 0.0, 0.0, 1.0), 0, 0),                  # a translation
          ((0.0, -1.5, 60.0, 1.5, 0.0, -12.0, 0.0, 0.0, 1.5), 7, 0x100),           # a similarity (a quarter turn), every element scaled
          ((10.0, 0.0, 0.0, 0.0, 10.0, 0.0, 1.0, 0.0, -24.0), 4095, 0x1),          # z = x - 24: both signs on the grid, 0 at x = 24
          ((1.0, 0.0, 0.0, 0.0, 1.0, NAN, 0.0, 0.0, 1.0), 1, 0),                    # a NaN: no row has a centre
          ((0.0,) * 9, 2, 0),                                                       # the zero model: 0 / 0
          ((1.0, 0.0, 8.0, 0.0, 1.0, -8.0, 0.0, 0.0, 1.0), -1, 0),                  # no valid hypothesis
          ((1.0, 0.0, 8.0, 0.0, 1.0, -8.0, 0.0, 0.0, 1.0), 3, PAIR_NO_MODEL),
          ((NAN,) * 9, 0, PAIR_BAD)]


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


def model_records(B, models):
    rec = np.zeros(len(models), B.PAIR_MODEL)
    for i, (h, hyp, flags) in enumerate(models):
        rec[i]["h"], rec[i]["hypothesis"], rec[i]["flags"] = h, hyp, flags
        rec[i]["records"], rec[i]["usable"], rec[i]["inliers"], rec[i]["valid"] = -1, -2, -3, -4     # (not read)
    return rec


def upload_models(rec):
    import torch
    return torch.from_numpy(rec.view(np.int64).reshape(len(rec), 12).copy()).cuda()


def guide_mask(window, fallback, model, kq, kt):
    """M[q][t] for one pair: the gate's mask with the query positions replaced by the restated centres, no row without a centre.
    model: a PAIR_MODEL record.  Also returns has-centre per query row."""
    cx, cy, has = restated_centres(model["h"], model["hypothesis"], model["flags"], fallback, kq["x"], kq["y"])
    kc = kq.copy()
    kc["x"], kc["y"] = cx, cy
    M = gate_mask(window, kc, kt)
    M[~has] = 0
    return M, has


def guide_of(B, window, fallback):
    return B.MatchGuide(B.MatchGate(*window), fallback)


class Tally:
    """what a call's restated masks hold: allowed train rows per query row, guided and unguided pairs, rows without a centre inside a
    guided pair"""

    def __init__(self):
        self.allowed, self.guided, self.unguided, self.no_centre = [], 0, 0, 0

    def add(self, M, has, model, rows):
        g = model["hypothesis"] >= 0 and (model["flags"] & (PAIR_BAD | PAIR_NO_MODEL)) == 0
        self.guided, self.unguided = self.guided + bool(g), self.unguided + (not g)
        self.no_centre += int((~has[:rows]).sum()) if g else 0
        self.allowed += [int(a) for a in M[:rows].sum(axis=1)] if M.size else [0] * rows

    def check(self):
        a = np.array(self.allowed)
        assert (a == 0).sum() >= 1 and (a == 1).sum() >= 1 and (a > 2).sum() >= 1, np.bincount(a)
        assert self.unguided >= 1 and self.guided >= 1 and self.no_centre >= 1


def run_guided(B, ctx, qs, qk, ts, tk, pairs, models, window, fallback, mode, rows_cap=CAP, cap=8, max_distance=None):
    """one guided call against the oracle under the restated masks; models: PAIR_MODEL records, one per pair.  Returns the Tally."""
    import torch
    spec, plist, keep = spec_of(B, pairs)
    assert len(models) == len(plist)
    d_models = upload_models(models)
    guide = guide_of(B, window, fallback)
    torch.cuda.synchronize()
    if mode == "radius":
        got, counts = ctx.match_radius_pairs_guided(qs.set, ts.set, spec, max_distance, cap, d_models, guide, rows_cap=rows_cap, query_kps=qk.set,
                                                    train_kps=tk.set, dim_bytes=qs.dim, download=True)
    else:
        k = {"k1": 1, "k2": 2}[mode]
        got = ctx.match_knn_pairs_guided(qs.set, ts.set, spec, k, d_models, guide, rows_cap=rows_cap, query_kps=qk.set, train_kps=tk.set,
                                         dim_bytes=qs.dim, download=True)
        counts = [None] * len(got)
    assert len(got) == len(plist)
    tally = Tally()
    for p, ((a, b), rows, c) in enumerate(zip(plist, got, counts)):
        if not (0 <= a < len(qs.desc) and 0 <= b < len(ts.desc)):
            assert rows == [] and (c is None or len(c) == 0)        # a bad entry of the list: d_pair_rows -1, no rows
            continue
        M, has = guide_mask(window, fallback, models[p], qk.kps[a], tk.kps[b])
        tally.add(M, has, models[p], min(len(qs.desc[a]), rows_cap))
        if mode == "radius":
            same_cut(rows, c, oracle_radius(qs.desc[a], ts.desc[b], M, b, max_distance)[:rows_cap], cap)
        else:
            same_rows(rows, oracle_knn(qs.desc[a], ts.desc[b], M, b, k)[:rows_cap])
    return tally


def sets(B, rng, dim, pitch, base_off, slack):
    """the query set A and the train sets Bs and T (COUNTS_T) with their keypoints"""
    A = SynthSet(B, rng, dim, pitch, COUNTS_A, CAP, base_off, 3, slack)
    Bs = SynthSet(B, rng, dim, pitch + 4 * (dim == 48), COUNTS_B, CAP, 0, 1, 0)
    T = SynthSet(B, rng, dim, pitch, COUNTS_T, CAP, 0, 2, 0)
    Ak = SynthKp(B, rng, COUNTS_A, CAP, slack=40, nan_every=17)
    Bk = SynthKp(B, rng, COUNTS_B, CAP, nan_every=23)
    Tk = SynthKp(B, rng, COUNTS_T, CAP)
    return A, Ak, Bs, Bk, T, Tk


DIMS = [(16, 20, 0, 0), (32, 48, 0, 4), (48, 64, 0, 0), (48, 51, 1, 3), (64, 64, 0, 0)]


# ---- 1: identity models = the gated matcher ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,pitch,base_off,slack", DIMS)
def test_identity_models_equal_the_gated_matcher(B, dim, pitch, base_off, slack):
    """all three output arrays, byte for byte, the sentinel-filled parts included"""
    import torch
    rng = np.random.default_rng(dim * 1000 + pitch + 2)
    ctx = B.default_context(0)
    A, Ak, Bs, Bk, T, Tk = sets(B, rng, dim, pitch, base_off, slack)
    nA = len(COUNTS_A)
    d_models = upload_models(model_records(B, [(IDENTITY, 0, 0)] * nA))
    spec = B.PairSpec(nA, 0, 1, 0, 1, None)
    gate, guide = B.MatchGate(*GRID_WINDOW), guide_of(B, GRID_WINDOW, 0)
    wrote = 0
    for ts, tk in ((Bs, Bk), (T, Tk)):
        for rows_cap in (CAP, 64):
            for mode, per in (("k1", 1), ("k2", 2), ("radius", 6), ("radius", 40)):
                want, got = sentinel_outputs(nA, rows_cap, per), sentinel_outputs(nA, rows_cap, per)
                torch.cuda.synchronize()
                if mode == "radius":
                    r = 4 * dim + 0.5 if per == 6 else 1e9
                    ctx.match_radius_pairs(A.set, ts.set, spec, r, per, rows_cap=rows_cap, dim_bytes=dim, out=want, gate=gate, query_kps=Ak.set,
                                           train_kps=tk.set)
                    ctx.match_radius_pairs_guided(A.set, ts.set, spec, r, per, d_models, guide, rows_cap=rows_cap, query_kps=Ak.set,
                                                  train_kps=tk.set, dim_bytes=dim, out=got)
                else:
                    ctx.match_knn_pairs(A.set, ts.set, spec, per, rows_cap=rows_cap, dim_bytes=dim, out=want, gate=gate, query_kps=Ak.set,
                                        train_kps=tk.set)
                    ctx.match_knn_pairs_guided(A.set, ts.set, spec, per, d_models, guide, rows_cap=rows_cap, query_kps=Ak.set, train_kps=tk.set,
                                               dim_bytes=dim, out=got)
                torch.cuda.synchronize()
                for name, g, w in zip(("matches", "counts", "pair_rows"), got, want):
                    g, w = g.cpu().numpy(), w.cpu().numpy()
                    assert g.tobytes() == w.tobytes(), (mode, per, rows_cap, name)
                    wrote += int((w != SENTINEL).sum()) if name == "matches" else 0
    assert wrote > 1000                                             # (the comparison is not one of sentinels alone)


# ---- 2: a model per pair, all pair forms ------------------------------------------------------------------------------------------

def cycled(B, n, first):
    """n model records, the eight kinds in turn from kind `first`"""
    return model_records(B, [MODELS[(first + p) % len(MODELS)] for p in range(n)])


@pytest.mark.parametrize("fallback", [0, 1])
@pytest.mark.parametrize("dim,pitch,base_off,slack", DIMS)
def test_a_model_per_pair(B, dim, pitch, base_off, slack, fallback):
    rng = np.random.default_rng(dim * 1000 + pitch + 3)
    ctx = B.default_context(0)
    A, Ak, Bs, Bk, T, Tk = sets(B, rng, dim, pitch, base_off, slack)
    nA = len(COUNTS_A)
    shuffled = [(int(a), int(b)) for a, b in zip(rng.integers(0, nA, 9), rng.integers(0, nA, 9))]
    shuffled.insert(4, shuffled[1])                                 # a repeated pair: two models for the same frames
    shuffled.insert(2, (nA, 0))                                     # out-of-range entries
    shuffled.append((0, -1))
    # (the window and the kind of the first pair's model: chosen, on the restatement alone, so that every call has all classes of rows)
    forms = [(A, Ak, A, Ak, (nA - 1, 1, 1, 0, 1), NARROW, 5),       # the chain: frame to previous frame
             (Bs, Bk, A, Ak, (nA, 0, 1, 5, 0), NARROW, 3),          # every frame against ONE keyframe (130 rows): a model per PAIR
             (A, Ak, Bs, Bk, shuffled, NARROW, 2),                  # a shuffled device list
             (A, Ak, T, Tk, (nA, 0, 1, 0, 1), GRID_WINDOW, 4)]      # side by side against 0 ... 33 train rows
    for qs, qk, ts, tk, pairs, window, first in forms:
        n = pairs[0] if isinstance(pairs, tuple) else len(pairs)
        models = cycled(B, n, first)
        for mode in ("k1", "k2", "radius"):
            run_guided(B, ctx, qs, qk, ts, tk, pairs, models, window, fallback, mode, max_distance=4 * dim + 0.5).check()
    # rows_cap cutting a frame (65 and 130 rows), and a radius row cut by cap_per_query
    for mode in ("k2", "radius"):
        run_guided(B, ctx, A, Ak, Bs, Bk, (nA, 0, 1, 0, 1), cycled(B, nA, 0), GRID_WINDOW, fallback, mode, rows_cap=64, cap=3, max_distance=1e9)
        run_guided(B, ctx, Bs, Bk, A, Ak, (nA, 0, 1, 5, 0), cycled(B, nA, 1), GRID_WINDOW, fallback, mode, rows_cap=64, cap=3, max_distance=1e9)


def test_the_keyframe_form_indexes_the_models_by_pair(B):
    """train_step = 0: every pair has the same train frame, and the translation that fits only pair p is found at d_models[p] - a
    kernel that indexed by the train frame would use one model for all"""
    rng = np.random.default_rng(77)
    ctx = B.default_context(0)
    A, Ak, Bs, Bk, T, Tk = sets(B, rng, 48, 64, 0, 0)
    nA = len(COUNTS_A)
    models = model_records(B, [((1.0, 0.0, 8.0 * (p - 3), 0.0, 1.0, 8.0 * (p % 3 - 1), 0.0, 0.0, 1.0), p, 0) for p in range(nA)])
    pairs = (nA, 0, 1, 1, 0)                                        # all of A against Bs' frame 1 (130 rows)
    masks = [guide_mask((0.0, 0.0, 0.0, 0.0, -1), 0, models[p], Ak.kps[p], Bk.kps[1])[0] for p in range(nA)]
    by_frame = [guide_mask((0.0, 0.0, 0.0, 0.0, -1), 0, models[1], Ak.kps[p], Bk.kps[1])[0] for p in range(nA)]
    assert sum(not np.array_equal(m, f) for m, f in zip(masks, by_frame)) >= 4    # the two readings differ on the restatement
    run_guided(B, ctx, A, Ak, Bs, Bk, pairs, models, (0.0, 0.0, 0.0, 0.0, -1), 0, "k2")


# ---- the radius kernel's dense path: rows with exactly 32 and 33 hits ---------------------------------------------------------------

class Kp:
    """given keypoint records for the frames of a set"""

    def __init__(self, B, kps, cap):
        import torch
        pitch = cap * B.KEYPOINT.itemsize
        buf = np.full(len(kps) * pitch + 64, 0xA5, np.uint8)
        for f, k in enumerate(kps):
            buf[f * pitch:f * pitch + k.nbytes] = k.view(np.uint8)
        self.kps, self.t_buf = kps, torch.from_numpy(buf).cuda()
        self.set = B.KpSet(self.t_buf.data_ptr(), pitch)


def test_rows_with_32_and_33_hits(B):
    """every allowed train row hits (the distance bound is off): query row 0's window holds exactly 32 train keypoints - the last row
    of the LDS list -, row 1's 33 - the first dense row -, under a projective model; rows 2 and 3 the same counts through the fallback
    of an unguided pair"""
    rng = np.random.default_rng(5)
    ctx = B.default_context(0)
    nq, nt = 66, 70
    A = SynthSet(B, rng, 32, 32, [nq, nq], CAP)
    Ts = SynthSet(B, rng, 32, 36, [nt, nt], CAP)
    h = (2.0, 0.0, 20.0, 0.0, 2.0, 10.0, 0.0, 0.001, 2.0)           # centre = (x + 10, y + 5) / (1 + y / 2000)
    models = model_records(B, [(h, 0, 0), (h, 0, PAIR_NO_MODEL)])
    kq = np.zeros(nq, B.KEYPOINT)
    kq["x"], kq["y"], kq["octave"] = 4000.0 + 100.0 * np.arange(nq), 0.0, 1
    kq["x"][:2] = (100.0, 300.0)
    kt = np.zeros(nt, B.KEYPOINT)
    kt["x"], kt["y"], kt["octave"] = 9000.0, 9000.0, 1
    window = (-3.0, 3.0, -3.0, 3.0, 0)
    order = rng.permutation(nt)                                     # the hits scattered over the waves' slices
    near0, near1 = order[:32], order[32:65]
    kps_t = []
    for guided in (True, False):
        k = kt.copy()
        c0, c1 = ((110.0, 5.0), (310.0, 5.0)) if guided else ((100.0, 0.0), (300.0, 0.0))
        k["x"][near0], k["y"][near0] = c0[0] + rng.integers(-12, 13, 32) / 4, c0[1] + rng.integers(-12, 13, 32) / 4
        k["x"][near1], k["y"][near1] = c1[0] + rng.integers(-12, 13, 33) / 4, c1[1] + rng.integers(-12, 13, 33) / 4
        kps_t.append(k)
    Ak, Tk = Kp(B, [kq, kq], CAP), Kp(B, kps_t, CAP)
    for p in range(2):
        M, has = guide_mask(window, 1, models[p], kq, kps_t[p])
        assert has.all() and M[0].sum() == LIST and M[1].sum() == LIST + 1 and M[2:].sum() == 0
    for cap in (40, 5):
        tally = run_guided(B, ctx, A, Ak, Ts, Tk, (2, 0, 1, 0, 1), models, window, 1, "radius", cap=cap, max_distance=1e9)
        assert sorted(tally.allowed)[-4:] == [LIST, LIST, LIST + 1, LIST + 1]
    run_guided(B, ctx, A, Ak, Ts, Tk, (2, 0, 1, 0, 1), models, window, 1, "radius", cap=40, max_distance=4 * 32 * 0.6)   # a real threshold


# ---- 3: nothing behind counts or beyond rows is written ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["k1", "k2", "radius"])
def test_nothing_behind_counts_or_beyond_rows_is_written(B, mode):
    import torch
    rng = np.random.default_rng(12)
    ctx = B.default_context(0)
    A, Bs = SynthSet(B, rng, 48, 64, COUNTS_A, CAP), SynthSet(B, rng, 48, 64, COUNTS_B, CAP)
    Ak, Bk = SynthKp(B, rng, COUNTS_A, CAP, nan_every=17), SynthKp(B, rng, COUNTS_B, CAP, slack=12)
    nA, rows_cap = len(COUNTS_A), 64
    per = {"k1": 1, "k2": 2, "radius": 6}[mode]
    # every kind; the pairs with many rows on both sides (0, 4, 5) get the translation, the similarity and the projective model
    models = model_records(B, [MODELS[i] for i in (0, 3, 4, 5, 1, 2, 6, 7)])
    d_models = upload_models(models)
    out = sentinel_outputs(nA, rows_cap, per)
    spec, guide = B.PairSpec(nA, 0, 1, 0, 1, None), guide_of(B, GRID_WINDOW, 0)
    torch.cuda.synchronize()
    if mode == "radius":
        ctx.match_radius_pairs_guided(A.set, Bs.set, spec, 4 * 48 + 0.5, per, d_models, guide, rows_cap=rows_cap, query_kps=Ak.set, train_kps=Bk.set,
                                      dim_bytes=48, out=out)
    else:
        ctx.match_knn_pairs_guided(A.set, Bs.set, spec, per, d_models, guide, rows_cap=rows_cap, query_kps=Ak.set, train_kps=Bk.set, dim_bytes=48,
                                   out=out)
    torch.cuda.synchronize()
    m, cnt, rows = (t.cpu().numpy() for t in out)
    assert np.array_equal(rows, np.array(COUNTS_A))                 # the TRUE counts, also where rows were cut or the pair is unguided
    m = m.view(B.DMATCH).reshape(nA, rows_cap, per)
    sent = np.full(4, SENTINEL, np.int32).view(B.DMATCH)[0]
    stored = 0
    for p in range(nA):
        M, _ = guide_mask(GRID_WINDOW, 0, models[p], Ak.kps[p], Bk.kps[p])
        want = oracle_radius(A.desc[p], Bs.desc[p], M, p, 4 * 48 + 0.5) if mode == "radius" else oracle_knn(A.desc[p], Bs.desc[p], M, p, per)
        nrows = min(COUNTS_A[p], rows_cap)
        same_cut([m[p, q, :min(cnt[p, q], per)] for q in range(nrows)], cnt[p, :nrows], want[:rows_cap], per)
        stored += int(np.minimum(cnt[p, :nrows], per).sum())
        for q in range(nrows):                                      # entries behind min(count, entries per row): untouched
            assert all(e == sent for e in m[p, q, min(cnt[p, q], per):])
        assert (cnt[p, nrows:] == SENTINEL).all()                   # rows beyond min(n_a, rows_cap): untouched
        assert (m[p, nrows:].view(np.int32) == SENTINEL).all()
    assert stored >= 10


# ---- 4: the real path, no host in between -----------------------------------------------------------------------------------------

SELECT, VERIFY = (90.0, 0.8, 1), (3.0, 256, 12, 0, 2024)
GUIDE_WINDOW, RESELECT = (-6.0, 6.0, -6.0, 6.0, 1), (90.0, 0.0, 1)


def near_h(kq, kt, rec, bound=5.0):
    """records whose train keypoint lies within `bound` pixels of H_1TO2's image of the query keypoint"""
    x, y = kq["x"][rec["queryIdx"]].astype(np.float64), kq["y"][rec["queryIdx"]].astype(np.float64)
    p = H_1TO2 @ np.stack([x, y, np.ones(len(x))])
    return int((np.hypot(p[0] / p[2] - kt["x"][rec["trainIdx"]], p[1] / p[2] - kt["y"][rec["trainIdx"]]) <= bound).sum())


def restated_guided_chain(B, desc, kps, rows_cap, first):
    """everything behind the first k-NN call, restated: select, verify, the guided k-NN (k = 1) under the restated models, select, link.
    first: the padded arrays of the k = 2 call on the host."""
    n = len(desc)
    node_rows = [len(k) for k in kps]
    xy = [np.stack([k["x"], k["y"]], axis=1).astype(np.float32).reshape(-1, 2) for k in kps]
    sel = restated_select(first, 2, SELECT)
    in_cap = (n - 1) * rows_cap * 2
    ver = restated_verify(chain_frames(n - 1), node_rows, node_rows, rows_cap, xy, xy, sel[3], sel[0], VERIFY, in_cap, in_cap)
    models = ver[0]
    rows = [oracle_knn(desc[p + 1], desc[p], guide_mask(GUIDE_WINDOW, 0, models[p], kps[p + 1], kps[p])[0], p, 1)[:rows_cap] for p in range(n - 1)]
    m = np.zeros((n - 1, rows_cap, 1), B.DMATCH)
    cnt = np.zeros((n - 1, rows_cap), np.int32)
    for p, rr in enumerate(rows):
        for q, r in enumerate(rr):
            m[p, q, :len(r)], cnt[p, q] = r, len(r)
    resel = restated_select((m, cnt, np.array(node_rows[1:], np.int32)), 1, RESELECT)
    link = restated_link(node_rows, rows_cap, resel[3], resel[0])
    return {"select": sel, "verify": ver, "guided": rows, "reselect": resel, "link": link}


def test_the_real_path_without_the_host(B, golden_ast):
    """detect + describe, k-NN (k = 2), select (ratio 0.8), verify, guided k-NN (k = 1, +-6 px, fallback 0) reading the verifier's models
    in place, select (keep 1), link - one stream, one synchronisation at the end; every array against the restated chain.
    For pair 0 (img1 -> img2, known H_1TO2) the records within 5 px of H_1TO2 in the verified list and in the guided list are printed.
    That the guided list holds at least as many of them as the verified one was decided on the CPU first, where it is deterministic:
    the oracle's keypoints and descriptors of these frames through restated_guided_chain give 243 verified records, all 243 within
    5 px, and 280 guided ones, 276 within 5 px (1951 links over the batch from the verified lists, 2089 from the guided ones).  So it
    is asserted."""
    import torch
    frames = batch_frames(golden_ast)
    n, h, w = frames.shape
    d = torch.from_numpy(frames).cuda()
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    first = ctx.match_knn_pairs(st, st, spec, 2, stream=s.cuda_stream)
    rows_cap = int(first[1].shape[1])
    sel = ctx.select_pair_matches(first, 2, B.MatchSelect(*SELECT), stream=s.cuda_stream)
    ver = ctx.verify_pair_matches(st, st, spec, rows_cap, sel[3], sel[0], B.PairVerify(*VERIFY), stream=s.cuda_stream)
    guided = ctx.match_knn_pairs_guided(st, st, spec, 1, ver[4], guide_of(B, GUIDE_WINDOW, 0), rows_cap=rows_cap, stream=s.cuda_stream)
    resel = ctx.select_pair_matches(guided, 1, B.MatchSelect(*RESELECT), stream=s.cuda_stream)
    linked = ctx.link_tracks((st, 0, 1), n, rows_cap, resel[3], resel[0], stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    kd = [ctx.batch_download(f, True, strings=dim) for f in range(n)]
    kps, desc = [k for k, _ in kd], [dd for _, dd in kd]
    counts = np.array([len(k) for k in kps])
    assert counts[3] == 0 and (np.delete(counts, 3) > 0).all()     # the blank frame is inside the batch
    hfirst = host_triple(B, first, 2)
    got_first, _ = knn_rows(B, tuple(t.cpu().numpy() for t in first), 2)
    for p in range(n - 1):
        same_rows(got_first[p], oracle_pair(desc[p + 1], desc[p], p, 2))
    want = restated_guided_chain(B, desc, kps, rows_cap, hfirst)
    for name, got, exp in (("select", sel, want["select"]), ("reselect", resel, want["reselect"])):
        gm, gc, gf, go = (t.cpu().numpy() for t in got)
        assert np.array_equal(gc, exp[1]) and np.array_equal(gf, exp[2]) and np.array_equal(go, exp[3]), name
        assert gm.view(B.DMATCH).reshape(-1)[:len(exp[0])].tobytes() == exp[0].tobytes(), name
    models, vcounts, vflags, voffs, vstored = want["verify"]
    assert ver[4].cpu().numpy().tobytes() == models.tobytes()
    assert ver[1].cpu().numpy().tobytes() == vcounts.tobytes() and ver[2].cpu().numpy().tobytes() == vflags.tobytes()
    assert ver[3].cpu().numpy().tobytes() == voffs.tobytes() and ver[0].cpu().numpy()[:len(vstored)].tobytes() == vstored.tobytes()
    is_guided = (models["hypothesis"] >= 0) & ((models["flags"] & (PAIR_BAD | PAIR_NO_MODEL)) == 0)
    assert is_guided[0] and not is_guided[2] and not is_guided[3]   # the pairs around the blank frame have no model
    got_rows, pair_rows = knn_rows(B, tuple(t.cpu().numpy() for t in guided), 1)
    assert np.array_equal(pair_rows, counts[1:])
    for p in range(n - 1):
        same_rows(got_rows[p], want["guided"][p])
        if not is_guided[p]:
            assert all(len(r) == 0 for r in got_rows[p])
    wl, gl = want["link"], tuple(t.cpu().numpy() for t in linked)
    wrote = wl[0] != SENT32
    for name, g, w_ in zip(("prev", "track", "age"), gl, wl):
        assert np.array_equal(g[wrote], w_[wrote]), name
    assert gl[3].tolist() == wl[3].tolist()
    g0 = want["reselect"][0][:int(want["reselect"][3][1])]
    v0 = vstored[:int(voffs[1])]
    nv, ng = near_h(kps[1], kps[0], v0), near_h(kps[1], kps[0], g0)
    print("pair 0: %d verified records, %d within 5 px of H_1TO2; %d guided records, %d within 5 px; links made over the batch: %d" %
          (len(v0), nv, len(g0), ng, int(wl[3][2])))
    assert nv > 50 and ng >= nv
    ext.close()
    ctx.close()


# ---- 5: stream order ----------------------------------------------------------------------------------------------------------------

GUIDED_K = 1


@pytest.fixture(scope="module")
def guided_env(env):
    """the held-stream environment of tests/test_gpu_stream_order.py, and the guided call's serial outputs for its two batches"""
    e, torch = env, env.torch
    e.guide = e.B.MatchGuide(e.B.MatchGate(-6.0, 6.0, -6.0, 6.0, 1), 1)
    e.guided_out = tuple(torch.empty(s, dtype=torch.int32, device="cuda") for s in ((e.n - 1, e.cap, GUIDED_K, 4), (e.n - 1, e.cap), (e.n - 1,)))
    e.guided_serial = {}
    for b in (1, 2):
        assert run_batch(e, b, sptr(e.main)) == 0
        fill_guided(e)
        assert call_guided(e, b, sptr(e.main)) == 0
        torch.cuda.synchronize()
        e.guided_serial[b] = [t.cpu().numpy().copy() for t in e.guided_out]
    for a1, a2 in zip(*e.guided_serial.values()):                   # a case on equal bytes would prove nothing
        assert a1.tobytes() != a2.tobytes()
    return e


def fill_guided(e):
    for t in e.guided_out:
        t.view(e.torch.uint8).fill_(0x5A)
    e.torch.cuda.synchronize()


def call_guided(e, b, s):
    """the guided k-NN call on the context's own sets, under the models the serial verification of batch b wrote (caller memory)"""
    m, cnt, rows = e.guided_out
    return e.L.brisk_hip_match_knn_pairs_guided_device(e.h, C.byref(e.st), C.byref(e.st), C.byref(e.kp), C.byref(e.kp), C.byref(e.spec),
                                                       C.c_void_p(e.serial_dev[b]["verify"][4].data_ptr()), C.byref(e.guide), e.dim, GUIDED_K,
                                                       e.cap, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), s)


def compare_guided(e, b):
    for name, t, w in zip(("matches", "counts", "pair_rows"), e.guided_out, e.guided_serial[b]):
        g = t.cpu().numpy()
        assert g.tobytes() == w.tobytes(), "%s is not the serial run's of batch %d; equal to batch %d's: %s" % (
            name, b, 3 - b, g.tobytes() == e.guided_serial[3 - b][["matches", "counts", "pair_rows"].index(name)].tobytes())


def test_write_after_read(guided_env):
    """batch 1 complete; the guided call on the held S, batch 2 - which overwrites the descriptors, keypoints and counts it is given - on
    S2.  Its outputs are batch 1's: batch 2 waited for it."""
    e = guided_env
    begin(e)
    fill_guided(e)
    race(e, lambda s: call_guided(e, 1, s), lambda s: run_batch(e, 2, s))
    compare_guided(e, 1)


def test_read_after_write(guided_env):
    """batch 1 complete; batch 2 on the held S, the guided call - given batch 2's models - on S2.  Its outputs are batch 2's: it waited
    for the batch."""
    e = guided_env
    begin(e)
    fill_guided(e)
    race(e, lambda s: run_batch(e, 2, s), lambda s: call_guided(e, 2, s))
    compare_guided(e, 2)


# ---- 6: arguments -----------------------------------------------------------------------------------------------------------------

def test_arguments(B):
    import torch
    rng = np.random.default_rng(3)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, 48, 64, COUNTS_A, CAP, count_stride=1)
    Ak = SynthKp(B, rng, COUNTS_A, CAP)
    nA, cpq = len(COUNTS_A), 2
    out = sentinel_outputs(nA, CAP, cpq)
    d_models = upload_models(model_records(B, [(IDENTITY, 0, 0)] * nA))
    torch.cuda.synchronize()
    m, cnt, rows = (t.data_ptr() for t in out)
    L, h = ctx._L, ctx._h
    guide = guide_of(B, GRID_WINDOW, 1)
    ARG, UNSUPPORTED = 1, 7

    def ref(x):
        return None if x is None else C.byref(x)

    def knn(q=A.set, t=A.set, qk=Ak.set, tk=Ak.set, md=d_models.data_ptr(), g=guide, spec=(nA - 1, 1, 1, 0, 1, None), dim=48, k=2, cap=CAP, m=m,
            cnt=cnt, rows=rows):
        return L.brisk_hip_match_knn_pairs_guided_device(h, ref(q), ref(t), ref(qk), ref(tk), C.byref(B.PairSpec(*spec)), md, ref(g), dim, k, cap,
                                                         m, cnt, rows, None)

    def radius(q=A.set, t=A.set, qk=Ak.set, tk=Ak.set, md=d_models.data_ptr(), g=guide, spec=(nA - 1, 1, 1, 0, 1, None), dim=48, r=200.0, cpq=cpq,
               cap=CAP, m=m, cnt=cnt, rows=rows):
        return L.brisk_hip_match_radius_pairs_guided_device(h, ref(q), ref(t), ref(qk), ref(tk), C.byref(B.PairSpec(*spec)), md, ref(g), dim, r,
                                                            cpq, cap, m, cnt, rows, None)

    for call in (knn, radius):
        # the guide's own arguments
        assert call(md=None) == ARG and call(md=d_models.data_ptr() + 4) == ARG and call(g=None) == ARG
        # ... the gated calls' keypoint sets
        assert call(qk=None) == ARG and call(tk=None) == ARG
        assert call(qk=B.KpSet(None, CAP * 28)) == ARG and call(tk=B.KpSet(None, CAP * 28)) == ARG
        assert call(qk=B.KpSet(Ak.set.d_kps + 2, CAP * 28)) == ARG and call(tk=B.KpSet(Ak.set.d_kps, CAP * 28 + 2)) == ARG
        assert call(tk=B.KpSet(Ak.set.d_kps, -28)) == ARG
        # ... and those of the ungated calls
        assert call(dim=40) == UNSUPPORTED and call(dim=96) == UNSUPPORTED
        assert call(spec=(nA, 1, 1, 0, 1, None)) == ARG            # the last pair's query frame is outside the set
        assert call(spec=(nA, 0, 1, -1, 1, None)) == ARG
        assert call(spec=(-1, 0, 1, 0, 1, None)) == ARG
        assert call(cap=0) == ARG
        narrow = B.DescSet(A.set.d_desc, A.set.d_counts, 1, A.set.frame_pitch, 40, nA)
        assert call(q=narrow) == ARG and call(t=narrow) == ARG      # row_pitch < dim_bytes
        assert call(m=None) == ARG and call(cnt=None) == ARG and call(rows=None) == ARG
        assert call(q=None) == ARG and call(t=None) == ARG
        assert call(spec=(0, 0, 1, 0, 1, None)) == 0                # no pairs: fine, nothing to do ...
        assert call(spec=(0, 0, 1, 0, 1, None), qk=None, tk=None, md=None, g=None, m=None, cnt=None, rows=None) == 0   # ... nothing is looked at
    assert knn(k=3) == ARG and knn(k=0) == ARG
    assert radius(cpq=0) == ARG and radius(cpq=-1) == ARG
    with pytest.raises(B.BriskHipError) as ei:
        ctx.match_knn_pairs_guided(A.set, A.set, B.PairSpec(2, 0, 1, 0, 1, None), 3, d_models, guide, rows_cap=CAP, query_kps=Ak.set,
                                   train_kps=Ak.set, dim_bytes=48, out=out)
    assert ei.value.code == ARG
    torch.cuda.synchronize()
    for t in out:                                                   # none of these calls launched anything
        assert (t.cpu().numpy() == SENTINEL).all()
    # models that guide nothing are no error: with fallback 0 every row is empty (a device pointer instead of a tensor)
    none = upload_models(model_records(B, [MODELS[5]] * nA))
    ctx.match_knn_pairs_guided(A.set, A.set, B.PairSpec(nA, 0, 1, 0, 1, None), cpq, none.data_ptr(), guide_of(B, GRID_WINDOW, 0), rows_cap=CAP,
                               query_kps=Ak.set, train_kps=Ak.set, dim_bytes=48, out=out)
    torch.cuda.synchronize()
    hm, hc, hr = (t.cpu().numpy() for t in out)
    assert list(hr) == COUNTS_A and (hm == SENTINEL).all()
    for p in range(nA):
        assert (hc[p, :COUNTS_A[p]] == 0).all() and (hc[p, COUNTS_A[p]:] == SENTINEL).all()
