"""GPU tests of brisk_hip_match_knn_pairs_epipolar_guided_device / brisk_hip_match_radius_pairs_epipolar_guided_device: the gated pair
matchers behind a band around each query keypoint's epipolar line under the pair's model.  The guide defines a mask per pair
(tests/test_abi_match_epiline.py restates it in NumPy); everything is compared with the CPU oracle matching with that mask, as the
gated and guided matchers' tests do - integer fields equal, distances equal as bit patterns, counts equal: no tolerance."""
import ctypes as C

import numpy as np
import pytest

from test_abi_epipolar import restated_inliers8
from test_abi_match_epiline import PAIR_BAD, PAIR_NO_MODEL, RECTIFIED, cross, is_guided, restated_lines, scaled
from test_abi_tracks import SENT32, restated_link
from test_gpu_epipolar import depth_scene
from test_gpu_match_export import expect as restated_select, host_triple
from test_gpu_match_gated import SynthKp, gate_mask, knn_rows, oracle_knn, oracle_radius, same_cut, sentinel_outputs, spec_of
from test_gpu_match_pairs import CAP, COUNTS_A, COUNTS_B, SENTINEL, SynthSet, same_rows
from test_gpu_stream_order import env, finish, hold, sptr  # noqa: F401 (env: the fixture of the held stream)
from test_gpu_verify import CAP as SCENE_CAP

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
COUNTS_T = [0, 1, 3, 4, 5, 8, 9, 33]        # train rows around the waves' chunks of four and their eight slices
LIST = 32                                   # MRP_LIST: radius rows with more hits take the kernel's dense path
# test 1: on SynthKp's grid of 8 pixels the differences hit the bounds exactly
STEREO_WINDOW, STEREO_BAND, STEREO_GATE = (-16.0, 16.0, -INF, INF, 1), 8.0, (-16.0, 16.0, -8.0, 8.0, 1)
STEREO_MODELS = [(scaled(RECTIFIED, 1.0), 0, 0), (scaled(RECTIFIED, 0.5), 4095, 0x100), (scaled(RECTIFIED, -2.0), 7, 0)]
# test 2: (f, hypothesis, flags), one of each kind.  SynthKp's keypoints lie on x = 0, 8 ... 56, y = 0, 8 ... 40
GENERAL = (0.0005, -0.001, 0.05, 0.00125, 0.00025, -0.375, -0.06, 0.35, 0.75)      # every element scaled by 0.5
MODELS = [(scaled(RECTIFIED, 1.0), 0, 0),                                           # rectified
          (cross(24.0, 16.0), 7, 0x100),                                            # [e]_x, e a grid keypoint: a row at e has no line
          (GENERAL, 4095, 0x1),                                                     # a general F
          (tuple(NAN if i == 5 else v for i, v in enumerate(GENERAL)), 1, 0),       # a NaN element: no row has a line
          ((0.0,) * 9, 2, 0),                                                       # the zero model
          (scaled(RECTIFIED, 1.0), -1, 0),                                          # no valid hypothesis
          (scaled(RECTIFIED, 1.0), 3, PAIR_NO_MODEL),
          ((NAN,) * 9, 0, PAIR_BAD)]
BAND = 3.0
WIDE_WINDOW = (-24.0, 24.0, -16.0, 16.0, 1)
NARROW = (-8.0, 8.0, -8.0, 8.0, 0)          # nine grid positions and one octave: dense frames keep rows with 0, 1 and many allowed
SPARSE = (-40.0, 40.0, -24.0, 24.0, -1)     # for train frames of a few rows


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


def model_records(B, models):
    rec = np.zeros(len(models), B.PAIR_EPIPOLAR_MODEL)
    for i, (f, hyp, flags) in enumerate(models):
        rec[i]["f"], rec[i]["hypothesis"], rec[i]["flags"] = f, hyp, flags
        rec[i]["records"], rec[i]["usable"], rec[i]["inliers"], rec[i]["valid"] = -1, -2, -3, -4     # (not read)
    return rec


def upload_models(rec):
    import torch
    return torch.from_numpy(rec.view(np.int64).reshape(len(rec), 12).copy()).cuda()


def epi_mask(window, band, fallback, model, kq, kt):
    """M[q][t] for one pair: the gate's mask of `window` between the keypoints themselves, and - in a guided pair - the band around
    the restated line of each query row, no row without a line.  model: a PAIR_EPIPOLAR_MODEL record.  Also returns has-line per
    query row."""
    G = gate_mask(window, kq, kt).astype(bool)
    l0, l1, l2, w, has = restated_lines(model["f"], model["hypothesis"], model["flags"], np.float32(band), kq["x"], kq["y"])
    if not is_guided(model["hypothesis"], model["flags"]):
        return np.ascontiguousarray((G if fallback else np.zeros_like(G)).astype(np.uint8)), np.zeros(len(kq), bool)
    tx, ty = kt["x"].astype(np.float32).astype(np.float64), kt["y"].astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        r = (tx[None, :] * l0[:, None] + ty[None, :] * l1[:, None]) + l2[:, None]
        ok = r * r <= w[:, None]
    return np.ascontiguousarray((G & ok & has[:, None]).astype(np.uint8)), has


def guide_of(B, window, band, fallback):
    return B.MatchEpipolarGuide(B.MatchGate(*window), band, fallback)


class Tally:
    """what a call's restated masks hold: allowed train rows per query row, guided and unguided pairs, rows without a line inside a
    guided pair"""

    def __init__(self):
        self.allowed, self.guided, self.unguided, self.no_line = [], 0, 0, 0

    def add(self, M, has, model, rows):
        g = bool(is_guided(model["hypothesis"], model["flags"]))
        self.guided, self.unguided = self.guided + g, self.unguided + (not g)
        self.no_line += int((~has[:rows]).sum()) if g else 0
        self.allowed += [int(a) for a in M[:rows].sum(axis=1)] if M.size else [0] * rows

    def check(self):
        a = np.array(self.allowed)
        assert (a == 0).sum() >= 1 and (a == 1).sum() >= 1 and (a > 2).sum() >= 1, np.bincount(a)
        assert self.unguided >= 1 and self.guided >= 1 and self.no_line >= 1


def restated_call(qs, qk, ts, tk, plist, models, window, band, fallback, rows_cap):
    """per pair (None for a bad entry of the list) the restated mask, and the Tally of the call: no GPU is needed for either"""
    masks, tally = [], Tally()
    for p, (a, b) in enumerate(plist):
        if not (0 <= a < len(qs.desc) and 0 <= b < len(ts.desc)):
            masks.append(None)
            continue
        M, has = epi_mask(window, band, fallback, models[p], qk.kps[a], tk.kps[b])
        tally.add(M, has, models[p], min(len(qs.desc[a]), rows_cap))
        masks.append(M)
    return masks, tally


def run_epiline(B, ctx, qs, qk, ts, tk, pairs, models, window, band, fallback, mode, rows_cap=CAP, cap=8, max_distance=None):
    """one call against the oracle under the restated masks; models: PAIR_EPIPOLAR_MODEL records, one per pair.  Returns the Tally."""
    import torch
    spec, plist, keep = spec_of(B, pairs)
    assert len(models) == len(plist)
    d_models = upload_models(models)
    guide = guide_of(B, window, band, fallback)
    masks, tally = restated_call(qs, qk, ts, tk, plist, models, window, band, fallback, rows_cap)
    torch.cuda.synchronize()
    if mode == "radius":
        got, counts = ctx.match_radius_pairs_epipolar_guided(qs.set, ts.set, spec, max_distance, cap, d_models, guide, rows_cap=rows_cap,
                                                             query_kps=qk.set, train_kps=tk.set, dim_bytes=qs.dim, download=True)
    else:
        k = {"k1": 1, "k2": 2}[mode]
        got = ctx.match_knn_pairs_epipolar_guided(qs.set, ts.set, spec, k, d_models, guide, rows_cap=rows_cap, query_kps=qk.set,
                                                  train_kps=tk.set, dim_bytes=qs.dim, download=True)
        counts = [None] * len(got)
    assert len(got) == len(plist)
    for (a, b), M, rows, c in zip(plist, masks, got, counts):
        if M is None:
            assert rows == [] and (c is None or len(c) == 0)        # a bad entry of the list: d_pair_rows -1, no rows
        elif mode == "radius":
            same_cut(rows, c, oracle_radius(qs.desc[a], ts.desc[b], M, b, max_distance)[:rows_cap], cap)
        else:
            same_rows(rows, oracle_knn(qs.desc[a], ts.desc[b], M, b, k)[:rows_cap])
    return tally


def sets(B, rng, dim, pitch, base_off, slack, spread=(8, 6)):
    """the query set A and the train sets Bs and T (COUNTS_T) with their keypoints; spread: the grid positions Bs' keypoints take"""
    A = SynthSet(B, rng, dim, pitch, COUNTS_A, CAP, base_off, 3, slack)
    Bs = SynthSet(B, rng, dim, pitch + 4 * (dim == 48), COUNTS_B, CAP, 0, 1, 0)
    T = SynthSet(B, rng, dim, pitch, COUNTS_T, CAP, 0, 2, 0)
    Ak = SynthKp(B, rng, COUNTS_A, CAP, slack=40, nan_every=17)
    Bk = SynthKp(B, rng, COUNTS_B, CAP, nan_every=23, spread=spread)
    Tk = SynthKp(B, rng, COUNTS_T, CAP)
    return A, Ak, Bs, Bk, T, Tk


DIMS = [(16, 20, 0, 0), (32, 48, 0, 4), (48, 64, 0, 0), (48, 51, 1, 3), (64, 64, 0, 0)]


# ---- 1: rectified models = the gated matcher --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,pitch,base_off,slack", DIMS)
def test_rectified_models_equal_the_gated_matcher(B, dim, pitch, base_off, slack):
    """F = s [0 0 0; 0 0 -1; 0 1 0] at three scales, band 8 and no bound on dy: all three output arrays equal the gated matcher's
    with dy in [-8, 8], byte for byte, the sentinel-filled parts included"""
    import torch
    rng = np.random.default_rng(dim * 1000 + pitch + 4)
    ctx = B.default_context(0)
    A, Ak, Bs, Bk, T, Tk = sets(B, rng, dim, pitch, base_off, slack, spread=(4, 3))     # (dense enough for rows with more than 32 hits)
    nA = len(COUNTS_A)
    d_models = upload_models(model_records(B, [STEREO_MODELS[p % 3] for p in range(nA)]))
    spec = B.PairSpec(nA, 0, 1, 0, 1, None)
    gate, guide = B.MatchGate(*STEREO_GATE), guide_of(B, STEREO_WINDOW, STEREO_BAND, 0)
    # the dense path of the radius kernel is taken: with the distance bound off a row has as many hits as the gate allows
    assert max(int(gate_mask(STEREO_GATE, Ak.kps[p], Bk.kps[p]).sum(axis=1).max()) for p in range(nA) if COUNTS_A[p] and COUNTS_B[p]) > LIST
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
                    ctx.match_radius_pairs_epipolar_guided(A.set, ts.set, spec, r, per, d_models, guide, rows_cap=rows_cap, query_kps=Ak.set,
                                                           train_kps=tk.set, dim_bytes=dim, out=got)
                else:
                    ctx.match_knn_pairs(A.set, ts.set, spec, per, rows_cap=rows_cap, dim_bytes=dim, out=want, gate=gate, query_kps=Ak.set,
                                        train_kps=tk.set)
                    ctx.match_knn_pairs_epipolar_guided(A.set, ts.set, spec, per, d_models, guide, rows_cap=rows_cap, query_kps=Ak.set,
                                                        train_kps=tk.set, dim_bytes=dim, out=got)
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


def pair_forms(rng, A, Ak, Bs, Bk, T, Tk):
    """(query set, its keypoints, train set, its keypoints, pairs, window, band, kind of the first pair's model).  Window, band and the
    first kind are chosen, on the restatement alone, so that every call has all classes of rows (Tally.check)"""
    nA = len(COUNTS_A)
    shuffled = [(int(a), int(b)) for a, b in zip(rng.integers(0, nA, 9), rng.integers(0, nA, 9))]
    shuffled.insert(4, shuffled[1])                                 # a repeated pair: two models for the same frames
    shuffled.insert(2, (nA, 0))                                     # out-of-range entries
    shuffled.append((0, -1))
    return [(A, Ak, A, Ak, (nA - 1, 1, 1, 0, 1), WIDE_WINDOW, BAND, 5),   # the chain: frame to previous frame
            (Bs, Bk, A, Ak, (nA, 0, 1, 5, 0), NARROW, BAND, 7),           # every frame against ONE keyframe (130 rows): a model per PAIR
            (A, Ak, Bs, Bk, shuffled, WIDE_WINDOW, BAND, 2),              # a shuffled device list
            (A, Ak, T, Tk, (nA, 0, 1, 0, 1), SPARSE, 9.0, 4)]             # side by side against 0 ... 33 train rows


@pytest.mark.parametrize("fallback", [0, 1])
@pytest.mark.parametrize("dim,pitch,base_off,slack", DIMS)
def test_a_model_per_pair(B, dim, pitch, base_off, slack, fallback):
    rng = np.random.default_rng(dim * 1000 + pitch + 5)
    ctx = B.default_context(0)
    A, Ak, Bs, Bk, T, Tk = sets(B, rng, dim, pitch, base_off, slack)
    nA = len(COUNTS_A)
    for qs, qk, ts, tk, pairs, window, band, first in pair_forms(rng, A, Ak, Bs, Bk, T, Tk):
        n = pairs[0] if isinstance(pairs, tuple) else len(pairs)
        models = cycled(B, n, first)
        for mode in ("k1", "k2", "radius"):
            run_epiline(B, ctx, qs, qk, ts, tk, pairs, models, window, band, fallback, mode, max_distance=4 * dim + 0.5).check()
    # rows_cap cutting a frame (65 and 130 rows), a radius row cut by cap_per_query, a window of one octave and a wide band
    for mode in ("k2", "radius"):
        run_epiline(B, ctx, A, Ak, Bs, Bk, (nA, 0, 1, 0, 1), cycled(B, nA, 0), NARROW, 9.0, fallback, mode, rows_cap=64, cap=3, max_distance=1e9)
        run_epiline(B, ctx, Bs, Bk, A, Ak, (nA, 0, 1, 5, 0), cycled(B, nA, 1), NARROW, 9.0, fallback, mode, rows_cap=64, cap=3, max_distance=1e9)


def test_the_keyframe_form_indexes_the_models_by_pair(B):
    """train_step = 0: every pair has the same train frame, and the line x' = x + 8 (p - 3) that fits only pair p is found at
    d_models[p] - a kernel that indexed by the train frame would use one model for all"""
    rng = np.random.default_rng(78)
    ctx = B.default_context(0)
    A, Ak, Bs, Bk, T, Tk = sets(B, rng, 48, 64, 0, 0)
    nA = len(COUNTS_A)
    models = model_records(B, [((0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0, -8.0 * (p - 3)), p, 0) for p in range(nA)])
    window = (-INF, INF, -8.0, 8.0, -1)
    masks = [epi_mask(window, 0.5, 0, models[p], Ak.kps[p], Bk.kps[1])[0] for p in range(nA)]
    by_frame = [epi_mask(window, 0.5, 0, models[1], Ak.kps[p], Bk.kps[1])[0] for p in range(nA)]
    assert sum(not np.array_equal(m, f) for m, f in zip(masks, by_frame)) >= 4    # the two readings differ on the restatement
    run_epiline(B, ctx, A, Ak, Bs, Bk, (nA, 0, 1, 1, 0), models, window, 0.5, 0, "k2")


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


def dense_case(B, rng):
    """query rows 0 and 1 of pair 0 (a general F, the band alone) have exactly 32 and 33 train keypoints inside the band, every other
    row none; pair 1 the same counts through the fallback of an unguided pair (the window alone)"""
    nq, nt = 66, 70
    models = model_records(B, [(GENERAL, 0, 0), (GENERAL, 0, PAIR_NO_MODEL)])
    kq = np.zeros(nq, B.KEYPOINT)
    kq["x"], kq["y"], kq["octave"] = 40.0, 2000.0 + 64.0 * np.arange(nq), 1
    kq["y"][:2] = (100.0, 300.0)
    kt = np.zeros(nt, B.KEYPOINT)
    kt["x"], kt["y"], kt["octave"] = -5000.0, -5000.0, 1
    order = rng.permutation(nt)                                     # the hits scattered over the waves' slices
    near = (order[:LIST], order[LIST:2 * LIST + 1])
    guided_t, fallback_t = kt.copy(), kt.copy()
    for row, idx in enumerate(near):
        l0, l1, l2, _, _ = restated_lines(GENERAL, 0, 0, np.float32(1), kq["x"][row], kq["y"][row])
        x = 40.0 + rng.integers(-160, 161, len(idx)) / 4            # on the line (to a quarter pixel in y, far inside a band of 2)
        guided_t["x"][idx], guided_t["y"][idx] = x, np.round(-(l0 * x + l2) / l1 * 4) / 4
        fallback_t["x"][idx] = kq["x"][row] + rng.integers(-8, 9, len(idx)) / 4
        fallback_t["y"][idx] = kq["y"][row] + rng.integers(-8, 9, len(idx)) / 4
    return models, kq, [guided_t, fallback_t], (nq, nt)


DENSE_WINDOW, DENSE_BAND = (-64.0, 64.0, -128.0, 128.0, 0), 2.0


def test_rows_with_32_and_33_hits(B):
    """every allowed train row hits (the distance bound is off): the last row of the LDS list and the first dense row, where the
    query's line is made again per wave"""
    rng = np.random.default_rng(6)
    ctx = B.default_context(0)
    models, kq, kps_t, (nq, nt) = dense_case(B, rng)
    A = SynthSet(B, rng, 32, 32, [nq, nq], CAP)
    Ts = SynthSet(B, rng, 32, 36, [nt, nt], CAP)
    Ak, Tk = Kp(B, [kq, kq], CAP), Kp(B, kps_t, CAP)
    for p in range(2):
        M, has = epi_mask(DENSE_WINDOW, DENSE_BAND, 1, models[p], kq, kps_t[p])
        assert has.all() == (p == 0) and M[0].sum() == LIST and M[1].sum() == LIST + 1 and M[2:].sum() == 0
    for cap in (40, 5):
        tally = run_epiline(B, ctx, A, Ak, Ts, Tk, (2, 0, 1, 0, 1), models, DENSE_WINDOW, DENSE_BAND, 1, "radius", cap=cap, max_distance=1e9)
        assert sorted(tally.allowed)[-4:] == [LIST, LIST, LIST + 1, LIST + 1]
    run_epiline(B, ctx, A, Ak, Ts, Tk, (2, 0, 1, 0, 1), models, DENSE_WINDOW, DENSE_BAND, 1, "radius", cap=40, max_distance=4 * 32 * 0.6)


# ---- 3: unguided pairs without the fallback; nothing behind counts or beyond rows is written ----------------------------------------

@pytest.mark.parametrize("mode", ["k1", "k2", "radius"])
def test_unguided_pairs_are_empty_and_nothing_else_is_written(B, mode):
    import torch
    rng = np.random.default_rng(13)
    ctx = B.default_context(0)
    A, Bs = SynthSet(B, rng, 48, 64, COUNTS_A, CAP), SynthSet(B, rng, 48, 64, COUNTS_B, CAP)
    Ak, Bk = SynthKp(B, rng, COUNTS_A, CAP, nan_every=17), SynthKp(B, rng, COUNTS_B, CAP, slack=12)
    nA, rows_cap = len(COUNTS_A), 64
    per = {"k1": 1, "k2": 2, "radius": 6}[mode]
    # every kind; the pairs with many rows on both sides (0, 4, 5) get the rectified, the unguided NO_MODEL and the general model
    models = model_records(B, [MODELS[i] for i in (0, 3, 4, 5, 6, 2, 1, 7)])
    guided = is_guided(models["hypothesis"], models["flags"])
    assert not guided[4] and COUNTS_A[4] >= 64 and COUNTS_B[4] >= 64 and guided[0] and guided[5]
    d_models = upload_models(models)
    out = sentinel_outputs(nA, rows_cap, per)
    spec, guide = B.PairSpec(nA, 0, 1, 0, 1, None), guide_of(B, WIDE_WINDOW, BAND, 0)
    torch.cuda.synchronize()
    if mode == "radius":
        ctx.match_radius_pairs_epipolar_guided(A.set, Bs.set, spec, 4 * 48 + 0.5, per, d_models, guide, rows_cap=rows_cap, query_kps=Ak.set,
                                               train_kps=Bk.set, dim_bytes=48, out=out)
    else:
        ctx.match_knn_pairs_epipolar_guided(A.set, Bs.set, spec, per, d_models, guide, rows_cap=rows_cap, query_kps=Ak.set, train_kps=Bk.set,
                                            dim_bytes=48, out=out)
    torch.cuda.synchronize()
    m, cnt, rows = (t.cpu().numpy() for t in out)
    assert np.array_equal(rows, np.array(COUNTS_A))                 # the TRUE counts, also where rows were cut or the pair is unguided
    m = m.view(B.DMATCH).reshape(nA, rows_cap, per)
    sent = np.full(4, SENTINEL, np.int32).view(B.DMATCH)[0]
    stored = 0
    for p in range(nA):
        M, _ = epi_mask(WIDE_WINDOW, BAND, 0, models[p], Ak.kps[p], Bk.kps[p])
        want = oracle_radius(A.desc[p], Bs.desc[p], M, p, 4 * 48 + 0.5) if mode == "radius" else oracle_knn(A.desc[p], Bs.desc[p], M, p, per)
        nrows = min(COUNTS_A[p], rows_cap)
        same_cut([m[p, q, :min(cnt[p, q], per)] for q in range(nrows)], cnt[p, :nrows], want[:rows_cap], per)
        stored += int(np.minimum(cnt[p, :nrows], per).sum())
        if not guided[p]:                                           # an unguided pair: counts of zero, and nothing else of its rows
            assert (cnt[p, :nrows] == 0).all() and (m[p].view(np.int32) == SENTINEL).all()
        for q in range(nrows):                                      # entries behind min(count, entries per row): untouched
            assert all(e == sent for e in m[p, q, min(cnt[p, q], per):])
        assert (cnt[p, nrows:] == SENTINEL).all()                   # rows beyond min(n_a, rows_cap): untouched
        assert (m[p, nrows:].view(np.int32) == SENTINEL).all()
    assert stored >= 10


# ---- 4: the pipeline, no host in between ------------------------------------------------------------------------------------------

DIM = 48
SELECT, RESELECT = (90.0, 0.8, 1), (90.0, 0.0, 1)
MAX_ERROR = 1.5
PIPE_WINDOW = (-200.0, 200.0, -200.0, 200.0, 1)
SCENE_ROWS = [200, 230, 256, 180, 300]      # the last frame has more rows than rows_cap: the rows beyond it are not matched


class DepthFrames:
    """test_gpu_epipolar.depth_scene with descriptors: row r of every frame sees 3-D point r - its descriptor with a few bits
    flipped per frame, so a true match is near and a random one far -, and every fourth point has a TWIN with the same descriptor
    (repetitive texture): the ratio test of the first pass drops both, the band of the second pass tells them apart"""

    def __init__(self, B, seed, kind):
        import torch
        sc = depth_scene(B, seed, SCENE_ROWS, kind=kind)
        rng = np.random.default_rng(seed + 9000)
        sc.kps["octave"] = np.arange(sc.alloc) % 3                  # a point keeps its octave in every frame
        sc.upload()
        base = rng.integers(0, 256, (sc.alloc, DIM), dtype=np.uint8)
        base[1::4] = base[0::4][:len(base[1::4])]
        desc = np.repeat(base[None], sc.nframes, axis=0)
        for f in range(sc.nframes):
            for _ in range(12):                                     # up to 12 flipped bits a row
                desc[f, np.arange(sc.alloc), rng.integers(0, DIM, sc.alloc)] ^= (1 << rng.integers(0, 8, sc.alloc)).astype(np.uint8)
        self.sc, self.host = sc, desc
        self.d_desc = torch.from_numpy(desc).cuda()
        self.set = B.DescSet(self.d_desc.data_ptr(), sc.d_counts.data_ptr(), sc.stride, sc.alloc * DIM, DIM, sc.nframes)
        self.desc = [desc[f, :sc.rows[f]] for f in range(sc.nframes)]
        self.kps = [sc.kps[f, :sc.rows[f]] for f in range(sc.nframes)]


def queue_pipeline(B, ctx, fr, spec, stream):
    """select -> epipolar verify -> the epipolar-guided k-NN reading the models in place -> select -> link, all on `stream`"""
    sc = fr.sc
    first = ctx.match_knn_pairs(fr.set, fr.set, spec, 2, rows_cap=SCENE_CAP, stream=stream, dim_bytes=DIM)
    sel = ctx.select_pair_matches(first, 2, B.MatchSelect(*SELECT), stream=stream)
    ver = ctx.verify_pair_matches_epipolar(fr.set, fr.set, spec, SCENE_CAP, sel[3], sel[0], B.PairVerify(MAX_ERROR, 128, 12, 0, 2026),
                                           query_kps=sc.kp_set, train_kps=sc.kp_set, stream=stream)
    ep = ctx.match_knn_pairs_epipolar_guided(fr.set, fr.set, spec, 1, ver[4], guide_of(B, PIPE_WINDOW, MAX_ERROR, 0), rows_cap=SCENE_CAP,
                                             query_kps=sc.kp_set, train_kps=sc.kp_set, stream=stream, dim_bytes=DIM)
    resel = ctx.select_pair_matches(ep, 1, B.MatchSelect(*RESELECT), stream=stream)
    linked = ctx.link_tracks((fr.set, 0, 1), sc.nframes, SCENE_CAP, resel[3], resel[0], stream=stream)
    return sel, ver, ep, resel, linked


def check_pipeline(B, fr, sel, ver, ep, resel, linked, kind):
    sc, n = fr.sc, fr.sc.nframes
    models = ver[4].cpu().numpy().reshape(-1).view(B.PAIR_EPIPOLAR_MODEL)
    guided = is_guided(models["hypothesis"], models["flags"])
    assert guided.all(), models["flags"]                             # every pair of the scene has its geometry found
    got_rows, pair_rows = knn_rows(B, tuple(t.cpu().numpy() for t in ep), 1)
    assert np.array_equal(pair_rows, np.array(sc.rows[1:]))
    gained = 0
    for p in range(n - 1):
        kq, kt = fr.kps[p + 1], fr.kps[p]
        M, has = epi_mask(PIPE_WINDOW, MAX_ERROR, 0, models[p], kq, kt)
        assert has.all()
        same_rows(got_rows[p], oracle_knn(fr.desc[p + 1], fr.desc[p], M, p, 1)[:SCENE_CAP])
        # band == max_error: every returned record is a Sampson inlier of the pair's F, by the verifier's restated score
        rec = np.concatenate(got_rows[p])
        q, t = rec["queryIdx"], rec["trainIdx"]
        inl = restated_inliers8(models["f"][p][None, :], MAX_ERROR * MAX_ERROR, kq["x"][q].astype(np.float64), kq["y"][q].astype(np.float64),
                                kt["x"][t].astype(np.float64), kt["y"][t].astype(np.float64))[0]
        assert len(rec) > 100 and inl.all(), (p, len(rec), int((~inl).sum()))
        gained += len(rec) - int(ver[1][p].item())
    print("%s: %d records verified in the first pass, %d more after the second" % (kind, int(ver[1].sum().item()), gained))
    assert gained > 0                                               # (the twins: decided on the restatement's inputs, not on the device)
    want = restated_select(host_triple(B, ep, 1), 1, RESELECT)
    gm, gc, gf, go = (t.cpu().numpy() for t in resel)
    assert np.array_equal(gc, want[1]) and np.array_equal(gf, want[2]) and np.array_equal(go, want[3])
    assert gm.view(B.DMATCH).reshape(-1)[:len(want[0])].tobytes() == want[0].tobytes()
    wl, gl = restated_link(sc.rows, SCENE_CAP, want[3], want[0]), tuple(t.cpu().numpy() for t in linked)
    wrote = wl[0] != SENT32
    for name, g, w_ in zip(("prev", "track", "age"), gl, wl):
        assert np.array_equal(g[wrote], w_[wrote]), name
    assert gl[3].tolist() == wl[3].tolist() and wl[3][2] > 300


@pytest.mark.parametrize("kind", ["general", "stereo"])
def test_the_pipeline(B, env, kind):
    """one stream, one synchronisation at the end; then once more with the verifier on the held stream S and everything behind it on
    S2: the epipolar-guided call waits for the models (PairCall::run orders the stream behind the context's previous call)"""
    import torch
    ctx = B.Context(0)
    fr = DepthFrames(B, {"general": 301, "stereo": 302}[kind], kind)
    spec = B.PairSpec(fr.sc.nframes - 1, 1, 1, 0, 1, None)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    out = queue_pipeline(B, ctx, fr, spec, s.cuda_stream)
    torch.cuda.synchronize()
    check_pipeline(B, fr, *out, kind)
    serial = [t.cpu().numpy().copy() for t in out[2]]
    # behind the hold: the first pass and its selection complete, the models pre-filled (0x5A: no pair is guided, every row empty)
    e, sc = env, fr.sc
    first = ctx.match_knn_pairs(fr.set, fr.set, spec, 2, rows_cap=SCENE_CAP, dim_bytes=DIM)
    sel = ctx.select_pair_matches(first, 2, B.MatchSelect(*SELECT))
    n = spec.npairs
    ver = (torch.empty((sel[0].shape[0], 4), dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
           torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
           torch.empty((n, 12), dtype=torch.int64, device="cuda"))
    ep = sentinel_outputs(n, SCENE_CAP, 1)
    ver[4].view(torch.uint8).fill_(0x5A)
    verify, guide = B.PairVerify(MAX_ERROR, 128, 12, 0, 2026), guide_of(B, PIPE_WINDOW, MAX_ERROR, 0)
    torch.cuda.synchronize()
    hev = hold(e)
    rc1 = ctx._L.brisk_hip_verify_pair_matches_epipolar_device(ctx._h, C.byref(fr.set), C.byref(fr.set), C.byref(sc.kp_set), C.byref(sc.kp_set),
                                                               C.byref(spec), SCENE_CAP, sel[3].data_ptr(), sel[0].data_ptr(), int(sel[0].shape[0]),
                                                               C.byref(verify), int(sel[0].shape[0]), ver[4].data_ptr(), ver[1].data_ptr(),
                                                               ver[2].data_ptr(), ver[3].data_ptr(), ver[0].data_ptr(), sptr(e.S))
    rc2 = ctx._L.brisk_hip_match_knn_pairs_epipolar_guided_device(ctx._h, C.byref(fr.set), C.byref(fr.set), C.byref(sc.kp_set), C.byref(sc.kp_set),
                                                                  C.byref(spec), C.c_void_p(ver[4].data_ptr()), C.byref(guide), DIM, 1, SCENE_CAP,
                                                                  ep[0].data_ptr(), ep[1].data_ptr(), ep[2].data_ptr(), sptr(e.S2))
    pending = not hev.query()
    finish(e)
    assert rc1 == 0 and rc2 == 0
    assert pending, "the hold of %.0f ms ended before both calls were queued: the run proved nothing" % e.hold_ms
    for name, t, w in zip(("matches", "counts", "pair_rows"), ep, serial):
        g = t.cpu().numpy()
        # (the serial run's tensors were not pre-filled: compare what the call writes)
        if name == "counts":
            for p in range(n):
                lim = min(sc.rows[p + 1], SCENE_CAP)
                assert np.array_equal(g[p, :lim], w[p, :lim]), (name, p)
                assert (g[p, lim:] == SENTINEL).all()
        elif name == "pair_rows":
            assert np.array_equal(g, w)
        else:
            cnt = serial[1]
            for p in range(n):
                lim = min(sc.rows[p + 1], SCENE_CAP)
                have = cnt[p, :lim] > 0
                assert have.sum() > 100 and np.array_equal(g[p, :lim][have], w[p, :lim][have]), (name, p)
                assert (g[p, :lim][~have] == SENTINEL).all() and (g[p, lim:] == SENTINEL).all()
    ctx.close()


# ---- 5: arguments -----------------------------------------------------------------------------------------------------------------

def test_arguments(B):
    import torch
    rng = np.random.default_rng(3)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, 48, 64, COUNTS_A, CAP, count_stride=1)
    Ak = SynthKp(B, rng, COUNTS_A, CAP)
    nA, cpq = len(COUNTS_A), 2
    out = sentinel_outputs(nA, CAP, cpq)
    d_models = upload_models(model_records(B, [MODELS[0]] * nA))
    torch.cuda.synchronize()
    m, cnt, rows = (t.data_ptr() for t in out)
    L, h = ctx._L, ctx._h
    guide = guide_of(B, WIDE_WINDOW, BAND, 1)
    ARG, UNSUPPORTED = 1, 7

    def ref(x):
        return None if x is None else C.byref(x)

    def knn(q=A.set, t=A.set, qk=Ak.set, tk=Ak.set, md=d_models.data_ptr(), g=guide, spec=(nA - 1, 1, 1, 0, 1, None), dim=48, k=2, cap=CAP, m=m,
            cnt=cnt, rows=rows):
        return L.brisk_hip_match_knn_pairs_epipolar_guided_device(h, ref(q), ref(t), ref(qk), ref(tk), C.byref(B.PairSpec(*spec)), md, ref(g), dim,
                                                                  k, cap, m, cnt, rows, None)

    def radius(q=A.set, t=A.set, qk=Ak.set, tk=Ak.set, md=d_models.data_ptr(), g=guide, spec=(nA - 1, 1, 1, 0, 1, None), dim=48, r=200.0, cpq=cpq,
               cap=CAP, m=m, cnt=cnt, rows=rows):
        return L.brisk_hip_match_radius_pairs_epipolar_guided_device(h, ref(q), ref(t), ref(qk), ref(tk), C.byref(B.PairSpec(*spec)), md, ref(g),
                                                                     dim, r, cpq, cap, m, cnt, rows, None)

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
        ctx.match_knn_pairs_epipolar_guided(A.set, A.set, B.PairSpec(2, 0, 1, 0, 1, None), 3, d_models, guide, rows_cap=CAP, query_kps=Ak.set,
                                            train_kps=Ak.set, dim_bytes=48, out=out)
    assert ei.value.code == ARG
    torch.cuda.synchronize()
    for t in out:                                                   # none of these calls launched anything
        assert (t.cpu().numpy() == SENTINEL).all()
    # a band that gives no row a line is no error: every row is empty (a device pointer instead of a tensor)
    ctx.match_knn_pairs_epipolar_guided(A.set, A.set, B.PairSpec(nA, 0, 1, 0, 1, None), cpq, d_models.data_ptr(), guide_of(B, WIDE_WINDOW, NAN, 1),
                                        rows_cap=CAP, query_kps=Ak.set, train_kps=Ak.set, dim_bytes=48, out=out)
    torch.cuda.synchronize()
    hm, hc, hr = (t.cpu().numpy() for t in out)
    assert list(hr) == COUNTS_A and (hm == SENTINEL).all()
    for p in range(nA):
        assert (hc[p, :COUNTS_A[p]] == 0).all() and (hc[p, COUNTS_A[p]:] == SENTINEL).all()
