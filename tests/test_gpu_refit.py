"""GPU tests of brisk_hip_refit_pair_models_device: each pair's homography fitted again to all its inliers.  The expectation is always
the NumPy restatement of the rule (test_abi_refit.restated_refit) on the host copies of the inputs - the input models are what the
verifier on the device wrote, downloaded -; every array - models, counts, flags, offsets, the kept records - is compared as bytes, and
outputs are pre-filled with the matcher tests' sentinel so that a write outside them shows.  The shapes sit at the seams of the
sums: the lane stride of 256 records, the LDS chunk of 1 024, the wave of 64."""
import ctypes as C

import numpy as np
import pytest

from gpu_prefill import settled
from test_abi_refit import IDENTITY, PAIR_REFIT, REJECTED, grid_rms, refit_of, restated_refit, seeded_scene
from test_abi_tracks import SENT32, restated_link
from test_abi_verify import PAIR_BAD, PAIR_NO_MODEL, ROWS_CUT, restated_verify
from test_gpu_match_export import expect as restated_select, host_triple
from test_gpu_match_gated import knn_rows, oracle_knn
from test_gpu_match_guided import SELECT, VERIFY, RESELECT, guide_mask, guide_of, model_records, near_h, upload_models
from test_gpu_match_pairs import SENTINEL, batch_frames, same_rows
from test_gpu_verify import CAP, Lists, Scene, chain_frames, raw_verify, same, sentinel_outputs
from test_oracle_golden import H_1TO2

pytestmark = pytest.mark.gpu

SEAMS = [4, 5, 255, 256, 257, 1023, 1024, 1025, 2049]
NARROW = (-2.0, 2.0, -2.0, 2.0, 1)                                  # the guided window a refitted model allows


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    assert int(SENT32) == SENTINEL
    return B


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0)
    yield c
    c.close()


def noisy(B, seed, rows, sigma=0.4, **kw):
    """test_gpu_verify's Scene with Gaussian noise on every keypoint: a four-point model is then exact for its sample only"""
    sc = Scene(B, seed, rows, **kw)
    rng = np.random.default_rng(seed + 5000)
    sc.kps["x"] = (sc.kps["x"] + rng.normal(0, sigma, sc.kps["x"].shape)).astype(np.float32)
    sc.kps["y"] = (sc.kps["y"] + rng.normal(0, sigma, sc.kps["y"].shape)).astype(np.float32)
    for f, r, field, v in kw.get("nan_rows", ()):
        sc.kps[field][f, r] = v
    sc.upload()
    return sc


def raw_refit(B, ctx, qs, ts, spec, lists, models_ptr, refit, out_cap, out=None, stream=None, in_cap=None, out_models_ptr=None):
    """the C entry point on pre-filled outputs (matches, counts, flags, offsets, models)"""
    out = out or sentinel_outputs(spec.npairs, out_cap)
    r = B.PairRefit(*refit)
    rc = ctx._L.brisk_hip_refit_pair_models_device(ctx._h, C.byref(qs.desc_set), C.byref(ts.desc_set), C.byref(qs.kp_set), C.byref(ts.kp_set),
                                                   C.byref(spec), CAP, lists.d_offsets.data_ptr(), lists.d_matches.data_ptr(),
                                                   lists.in_cap if in_cap is None else in_cap, models_ptr, C.byref(r), out_cap,
                                                   out[4].data_ptr() if out_models_ptr is None else out_models_ptr, out[1].data_ptr(),
                                                   out[2].data_ptr(), out[3].data_ptr(), out[0].data_ptr(), C.c_void_p(stream) if stream else None)
    return rc, out


def verified_models(B, ctx, qs, ts, spec, lists, verify):
    """the verifier on the device: (the models tensor [npairs + 1, 24] int32, its first npairs records on the host)"""
    import torch
    rc, out = raw_verify(B, ctx, qs, ts, spec, lists, verify, lists.in_cap)
    assert rc == 0
    torch.cuda.synchronize()
    return out[4], out[4].cpu().numpy()[:spec.npairs].reshape(-1).view(B.PAIR_MODEL).copy()


def expect(qs, ts, frames, lists, in_models, refit, out_cap, in_cap=None):
    return restated_refit(frames, qs.rows, ts.rows, CAP, qs.xy, ts.xy, lists.offsets, lists.matches, in_models, refit,
                          lists.in_cap if in_cap is None else in_cap, out_cap)


@pytest.fixture(scope="module")
def seam_scene(B, ctx):
    sc = noisy(B, 211, [300] * (len(SEAMS) + 1))                     # 300 rows a frame, 256 exist
    per = [sc.records(p + 1, p, m) for p, m in enumerate(SEAMS)]
    for rec in per[:2]:                                              # 4 and 5 records: distinct rows, all of them true pairs
        rec["queryIdx"] = rec["trainIdx"] = np.arange(len(rec)) * 37 + 11
    lists = Lists(B, per)
    spec = B.PairSpec(len(SEAMS), 1, 1, 0, 1, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, (2.0, 64, 4, 0, 5))
    return sc, lists, spec, d_models, models


@pytest.mark.parametrize("rounds", [1, 2, 8])
def test_record_counts_at_the_seams_of_the_sums(B, ctx, seam_scene, rounds):
    sc, lists, spec, d_models, models = seam_scene
    n = len(SEAMS)
    refit = (2.0, rounds, 4, 0)
    out_cap = int(lists.offsets[-1])
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
    assert rc == 0
    want = expect(sc, sc, chain_frames(n), lists, models, refit, out_cap)
    same(B, out, want, n, out_cap)
    got = want[0]
    assert got["records"].tolist() == SEAMS and (models["flags"] == 0).all()
    assert (got["flags"] == PAIR_REFIT).all() and (got["inliers"] >= models["inliers"]).all()
    assert (got["inliers"][2:] > models["inliers"][2:]).any()        # a kept list grows
    assert (got["valid"] >= 1).all() and (got["valid"] <= rounds).all() and (got["hypothesis"] == models["hypothesis"]).all()


def pair_scene(B, pairs):
    """hand-made pairs [(kq [rows, 2], kt [rows, 2], rec)]: pair p has the frames 2 p + 1 (query) and 2 p (train)"""
    rows = []
    for kq, kt, _ in pairs:
        rows += [len(kt), len(kq)]
    sc = Scene(B, 1, rows)
    sc.kps["x"], sc.kps["y"] = 0, 0
    for p, (kq, kt, _) in enumerate(pairs):
        sc.kps["x"][2 * p + 1, :len(kq)], sc.kps["y"][2 * p + 1, :len(kq)] = kq[:, 0], kq[:, 1]
        sc.kps["x"][2 * p, :len(kt)], sc.kps["y"][2 * p, :len(kt)] = kt[:, 0], kt[:, 1]
    sc.upload()
    return sc, Lists(B, [rec for _, _, rec in pairs]), B.PairSpec(len(pairs), 1, 2, 0, 2, None), [(2 * p + 1, 2 * p) for p in range(len(pairs))]


@pytest.mark.parametrize("keep", [0, 1])
def test_models_that_stand_are_replaced_fail_or_lost_their_sign(B, ctx, keep):
    from test_abi_verify import records
    a, b, rej = seeded_scene(2), seeded_scene(3), seeded_scene(**REJECTED)
    line = np.stack([np.arange(9, dtype=np.float32) * 16 + 3, np.full(9, 40, np.float32)], axis=1)
    point = np.tile(np.float32([[33, 44]]), (9, 1))
    ident = lambda k: records([(j, j) for j in range(k)])
    pairs = [(a["kq"], a["kt"], a["rec"]), (a["kq"], a["kt"], a["rec"]), (b["kq"], b["kt"], b["rec"]), (rej["kq"], rej["kt"], rej["rec"]),
             (line, line, ident(9)), (point, point, ident(9)), (a["kq"], a["kt"], a["rec"]), (a["kq"], a["kt"], a["rec"]),
             (a["kq"], a["kt"], a["rec"]), (b["kq"], b["kt"], b["rec"])]
    nan = a["h_in"].copy()
    nan[4] = np.nan
    models = model_records(B, [(a["h_in"], 5, 0), (-a["h_in"], 5, 0), (b["h_in"], 0, ROWS_CUT | 1), (rej["h_in"], 3, 0), (IDENTITY, 1, 0),
                               (IDENTITY, 2, 0), (nan, 1, 0), (a["h_in"], -1, 0), (a["h_in"], 4, PAIR_NO_MODEL), (b["h_in"], 6, PAIR_BAD)])
    sc, lists, spec, frames = pair_scene(B, pairs)
    d_models = upload_models(models)
    out_cap = int(lists.offsets[-1])
    refit = (3.0, 2, 8, keep)
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
    assert rc == 0
    want = expect(sc, sc, frames, lists, models, refit, out_cap)
    same(B, out, want, len(pairs), out_cap)
    got = want[0]
    assert got["h"][0].tobytes() == got["h"][1].tobytes() and want[1][0] == want[1][1]          # -H in: the same bytes out as for H
    assert got["flags"][:3].tolist() == [PAIR_REFIT] * 3 and got["valid"][:3].tolist() == [2, 2, 2]
    assert got["inliers"][0] > refit_of(seeded_scene(2), rounds=1)["n0"]                        # the kept list grew
    for p in (4, 5):                                                # the fit fails: the input model stands, byte for byte
        assert got["flags"][p] == 0 and got["valid"][p] == 0 and got["h"][p].tobytes() == models["h"][p].tobytes(), p
        assert want[1][p] == got["inliers"][p] == 9
    for p in (6, 7, 8, 9):                                          # records that are no model
        assert got["flags"][p] == PAIR_NO_MODEL and (got["h"][p] == 0).all() and got["hypothesis"][p] == -1
        assert want[1][p] == (got["usable"][p] if keep else 0)
    # the scene whose fit loses an inlier and is rejected, at its own threshold
    refit = (REJECTED["max_error"], 3, 4, keep)
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
    assert rc == 0
    want = expect(sc, sc, frames, lists, models, refit, out_cap)
    same(B, out, want, len(pairs), out_cap)
    got = want[0]
    assert got["flags"][3] == 0 and got["valid"][3] == 0 and got["h"][3].tobytes() == models["h"][3].tobytes() and want[1][3] == got["inliers"][3] >= 4


@pytest.mark.parametrize("keep", [0, 1])
def test_unusable_records(B, ctx, keep):
    nan_rows = [(1, 3, "x", np.nan), (1, 9, "y", np.inf), (0, 5, "y", np.nan), (2, 0, "x", -np.inf), (2, 17, "x", np.nan)]
    sc = noisy(B, 251, [300, 120, 256, 40, 257], nan_rows=nan_rows)  # frame 0 and 4 beyond rows_cap, frame 3 short
    per = [sc.records(1, 0, 200, odd=0.15), sc.records(2, 1, 300, odd=0.15), sc.records(3, 2, 90, inliers=0.0, odd=0.15),
           sc.records(4, 3, 70, odd=0.3)]
    for rec in per[:2]:                                             # records that name the rows with NaN coordinates
        rec["queryIdx"][:4], rec["trainIdx"][:4] = [3, 3, 9, 9], [3, 5, 9, 5]
    lists = Lists(B, per)
    spec = B.PairSpec(4, 1, 1, 0, 1, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, (2.0, 256, 10, keep, 123))
    refit = (2.0, 2, 10, keep)
    out_cap = int(lists.offsets[-1])
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
    assert rc == 0
    want = expect(sc, sc, chain_frames(4), lists, models, refit, out_cap)
    same(B, out, want, 4, out_cap)
    got = want[0]
    assert (got["usable"] < got["records"]).all() and (got["usable"] > 0).all() and (got["usable"] == models["usable"]).all()
    assert got["flags"][0] == PAIR_REFIT and got["flags"][1] == PAIR_REFIT and got["flags"][2] == PAIR_NO_MODEL     # pure outliers: no model
    assert want[1][2] == (got["usable"][2] if keep else 0)


def test_pair_forms(B, ctx):
    import torch
    sc = noisy(B, 261, [90, 100, 110, 120, 130, 140])
    verify, refit = (2.0, 64, 6, 0, 8), (2.0, 2, 6, 0)
    # a list on the device with entries outside the sets between good pairs
    frames = [(1, 0), (6, 0), (3, 5), (2, -1), (4, 4), (-2147483648, 2), (0, 6), (5, 1)]
    per = [sc.records(max(min(a, 5), 0), max(min(b, 5), 0), 50) for a, b in frames]
    lists = Lists(B, per)
    d_pairs = torch.from_numpy(np.array(frames, np.int32)).cuda()
    spec = B.PairSpec(len(frames), 9, 9, 9, 9, d_pairs.data_ptr())
    out_cap = int(lists.offsets[-1])
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, verify)
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
    assert rc == 0
    want = expect(sc, sc, frames, lists, models, refit, out_cap)
    same(B, out, want, len(frames), out_cap)
    bad = PAIR_BAD | PAIR_NO_MODEL
    assert [int(f) for f in want[2]] == [PAIR_REFIT, bad, PAIR_REFIT, bad, PAIR_REFIT, bad, bad, PAIR_REFIT]
    # a bad entry's input record is not read: a record that carries a model changes nothing
    forged = models.copy()
    forged[1] = models[0]
    d_forged = upload_models(forged)
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_forged.data_ptr(), refit, out_cap)
    assert rc == 0
    same(B, out, want, len(frames), out_cap)
    # everything against one frame: the keyframe form, a model per pair
    frames = [(p + 1, 0) for p in range(5)]
    lists = Lists(B, [sc.records(a, b, 45) for a, b in frames])
    spec = B.PairSpec(5, 1, 1, 0, 0, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, verify)
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, 225)
    assert rc == 0
    want = expect(sc, sc, frames, lists, models, refit, 225)
    same(B, out, want, 5, 225)
    assert (want[0]["flags"] == PAIR_REFIT).all() and len({m["h"].tobytes() for m in want[0]}) == 5
    # interleaved stereo: left frames 0, 2, 4 against right frames 1, 3, 5
    frames = [(0, 1), (2, 3), (4, 5)]
    lists = Lists(B, [sc.records(a, b, 45) for a, b in frames])
    spec = B.PairSpec(3, 0, 2, 1, 2, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, verify)
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, 135)
    assert rc == 0
    same(B, out, expect(sc, sc, frames, lists, models, refit, 135), 3, 135)


def test_capacity(B, ctx):
    """out_cap equal to the total, one short (the cut falls in the last pair that keeps anything, an empty pair in front of it and
    one behind), and 0"""
    sc = noisy(B, 271, [100] * 7)
    per = [sc.records(1, 0, 60), sc.records(2, 1, 0), sc.records(3, 2, 70), sc.records(4, 3, 30, inliers=0.0), sc.records(5, 4, 80),
           sc.records(6, 5, 0)]
    lists = Lists(B, per)
    spec = B.PairSpec(6, 1, 1, 0, 1, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, (2.0, 128, 10, 0, 4))
    refit = (2.0, 1, 10, 0)
    free = expect(sc, sc, chain_frames(6), lists, models, refit, 10 ** 6)
    total = int(free[3][-1])
    assert free[1][3] == 0 and free[1][4] > 20 and free[1][5] == 0 and total == free[1].sum()
    for out_cap in (total, total - 1, 0):
        rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
        assert rc == 0
        want = expect(sc, sc, chain_frames(6), lists, models, refit, out_cap)
        same(B, out, want, 6, out_cap)
        cut = [bool(f & ROWS_CUT) for f in want[2]]
        assert cut == {total: [False] * 6, total - 1: [False] * 4 + [True] * 2, 0: [True] * 6}[out_cap]
        assert want[1].tolist() == free[1].tolist()                  # the true counts are still reported


def test_more_pairs_than_the_offsets_workgroup_has_threads(B, ctx):
    """1 025 pairs of 0 ... 13 records, with a cut"""
    import torch
    rng = np.random.default_rng(281)
    sc = noisy(B, 281, [60] * 12)
    n = 1025
    frames = [(int(a), int(b)) for a, b in rng.integers(0, 12, (n, 2))]
    lists = Lists(B, [sc.records(a, b, int(rng.integers(0, 14)), inliers=0.9) for a, b in frames])
    d_pairs = torch.from_numpy(np.array(frames, np.int32)).cuda()
    spec = B.PairSpec(n, 0, 0, 0, 0, d_pairs.data_ptr())
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, (2.0, 16, 4, 1, 2))
    refit = (2.0, 1, 4, 1)
    free = expect(sc, sc, frames, lists, models, refit, 10 ** 7)
    total = int(free[3][-1])
    assert total > 3000 and (free[0]["flags"] & PAIR_REFIT).sum() > 300
    for out_cap in (total, total * 2 // 3):
        rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
        assert rc == 0
        want = free if out_cap == total else expect(sc, sc, frames, lists, models, refit, out_cap)
        same(B, out, want, n, out_cap)
    assert 300 < int(np.flatnonzero(want[2] & ROWS_CUT)[0]) < 1000


def test_in_place_and_a_second_call_on_the_stream(B, ctx, seam_scene):
    """d_out_models == d_models; then two more calls back to back on one stream, the second smaller than the first (it runs in the
    scratch the first one grew), no synchronisation in between"""
    import torch
    sc, big, spec, d_models, models = seam_scene
    n = len(SEAMS)
    r1, r2 = (2.0, 2, 4, 0), (2.0, 1, 5, 1)
    cap1, cap2 = int(big.offsets[-1]), 77
    want1 = expect(sc, sc, chain_frames(n), big, models, r1, cap1)
    inplace = settled(d_models.clone())                                 # [npairs + 1, 24] int32: a sentinel record behind the pairs'
    out = sentinel_outputs(n, cap1)
    rc, _ = raw_refit(B, ctx, sc, sc, spec, big, inplace.data_ptr(), r1, cap1, out=out, out_models_ptr=inplace.data_ptr())
    assert rc == 0
    same(B, (out[0], out[1], out[2], out[3], inplace), want1, n, cap1)
    assert (out[4].cpu().numpy() == SENTINEL).all()
    small_sc = noisy(B, 291, [50, 60, 70])
    small = Lists(B, [small_sc.records(1, 0, 33), small_sc.records(2, 1, 44)])
    spec2 = B.PairSpec(2, 1, 1, 0, 1, None)
    d_models2, models2 = verified_models(B, ctx, small_sc, small_sc, spec2, small, (2.0, 32, 5, 1, 6))
    s = torch.cuda.Stream()
    rc1, out1 = raw_refit(B, ctx, sc, sc, spec, big, d_models.data_ptr(), r1, cap1, stream=s.cuda_stream)
    rc2, out2 = raw_refit(B, ctx, small_sc, small_sc, spec2, small, d_models2.data_ptr(), r2, cap2, stream=s.cuda_stream)
    rc3, out3 = raw_refit(B, ctx, sc, sc, spec, big, d_models.data_ptr(), r1, cap1, stream=s.cuda_stream)
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    same(B, out1, want1, n, cap1)
    same(B, out2, expect(small_sc, small_sc, chain_frames(2), small, models2, r2, cap2), 2, cap2)
    same(B, out3, want1, n, cap1)


def restated_refit_chain(B, desc, kps, rows_cap, first, refit):
    """everything behind the first k-NN call, restated: select, verify, refit, the guided k-NN (k = 1, +-2 px) under the refitted
    models, select, link"""
    n = len(desc)
    node_rows = [len(k) for k in kps]
    xy = [np.stack([k["x"], k["y"]], axis=1).astype(np.float32).reshape(-1, 2) for k in kps]
    sel = restated_select(first, 2, SELECT)
    in_cap = (n - 1) * rows_cap * 2
    ver = restated_verify(chain_frames(n - 1), node_rows, node_rows, rows_cap, xy, xy, sel[3], sel[0], VERIFY, in_cap, in_cap)
    ref = restated_refit(chain_frames(n - 1), node_rows, node_rows, rows_cap, xy, xy, sel[3], sel[0], ver[0], refit, in_cap, in_cap)
    models = ref[0]
    rows = [oracle_knn(desc[p + 1], desc[p], guide_mask(NARROW, 0, models[p], kps[p + 1], kps[p])[0], p, 1)[:rows_cap] for p in range(n - 1)]
    m = np.zeros((n - 1, rows_cap, 1), B.DMATCH)
    cnt = np.zeros((n - 1, rows_cap), np.int32)
    for p, rr in enumerate(rows):
        for q, r in enumerate(rr):
            m[p, q, :len(r)], cnt[p, q] = r, len(r)
    resel = restated_select((m, cnt, np.array(node_rows[1:], np.int32)), 1, RESELECT)
    link = restated_link(node_rows, rows_cap, resel[3], resel[0])
    return {"select": sel, "verify": ver, "refit": ref, "guided": rows, "reselect": resel, "link": link}


def same_lists(B, got, exp, name):
    gm, gc, gf, go = (t.cpu().numpy() for t in got[:4])
    assert np.array_equal(gc, exp[1]) and np.array_equal(gf, exp[2]) and np.array_equal(go, exp[3]), name
    assert gm.view(B.DMATCH).reshape(-1)[:len(exp[4])].tobytes() == exp[4].tobytes(), name


def test_the_pipeline(B, golden_ast):
    """detect + describe, k-NN (k = 2), select, verify, refit (2 rounds, the models in place of the verifier's), guided k-NN (k = 1,
    +-2 px) reading the refitted models, select, link - one stream, one synchronisation at the end; every array against the restated
    chain.  Pair 0 is (img1, img2) with the known H_1TO2: the refit's inliers are at least the verifier's (the rule guarantees it);
    the models' distances to H_1TO2 over the 9 x 7 grid are printed (a recorded result: profiles/refit_pairs.json), not asserted."""
    import torch
    frames = batch_frames(golden_ast)
    n, h, w = frames.shape
    d = torch.from_numpy(frames).cuda()
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    refit = (VERIFY[0], 2, VERIFY[2], 0)
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    first = ctx.match_knn_pairs(st, st, spec, 2, stream=s.cuda_stream)
    rows_cap = int(first[1].shape[1])
    sel = ctx.select_pair_matches(first, 2, B.MatchSelect(*SELECT), stream=s.cuda_stream)
    ver = ctx.verify_pair_matches(st, st, spec, rows_cap, sel[3], sel[0], B.PairVerify(*VERIFY), stream=s.cuda_stream)
    ref = ctx.refit_pair_models(st, st, spec, rows_cap, sel[3], sel[0], ver[4], B.PairRefit(*refit), stream=s.cuda_stream)
    guided = ctx.match_knn_pairs_guided(st, st, spec, 1, ref[4], guide_of(B, NARROW, 0), rows_cap=rows_cap, stream=s.cuda_stream)
    resel = ctx.select_pair_matches(guided, 1, B.MatchSelect(*RESELECT), stream=s.cuda_stream)
    linked = ctx.link_tracks((st, 0, 1), n, rows_cap, resel[3], resel[0], stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    kd = [ctx.batch_download(f, True, strings=dim) for f in range(n)]
    kps, desc = [k for k, _ in kd], [dd for _, dd in kd]
    want = restated_refit_chain(B, desc, kps, rows_cap, host_triple(B, first, 2), refit)
    for name, got in (("verify", ver), ("refit", ref)):
        exp = want[name]
        assert got[4].cpu().numpy().tobytes() == exp[0].tobytes(), name
        same_lists(B, got, exp, name)
    for name, got in (("select", sel), ("reselect", resel)):
        exp = want[name]
        same_lists(B, got, (None, exp[1], exp[2], exp[3], exp[0]), name)
    vm, rm = want["verify"][0], want["refit"][0]
    assert vm["flags"][0] == 0 and (rm["flags"][0] & PAIR_NO_MODEL) == 0 and rm["inliers"][0] >= vm["inliers"][0] > 50
    assert rm["flags"][2] == PAIR_NO_MODEL and rm["hypothesis"][2] == -1                # the blank frame: no input model
    got_rows, _ = knn_rows(B, tuple(t.cpu().numpy() for t in guided), 1)
    for p in range(n - 1):
        same_rows(got_rows[p], want["guided"][p])
    wl, gl = want["link"], tuple(t.cpu().numpy() for t in linked)
    wrote = wl[0] != SENT32
    for name, g, w_ in zip(("prev", "track", "age"), gl, wl):
        assert np.array_equal(g[wrote], w_[wrote]), name
    assert gl[3].tolist() == wl[3].tolist()
    g0 = want["reselect"][0][:int(want["reselect"][3][1])]
    print("pair 0 (img1 -> img2): inliers %d -> %d in %d round(s); RMS distance to H_1TO2 over the 9 x 7 grid %.3f px -> %.3f px; "
          "%d guided records inside +-2 px, %d within 5 px of H_1TO2; links made over the batch: %d" %
          (vm["inliers"][0], rm["inliers"][0], rm["valid"][0], grid_rms(vm["h"][0], H_1TO2), grid_rms(rm["h"][0], H_1TO2), len(g0),
           near_h(kps[1], kps[0], g0), int(wl[3][2])))
    ext.close()
    ctx.close()


def test_arguments(B, ctx):
    """BRISK_HIP_ERR_ARG before anything is launched: the sentinel stays in every output"""
    import torch
    sc = noisy(B, 301, [50, 60, 70])
    lists = Lists(B, [sc.records(1, 0, 30), sc.records(2, 1, 30)])
    spec = B.PairSpec(2, 1, 1, 0, 1, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, (2.0, 64, 6, 0, 1))
    out = sentinel_outputs(2, 60)
    L, h = ctx._L, ctx._h

    def call(**kw):
        a = dict(ctx=h, query=sc.desc_set, train=sc.desc_set, query_kps=sc.kp_set, train_kps=sc.kp_set, pairs=B.PairSpec(2, 1, 1, 0, 1, None),
                 rows_cap=CAP, offsets=lists.d_offsets.data_ptr(), matches=lists.d_matches.data_ptr(), in_cap=lists.in_cap,
                 in_models=d_models.data_ptr(), refit=B.PairRefit(2.0, 2, 6, 0), out_cap=60, models=out[4].data_ptr(), counts=out[1].data_ptr(),
                 flags=out[2].data_ptr(), out_offsets=out[3].data_ptr(), out_matches=out[0].data_ptr())
        a.update(kw)
        ref = lambda v: None if v is None else C.byref(v)
        return L.brisk_hip_refit_pair_models_device(a["ctx"], ref(a["query"]), ref(a["train"]), ref(a["query_kps"]), ref(a["train_kps"]),
                                                    ref(a["pairs"]), a["rows_cap"], a["offsets"], a["matches"], a["in_cap"], a["in_models"],
                                                    ref(a["refit"]), a["out_cap"], a["models"], a["counts"], a["flags"], a["out_offsets"],
                                                    a["out_matches"], None)

    def desc(**kw):
        f = dict(d_desc=None, d_counts=sc.d_counts.data_ptr(), count_stride=sc.stride, frame_pitch=0, row_pitch=0, frames=3)
        f.update(kw)
        return B.DescSet(f["d_desc"], f["d_counts"], f["count_stride"], f["frame_pitch"], f["row_pitch"], f["frames"])

    kp = sc.d_kps.data_ptr()
    bad = [dict(ctx=None), dict(query=None), dict(train=None), dict(query_kps=None), dict(train_kps=None), dict(pairs=None), dict(refit=None),
           dict(rows_cap=0), dict(in_cap=-1), dict(out_cap=-1), dict(pairs=B.PairSpec(-1, 1, 1, 0, 1, None)),
           dict(offsets=None), dict(matches=None), dict(models=None), dict(counts=None), dict(flags=None), dict(out_offsets=None),
           dict(out_matches=None), dict(in_models=None), dict(in_models=d_models.data_ptr() + 4),
           dict(offsets=lists.d_offsets.data_ptr() + 4), dict(matches=lists.d_matches.data_ptr() + 8), dict(models=out[4].data_ptr() + 4),
           dict(counts=out[1].data_ptr() + 2), dict(flags=out[2].data_ptr() + 1), dict(out_offsets=out[3].data_ptr() + 4),
           dict(out_matches=out[0].data_ptr() + 8),
           dict(refit=B.PairRefit(2.0, 0, 6, 0)), dict(refit=B.PairRefit(2.0, 9, 6, 0)), dict(refit=B.PairRefit(2.0, -1, 6, 0)),
           dict(refit=B.PairRefit(2.0, 2, 3, 0)), dict(refit=B.PairRefit(2.0, 2, -1, 0)),
           dict(pairs=B.PairSpec(2, 2, 1, 0, 1, None)), dict(pairs=B.PairSpec(2, 1, 1, -1, 1, None)), dict(pairs=B.PairSpec(2, 1, 1, 2, 1, None)),
           dict(pairs=B.PairSpec(2, 0, -1, 0, 1, None)), dict(pairs=B.PairSpec(2, 1, 1, 0, 1, lists.d_offsets.data_ptr() + 2)),
           dict(query=desc(d_counts=None)), dict(train=desc(frames=0)), dict(query=desc(count_stride=0)),
           dict(train=desc(d_counts=sc.d_counts.data_ptr() + 2)),
           dict(query_kps=B.KpSet(None, 28)), dict(train_kps=B.KpSet(kp + 2, 28)), dict(query_kps=B.KpSet(kp, -28)),
           dict(train_kps=B.KpSet(kp, 30))]
    for kw in bad:
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.int32) == SENTINEL).all() for t in out)        # nothing was launched
    # npairs == 0: OK, d_out_offsets[0] = 0 and nothing else; NULL arrays are then allowed
    assert call(pairs=B.PairSpec(0, 1, 1, 0, 1, None), out_offsets=None, models=None, counts=None, flags=None, offsets=None, in_models=None) == 0
    assert call(pairs=B.PairSpec(0, 7, 7, 7, 7, None)) == 0
    torch.cuda.synchronize()
    o = out[3].cpu().numpy()
    assert o[0] == 0 and (o[1:] == np.int64(0x5A5A5A5A5A5A5A5A)).all()
    assert all((t.cpu().numpy().view(np.int32) == SENTINEL).all() for t in (out[0], out[1], out[2], out[4]))
    # offsets that are no range inside [0, in_cap]: the pair is flagged bad on the device, nothing of it is read
    refit = (2.0, 2, 6, 0)
    rc, got = raw_refit(B, ctx, sc, sc, B.PairSpec(2, 1, 1, 0, 1, None), lists, d_models.data_ptr(), refit, 60, in_cap=45)
    assert rc == 0
    want = expect(sc, sc, chain_frames(2), lists, models, refit, 60, in_cap=45)
    same(B, got, want, 2, 60)
    assert want[2].tolist() == [PAIR_REFIT, PAIR_BAD | PAIR_NO_MODEL] and want[1][0] > 6 and want[1][1] == 0
    assert call() == 0
    same(B, out, expect(sc, sc, chain_frames(2), lists, models, refit, 60), 2, 60)
