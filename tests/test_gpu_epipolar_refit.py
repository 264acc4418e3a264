"""GPU tests of brisk_hip_refit_pair_models_epipolar_device: each pair's fundamental matrix fitted again to all its inliers, rank 2
enforced.  The expectation is always the NumPy restatement of the rule (test_abi_epipolar_refit.restated_epipolar_refit) on the host
copies of the inputs - the input models are what the epipolar verifier on the device wrote, downloaded -; every array - models,
counts, flags, offsets, the kept records - is compared as bytes, and outputs are pre-filled with the matcher tests' sentinel so that
a write outside them shows.  The shapes sit at the seams of the sums: the sample of 8, the lane stride of 256 records, the LDS chunk
of 1 024."""
import ctypes as C

import numpy as np
import pytest

from gpu_prefill import settled
from test_abi_epipolar import planted_depth
from test_abi_epipolar_refit import SEAMS, degenerate_scenes, hand_views, restated_epipolar_refit, winner_of
from test_abi_refit import PAIR_REFIT
from test_abi_verify import PAIR_BAD, PAIR_NO_MODEL, ROWS_CUT, records
from test_gpu_epipolar import depth_scene, raw_epipolar
from test_gpu_match_epiline import epi_mask, guide_of
from test_gpu_match_gated import knn_rows, oracle_knn
from test_gpu_match_pairs import SENTINEL, batch_frames, same_rows
from test_gpu_refit import pair_scene
from test_gpu_verify import CAP, Lists, chain_frames, same, sentinel_outputs

pytestmark = pytest.mark.gpu

VERIFY = (1.5, 256, 8, 0, 5)                                        # max_error, hypotheses, min_inliers, keep_unverified, seed


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0)
    yield c
    c.close()


def noisy_depth(B, seed, rows, sigma=0.25, nan_rows=(), **kw):
    """test_gpu_epipolar.depth_scene with Gaussian noise on every keypoint: an eight-point model is then exact for its sample only"""
    sc = depth_scene(B, seed, rows, **kw)
    rng = np.random.default_rng(seed + 7000)
    sc.kps["x"] = (sc.kps["x"] + rng.normal(0, sigma, sc.kps["x"].shape)).astype(np.float32)
    sc.kps["y"] = (sc.kps["y"] + rng.normal(0, sigma, sc.kps["y"].shape)).astype(np.float32)
    for f, r, field, v in nan_rows:
        sc.kps[field][f, r] = v
    sc.upload()
    return sc


def filled_outputs(npairs, out_cap):
    """test_gpu_verify.sentinel_outputs, the sentinel in place on return"""
    import torch
    out = sentinel_outputs(npairs, out_cap)
    torch.cuda.synchronize()
    return out


def raw_refit(B, ctx, qs, ts, spec, lists, models_ptr, refit, out_cap, out=None, stream=None, in_cap=None, out_models_ptr=None):
    """the C entry point on pre-filled outputs (matches, counts, flags, offsets, models).  Outputs made here are complete before the
    call: the fills run on torch's stream, the call on the context's own, which does not wait for it"""
    out = out or filled_outputs(spec.npairs, out_cap)
    r = B.PairEpipolarRefit(*refit)
    rc = ctx._L.brisk_hip_refit_pair_models_epipolar_device(ctx._h, C.byref(qs.desc_set), C.byref(ts.desc_set), C.byref(qs.kp_set),
                                                            C.byref(ts.kp_set), C.byref(spec), CAP, lists.d_offsets.data_ptr(),
                                                            lists.d_matches.data_ptr(), lists.in_cap if in_cap is None else in_cap, models_ptr,
                                                            C.byref(r), out_cap, out[4].data_ptr() if out_models_ptr is None else out_models_ptr,
                                                            out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[0].data_ptr(),
                                                            C.c_void_p(stream) if stream else None)
    return rc, out


def verified_models(B, ctx, qs, ts, spec, lists, verify):
    """the epipolar verifier on the device: (the models tensor [npairs + 1, 24] int32, its first npairs records on the host)"""
    import torch
    rc, out = raw_epipolar(B, ctx, qs, ts, spec, lists, verify, lists.in_cap, out=filled_outputs(spec.npairs, lists.in_cap))
    assert rc == 0
    torch.cuda.synchronize()
    return out[4], out[4].cpu().numpy()[:spec.npairs].reshape(-1).view(B.PAIR_EPIPOLAR_MODEL).copy()


def upload_models(rec):
    """PAIR_EPIPOLAR_MODEL records and a sentinel record behind them -> the device"""
    import torch
    full = np.full((len(rec) + 1, 24), SENTINEL, np.int32)
    full[:len(rec)] = rec.view(np.int32).reshape(len(rec), 24)
    return torch.from_numpy(full).cuda()


def expect(qs, ts, frames, lists, in_models, refit, out_cap, in_cap=None):
    return restated_epipolar_refit(frames, qs.rows, ts.rows, CAP, qs.xy, ts.xy, lists.offsets, lists.matches, in_models, refit,
                                   lists.in_cap if in_cap is None else in_cap, out_cap)


@pytest.fixture(scope="module")
def seam_scene(B, ctx):
    sc = noisy_depth(B, 312, [300] * (len(SEAMS) + 1))              # 300 rows a frame, 256 exist; the seed: every pair is refitted
    per = [sc.records(p + 1, p, m) for p, m in enumerate(SEAMS)]
    for rec in per[:2]:                                              # 8 and 9 records: distinct rows, all of them true pairs
        rec["queryIdx"] = rec["trainIdx"] = np.arange(len(rec)) * 23 + 11
    lists = Lists(B, per)
    spec = B.PairSpec(len(SEAMS), 1, 1, 0, 1, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, VERIFY)
    return sc, lists, spec, d_models, models


@pytest.mark.parametrize("rank2", [0, 1])
@pytest.mark.parametrize("rounds", [1, 2, 8])
def test_record_counts_at_the_seams_of_the_sums(B, ctx, seam_scene, rounds, rank2):
    sc, lists, spec, d_models, models = seam_scene
    n = len(SEAMS)
    refit = (1.5, rounds, 8, 0, rank2)
    out_cap = int(lists.offsets[-1])
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
    assert rc == 0
    want = expect(sc, sc, chain_frames(n), lists, models, refit, out_cap)
    same(B, out, want, n, out_cap)
    got = want[0]
    assert got["records"].tolist() == list(SEAMS) and (models["flags"] == 0).all()
    assert (got["flags"] == PAIR_REFIT).all() and (got["inliers"] >= models["inliers"]).all()
    assert (got["inliers"][2:] > models["inliers"][2:]).any()        # a kept list grows
    assert (want[1] == got["inliers"]).all()
    assert (got["valid"] >= 1).all() and (got["valid"] <= rounds).all() and (got["hypothesis"] == models["hypothesis"]).all()


STANDS = dict(seed=4000, kind="plane", true=16, random=10, noise=1.0)       # found by a search on the CPU: the fitted model loses an inlier
HAND_VERIFY = (1.5, 64, 8, 0, 77)


def hand_pairs():
    """pair 0: a model that stands (its refit counts fewer inliers); 1: a model that is replaced; 2: twelve exact records (they lose
    acceptance at min_inliers 13); 3, 4: inliers of pair 2's model on an axis-parallel line, on the query and on the train side (the
    fit fails); 5: unusable records - indices beyond the rows that exist, NaN keypoints"""
    kq0, kt0, rec0, _ = planted_depth(np.random.default_rng(STANDS["seed"]), STANDS["kind"], STANDS["true"], STANDS["random"], noise=STANDS["noise"])
    kq1, kt1, rec1, _ = planted_depth(np.random.default_rng(4101), "general", 48, 12)
    sq, st, _ = hand_views()
    ident = records([(j, j) for j in range(12)])
    hand = winner_of(HAND_VERIFY[4], 2, HAND_VERIFY[1], HAND_VERIFY[0], sq, st, ident)
    assert hand[2] == 0 and hand[3] == 12
    axis = [(kq, kt, ident.copy()) for name, kq, kt in degenerate_scenes(hand[0]) if name == "axis"]
    assert len(axis) == 2
    kq5, kt5, rec5, _ = planted_depth(np.random.default_rng(4105), "stereo", 40, 10)
    rec5["queryIdx"][[3, 17]], rec5["trainIdx"][[8, 30]] = [50, -1], [50, 2 ** 31 - 1]
    kq5[rec5["queryIdx"][5], 0], kt5[rec5["trainIdx"][11], 1] = np.nan, np.inf
    return [(kq0, kt0, rec0), (kq1, kt1, rec1), (sq, st, ident), axis[0], axis[1], (kq5, kt5, rec5)], hand


@pytest.mark.parametrize("keep", [0, 1])
def test_models_that_stand_are_replaced_fail_or_lose_acceptance(B, ctx, keep):
    pairs, hand = hand_pairs()
    sc, lists, spec, frames = pair_scene(B, pairs)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, HAND_VERIFY[:3] + (keep,) + HAND_VERIFY[4:])
    assert models["f"][2].tobytes() == hand[0].tobytes() and models["flags"][2] == 0      # the device's model is the restated one
    assert (models["flags"][[3, 4]] == PAIR_NO_MODEL).all()          # the verifier finds nothing on an axis-parallel line ...
    models[3] = models[2]                                            # ... the records are inliers of pair 2's model: the refit's input
    models[4] = models[2]
    d_models = upload_models(models)
    out_cap = int(lists.offsets[-1])
    for min_inl in (8, 13):
        for rank2 in (0, 1):
            refit = (1.5, 2, min_inl, keep, rank2)
            rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
            assert rc == 0
            want = expect(sc, sc, frames, lists, models, refit, out_cap)
            same(B, out, want, len(pairs), out_cap)
            got = want[0]
            # the model that stands: the input's bytes, no REFIT flag
            assert got["flags"][0] == 0 and got["valid"][0] == 0 and got["f"][0].tobytes() == models["f"][0].tobytes()
            assert want[1][0] == got["inliers"][0] == models["inliers"][0]
            assert got["flags"][1] == PAIR_REFIT and got["valid"][1] == 2 and got["inliers"][1] >= models["inliers"][1] > 40
            lost = 0 if min_inl == 8 else PAIR_NO_MODEL
            assert got["flags"][2] == PAIR_REFIT | lost and got["inliers"][2] == 12 and want[1][2] == (12 if keep or not lost else 0)
            for p in (3, 4):                                         # the fit fails: the input model stands, byte for byte
                assert got["flags"][p] == lost and got["valid"][p] == 0 and got["f"][p].tobytes() == models["f"][2].tobytes(), p
                assert got["inliers"][p] == 12 and want[1][p] == (12 if keep or not lost else 0)
            assert got["usable"][5] == got["records"][5] - 6 and got["flags"][5] == PAIR_REFIT and want[1][5] == got["inliers"][5] > 30


def test_pair_forms(B, ctx):
    import torch
    sc = noisy_depth(B, 361, [90, 100, 110, 120, 130, 140])
    verify, refit = (1.5, 64, 10, 0, 8), (1.5, 2, 10, 0, 1)
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
    assert [int(f) & ~PAIR_REFIT for f in want[2]] == [0, bad, 0, bad, 0, bad, bad, 0] and (want[2] & PAIR_REFIT).sum() >= 3
    # a bad entry's input record is not read: a record that carries a model changes nothing
    forged = models.copy()
    forged[1] = models[0]
    d_forged = upload_models(forged)                                 # (held: the call takes its address)
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_forged.data_ptr(), refit, out_cap)
    assert rc == 0
    same(B, out, want, len(frames), out_cap)
    # the arithmetic form - interleaved stereo: left frames 0, 2, 4 against right frames 1, 3, 5
    frames = [(0, 1), (2, 3), (4, 5)]
    lists = Lists(B, [sc.records(a, b, 45) for a, b in frames])
    spec = B.PairSpec(3, 0, 2, 1, 2, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, verify)
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, 135)
    assert rc == 0
    want = expect(sc, sc, frames, lists, models, refit, 135)
    same(B, out, want, 3, 135)
    assert (want[0]["flags"] & PAIR_REFIT).any()


def test_capacity(B, ctx):
    """out_cap equal to the total, one short (the cut falls in the last pair that keeps anything, an empty pair in front of it and
    one behind), and 0; in_cap 0: every pair with records is BAD"""
    sc = noisy_depth(B, 371, [100] * 7)
    per = [sc.records(1, 0, 60), sc.records(2, 1, 0), sc.records(3, 2, 70), sc.records(4, 3, 30, inliers=0.0), sc.records(5, 4, 80),
           sc.records(6, 5, 0)]
    lists = Lists(B, per)
    spec = B.PairSpec(6, 1, 1, 0, 1, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, (1.0, 128, 16, 0, 4))
    refit = (1.0, 1, 16, 0, 1)
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
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, total, in_cap=0)
    assert rc == 0
    want = expect(sc, sc, chain_frames(6), lists, models, refit, total, in_cap=0)
    same(B, out, want, 6, total)
    assert [int(f) & PAIR_BAD for f in want[2]] == [PAIR_BAD] * 6 and want[1].sum() == 0 and want[0]["records"].sum() == 0


def test_more_pairs_than_the_offsets_workgroup_has_threads(B, ctx):
    """1 025 pairs of 8 ... 12 records, with a cut"""
    import torch
    rng = np.random.default_rng(381)
    sc = noisy_depth(B, 381, [60] * 12)
    n = 1025
    frames = [(int(a), int(b)) for a, b in rng.integers(0, 12, (n, 2))]
    lists = Lists(B, [sc.records(a, b, int(rng.integers(8, 13)), inliers=0.95) for a, b in frames])
    d_pairs = torch.from_numpy(np.array(frames, np.int32)).cuda()
    spec = B.PairSpec(n, 0, 0, 0, 0, d_pairs.data_ptr())
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, (1.5, 16, 8, 1, 2))
    refit = (1.5, 1, 8, 1, 1)
    out_cap = 6000
    rc, out = raw_refit(B, ctx, sc, sc, spec, lists, d_models.data_ptr(), refit, out_cap)
    assert rc == 0
    want = expect(sc, sc, frames, lists, models, refit, out_cap)
    same(B, out, want, n, out_cap)
    assert want[1].sum() > out_cap + 1000 and (want[0]["flags"] & PAIR_REFIT).sum() > 200
    assert 300 < int(np.flatnonzero(want[2] & ROWS_CUT)[0]) < 1000


def test_in_place_and_a_second_call_on_the_stream(B, ctx, seam_scene):
    """d_out_models == d_models; then two more calls back to back on one stream, the second smaller than the first (it runs in the
    scratch the first one grew), no synchronisation in between"""
    import torch
    sc, big, spec, d_models, models = seam_scene
    n = len(SEAMS)
    r1, r2 = (1.5, 2, 8, 0, 1), (1.5, 1, 9, 1, 0)
    cap1, cap2 = int(big.offsets[-1]), 77
    want1 = expect(sc, sc, chain_frames(n), big, models, r1, cap1)
    inplace = settled(d_models.clone())                                 # [npairs + 1, 24] int32: a sentinel record behind the pairs'
    out = filled_outputs(n, cap1)
    rc, _ = raw_refit(B, ctx, sc, sc, spec, big, inplace.data_ptr(), r1, cap1, out=out, out_models_ptr=inplace.data_ptr())
    assert rc == 0
    same(B, (out[0], out[1], out[2], out[3], inplace), want1, n, cap1)
    assert (out[4].cpu().numpy() == SENTINEL).all()
    small_sc = noisy_depth(B, 391, [50, 60, 70])
    small = Lists(B, [small_sc.records(1, 0, 33), small_sc.records(2, 1, 44)])
    spec2 = B.PairSpec(2, 1, 1, 0, 1, None)
    d_models2, models2 = verified_models(B, ctx, small_sc, small_sc, spec2, small, (1.5, 32, 9, 1, 6))
    s = torch.cuda.Stream()
    outs = [filled_outputs(n, cap1), filled_outputs(2, cap2), filled_outputs(n, cap1)]          # (made before the three calls)
    rc1, out1 = raw_refit(B, ctx, sc, sc, spec, big, d_models.data_ptr(), r1, cap1, out=outs[0], stream=s.cuda_stream)
    rc2, out2 = raw_refit(B, ctx, small_sc, small_sc, spec2, small, d_models2.data_ptr(), r2, cap2, out=outs[1], stream=s.cuda_stream)
    rc3, out3 = raw_refit(B, ctx, sc, sc, spec, big, d_models.data_ptr(), r1, cap1, out=outs[2], stream=s.cuda_stream)
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    same(B, out1, want1, n, cap1)
    same(B, out2, expect(small_sc, small_sc, chain_frames(2), small, models2, r2, cap2), 2, cap2)
    same(B, out3, want1, n, cap1)


BAND = 2.0
PIPE_WINDOW = (-200.0, 200.0, -200.0, 200.0, 1)


def test_the_pipeline(B, golden_ast):
    """detect + describe, k-NN (k = 2), select, epipolar verify, epipolar refit (2 rounds, rank 2), then the epipolar-guided k-NN
    (k = 1, a band of 2 px) reading the refitted records IN PLACE - one stream, one synchronisation at the end; every array against
    the restated chain.  The guided matcher takes records that carry BRISK_HIP_PAIR_REFIT (0x10)."""
    import torch
    from test_abi_epipolar import restated_epipolar
    frames = batch_frames(golden_ast)[:5]
    n, h, w = frames.shape
    d = torch.from_numpy(frames).cuda()
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    verify, refit = (3.0, 256, 12, 0, 2024), (3.0, 2, 12, 0, 1)
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    first = ctx.match_knn_pairs(st, st, spec, 2, stream=s.cuda_stream)
    rows_cap = int(first[1].shape[1])
    sel = ctx.select_pair_matches(first, 2, B.MatchSelect(90.0, 0.9, 1), stream=s.cuda_stream)
    ver = ctx.verify_pair_matches_epipolar(st, st, spec, rows_cap, sel[3], sel[0], B.PairVerify(*verify), stream=s.cuda_stream)
    ref = ctx.refit_pair_models_epipolar(st, st, spec, rows_cap, sel[3], sel[0], ver[4], B.PairEpipolarRefit(*refit), stream=s.cuda_stream)
    guided = ctx.match_knn_pairs_epipolar_guided(st, st, spec, 1, ref[4], guide_of(B, PIPE_WINDOW, BAND, 0), rows_cap=rows_cap,
                                                 stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    kd = [ctx.batch_download(f, True, strings=dim) for f in range(n)]
    kps, desc = [k for k, _ in kd], [dd for _, dd in kd]
    node_rows = [len(k) for k in kps]
    xy = [np.stack([k["x"], k["y"]], axis=1).astype(np.float32).reshape(-1, 2) for k in kps]
    so = sel[3].cpu().numpy()
    sm = sel[0].cpu().numpy().view(B.DMATCH).reshape(-1)
    in_cap = len(sm)
    wver = restated_epipolar(chain_frames(n - 1), node_rows, node_rows, rows_cap, xy, xy, so, sm[:int(so[-1])], verify, in_cap, in_cap)
    assert ver[4].cpu().numpy().tobytes() == wver[0].tobytes()
    want = restated_epipolar_refit(chain_frames(n - 1), node_rows, node_rows, rows_cap, xy, xy, so, sm[:int(so[-1])], wver[0], refit, in_cap,
                                   in_cap)
    models, counts, flags, offs, stored = want
    assert ref[4].cpu().numpy().tobytes() == models.tobytes()
    assert ref[1].cpu().numpy().tobytes() == counts.tobytes() and ref[2].cpu().numpy().tobytes() == flags.tobytes()
    assert ref[3].cpu().numpy().tobytes() == offs.tobytes() and ref[0].cpu().numpy()[:len(stored)].tobytes() == stored.tobytes()
    # pair 0 is (img1, img2), the reference's matching test: the refit keeps at least the verifier's inliers, and models are replaced
    assert models["inliers"][0] >= wver[0]["inliers"][0] > 50 and (flags & PAIR_REFIT).any()
    assert models["flags"][2] == PAIR_NO_MODEL and models["hypothesis"][2] == -1          # the blank frame: no input model
    got_rows, _ = knn_rows(B, tuple(t.cpu().numpy() for t in guided), 1)
    found = 0
    for p in range(n - 1):
        M, _ = epi_mask(PIPE_WINDOW, BAND, 0, models[p], kps[p + 1], kps[p])
        rows = oracle_knn(desc[p + 1], desc[p], M, p, 1)[:rows_cap]
        same_rows(got_rows[p], rows)
        found += sum(len(r) for r in rows) if models["flags"][p] & PAIR_REFIT else 0
    assert found > 50                                               # records matched under a model that carries 0x10
    print("pair 0 (img1 -> img2): inliers %d -> %d in %d round(s); %d guided records under refitted models"
          % (wver[0]["inliers"][0], models["inliers"][0], models["valid"][0], found))
    ext.close()
    ctx.close()


def test_arguments(B, ctx):
    """BRISK_HIP_ERR_ARG before anything is launched: the sentinel stays in every output"""
    import torch
    sc = noisy_depth(B, 401, [50, 60, 70])
    lists = Lists(B, [sc.records(1, 0, 30), sc.records(2, 1, 30)])
    spec = B.PairSpec(2, 1, 1, 0, 1, None)
    d_models, models = verified_models(B, ctx, sc, sc, spec, lists, (1.5, 64, 8, 0, 1))
    out = filled_outputs(2, 60)
    L, h = ctx._L, ctx._h
    R = B.PairEpipolarRefit

    def call(**kw):
        a = dict(ctx=h, query=sc.desc_set, train=sc.desc_set, query_kps=sc.kp_set, train_kps=sc.kp_set, pairs=B.PairSpec(2, 1, 1, 0, 1, None),
                 rows_cap=CAP, offsets=lists.d_offsets.data_ptr(), matches=lists.d_matches.data_ptr(), in_cap=lists.in_cap,
                 in_models=d_models.data_ptr(), refit=R(1.5, 2, 8, 0, 1), out_cap=60, models=out[4].data_ptr(), counts=out[1].data_ptr(),
                 flags=out[2].data_ptr(), out_offsets=out[3].data_ptr(), out_matches=out[0].data_ptr())
        a.update(kw)
        ref = lambda v: None if v is None else C.byref(v)
        return L.brisk_hip_refit_pair_models_epipolar_device(a["ctx"], ref(a["query"]), ref(a["train"]), ref(a["query_kps"]), ref(a["train_kps"]),
                                                             ref(a["pairs"]), a["rows_cap"], a["offsets"], a["matches"], a["in_cap"],
                                                             a["in_models"], ref(a["refit"]), a["out_cap"], a["models"], a["counts"], a["flags"],
                                                             a["out_offsets"], a["out_matches"], None)

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
           dict(refit=R(1.5, 0, 8, 0, 1)), dict(refit=R(1.5, 9, 8, 0, 1)), dict(refit=R(1.5, -1, 8, 0, 0)),
           dict(refit=R(1.5, 2, 7, 0, 1)), dict(refit=R(1.5, 2, 4, 0, 1)), dict(refit=R(1.5, 2, -1, 0, 0)),
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
    refit = (1.5, 2, 8, 0, 1)
    rc, got = raw_refit(B, ctx, sc, sc, B.PairSpec(2, 1, 1, 0, 1, None), lists, d_models.data_ptr(), refit, 60, in_cap=45)
    assert rc == 0
    want = expect(sc, sc, chain_frames(2), lists, models, refit, 60, in_cap=45)
    same(B, got, want, 2, 60)
    assert int(want[2][0]) & ~PAIR_REFIT == 0 and want[2][1] == PAIR_BAD | PAIR_NO_MODEL and want[1][0] > 8 and want[1][1] == 0
    assert call() == 0
    same(B, out, expect(sc, sc, chain_frames(2), lists, models, refit, 60), 2, 60)
