"""GPU tests (run with -m gpu) of the dispatch branches behind the public ABI (include/brisk_hip.h) that sizes select: the
tie kernel's forms by frame count, k_describe's ticketed queues, the staged exit of a single-frame result beyond the pinned
buffer, the large-count ordering kernels, the integral format by the density rule, the k_describe variants, the ordered path,
ComputeScale's two forms, host-fed slices, the pool, the post-filters and the 16-bit image functions.

Public-ABI calls only - no brisk_hip_debug_* entry point, no debug bit, no environment knob - so the module runs unchanged on
both builds: in this process on libbrisk_hip.so like every other module, and a second time on libbrisk_hip_release.so, where
nothing but real sizes can reach these branches (test_gpu_release.py, one child process per case group).  Inputs, expected
values and the oracle-side condition that makes each case reach its branch: boundary_cases.py (checked without a GPU by
test_boundary_cases.py).  Keypoints are compared field by field as bit patterns, descriptors as bytes.

Test names carry their case group: test_<a ... g>_..."""
import ctypes as C
import threading

import numpy as np
import pytest

import boundary_cases as BC
from batch_scale_lib import slot_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f].view(np.uint32) if a[f].dtype == np.float32 else a[f],
                                                   b[f].view(np.uint32) if b[f].dtype == np.float32 else b[f]) for f in b.dtype.names)


def explain(a, b):
    if len(a) != len(b):
        return "count %d vs %d" % (len(a), len(b))
    return {f: int((a[f] != b[f]).sum()) for f in b.dtype.names}


def require_256_cus():
    """The frame counts of group (a) select their forms on a 256-CU device (brisk_launch_detect sizes its grids by the device's
    compute units, read from the device properties as here)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip("the tie-kernel forms of these frame counts are derived for 256 compute units, this device has %d (256 on an MI355X)" % cus)


def check_results(res, det, slots, want_of, tag, strings=48):
    """every slot of a batch's two host exits (described rows, detected keypoints) against the oracle"""
    for f in slots:
        ko, ko2, do = want_of(f)
        k, d = res.frame(f, strings)
        assert int(res.flags[f]) == 0 and int(res.counts[f]) == len(ko2), (tag, f, int(res.flags[f]), int(res.counts[f]), len(ko2))
        assert same(k, ko2), (tag, f, explain(k, ko2))
        assert np.array_equal(d, do), (tag, f)
        if det is not None:
            kd, _ = det.frame(f)
            assert int(det.flags[f]) == 0 and same(kd, ko), (tag, f, explain(kd, ko))


def run_batch(B, ctx, ext, stack, thr, octaves, want_of, tag, strings=48):
    """one device-resident batch, both exits to host memory, every slot against the oracle"""
    import torch
    n, h, w = stack.shape
    d = torch.from_numpy(stack).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, thr, octaves, stream)
    rows = sum(len(want_of(f)[1]) for f in range(n))
    rows_det = sum(len(want_of(f)[0]) for f in range(n))
    res = B.HostResults(n, rows + 8, strings, pinned=True)
    det = B.HostResults(n, rows_det + 8, 0, pinned=True)
    t1 = ctx.batch_download_all(res, described=True, stream=stream)
    t0 = ctx.batch_download_all(det, described=False, stream=stream)
    assert ctx.batch_download_wait(t1) == 0 and ctx.batch_download_wait(t0) == 0, tag
    assert ctx.batch_status(n) == 0
    assert int(res.offsets[n]) == rows and int(det.offsets[n]) == rows_det, (tag, int(res.offsets[n]), rows)
    check_results(res, det, range(n), want_of, tag, strings)
    for f in sorted({0, n - 1}):   # the per-frame exit too
        kg, dg = ctx.batch_download(f, described=True, strings=strings)
        assert same(kg, want_of(f)[1]) and np.array_equal(dg, want_of(f)[2]), (tag, f)


# ---- (a) tie-kernel and k_describe queue forms by frame count
A_CASES = [(n,) + BC.A_SIZES[0] for n in BC.A_COUNTS] + [(n,) + BC.A_SIZES[1] for n in BC.A_COUNTS_ODD]


@pytest.mark.parametrize("n,w,h", A_CASES, ids=["%dx%dx%d" % c for c in A_CASES])
def test_a_batch_forms_by_frame_count(B, n, w, h):
    """Four layers on 256 CUs: 1 / 9 / 33 frames = pair form with 8 / 4 / 1 bands, 65 = persistent ticketed k_tie_resolve (288
    tickets), 129 / 200 = four layers per workgroup with 16 / 12 waves, 257 = persistent again; from 8 frames on k_describe runs
    on its eight ticketed queues.  256 x 192: layer 0 read in place; 201 x 131: copied, odd column classes.  Every slot against
    the oracle, on a fresh workspace and on the dirty one."""
    require_256_cus()
    distinct, want = BC.batch_frames(w, h)
    stack = np.stack([distinct[slot_frame(f, 4)] for f in range(n)])
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    for rep in ("fresh", "dirty"):
        run_batch(B, ctx, ext, stack, BC.A_THR, BC.A_OCT, lambda f: want[slot_frame(f, 4)], (n, w, h, rep))
    ext.close()
    ctx.close()


# ---- (b) dense frames: staged copies and the large-count kernels
def test_b_dense_single_frame_leaves_through_the_staged_path(B):
    """640 x 480 noise at threshold 30: the described result (rows of 28 + 64 bytes) exceeds the pinned single-frame buffer,
    the frame has more keypoints than k_finalize and k_desc_prepare keep on chip (boundary_cases.dense_single asserts all three on
    the oracle's counts); host detect, then compute."""
    img, (ko, ko2, do) = BC.dense_single()
    ctx = B.Context(0, max_candidates=262144, max_keypoints=65536)
    ext = B.BriskDescriptorExtractor(context=ctx)
    det = B.BriskFeatureDetector(BC.B_THR, 4, context=ctx)
    for rep in range(2):
        k = det.detect(img, capacity=65536)
        assert same(k, ko), (rep, explain(k, ko))
        k2, d = ext.compute(img, k)
        assert same(k2, ko2), (rep, explain(k2, ko2))
        assert np.array_equal(d, do), rep
    ext.close()
    ctx.close()


def test_b_dense_batch_reaches_the_same_kernels(B):
    frames, want = BC.dense_batch()
    ctx = B.Context(0, max_candidates=262144, max_keypoints=16384)
    ext = B.BriskDescriptorExtractor(context=ctx)
    for rep in ("fresh", "dirty"):
        run_batch(B, ctx, ext, np.stack(frames), BC.B_THR, 2, lambda f: want[f], ("dense batch", rep))
    ext.close()
    ctx.close()


# ---- (c) the integral format by the density rule
def test_c_integral_format_follows_the_previous_batch(B):
    """One context, batches D D F D D (D dense, F constant frames): by the density rule the integral image has 24, 32, 32, 24
    and 32 bits - it shrinks and grows inside one workspace; every batch against the oracle.  Then the format set by the caller:
    descriptor-only calls with 24 and with 32 bits (k_describe's i24 variants without a detector in front)."""
    dense, want = BC.dense_batch()
    flat = BC.flat_batch()
    none = (np.zeros(0, B.KEYPOINT), np.zeros(0, B.KEYPOINT), np.zeros((0, 48), np.uint8))
    ctx = B.Context(0, max_candidates=262144, max_keypoints=16384)
    ext = B.BriskDescriptorExtractor(context=ctx)
    for i, kind in enumerate("DDFDD"):
        if kind == "D":
            run_batch(B, ctx, ext, np.stack(dense), BC.B_THR, 2, lambda f: want[f], ("batch %d (D)" % i))
        else:
            run_batch(B, ctx, ext, np.stack(flat), BC.B_THR, 2, lambda f: none, ("batch %d (F)" % i))
    for fmt in (24, 32, 24, 0):
        ctx.set_integral_format(fmt)
        for f in (0, 3):
            k2, d = ext.compute(dense[f], want[f][0])
            assert same(k2, want[f][1]), (fmt, f, explain(k2, want[f][1]))
            assert np.array_equal(d, want[f][2]), (fmt, f)
    ext.close()
    ctx.close()


# ---- (d) the other k_describe variants
@pytest.mark.parametrize("name", BC.VARIANTS)
def test_d_describe_variant(B, name):
    """briskV1 at patternScale 0.7 (1 024 short pairs: the LDS-table variant) / a custom .ptn pattern at 0.45 (bilinear branch,
    fixed runs): a host call on provided keypoints and a nine-frame batch (the ticketed queues)."""
    kw, X, k, (ko, do), frames, want = BC.variant(name)
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx, **kw)
    assert ext.descriptorSize() == X.strings
    kg, dg = ext.compute(BC.golden_image()["image"], k)
    assert same(kg, ko), explain(kg, ko)
    assert dg.shape == do.shape and np.array_equal(dg, do)
    stack = np.stack([frames[slot_frame(f, 2)] for f in range(9)])
    for rep in ("fresh", "dirty"):
        run_batch(B, ctx, ext, stack, BC.D_THR, BC.D_OCT, lambda f: want[slot_frame(f, 2)], (name, rep), strings=X.strings)
    ext.close()
    ctx.close()


# ---- (e) ordered path and ComputeScale
def test_e_ordered_path_and_no_scale_nms(B):
    img, (ko, ko2, do) = BC.ordered_frame()
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    k = B.BriskFeatureDetector(5, 2, context=ctx).detect(img)
    assert same(k, ko), explain(k, ko)
    k2, d = ext.compute(img, k)
    assert same(k2, ko2) and np.array_equal(d, do)
    run_batch(B, ctx, ext, np.stack([img, img]), 5, 2, lambda f: (ko, ko2, do), "ordered batch")
    img, ko = BC.no_scale_nms_frame()
    k = B.BriskFeatureDetector(60, 2, suppressScaleNonmaxima=False, context=ctx).detect(img)
    assert same(k, ko), explain(k, ko)
    ext.close()
    ctx.close()


def test_e_compute_scale_parallel_form_and_one_lane_walk(B):
    """brisk_hip_compute_scale on a context of 4 096 candidates, four layers: a list of 2 000 points (within 2 x cand_cap /
    nlayers: one lane per (layer, point)) and one of 2 500 (beyond: the one-lane walk - nothing but the size selects it)."""
    img, lists = BC.compute_scale_lists()
    h, w = img.shape
    ctx = B.Context(0, max_candidates=BC.CS_CAND_CAP, max_keypoints=16384)
    for rep in range(2):
        for k, ko in lists:
            out = np.zeros(16384, B.KEYPOINT)
            n = C.c_int()
            ctx.check(ctx._L.brisk_hip_compute_scale(ctx._h, img.ctypes.data_as(C.c_void_p), w, h, w, BC.CS_THR, BC.CS_OCT, 1,
                                                     k.ctypes.data_as(C.c_void_p), len(k), out.ctypes.data_as(C.c_void_p), len(out),
                                                     C.byref(n)))
            assert same(out[:n.value], ko), (rep, len(k), explain(out[:n.value], ko))
    ctx.close()


# ---- (f) host-fed slices and the pool
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_f_host_fed_batch_of_two_slices(B, pinned):
    """brisk_hip_detect_describe_batch_host_results on 65 frames - one more than the default slice of 64 -, destinations in
    pageable and in pinned memory"""
    import torch
    n = BC.HOST_SLICE + 1
    w, h = BC.A_SIZES[0]
    distinct, want = BC.batch_frames(w, h)
    src = torch.from_numpy(np.stack([distinct[slot_frame(f, 4)] for f in range(n)])).pin_memory()
    rows = sum(len(want[slot_frame(f, 4)][1]) for f in range(n))
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    for rep in ("fresh", "dirty"):
        res = B.HostResults(n, rows, 48, pinned=pinned)
        t = ctx.detect_describe_batch_host_results(ext, src.data_ptr(), n, w, h, w * h, w, BC.A_THR, BC.A_OCT, res)
        assert ctx.batch_download_wait(t) == 0
        assert int(res.offsets[n]) == rows
        check_results(res, None, range(n), lambda f: want[slot_frame(f, 4)], ("host-fed", pinned, rep))
    ext.close()
    ctx.close()


def test_f_pool_of_six_threads_on_two_frame_sizes(B):
    cases = BC.pool_frames()
    pool = B.Pool(0, max_batch=8)
    ext = B.BriskDescriptorExtractor()
    errors = []

    def worker(t):
        try:
            for it in range(6):
                img, thr, octv, (wk, wk2, wd) = cases[(t + it) % len(cases)]
                k, tok = pool.detect(img, thr, octv)
                use = tok if it % 3 == 0 else ((tok ^ (0x5A5A << 16)) if it % 3 == 1 else 0)
                k2, d = pool.describe(ext, img, k, use)
                if not (same(k, wk) and same(k2, wk2) and np.array_equal(d, wd)):
                    errors.append((t, it, img.shape, "detected %s" % same(k, wk), "described %s" % same(k2, wk2), hex(use)))
        except Exception as e:
            errors.append((t, repr(e)))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[:5]
    groups, calls = pool.stats()
    assert calls == 6 * 6 * 2 and groups <= calls
    pool.close()
    ext.close()


# ---- (g) post-filters and the 16-bit functions
def test_g_post_filters(B):
    img, (radius, budget_u, ku), (nbu, nbv, budget_b, kb), _ = BC.postfilter_case()
    ctx = B.Context(0)
    k = B.BriskFeatureDetector(BC.G_THR, BC.G_OCT, context=ctx, uniformityRadius=radius, maxNumKpt=budget_u).detect(img)
    assert same(k, ku), explain(k, ku)
    k = B.BriskFeatureDetector(BC.G_THR, BC.G_OCT, context=ctx, maxNumKpt=budget_b, numBucketsU=nbu, numBucketsV=nbv).detect(img)
    assert same(k, kb), explain(k, kb)
    ctx.close()


def test_g_16bit_functions_on_every_width_residue(B):
    """Halfsample16 / Twothirdsample16 / IntegralImage16 on 12 heights x 36 widths (13 ... 48: every residue of the SSE blocks of
    the reference's loops); where the reference writes nothing the engine writes nothing"""
    import oracle_lib as O
    ctx = B.Context(0)
    bad = []
    for h, w in BC.SHAPES16:
        img = BC.image16(h, w)
        for name, fn, ofn in (("half", ctx.halfsample16, O.halfsample16), ("twothird", ctx.twothirdsample16, O.twothirdsample16)):
            want, got = ofn(img), fn(img)
            if (got.any() if want is None else not np.array_equal(got, want)):
                bad.append((name, h, w, "the reference writes nothing" if want is None else "differs"))
        if not np.array_equal(ctx.integral_image16(img).view(np.uint32), O.integral16(img).view(np.uint32)):
            bad.append(("integral", h, w))
    assert not bad, (len(bad), bad[:12])
    ctx.close()


def _cases(fn):
    n = 1
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            n *= len(m.args[1])
    return n


# {case group: {test name: number of cases}} - what test_gpu_release.py selects and expects to pass
GROUPS = {}
for _name, _fn in list(globals().items()):
    if _name.startswith("test_") and callable(_fn):
        GROUPS.setdefault(_name[5], {})[_name] = _cases(_fn)
