"""GPU tests of k_tie_resolve's static step over the window's candidate list (run with -m gpu).

k_tie_resolve (more than 64 frames per call) walks the candidates of a tie's 9 x 9 window where that list has at most
BRISK_TIE_LIST_CAP entries and takes the unrolled loop over the pixel's 24 neighbours for longer lists.  Small frames whose
ties fall on both sides of the cap - inside one launch, one workgroup and one frame - run at the smallest batch that takes this
kernel and at the smallest one whose workgroups own a whole frame; every slot against the oracle, on a fresh workspace and on
the dirty one."""
import ctypes as C

import numpy as np
import pytest

import synth
from test_emul_tie_list import lib as emul_lib
import oracle_lib as O
from batch_scale_lib import slot_frame
from test_gpu_parity import same_kps, explain

W, H, OCTAVES = 200, 150, 4


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


def _blocks(levels, step, base):
    """3 x 3 blocks of random grey levels: every detection is a tie"""
    cells = np.random.default_rng(1487).integers(0, levels, (H // 3 + 1, W // 3 + 1)) * step + base
    return np.kron(cells, np.ones((3, 3)))[:H, :W].astype(np.uint8)


def _frames():
    """three recipe frames; the four-grey-level block image (at threshold 30 more detections than other pixels); a two-level
    block image, whose steps of 200 grey levels keep it dense at threshold 80; one frame with the recipe on the left and the
    four-level blocks on the right"""
    recipe = [synth.gen(W, H, 8100 + s, 12) for s in range(3)]
    blocks4, blocks2 = _blocks(4, 85, 0), _blocks(2, 200, 20)
    mixed = recipe[0].copy()
    mixed[:, W // 2:] = blocks4[:, W // 2:]
    return recipe + [blocks4, blocks2, mixed]


def _window_histogram(img, thr):
    """detections of the full-resolution layer by the number of detections in entries 0 ... 40 of their window"""
    L = emul_lib()
    L.tl_window_histogram.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    hist = np.zeros(42, np.int64)
    img = np.ascontiguousarray(img)
    n = L.tl_window_histogram(img.ctypes.data, img.shape[1], img.shape[0], img.shape[1], thr, hist.ctypes.data)
    assert n == hist.sum()
    return hist


@pytest.mark.parametrize("thr", [80, 30])
def test_the_frames_reach_both_forms(thr):
    """(needs no GPU) lists up to the cap and beyond it on the full-resolution layer, within one frame: at threshold 30 in the
    four-level block image and in the mixed frame, at threshold 80 in the two-level
    block image (the four-level one then has short lists: its steps are 85 grey levels)"""
    cap = emul_lib().tl_cap()
    recipe0, _, _, blocks4, blocks2, mixed = _frames()
    short, long_ = {}, {}
    for name, f in (("recipe", recipe0), ("blocks4", blocks4), ("blocks2", blocks2), ("mixed", mixed)):
        h = _window_histogram(f, thr)
        short[name], long_[name] = int(h[1:cap + 1].sum()), int(h[cap + 1:].sum())
    print("thr %d, cap %d: detections with lists up to the cap %s, beyond it %s" % (thr, cap, short, long_))
    # (bounds that hold for any cap from 6 to 16)
    if thr == 30:
        assert short["recipe"] > 300
        assert short["blocks4"] > 100 and long_["blocks4"] > 1000
        assert short["mixed"] > 300 and long_["mixed"] > 500
    else:
        assert short["blocks4"] > 300
        assert short["blocks2"] > 1000 and long_["blocks2"] > 20


_want = {}   # threshold -> per distinct frame (detected keypoints, described keypoints, descriptors): computed once, left unchanged


def _oracle(thr):
    if thr not in _want:
        X = O.Extractor()
        _want[thr] = []
        for img in _frames():
            ko = O.detect(img, thr, OCTAVES)
            _want[thr].append((ko,) + X.compute(img, ko))
    return _want[thr]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 192])
@pytest.mark.parametrize("thr", [80, 30])
def test_batches_whose_ties_take_both_forms(B, n, thr):
    """65 frames: the smallest call that runs k_tie_resolve (three layers per workgroup, 16 waves); 192 frames: 12 waves and
    a workgroup that owns a whole frame.  Slot f holds distinct frame slot_frame(f, 6): the two forms alternate from workgroup
    to workgroup and, in the block and mixed frames, from tie to tie.  Every slot against the oracle - keypoints as detected,
    as described, descriptors - on a fresh workspace and again on the dirty one."""
    import torch
    distinct, want = _frames(), _oracle(thr)
    nd = len(distinct)
    assert sum(len(k[1]) for k in want) > (3000 if thr == 30 else 1000)
    d = torch.from_numpy(np.stack([distinct[slot_frame(f, nd)] for f in range(n)])).cuda()
    # (the four-level block image has 12 k ties on its full-resolution layer at threshold 30: tie capacity = candidates / 4)
    ctx = B.Context(0, max_candidates=131072, max_keypoints=32768)
    ext = B.BriskDescriptorExtractor(context=ctx)
    for rep in ("fresh", "dirty"):
        ctx.detect_describe_batch(ext, d.data_ptr(), n, W, H, W * H, W, thr, OCTAVES, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert ctx.batch_status(n) == 0
        for f in range(n):
            ko, ko2, do = want[slot_frame(f, nd)]
            kd, _ = ctx.batch_download(f, described=False)
            kg, dg = ctx.batch_download(f, described=True)
            assert same_kps(kd, ko), (n, rep, f, explain(kd, ko))
            assert same_kps(kg, ko2), (n, rep, f, explain(kg, ko2))
            assert np.array_equal(dg, do), (n, rep, f)
    ctx.close()
