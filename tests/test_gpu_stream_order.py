"""GPU tests of the context's promise (include/brisk_hip.h): "every call orders its stream behind the previous call's work,
whichever stream that ran on" - for the calls that follow a batch: the pair matchers, verification, the linker, the list, the track
points and the exits to host memory.

The method: a caller's stream S is HELD by a bounded spin kernel (torch.cuda._sleep).  The first call of a pair is queued on S behind
the hold, the second on another stream S2 that was shown to run beside a held S.  A call that does not order itself then runs too
early - a reader before its writer, a writer before its reader - and the result holds the wrong batch's data, the same way on every
run.  The expectation is the same chain run serially (a synchronisation after every call) for two batches whose outputs differ in
every compared array; other modules compare those outputs with the oracle and the restatements, here they are the expectation of
an ordering property.  Everything is compared as bytes, every output pre-filled with the byte 0x5A of the other modules' sentinels.

No run can pass without having raced: each one asserts that the hold was still pending after its last call was queued."""
import ctypes as C

import numpy as np
import pytest

from test_abi_tracks import restated_link
from test_gpu_match_pairs import batch_frames
from test_gpu_tracks import Chain, make_chain, same_link, sentinel_link_outputs
from test_gpu_verify import CAP, Lists, Scene, chain_frames, expect, raw_verify, same, sentinel_outputs

pytestmark = pytest.mark.gpu

K = 2                                   # the k-NN calls
GATE = (-40.0, 40.0, -40.0, 40.0, 1)    # the gated call: a window that the shifted frames pass and most of (img1, img2) does not
RADIUS, PER_QUERY = 90.0, 4             # the radius call
SELECT = (90.0, 0.9, 1)                 # selection, verification and list: test_gpu_verify.test_the_pipeline's
VERIFY = (3.0, 256, 12, 0, 2024)
MIN_LEN = 2
HOLD_MIN_MS, HOLD_MAX_MS, HOLD_FACTOR = 100.0, 1000.0, 20.0

# the outputs of every call of the chain, in the order the Context methods return them
NAMES = {"knn": ("matches", "counts", "pair_rows"), "gated": ("matches", "counts", "pair_rows"), "radius": ("matches", "counts", "pair_rows"),
         "select": ("matches", "counts", "flags", "offsets"), "verify": ("matches", "counts", "flags", "offsets", "models"),
         "link": ("prev", "track", "age", "summary"), "list": ("track", "len", "offsets", "obs", "summary"), "points": ("points",),
         "tracks": ("summary", "track", "len", "offsets", "points"), "rows": ("counts", "flags", "offsets", "kps", "desc")}
# the calls whose ordering is tested (the selection reads caller memory only: it is a step of the chain, not a reader of the context)
READERS = ("knn", "gated", "radius", "verify", "link", "list", "points", "tracks", "rows")
# the one compared array that is the same for both batches: no frame of either overflows, its flags are 0
CONSTANT = {("rows", "flags")}


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


class Env:
    """one context, one extractor, two batches, the streams and every preallocated output"""


def sptr(stream):
    return C.c_void_p(stream.cuda_stream)


def new_outputs(e):
    """every output of the chain, device tensors and pinned host arrays, sized for everything to fit"""
    torch, B = e.torch, e.B
    np_, cap, n = e.n - 1, e.cap, e.n

    def dev(shape, dtype=torch.int32):
        return torch.empty(shape, dtype=dtype, device="cuda")

    def triple(per_row):
        return dev((np_, cap, per_row, 4)), dev((np_, cap)), dev((np_,))
    i64 = torch.int64
    return {"knn": triple(K), "gated": triple(K), "radius": triple(PER_QUERY),
            "select": (dev((e.matches_cap, 4)), dev((np_,)), dev((np_,)), dev((np_ + 1,), i64)),
            "verify": (dev((e.matches_cap, 4)), dev((np_,)), dev((np_,)), dev((np_ + 1,), i64), dev((np_, 12), i64)),
            "link": (dev((n, cap)), dev((n, cap), i64), dev((n, cap)), dev((8,), i64)),
            "list": (dev((e.list_cap,), i64), dev((e.list_cap,)), dev((e.list_cap + 1,), i64), dev((e.list_cap, 2)), dev((4,), i64)),
            "points": (dev((e.list_cap, 9)),),
            "tracks": B.HostTrackList(e.list_cap, e.list_cap), "rows": B.HostResults(n, n * cap, e.dim)}


def host_arrays(out, key):
    o = out[key]
    return [getattr(o, name) for name in NAMES[key]] if key in ("tracks", "rows") else None


def prefill(e, out):
    """0x5A in every byte of every output (the sentinels of the other modules, whatever the element size)"""
    for key, o in out.items():
        if key in ("tracks", "rows"):
            for a in host_arrays(out, key):
                a.view(np.uint8)[...] = 0x5A
        else:
            for t in o:
                t.view(e.torch.uint8).fill_(0x5A)
    e.torch.cuda.synchronize()


def download(e, out, keys):
    """host copies {key: {array name: ndarray}} of the outputs `keys` (the device idle)"""
    res = {}
    for key in keys:
        arrays = host_arrays(out, key) or [t.cpu().numpy() for t in out[key]]
        res[key] = {name: np.array(a, copy=True) for name, a in zip(NAMES[key], arrays)}
    return res


# ---- the calls, each on preallocated outputs through the C entry points: nothing is allocated between a hold and its end ------------
# call(e, src, out, s): src = the outputs of the serial run whose lists the call is given (caller memory), out = where it writes,
# s = the stream; returns the C return code, a download its ticket as well

def run_batch(e, b, s):
    d = e.d_frames[b]
    return e.L.brisk_hip_detect_describe_batch(e.h, e.ext._h, C.c_void_p(d.data_ptr()), e.n, e.w, e.h_, e.w * e.h_, e.w, 70, 2, s)


def call_knn(e, src, out, s):
    m, cnt, rows = out["knn"]
    return e.L.brisk_hip_match_knn_pairs_device(e.h, C.byref(e.st), C.byref(e.st), C.byref(e.spec), e.dim, K, 0, e.cap, m.data_ptr(),
                                                cnt.data_ptr(), rows.data_ptr(), s)


def call_gated(e, src, out, s):
    m, cnt, rows = out["gated"]
    return e.L.brisk_hip_match_knn_pairs_gated_device(e.h, C.byref(e.st), C.byref(e.st), C.byref(e.kp), C.byref(e.kp), C.byref(e.gate),
                                                      C.byref(e.spec), e.dim, K, 0, e.cap, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), s)


def call_radius(e, src, out, s):
    m, cnt, rows = out["radius"]
    return e.L.brisk_hip_match_radius_pairs_device(e.h, C.byref(e.st), C.byref(e.st), C.byref(e.spec), e.dim, RADIUS, PER_QUERY, e.cap,
                                                   m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), s)


def call_select(e, src, out, s):
    m, cnt, rows = src["knn"]
    o = out["select"]
    return e.L.brisk_hip_select_pair_matches_device(e.h, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), e.n - 1, e.cap, K, C.byref(e.select),
                                                    e.matches_cap, o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[0].data_ptr(), s)


def call_verify(e, src, out, s):
    sel, o = src["select"], out["verify"]
    return e.L.brisk_hip_verify_pair_matches_device(e.h, C.byref(e.st), C.byref(e.st), C.byref(e.kp), C.byref(e.kp), C.byref(e.spec), e.cap,
                                                    sel[3].data_ptr(), sel[0].data_ptr(), e.matches_cap, C.byref(e.verify), e.matches_cap,
                                                    o[4].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[0].data_ptr(), s)


def node_rows(e):
    """the chain of the set's frames 0, 1, ...: the counts in the context's own memory"""
    return int(e.st.d_counts), int(e.st.count_stride)


def call_link(e, src, out, s):
    ver, o = src["verify"], out["link"]
    return e.L.brisk_hip_link_tracks_device(e.h, *node_rows(e), e.n, e.cap, ver[3].data_ptr(), ver[0].data_ptr(), None, o[0].data_ptr(),
                                            o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), s)


def call_list(e, src, out, s):
    ln, o = src["link"], out["list"]
    return e.L.brisk_hip_list_tracks_device(e.h, *node_rows(e), e.n, e.cap, ln[0].data_ptr(), ln[1].data_ptr(), ln[2].data_ptr(), MIN_LEN,
                                            e.list_cap, e.list_cap, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                                            o[4].data_ptr(), s)


def call_points(e, src, out, s):
    ls = src["list"]
    return e.L.brisk_hip_track_points_device(e.h, *node_rows(e), e.n, e.cap, ls[2].data_ptr(), ls[3].data_ptr(), ls[4].data_ptr(), e.list_cap,
                                             C.byref(e.kp), 0, 1, out["points"][0].data_ptr(), s)


def call_tracks(e, src, out, s):
    ln, t = src["link"], C.c_uint(0)
    rc = e.L.brisk_hip_tracks_download(e.h, *node_rows(e), e.n, e.cap, ln[0].data_ptr(), ln[1].data_ptr(), ln[2].data_ptr(), MIN_LEN,
                                       C.byref(e.kp), 0, 1, C.byref(out["tracks"].struct), s, C.byref(t))
    e.tickets.append((e.ctx.tracks_wait, t.value))
    return rc


def call_rows(e, src, out, s):
    t = C.c_uint(0)
    rc = e.L.brisk_hip_batch_download_all(e.h, 1, C.byref(out["rows"].struct), s, C.byref(t))
    e.tickets.append((e.ctx.batch_download_wait, t.value))
    return rc


CALLS = {"knn": call_knn, "gated": call_gated, "radius": call_radius, "select": call_select, "verify": call_verify, "link": call_link,
         "list": call_list, "points": call_points, "tracks": call_tracks, "rows": call_rows}
CHAIN = ("knn", "gated", "radius", "select", "verify", "link", "list", "points", "tracks", "rows")     # (NAMES' order)


def finish(e):
    """the device idle, then the transfers queued since the last call completed: none of them flagged"""
    e.torch.cuda.synchronize()
    for wait, ticket in e.tickets:
        assert ticket != 0 and wait(ticket) == 0
    e.tickets.clear()


def run_chain(e, b, out, s, serial):
    """batch b and its whole chain on stream s, every step reading the lists the step before wrote into `out`"""
    assert run_batch(e, b, s) == 0
    for key in CHAIN:
        if serial:
            e.torch.cuda.synchronize()
        assert CALLS[key](e, out, out, s) == 0, (key, e.ctx._L.brisk_hip_last_error(e.h))
    if serial:
        finish(e)


def timed_sleep(e, cycles):
    torch = e.torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(e.S):
        a.record()
        torch.cuda._sleep(int(cycles))
        b.record()
    b.synchronize()
    return a.elapsed_time(b)


def hold(e):
    """stream S busy for the calibrated time; the event behind the spin kernel"""
    ev = e.torch.cuda.Event()
    with e.torch.cuda.stream(e.S):
        e.torch.cuda._sleep(e.hold_cycles)
        ev.record()
    return ev


@pytest.fixture(scope="module")
def env(B, golden_ast):
    import torch
    e = Env()
    e.B, e.torch, e.tickets = B, torch, []
    frames = batch_frames(golden_ast)[:5]
    e.n, e.h_, e.w = frames.shape
    e.host_frame = np.ascontiguousarray(frames[1])
    e.d_frames = {1: torch.from_numpy(frames).cuda(), 2: torch.from_numpy(np.ascontiguousarray(frames[::-1])).cuda()}
    e.ctx = B.Context(0)
    e.L, e.h = e.ctx._L, e.ctx._h
    e.ext = B.BriskDescriptorExtractor(context=e.ctx)
    e.det = B.BriskFeatureDetector(70, 2, context=e.ctx)
    e.spec, e.gate = B.PairSpec(e.n - 1, 1, 1, 0, 1, None), B.MatchGate(*GATE)
    e.select, e.verify = B.MatchSelect(*SELECT), B.PairVerify(*VERIFY)
    e.S, e.main = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    # the first batch: the sets every later call is given.  They name the context's own buffers, the same for every batch - which
    # is what makes the next batch a writer of what the readers of this one read
    assert run_batch(e, 1, sptr(e.main)) == 0
    torch.cuda.synchronize()
    (e.st, e.dim), e.kp = e.ctx.batch_desc_set(), e.ctx.batch_kp_set()
    cap = C.c_int()
    e.ctx.check(e.L.brisk_hip_batch_results(e.h, None, None, None, None, None, None, C.byref(cap), None))
    e.cap = cap.value
    e.matches_cap, e.list_cap = (e.n - 1) * e.cap * K, e.n * e.cap
    # the serial reference; it grows every scratch, both slabs of both transfer rings and the result buffers
    e.serial_dev, e.serial = {}, {}
    for b in (1, 2):
        e.serial_dev[b] = new_outputs(e)
        prefill(e, e.serial_dev[b])
        run_chain(e, b, e.serial_dev[b], sptr(e.main), serial=True)
        assert e.ctx.batch_status(e.n) == 0
        st, kp = e.ctx.batch_desc_set()[0], e.ctx.batch_kp_set()
        assert bytes(st) == bytes(e.st) and bytes(kp) == bytes(e.kp)
        e.serial[b] = download(e, e.serial_dev[b], CHAIN)
    same_arrays = [(key, name) for key in READERS for name in NAMES[key]
                   if e.serial[1][key][name].tobytes() == e.serial[2][key][name].tobytes()]
    assert set(same_arrays) == CONSTANT, "a case on these arrays would prove nothing: the two batches give the same bytes %r" % (same_arrays,)
    assert not e.serial[1]["rows"]["flags"][:e.n].any()
    e.detected = e.det.detect(e.host_frame)              # (the host call's own buffers grow here)
    assert len(e.detected) > 100
    # the device time of one batch and its chain, queued without a pause
    e.out = new_outputs(e)
    prefill(e, e.out)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(e.main)
    run_chain(e, 1, e.out, sptr(e.main), serial=False)
    t1.record(e.main)
    finish(e)
    e.chain_ms = t0.elapsed_time(t1)
    for key in READERS:                                    # (and the chain without synchronisations gives the serial bytes)
        compare(e, key, 1)
    # the hold: cycles of the spin kernel for max(100 ms, 20 x chain), at most 1 s - per-machine calibrations, printed only
    timed_sleep(e, 1000)
    small = max(timed_sleep(e, 1000000), 1e-3)
    cycles = 1000000 * 20.0 / small                       # about 20 ms: long against the launch
    per_ms = cycles / max(timed_sleep(e, cycles), 1e-3)
    e.hold_ms = min(HOLD_MAX_MS, max(HOLD_MIN_MS, HOLD_FACTOR * e.chain_ms))
    e.hold_cycles = int(e.hold_ms * per_ms)
    measured = timed_sleep(e, e.hold_cycles)
    print("\nstream order: chain %.3f ms, hold %.0f ms = %d cycles (measured %.1f ms)" % (e.chain_ms, e.hold_ms, e.hold_cycles, measured))
    assert 0.5 * e.hold_ms < measured < 2.0 * HOLD_MAX_MS, "the spin kernel's length does not follow its cycles"
    # S2: the first fresh stream that runs a kernel to its end while S is held (two streams can share a hardware queue)
    flag = torch.zeros(64, dtype=torch.int32, device="cuda")
    e.S2, tried = None, []
    for _ in range(8):
        cand = torch.cuda.Stream()
        torch.cuda.synchronize()
        hev, done = hold(e), torch.cuda.Event()
        with torch.cuda.stream(cand):
            flag.fill_(1)
            done.record()
        done.synchronize()
        beside = not hev.query()
        torch.cuda.synchronize()
        tried.append((hex(cand.cuda_stream), beside))
        if beside:
            e.S2 = cand
            break
    print("stream order: S = %s, candidates for S2 (ran beside the held S): %r" % (hex(e.S.cuda_stream), tried))
    assert e.S2 is not None, "none of 8 fresh streams ran beside the held stream S: no case of this module can race (%r)" % (tried,)
    # information: does a whole batch on S2 - it also uses streams of the context's own - end inside a hold of S?  (What a writer
    # that wrongly does not wait needs, to be seen by the reader behind the hold.)
    hev, done = hold(e), torch.cuda.Event()
    assert run_batch(e, 2, sptr(e.S2)) == 0
    done.record(e.S2)
    done.synchronize()
    print("stream order: a batch on S2 ended inside a hold of S: %s" % (not hev.query()))
    torch.cuda.synchronize()
    yield e
    torch.cuda.synchronize()
    e.ext.close()
    e.ctx.close()


def compare(e, key, b, out=None):
    """the outputs `key` of e.out (or out), as bytes, against the serial run of batch b; the message names the array"""
    got = download(e, out or e.out, [key])[key]
    for name in NAMES[key]:
        g, w = got[name], e.serial[b][key][name]
        if g.tobytes() != w.tobytes():
            other = e.serial[3 - b][key][name]
            gw, ww = g.view(np.uint8).reshape(-1), w.view(np.uint8).reshape(-1)
            bad = np.flatnonzero(gw != ww)
            raise AssertionError("%s.%s is not the serial run's of batch %d: %d of %d bytes differ, the first at %d; equal to batch %d's: %s; "
                                 "still all sentinel: %s" % (key, name, b, len(bad), len(gw), bad[0], 3 - b, g.tobytes() == other.tobytes(),
                                                             bool((gw == 0x5A).all())))


def begin(e):
    """batch 1 complete and the context idle, the outputs pre-filled: where every case starts"""
    assert run_batch(e, 1, sptr(e.main)) == 0
    prefill(e, e.out)


def race(e, first, second):
    """hold(S), first(S), second(S2); the hold must still be pending when both are queued.  Also prints whether S2's work ended
    inside the hold (information: with calls that are ordered it cannot)"""
    torch = e.torch
    hev, done2 = hold(e), torch.cuda.Event()
    assert first(sptr(e.S)) == 0, e.L.brisk_hip_last_error(e.h)
    assert second(sptr(e.S2)) == 0, e.L.brisk_hip_last_error(e.h)
    done2.record(e.S2)
    pending = not hev.query()
    done2.synchronize()
    inside = not hev.query()
    finish(e)
    assert pending, "the hold of %.0f ms ended before both calls were queued: the run proved nothing" % e.hold_ms
    print("  S2's work ended inside the hold: %s" % inside)


@pytest.mark.parametrize("reader", READERS)
def test_write_after_read(env, reader):
    """batch 1 complete; the reader on the held S, batch 2 - which overwrites the descriptors, keypoints and counts the reader is
    given - on S2.  The reader's outputs are batch 1's: batch 2 waited for it."""
    e = env
    begin(e)
    race(e, lambda s: CALLS[reader](e, e.serial_dev[1], e.out, s), lambda s: run_batch(e, 2, s))
    compare(e, reader, 1)


@pytest.mark.parametrize("reader", READERS)
def test_read_after_write(env, reader):
    """batch 1 complete; batch 2 on the held S, the reader - given batch 2's lists - on S2.  Its outputs are batch 2's: it waited
    for the batch."""
    e = env
    begin(e)
    race(e, lambda s: run_batch(e, 2, s), lambda s: CALLS[reader](e, e.serial_dev[2], e.out, s))
    compare(e, reader, 2)


@pytest.mark.parametrize("reader", ["knn", "points"])
def test_the_context_s_own_stream(env, reader):
    """the reader on the held S, then a host detect() of one frame on the same context: it runs on the context's stream, rewrites
    frame 0 of the buffers the reader is given and returns when its results are on the host - so when it returns, the reader, and
    the hold in front of it, must be over.  The context's stream cannot be shown to run beside S beforehand (it is the context's
    own): if the two share a hardware queue the host call waits for the hold whatever the code does, and this case passes
    vacuously.  The two directions above cannot."""
    e = env
    begin(e)
    hev = hold(e)
    assert CALLS[reader](e, e.serial_dev[1], e.out, sptr(e.S)) == 0
    pending = not hev.query()
    kps = e.det.detect(e.host_frame)
    over = hev.query()
    finish(e)
    assert pending, "the hold of %.0f ms ended before the reader was queued: the run proved nothing" % e.hold_ms
    assert over, "detect() returned while the reader on the other stream was still waiting: it did not order itself behind it"
    assert kps.tobytes() == e.detected.tobytes()
    compare(e, reader, 1)


def test_two_scratch_users_on_two_streams(B, env):
    """verify of batch 1's lists on the held S; link, then verify, of a smaller hand-made input on S2 - the second verify runs in the
    scratch the first one sized.  All three results are right.  What this shows: the calls accept the pattern, scratch that is
    shared across streams included.  What it cannot show: a missing wait - with the hold, calls that are not ordered run one after
    the other anyway, in the other order, and users of one scratch that do not overlap in time do not disturb each other."""
    e = env
    sc = Scene(B, 91, [50, 60, 70])
    lists = Lists(B, [sc.records(1, 0, 33), sc.records(2, 1, 44)])
    small_spec, small_verify, small_cap = B.PairSpec(2, 1, 1, 0, 1, None), (1.0, 32, 5, 1, 6), 77
    rows = [65, 0, 40]
    offsets, m = make_chain(B, 7, rows)
    ch = Chain(B, rows, CAP, offsets, m)
    link_out = sentinel_link_outputs(ch.nodes, ch.rows_cap)
    ver_out = sentinel_outputs(2, small_cap)
    begin(e)

    def second(s):
        rc = e.L.brisk_hip_link_tracks_device(e.h, ch.d_rows.data_ptr(), ch.stride, ch.nodes, ch.rows_cap, ch.d_offsets.data_ptr(),
                                              ch.d_matches.data_ptr(), None, link_out[0].data_ptr(), link_out[1].data_ptr(),
                                              link_out[2].data_ptr(), link_out[3].data_ptr(), s)
        return rc or raw_verify(B, e.ctx, sc, sc, small_spec, lists, small_verify, small_cap, out=ver_out, stream=e.S2.cuda_stream)[0]
    race(e, lambda s: call_verify(e, e.serial_dev[1], e.out, s), second)
    compare(e, "verify", 1)
    same_link(tuple(t.cpu().numpy() for t in link_out), restated_link(rows, CAP, offsets, m))
    same(B, ver_out, expect(sc, sc, chain_frames(2), lists, small_verify, small_cap), 2, small_cap)
