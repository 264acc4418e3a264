#!/usr/bin/env python3
"""What matching adds to the bench line's stream: bench.py's workload (1080p App.-C frames, threshold 80, 4 octaves, 512 frames
per batch, frames resident in HBM), every frame matched against the previous one, k = 2.  In ONE process, after warm-up,
alternating windows that each end in a synchronise:
  A  detect_describe_batch alone
  B  detect_describe_batch + match_knn_pairs on the same stream (brisk_hip_match_knn_pairs_device: one launch, counts read on
     the device)
  C  detect_describe_batch, synchronise, download the counts, one brisk_hip_match_knn_device call per pair - the only way
     there was before the pair call (that entry point is unchanged)
and writes profiles/match_pairs.json: frames/s of A, B, C, the matching cost per batch (B - A, C - A), the spread over the
repeats, the kernel revision and whether B's and C's rows are identical.
With --radius R [--cap N] the same three windows for radius matching (profiles/match_radius_pairs.json):
  B  detect_describe_batch + match_radius_pairs on the same stream (brisk_hip_match_radius_pairs_device)
  C  detect_describe_batch, synchronise, download every frame's rows, one brisk_hip_match_radius call per pair (host pointers:
     each call uploads its rows again) - the only way there was before the radius pair call
plus the threshold, the cap, the hits per query row (mean, max) and the share of rows that took the kernel's dense path.
With --gate dx_min,dx_max,dy_min,dy_max[,octaves] (with and without --radius) five windows instead of three
(profiles/match_pairs_gated.json / profiles/match_radius_pairs_gated.json):
  B  as above - the UNGATED pair call
  G  detect_describe_batch + the gated pair call with the given gate (brisk_hip_match_knn_pairs_gated_device /
     brisk_hip_match_radius_pairs_gated_device, keypoints from brisk_hip_batch_kp_set)
  I  the same with the all-pass gate (-inf, +inf, -inf, +inf, -1): what the predicate costs when it rejects nothing
  C  what a caller had to do before: synchronise, download every frame's keypoints and rows, build the mask of every pair on
     the host, one brisk_hip_match_knn / brisk_hip_match_radius call with that mask per pair
plus, computed on the host from the downloaded keypoints: the share of (64-query wave, train row) steps in which no lane is
allowed (the steps the gated kernels skip), the share of query rows with no allowed row, the mask density, and whether G's rows
equal C's (k-NN: C's rows without the reference's top-up entries of distance 2147483648, which the gated call never writes).
With --export (k-NN only, profiles/match_pairs_export.json) the cost of getting the matches to the HOST, three windows:
  B  detect_describe_batch + match_knn_pairs on the same stream: the matches stay in HBM
  E  B + pair_matches_download (brisk_hip_pair_matches_download: ratio test 0.8, best match per row) into pinned memory, two
     destinations alternating, a ticket waited for two batches later
  D  B + a plain asynchronous device-to-host copy of the three padded arrays (at --rows-cap) on a copy stream, two device triples
     and two pinned destinations alternating - what a caller could do without the packed exit
plus the bytes E and D move per batch and the share of query rows whose match is selected.
With --tracks (k-NN only, profiles/track_pairs.json) what linking the matches into feature tracks adds, two windows:
  B  detect_describe_batch + match_knn_pairs + select_pair_matches (ratio 0.8, best match per row) on the same stream
  T  B + brisk_hip_link_tracks_device + brisk_hip_list_tracks_device (min_len 3) on the same stream, every batch numbered on from
     the one before through d_first_new (the call's own summary word: no synchronisation)
plus the HIP-event time of the link call and of the list call (six launches each; a `rocprofv3 --kernel-trace --stats` pass
around --tracks --stats-pass gives the single kernels: profiles/track_pairs_kernel_stats.csv), tracks and links per batch, and
whether the device's arrays equal a host restatement of the rule on the downloaded lists of one batch.
With --tracks-download (k-NN only, profiles/track_download.json) what getting the listed tracks to the HOST costs, three windows:
  T  --tracks' window T: detect + describe + match + select + link + list, the lists stay in HBM
  D  T with brisk_hip_tracks_download (min_len 3) into pinned memory in place of the list call, two destinations alternating, a
     ticket waited for one batch later
  P  what a caller had to do before that exit, with the other entry points only: T, a synchronisation to read the list's summary,
     one hipMemcpy per list array (the stored prefixes) and brisk_hip_batch_download_all of the batch's keypoints, waited for at
     once; the join of (node, row) against those keypoints on the host is NOT timed
plus D / T, D / P, the spread of T's windows, the bytes that cross the link per batch in D and in P, and whether D's arrays equal
the list call's arrays joined with batch_download_all's keypoints on the host (--stats-pass: D iterations only, for the kernel
trace behind profiles/track_download_kernel_stats.csv).
With --verify (k-NN only, profiles/verify_pairs.json) what checking the matches against a homography adds, two windows:
  T  --tracks' window T: detect + describe + match + select + link + list
  V  T with brisk_hip_verify_pair_matches_device (--hypotheses 256, --max-error 3, --min-inliers 8, pairs without a model keep their
     usable records) between select and link: the linker reads the verified lists
plus V / T beside the spread of both windows, the HIP-event time of the verify call (three launches; a `rocprofv3 --kernel-trace
--stats` pass around --verify --stats-pass gives the single kernels), the records per pair that go in and come out, the pairs with
an accepted model, and whether the device's arrays equal the NumPy restatement of the rule on one batch's downloaded lists.
With --epipolar (k-NN only, profiles/epipolar_pairs.json) the same two windows with brisk_hip_verify_pair_matches_epipolar_device in
the verifier's place, E instead of V: E / T, the HIP-event time of the call, the records in and out, and whether the device's arrays
equal the restatement of the epipolar rule (tests/test_abi_epipolar.py).  --epipolar --stats-pass runs E and, on the same lists, the
homography verifier, so that a `rocprofv3 --kernel-trace --stats` pass around it gives k_epipolar_ransac beside k_verify_ransac.
With --refit (k-NN only, profiles/refit_pairs.json) what fitting the pairs' models again to all their inliers adds, two windows:
  V  --verify's window V: detect + describe + match + select + verify + link + list
  R  V with brisk_hip_refit_pair_models_device (--rounds 2, the verifier's threshold, the models in place) between verify and link
plus R / V beside the spread of both windows and the HIP-event time of the refit call (three launches).  The stream's consecutive
frames are unrelated, so no pair there has a model (as with --guided): the call's time is also taken on a RELATED batch made here
(as many pairs, 1 024 points a frame seen through mild homographies with 0.5 px noise, --related-records 200 records a pair, three
quarters of them true), whose result is compared with the restated rule.  --refit --stats-pass runs the related batch only, so
that a `rocprofv3 --kernel-trace --stats` pass around it gives k_refit_models on pairs that have models.
With --epirefit (profiles/epipolar_refit_pairs.json) the refit of the epipolar branch beside its yardstick, two windows of back-to-back
calls on --refit's related batch (--batch - 1 pairs, the same lists, the same --rounds, one process; no frame is detected):
  H  brisk_hip_refit_pair_models_device on the homography verifier's models            (the yardstick)
  F  brisk_hip_refit_pair_models_epipolar_device (--rank2 1) on the epipolar verifier's models
plus F / H of the windows' medians and of the HIP-event times of one call each, the rounds that replaced a model in either, and
whether F's arrays equal the restated rule (tests/test_abi_epipolar_refit.py).  The related batch is a PLANE seen through homographies:
both verifiers find models on it.  --epirefit --stats-pass runs ten calls of each, for a `rocprofv3 --kernel-trace --stats` pass:
k_refit_epipolar beside k_refit_models (profiles/epipolar_refit_pairs_kernel_stats.csv).
With --epiguided (k-NN only, profiles/epiguided_pairs.json) the second pass of the epipolar branch, two windows:
  E  --epipolar's E
  L  E followed by brisk_hip_match_knn_pairs_epipolar_guided_device (k = 1, band = --max-error, window +-64 px, octave difference 1,
     fallback 0) reading the verifier's models in place, select (keep 1) and link on the new lists
plus L / E beside the spread of both windows, the HIP-event time of the call, the records per pair that reach the linker and the links
made in E and in L, and whether every record of L is a Sampson inlier of its pair's model inside the window.  The stream's frames are
unrelated, yet the epipolar verifier accepts models at --min-inliers 8, so L does scan.  --epiguided --stats-pass [--epi-case window |
band] is for a `rocprofv3 --kernel-trace --stats` pass of its own per case: k_epiline_knn_pairs<12> with the band off under a +-6 px
window beside k_match_knn_pairs_gated<12, false> at the same window and shapes (the same rows pass: the difference is the band's
arithmetic), and with band 3 under an all-pass window beside the ungated k_match_knn_pairs<12, false> (whether skipping rows pays for the
fp64 test): profiles/epiguided_pairs_kernel_stats.csv.

With --guided --mutual or --epiguided --mutual (profiles/match_mutual_pairs.json, one entry per form) the mutual guided call beside its
yardsticks, four windows of back-to-back calls on one batch's sets, every pair guided (identity models under a +-6 px window; rectified
models under band = --max-error and a +-64 px window):
  U  the guided (epipolar-guided) k-NN call, k = 1        M  the mutual call
  N  the gated k-NN call at the same window, k = 1        X  N with cross_check = 1
plus M / U beside X / N - the same backward scan with the lane's own position instead of a staged centre -, the HIP-event time of one
call of each, and, under identity models, whether M's arrays equal X's byte for byte.

With --guided (k-NN only, profiles/guided_pairs.json) what matching again under the pairs' models adds, two windows:
  V  --verify's window V: detect + describe + match + select + verify + link + list
  G  V followed by brisk_hip_match_knn_pairs_guided_device (k = 1, window +-6 px, octave difference 1, fallback 0) reading the verifier's
     models in place, brisk_hip_select_pair_matches_device (distance bound only, keep 1) and brisk_hip_link_tracks_device on the
     guided lists
plus G / V beside the spread of both windows, the HIP-event time of the guided call (one launch; a `rocprofv3 --kernel-trace --stats`
pass around --guided --stats-pass gives the guided kernel - under identity models, so that every pair is guided and the same rows pass -
beside the gated k-NN kernel at the same window, shapes and build: profiles/guided_pairs_kernel_stats.csv), the records per pair that reach the linker and the links it makes in V and in G, and
whether every guided record lies inside the window around its restated centre.
Usage: python tools/bench_match_pairs.py [--repeats 5] [--window 0.4] [--rows-cap 2048] [--radius R [--cap N]] [--gate ...] [--out FILE]
       --stats-pass: warm-up + a few B iterations (with --gate: B, G and I) only, nothing written (the run a
       `rocprofv3 --kernel-trace --stats` pass wraps; its kernel statistics are kept as profiles/match_pairs_kernel_stats.csv)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import ethzasl_brisk_amd as B
from bench import gen_frames, W, H, OCTAVES, THRESHOLD   # the bench line's frame generator and workload constants
import synth


class DeviceBytes:
    """a device pointer as a flat uint8 array torch can wrap (the descriptor rows of the last batch)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}


class DeviceInts:
    """a device pointer as a flat int32 array torch can wrap (the counters of the last batch)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def export_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, batch, run_b):
    """--export: windows B, E, D (see the module's text); writes a.out"""
    st = work.cuda_stream
    select = B.MatchSelect(float("inf"), 0.8, 1)
    dst = [B.HostMatches(n - 1, (n - 1) * cap, pinned=True) for _ in range(2)]        # (one match per row at the most)
    tickets = []

    def run_e():
        run_b()
        if len(tickets) >= 2:                                      # the destination about to be reused: its ticket from two batches ago
            ctx.pair_matches_wait(tickets[-2])
        tickets.append(ctx.pair_matches_download(outs["B"], k, select, dst[len(tickets) % 2], stream=st))

    def drain_e():
        for t in tickets[-2:]:
            ctx.pair_matches_wait(t)
        del tickets[:]

    copy = torch.cuda.Stream(device=dev)
    triples = [outs["B"], outs["C"]]
    pinned = [tuple(torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in outs["B"]) for _ in range(2)]
    copied = [torch.cuda.Event(), torch.cuda.Event()]
    calls_d = [0]

    def run_d():
        i = calls_d[0] % 2
        calls_d[0] += 1
        work.wait_event(copied[i])                                 # this triple's copy of two batches ago
        copied[i].synchronize()                                    # ... and the host is done with its destination (as E's wait)
        batch()
        dset, dim = ctx.batch_desc_set()
        ctx.match_knn_pairs(dset, dset, B.PairSpec(n - 1, 1, 1, 0, 1, None), k, rows_cap=cap, stream=st, dim_bytes=dim, out=triples[i])
        copy.wait_stream(work)
        with torch.cuda.stream(copy):
            for h, t in zip(pinned[i], triples[i]):
                h.copy_(t, non_blocking=True)
            copied[i].record(copy)

    for ev in copied:
        ev.record(work)
    runs = {"B": run_b, "E": run_e, "D": run_d}
    ends = {"B": lambda: None, "E": drain_e, "D": lambda: None}
    order = "BED"
    for v in order + "BE":                                         # warm-up: buffers sized, slabs grown
        runs[v]()
        ends[v]()
        torch.cuda.synchronize()

    # what E delivers, checked against the padded arrays D copied (the same batch content in every call)
    run_e()
    drain_e()
    run_d()
    torch.cuda.synchronize()
    m, cnt, rows = (h.numpy() for h in pinned[(calls_d[0] - 1) % 2])
    m = m.view(B.DMATCH).reshape(n - 1, cap, k)
    d0, d1 = m[:, :, 0]["distance"], m[:, :, k - 1]["distance"]
    valid = (np.arange(cap)[None, :] < np.minimum(rows, cap)[:, None]) & (cnt >= 1)
    top = np.float32(2147483648.0)
    keep = valid & (d0 != top) & ((cnt == 1) | (d1 == top) | (d0 < np.float32(0.8) * d1)) if k >= 2 else valid & (d0 != top)
    got = [d for d in dst if int(d.offsets[n - 1]) == int(keep.sum())]
    identical = bool(got) and got[0].matches[:int(keep.sum())].tobytes() == m[:, :, 0][keep].tobytes()
    selected = int(keep.sum())
    bytes_e = 4 * 3 * (n - 1) + 8 * n + 16 * selected
    bytes_d = sum(t.numel() * t.element_size() for t in outs["B"])

    fps = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                runs[v]()
                calls += 1
                if time.perf_counter() - t0 >= a.window:
                    break
            ends[v]()
            torch.cuda.synchronize()
            fps[v].append(calls * n / (time.perf_counter() - t0))
    med = {v: float(np.median(fps[v])) for v in order}
    ms = {v: 1e3 * n / med[v] for v in order}
    spread = {v: (max(fps[v]) - min(fps[v])) / med[v] for v in order}
    res = {
        "workload": "bench.py's stream: %dx%d, threshold %d, %d octaves, %d frames per batch (%d distinct) in HBM; frame-to-previous-frame, "
                    "k = %d, rows_cap %d; E selects with ratio 0.8, one match per row" % (W, H, THRESHOLD, OCTAVES, n, nd, k, cap),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window,
                    "order": ", ".join(order) + " alternating; every window ends with its transfers complete and a synchronise"},
        "frames_per_s": {v: round(med[v], 1) for v in order},
        "frames_per_s_all": {v: [round(x, 1) for x in fps[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "ms_per_batch": {v: round(ms[v], 4) for v in order},
        "exit_ms_per_batch": {"E_minus_B": round(ms["E"] - ms["B"], 4), "D_minus_B": round(ms["D"] - ms["B"], 4)},
        "E_over_B_frames_per_s": round(med["E"] / med["B"], 4),
        "E_over_D_frames_per_s": round(med["E"] / med["D"], 4),
        "bytes_per_batch": {"E": bytes_e, "D": bytes_d},
        "rows_with_entries": int(valid.sum()),
        "matches_selected": selected,
        "share_of_rows_selected": round(selected / max(int(valid.sum()), 1), 4),
        "E_equals_rule_on_D_arrays": identical,
        "legend": {"B": "detect_describe_batch + brisk_hip_match_knn_pairs_device on the same stream",
                   "E": "B + brisk_hip_pair_matches_download (ratio 0.8) into pinned memory, waited for two batches later",
                   "D": "B + asynchronous device-to-host copies of d_out, d_out_count, d_pair_rows (padded) on a copy stream"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ext.close()
    ctx.close()


def tracks_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b0):
    """--tracks: windows B and T (see the module's text); writes a.out"""
    from test_abi_tracks import restated_link, restated_list, SENT32
    st = work.cuda_stream
    select = B.MatchSelect(float("inf"), 0.8, 1)
    L, h = ctx._L, ctx._h
    mcap = (n - 1) * cap                                            # (one match per row at the most)
    sel = (torch.zeros((mcap, 4), dtype=torch.int32, device=dev), torch.zeros(n - 1, dtype=torch.int32, device=dev),
           torch.zeros(n - 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))
    prev, age = (torch.zeros((n, cap), dtype=torch.int32, device=dev) for _ in range(2))
    track = torch.zeros((n, cap), dtype=torch.int64, device=dev)
    summary = torch.zeros(8, dtype=torch.int64, device=dev)
    tcap, ocap = n * cap // 4, n * cap
    lists = (torch.zeros(tcap, dtype=torch.int64, device=dev), torch.zeros(tcap, dtype=torch.int32, device=dev),
             torch.zeros(tcap + 1, dtype=torch.int64, device=dev), torch.zeros((ocap, 2), dtype=torch.int32, device=dev),
             torch.zeros(4, dtype=torch.int64, device=dev))
    seed = B.TrackSeed(None, None, 0, summary.data_ptr())           # numbered on from the call before
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    m, cnt, rows = outs["B"]

    def run_b():
        run_b0()
        ctx.check(L.brisk_hip_select_pair_matches_device(h, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), n - 1, cap, k, C.byref(select), mcap,
                                                         sel[1].data_ptr(), sel[2].data_ptr(), sel[3].data_ptr(), sel[0].data_ptr(), st))

    def run_t(timed=False):
        run_b()
        dset, _ = ctx.batch_desc_set()
        ptr, stride = ctx._node_rows((dset, 0, 1))
        if timed:
            ev[0].record(work)
        ctx.check(L.brisk_hip_link_tracks_device(h, ptr, stride, n, cap, sel[3].data_ptr(), sel[0].data_ptr(), C.byref(seed), prev.data_ptr(),
                                                 track.data_ptr(), age.data_ptr(), summary.data_ptr(), st))
        if timed:
            ev[1].record(work)
        ctx.check(L.brisk_hip_list_tracks_device(h, ptr, stride, n, cap, prev.data_ptr(), track.data_ptr(), age.data_ptr(), 3, tcap, ocap,
                                                 lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(), lists[3].data_ptr(),
                                                 lists[4].data_ptr(), st))
        if timed:
            ev[2].record(work)

    runs = {"B": run_b, "T": run_t}
    order = "BT"
    for v in order + "BT":                                          # warm-up: buffers sized, scratch grown
        runs[v]()
        torch.cuda.synchronize()
    if a.stats_pass:
        for _ in range(8):
            run_t()
        torch.cuda.synchronize()
        return

    # one batch against the restatement of the rule on its downloaded lists
    summary.zero_()
    run_t()
    torch.cuda.synchronize()
    dset, _ = ctx.batch_desc_set()
    ints = dset.count_stride
    node_rows = torch.as_tensor(DeviceInts(dset.d_counts, (n - 1) * ints + 1), device=dev)[::ints].cpu().numpy()
    want = restated_link(node_rows, cap, sel[3].cpu().numpy(), sel[0].cpu().numpy().view(B.DMATCH).reshape(-1))
    wrote = want[0] != SENT32
    got = [t.cpu().numpy() for t in (prev, track, age, summary)]
    identical = all(np.array_equal(g[wrote], w[wrote]) for g, w in zip(got[:3], want[:3])) and got[3].tolist() == want[3].tolist()
    wl = restated_list(node_rows, cap, *want[:3], 3, tcap, ocap)
    gl = [t.cpu().numpy() for t in lists]
    stored, sobs = int(wl[4][2]), int(wl[2][-1])
    identical = bool(identical and gl[4].tolist() == wl[4].tolist() and gl[0][:stored].tobytes() == wl[0].tobytes() and
                     gl[1][:stored].tobytes() == wl[1].tobytes() and gl[2][:stored + 1].tobytes() == wl[2].tobytes() and
                     gl[3][:sobs].tobytes() == wl[3].tobytes())
    lens = wl[1]

    call_ms = {"link": [], "list": []}
    for _ in range(max(a.repeats, 5)):
        run_t(timed=True)
        torch.cuda.synchronize()
        call_ms["link"].append(ev[0].elapsed_time(ev[1]))
        call_ms["list"].append(ev[1].elapsed_time(ev[2]))

    fps = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                runs[v]()
                calls += 1
                if time.perf_counter() - t0 >= a.window:
                    break
            torch.cuda.synchronize()
            fps[v].append(calls * n / (time.perf_counter() - t0))
    med = {v: float(np.median(fps[v])) for v in order}
    ms = {v: 1e3 * n / med[v] for v in order}
    spread = {v: (max(fps[v]) - min(fps[v])) / med[v] for v in order}
    res = {
        "workload": "bench.py's stream: %dx%d, threshold %d, %d octaves, %d frames per batch (%d distinct) in HBM; frame-to-previous-frame, "
                    "k = %d, rows_cap %d, ratio 0.8, one match per row; tracks of min_len 3, tracks_cap %d, obs_cap %d"
                    % (W, H, THRESHOLD, OCTAVES, n, nd, k, cap, tcap, ocap),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window, "order": ", ".join(order) + " alternating; every window ends in a synchronise"},
        "frames_per_s": {v: round(med[v], 1) for v in order},
        "frames_per_s_all": {v: [round(x, 1) for x in fps[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "ms_per_batch": {v: round(ms[v], 4) for v in order},
        "tracking_ms_per_batch": {"T_minus_B": round(ms["T"] - ms["B"], 4)},
        "T_over_B_frames_per_s": round(med["T"] / med["B"], 4),
        "hip_event_ms": {"link_call_6_launches": {"median": round(float(np.median(call_ms["link"])), 4), "all": [round(x, 4) for x in call_ms["link"]]},
                         "list_call_6_launches": {"median": round(float(np.median(call_ms["list"])), 4), "all": [round(x, 4) for x in call_ms["list"]]}},
        "chain_walk": "a walk from each head along the forward pointers (the only form built): nodes - 1 = %d dependent loads on the longest "
                      "possible track" % (n - 1),
        "per_batch": {"nodes": n, "observations": int(want[3][5]), "tracks_started": int(want[3][1]), "links": int(want[3][2]),
                      "proposals_lost": int(want[3][3]), "records_ignored": int(want[3][4]), "tracks_listed_min_len_3": int(wl[4][0]),
                      "their_observations": int(wl[4][1]), "longest_track": int(lens.max()) if len(lens) else 0,
                      "list_cut": bool(wl[4][3])},
        "T_equals_the_restated_rule": identical,
        "legend": {"B": "detect_describe_batch + brisk_hip_match_knn_pairs_device + brisk_hip_select_pair_matches_device on one stream",
                   "T": "B + brisk_hip_link_tracks_device + brisk_hip_list_tracks_device on the same stream"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ext.close()
    ctx.close()


def verify_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b0, epipolar=False):
    """--verify: windows T and V; --epipolar: windows T and E, the same with the epipolar call (see the module's text); writes a.out"""
    from test_abi_epipolar import restated_epipolar
    from test_abi_verify import restated_verify
    win = "E" if epipolar else "V"
    entry = "brisk_hip_verify_pair_matches_epipolar_device" if epipolar else "brisk_hip_verify_pair_matches_device"
    restated, model_dtype = (restated_epipolar, B.PAIR_EPIPOLAR_MODEL) if epipolar else (restated_verify, B.PAIR_MODEL)
    st = work.cuda_stream
    select = B.MatchSelect(float("inf"), 0.8, 1)
    verify = B.PairVerify(a.max_error, a.hypotheses, a.min_inliers, 1, 2024)
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    L, h = ctx._L, ctx._h
    mcap = (n - 1) * cap                                            # (one match per row at the most)

    def lists_of():
        return (torch.zeros((mcap, 4), dtype=torch.int32, device=dev), torch.zeros(n - 1, dtype=torch.int32, device=dev),
                torch.zeros(n - 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))

    sel, ver = lists_of(), lists_of()
    models = torch.zeros((n - 1, 12), dtype=torch.int64, device=dev)
    prev, age = (torch.zeros((n, cap), dtype=torch.int32, device=dev) for _ in range(2))
    track = torch.zeros((n, cap), dtype=torch.int64, device=dev)
    summary = torch.zeros(8, dtype=torch.int64, device=dev)
    tcap, ocap = n * cap // 4, n * cap
    lists = (torch.zeros(tcap, dtype=torch.int64, device=dev), torch.zeros(tcap, dtype=torch.int32, device=dev),
             torch.zeros(tcap + 1, dtype=torch.int64, device=dev), torch.zeros((ocap, 2), dtype=torch.int32, device=dev),
             torch.zeros(4, dtype=torch.int64, device=dev))
    seed = B.TrackSeed(None, None, 0, summary.data_ptr())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    m, cnt, rows = outs["B"]

    def run(verified, timed=False, call=None):
        run_b0()
        ctx.check(L.brisk_hip_select_pair_matches_device(h, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), n - 1, cap, k, C.byref(select), mcap,
                                                         sel[1].data_ptr(), sel[2].data_ptr(), sel[3].data_ptr(), sel[0].data_ptr(), st))
        dset, _ = ctx.batch_desc_set()
        src = sel
        if verified:
            kps = ctx.batch_kp_set()
            if timed:
                ev[0].record(work)
            ctx.check(getattr(L, call or entry)(h, C.byref(dset), C.byref(dset), C.byref(kps), C.byref(kps), C.byref(spec), cap,
                                                sel[3].data_ptr(), sel[0].data_ptr(), mcap, C.byref(verify), mcap, models.data_ptr(),
                                                ver[1].data_ptr(), ver[2].data_ptr(), ver[3].data_ptr(), ver[0].data_ptr(), st))
            if timed:
                ev[1].record(work)
            src = ver
        ptr, stride = ctx._node_rows((dset, 0, 1))
        ctx.check(L.brisk_hip_link_tracks_device(h, ptr, stride, n, cap, src[3].data_ptr(), src[0].data_ptr(), C.byref(seed), prev.data_ptr(),
                                                 track.data_ptr(), age.data_ptr(), summary.data_ptr(), st))
        ctx.check(L.brisk_hip_list_tracks_device(h, ptr, stride, n, cap, prev.data_ptr(), track.data_ptr(), age.data_ptr(), 3, tcap, ocap,
                                                 lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(), lists[3].data_ptr(),
                                                 lists[4].data_ptr(), st))

    runs = {"T": lambda: run(False), win: lambda: run(True)}
    order = "T" + win
    for v in order + order:                                         # warm-up: buffers sized, scratch grown
        runs[v]()
        torch.cuda.synchronize()
    if a.stats_pass:
        for _ in range(8):
            runs[win]()
            if epipolar:                                            # k_verify_ransac beside k_epipolar_ransac, on the same lists
                run(True, call="brisk_hip_verify_pair_matches_device")
        torch.cuda.synchronize()
        return

    # one batch against the restatement of the rule on its downloaded lists and keypoints
    runs[win]()
    torch.cuda.synchronize()
    dset, dim = ctx.batch_desc_set()
    ints = dset.count_stride
    node_rows = torch.as_tensor(DeviceInts(dset.d_counts, (n - 1) * ints + 1), device=dev)[::ints].cpu().numpy()
    xy = []
    for f in range(n):
        kp = ctx.batch_download(f, True, strings=dim)[0]
        xy.append(np.stack([kp["x"], kp["y"]], axis=1).astype(np.float32).reshape(-1, 2))
    so, sm = sel[3].cpu().numpy(), sel[0].cpu().numpy().view(B.DMATCH).reshape(-1)
    want = restated([(p + 1, p) for p in range(n - 1)], node_rows, node_rows, cap, xy, xy, so, sm[:int(so[-1])],
                    (a.max_error, a.hypotheses, a.min_inliers, 1, 2024), mcap, mcap)
    got_models = models.cpu().numpy().reshape(-1).view(model_dtype)
    stored = int(want[3][-1])
    identical = bool(got_models.tobytes() == want[0].tobytes() and ver[1].cpu().numpy().tobytes() == want[1].tobytes() and
                     ver[2].cpu().numpy().tobytes() == want[2].tobytes() and ver[3].cpu().numpy().tobytes() == want[3].tobytes() and
                     ver[0].cpu().numpy()[:stored].tobytes() == want[4].tobytes())

    call_ms = []
    for _ in range(max(a.repeats, 5)):
        run(True, timed=True)
        torch.cuda.synchronize()
        call_ms.append(ev[0].elapsed_time(ev[1]))

    fps = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                runs[v]()
                calls += 1
                if time.perf_counter() - t0 >= a.window:
                    break
            torch.cuda.synchronize()
            fps[v].append(calls * n / (time.perf_counter() - t0))
    med = {v: float(np.median(fps[v])) for v in order}
    ms = {v: 1e3 * n / med[v] for v in order}
    spread = {v: (max(fps[v]) - min(fps[v])) / med[v] for v in order}
    mod = want[0]
    res = {
        "workload": "bench.py's stream: %dx%d, threshold %d, %d octaves, %d frames per batch (%d distinct) in HBM; frame-to-previous-frame, "
                    "k = %d, rows_cap %d, ratio 0.8, one match per row; %s: %d hypotheses, max_error %g, min_inliers %d, "
                    "keep_unverified 1; tracks of min_len 3" % (W, H, THRESHOLD, OCTAVES, n, nd, k, cap, "epipolar verify" if epipolar else "verify",
                                                                a.hypotheses, a.max_error, a.min_inliers),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window, "order": ", ".join(order) + " alternating; every window ends in a synchronise"},
        "frames_per_s": {v: round(med[v], 1) for v in order},
        "frames_per_s_all": {v: [round(x, 1) for x in fps[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "ms_per_batch": {v: round(ms[v], 4) for v in order},
        "verify_ms_per_batch": {win + "_minus_T": round(ms[win] - ms["T"], 4)},
        win + "_over_T_frames_per_s": round(med[win] / med["T"], 4),
        "hip_event_ms": {"verify_call_3_launches": {"median": round(float(np.median(call_ms)), 4), "all": [round(x, 4) for x in call_ms]}},
        "per_batch": {"pairs": n - 1, "hypotheses": a.hypotheses, "records_per_pair_mean": round(float(mod["records"].mean()), 2),
                      "records_per_pair_max": int(mod["records"].max()), "usable_per_pair_mean": round(float(mod["usable"].mean()), 2),
                      "kept_per_pair_mean": round(float(want[1].mean()), 2), "pairs_with_a_model": int((mod["flags"] & B.PAIR_NO_MODEL == 0).sum()),
                      "inliers_per_model_mean": round(float(mod["inliers"][mod["flags"] & B.PAIR_NO_MODEL == 0].mean()), 2)
                      if (mod["flags"] & B.PAIR_NO_MODEL == 0).any() else 0.0},
        win + "_equals_the_restated_rule": identical,
        "legend": {"T": "detect_describe_batch + match_knn_pairs + select + brisk_hip_link_tracks_device + brisk_hip_list_tracks_device on one stream",
                   win: "T with %s between select and link" % entry},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ext.close()
    ctx.close()


def related_batch(dev, npairs, rows, per_pair, noise, seed=2024):
    """a batch whose consecutive frames ARE related: `rows` points seen by npairs + 1 frames, each through a mild homography of its own
    with Gaussian noise of `noise` px; pair p = (frame p + 1, frame p) has per_pair records, three quarters of them true.  Returns
    (DescSet - the counts only -, KpSet, offsets, matches, the tensors that must stay alive)."""
    rng = np.random.default_rng(seed)
    nf = npairs + 1
    base = np.stack([rng.uniform(20, 1900, rows), rng.uniform(20, 1060, rows)], axis=1)
    kps = np.zeros((nf, rows), B.KEYPOINT)
    for f in range(nf):
        a_ = float(rng.uniform(-0.05, 0.05))
        Hm = np.array([[np.cos(a_), -np.sin(a_), rng.uniform(-20, 20)], [np.sin(a_), np.cos(a_), rng.uniform(-20, 20)],
                       [rng.uniform(-2e-5, 2e-5), rng.uniform(-2e-5, 2e-5), 1.0]])
        w = Hm[2, 0] * base[:, 0] + Hm[2, 1] * base[:, 1] + Hm[2, 2]
        kps["x"][f] = ((Hm[0, 0] * base[:, 0] + Hm[0, 1] * base[:, 1] + Hm[0, 2]) / w + rng.normal(0, noise, rows)).astype(np.float32)
        kps["y"][f] = ((Hm[1, 0] * base[:, 0] + Hm[1, 1] * base[:, 1] + Hm[1, 2]) / w + rng.normal(0, noise, rows)).astype(np.float32)
    rec = np.zeros((npairs, per_pair), B.DMATCH)
    q = np.sort(rng.integers(0, rows, (npairs, per_pair)), axis=1)
    rec["queryIdx"] = q
    rec["trainIdx"] = np.where(rng.random((npairs, per_pair)) < 0.75, q, rng.integers(0, rows, (npairs, per_pair)))
    rec["distance"] = rng.integers(0, 90, (npairs, per_pair))
    d_counts = torch.full((nf,), rows, dtype=torch.int32, device=dev)
    d_kps = torch.from_numpy(kps.view(np.int32).reshape(nf, rows, 7).copy()).to(dev)
    d_off = torch.arange(npairs + 1, dtype=torch.int64, device=dev) * per_pair
    d_rec = torch.from_numpy(rec.view(np.int32).reshape(-1, 4).copy()).to(dev)
    return (B.DescSet(None, d_counts.data_ptr(), 1, 0, 0, nf), B.KpSet(d_kps.data_ptr(), rows * 28), d_off, d_rec, (d_counts, d_kps),
            [np.stack([kps["x"][f], kps["y"][f]], axis=1) for f in range(nf)], rec.reshape(-1))


def epirefit_mode(a, dev):
    """--epirefit: windows H and F (see the module's text); writes a.out"""
    from test_abi_epipolar_refit import restated_epipolar_refit
    ctx = B.Context(0)
    work = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(work)
    st = work.cuda_stream
    L, h = ctx._L, ctx._h
    min_inl = max(a.min_inliers, 8)
    verify = B.PairVerify(a.max_error, a.hypotheses, min_inl, 1, 2024)
    refit_h = B.PairRefit(a.max_error, a.rounds, min_inl, 1)
    refit_f = B.PairEpipolarRefit(a.max_error, a.rounds, min_inl, 1, a.rank2)
    rp, rrows, rper = a.batch - 1, 1024, a.related_records
    rset, rkps, roff, rrec, keep_alive, rxy, rhost = related_batch(dev, rp, rrows, rper, 0.5)
    rspec = B.PairSpec(rp, 1, 1, 0, 1, None)
    rcap = rp * rper

    def arrays():
        return (torch.zeros((rcap, 4), dtype=torch.int32, device=dev), torch.zeros(rp, dtype=torch.int32, device=dev),
                torch.zeros(rp, dtype=torch.int32, device=dev), torch.zeros(rp + 1, dtype=torch.int64, device=dev),
                torch.zeros((rp, 12), dtype=torch.int64, device=dev))

    ver = {"H": arrays(), "F": arrays()}
    out = {"H": arrays(), "F": arrays()}
    entry = {"H": (L.brisk_hip_verify_pair_matches_device, L.brisk_hip_refit_pair_models_device, refit_h),
             "F": (L.brisk_hip_verify_pair_matches_epipolar_device, L.brisk_hip_refit_pair_models_epipolar_device, refit_f)}
    for v in "HF":                                                  # the input models of either call: written once, read by every call
        ctx.check(entry[v][0](h, C.byref(rset), C.byref(rset), C.byref(rkps), C.byref(rkps), C.byref(rspec), rrows, roff.data_ptr(),
                              rrec.data_ptr(), rcap, C.byref(verify), rcap, ver[v][4].data_ptr(), ver[v][1].data_ptr(), ver[v][2].data_ptr(),
                              ver[v][3].data_ptr(), ver[v][0].data_ptr(), st))

    def call(v):
        o = out[v]
        ctx.check(entry[v][1](h, C.byref(rset), C.byref(rset), C.byref(rkps), C.byref(rkps), C.byref(rspec), rrows, roff.data_ptr(),
                              rrec.data_ptr(), rcap, ver[v][4].data_ptr(), C.byref(entry[v][2]), rcap, o[4].data_ptr(), o[1].data_ptr(),
                              o[2].data_ptr(), o[3].data_ptr(), o[0].data_ptr(), st))

    order = "HF"
    for v in order + order:                                         # warm-up: the scratch grown
        call(v)
    torch.cuda.synchronize()
    if a.stats_pass:
        for _ in range(10):
            for v in order:
                call(v)
        torch.cuda.synchronize()
        ctx.close()
        return
    # F against the restatement of the rule
    fm = ver["F"][4].cpu().numpy().reshape(-1).view(B.PAIR_EPIPOLAR_MODEL).copy()
    hm = ver["H"][4].cpu().numpy().reshape(-1).view(B.PAIR_MODEL).copy()
    counts_r = [rrows] * (rp + 1)
    want = restated_epipolar_refit([(p + 1, p) for p in range(rp)], counts_r, counts_r, rrows, rxy, rxy, roff.cpu().numpy(), rhost, fm,
                                   (a.max_error, a.rounds, min_inl, 1, a.rank2), rcap, rcap)
    o = out["F"]
    stored = int(want[3][-1])
    identical = bool(o[4].cpu().numpy().reshape(-1).view(B.PAIR_EPIPOLAR_MODEL).tobytes() == want[0].tobytes() and
                     o[1].cpu().numpy().tobytes() == want[1].tobytes() and o[2].cpu().numpy().tobytes() == want[2].tobytes() and
                     o[3].cpu().numpy().tobytes() == want[3].tobytes() and o[0].cpu().numpy()[:stored].tobytes() == want[4].tobytes())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    event_ms = {v: [] for v in order}
    for _ in range(max(a.repeats, 5)):
        for v in order:
            ev[0].record(work)
            call(v)
            ev[1].record(work)
            torch.cuda.synchronize()
            event_ms[v].append(ev[0].elapsed_time(ev[1]))
    ms = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                call(v)
                calls += 1
                if calls % 8 == 0:
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= a.window:
                        break
            torch.cuda.synchronize()
            ms[v].append(1e3 * (time.perf_counter() - t0) / calls)
    med = {v: float(np.median(ms[v])) for v in order}
    emed = {v: float(np.median(event_ms[v])) for v in order}
    spread = {v: (max(ms[v]) - min(ms[v])) / med[v] for v in order}
    hr = out["H"][4].cpu().numpy().reshape(-1).view(B.PAIR_MODEL)
    fr = want[0]
    has_h, has_f = (hm["flags"] & B.PAIR_NO_MODEL) == 0, (fm["flags"] & B.PAIR_NO_MODEL) == 0

    def side(vm, rm, has):
        return {"pairs_with_an_input_model": int(has.sum()), "pairs_refitted": int(((rm["flags"] & B.PAIR_REFIT) != 0).sum()),
                "inliers_per_model_mean_verifier": round(float(vm["inliers"][has].mean()), 2) if has.any() else 0.0,
                "inliers_per_model_mean_refit": round(float(rm["inliers"][has].mean()), 2) if has.any() else 0.0,
                "rounds_that_replaced_mean": round(float(rm["valid"][has].mean()), 2) if has.any() else 0.0}

    res = {
        "workload": "a related batch: %d pairs, %d points a frame on a plane seen through mild homographies with 0.5 px noise, %d records a pair, "
                    "three quarters of them true; both verifiers: %d hypotheses, max_error %g, min_inliers %d, keep_unverified 1; both refits: "
                    "%d rounds, rank2 %d, the same lists, one process" % (rp, rrows, rper, a.hypotheses, a.max_error, min_inl, a.rounds, a.rank2),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window,
                    "order": ", ".join(order) + " alternating; a window is back-to-back calls of ONE kind, synchronised every 8 calls and at its end"},
        "ms_per_call": {v: round(med[v], 4) for v in order},
        "ms_per_call_all": {v: [round(x, 4) for x in ms[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "F_over_H_ms_per_call": round(med["F"] / med["H"], 4),
        "hip_event_ms": {v: {"median": round(emed[v], 4), "all": [round(x, 4) for x in event_ms[v]]} for v in order},
        "F_over_H_hip_event_ms": round(emed["F"] / emed["H"], 4),
        "related_batch": {"pairs": rp, "rows_per_frame": rrows, "records_per_pair": rper, "true_share": 0.75, "noise_px": 0.5,
                          "H": side(hm, hr, has_h), "F": side(fm, fr, has_f), "F_equals_the_restated_rule": identical},
        "legend": {"H": "brisk_hip_refit_pair_models_device on the homography verifier's models (three launches): the yardstick",
                   "F": "brisk_hip_refit_pair_models_epipolar_device on the epipolar verifier's models (three launches)"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ctx.close()


def refit_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b0):
    """--refit: windows V and R (see the module's text); writes a.out"""
    from test_abi_refit import restated_refit
    st = work.cuda_stream
    select = B.MatchSelect(float("inf"), 0.8, 1)
    verify = B.PairVerify(a.max_error, a.hypotheses, a.min_inliers, 1, 2024)
    refit = B.PairRefit(a.max_error, a.rounds, a.min_inliers, 1)
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    L, h = ctx._L, ctx._h
    mcap = (n - 1) * cap                                            # (one match per row at the most)

    def lists_of():
        return (torch.zeros((mcap, 4), dtype=torch.int32, device=dev), torch.zeros(n - 1, dtype=torch.int32, device=dev),
                torch.zeros(n - 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))

    sel, ver, ref = lists_of(), lists_of(), lists_of()
    models = torch.zeros((n - 1, 12), dtype=torch.int64, device=dev)
    prev, age = (torch.zeros((n, cap), dtype=torch.int32, device=dev) for _ in range(2))
    track = torch.zeros((n, cap), dtype=torch.int64, device=dev)
    summary = torch.zeros(8, dtype=torch.int64, device=dev)
    tcap, ocap = n * cap // 4, n * cap
    lists = (torch.zeros(tcap, dtype=torch.int64, device=dev), torch.zeros(tcap, dtype=torch.int32, device=dev),
             torch.zeros(tcap + 1, dtype=torch.int64, device=dev), torch.zeros((ocap, 2), dtype=torch.int32, device=dev),
             torch.zeros(4, dtype=torch.int64, device=dev))
    seed = B.TrackSeed(None, None, 0, summary.data_ptr())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    m, cnt, rows = outs["B"]

    def run(refitted, timed=False):
        run_b0()
        ctx.check(L.brisk_hip_select_pair_matches_device(h, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), n - 1, cap, k, C.byref(select), mcap,
                                                         sel[1].data_ptr(), sel[2].data_ptr(), sel[3].data_ptr(), sel[0].data_ptr(), st))
        dset, _ = ctx.batch_desc_set()
        kps = ctx.batch_kp_set()
        ctx.check(L.brisk_hip_verify_pair_matches_device(h, C.byref(dset), C.byref(dset), C.byref(kps), C.byref(kps), C.byref(spec), cap,
                                                         sel[3].data_ptr(), sel[0].data_ptr(), mcap, C.byref(verify), mcap, models.data_ptr(),
                                                         ver[1].data_ptr(), ver[2].data_ptr(), ver[3].data_ptr(), ver[0].data_ptr(), st))
        src = ver
        if refitted:                                                # the models in place
            if timed:
                ev[0].record(work)
            ctx.check(L.brisk_hip_refit_pair_models_device(h, C.byref(dset), C.byref(dset), C.byref(kps), C.byref(kps), C.byref(spec), cap,
                                                           sel[3].data_ptr(), sel[0].data_ptr(), mcap, models.data_ptr(), C.byref(refit), mcap,
                                                           models.data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ref[3].data_ptr(),
                                                           ref[0].data_ptr(), st))
            if timed:
                ev[1].record(work)
            src = ref
        ptr, stride = ctx._node_rows((dset, 0, 1))
        ctx.check(L.brisk_hip_link_tracks_device(h, ptr, stride, n, cap, src[3].data_ptr(), src[0].data_ptr(), C.byref(seed), prev.data_ptr(),
                                                 track.data_ptr(), age.data_ptr(), summary.data_ptr(), st))
        ctx.check(L.brisk_hip_list_tracks_device(h, ptr, stride, n, cap, prev.data_ptr(), track.data_ptr(), age.data_ptr(), 3, tcap, ocap,
                                                 lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(), lists[3].data_ptr(),
                                                 lists[4].data_ptr(), st))

    # the related batch: the stream's consecutive frames are unrelated (no pair has a model there, as with --guided), so the kernel's
    # own time is taken on pairs that have one
    rp, rrows, rper = n - 1, 1024, a.related_records
    rset, rkps, roff, rrec, keep_alive, rxy, rhost = related_batch(dev, rp, rrows, rper, 0.5)
    rspec = B.PairSpec(rp, 1, 1, 0, 1, None)
    rcap = rp * rper
    rmodels = torch.zeros((rp, 12), dtype=torch.int64, device=dev)
    rver, rref = [(torch.zeros((rcap, 4), dtype=torch.int32, device=dev), torch.zeros(rp, dtype=torch.int32, device=dev),
                   torch.zeros(rp, dtype=torch.int32, device=dev), torch.zeros(rp + 1, dtype=torch.int64, device=dev)) for _ in range(2)]
    rout = torch.zeros((rp, 12), dtype=torch.int64, device=dev)

    def run_related(timed=False):
        ctx.check(L.brisk_hip_verify_pair_matches_device(h, C.byref(rset), C.byref(rset), C.byref(rkps), C.byref(rkps), C.byref(rspec), rrows,
                                                         roff.data_ptr(), rrec.data_ptr(), rcap, C.byref(verify), rcap, rmodels.data_ptr(),
                                                         rver[1].data_ptr(), rver[2].data_ptr(), rver[3].data_ptr(), rver[0].data_ptr(), st))
        if timed:
            ev[0].record(work)
        ctx.check(L.brisk_hip_refit_pair_models_device(h, C.byref(rset), C.byref(rset), C.byref(rkps), C.byref(rkps), C.byref(rspec), rrows,
                                                       roff.data_ptr(), rrec.data_ptr(), rcap, rmodels.data_ptr(), C.byref(refit), rcap,
                                                       rout.data_ptr(), rref[1].data_ptr(), rref[2].data_ptr(), rref[3].data_ptr(),
                                                       rref[0].data_ptr(), st))
        if timed:
            ev[1].record(work)

    if a.stats_pass:                                                # (the related batch only: every launch of k_refit_models in the trace has models to fit)
        for _ in range(10):
            run_related()
        torch.cuda.synchronize()
        return
    runs = {"V": lambda: run(False), "R": lambda: run(True)}
    order = "VR"
    for v in order + "VR":                                          # warm-up: buffers sized, scratch grown
        runs[v]()
        torch.cuda.synchronize()
    run_related()
    torch.cuda.synchronize()

    # the related batch against the restatement of the rule
    vm = rmodels.cpu().numpy().reshape(-1).view(B.PAIR_MODEL).copy()
    counts_r = [rrows] * (rp + 1)
    want = restated_refit([(p + 1, p) for p in range(rp)], counts_r, counts_r, rrows, rxy, rxy, roff.cpu().numpy(), rhost, vm,
                          (a.max_error, a.rounds, a.min_inliers, 1), rcap, rcap)
    stored = int(want[3][-1])
    identical = bool(rout.cpu().numpy().reshape(-1).view(B.PAIR_MODEL).tobytes() == want[0].tobytes() and
                     rref[1].cpu().numpy().tobytes() == want[1].tobytes() and rref[2].cpu().numpy().tobytes() == want[2].tobytes() and
                     rref[3].cpu().numpy().tobytes() == want[3].tobytes() and rref[0].cpu().numpy()[:stored].tobytes() == want[4].tobytes())
    related_ms, call_ms = [], []
    for _ in range(max(a.repeats, 5)):
        run_related(timed=True)
        torch.cuda.synchronize()
        related_ms.append(ev[0].elapsed_time(ev[1]))
    for _ in range(max(a.repeats, 5)):
        run(True, timed=True)
        torch.cuda.synchronize()
        call_ms.append(ev[0].elapsed_time(ev[1]))
    stream_models = models.cpu().numpy().reshape(-1).view(B.PAIR_MODEL)

    fps = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                runs[v]()
                calls += 1
                if time.perf_counter() - t0 >= a.window:
                    break
            torch.cuda.synchronize()
            fps[v].append(calls * n / (time.perf_counter() - t0))
    med = {v: float(np.median(fps[v])) for v in order}
    ms = {v: 1e3 * n / med[v] for v in order}
    spread = {v: (max(fps[v]) - min(fps[v])) / med[v] for v in order}
    rm = want[0]
    has = (rm["flags"] & B.PAIR_NO_MODEL) == 0
    res = {
        "workload": "bench.py's stream: %dx%d, threshold %d, %d octaves, %d frames per batch (%d distinct) in HBM; frame-to-previous-frame, "
                    "k = %d, rows_cap %d, ratio 0.8, one match per row; verify: %d hypotheses, max_error %g, min_inliers %d, "
                    "keep_unverified 1; refit: %d rounds, the models in place; tracks of min_len 3" %
                    (W, H, THRESHOLD, OCTAVES, n, nd, k, cap, a.hypotheses, a.max_error, a.min_inliers, a.rounds),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window, "order": ", ".join(order) + " alternating; every window ends in a synchronise"},
        "frames_per_s": {v: round(med[v], 1) for v in order},
        "frames_per_s_all": {v: [round(x, 1) for x in fps[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "ms_per_batch": {v: round(ms[v], 4) for v in order},
        "refit_ms_per_batch": {"R_minus_V": round(ms["R"] - ms["V"], 4)},
        "R_over_V_frames_per_s": round(med["R"] / med["V"], 4),
        "hip_event_ms": {"refit_call_3_launches_stream": {"median": round(float(np.median(call_ms)), 4), "all": [round(x, 4) for x in call_ms]},
                         "refit_call_3_launches_related_batch": {"median": round(float(np.median(related_ms)), 4),
                                                                 "all": [round(x, 4) for x in related_ms]}},
        "stream_per_batch": {"pairs": n - 1, "pairs_with_an_input_model": int(((stream_models["hypothesis"] >= 0) &
                                                                               ((stream_models["flags"] & B.PAIR_NO_MODEL) == 0)).sum()),
                             "note": "the stream's consecutive frames are unrelated: no pair has a model, as with --guided; the call then "
                                     "costs its launches and one sweep over the records"},
        "related_batch": {"pairs": rp, "rows_per_frame": rrows, "records_per_pair": rper, "true_share": 0.75, "noise_px": 0.5,
                          "pairs_with_a_model": int(has.sum()), "pairs_refitted": int(((rm["flags"] & B.PAIR_REFIT) != 0).sum()),
                          "inliers_per_model_mean_verifier": round(float(vm["inliers"][has].mean()), 2) if has.any() else 0.0,
                          "inliers_per_model_mean_refit": round(float(rm["inliers"][has].mean()), 2) if has.any() else 0.0,
                          "rounds_that_replaced_mean": round(float(rm["valid"][has].mean()), 2) if has.any() else 0.0,
                          "equals_the_restated_rule": identical},
        "legend": {"V": "detect_describe_batch + match_knn_pairs + select + brisk_hip_verify_pair_matches_device + link + list on one stream",
                   "R": "V with brisk_hip_refit_pair_models_device between verify and link (the linker reads the refit's lists)"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ext.close()
    ctx.close()


def guided_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b0):
    """--guided: windows V and G (see the module's text); writes a.out"""
    from test_abi_match_guided import restated_centres
    st = work.cuda_stream
    select = B.MatchSelect(float("inf"), 0.8, 1)
    reselect = B.MatchSelect(float("inf"), 0.0, 1)                  # the guided lists: the distance bound only, one entry per row
    verify = B.PairVerify(a.max_error, a.hypotheses, a.min_inliers, 1, 2024)
    radius, octaves = 6.0, 1
    guide = B.MatchGuide.around(radius, max_octave_diff=octaves, fallback=0)
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    L, h = ctx._L, ctx._h
    mcap = (n - 1) * cap                                            # (one match per row at the most)

    def lists_of():
        return (torch.zeros((mcap, 4), dtype=torch.int32, device=dev), torch.zeros(n - 1, dtype=torch.int32, device=dev),
                torch.zeros(n - 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))

    def link_of():
        return (torch.zeros((n, cap), dtype=torch.int32, device=dev), torch.zeros((n, cap), dtype=torch.int64, device=dev),
                torch.zeros((n, cap), dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int64, device=dev))

    sel, ver, gsel = lists_of(), lists_of(), lists_of()
    models = torch.zeros((n - 1, 12), dtype=torch.int64, device=dev)
    link_v, link_g = link_of(), link_of()
    tcap, ocap = n * cap // 4, n * cap
    lists = (torch.zeros(tcap, dtype=torch.int64, device=dev), torch.zeros(tcap, dtype=torch.int32, device=dev),
             torch.zeros(tcap + 1, dtype=torch.int64, device=dev), torch.zeros((ocap, 2), dtype=torch.int32, device=dev),
             torch.zeros(4, dtype=torch.int64, device=dev))
    seeds = {id(lk): B.TrackSeed(None, None, 0, lk[3].data_ptr()) for lk in (link_v, link_g)}   # numbered on from the call before
    guided = (torch.zeros((n - 1, cap, 1, 4), dtype=torch.int32, device=dev), torch.zeros((n - 1, cap), dtype=torch.int32, device=dev),
              torch.zeros(n - 1, dtype=torch.int32, device=dev))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    m, cnt, rows = outs["B"]

    def link(dset, src, lk):
        ptr, stride = ctx._node_rows((dset, 0, 1))
        ctx.check(L.brisk_hip_link_tracks_device(h, ptr, stride, n, cap, src[3].data_ptr(), src[0].data_ptr(), C.byref(seeds[id(lk)]),
                                                 lk[0].data_ptr(), lk[1].data_ptr(), lk[2].data_ptr(), lk[3].data_ptr(), st))
        return ptr, stride

    def run_v():
        run_b0()
        ctx.check(L.brisk_hip_select_pair_matches_device(h, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), n - 1, cap, k, C.byref(select), mcap,
                                                         sel[1].data_ptr(), sel[2].data_ptr(), sel[3].data_ptr(), sel[0].data_ptr(), st))
        dset, dim = ctx.batch_desc_set()
        kps = ctx.batch_kp_set()
        ctx.check(L.brisk_hip_verify_pair_matches_device(h, C.byref(dset), C.byref(dset), C.byref(kps), C.byref(kps), C.byref(spec), cap,
                                                         sel[3].data_ptr(), sel[0].data_ptr(), mcap, C.byref(verify), mcap, models.data_ptr(),
                                                         ver[1].data_ptr(), ver[2].data_ptr(), ver[3].data_ptr(), ver[0].data_ptr(), st))
        ptr, stride = link(dset, ver, link_v)
        ctx.check(L.brisk_hip_list_tracks_device(h, ptr, stride, n, cap, link_v[0].data_ptr(), link_v[1].data_ptr(), link_v[2].data_ptr(), 3,
                                                 tcap, ocap, lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(), lists[3].data_ptr(),
                                                 lists[4].data_ptr(), st))
        return dset, dim, kps

    def run_g(timed=False):
        dset, dim, kps = run_v()
        if timed:
            ev[0].record(work)
        ctx.check(L.brisk_hip_match_knn_pairs_guided_device(h, C.byref(dset), C.byref(dset), C.byref(kps), C.byref(kps), C.byref(spec),
                                                            models.data_ptr(), C.byref(guide), dim, 1, cap, guided[0].data_ptr(),
                                                            guided[1].data_ptr(), guided[2].data_ptr(), st))
        if timed:
            ev[1].record(work)
        ctx.check(L.brisk_hip_select_pair_matches_device(h, guided[0].data_ptr(), guided[1].data_ptr(), guided[2].data_ptr(), n - 1, cap, 1,
                                                         C.byref(reselect), mcap, gsel[1].data_ptr(), gsel[2].data_ptr(), gsel[3].data_ptr(),
                                                         gsel[0].data_ptr(), st))
        link(dset, gsel, link_g)

    identity = np.zeros(n - 1, B.PAIR_MODEL)
    identity["h"] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    identity = torch.from_numpy(identity.view(np.int64).reshape(n - 1, 12).copy()).to(dev)

    def run_yardstick():
        """the kernel trace's pair: the guided k-NN call with EVERY pair guided (identity models: the gated call's mask, so the same
        rows pass) and the gated k-NN call at the same window, k and shapes - the guided kernel's yardstick"""
        dset, dim = ctx.batch_desc_set()
        kps = ctx.batch_kp_set()
        ctx.match_knn_pairs_guided(dset, dset, spec, 1, identity, guide, rows_cap=cap, query_kps=kps, train_kps=kps, stream=st, dim_bytes=dim,
                                   out=guided)
        ctx.match_knn_pairs(dset, dset, spec, 1, rows_cap=cap, stream=st, dim_bytes=dim, out=guided, gate=guide.window, query_kps=kps,
                            train_kps=kps)

    runs = {"V": run_v, "G": run_g}
    order = "VG"
    if a.stats_pass:                                                # (no G: every launch of the guided kernel in the trace is the yardstick's)
        for _ in range(2 + 8):
            run_v()
            run_yardstick()
            torch.cuda.synchronize()
        return
    for v in order + "VG":                                          # warm-up: buffers sized, scratch grown
        runs[v]()
        torch.cuda.synchronize()

    # one batch: what reaches the linker and what it makes of it, in V and in G; every guided record inside its window
    run_g()
    torch.cuda.synchronize()
    dset, dim = ctx.batch_desc_set()
    mod = models.cpu().numpy().reshape(-1).view(B.PAIR_MODEL)
    has_model = (mod["hypothesis"] >= 0) & ((mod["flags"] & (B.PAIR_NO_MODEL | B.PAIR_BAD)) == 0)
    vcounts, gcounts = ver[1].cpu().numpy(), gsel[1].cpu().numpy()
    sum_v, sum_g = link_v[3].cpu().numpy(), link_g[3].cpu().numpy()
    goffs, grec = gsel[3].cpu().numpy(), gsel[0].cpu().numpy().view(B.DMATCH).reshape(-1)
    kps = [ctx.batch_download(f, True, strings=dim)[0] for f in range(n)]
    inside = True
    for p in range(n - 1):
        rec = grec[int(goffs[p]):int(goffs[p + 1])]
        if not has_model[p]:
            inside = inside and len(rec) == 0
            continue
        kq, kt = kps[p + 1][rec["queryIdx"]], kps[p][rec["trainIdx"]]
        cx, cy, has = restated_centres(mod["h"][p], mod["hypothesis"][p], mod["flags"][p], 0, kq["x"], kq["y"])
        inside = bool(inside and has.all() and (np.abs(kt["x"] - cx) <= np.float32(radius)).all() and
                      (np.abs(kt["y"] - cy) <= np.float32(radius)).all() and (np.abs(kt["octave"] - kq["octave"]) <= octaves).all())

    call_ms = []
    for _ in range(max(a.repeats, 5)):
        run_g(timed=True)
        torch.cuda.synchronize()
        call_ms.append(ev[0].elapsed_time(ev[1]))

    fps = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                runs[v]()
                calls += 1
                if time.perf_counter() - t0 >= a.window:
                    break
            torch.cuda.synchronize()
            fps[v].append(calls * n / (time.perf_counter() - t0))
    med = {v: float(np.median(fps[v])) for v in order}
    ms = {v: 1e3 * n / med[v] for v in order}
    spread = {v: (max(fps[v]) - min(fps[v])) / med[v] for v in order}
    res = {
        "workload": "bench.py's stream: %dx%d, threshold %d, %d octaves, %d frames per batch (%d distinct) in HBM; frame-to-previous-frame, "
                    "k = %d, rows_cap %d, ratio 0.8, one match per row; verify: %d hypotheses, max_error %g, min_inliers %d, "
                    "keep_unverified 1; guided: k = 1, window +-%g px, octave difference %d, fallback 0, then keep 1 without a ratio; "
                    "tracks of min_len 3" % (W, H, THRESHOLD, OCTAVES, n, nd, k, cap, a.hypotheses, a.max_error, a.min_inliers, radius, octaves),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window, "order": ", ".join(order) + " alternating; every window ends in a synchronise"},
        "frames_per_s": {v: round(med[v], 1) for v in order},
        "frames_per_s_all": {v: [round(x, 1) for x in fps[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "ms_per_batch": {v: round(ms[v], 4) for v in order},
        "guided_ms_per_batch": {"G_minus_V": round(ms["G"] - ms["V"], 4)},
        "G_over_V_frames_per_s": round(med["G"] / med["V"], 4),
        "hip_event_ms": {"guided_call_1_launch": {"median": round(float(np.median(call_ms)), 4), "all": [round(x, 4) for x in call_ms]}},
        "per_batch": {"pairs": n - 1, "pairs_with_a_model": int(has_model.sum()),
                      "records_per_pair_to_the_linker": {"V": round(float(vcounts.mean()), 2), "G": round(float(gcounts.mean()), 2)},
                      "links": {"V": int(sum_v[2]), "G": int(sum_g[2])},
                      "proposals_lost": {"V": int(sum_v[3]), "G": int(sum_g[3])}},
        "G_records_inside_their_windows": inside,
        "legend": {"V": "detect_describe_batch + match_knn_pairs + select + brisk_hip_verify_pair_matches_device + link + list on one stream",
                   "G": "V + brisk_hip_match_knn_pairs_guided_device on the verifier's models + select (keep 1) + link on the guided lists"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ext.close()
    ctx.close()


def epiguided_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b0):
    """--epiguided: windows E and L (see the module's text); writes a.out"""
    from test_abi_epipolar import restated_inliers8
    st = work.cuda_stream
    select = B.MatchSelect(float("inf"), 0.8, 1)
    reselect = B.MatchSelect(float("inf"), 0.0, 1)                  # the second pass' lists: the distance bound only, one entry per row
    verify = B.PairVerify(a.max_error, a.hypotheses, a.min_inliers, 1, 2024)
    window_px, octaves = 64.0, 1
    guide = B.MatchEpipolarGuide.around(a.max_error, window=(-window_px, window_px, -window_px, window_px), max_octave_diff=octaves, fallback=0)
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    L, h = ctx._L, ctx._h
    mcap = (n - 1) * cap                                            # (one match per row at the most)

    def lists_of():
        return (torch.zeros((mcap, 4), dtype=torch.int32, device=dev), torch.zeros(n - 1, dtype=torch.int32, device=dev),
                torch.zeros(n - 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))

    def link_of():
        return (torch.zeros((n, cap), dtype=torch.int32, device=dev), torch.zeros((n, cap), dtype=torch.int64, device=dev),
                torch.zeros((n, cap), dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int64, device=dev))

    sel, ver, lsel = lists_of(), lists_of(), lists_of()
    models = torch.zeros((n - 1, 12), dtype=torch.int64, device=dev)
    link_e, link_l = link_of(), link_of()
    tcap, ocap = n * cap // 4, n * cap
    lists = (torch.zeros(tcap, dtype=torch.int64, device=dev), torch.zeros(tcap, dtype=torch.int32, device=dev),
             torch.zeros(tcap + 1, dtype=torch.int64, device=dev), torch.zeros((ocap, 2), dtype=torch.int32, device=dev),
             torch.zeros(4, dtype=torch.int64, device=dev))
    seeds = {id(lk): B.TrackSeed(None, None, 0, lk[3].data_ptr()) for lk in (link_e, link_l)}   # numbered on from the call before
    again = (torch.zeros((n - 1, cap, 1, 4), dtype=torch.int32, device=dev), torch.zeros((n - 1, cap), dtype=torch.int32, device=dev),
             torch.zeros(n - 1, dtype=torch.int32, device=dev))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    m, cnt, rows = outs["B"]

    def link(dset, src, lk):
        ptr, stride = ctx._node_rows((dset, 0, 1))
        ctx.check(L.brisk_hip_link_tracks_device(h, ptr, stride, n, cap, src[3].data_ptr(), src[0].data_ptr(), C.byref(seeds[id(lk)]),
                                                 lk[0].data_ptr(), lk[1].data_ptr(), lk[2].data_ptr(), lk[3].data_ptr(), st))
        return ptr, stride

    def run_e():
        run_b0()
        ctx.check(L.brisk_hip_select_pair_matches_device(h, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), n - 1, cap, k, C.byref(select), mcap,
                                                         sel[1].data_ptr(), sel[2].data_ptr(), sel[3].data_ptr(), sel[0].data_ptr(), st))
        dset, dim = ctx.batch_desc_set()
        kps = ctx.batch_kp_set()
        ctx.check(L.brisk_hip_verify_pair_matches_epipolar_device(h, C.byref(dset), C.byref(dset), C.byref(kps), C.byref(kps), C.byref(spec), cap,
                                                                  sel[3].data_ptr(), sel[0].data_ptr(), mcap, C.byref(verify), mcap,
                                                                  models.data_ptr(), ver[1].data_ptr(), ver[2].data_ptr(), ver[3].data_ptr(),
                                                                  ver[0].data_ptr(), st))
        ptr, stride = link(dset, ver, link_e)
        ctx.check(L.brisk_hip_list_tracks_device(h, ptr, stride, n, cap, link_e[0].data_ptr(), link_e[1].data_ptr(), link_e[2].data_ptr(), 3,
                                                 tcap, ocap, lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(), lists[3].data_ptr(),
                                                 lists[4].data_ptr(), st))
        return dset, dim, kps

    def run_l(timed=False):
        dset, dim, kps = run_e()
        if timed:
            ev[0].record(work)
        ctx.check(L.brisk_hip_match_knn_pairs_epipolar_guided_device(h, C.byref(dset), C.byref(dset), C.byref(kps), C.byref(kps), C.byref(spec),
                                                                     models.data_ptr(), C.byref(guide), dim, 1, cap, again[0].data_ptr(),
                                                                     again[1].data_ptr(), again[2].data_ptr(), st))
        if timed:
            ev[1].record(work)
        ctx.check(L.brisk_hip_select_pair_matches_device(h, again[0].data_ptr(), again[1].data_ptr(), again[2].data_ptr(), n - 1, cap, 1,
                                                         C.byref(reselect), mcap, lsel[1].data_ptr(), lsel[2].data_ptr(), lsel[3].data_ptr(),
                                                         lsel[0].data_ptr(), st))
        link(dset, lsel, link_l)

    rectified = np.zeros(n - 1, B.PAIR_EPIPOLAR_MODEL)
    rectified["f"] = (0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0)
    rectified = torch.from_numpy(rectified.view(np.int64).reshape(n - 1, 12).copy()).to(dev)

    def run_yardstick():
        """the kernel trace's pairs, EVERY pair guided by the rectified model (every row has a line).  --epi-case window: the band off
        (+inf) under a +-6 px window, beside the gated k-NN call at the same window, k and shapes - the same rows pass, the difference
        is the band's arithmetic.  --epi-case band: band 3 under an all-pass window, beside the UNGATED k-NN call - whether skipping
        rows pays for the fp64 test."""
        dset, dim = ctx.batch_desc_set()
        kps = ctx.batch_kp_set()
        if a.epi_case == "window":
            g = B.MatchEpipolarGuide.around(float("inf"), window=(-6.0, 6.0, -6.0, 6.0), max_octave_diff=1, fallback=0)
            ctx.match_knn_pairs_epipolar_guided(dset, dset, spec, 1, rectified, g, rows_cap=cap, query_kps=kps, train_kps=kps, stream=st,
                                                dim_bytes=dim, out=again)
            ctx.match_knn_pairs(dset, dset, spec, 1, rows_cap=cap, stream=st, dim_bytes=dim, out=again, gate=g.window, query_kps=kps,
                                train_kps=kps)
        else:
            g = B.MatchEpipolarGuide.around(3.0, fallback=0)
            ctx.match_knn_pairs_epipolar_guided(dset, dset, spec, 1, rectified, g, rows_cap=cap, query_kps=kps, train_kps=kps, stream=st,
                                                dim_bytes=dim, out=again)
            ctx.match_knn_pairs(dset, dset, spec, 1, rows_cap=cap, stream=st, dim_bytes=dim, out=again)

    runs = {"E": run_e, "L": run_l}
    order = "EL"
    if a.stats_pass:                                                # (no L: every launch of the new kernel in the trace is the yardstick's)
        for _ in range(2 + 8):
            run_e()
            run_yardstick()
            torch.cuda.synchronize()
        return
    for v in order + "EL":                                          # warm-up: buffers sized, scratch grown
        runs[v]()
        torch.cuda.synchronize()

    # one batch: what reaches the linker and what it makes of it, in E and in L; band == max_error: every record of L is a Sampson
    # inlier of its pair's model by the verifier's restated score
    run_l()
    torch.cuda.synchronize()
    dset, dim = ctx.batch_desc_set()
    mod = models.cpu().numpy().reshape(-1).view(B.PAIR_EPIPOLAR_MODEL)
    has_model = (mod["hypothesis"] >= 0) & ((mod["flags"] & (B.PAIR_NO_MODEL | B.PAIR_BAD)) == 0)
    ecounts, lcounts = ver[1].cpu().numpy(), lsel[1].cpu().numpy()
    sum_e, sum_l = link_e[3].cpu().numpy(), link_l[3].cpu().numpy()
    loffs, lrec = lsel[3].cpu().numpy(), lsel[0].cpu().numpy().view(B.DMATCH).reshape(-1)
    kps = [ctx.batch_download(f, True, strings=dim)[0] for f in range(n)]
    inliers = True
    for p in range(n - 1):
        rec = lrec[int(loffs[p]):int(loffs[p + 1])]
        if not has_model[p]:
            inliers = inliers and len(rec) == 0
            continue
        kq, kt = kps[p + 1][rec["queryIdx"]], kps[p][rec["trainIdx"]]
        ok = restated_inliers8(mod["f"][p][None, :], float(np.float32(a.max_error)) ** 2, kq["x"].astype(np.float64), kq["y"].astype(np.float64),
                               kt["x"].astype(np.float64), kt["y"].astype(np.float64))[0]
        inliers = bool(inliers and ok.all() and (np.abs(kt["x"] - kq["x"]) <= window_px).all() and (np.abs(kt["y"] - kq["y"]) <= window_px).all()
                       and (np.abs(kt["octave"] - kq["octave"]) <= octaves).all())

    call_ms = []
    for _ in range(max(a.repeats, 5)):
        run_l(timed=True)
        torch.cuda.synchronize()
        call_ms.append(ev[0].elapsed_time(ev[1]))

    fps = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                runs[v]()
                calls += 1
                if time.perf_counter() - t0 >= a.window:
                    break
            torch.cuda.synchronize()
            fps[v].append(calls * n / (time.perf_counter() - t0))
    med = {v: float(np.median(fps[v])) for v in order}
    ms = {v: 1e3 * n / med[v] for v in order}
    spread = {v: (max(fps[v]) - min(fps[v])) / med[v] for v in order}
    res = {
        "workload": "bench.py's stream: %dx%d, threshold %d, %d octaves, %d frames per batch (%d distinct) in HBM; frame-to-previous-frame, "
                    "k = %d, rows_cap %d, ratio 0.8, one match per row; epipolar verify: %d hypotheses, max_error %g, min_inliers %d, "
                    "keep_unverified 1; second pass: k = 1, band %g px, window +-%g px, octave difference %d, fallback 0, then keep 1 without "
                    "a ratio; tracks of min_len 3" % (W, H, THRESHOLD, OCTAVES, n, nd, k, cap, a.hypotheses, a.max_error, a.min_inliers,
                                                      a.max_error, window_px, octaves),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window, "order": ", ".join(order) + " alternating; every window ends in a synchronise"},
        "frames_per_s": {v: round(med[v], 1) for v in order},
        "frames_per_s_all": {v: [round(x, 1) for x in fps[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "ms_per_batch": {v: round(ms[v], 4) for v in order},
        "second_pass_ms_per_batch": {"L_minus_E": round(ms["L"] - ms["E"], 4)},
        "L_over_E_frames_per_s": round(med["L"] / med["E"], 4),
        "hip_event_ms": {"epipolar_guided_call_1_launch": {"median": round(float(np.median(call_ms)), 4), "all": [round(x, 4) for x in call_ms]}},
        "per_batch": {"pairs": n - 1, "pairs_with_a_model": int(has_model.sum()),
                      "records_per_pair_to_the_linker": {"E": round(float(ecounts.mean()), 2), "L": round(float(lcounts.mean()), 2)},
                      "links": {"E": int(sum_e[2]), "L": int(sum_l[2])},
                      "proposals_lost": {"E": int(sum_e[3]), "L": int(sum_l[3])}},
        "L_records_are_sampson_inliers_inside_their_windows": inliers,
        "note": "the stream's consecutive frames are unrelated; the epipolar verifier still accepts models at min_inliers %d, so L does scan" %
                a.min_inliers,
        "legend": {"E": "detect_describe_batch + match_knn_pairs + select + brisk_hip_verify_pair_matches_epipolar_device + link + list on one "
                        "stream",
                   "L": "E + brisk_hip_match_knn_pairs_epipolar_guided_device on the verifier's models + select (keep 1) + link on the new lists"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ext.close()
    ctx.close()


def mutual_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, batch, line):
    """--guided --mutual / --epiguided --mutual: the mutual guided call beside its yardsticks (see the module's text); writes a.out"""
    st = work.cuda_stream
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    if line:
        guide = B.MatchEpipolarGuide.around(a.max_error, window=(-64.0, 64.0, -64.0, 64.0), max_octave_diff=1, fallback=0)
        rec = np.zeros(n - 1, B.PAIR_EPIPOLAR_MODEL)
        rec["f"] = (0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0)  # rectified: every row has a line
    else:
        guide = B.MatchGuide.around(6.0, max_octave_diff=1, fallback=0)
        rec = np.zeros(n - 1, B.PAIR_MODEL)
        rec["h"] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)   # the identity: every pair guided, the gated call's mask
    models = torch.from_numpy(rec.view(np.int64).reshape(n - 1, 12).copy()).to(dev)
    out = {v: (torch.zeros((n - 1, cap, 1, 4), dtype=torch.int32, device=dev), torch.zeros((n - 1, cap), dtype=torch.int32, device=dev),
               torch.zeros(n - 1, dtype=torch.int32, device=dev)) for v in "UMNX"}
    batch()                                                          # one batch: the four calls read its sets
    torch.cuda.synchronize()
    dset, dim = ctx.batch_desc_set()
    kps = ctx.batch_kp_set()
    guided_call = ctx.match_knn_pairs_epipolar_guided if line else ctx.match_knn_pairs_guided
    mutual_call = ctx.match_mutual_pairs_epipolar_guided if line else ctx.match_mutual_pairs_guided
    runs = {
        "U": lambda: guided_call(dset, dset, spec, 1, models, guide, rows_cap=cap, query_kps=kps, train_kps=kps, stream=st, dim_bytes=dim, out=out["U"]),
        "M": lambda: mutual_call(dset, dset, spec, models, guide, rows_cap=cap, query_kps=kps, train_kps=kps, stream=st, dim_bytes=dim, out=out["M"]),
        "N": lambda: ctx.match_knn_pairs(dset, dset, spec, 1, rows_cap=cap, stream=st, dim_bytes=dim, out=out["N"], gate=guide.window, query_kps=kps,
                                         train_kps=kps),
        "X": lambda: ctx.match_knn_pairs(dset, dset, spec, 1, cross_check=True, rows_cap=cap, stream=st, dim_bytes=dim, out=out["X"],
                                         gate=guide.window, query_kps=kps, train_kps=kps),
    }
    order = "UMNX"
    for v in order + order:                                         # warm-up
        runs[v]()
        torch.cuda.synchronize()
    kept = {v: int((out[v][1][:, :] == 1).sum().item()) for v in order}
    same = bool(all(torch.equal(x, y) for x, y in zip(out["M"], out["X"]))) if not line else None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    call_ms = {v: [] for v in order}
    for _ in range(max(a.repeats, 5)):
        for v in order:
            ev[0].record(work)
            runs[v]()
            ev[1].record(work)
            torch.cuda.synchronize()
            call_ms[v].append(ev[0].elapsed_time(ev[1]))
    per = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                runs[v]()
                calls += 1
                if calls % 8 == 0:                                   # (the queue is drained now and then: the clock is the device's, not the enqueue's)
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= a.window:
                        break
            torch.cuda.synchronize()
            per[v].append(1e3 * (time.perf_counter() - t0) / calls)
    med = {v: float(np.median(per[v])) for v in order}
    spread = {v: (max(per[v]) - min(per[v])) / med[v] for v in order}
    res = {
        "workload": "bench.py's stream: %dx%d, threshold %d, %d octaves, %d frames per batch (%d distinct) in HBM; frame-to-previous-frame, "
                    "k = 1, rows_cap %d; every pair guided: %s; the four calls read one batch's sets"
                    % (W, H, THRESHOLD, OCTAVES, n, nd, cap,
                       "rectified models, band %g px, window +-64 px, octave difference 1" % a.max_error if line
                       else "identity models, window +-6 px, octave difference 1 (the gated call's mask)"),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window,
                    "order": ", ".join(order) + " alternating; a window is back-to-back calls of ONE kind, synchronised every 8 calls and at its end"},
        "ms_per_call": {v: round(med[v], 4) for v in order},
        "ms_per_call_all": {v: [round(x, 4) for x in per[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "hip_event_ms_1_call": {v: {"median": round(float(np.median(call_ms[v])), 4), "all": [round(x, 4) for x in call_ms[v]]} for v in order},
        "M_over_U": round(med["M"] / med["U"], 4),
        "X_over_N": round(med["X"] / med["N"], 4),
        "M_over_U_relative_to_X_over_N": round((med["M"] / med["U"]) / (med["X"] / med["N"]), 4),
        "rows_with_a_match": kept,
        "M_equals_X_bytewise": same,
        "legend": {"U": "the guided k-NN call, k = 1" if not line else "the epipolar-guided k-NN call, k = 1",
                   "M": "the mutual guided call" if not line else "the mutual epipolar-guided call",
                   "N": "the gated k-NN call at the guide's window, k = 1, no cross check",
                   "X": "the gated k-NN call at the guide's window, k = 1, cross_check = 1",
                   "yardstick": "X / N: the same backward scan with the lane's own position instead of a staged centre"
                                + ("" if not line else " (the line form's mask differs from the gate's: its ratio is reported without a bar)")},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if os.path.exists(a.out):                                       # one file for both forms
        with open(a.out) as f:
            both = json.load(f)
    else:
        both = {}
    both["line" if line else "centre"] = res
    with open(a.out, "w") as f:
        json.dump(both, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ext.close()
    ctx.close()


def tracks_download_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b0):
    """--tracks-download: windows T, D and P (see the module's text); writes a.out"""
    st = work.cuda_stream
    select = B.MatchSelect(float("inf"), 0.8, 1)
    L, h = ctx._L, ctx._h
    mcap = (n - 1) * cap                                            # (one match per row at the most)
    sel = (torch.zeros((mcap, 4), dtype=torch.int32, device=dev), torch.zeros(n - 1, dtype=torch.int32, device=dev),
           torch.zeros(n - 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))
    prev, age = (torch.zeros((n, cap), dtype=torch.int32, device=dev) for _ in range(2))
    track = torch.zeros((n, cap), dtype=torch.int64, device=dev)
    summary = torch.zeros(8, dtype=torch.int64, device=dev)
    tcap, ocap = n * cap // 4, n * cap
    lists = (torch.zeros(tcap, dtype=torch.int64, device=dev), torch.zeros(tcap, dtype=torch.int32, device=dev),
             torch.zeros(tcap + 1, dtype=torch.int64, device=dev), torch.zeros((ocap, 2), dtype=torch.int32, device=dev),
             torch.zeros(4, dtype=torch.int64, device=dev))
    seed = B.TrackSeed(None, None, 0, summary.data_ptr())           # numbered on from the call before
    m, cnt, rows = outs["B"]
    dst = [B.HostTrackList(tcap, ocap, pinned=True) for _ in range(2)]
    tickets = []
    # P's destinations: pinned, as large as the device arrays; the keypoints of every frame
    plists = tuple(torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in lists)
    prow = B.HostResults(n, n * cap, 0, pinned=True)
    last = {}

    def run_link():
        run_b0()
        ctx.check(L.brisk_hip_select_pair_matches_device(h, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), n - 1, cap, k, C.byref(select), mcap,
                                                         sel[1].data_ptr(), sel[2].data_ptr(), sel[3].data_ptr(), sel[0].data_ptr(), st))
        dset, _ = ctx.batch_desc_set()
        ptr, stride = ctx._node_rows((dset, 0, 1))
        ctx.check(L.brisk_hip_link_tracks_device(h, ptr, stride, n, cap, sel[3].data_ptr(), sel[0].data_ptr(), C.byref(seed), prev.data_ptr(),
                                                 track.data_ptr(), age.data_ptr(), summary.data_ptr(), st))
        return dset, ptr, stride

    def run_t():
        _, ptr, stride = run_link()
        ctx.check(L.brisk_hip_list_tracks_device(h, ptr, stride, n, cap, prev.data_ptr(), track.data_ptr(), age.data_ptr(), 3, tcap, ocap,
                                                 lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(), lists[3].data_ptr(),
                                                 lists[4].data_ptr(), st))

    def run_d():
        dset, _, _ = run_link()
        tickets.append(ctx.tracks_download((dset, 0, 1), n, cap, prev, track, age, 3, dst[len(tickets) % 2], stream=st))
        if len(tickets) >= 2:                                      # the batch before: its destination is the next one to be reused
            ctx.tracks_wait(tickets[-2])

    def drain_d():
        if tickets:
            ctx.tracks_wait(tickets[-1])
        del tickets[:]

    def run_p():
        run_t()
        work.synchronize()                                         # the summary says how much there is to copy
        plists[4].copy_(lists[4])
        stored = int(plists[4][2])
        plists[2][:stored + 1].copy_(lists[2][:stored + 1])
        nobs = int(plists[2][stored])
        plists[0][:stored].copy_(lists[0][:stored])
        plists[1][:stored].copy_(lists[1][:stored])
        plists[3][:nobs].copy_(lists[3][:nobs])
        ctx.batch_download_wait(ctx.batch_download_all(prow, stream=st))
        last["stored"], last["nobs"] = stored, nobs

    runs = {"T": run_t, "D": run_d, "P": run_p}
    ends = {"T": lambda: None, "D": drain_d, "P": lambda: None}
    order = "TDP"
    for v in order + "TD":                                         # warm-up: buffers sized, scratch and slabs grown
        runs[v]()
        ends[v]()
        torch.cuda.synchronize()
    if a.stats_pass:
        for _ in range(8):
            run_d()
        drain_d()
        torch.cuda.synchronize()
        return

    # what D delivers against what P delivers, joined on the host (the same batch content in every call; numbers apart: every
    # batch is numbered on from the one before)
    run_d()
    drain_d()
    run_p()
    torch.cuda.synchronize()
    d = dst[0]
    stored, nobs = last["stored"], last["nobs"]
    obs = plists[3][:nobs].numpy()
    joined = np.stack([prow.kps[int(prow.offsets[f]) + r] for f, r in obs]) if nobs else np.zeros(0, B.KEYPOINT)
    pw = d.points[:nobs].view(np.uint32).reshape(-1, 9)
    identical = bool(d.summary.tolist() == plists[4].tolist() and d.len[:stored].tobytes() == plists[1][:stored].numpy().tobytes() and
                     d.offsets[:stored + 1].tobytes() == plists[2][:stored + 1].numpy().tobytes() and
                     np.array_equal(np.diff(d.track[:stored]), np.diff(plists[0][:stored].numpy())) and
                     pw[:, :2].tobytes() == obs.tobytes() and pw[:, 2:].tobytes() == joined.tobytes())
    nrows = int(prow.offsets[n])
    bytes_d = 32 + 8 * stored + 4 * stored + 8 * (stored + 1) + 36 * nobs
    bytes_p = 32 + 8 * stored + 4 * stored + 8 * (stored + 1) + 8 * nobs + 4 * n + 4 * n + 8 * (n + 1) + 28 * nrows

    fps = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                runs[v]()
                calls += 1
                if time.perf_counter() - t0 >= a.window:
                    break
            ends[v]()
            torch.cuda.synchronize()
            fps[v].append(calls * n / (time.perf_counter() - t0))
    med = {v: float(np.median(fps[v])) for v in order}
    ms = {v: 1e3 * n / med[v] for v in order}
    spread = {v: (max(fps[v]) - min(fps[v])) / med[v] for v in order}
    res = {
        "workload": "bench.py's stream: %dx%d, threshold %d, %d octaves, %d frames per batch (%d distinct) in HBM; frame-to-previous-frame, "
                    "k = %d, rows_cap %d, ratio 0.8, one match per row; tracks of min_len 3, tracks_cap %d, points_cap %d"
                    % (W, H, THRESHOLD, OCTAVES, n, nd, k, cap, tcap, ocap),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window,
                    "order": ", ".join(order) + " alternating; every window ends with its transfers complete and a synchronise"},
        "frames_per_s": {v: round(med[v], 1) for v in order},
        "frames_per_s_all": {v: [round(x, 1) for x in fps[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "ms_per_batch": {v: round(ms[v], 4) for v in order},
        "D_over_T_frames_per_s": round(med["D"] / med["T"], 4),
        "D_over_P_frames_per_s": round(med["D"] / med["P"], 4),
        "bar": {"D_not_slower_than_P_by_more_than_T_spread": bool(med["D"] >= med["P"] * (1.0 - spread["T"])), "T_spread_rel": round(spread["T"], 4)},
        "bytes_per_batch": {"D": bytes_d, "P": bytes_p},
        "per_batch": {"nodes": n, "rows": nrows, "tracks_listed_min_len_3": int(d.summary[0]), "their_observations": int(d.summary[1]),
                      "tracks_stored": stored, "points_stored": nobs, "share_of_rows_listed": round(nobs / max(nrows, 1), 4),
                      "list_cut": bool(d.summary[3])},
        "D_equals_P_joined_on_the_host": identical,
        "legend": {"T": "detect_describe_batch + match_knn_pairs + select + brisk_hip_link_tracks_device + brisk_hip_list_tracks_device on one stream",
                   "D": "T with brisk_hip_tracks_download into pinned memory in place of the list call, waited for one batch later",
                   "P": "T, synchronise, hipMemcpy of the summary and the four list arrays' stored prefixes, brisk_hip_batch_download_all of the "
                        "keypoints and its wait; the host join is not timed"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ext.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds per window (repeats x window >= 1 s per variant)")
    ap.add_argument("--rows-cap", type=int, default=2048, help="rows per pair in the match buffers (the stream has ~1k keypoints per frame)")
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--radius", type=float, default=None, help="radius matching with this max_distance instead of k-NN")
    ap.add_argument("--cap", type=int, default=8, help="cap_per_query of the radius calls")
    ap.add_argument("--gate", default=None, help="dx_min,dx_max,dy_min,dy_max[,max_octave_diff]: adds the gated windows G, I and the masked C")
    ap.add_argument("--out", default=None, help="default: profiles/match_pairs.json, with --radius profiles/match_radius_pairs.json, "
                                                "with --gate the same names ending in _gated.json")
    ap.add_argument("--stats-pass", action="store_true")
    ap.add_argument("--export", action="store_true", help="windows B, E (packed, selected matches to the host) and D (padded arrays to the host)")
    ap.add_argument("--tracks", action="store_true", help="windows B (match + select) and T (B + link_tracks + list_tracks)")
    ap.add_argument("--tracks-download", action="store_true",
                    help="windows T (--tracks' T), D (tracks_download in place of the list call) and P (list, synchronise, copies, batch_download_all)")
    ap.add_argument("--verify", action="store_true", help="windows T (--tracks' T) and V (T with verify_pair_matches between select and link)")
    ap.add_argument("--epipolar", action="store_true",
                    help="windows T (--tracks' T) and E (T with verify_pair_matches_epipolar between select and link)")
    ap.add_argument("--guided", action="store_true",
                    help="windows V (--verify's V) and G (V + match_knn_pairs_guided on the verifier's models + select + link)")
    ap.add_argument("--epiguided", action="store_true",
                    help="windows E (--epipolar's E) and L (E + match_knn_pairs_epipolar_guided on the verifier's models + select + link)")
    ap.add_argument("--mutual", action="store_true",
                    help="with --guided or --epiguided: the mutual call (k = 1 with the cross check) beside the guided k = 1 call and the gated "
                         "k = 1 call with and without cross_check, every pair guided, in the same windows")
    ap.add_argument("--epi-case", choices=("window", "band"), default="window",
                    help="--epiguided --stats-pass: the new kernel with the band off under a +-6 px window beside the gated kernel, or with "
                         "band 3 under an all-pass window beside the ungated kernel (one rocprofv3 run each: the stats merge a kernel's launches)")
    ap.add_argument("--refit", action="store_true",
                    help="windows V (--verify's V) and R (V with refit_pair_models between verify and link), and the call on a related batch")
    ap.add_argument("--epirefit", action="store_true",
                    help="windows H (refit_pair_models) and F (refit_pair_models_epipolar) of back-to-back calls on the related batch")
    ap.add_argument("--rank2", type=int, default=1, help="--epirefit: 0 = the least-squares F as fitted, else its rank-2 projection")
    ap.add_argument("--rounds", type=int, default=2, help="--refit / --epirefit: rounds of fit and recount")
    ap.add_argument("--related-records", type=int, default=200, help="--refit: records per pair of the related batch")
    ap.add_argument("--hypotheses", type=int, default=256, help="--verify: hypotheses per pair")
    ap.add_argument("--max-error", type=float, default=3.0, help="--verify: the inlier threshold in pixels")
    ap.add_argument("--min-inliers", type=int, default=8, help="--verify: inliers an accepted model needs")
    a = ap.parse_args()

    radius = a.radius
    gate = None
    if a.gate is not None:
        g = [float(v) for v in a.gate.split(",")]
        gate = (g[0], g[1], g[2], g[3], int(g[4]) if len(g) > 4 else -1)
    if a.export:
        if radius is not None or gate:
            ap.error("--export measures the k-NN pair call: without --radius / --gate")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "match_pairs_export.json")
    if a.tracks:
        if radius is not None or gate or a.export:
            ap.error("--tracks measures the k-NN pair call: without --radius / --gate / --export")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "track_pairs.json")
    if a.tracks_download:
        if radius is not None or gate or a.export or a.tracks:
            ap.error("--tracks-download measures the k-NN pair call: without --radius / --gate / --export / --tracks")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "track_download.json")
    if a.verify:
        if radius is not None or gate or a.export or a.tracks or a.tracks_download:
            ap.error("--verify measures the k-NN pair call: without --radius / --gate / --export / --tracks / --tracks-download")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "verify_pairs.json")
    if a.epipolar:
        if radius is not None or gate or a.export or a.tracks or a.tracks_download or a.verify or a.guided or a.refit:
            ap.error("--epipolar measures the k-NN pair call: without --radius / --gate / --export / --tracks / --tracks-download / --verify / "
                     "--guided / --refit")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "epipolar_pairs.json")
    if a.mutual:
        if a.guided == a.epiguided:
            ap.error("--mutual goes with --guided or with --epiguided")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "match_mutual_pairs.json")
    if a.guided:
        if radius is not None or gate or a.export or a.tracks or a.tracks_download or a.verify:
            ap.error("--guided measures the k-NN pair call: without --radius / --gate / --export / --tracks / --tracks-download / --verify")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "guided_pairs.json")
    if a.epiguided:
        if radius is not None or gate or a.export or a.tracks or a.tracks_download or a.verify or a.guided or a.refit or a.epipolar:
            ap.error("--epiguided measures the k-NN pair call: without --radius / --gate / --export / --tracks / --tracks-download / --verify / "
                     "--guided / --refit / --epipolar")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "epiguided_pairs.json")
    if a.refit:
        if radius is not None or gate or a.export or a.tracks or a.tracks_download or a.verify or a.guided:
            ap.error("--refit measures the k-NN pair call: without --radius / --gate / --export / --tracks / --tracks-download / --verify / --guided")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "refit_pairs.json")
    if a.epirefit:
        if radius is not None or gate or a.export or a.tracks or a.tracks_download or a.verify or a.guided or a.refit or a.epipolar or a.epiguided:
            ap.error("--epirefit times the two refit calls on the related batch: without any other mode")
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "epipolar_refit_pairs.json")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", ("match_radius_pairs" if radius is not None else "match_pairs") +
                             ("_gated" if gate else "") + ".json")
    n, k, cap = a.batch, (a.cap if radius is not None else a.k), a.rows_cap   # (k: entries per row of the match buffers)
    LIST = 32                                  # MRP_LIST of brisk_match.hip: rows with more hits take the dense path
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.epirefit:                             # (no frame is detected: the related batch is made on the host)
        epirefit_mode(a, dev)
        return
    nd = min(a.distinct, n)
    ring = torch.from_numpy(np.stack(gen_frames(synth.frame_1080p, list(range(nd))))).to(dev)
    frames = ring[torch.arange(n, device=dev) % nd].contiguous()
    del ring
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    work = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(work)
    st = work.cuda_stream
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)   # frame to previous frame
    outs = {v: (torch.zeros((n - 1, cap, k, 4), dtype=torch.int32, device=dev), torch.zeros((n - 1, cap), dtype=torch.int32, device=dev),
                torch.zeros(n - 1, dtype=torch.int32, device=dev)) for v in "BCGI"}

    def batch():
        ctx.detect_describe_batch(ext, frames.data_ptr(), n, W, H, W * H, W, THRESHOLD, OCTAVES, st)

    def run_a():
        batch()

    def run_b():
        batch()
        dset, dim = ctx.batch_desc_set()
        if radius is not None:
            ctx.match_radius_pairs(dset, dset, spec, radius, k, rows_cap=cap, stream=st, dim_bytes=dim, out=outs["B"])
        else:
            ctx.match_knn_pairs(dset, dset, spec, k, rows_cap=cap, stream=st, dim_bytes=dim, out=outs["B"])

    def run_gated(which, g):
        batch()
        dset, dim = ctx.batch_desc_set()
        kps = ctx.batch_kp_set()
        if radius is not None:
            ctx.match_radius_pairs(dset, dset, spec, radius, k, rows_cap=cap, stream=st, dim_bytes=dim, out=outs[which], gate=g, query_kps=kps,
                                   train_kps=kps)
        else:
            ctx.match_knn_pairs(dset, dset, spec, k, rows_cap=cap, stream=st, dim_bytes=dim, out=outs[which], gate=g, query_kps=kps,
                                train_kps=kps)

    if a.export:
        export_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, batch, run_b)
        return
    if a.tracks:
        tracks_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b)
        return
    if a.tracks_download:
        tracks_download_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b)
        return
    if a.verify:
        verify_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b)
        return
    if a.epipolar:
        verify_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b, epipolar=True)
        return
    if a.mutual:
        mutual_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, batch, line=a.epiguided)
        return
    if a.guided:
        guided_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b)
        return
    if a.refit:
        refit_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b)
        return
    if a.epiguided:
        epiguided_mode(a, ctx, ext, n, nd, k, cap, dev, work, outs, run_b)
        return

    vp = C.c_void_p

    def run_c():
        batch()
        torch.cuda.synchronize()
        d_n, d_desc, cstride, kcap, pitch = vp(), vp(), C.c_int(), C.c_int(), C.c_int()
        ctx.check(ctx._L.brisk_hip_batch_results(ctx._h, None, C.byref(d_n), C.byref(cstride), None, None, C.byref(d_desc), C.byref(kcap),
                                                 C.byref(pitch)))
        ints = cstride.value // 4
        counts = torch.as_tensor(DeviceInts(d_n.value, (n - 1) * ints + 1), device=dev)[::ints].cpu().numpy()
        m, cnt, rows = outs["C"]
        fp = kcap.value * pitch.value
        L, h, fn = ctx._L, ctx._h, ctx._L.brisk_hip_match_knn_device
        for p in range(n - 1):
            nq, nt = min(int(counts[p + 1]), cap), int(counts[p])
            ctx.check(fn(h, d_desc.value + (p + 1) * fp, nq, pitch.value, d_desc.value + p * fp, nt, pitch.value, 48, k,
                         m.data_ptr() + p * cap * k * 16, cnt.data_ptr() + p * cap * 4, st))
        rows.copy_(torch.from_numpy(counts[1:].copy()), non_blocking=False)

    host_c = {"m": np.zeros((n - 1, cap, k), B.DMATCH), "cnt": np.zeros((n - 1, cap), np.int32)}

    def run_c_radius():
        batch()
        torch.cuda.synchronize()
        d_n, d_desc, cstride, kcap, pitch = vp(), vp(), C.c_int(), C.c_int(), C.c_int()
        ctx.check(ctx._L.brisk_hip_batch_results(ctx._h, None, C.byref(d_n), C.byref(cstride), None, None, C.byref(d_desc), C.byref(kcap),
                                                 C.byref(pitch)))
        ints = cstride.value // 4
        counts = torch.as_tensor(DeviceInts(d_n.value, (n - 1) * ints + 1), device=dev)[::ints].cpu().numpy()
        fp = kcap.value * pitch.value
        rows_dev = torch.as_tensor(DeviceBytes(d_desc.value, n * fp), device=dev).view(n, fp)
        desc = [rows_dev[f, :int(counts[f]) * pitch.value].cpu().numpy().reshape(-1, pitch.value) for f in range(n)]   # the rows of every frame
        L, h, fn = ctx._L, ctx._h, ctx._L.brisk_hip_match_radius
        one, pt = np.zeros(1, np.int32), np.array([pitch.value], np.int32)
        for p in range(n - 1):
            q, t = desc[p + 1], desc[p]
            nq = min(len(q), cap)
            one[0] = len(t)
            tptr = (C.c_void_p * 1)(t.ctypes.data if len(t) else None)
            ctx.check(fn(h, q.ctypes.data if nq else None, nq, pitch.value, 48, 1, tptr, one.ctypes.data, pt.ctypes.data, None, None,
                         float(radius), k, host_c["m"][p].ctypes.data, host_c["cnt"][p].ctypes.data))
        host_c["rows"] = counts[1:].copy()

    def gate_mask(kq, kt):
        """the mask the gate defines, in float32 as the header states it"""
        with np.errstate(invalid="ignore"):
            dx, dy = kt["x"][None, :] - kq["x"][:, None], kt["y"][None, :] - kq["y"][:, None]
            m = (dx >= np.float32(gate[0])) & (dx <= np.float32(gate[1])) & (dy >= np.float32(gate[2])) & (dy <= np.float32(gate[3]))
        if gate[4] >= 0:
            m &= np.abs(kt["octave"][None, :].astype(np.int64) - kq["octave"][:, None]) <= gate[4]
        return m

    gate_stats = {"steps": 0, "skipped": 0, "rows": 0, "rows_nothing_allowed": 0, "allowed": 0, "cells": 0}

    def run_c_gated(stats=False):
        batch()
        torch.cuda.synchronize()
        d_n, d_kps, d_desc, cstride, kcap, pitch = vp(), vp(), vp(), C.c_int(), C.c_int(), C.c_int()
        ctx.check(ctx._L.brisk_hip_batch_results(ctx._h, None, C.byref(d_n), C.byref(cstride), None, C.byref(d_kps), C.byref(d_desc),
                                                 C.byref(kcap), C.byref(pitch)))
        ints = cstride.value // 4
        counts = torch.as_tensor(DeviceInts(d_n.value, (n - 1) * ints + 1), device=dev)[::ints].cpu().numpy()
        fp, kfp = kcap.value * pitch.value, kcap.value * B.KEYPOINT.itemsize
        rows_dev = torch.as_tensor(DeviceBytes(d_desc.value, n * fp), device=dev).view(n, fp)
        kps_dev = torch.as_tensor(DeviceBytes(d_kps.value, n * kfp), device=dev).view(n, kfp)
        desc = [rows_dev[f, :int(counts[f]) * pitch.value].cpu().numpy().reshape(-1, pitch.value) for f in range(n)]
        kps = [kps_dev[f, :int(counts[f]) * B.KEYPOINT.itemsize].cpu().numpy().view(B.KEYPOINT) for f in range(n)]
        L, h = ctx._L, ctx._h
        one, pt, mp = np.zeros(1, np.int32), np.array([pitch.value], np.int32), np.zeros(1, np.int32)
        for p in range(n - 1):
            q, t = desc[p + 1], desc[p]
            nq = min(len(q), cap)
            one[0] = len(t)
            m = np.ascontiguousarray(gate_mask(kps[p + 1][:nq], kps[p]).astype(np.uint8))
            if stats and m.size:
                for w0 in range(0, nq, 64):
                    live = m[w0:w0 + 64].any(axis=0)
                    gate_stats["steps"] += live.size
                    gate_stats["skipped"] += int((~live).sum())
                gate_stats["rows"] += nq
                gate_stats["rows_nothing_allowed"] += int((m.sum(axis=1) == 0).sum())
                gate_stats["allowed"] += int(m.sum())
                gate_stats["cells"] += m.size
            mp[0] = m.strides[0] if m.size else 0
            tptr = (C.c_void_p * 1)(t.ctypes.data if len(t) else None)
            mptr = (C.c_void_p * 1)(m.ctypes.data if m.size else None)
            if radius is not None:
                ctx.check(L.brisk_hip_match_radius(h, q.ctypes.data if nq else None, nq, pitch.value, 48, 1, tptr, one.ctypes.data,
                                                   pt.ctypes.data, mptr, mp.ctypes.data, float(radius), k, host_c["m"][p].ctypes.data,
                                                   host_c["cnt"][p].ctypes.data))
            else:
                ctx.check(L.brisk_hip_match_knn(h, q.ctypes.data if nq else None, nq, pitch.value, 48, 1, tptr, one.ctypes.data,
                                                pt.ctypes.data, mptr, mp.ctypes.data, k, host_c["m"][p].ctypes.data,
                                                host_c["cnt"][p].ctypes.data))
        host_c["rows"] = counts[1:].copy()

    runs = {"A": run_a, "B": run_b, "C": run_c_radius if radius is not None else run_c}
    order = "ABC"
    if gate:
        g_given, g_all = B.MatchGate(*gate), B.MatchGate.all_pass()
        runs.update({"G": lambda: run_gated("G", g_given), "I": lambda: run_gated("I", g_all), "C": run_c_gated})
        order = "ABGIC"
    for v in order + "AB":                  # warm-up: buffers sized, the integral format settled on the stream's density
        runs[v]()
        torch.cuda.synchronize()
    if a.stats_pass:
        for _ in range(8):
            for v in ("BGI" if gate else "B"):
                runs[v]()
        torch.cuda.synchronize()
        return

    # B's rows against C's (with --gate: G's against the masked C's): the same matches, row for row (imgIdx aside: the pair call
    # writes the train frame's index, the one-pair call knows of one train image only and writes 0)
    dev_v = "G" if gate else "B"
    for t in outs[dev_v] + outs["C"]:
        t.zero_()
    runs[dev_v]()
    torch.cuda.synchronize()
    if gate:
        run_c_gated(stats=True)
        if radius is None:   # the reference's top-up entries (distance 2147483648, sorted last) are not part of a gated row
            real = (host_c["m"]["distance"] != np.float32(2147483648.0)) & (np.arange(k)[None, None, :] < host_c["cnt"][:, :, None])
            host_c["cnt"] = real.sum(axis=2).astype(np.int32)
    else:
        runs["C"]()
    torch.cuda.synchronize()
    if radius is not None or gate:   # variant C wrote host arrays: into the device triple the comparison below reads
        outs["C"][0].copy_(torch.from_numpy(host_c["m"].view(np.int32).reshape(n - 1, cap, k, 4)))
        outs["C"][1].copy_(torch.from_numpy(host_c["cnt"]))
        outs["C"][2].copy_(torch.from_numpy(host_c["rows"]))
    (mb, cb, rb), (mc, cc, rc) = outs[dev_v], outs["C"]
    valid = torch.arange(cap, device=dev)[None, :] < rb[:, None]
    sel = valid[:, :, None] & (torch.arange(k, device=dev)[None, None, :] < cb[:, :, None])   # the entries a row's count covers
    pidx = torch.arange(n - 1, device=dev, dtype=torch.int32)[:, None, None].expand(-1, cap, k)
    identical = bool(torch.equal(rb, rc) and torch.equal(cb[valid], cc[valid]) and
                     torch.equal(mb[sel][:, [0, 1, 3]], mc[sel][:, [0, 1, 3]]) and torch.equal(mb[..., 2][sel], pidx[sel]))
    rows_host = rb.cpu().numpy()
    hits = cb[valid].cpu().numpy()             # per query row: k-NN entries, or radius matches FOUND

    fps = {v: [] for v in order}
    for _ in range(a.repeats):
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            while True:
                runs[v]()
                calls += 1
                if time.perf_counter() - t0 >= a.window:
                    break
            torch.cuda.synchronize()
            fps[v].append(calls * n / (time.perf_counter() - t0))

    med = {v: float(np.median(fps[v])) for v in order}
    ms = {v: 1e3 * n / med[v] for v in order}            # per batch
    spread = {v: (max(fps[v]) - min(fps[v])) / med[v] for v in order}
    res = {
        "workload": "bench.py's stream: %dx%d, threshold %d, %d octaves, %d frames per batch (%d distinct) in HBM; frame-to-previous-frame, "
                    "%s, rows_cap %d" % (W, H, THRESHOLD, OCTAVES, n, nd,
                                         ("max_distance %g, cap_per_query %d" % (radius, k)) if radius is not None else "k = %d" % k, cap),
        "kernel_revision": ctx.kernel_revision(),
        "device": torch.cuda.get_device_name(0),
        "windows": {"repeats": a.repeats, "seconds_each": a.window,
                    "order": ", ".join(order) + " alternating; every window ends in a synchronise"},
        "frames_per_s": {v: round(med[v], 1) for v in order},
        "frames_per_s_all": {v: [round(x, 1) for x in fps[v]] for v in order},
        "spread_rel": {v: round(spread[v], 4) for v in order},
        "ms_per_batch": {v: round(ms[v], 4) for v in order},
        "matching_ms_per_batch": {"B_minus_A": round(ms["B"] - ms["A"], 4), "C_minus_A": round(ms["C"] - ms["A"], 4)},
        "B_over_C_frames_per_s": round(med["B"] / med["C"], 4),
        "matching_share_of_chunk_B": round((ms["B"] - ms["A"]) / ms["A"], 4),
        ("rows_identical_G_C" if gate else "rows_identical_B_C"): identical,
        "rows_per_pair": {"mean": round(float(rows_host.mean()), 1), "max": int(rows_host.max()), "cut_pairs": int((rows_host > cap).sum())},
        "legend": {"A": "detect_describe_batch", "B": "A + brisk_hip_match_knn_pairs_device on the same stream",
                   "C": "A, synchronise, counts to the host, one brisk_hip_match_knn_device call per pair"},
    }
    if radius is not None:
        res["legend"].update({"B": "A + brisk_hip_match_radius_pairs_device on the same stream",
                              "C": "A, synchronise, every frame's rows to the host, one brisk_hip_match_radius call per pair"})
        res.update({"max_distance": radius, "cap_per_query": k,
                    "hits_per_query": {"mean": round(float(hits.mean()), 4), "max": int(hits.max()), "rows": int(hits.size),
                                       "rows_without_a_hit": round(float((hits == 0).mean()), 4),
                                       "rows_over_the_cap": round(float((hits > k).mean()), 6)},
                    "dense_path_share_of_rows": round(float((hits > LIST).mean()), 6), "dense_path_list_keys": LIST})
    if gate:
        ms_spread = {v: ms[v] * spread[v] for v in order}   # the spread of a window's frames/s as milliseconds per batch
        res["legend"].update({"B": res["legend"]["B"] + " (the UNGATED call)",
                              "G": "A + the gated pair call with the given gate on the same stream",
                              "I": "A + the gated pair call with the all-pass gate",
                              "C": "A, synchronise, every frame's keypoints and rows to the host, the pair's mask built there, one "
                                   "brisk_hip_match_%s call with that mask per pair" % ("radius" if radius is not None else "knn")})
        res["matching_ms_per_batch"].update({"G_minus_A": round(ms["G"] - ms["A"], 4), "I_minus_A": round(ms["I"] - ms["A"], 4)})
        res.update({
            "gate": {"dx_min": gate[0], "dx_max": gate[1], "dy_min": gate[2], "dy_max": gate[3], "max_octave_diff": gate[4]},
            "gate_on_the_bench_frames": {
                "mask_density": round(gate_stats["allowed"] / max(gate_stats["cells"], 1), 6),
                "wave_row_steps_without_an_allowed_lane": round(gate_stats["skipped"] / max(gate_stats["steps"], 1), 4),
                "query_rows_with_no_allowed_row": round(gate_stats["rows_nothing_allowed"] / max(gate_stats["rows"], 1), 4)},
            "G_against_B": {"added_ms_G": round(ms["G"] - ms["A"], 4), "added_ms_B": round(ms["B"] - ms["A"], 4),
                            "G_minus_B_ms": round(ms["G"] - ms["B"], 4),
                            "spread_ms_B_plus_G": round(ms_spread["B"] + ms_spread["G"], 4),
                            "bar_met": bool(ms["G"] - ms["B"] <= ms_spread["B"] + ms_spread["G"])},
            "I_against_B": {"added_ms_I": round(ms["I"] - ms["A"], 4), "I_minus_B_ms": round(ms["I"] - ms["B"], 4),
                            "added_ratio_I_over_B": round((ms["I"] - ms["A"]) / max(ms["B"] - ms["A"], 1e-9), 4)},
            "G_over_C_frames_per_s": round(med["G"] / med["C"], 4)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ext.close()
    ctx.close()


if __name__ == "__main__":
    main()
