"""ethzasl_brisk_amd - MI355X-native BRISK detect+describe engine.

Python-side mirror of the two reference classes over the C ABI (include/brisk_hip.h).  It exists for
the test-suite and bench.py; the product is libbrisk_hip.so plus the C++ host classes in
include/brisk/.  There is no CPU fallback: every compute call needs the HIP library and a GPU.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# BRISK_HIP_LIB: tuning experiments only (an alternative build of the same library, e.g. with another -D knob)
LIB_PATH = os.environ.get("BRISK_HIP_LIB") or os.path.join(HERE, "libbrisk_hip.so")

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

ERRORS = {1: "BRISK_HIP_ERR_ARG", 2: "BRISK_HIP_ERR_NO_DEVICE", 3: "BRISK_HIP_ERR_HIP", 4: "BRISK_HIP_ERR_CAPACITY",
          5: "BRISK_HIP_ERR_THRESHOLD", 6: "BRISK_HIP_ERR_PATTERN", 7: "BRISK_HIP_ERR_UNSUPPORTED"}

# every symbol include/brisk_hip.h declares
ABI_SYMBOLS = [
    "brisk_hip_create", "brisk_hip_destroy", "brisk_hip_last_error", "brisk_hip_set_capacity",
    "brisk_hip_device_count", "brisk_hip_pattern_create", "brisk_hip_pattern_create_from_text",
    "brisk_hip_pattern_destroy", "brisk_hip_pattern_descriptor_size", "brisk_hip_pattern_points",
    "brisk_hip_pattern_tables", "brisk_hip_detect", "brisk_hip_describe", "brisk_hip_detect_describe_batch",
    "brisk_hip_detect_batch", "brisk_hip_batch_results", "brisk_hip_batch_download", "brisk_hip_batch_status",
    "brisk_hip_profile_enable", "brisk_hip_profile_stages",
    "brisk_hip_profile_stage_name", "brisk_hip_profile_read", "brisk_hip_set_bucketing", "brisk_hip_halfsample16", "brisk_hip_twothirdsample16",
    "brisk_hip_integral_image16",
    "brisk_hip_set_streams", "brisk_hip_profile_frames_per_launch",
    "brisk_hip_match_knn", "brisk_hip_match_radius", "brisk_hip_match_knn_device", "brisk_hip_set_uniformity",
    "brisk_hip_reserve", "brisk_hip_detect_uniform", "brisk_hip_detect_describe_batch_host", "brisk_hip_stream_ceiling",
    "brisk_hip_kernel_revision", "brisk_hip_compute_scale", "brisk_hip_describe_same_image", "brisk_hip_detect_filtered",
    "brisk_hip_comm_unique_id", "brisk_hip_comm_create", "brisk_hip_comm_destroy", "brisk_hip_comm_rank", "brisk_hip_comm_world",
    "brisk_hip_comm_gather_results", "brisk_hip_comm_wait",
    "brisk_hip_set_integral_format",
    "brisk_hip_host_register", "brisk_hip_host_unregister", "brisk_hip_usable_cpus",
    "brisk_hip_detect_images", "brisk_hip_describe_images",
    "brisk_hip_pool_create", "brisk_hip_pool_destroy", "brisk_hip_pool_last_error", "brisk_hip_pool_detect", "brisk_hip_pool_describe", "brisk_hip_pool_stats",
    "brisk_hip_batch_download_all", "brisk_hip_batch_download_wait", "brisk_hip_detect_describe_batch_host_results",
    "brisk_hip_batch_desc_set", "brisk_hip_match_knn_pairs_device",
    "brisk_hip_match_radius_pairs_device", "brisk_hip_match_radius_device",
    "brisk_hip_batch_kp_set", "brisk_hip_match_knn_pairs_gated_device", "brisk_hip_match_radius_pairs_gated_device",
    "brisk_hip_select_pair_matches_device", "brisk_hip_pair_matches_download", "brisk_hip_pair_matches_wait",
    "brisk_hip_verify_pair_matches_device", "brisk_hip_refit_pair_models_device",
    "brisk_hip_verify_pair_matches_epipolar_device", "brisk_hip_refit_pair_models_epipolar_device",
    "brisk_hip_match_knn_pairs_guided_device", "brisk_hip_match_radius_pairs_guided_device",
    "brisk_hip_match_knn_pairs_epipolar_guided_device", "brisk_hip_match_radius_pairs_epipolar_guided_device",
    "brisk_hip_match_mutual_pairs_guided_device", "brisk_hip_match_mutual_pairs_epipolar_guided_device",
    "brisk_hip_link_tracks_device", "brisk_hip_list_tracks_device",
    "brisk_hip_track_points_device", "brisk_hip_tracks_download", "brisk_hip_tracks_wait",
]
# every symbol include/brisk_hip_debug.h declares: test / tuning builds (BRISK_HIP_TUNING) only
DEBUG_SYMBOLS = [
    "brisk_hip_debug_layer", "brisk_hip_debug_integral", "brisk_hip_debug_counters", "brisk_hip_debug_counters_raw",
    "brisk_hip_debug_set_flags", "brisk_hip_debug_image_reuse", "brisk_hip_debug_filter_keypoints", "brisk_hip_debug_integral_bits",
    "brisk_hip_debug_forge_pattern_device", "brisk_hip_debug_pool_phases",
]


class PostFilter(C.Structure):
    """brisk_hip_postfilter: the optional post-filters of one detect call"""
    _fields_ = [("uniformity_radius", C.c_double), ("uniformity_max_keypoints", C.c_int), ("num_buckets_u", C.c_int),
                ("num_buckets_v", C.c_int), ("bucket_max_keypoints", C.c_int)]


class BatchHostResults(C.Structure):
    """brisk_hip_batch_host_results: capacities + the five destination arrays of a whole batch in host memory"""
    _fields_ = [("frames_cap", C.c_int), ("desc_stride", C.c_int), ("rows_cap", C.c_longlong), ("counts", C.c_void_p),
                ("flags", C.c_void_p), ("offsets", C.c_void_p), ("kps", C.c_void_p), ("desc", C.c_void_p)]


ROWS_CUT = 0x100


class DescSet(C.Structure):
    """brisk_hip_desc_set: `frames` frames of descriptor rows in device memory, the row counts in device memory too"""
    _fields_ = [("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("count_stride", C.c_int), ("frame_pitch", C.c_long),
                ("row_pitch", C.c_int), ("frames", C.c_int)]


class PairSpec(C.Structure):
    """brisk_hip_pair_spec: pair p = (query_first + p * query_step, train_first + p * train_step), or - d_pairs set - a
    device array of npairs x {query frame, train frame}"""
    _fields_ = [("npairs", C.c_int), ("query_first", C.c_int), ("query_step", C.c_int), ("train_first", C.c_int),
                ("train_step", C.c_int), ("d_pairs", C.c_void_p)]


class KpSet(C.Structure):
    """brisk_hip_kp_set: the keypoint records (28 bytes each, device memory) that belong to the rows of a DescSet"""
    _fields_ = [("d_kps", C.c_void_p), ("frame_pitch", C.c_long)]


class MatchGate(C.Structure):
    """brisk_hip_match_gate: rows q, t may match iff dx_min <= T.x - Q.x <= dx_max, dy_min <= T.y - Q.y <= dy_max and
    (max_octave_diff < 0 or |T.octave - Q.octave| <= max_octave_diff); -inf / +inf switch a bound off"""
    _fields_ = [("dx_min", C.c_float), ("dx_max", C.c_float), ("dy_min", C.c_float), ("dy_max", C.c_float), ("max_octave_diff", C.c_int)]

    @classmethod
    def all_pass(cls):
        return cls(-float("inf"), float("inf"), -float("inf"), float("inf"), -1)


class MatchGuide(C.Structure):
    """brisk_hip_match_guide: the gate's window around the centre C = H_p(Q) the pair's model gives query keypoint Q (bounds on T - C,
    max_octave_diff between Q and T); fallback: a pair without a usable model - 0 = its rows match nothing, else C = Q"""
    _fields_ = [("window", MatchGate), ("fallback", C.c_int)]

    @classmethod
    def around(cls, radius, max_octave_diff=-1, fallback=0):
        """a square window of +-radius pixels"""
        r = float(radius)
        return cls(MatchGate(-r, r, -r, r, int(max_octave_diff)), int(fallback))


class MatchEpipolarGuide(C.Structure):
    """brisk_hip_match_epipolar_guide: a train keypoint T may match query keypoint Q iff it lies within `band` pixels of Q's epipolar
    line under the pair's model F and passes the gate `window` around Q itself (bounds on T - Q, max_octave_diff between Q and T);
    fallback: a pair without a usable model - 0 = its rows match nothing, else the plain gate of `window`"""
    _fields_ = [("window", MatchGate), ("band", C.c_float), ("fallback", C.c_int)]

    @classmethod
    def around(cls, band, window=None, max_octave_diff=-1, fallback=0):
        """+-band pixels around the line; window: a MatchGate or its (dx_min, dx_max, dy_min, dy_max) - None = all-pass -, whose
        octave rule is max_octave_diff"""
        w = MatchGate.all_pass() if window is None else window if isinstance(window, MatchGate) else MatchGate(*[float(v) for v in window][:4])
        return cls(MatchGate(w.dx_min, w.dx_max, w.dy_min, w.dy_max, int(max_octave_diff)), float(band), int(fallback))


class MatchSelect(C.Structure):
    """brisk_hip_match_select: an entry is kept iff distance < max_distance (and it is no top-up entry); ratio > 0: Lowe's ratio
    test, the row gives at most its best entry; otherwise the leading keep_per_row entries that pass"""
    _fields_ = [("max_distance", C.c_float), ("ratio", C.c_float), ("keep_per_row", C.c_int)]

    @classmethod
    def everything(cls, per_row):
        return cls(float("inf"), 0.0, int(per_row))


class PairHostMatches(C.Structure):
    """brisk_hip_pair_host_matches: capacities + the five destination arrays of a batch's selected matches in host memory"""
    _fields_ = [("pairs_cap", C.c_int), ("matches_cap", C.c_longlong), ("pair_rows", C.c_void_p), ("counts", C.c_void_p),
                ("flags", C.c_void_p), ("offsets", C.c_void_p), ("matches", C.c_void_p)]


class PairVerify(C.Structure):
    """brisk_hip_pair_verify: a record is an inlier of a hypothesis iff its transfer error is at most max_error pixels (train frame);
    `hypotheses` four-record samples per pair (1 ... 4096), a model needs min_inliers (>= 4) inliers; keep_unverified: what a pair
    without an accepted model keeps (0 = nothing, else its usable records); seed: of the sampler"""
    _fields_ = [("max_error", C.c_float), ("hypotheses", C.c_int), ("min_inliers", C.c_int), ("keep_unverified", C.c_int),
                ("seed", C.c_uint)]


class PairRefit(C.Structure):
    """brisk_hip_pair_refit: max_error - the verifier's inlier threshold, pixels in the train frame; rounds (1 ... 8) of fit and
    recount; a model needs min_inliers (>= 4) inliers; keep_unverified: as PairVerify"""
    _fields_ = [("max_error", C.c_float), ("rounds", C.c_int), ("min_inliers", C.c_int), ("keep_unverified", C.c_int)]


class PairEpipolarRefit(C.Structure):
    """brisk_hip_pair_epipolar_refit: max_error - the epipolar verifier's threshold, the Sampson distance in pixels; rounds (1 ... 8)
    of fit and recount; a model needs min_inliers (>= 8) inliers; keep_unverified: as PairVerify; rank2: 0 = the least-squares F as
    fitted, else its rank-2 projection"""
    _fields_ = [("max_error", C.c_float), ("rounds", C.c_int), ("min_inliers", C.c_int), ("keep_unverified", C.c_int), ("rank2", C.c_int)]


# brisk_hip_pair_model: the winner's normalised H and the pair's counts
PAIR_MODEL = np.dtype([("h", "<f8", (9,)), ("records", "<i4"), ("usable", "<i4"), ("inliers", "<i4"), ("hypothesis", "<i4"),
                       ("valid", "<i4"), ("flags", "<i4")])

# brisk_hip_pair_epipolar_model: the winner's normalised F (row-major, x'^T F x = 0) and the pair's counts.  PAIR_MODEL's layout under
# another name on purpose: refit_pair_models and the guided matchers read a PAIR_MODEL as a homography; the epipolar-guided matchers
# read these
PAIR_EPIPOLAR_MODEL = np.dtype([("f", "<f8", (9,)), ("records", "<i4"), ("usable", "<i4"), ("inliers", "<i4"), ("hypothesis", "<i4"),
                                ("valid", "<i4"), ("flags", "<i4")])


class TrackSeed(C.Structure):
    """brisk_hip_track_seed: d_track / d_age [rows_cap] device arrays (row r of node 0 continues track d_track[r] >= 0 at age
    d_age[r]; both None = no seeds), first_new = the first number the call may give - read from the device word d_first_new when
    that is set (the previous call's summary).  The structure holds raw pointers: the caller keeps the tensors alive."""
    _fields_ = [("d_track", C.c_void_p), ("d_age", C.c_void_p), ("first_new", C.c_longlong), ("d_first_new", C.c_void_p)]


TRACK_OBS = np.dtype([("node", "<i4"), ("row", "<i4")])   # brisk_hip_track_obs
TRACKS_CUT = 1                                              # flag bit 0 of list_tracks' summary
# brisk_hip_track_point: an observation and the keypoint it names, byte-identical to the source record
TRACK_POINT = np.dtype([("node", "<i4"), ("row", "<i4")] + [(n, KEYPOINT.fields[n][0]) for n in KEYPOINT.names])


class HostTracks(C.Structure):
    """brisk_hip_host_tracks: capacities + the five destination arrays of a batch's listed tracks in host memory"""
    _fields_ = [("tracks_cap", C.c_longlong), ("points_cap", C.c_longlong), ("summary", C.c_void_p), ("track", C.c_void_p),
                ("len", C.c_void_p), ("offsets", C.c_void_p), ("points", C.c_void_p)]


# flags of a pair in the selected lists (ROWS_CUT: the pair and every pair behind it did not fit matches_cap)
PAIR_ROWS_CUT, PAIR_BAD, PAIR_ENTRIES_CUT = 1, 2, 4
PAIR_NO_MODEL = 8   # verify_pair_matches: the pair has no accepted model
PAIR_REFIT = 0x10   # refit_pair_models / refit_pair_models_epipolar: at least one round replaced the input model


def _host_array(n, dtype, pinned, keep):
    """n (at least 1) elements of host memory: from torch's pinned allocator (kept alive in `keep`), or a plain NumPy array"""
    n = max(int(n), 1)
    if pinned:
        import torch
        t = torch.empty(n * np.dtype(dtype).itemsize, dtype=torch.uint8).pin_memory()
        keep.append(t)
        return t.numpy().view(dtype)
    return np.empty(n, dtype)


class HostMatches:
    """Destination arrays of brisk_hip_pair_matches_download: `pairs` pairs, `matches` DMATCH records in total.  pinned as in
    HostResults."""

    def __init__(self, pairs, matches, pinned=True):
        self.pairs, self.matches_cap = int(pairs), int(matches)
        self._keep = []
        self.pair_rows = _host_array(pairs, np.int32, pinned, self._keep)
        self.counts = _host_array(pairs, np.int32, pinned, self._keep)
        self.flags = _host_array(pairs, np.int32, pinned, self._keep)
        self.offsets = _host_array(pairs + 1, np.int64, pinned, self._keep)
        self.matches = _host_array(matches, DMATCH, pinned, self._keep)
        self.struct = PairHostMatches(self.pairs, self.matches_cap, self.pair_rows.ctypes.data, self.counts.ctypes.data,
                                      self.flags.ctypes.data, self.offsets.ctypes.data, self.matches.ctypes.data)

    def pair(self, p):
        """the selected matches of pair p, in (query row, rank) order: a view of the records [offsets[p], offsets[p + 1])"""
        return self.matches[int(self.offsets[p]):int(self.offsets[p + 1])]


class HostTrackList:
    """Destination arrays of brisk_hip_tracks_download: `tracks` pieces, `points` TRACK_POINT records in total; summary = pieces
    listed, their observations, pieces stored, flags.  pinned as in HostResults."""

    def __init__(self, tracks, points, pinned=True):
        self.tracks_cap, self.points_cap = int(tracks), int(points)
        self._keep = []
        self.summary = _host_array(4, np.int64, pinned, self._keep)
        self.track = _host_array(tracks, np.int64, pinned, self._keep)
        self.len = _host_array(tracks, np.int32, pinned, self._keep)
        self.offsets = _host_array(tracks + 1, np.int64, pinned, self._keep)
        self.points = _host_array(points, TRACK_POINT, pinned, self._keep)
        self.struct = HostTracks(self.tracks_cap, self.points_cap, self.summary.ctypes.data, self.track.ctypes.data, self.len.ctypes.data,
                                 self.offsets.ctypes.data, self.points.ctypes.data)

    @property
    def stored(self):
        return int(self.summary[2])

    def piece(self, i):
        """(track number, length, points) of stored piece i: the points a view of the records [offsets[i], offsets[i + 1])"""
        return int(self.track[i]), int(self.len[i]), self.points[int(self.offsets[i]):int(self.offsets[i + 1])]


class HostResults:
    """Destination arrays of brisk_hip_batch_download_all: `frames` frames, `rows` rows in total, descriptor rows of
    `desc_stride` bytes (0 = keypoints only).  pinned=True takes them from torch's pinned allocator (the device then writes
    them directly); otherwise plain NumPy arrays (pageable: the engine goes through its own pinned bounce buffer)."""

    def __init__(self, frames, rows, desc_stride=48, pinned=True):
        self.frames, self.rows, self.desc_stride = int(frames), int(rows), int(desc_stride)
        self._keep = []

        def arr(n, dtype):
            return _host_array(n, dtype, pinned, self._keep)
        self.counts = arr(frames, np.int32)
        self.flags = arr(frames, np.int32)
        self.offsets = arr(frames + 1, np.int64)
        self.kps = arr(rows, KEYPOINT)
        self.desc = arr(rows * max(desc_stride, 1), np.uint8).reshape(max(rows, 1), max(desc_stride, 1)) if desc_stride else None
        self.struct = BatchHostResults(self.frames, self.desc_stride or 4, self.rows, self.counts.ctypes.data, self.flags.ctypes.data,
                                       self.offsets.ctypes.data, self.kps.ctypes.data,
                                       self.desc.ctypes.data if self.desc is not None else None)

    def frame(self, f, strings=None):
        """(keypoints, descriptors) of frame f: views of the rows [offsets[f], offsets[f + 1])"""
        a, b = int(self.offsets[f]), int(self.offsets[f + 1])
        d = None if self.desc is None else self.desc[a:b, :strings or self.desc_stride]
        return self.kps[a:b], d


class BriskHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERRORS.get(code, code), msg))
        self.code = code


_lib = None


def load_library():
    """Loads libbrisk_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # torch wheels bundle their own HIP runtime under the same SONAME (libamdhip64.so.7).  If torch is
        # going to be used in this process (tests, bench.py) it must be loaded first so that this library
        # binds to the runtime already in the process: two HIP runtimes in one process cannot both own the GPU.
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError("libbrisk_hip.so is missing: run `python -m ethzasl_brisk_amd.build` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.brisk_hip_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.brisk_hip_destroy.argtypes = [vp]
    L.brisk_hip_destroy.restype = None
    L.brisk_hip_last_error.argtypes = [vp]
    L.brisk_hip_last_error.restype = C.c_char_p
    L.brisk_hip_set_capacity.argtypes = [vp, C.c_int, C.c_int]
    L.brisk_hip_pattern_create.argtypes = [vp, C.c_int, C.c_float, C.POINTER(vp)]
    L.brisk_hip_pattern_create_from_text.argtypes = [vp, C.c_char_p, C.c_float, C.POINTER(vp)]
    L.brisk_hip_pattern_destroy.argtypes = [vp]
    L.brisk_hip_pattern_destroy.restype = None
    L.brisk_hip_pattern_descriptor_size.argtypes = [vp]
    L.brisk_hip_pattern_points.argtypes = [vp]
    L.brisk_hip_pattern_tables.argtypes = [vp, vp, vp, vp]
    L.brisk_hip_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp,
                                   C.c_int, ip]
    L.brisk_hip_describe.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, ip, vp, C.c_int, C.c_int, C.c_int]
    L.brisk_hip_describe_same_image.argtypes = L.brisk_hip_describe.argtypes
    L.brisk_hip_detect_describe_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int,
                                                  C.c_int, vp]
    L.brisk_hip_detect_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, vp]
    L.brisk_hip_batch_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), ip, C.POINTER(vp), C.POINTER(vp),
                                          C.POINTER(vp), ip, ip]
    L.brisk_hip_batch_download.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, ip, vp, C.c_int]
    L.brisk_hip_batch_status.argtypes = [vp, C.c_int, ip]
    if hasattr(L, "brisk_hip_debug_layer"):
        L.brisk_hip_debug_layer.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, ip, ip]
    if hasattr(L, "brisk_hip_debug_integral"):
        L.brisk_hip_debug_integral.argtypes = [vp, C.c_int, vp]
    if hasattr(L, "brisk_hip_debug_integral_bits"):
        L.brisk_hip_debug_integral_bits.argtypes = [vp, C.c_int]
    if hasattr(L, "brisk_hip_debug_counters"):
        L.brisk_hip_debug_counters.argtypes = [vp, C.c_int, vp, ip]
    if hasattr(L, "brisk_hip_debug_counters_raw"):
        L.brisk_hip_debug_counters_raw.argtypes = [vp, C.c_int, vp, C.c_int]
    L.brisk_hip_profile_enable.argtypes = [vp, C.c_int]
    if hasattr(L, "brisk_hip_debug_set_flags"):
        L.brisk_hip_debug_set_flags.argtypes = [vp, C.c_int]
    L.brisk_hip_set_integral_format.argtypes = [vp, C.c_int]
    if hasattr(L, "brisk_hip_debug_forge_pattern_device"):
        L.brisk_hip_debug_forge_pattern_device.argtypes = [vp, C.c_int]
    if hasattr(L, "brisk_hip_debug_image_reuse"):
        L.brisk_hip_debug_image_reuse.argtypes = [vp]
    L.brisk_hip_set_bucketing.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    for f in (L.brisk_hip_halfsample16, L.brisk_hip_twothirdsample16, L.brisk_hip_integral_image16):
        f.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int]
    L.brisk_hip_set_streams.argtypes = [vp, C.c_int]
    L.brisk_hip_profile_frames_per_launch.argtypes = [vp]
    L.brisk_hip_profile_stage_name.argtypes = [C.c_int]
    L.brisk_hip_profile_stage_name.restype = C.c_char_p
    L.brisk_hip_profile_read.argtypes = [vp, vp, ip]
    L.brisk_hip_set_uniformity.argtypes = [vp, C.c_double, C.c_int]
    L.brisk_hip_match_knn.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp]
    L.brisk_hip_match_radius.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_float,
                                         C.c_int, vp, vp]
    L.brisk_hip_match_knn_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.brisk_hip_batch_desc_set.argtypes = [vp, C.POINTER(DescSet), ip]
    L.brisk_hip_match_knn_pairs_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(PairSpec), C.c_int, C.c_int,
                                                   C.c_int, C.c_int, vp, vp, vp, vp]
    L.brisk_hip_match_radius_pairs_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(PairSpec), C.c_int, C.c_float,
                                                      C.c_int, C.c_int, vp, vp, vp, vp]
    L.brisk_hip_match_radius_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp]
    L.brisk_hip_batch_kp_set.argtypes = [vp, C.POINTER(KpSet)]
    L.brisk_hip_match_knn_pairs_gated_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                         C.POINTER(MatchGate), C.POINTER(PairSpec), C.c_int, C.c_int, C.c_int, C.c_int,
                                                         vp, vp, vp, vp]
    L.brisk_hip_match_radius_pairs_gated_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                            C.POINTER(MatchGate), C.POINTER(PairSpec), C.c_int, C.c_float, C.c_int, C.c_int,
                                                            vp, vp, vp, vp]
    L.brisk_hip_select_pair_matches_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(MatchSelect), C.c_longlong,
                                                       vp, vp, vp, vp, vp]
    L.brisk_hip_pair_matches_download.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(MatchSelect),
                                                  C.POINTER(PairHostMatches), vp, C.POINTER(C.c_uint)]
    L.brisk_hip_pair_matches_wait.argtypes = [vp, C.c_uint, ip]
    L.brisk_hip_verify_pair_matches_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                       C.POINTER(PairSpec), C.c_int, vp, vp, C.c_longlong, C.POINTER(PairVerify),
                                                       C.c_longlong, vp, vp, vp, vp, vp, vp]
    L.brisk_hip_verify_pair_matches_epipolar_device.argtypes = L.brisk_hip_verify_pair_matches_device.argtypes
    L.brisk_hip_refit_pair_models_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                     C.POINTER(PairSpec), C.c_int, vp, vp, C.c_longlong, vp, C.POINTER(PairRefit),
                                                     C.c_longlong, vp, vp, vp, vp, vp, vp]
    L.brisk_hip_refit_pair_models_epipolar_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                              C.POINTER(PairSpec), C.c_int, vp, vp, C.c_longlong, vp,
                                                              C.POINTER(PairEpipolarRefit), C.c_longlong, vp, vp, vp, vp, vp, vp]
    L.brisk_hip_match_knn_pairs_guided_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                          C.POINTER(PairSpec), vp, C.POINTER(MatchGuide), C.c_int, C.c_int, C.c_int,
                                                          vp, vp, vp, vp]
    L.brisk_hip_match_knn_pairs_epipolar_guided_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                                   C.POINTER(PairSpec), vp, C.POINTER(MatchEpipolarGuide), C.c_int, C.c_int, C.c_int,
                                                                   vp, vp, vp, vp]
    L.brisk_hip_match_radius_pairs_epipolar_guided_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                                      C.POINTER(PairSpec), vp, C.POINTER(MatchEpipolarGuide), C.c_int, C.c_float,
                                                                      C.c_int, C.c_int, vp, vp, vp, vp]
    L.brisk_hip_match_radius_pairs_guided_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                             C.POINTER(PairSpec), vp, C.POINTER(MatchGuide), C.c_int, C.c_float, C.c_int,
                                                             C.c_int, vp, vp, vp, vp]
    L.brisk_hip_match_mutual_pairs_guided_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                             C.POINTER(PairSpec), vp, C.POINTER(MatchGuide), C.c_int, C.c_int, vp, vp, vp, vp]
    L.brisk_hip_match_mutual_pairs_epipolar_guided_device.argtypes = [vp, C.POINTER(DescSet), C.POINTER(DescSet), C.POINTER(KpSet), C.POINTER(KpSet),
                                                                      C.POINTER(PairSpec), vp, C.POINTER(MatchEpipolarGuide), C.c_int, C.c_int,
                                                                      vp, vp, vp, vp]
    L.brisk_hip_link_tracks_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(TrackSeed), vp, vp, vp, vp, vp]
    L.brisk_hip_list_tracks_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_longlong, C.c_longlong,
                                               vp, vp, vp, vp, vp, vp]
    L.brisk_hip_track_points_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_longlong, C.POINTER(KpSet), C.c_int,
                                                C.c_int, vp, vp]
    L.brisk_hip_tracks_download.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.POINTER(KpSet), C.c_int, C.c_int,
                                            C.POINTER(HostTracks), vp, C.POINTER(C.c_uint)]
    L.brisk_hip_tracks_wait.argtypes = [vp, C.c_uint, ip]
    L.brisk_hip_reserve.argtypes = [vp, C.c_int, C.c_int]
    L.brisk_hip_detect_uniform.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                           C.c_double, C.c_int, vp, C.c_int, ip]
    L.brisk_hip_detect_filtered.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                            C.POINTER(PostFilter), vp, C.c_int, ip]
    if hasattr(L, "brisk_hip_debug_filter_keypoints"):
        L.brisk_hip_debug_filter_keypoints.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp, ip]
    L.brisk_hip_comm_unique_id.argtypes = [vp]
    L.brisk_hip_comm_create.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.brisk_hip_comm_destroy.argtypes = [vp]
    L.brisk_hip_comm_destroy.restype = None
    L.brisk_hip_comm_rank.argtypes = [vp]
    L.brisk_hip_comm_world.argtypes = [vp]
    L.brisk_hip_comm_gather_results.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.brisk_hip_comm_wait.argtypes = [vp, vp]
    L.brisk_hip_compute_scale.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp,
                                          C.c_int, ip]
    L.brisk_hip_detect_describe_batch_host.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int,
                                                       C.c_int]
    L.brisk_hip_pool_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.brisk_hip_pool_destroy.argtypes = [vp]
    L.brisk_hip_pool_destroy.restype = None
    L.brisk_hip_pool_last_error.argtypes = [vp]
    L.brisk_hip_pool_last_error.restype = C.c_char_p
    L.brisk_hip_pool_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.brisk_hip_pool_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, ip, C.POINTER(C.c_ulonglong)]
    L.brisk_hip_pool_describe.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, ip, vp, C.c_int, C.c_int, C.c_int, C.c_ulonglong]
    L.brisk_hip_detect_images.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(BatchHostResults),
                                          C.POINTER(C.c_uint)]
    L.brisk_hip_describe_images.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(BatchHostResults), C.POINTER(C.c_uint)]
    L.brisk_hip_host_register.argtypes = [vp, C.c_size_t]
    L.brisk_hip_host_unregister.argtypes = [vp]
    L.brisk_hip_batch_download_all.argtypes = [vp, C.c_int, C.POINTER(BatchHostResults), vp, C.POINTER(C.c_uint)]
    L.brisk_hip_batch_download_wait.argtypes = [vp, C.c_uint, ip]
    L.brisk_hip_detect_describe_batch_host_results.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int,
                                                               C.c_int, C.POINTER(BatchHostResults), C.POINTER(C.c_uint)]
    L.brisk_hip_stream_ceiling.argtypes = [vp, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.brisk_hip_kernel_revision.argtypes = []
    L.brisk_hip_kernel_revision.restype = C.c_char_p
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _kcopy(a, n=None):
    """copy of the first n records of a contiguous KEYPOINT array through a byte view (NumPy copies structured arrays
    field by field: 2.8 ms per 100 000 keypoints instead of 0.1 ms)"""
    n = len(a) if n is None else n
    out = np.empty(n, KEYPOINT)
    out.view(np.uint8)[:] = a.view(np.uint8)[:n * KEYPOINT.itemsize]
    return out


class Context:
    """Device workspace (one per GPU).  Shared by detector and extractor objects."""

    def __init__(self, device=0, max_candidates=None, max_keypoints=None):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.brisk_hip_create(device, C.byref(h))
        if rc:
            raise BriskHipError(rc, "brisk_hip_create(device=%d) failed" % device)
        self._h = h
        self.device = device
        if max_candidates or max_keypoints:
            self.check(self._L.brisk_hip_set_capacity(h, max_candidates or 65536, max_keypoints or 16384))

    def check(self, rc):
        if rc:
            raise BriskHipError(rc, self._L.brisk_hip_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.brisk_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- per-stage access (parity tests) --
    def debug_layer(self, frame, layer, which=0):
        w, h = C.c_int(), C.c_int()
        self.check(self._L.brisk_hip_debug_layer(self._h, frame, layer, which, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        self.check(self._L.brisk_hip_debug_layer(self._h, frame, layer, which, _ptr(out), C.byref(w), C.byref(h)))
        return out

    def debug_counters(self, frame):
        """work counts of one frame of the last batch: candidates, keypoints, described, flags, ties per layer"""
        out = np.zeros(28, np.int32)
        nl = C.c_int()
        self.check(self._L.brisk_hip_debug_counters(self._h, frame, _ptr(out), C.byref(nl)))
        return {"candidates": int(out[0]), "keypoints": int(out[1]), "described": int(out[2]), "flags": int(out[3]),
                "ties": [int(v) for v in out[4:4 + nl.value]], "experiment": [int(v) for v in out[20:28]]}

    def debug_counters_raw(self, frame):
        """the frame's counter record as int32 words (instrumented build variants append fields)"""
        out = np.zeros(1024, np.int32)
        n = self._L.brisk_hip_debug_counters_raw(self._h, frame, _ptr(out), out.nbytes)
        if n < 0:
            raise BriskHipError(-1, "brisk_hip_debug_counters_raw failed")
        return out[:n // 4]

    def debug_integral(self, frame, w, h):
        """(h + 1) x (w + 1) u32: the integral image of the last describe, modulo 2 ** debug_integral_bits()"""
        out = np.zeros((h + 1, w + 1), np.uint32)
        self.check(self._L.brisk_hip_debug_integral(self._h, frame, _ptr(out)))
        return out

    def debug_integral_bits(self, frame=0):
        return self._L.brisk_hip_debug_integral_bits(self._h, frame)

    def set_uniformity(self, radius, max_keypoints=0x7FFFFFFF):
        """Optional uniformity enforcement after the detector (0 = off); see brisk_hip_set_uniformity."""
        self.check(self._L.brisk_hip_set_uniformity(self._h, float(radius), int(max_keypoints)))

    def set_bucketing(self, num_buckets_u, num_buckets_v, max_keypoints):
        """Optional KeyPointBucketing after the detector while uniformity is off ((0, 0, *) = off); see brisk_hip_set_bucketing."""
        self.check(self._L.brisk_hip_set_bucketing(self._h, int(num_buckets_u), int(num_buckets_v), int(max_keypoints)))

    def _image16(self, fn, image, out):
        img = np.ascontiguousarray(image, np.uint16)
        h, w = img.shape
        self.check(fn(self._h, _ptr(img), w, h, w, _ptr(out), out.shape[1]))
        return out

    def halfsample16(self, image):
        """brisk::Halfsample16 (image-down-sampling.cc:56-139)"""
        h, w = np.shape(image)
        return self._image16(self._L.brisk_hip_halfsample16, image, np.zeros((h // 2, w // 2), np.uint16))

    def twothirdsample16(self, image):
        """brisk::Twothirdsample16 (image-down-sampling.cc:394-548)"""
        h, w = np.shape(image)
        return self._image16(self._L.brisk_hip_twothirdsample16, image, np.zeros((h // 3 * 2, w // 3 * 2), np.uint16))

    def integral_image16(self, image):
        """brisk::IntegralImage16 (internal/integral-image.h:163-218): (h + 1) x (w + 1) float32"""
        h, w = np.shape(image)
        return self._image16(self._L.brisk_hip_integral_image16, image, np.zeros((h + 1, w + 1), np.float32))

    def set_streams(self, n):
        self.check(self._L.brisk_hip_set_streams(self._h, n))

    def profile_frames_per_launch(self):
        return self._L.brisk_hip_profile_frames_per_launch(self._h)

    def debug_image_reuse(self):
        """describe calls that reused the device copy of the image a detect call had uploaded"""
        return self._L.brisk_hip_debug_image_reuse(self._h)

    def set_integral_format(self, fmt):
        """0 = automatic (from the previous batch's candidate density), 24 / 32 = that element size for every call"""
        self.check(self._L.brisk_hip_set_integral_format(self._h, int(fmt)))

    def debug_set_flags(self, flags):
        self.check(self._L.brisk_hip_debug_set_flags(self._h, flags))

    # -- per-stage HIP-event timing of the batch path --
    def profile_enable(self, on=True):
        self.check(self._L.brisk_hip_profile_enable(self._h, int(on)))

    def profile_read(self):
        """{stage name: average ms per call}, number of calls averaged."""
        n = self._L.brisk_hip_profile_stages()
        ms = np.zeros(n, np.float32)
        calls = C.c_int()
        self.check(self._L.brisk_hip_profile_read(self._h, _ptr(ms), C.byref(calls)))
        return {self._L.brisk_hip_profile_stage_name(i).decode(): float(ms[i]) for i in range(n)}, calls.value

    # -- device-resident batch path --
    def detect_describe_batch(self, pattern, d_frames_ptr, nframes, w, h, frame_pitch, row_pitch, threshold, octaves,
                              stream=None):
        self.check(self._L.brisk_hip_detect_describe_batch(self._h, pattern._h, C.c_void_p(d_frames_ptr), nframes, w, h,
                                                           frame_pitch, row_pitch, threshold, octaves,
                                                           C.c_void_p(stream) if stream else None))

    def detect_describe_batch_host(self, pattern, h_frames_ptr, nframes, w, h, frame_pitch, row_pitch, threshold, octaves):
        """frames in (pinned) HOST memory: sliced H2D copies on a copy stream overlapped with compute"""
        self.check(self._L.brisk_hip_detect_describe_batch_host(self._h, pattern._h, C.c_void_p(h_frames_ptr), nframes, w,
                                                                h, frame_pitch, row_pitch, threshold, octaves))

    def batch_download_all(self, dst, described=True, stream=None):
        """queues the transfer of the last batch's results into `dst` (HostResults); returns the ticket"""
        t = C.c_uint()
        self.check(self._L.brisk_hip_batch_download_all(self._h, int(described), C.byref(dst.struct),
                                                        C.c_void_p(stream) if stream else None, C.byref(t)))
        return t.value

    def batch_download_wait(self, ticket, check=True):
        """completes transfer `ticket`; returns the number of flagged frames (check=False: (rc, flagged) instead of raising)"""
        n = C.c_int()
        rc = self._L.brisk_hip_batch_download_wait(self._h, ticket, C.byref(n))
        if not check:
            return rc, n.value
        self.check(rc)
        return n.value

    def detect_describe_batch_host_results(self, pattern, h_frames_ptr, nframes, w, h, frame_pitch, row_pitch, threshold, octaves,
                                           dst):
        """host frames in, host results out (everything queued on return); returns the ticket"""
        t = C.c_uint()
        self.check(self._L.brisk_hip_detect_describe_batch_host_results(self._h, pattern._h, C.c_void_p(h_frames_ptr), nframes, w, h,
                                                                        frame_pitch, row_pitch, threshold, octaves,
                                                                        C.byref(dst.struct), C.byref(t)))
        return t.value

    def detect_images(self, images, threshold, octaves, dst):
        """cv::FeatureDetector::detect(vector<Mat>) as one batch: `images` = equally sized 2-D uint8 arrays; returns the ticket"""
        imgs = [np.ascontiguousarray(a, np.uint8) for a in images]
        h, w = imgs[0].shape
        ptrs = (C.c_void_p * len(imgs))(*[a.ctypes.data for a in imgs])
        t = C.c_uint()
        self.check(self._L.brisk_hip_detect_images(self._h, ptrs, len(imgs), w, h, w, threshold, octaves, C.byref(dst.struct), C.byref(t)))
        self._keep_images = imgs
        return t.value

    def describe_images(self, pattern, images, keypoints, dst, rotation_invariant=True, scale_invariant=True, same_images=False):
        """cv::DescriptorExtractor::compute(vector<Mat>, vector<vector<KeyPoint>>) as one batch; returns the ticket.
        same_images: `images` are the arrays the last detect_images call was given, unchanged (no second upload)"""
        imgs = [np.ascontiguousarray(a, np.uint8) for a in images]
        ks = [np.ascontiguousarray(k, KEYPOINT) for k in keypoints]
        h, w = imgs[0].shape
        ptrs = (C.c_void_p * len(imgs))(*[a.ctypes.data for a in imgs])
        kptrs = (C.c_void_p * len(ks))(*[k.ctypes.data if len(k) else None for k in ks])
        nk = np.array([len(k) for k in ks], np.int32)
        t = C.c_uint()
        self.check(self._L.brisk_hip_describe_images(self._h, pattern._h, ptrs, len(imgs), w, h, w, kptrs, _ptr(nk), int(rotation_invariant),
                                                     int(scale_invariant), int(same_images), C.byref(dst.struct), C.byref(t)))
        self._keep_images = (imgs, ks, nk)
        return t.value

    def reserve(self, min_candidates, min_keypoints):
        self.check(self._L.brisk_hip_reserve(self._h, int(min_candidates), int(min_keypoints)))

    def stream_ceiling(self, nbytes=1 << 30):
        """(copy GB/s counting read + write, read-only GB/s) of the engine's float4 streaming kernels on this box"""
        a, b = C.c_double(), C.c_double()
        self.check(self._L.brisk_hip_stream_ceiling(self._h, nbytes, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kernel_revision(self):
        return self._L.brisk_hip_kernel_revision().decode()

    def detect_batch(self, d_frames_ptr, nframes, w, h, frame_pitch, row_pitch, threshold, octaves, stream=None):
        self.check(self._L.brisk_hip_detect_batch(self._h, C.c_void_p(d_frames_ptr), nframes, w, h, frame_pitch,
                                                  row_pitch, threshold, octaves, C.c_void_p(stream) if stream else None))

    def batch_status(self, nframes):
        f = C.c_int()
        self.check(self._L.brisk_hip_batch_status(self._h, nframes, C.byref(f)))
        return f.value

    def batch_download(self, frame, described=True, strings=48):
        n = C.c_int()
        self.check(self._L.brisk_hip_batch_download(self._h, frame, int(described), None, 0, C.byref(n), None, 0))
        kps = np.zeros(max(n.value, 1), KEYPOINT)
        desc = np.zeros((max(n.value, 1), strings), np.uint8)
        self.check(self._L.brisk_hip_batch_download(self._h, frame, int(described), _ptr(kps), len(kps), C.byref(n),
                                                    _ptr(desc) if described else None, strings))
        return _kcopy(kps, n.value), (desc[:n.value].copy() if described else None)

    # -- all frame pairs of a batch matched in one call --
    def batch_desc_set(self):
        """(DescSet of the last batch's described rows, descriptor bytes); valid until the context's next batch"""
        st, dim = DescSet(), C.c_int()
        self.check(self._L.brisk_hip_batch_desc_set(self._h, C.byref(st), C.byref(dim)))
        return st, dim.value

    def batch_kp_set(self):
        """KpSet of the last batch's described keypoints, row for row with batch_desc_set()'s rows; valid as long as that set"""
        kps = KpSet()
        self.check(self._L.brisk_hip_batch_kp_set(self._h, C.byref(kps)))
        return kps

    def _kp_sets(self, query_kps, train_kps):
        """keypoint sets left out = the last batch's"""
        if query_kps is None or train_kps is None:
            own = self.batch_kp_set()
            query_kps = own if query_kps is None else query_kps
            train_kps = own if train_kps is None else train_kps
        return query_kps, train_kps

    def _gate_args(self, gate, query_kps, train_kps):
        """the three extra arguments of the gated calls"""
        query_kps, train_kps = self._kp_sets(query_kps, train_kps)
        return C.byref(query_kps), C.byref(train_kps), C.byref(gate)

    def _pairs_prologue(self, pairs, dim_bytes, rows_cap, per_row, out):
        """what the pair matchers share: dim_bytes None = the last batch's descriptor size, rows_cap None = the context's keypoint
        capacity, out None = new (uninitialised) device tensors (matches [npairs, rows_cap, per_row, 4], counts, pair_rows)"""
        import torch
        if dim_bytes is None:
            dim_bytes = self.batch_desc_set()[1]
        if rows_cap is None:
            cap = C.c_int()
            self.check(self._L.brisk_hip_batch_results(self._h, None, None, None, None, None, None, C.byref(cap), None))
            rows_cap = cap.value
        if out is None:
            n, dev = max(pairs.npairs, 0), "cuda:%d" % self.device
            out = (torch.empty((n, max(rows_cap, 0), max(per_row, 1), 4), dtype=torch.int32, device=dev),
                   torch.empty((n, max(rows_cap, 0)), dtype=torch.int32, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev))
        return dim_bytes, rows_cap, out

    def match_knn_pairs(self, query, train, pairs, k, cross_check=False, rows_cap=None, stream=None, dim_bytes=None, out=None,
                        download=False, gate=None, query_kps=None, train_kps=None):
        """brisk_hip_match_knn_pairs_device.  query / train: DescSet; pairs: PairSpec.  rows_cap None = the context's keypoint
        capacity, dim_bytes None = the last batch's descriptor size.  Returns the device tensors (matches [npairs, rows_cap, k, 4]
        int32 - DMATCH records -, counts [npairs, rows_cap], pair_rows [npairs]); `out` = such a triple to be written instead of
        new (uninitialised) tensors.  Asynchronous unless download=True: that synchronises and returns, per pair, the list of
        per-query DMATCH arrays BruteForceMatcher.knnMatch returns (a pair with pair_rows -1: an empty list).
        gate (a MatchGate): brisk_hip_match_knn_pairs_gated_device - only rows whose keypoints (query_kps / train_kps: KpSet, None =
        the last batch's) pass the gate are matched, and a row holds real matches only (no top-up entry)."""
        import torch
        n = pairs.npairs
        dim_bytes, rows_cap, out = self._pairs_prologue(pairs, dim_bytes, rows_cap, k, out)
        m, cnt, rows = out
        if gate is not None:
            self.check(self._L.brisk_hip_match_knn_pairs_gated_device(self._h, C.byref(query), C.byref(train),
                                                                      *self._gate_args(gate, query_kps, train_kps), C.byref(pairs),
                                                                      int(dim_bytes), int(k), int(bool(cross_check)), int(rows_cap),
                                                                      m.data_ptr(), cnt.data_ptr(), rows.data_ptr(),
                                                                      C.c_void_p(stream) if stream else None))
        else:
            self.check(self._L.brisk_hip_match_knn_pairs_device(self._h, C.byref(query), C.byref(train), C.byref(pairs), int(dim_bytes), int(k),
                                                                int(bool(cross_check)), int(rows_cap), m.data_ptr(), cnt.data_ptr(),
                                                                rows.data_ptr(), C.c_void_p(stream) if stream else None))
        return self._knn_rows(out, n, rows_cap, k) if download else out

    def match_radius_pairs(self, query, train, pairs, max_distance, cap_per_query, rows_cap=None, stream=None, dim_bytes=None, out=None,
                           download=False, gate=None, query_kps=None, train_kps=None):
        """brisk_hip_match_radius_pairs_device; the conventions of match_knn_pairs.  Returns the device tensors (matches
        [npairs, rows_cap, cap_per_query, 4] int32 - DMATCH records -, counts [npairs, rows_cap] = matches FOUND, pair_rows
        [npairs]) or writes the triple `out`.  Asynchronous unless download=True: that synchronises and returns (rows, counts):
        per pair the list of per-query DMATCH arrays cut to min(count, cap_per_query), and per pair the counts of those rows.
        gate / query_kps / train_kps as in match_knn_pairs: brisk_hip_match_radius_pairs_gated_device."""
        import torch
        n, cpq = pairs.npairs, int(cap_per_query)
        dim_bytes, rows_cap, out = self._pairs_prologue(pairs, dim_bytes, rows_cap, cpq, out)
        m, cnt, rows = out
        if gate is not None:
            self.check(self._L.brisk_hip_match_radius_pairs_gated_device(self._h, C.byref(query), C.byref(train),
                                                                         *self._gate_args(gate, query_kps, train_kps), C.byref(pairs),
                                                                         int(dim_bytes), float(max_distance), cpq, int(rows_cap),
                                                                         m.data_ptr(), cnt.data_ptr(), rows.data_ptr(),
                                                                         C.c_void_p(stream) if stream else None))
        else:
            self.check(self._L.brisk_hip_match_radius_pairs_device(self._h, C.byref(query), C.byref(train), C.byref(pairs), int(dim_bytes),
                                                                   float(max_distance), cpq, int(rows_cap), m.data_ptr(), cnt.data_ptr(),
                                                                   rows.data_ptr(), C.c_void_p(stream) if stream else None))
        return self._radius_rows(out, n, rows_cap, cpq) if download else out

    def _knn_rows(self, out, n, rows_cap, k):
        """download=True of the k-NN pair matchers: synchronises; per pair the list of per-query DMATCH arrays"""
        import torch
        m, cnt, rows = out
        torch.cuda.synchronize(self.device)
        hm = m.cpu().numpy().view(DMATCH).reshape(n, rows_cap, max(k, 1))
        hc, hr = cnt.cpu().numpy(), rows.cpu().numpy()
        return [[hm[p, q, :hc[p, q]].copy() for q in range(min(max(int(hr[p]), 0), rows_cap))] for p in range(n)]

    def _radius_rows(self, out, n, rows_cap, cpq):
        """download=True of the radius pair matchers: synchronises; (rows, counts)"""
        import torch
        m, cnt, rows = out
        torch.cuda.synchronize(self.device)
        hm = m.cpu().numpy().view(DMATCH).reshape(n, rows_cap, cpq)
        hc, hr = cnt.cpu().numpy(), rows.cpu().numpy()
        nrows = [min(max(int(hr[p]), 0), rows_cap) for p in range(n)]
        return ([[hm[p, q, :min(int(hc[p, q]), cpq)].copy() for q in range(nrows[p])] for p in range(n)],
                [hc[p, :nrows[p]].copy() for p in range(n)])

    # -- the pairs matched again inside a window around each pair's model --
    def _guide_args(self, models, guide, query_kps, train_kps):
        """the four extra arguments of the guided calls; models: the tensor verify_pair_matches returns, or a device pointer"""
        query_kps, train_kps = self._kp_sets(query_kps, train_kps)
        ptr = models.data_ptr() if hasattr(models, "data_ptr") else models
        return C.byref(query_kps), C.byref(train_kps), (C.c_void_p(int(ptr)) if ptr else None), C.byref(guide)

    def _guided_call(self, fn, rows_form, query, train, pairs, models, guide, rows_cap, query_kps, train_kps, stream, dim_bytes, out, download,
                     per_row, scalars=()):
        """what the six guided matchers share.  fn: the entry point; rows_form: what download=True returns, _knn_rows or _radius_rows;
        per_row: the entries of a row; scalars: fn's arguments between dim_bytes and rows_cap"""
        n = pairs.npairs
        dim_bytes, rows_cap, out = self._pairs_prologue(pairs, dim_bytes, rows_cap, per_row, out)
        m, cnt, pair_rows = out
        qk, tk, mp, gp = self._guide_args(models, guide, query_kps, train_kps)
        self.check(fn(self._h, C.byref(query), C.byref(train), qk, tk, C.byref(pairs), mp, gp, int(dim_bytes), *scalars, int(rows_cap),
                      m.data_ptr(), cnt.data_ptr(), pair_rows.data_ptr(), C.c_void_p(stream) if stream else None))
        return rows_form(out, n, rows_cap, per_row) if download else out

    def match_knn_pairs_guided(self, query, train, pairs, k, models, guide, rows_cap=None, query_kps=None, train_kps=None, stream=None,
                               dim_bytes=None, out=None, download=False):
        """brisk_hip_match_knn_pairs_guided_device: match_knn_pairs behind the window of `guide` (a MatchGuide) centred where pair
        p's model models[p] puts each query keypoint.  models: the tensor verify_pair_matches returns ([npairs, 12] int64, PAIR_MODEL
        records), or any device pointer to npairs records.  No cross_check argument (match_mutual_pairs_guided).  Everything else, and what is returned, as match_knn_pairs
        with a gate."""
        return self._guided_call(self._L.brisk_hip_match_knn_pairs_guided_device, self._knn_rows, query, train, pairs, models, guide, rows_cap,
                                 query_kps, train_kps, stream, dim_bytes, out, download, per_row=k, scalars=(int(k),))

    def match_radius_pairs_guided(self, query, train, pairs, max_distance, cap_per_query, models, guide, rows_cap=None, query_kps=None,
                                  train_kps=None, stream=None, dim_bytes=None, out=None, download=False):
        """brisk_hip_match_radius_pairs_guided_device: match_radius_pairs behind the guide; the conventions of
        match_knn_pairs_guided, and what is returned as match_radius_pairs."""
        cpq = int(cap_per_query)
        return self._guided_call(self._L.brisk_hip_match_radius_pairs_guided_device, self._radius_rows, query, train, pairs, models, guide, rows_cap,
                                 query_kps, train_kps, stream, dim_bytes, out, download, per_row=cpq, scalars=(float(max_distance), cpq))

    # -- the pairs matched again inside a band around each epipolar line --
    def match_knn_pairs_epipolar_guided(self, query, train, pairs, k, models, guide, rows_cap=None, query_kps=None, train_kps=None, stream=None,
                                        dim_bytes=None, out=None, download=False):
        """brisk_hip_match_knn_pairs_epipolar_guided_device: match_knn_pairs behind `guide` (a MatchEpipolarGuide) - the band around each
        query keypoint's epipolar line under pair p's model models[p], inside the guide's window around the keypoint.  models: the
        tensor verify_pair_matches_epipolar returns ([npairs, 12] int64, PAIR_EPIPOLAR_MODEL records), or any device pointer to npairs
        records.  No cross_check argument (match_mutual_pairs_epipolar_guided).  Everything else, and what is returned, as match_knn_pairs
        with a gate."""
        return self._guided_call(self._L.brisk_hip_match_knn_pairs_epipolar_guided_device, self._knn_rows, query, train, pairs, models, guide,
                                 rows_cap, query_kps, train_kps, stream, dim_bytes, out, download, per_row=k, scalars=(int(k),))

    def match_radius_pairs_epipolar_guided(self, query, train, pairs, max_distance, cap_per_query, models, guide, rows_cap=None, query_kps=None,
                                           train_kps=None, stream=None, dim_bytes=None, out=None, download=False):
        """brisk_hip_match_radius_pairs_epipolar_guided_device: match_radius_pairs behind the epipolar guide; the conventions of
        match_knn_pairs_epipolar_guided, and what is returned as match_radius_pairs."""
        cpq = int(cap_per_query)
        return self._guided_call(self._L.brisk_hip_match_radius_pairs_epipolar_guided_device, self._radius_rows, query, train, pairs, models,
                                 guide, rows_cap, query_kps, train_kps, stream, dim_bytes, out, download, per_row=cpq,
                                 scalars=(float(max_distance), cpq))

    # -- the guided pair matchers' mutual forms: k = 1 with the cross check --
    def match_mutual_pairs_guided(self, query, train, pairs, models, guide, rows_cap=None, query_kps=None, train_kps=None, stream=None,
                                  dim_bytes=None, out=None, download=False):
        """brisk_hip_match_mutual_pairs_guided_device: match_knn_pairs_guided for k = 1 with the cross check - row q keeps its record
        iff, under the same mask asked from the train side, its train row's best match among ALL rows of the query frame is q.
        Arguments, and what is returned, as match_knn_pairs_guided with k = 1."""
        return self._guided_call(self._L.brisk_hip_match_mutual_pairs_guided_device, self._knn_rows, query, train, pairs, models, guide, rows_cap,
                                 query_kps, train_kps, stream, dim_bytes, out, download, per_row=1)

    def match_mutual_pairs_epipolar_guided(self, query, train, pairs, models, guide, rows_cap=None, query_kps=None, train_kps=None, stream=None,
                                           dim_bytes=None, out=None, download=False):
        """brisk_hip_match_mutual_pairs_epipolar_guided_device: match_knn_pairs_epipolar_guided for k = 1 with the cross check; the
        conventions of match_mutual_pairs_guided."""
        return self._guided_call(self._L.brisk_hip_match_mutual_pairs_epipolar_guided_device, self._knn_rows, query, train, pairs, models, guide,
                                 rows_cap, query_kps, train_kps, stream, dim_bytes, out, download, per_row=1)

    # -- the pair matchers' exit: selected matches, packed --
    def select_pair_matches(self, out_triple, per_row, select, matches_cap=None, stream=None):
        """brisk_hip_select_pair_matches_device on what match_knn_pairs / match_radius_pairs returned (out_triple; per_row = that
        call's k or cap_per_query).  select: a MatchSelect.  matches_cap None = every stored entry fits (npairs * rows_cap * per_row).
        Returns the device tensors (matches [matches_cap, 4] int32 - DMATCH records in (pair, query row, rank) order -, counts
        [npairs], flags [npairs], offsets [npairs + 1] int64; offsets[npairs] = matches stored).  Asynchronous on `stream`."""
        import torch
        m, cnt, rows = out_triple
        n, rows_cap = int(cnt.shape[0]), int(cnt.shape[1])
        if matches_cap is None:
            matches_cap = n * rows_cap * int(per_row)
        dev = m.device
        res = (torch.empty((max(int(matches_cap), 0), 4), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev))
        self.check(self._L.brisk_hip_select_pair_matches_device(self._h, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), n, rows_cap,
                                                                int(per_row), C.byref(select), int(matches_cap), res[1].data_ptr(),
                                                                res[2].data_ptr(), res[3].data_ptr(), res[0].data_ptr(),
                                                                C.c_void_p(stream) if stream else None))
        return res

    def pair_matches_download(self, out_triple, per_row, select, dst, stream=None):
        """brisk_hip_pair_matches_download: selection + transfer of out_triple's matches into `dst` (HostMatches) queued on `stream`
        (the stream the matcher ran on); out_triple may be overwritten by the next batch in stream order.  Returns the ticket."""
        m, cnt, rows = out_triple
        t = C.c_uint()
        self.check(self._L.brisk_hip_pair_matches_download(self._h, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), int(cnt.shape[0]),
                                                           int(cnt.shape[1]), int(per_row), C.byref(select), C.byref(dst.struct),
                                                           C.c_void_p(stream) if stream else None, C.byref(t)))
        return t.value

    def pair_matches_wait(self, ticket, check=True):
        """completes transfer `ticket`; returns the number of flagged pairs (check=False: (rc, flagged) instead of raising)"""
        n = C.c_int()
        rc = self._L.brisk_hip_pair_matches_wait(self._h, ticket, C.byref(n))
        if not check:
            return rc, n.value
        self.check(rc)
        return n.value

    # -- a batch's pair matches checked against a model of the pair --
    @staticmethod
    def _pair_lists(n, out_cap, dev):
        """the five device tensors the pair-model calls return: matches, counts, flags, offsets, models"""
        import torch
        n = max(n, 0)
        return (torch.empty((max(int(out_cap), 0), 4), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev),
                torch.empty((n, 12), dtype=torch.int64, device=dev))

    def _pair_models_call(self, fn, query, train, pairs, rows_cap, offsets, matches, rule, out_cap, query_kps, train_kps, stream, models=()):
        """what the two verifiers and the refit share.  fn: the entry point; rule: its PairVerify or PairRefit; models: the
        arguments in front of it (the refit's input models)"""
        n, in_cap = int(pairs.npairs), int(matches.shape[0])
        if out_cap is None:
            out_cap = in_cap
        query_kps, train_kps = self._kp_sets(query_kps, train_kps)
        res = self._pair_lists(n, out_cap, matches.device)
        self.check(fn(self._h, C.byref(query), C.byref(train), C.byref(query_kps), C.byref(train_kps), C.byref(pairs), int(rows_cap),
                      offsets.data_ptr(), matches.data_ptr(), in_cap, *models, C.byref(rule), int(out_cap), res[4].data_ptr(),
                      res[1].data_ptr(), res[2].data_ptr(), res[3].data_ptr(), res[0].data_ptr(), C.c_void_p(stream) if stream else None))
        return res

    # -- a batch's pair matches checked against a homography --
    def verify_pair_matches(self, query, train, pairs, rows_cap, offsets, matches, verify, out_cap=None, query_kps=None, train_kps=None,
                            stream=None):
        """brisk_hip_verify_pair_matches_device on what select_pair_matches returned for these pairs (offsets [npairs + 1], matches
        [in_cap, 4]: in_cap = the selection's matches_cap).  query / train: DescSet (the row counts); pairs: PairSpec; verify: a
        PairVerify; query_kps / train_kps: KpSet (None = the last batch's); out_cap None = in_cap.  Returns the device tensors
        (matches [out_cap, 4] int32 - the kept DMATCH records, in order -, counts [npairs], flags [npairs], offsets [npairs + 1]
        int64, models [npairs, 12] int64 - PAIR_MODEL records); the first four are what link_tracks and the exits take.
        Asynchronous on `stream`."""
        return self._pair_models_call(self._L.brisk_hip_verify_pair_matches_device, query, train, pairs, rows_cap, offsets, matches, verify,
                                      out_cap, query_kps, train_kps, stream)

    # -- a batch's pair matches checked against an epipolar geometry --
    def verify_pair_matches_epipolar(self, query, train, pairs, rows_cap, offsets, matches, verify, out_cap=None, query_kps=None,
                                     train_kps=None, stream=None):
        """brisk_hip_verify_pair_matches_epipolar_device: verify_pair_matches with an eight-point fundamental matrix in the
        homography's place, for scenes with depth (left against right, a moving camera).  The arguments are verify_pair_matches';
        verify: a PairVerify whose max_error is the Sampson distance in pixels and whose min_inliers is >= 8.  Returns the same
        five device tensors; models [npairs, 12] int64 holds PAIR_EPIPOLAR_MODEL records - not homographies: they are not for
        refit_pair_models or the guided matchers.  Asynchronous on `stream`."""
        return self._pair_models_call(self._L.brisk_hip_verify_pair_matches_epipolar_device, query, train, pairs, rows_cap, offsets, matches,
                                      verify, out_cap, query_kps, train_kps, stream)

    # -- each pair's homography fitted again to all its inliers --
    def refit_pair_models(self, query, train, pairs, rows_cap, offsets, matches, models, refit, out_cap=None, query_kps=None, train_kps=None,
                          stream=None):
        """brisk_hip_refit_pair_models_device behind verify_pair_matches.  offsets / matches: what the VERIFIER was given (the
        selection's output), not what it returned; models: the models tensor it returned ([npairs, 12] int64, PAIR_MODEL records) or
        a device pointer to npairs records; refit: a PairRefit.  Everything else, and what is returned (matches, counts, flags,
        offsets, models), as verify_pair_matches.  Asynchronous on `stream`."""
        ptr = models.data_ptr() if hasattr(models, "data_ptr") else models
        return self._pair_models_call(self._L.brisk_hip_refit_pair_models_device, query, train, pairs, rows_cap, offsets, matches, refit,
                                      out_cap, query_kps, train_kps, stream, models=(C.c_void_p(int(ptr)) if ptr else None,))

    # -- each pair's fundamental matrix fitted again to all its inliers, rank 2 enforced --
    def refit_pair_models_epipolar(self, query, train, pairs, rows_cap, offsets, matches, models, refit, out_cap=None, query_kps=None,
                                   train_kps=None, stream=None):
        """brisk_hip_refit_pair_models_epipolar_device behind verify_pair_matches_epipolar: refit_pair_models for the epipolar branch.
        offsets / matches: what the VERIFIER was given (the selection's output); models: the models tensor it returned ([npairs, 12]
        int64, PAIR_EPIPOLAR_MODEL records) or a device pointer to npairs records; refit: a PairEpipolarRefit.  Returns (matches,
        counts, flags, offsets, models) as verify_pair_matches_epipolar; a record with PAIR_REFIT in its flags holds the refitted F
        (rank 2 if refit.rank2), any other still the verifier's.  The epipolar-guided matchers take the models in place.
        Asynchronous on `stream`."""
        ptr = models.data_ptr() if hasattr(models, "data_ptr") else models
        return self._pair_models_call(self._L.brisk_hip_refit_pair_models_epipolar_device, query, train, pairs, rows_cap, offsets, matches,
                                      refit, out_cap, query_kps, train_kps, stream, models=(C.c_void_p(int(ptr)) if ptr else None,))

    # -- a batch's pair matches linked into feature tracks --
    @staticmethod
    def _node_rows(node_rows):
        """(device pointer, stride in ints) of a chain's row counts: a (tensor, stride) pair, or a (DescSet, first, step) triple -
        the frames first + i * step of the set"""
        if len(node_rows) == 3:
            st, first, step = node_rows
            return int(st.d_counts) + 4 * int(first) * int(st.count_stride), int(step) * int(st.count_stride)
        t, stride = node_rows
        return t.data_ptr(), int(stride)

    def link_tracks(self, node_rows, nodes, rows_cap, offsets, matches, seed=None, stream=None):
        """brisk_hip_link_tracks_device.  node_rows: (int32 device tensor, stride) or (DescSet, first, step); offsets / matches: what
        select_pair_matches returned for the chain's nodes - 1 pairs (None with nodes == 1); seed: a TrackSeed.  Returns the device
        tensors (prev [nodes, rows_cap] int32, track [nodes, rows_cap] int64, age [nodes, rows_cap] int32, summary [8] int64); only
        the rows below each node's count are written.  Asynchronous on `stream`."""
        import torch
        ptr, stride = self._node_rows(node_rows)
        dev = "cuda:%d" % self.device
        shape = (int(nodes), int(rows_cap))
        res = (torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.int64, device=dev),
               torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(8, dtype=torch.int64, device=dev))
        self.check(self._L.brisk_hip_link_tracks_device(self._h, ptr, stride, int(nodes), int(rows_cap),
                                                        None if offsets is None else offsets.data_ptr(),
                                                        None if matches is None else matches.data_ptr(),
                                                        C.byref(seed) if seed is not None else None, res[0].data_ptr(), res[1].data_ptr(),
                                                        res[2].data_ptr(), res[3].data_ptr(), C.c_void_p(stream) if stream else None))
        return res

    def list_tracks(self, node_rows, nodes, rows_cap, prev, track, age, min_len, tracks_cap=None, obs_cap=None, stream=None):
        """brisk_hip_list_tracks_device on what link_tracks returned.  tracks_cap / obs_cap None = everything fits (nodes * rows_cap).
        Returns the device tensors (list_track [tracks_cap] int64, list_len [tracks_cap] int32, list_offsets [tracks_cap + 1] int64,
        list_obs [obs_cap, 2] int32 - {node, row} records -, summary [4] int64: pieces listed, their observations, pieces stored,
        flags).  Asynchronous on `stream`."""
        import torch
        ptr, stride = self._node_rows(node_rows)
        if tracks_cap is None:
            tracks_cap = int(nodes) * int(rows_cap)
        if obs_cap is None:
            obs_cap = int(nodes) * int(rows_cap)
        dev, tc, oc = prev.device, max(int(tracks_cap), 0), max(int(obs_cap), 0)
        res = (torch.empty(tc, dtype=torch.int64, device=dev), torch.empty(tc, dtype=torch.int32, device=dev),
               torch.empty(tc + 1, dtype=torch.int64, device=dev), torch.empty((oc, 2), dtype=torch.int32, device=dev),
               torch.empty(4, dtype=torch.int64, device=dev))
        self.check(self._L.brisk_hip_list_tracks_device(self._h, ptr, stride, int(nodes), int(rows_cap), prev.data_ptr(), track.data_ptr(),
                                                        age.data_ptr(), int(min_len), int(tracks_cap), int(obs_cap), res[0].data_ptr(),
                                                        res[1].data_ptr(), res[2].data_ptr(), res[3].data_ptr(), res[4].data_ptr(),
                                                        C.c_void_p(stream) if stream else None))
        return res

    # -- the tracker's exit: the listed tracks with their keypoints --
    def track_points(self, node_rows, nodes, rows_cap, list_offsets, list_obs, list_summary, kps=None, kp_first=0, kp_step=1, stream=None):
        """brisk_hip_track_points_device on what list_tracks returned (list_offsets, list_obs, list_summary).  kps: a KpSet (None =
        the last batch's); node i's keypoints are frame kp_first + i * kp_step of it.  Returns the device tensor points [obs_cap, 9]
        int32 - TRACK_POINT records -; only the points of the stored observations are written.  Asynchronous on `stream`, ordered
        behind the context's previous call and in front of its next (the next batch overwrites the keypoints), whichever streams
        those use."""
        import torch
        ptr, stride = self._node_rows(node_rows)
        if kps is None:
            kps = self.batch_kp_set()
        cap = int(list_obs.shape[0])
        points = torch.empty((cap, 9), dtype=torch.int32, device=list_obs.device)
        self.check(self._L.brisk_hip_track_points_device(self._h, ptr, stride, int(nodes), int(rows_cap), list_offsets.data_ptr(),
                                                         list_obs.data_ptr(), list_summary.data_ptr(), cap, C.byref(kps), int(kp_first),
                                                         int(kp_step), points.data_ptr(), C.c_void_p(stream) if stream else None))
        return points

    def tracks_download(self, node_rows, nodes, rows_cap, prev, track, age, min_len, dst, kps=None, kp_first=0, kp_step=1, stream=None):
        """brisk_hip_tracks_download: list + points + transfer of what link_tracks returned into `dst` (HostTrackList) queued on
        `stream` (the stream link_tracks ran on); prev / track / age and the keypoints may be overwritten by the next batch in
        stream order.  kps / kp_first / kp_step as in track_points.  Returns the ticket."""
        ptr, stride = self._node_rows(node_rows)
        if kps is None:
            kps = self.batch_kp_set()
        t = C.c_uint()
        self.check(self._L.brisk_hip_tracks_download(self._h, ptr, stride, int(nodes), int(rows_cap), prev.data_ptr(), track.data_ptr(),
                                                     age.data_ptr(), int(min_len), C.byref(kps), int(kp_first), int(kp_step),
                                                     C.byref(dst.struct), C.c_void_p(stream) if stream else None, C.byref(t)))
        return t.value

    def tracks_wait(self, ticket, check=True):
        """completes transfer `ticket`; returns 1 when the list was cut, else 0 (check=False: (rc, cut) instead of raising)"""
        n = C.c_int()
        rc = self._L.brisk_hip_tracks_wait(self._h, ticket, C.byref(n))
        if not check:
            return rc, n.value
        self.check(rc)
        return n.value

    def match_radius_device(self, d_query, nq, q_pitch, d_train, nt, t_pitch, dim_bytes, max_distance, cap_per_query, d_out, d_out_count,
                            stream=None):
        """brisk_hip_match_radius_device: device pointers (ints), host counts; d_out [nq][cap_per_query] DMATCH records, d_out_count
        [nq] = matches found.  Asynchronous on `stream` (None = the context's)."""
        self.check(self._L.brisk_hip_match_radius_device(self._h, d_query, int(nq), int(q_pitch), d_train, int(nt), int(t_pitch), int(dim_bytes),
                                                         float(max_distance), int(cap_per_query), d_out, d_out_count,
                                                         C.c_void_p(stream) if stream else None))


class Pool:
    """brisk_hip_pool: the one-frame calls of many threads combined into batches (thread-safe, blocking calls)"""

    def __init__(self, device=0, max_batch=16, max_keypoints=16384):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.brisk_hip_pool_create(device, max_batch, max_keypoints, C.byref(h))
        if rc:
            raise BriskHipError(rc, "brisk_hip_pool_create failed")
        self._h = h

    def _check(self, rc):
        if rc:
            raise BriskHipError(rc, self._L.brisk_hip_pool_last_error(self._h).decode())

    def detect(self, image, threshold, octaves, capacity=16384):
        """-> (keypoints, token of the frame's device copy)"""
        img = np.ascontiguousarray(image, np.uint8)
        h, w = img.shape
        out = np.empty(capacity, KEYPOINT)
        n, tok = C.c_int(), C.c_ulonglong()
        self._check(self._L.brisk_hip_pool_detect(self._h, _ptr(img), w, h, w, threshold, octaves, _ptr(out), capacity, C.byref(n), C.byref(tok)))
        return _kcopy(out, n.value), tok.value

    def describe(self, pattern, image, keypoints, token=0, rotation_invariant=True, scale_invariant=True):
        img = np.ascontiguousarray(image, np.uint8)
        h, w = img.shape
        k = _kcopy(np.ascontiguousarray(keypoints, KEYPOINT))
        n = C.c_int(len(k))
        s = pattern.descriptorSize()
        desc = np.empty((max(len(k), 1), s), np.uint8)
        if len(k) == 0:
            k = np.zeros(1, KEYPOINT)
        self._check(self._L.brisk_hip_pool_describe(self._h, pattern._h, _ptr(img), w, h, w, _ptr(k), C.byref(n), _ptr(desc), s,
                                                    int(rotation_invariant), int(scale_invariant), token))
        return k[:n.value], desc[:n.value]

    def stats(self):
        """(groups run, calls they carried)"""
        g, c = C.c_ulonglong(), C.c_ulonglong()
        self._L.brisk_hip_pool_stats(self._h, C.byref(g), C.byref(c))
        return g.value, c.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.brisk_hip_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


class BriskFeatureDetector:
    """Mirror of brisk::BriskFeatureDetector (brisk/include/brisk/brisk-feature-detector.h:51-83)."""

    def __init__(self, thresh, octaves=3, suppressScaleNonmaxima=True, context=None, uniformityRadius=0.0,
                 maxNumKpt=0x7FFFFFFF, numBucketsU=0, numBucketsV=0):
        self.threshold = int(thresh)
        self.octaves = int(octaves)
        self.m_suppressScaleNonmaxima = bool(suppressScaleNonmaxima)
        # engine option (not reference behaviour of this class): EnforceKeyPointUniformity as a post-filter
        self.uniformityRadius, self.maxNumKpt = float(uniformityRadius), int(maxNumKpt)
        # engine option as well: KeyPointBucketing (what the reference's ScaleSpaceLayer uses while uniformity is off)
        self.numBucketsU, self.numBucketsV = int(numBucketsU), int(numBucketsV)
        self._ctx = context or default_context()

    def detect(self, image, mask=None, capacity=16384):
        """detectImpl (brisk-feature-detector.cc:77-85): returns the keypoints (KEYPOINT array)."""
        img = np.ascontiguousarray(image)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("image must be a 2-D uint8 array (CV_8UC1)")
        h, w = img.shape
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            if m.shape != img.shape:
                raise ValueError("mask must have the image's shape")
        out = np.empty(capacity, KEYPOINT)   # (records [0, n) are written by the call)
        n = C.c_int()
        c = self._ctx
        # the object's post-filter settings travel with the call (the context's own settings are neither used nor changed)
        pf = PostFilter(self.uniformityRadius, self.maxNumKpt, self.numBucketsU, self.numBucketsV, self.maxNumKpt)
        c.check(c._L.brisk_hip_detect_filtered(c._h, _ptr(img), w, h, w, self.threshold, self.octaves,
                                               int(self.m_suppressScaleNonmaxima), _ptr(m), w if m is not None else 0,
                                               C.byref(pf), _ptr(out), capacity, C.byref(n)))
        return _kcopy(out, n.value)


    def ComputeScale(self, image, keypoints, capacity=None):
        """ComputeScale (brisk-feature-detector.cc:87-92): returns the keypoints GetKeypoints produces for the provided
        ones (the reference replaces the vector's contents)."""
        img = np.ascontiguousarray(image)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("image must be a 2-D uint8 array (CV_8UC1)")
        h, w = img.shape
        k = np.ascontiguousarray(keypoints, KEYPOINT)
        layers = 1 if self.octaves == 0 else 2 * self.octaves
        cap = capacity or (len(k) * layers + 65536)
        c = self._ctx
        c.reserve(65536, max(len(k), cap))
        out = np.zeros(cap, KEYPOINT)
        n = C.c_int()
        c.check(c._L.brisk_hip_compute_scale(c._h, _ptr(img), w, h, w, self.threshold, self.octaves,
                                             int(self.m_suppressScaleNonmaxima), _ptr(k) if len(k) else None, len(k),
                                             _ptr(out), cap, C.byref(n)))
        return _kcopy(out, n.value)


class BriskDescriptorExtractor:
    """Mirror of brisk::BriskDescriptorExtractor (brisk/include/brisk/brisk-descriptor-extractor.h:54-202)."""
    briskV1 = 1
    briskV2 = 2
    kDescriptorLength = 384

    def __init__(self, rotationInvariant=True, scaleInvariant=True, version=2, patternScale=1.0, fname=None,
                 pattern_text=None, context=None):
        self.rotationInvariance = bool(rotationInvariant)
        self.scaleInvariance = bool(scaleInvariant)
        self._ctx = c = context or default_context()
        h = C.c_void_p()
        if fname is not None:
            pattern_text = open(fname).read()
        if pattern_text is not None:
            c.check(c._L.brisk_hip_pattern_create_from_text(c._h, pattern_text.encode(), patternScale, C.byref(h)))
        else:
            if version not in (1, 2):
                raise RuntimeError("only Version::briskV1 or Version::briskV2 supported!")
            c.check(c._L.brisk_hip_pattern_create(c._h, version, patternScale, C.byref(h)))
        self._h = h

    def descriptorSize(self):
        return self._ctx._L.brisk_hip_pattern_descriptor_size(self._h)

    @property
    def points(self):
        """number of pattern points (60 for briskV1, 66 for briskV2)"""
        return self._ctx._L.brisk_hip_pattern_points(self._h)

    def descriptorType(self):
        return 0  # CV_8U

    def tables(self):
        a, b, t = np.zeros(64, np.float32), np.zeros(64, np.int32), np.zeros(64, np.float32)
        self._ctx.check(self._ctx._L.brisk_hip_pattern_tables(self._h, _ptr(a), _ptr(b), _ptr(t)))
        return a, b, t

    def compute(self, image, keypoints, same_image=False):
        """compute() (brisk-descriptor-extractor.cc:612-778): returns (filtered keypoints, descriptors).
        same_image: the caller states that `image` is the very buffer the context's last detect() call was given and
        that it has not changed (brisk_hip_describe_same_image: no second upload)."""
        img = np.ascontiguousarray(image)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise RuntimeError("Unsupported image format. Must be CV_16UC1 or CV_8UC1.")  # :678 (8-bit only here)
        h, w = img.shape
        k = _kcopy(np.ascontiguousarray(keypoints, KEYPOINT))
        n = C.c_int(len(k))
        s = self.descriptorSize()
        desc = np.empty((max(len(k), 1), s), np.uint8)   # (rows [0, n) are written by the call, the others dropped below)
        if len(k) == 0:
            k = np.zeros(1, KEYPOINT)
        c = self._ctx
        fn = c._L.brisk_hip_describe_same_image if same_image else c._L.brisk_hip_describe
        c.check(fn(c._h, self._h, _ptr(img), w, h, w, _ptr(k), C.byref(n), _ptr(desc), s,
                   int(self.rotationInvariance), int(self.scaleInvariance)))
        return k[:n.value], desc[:n.value]

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._ctx._L.brisk_hip_pattern_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])  # cv::DMatch


class BruteForceMatcher:
    """Mirror of brisk::BruteForceMatcher with brisk::Hamming (brisk/include/brisk/brute-force-matcher.h:52-93,
    brisk/src/brute-force-matcher.cc:80-213): add() train descriptor sets, then knnMatch / radiusMatch / match.
    Matches come back as one structured array (DMATCH) per query, ordered by (distance, imgIdx, trainIdx)."""

    def __init__(self, context=None):
        self.ctx = context or default_context()
        self.trainDescCollection = []

    def add(self, descriptors):
        for d in (descriptors if isinstance(descriptors, (list, tuple)) else [descriptors]):
            self.trainDescCollection.append(np.ascontiguousarray(d, np.uint8))

    def clear(self):
        self.trainDescCollection = []

    def empty(self):
        return not self.trainDescCollection

    def isMaskSupported(self):
        return True

    def _args(self, query, masks):
        query = np.ascontiguousarray(query, np.uint8)
        if query.ndim != 2:
            raise ValueError("descriptors must be a 2-D uint8 array")
        train = self.trainDescCollection
        nimg = len(train)
        for t in train:
            if t.ndim != 2 or (t.shape[0] and t.shape[1] != query.shape[1]):
                raise ValueError("train descriptors must have the query's descriptor size")
        tptr = (C.c_void_p * max(nimg, 1))(*[t.ctypes.data for t in train])
        ntr = np.array([t.shape[0] for t in train] + [0], np.int32)
        tpitch = np.array([t.strides[0] if t.shape[0] else query.shape[1] for t in train] + [0], np.int32)
        mptr, mpitch, keep = None, None, []
        if masks is not None:
            if len(masks) != nimg:
                raise ValueError("one mask (or None) per train image")
            ms = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in masks]
            for m, t in zip(ms, train):
                if m is not None and m.shape != (query.shape[0], t.shape[0]):
                    raise ValueError("mask must be queries x train descriptors")
            keep = ms
            mptr = (C.c_void_p * max(nimg, 1))(*[None if m is None else m.ctypes.data for m in ms])
            mpitch = np.array([0 if m is None else m.strides[0] for m in ms] + [0], np.int32)
        return query, nimg, tptr, ntr, tpitch, mptr, mpitch, keep

    def knnMatch(self, queryDescriptors, k, masks=None, compactResult=False):
        q, nimg, tptr, ntr, tpitch, mptr, mpitch, keep = self._args(queryDescriptors, masks)
        nq = q.shape[0]
        out = np.zeros((nq, max(k, 1)), DMATCH)
        cnt = np.zeros(max(nq, 1), np.int32)
        L = self.ctx._L
        self.ctx.check(L.brisk_hip_match_knn(self.ctx._h, _ptr(q), nq, q.strides[0] if nq else q.shape[1], q.shape[1], nimg,
                                             tptr, _ptr(ntr), _ptr(tpitch), mptr, None if mpitch is None else _ptr(mpitch),
                                             k, _ptr(out), _ptr(cnt)))
        rows = [out[i, :cnt[i]].copy() for i in range(nq)]
        return [r for r in rows if len(r)] if compactResult else rows

    def radiusMatch(self, queryDescriptors, maxDistance, masks=None, compactResult=False):
        q, nimg, tptr, ntr, tpitch, mptr, mpitch, keep = self._args(queryDescriptors, masks)
        nq = q.shape[0]
        L = self.ctx._L
        cap = 64
        while True:
            out = np.zeros((nq, cap), DMATCH)
            cnt = np.zeros(max(nq, 1), np.int32)
            self.ctx.check(L.brisk_hip_match_radius(self.ctx._h, _ptr(q), nq, q.strides[0] if nq else q.shape[1], q.shape[1],
                                                    nimg, tptr, _ptr(ntr), _ptr(tpitch), mptr,
                                                    None if mpitch is None else _ptr(mpitch), float(maxDistance), cap,
                                                    _ptr(out), _ptr(cnt)))
            need = int(cnt[:nq].max()) if nq else 0
            if need <= cap:
                break
            cap = need
        rows = [out[i, :cnt[i]].copy() for i in range(nq)]
        return [r for r in rows if len(r)] if compactResult else rows

    def match(self, queryDescriptors, masks=None):
        """cv::DescriptorMatcher::match: the best match of every query (queries without one are dropped)."""
        rows = self.knnMatch(queryDescriptors, 1, masks, compactResult=True)
        return np.concatenate(rows) if rows else np.zeros(0, DMATCH)
