/*
 * brisk_hip.h - C ABI of the MI355X-native BRISK detect+describe engine (libbrisk_hip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  The two host classes
 * brisk::BriskFeatureDetector / brisk::BriskDescriptorExtractor (include/brisk/, mirroring the
 * reference headers) are thin wrappers over these entry points, and a maintainer of the reference
 * would bind exactly these from brisk-feature-detector.cc / brisk-descriptor-extractor.cc
 * (see INTEGRATION.md).  Reference paths below are relative to the ethzasl_brisk tree.
 *
 * All functions return BRISK_HIP_OK (0) or an error code; brisk_hip_last_error() gives the text.
 * There is no CPU fallback: without a HIP device every compute entry point fails with
 * BRISK_HIP_ERR_NO_DEVICE.
 */
#ifndef BRISK_HIP_H_
#define BRISK_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  BRISK_HIP_OK = 0,
  BRISK_HIP_ERR_ARG = 1,        /* null pointer / non-positive size / bad enum */
  BRISK_HIP_ERR_NO_DEVICE = 2,  /* no usable HIP device */
  BRISK_HIP_ERR_HIP = 3,        /* a HIP runtime call failed */
  BRISK_HIP_ERR_CAPACITY = 4,   /* more candidates / keypoints than the configured capacity */
  BRISK_HIP_ERR_THRESHOLD = 5,  /* AGAST threshold outside [1, 255] (below 20 some frames run the ordered path) */
  BRISK_HIP_ERR_PATTERN = 6,    /* malformed pattern (reference: CHECK_EQ(noShortPairs_, 384), :286) */
  BRISK_HIP_ERR_UNSUPPORTED = 7 /* no defined result in the reference on this input (see brisk_hip_detect), or an unsupported size */
};

/* Binary-identical to cv::KeyPoint {Point2f pt; float size, angle, response; int octave, class_id;} */
typedef struct brisk_hip_keypoint {
  float x, y, size, angle, response;
  int octave, class_id;
} brisk_hip_keypoint;

typedef struct brisk_hip_ctx brisk_hip_ctx;          /* device workspace + stream          */
typedef struct brisk_hip_pattern brisk_hip_pattern;  /* sampling pattern tables (extractor) */

/* ---- context ------------------------------------------------------------------------------- */
/* device: HIP device ordinal.  Buffers are sized lazily for the largest (w, h, octaves, batch) seen.  The calls of one
 * context are serialised (mutex) and share one workspace: every call orders its stream behind the previous call's work,
 * whichever stream that ran on.  For concurrency use one context per host thread (what include/brisk/hip-context.h
 * does); pattern handles are plain device tables and may be shared by all contexts of a device. */
int brisk_hip_create(int device, brisk_hip_ctx** out);
void brisk_hip_destroy(brisk_hip_ctx* ctx);
const char* brisk_hip_last_error(const brisk_hip_ctx* ctx);
/* per-frame capacities: AGAST candidates (default 65536) and keypoints (default 16384; below 2^23) */
int brisk_hip_set_capacity(brisk_hip_ctx* ctx, int max_candidates, int max_keypoints);
int brisk_hip_device_count(void);
/* CPUs the process may use (affinity mask, cut by a cgroup quota).  A one-frame call POLLS for its results while fewer threads
 * than that are polling (a wake-up costs more than the call's tail) and sleeps on a blocking event otherwise; the classes of
 * include/brisk/ hand calls to the device's shared pool from more concurrent callers than CPUs on. */
int brisk_hip_usable_cpus(void);
/* raises the capacities to at least these values; never lowers them (no reallocation for smaller requests) */
int brisk_hip_reserve(brisk_hip_ctx* ctx, int min_candidates, int min_keypoints);

/* Page-locks a caller's host buffer (an image, a frame ring, result arrays) so that the device reads / writes it directly:
 * hipHostRegister / hipHostUnregister for callers that do not link the HIP runtime themselves.  A registered image is
 * uploaded by DMA straight from the buffer (a pageable one goes through the runtime's staging copies, on the calling
 * thread); registered result arrays make brisk_hip_batch_download_all write them without a bounce buffer.  The buffer must
 * be unregistered before it is freed.  Registration costs ~0.1 ms per MB: register buffers that are reused. */
int brisk_hip_host_register(void* ptr, size_t bytes);
int brisk_hip_host_unregister(void* ptr);

/* ---- pattern: replaces the BriskDescriptorExtractor constructors ---------------------------- */
/* brisk-descriptor-extractor.cc:293-343: version 2 = built-in 66-point pattern (InitFromStream :180-291),
 * version 1 = generated 60-point BRISK 1.0 kernel (generateKernel :65-178, 512 bits). */
int brisk_hip_pattern_create(brisk_hip_ctx* ctx, int version, float pattern_scale, brisk_hip_pattern** out);
/* :345-367: pattern file contents (.ptn syntax: N, N x {x y sigma}, S, S x {i j}, L, L x {i j}) */
int brisk_hip_pattern_create_from_text(brisk_hip_ctx* ctx, const char* ptn_text, float pattern_scale,
                                       brisk_hip_pattern** out);
void brisk_hip_pattern_destroy(brisk_hip_pattern* p);
int brisk_hip_pattern_descriptor_size(const brisk_hip_pattern* p); /* descriptorSize() :780-782 (48; 64 for briskV1; 16 ... 224 for briskV1 at other pattern scales) */
int brisk_hip_pattern_points(const brisk_hip_pattern* p);
/* host copies of the derived tables, for inspection / tests: 64 entries each */
int brisk_hip_pattern_tables(const brisk_hip_pattern* p, float* scale_list, int* size_list, float* size_thresh);

/* ---- host-buffer calls: what the two host classes forward to --------------------------------- */
/* BriskFeatureDetector::detectImpl (brisk-feature-detector.cc:77-85): clears/overwrites `out`.
 * img: h x w u8, row pitch `stride` bytes.  mask: optional h x w u8 (0 = drop keypoint), or NULL.
 * threshold: 1..255 (20..255 on the fast path; below 20 a frame in which a detection stores a score <= 2 - nearly every
 * frame below 10, few at 10..19 - takes the sequential ordered path, bit-exact but slow: ~19 us per AGAST candidate).
 * suppress_scale_nonmaxima = 0 (brisk-scale-space.cc:131-170): with octaves == 0 the single-layer 2-D refinement; with
 * more layers the reference takes every layer's point coordinates from layer 0's list (`agastPoints.at(0)[n]`, :137) -
 * reproduced on the ordered path; where that indexing leaves layer 0's list or a score matrix (the usual case for
 * ordinary images: undefined behaviour in the reference) the call fails with BRISK_HIP_ERR_UNSUPPORTED.
 * out: capacity `cap` keypoints; *n receives the count (BRISK_HIP_ERR_CAPACITY if cap is too small). */
int brisk_hip_detect(brisk_hip_ctx* ctx, const uint8_t* img, int w, int h, int stride, int threshold, int octaves,
                     int suppress_scale_nonmaxima, const uint8_t* mask, int mask_stride, brisk_hip_keypoint* out,
                     int cap, int* n);
/* The same call with the uniformity post-filter (see brisk_hip_set_uniformity) given per call instead of as context
 * state: uniformity_radius 0 = off, else >= 1; at most max_keypoints keypoints are kept.  Nothing of the context's
 * settings applies to this call: with radius 0 it returns the unfiltered detections even if brisk_hip_set_uniformity /
 * brisk_hip_set_bucketing are set on the context (those are for the batch path and brisk_hip_detect). */
int brisk_hip_detect_uniform(brisk_hip_ctx* ctx, const uint8_t* img, int w, int h, int stride, int threshold, int octaves,
                             int suppress_scale_nonmaxima, const uint8_t* mask, int mask_stride, double uniformity_radius,
                             int max_keypoints, brisk_hip_keypoint* out, int cap, int* n);
/* The same call with BOTH optional post-filters given per call: nothing is read from or written to the context's settings
 * (brisk_hip_set_uniformity / brisk_hip_set_bucketing), so detector objects with different settings can share a
 * context.  uniformity_radius 0 = off, else >= 1; bucketing takes effect while uniformity is off, (0, 0) buckets = off. */
typedef struct brisk_hip_postfilter {
  double uniformity_radius;
  int uniformity_max_keypoints;
  int num_buckets_u, num_buckets_v, bucket_max_keypoints;
} brisk_hip_postfilter;
int brisk_hip_detect_filtered(brisk_hip_ctx* ctx, const uint8_t* img, int w, int h, int stride, int threshold, int octaves,
                              int suppress_scale_nonmaxima, const uint8_t* mask, int mask_stride,
                              const brisk_hip_postfilter* pf, brisk_hip_keypoint* out, int cap, int* n);
/* BriskFeatureDetector::ComputeScale (brisk-feature-detector.cc:87-92; brisk-scale-space.cc:104-123 and the branches
 * behind it): scores / scales for PROVIDED keypoints on a pyramid with lower threshold 0.  Every provided keypoint yields
 * up to one output per layer that admits it (layer order, provided order inside a layer; class_id is kept).  Sequential
 * on the device - one lane per (layer, provided point): the walk's phases are order-free among themselves (3 000 points on a
 * 1080p frame: 0.6 ms); a call in which some layer admits no provided point, and therefore detects, runs the reference's
 * sequential walk on one lane -, parity unpinned (nothing in the reference exercises this entry).
 * BRISK_HIP_ERR_UNSUPPORTED where the reference has no defined result: a provided point in the last admitted rows of a
 * layer (within about 5 rows x the layer's scale of the bottom border) makes the reference read beyond the image.
 * in: n_in keypoints (only x, y and the copied-through fields matter); out: capacity cap; *n receives the count. */
int brisk_hip_compute_scale(brisk_hip_ctx* ctx, const uint8_t* img, int w, int h, int stride, int threshold, int octaves,
                            int suppress_scale_nonmaxima, const brisk_hip_keypoint* in, int n_in, brisk_hip_keypoint* out,
                            int cap, int* n);
/* BriskDescriptorExtractor::compute (brisk-descriptor-extractor.cc:612-778): filters `kps` in place
 * (border test), fills kps[i].angle, writes *n rows of descriptorSize() bytes at pitch desc_stride. */
int brisk_hip_describe(brisk_hip_ctx* ctx, const brisk_hip_pattern* pat, const uint8_t* img, int w, int h, int stride,
                       brisk_hip_keypoint* kps, int* n, uint8_t* desc, int desc_stride, int rotation_invariant,
                       int scale_invariant);
/* The same call for the usual detect() -> compute() pair on one image (test-binary-equal.cc:215,237): the caller STATES
 * that `img` is the buffer the context's last brisk_hip_detect / _detect_uniform call was given and that its pixels have
 * not changed since.  The upload and the layer-0 pass are then skipped (the device still holds the image).  If pointer,
 * size or stride differ from that call's, or another call used the context in between, the image is uploaded as in
 * brisk_hip_describe.  A caller whose pixels DID change gets the descriptors of the old pixels: brisk_hip_describe never
 * makes that assumption (it always uploads, as the reference's compute() always reads the current pixels), unless the
 * environment opts in with BRISK_HIP_IMAGE_CACHE=1 - the buffer is then recognised by pointer, size, stride and a 64-bit
 * hash over one 8-byte word per 128 bytes of every row, and a change that avoids every sampled word (a small overlay, rows
 * narrower than 8 + the row's phase) goes unnoticed. */
int brisk_hip_describe_same_image(brisk_hip_ctx* ctx, const brisk_hip_pattern* pat, const uint8_t* img, int w, int h, int stride,
                                  brisk_hip_keypoint* kps, int* n, uint8_t* desc, int desc_stride, int rotation_invariant,
                                  int scale_invariant);

/* ---- device-resident batch path (frames already in HBM; results stay in HBM) ----------------- */
/* d_frames: nframes images, frame f at d_frames + f*frame_pitch, row pitch row_pitch.  Runs
 * detect (threshold, octaves) then describe (pat) for every frame on `stream` (hipStream_t, may be
 * NULL = the context's stream, a non-blocking stream that is NOT ordered with the legacy default stream: pass
 * your own stream if other work has to be ordered with the batch).  Asynchronous: synchronise the stream before
 * reading results.  The frames must stay unchanged until then: when they already have the pyramid's layer-0 layout
 * (row_pitch = width, a multiple of 64; 16-byte aligned base and frame pitch) every kernel reads them in place
 * instead of from a private copy (the reference clones the image, brisk-scale-space.cc:74; the result is the same). */
int brisk_hip_detect_describe_batch(brisk_hip_ctx* ctx, const brisk_hip_pattern* pat, const uint8_t* d_frames,
                                    int nframes, int w, int h, long frame_pitch, int row_pitch, int threshold,
                                    int octaves, void* stream);
/* Element format of the integral image the descriptor kernels build and sample (IntegralImage8,
 * brisk/include/brisk/internal/integral-image.h:56-161).  The result never depends on it - both forms are bit-equal to
 * the reference wherever the 24-bit form is used at all - only the speed does:
 *   BRISK_HIP_INTEGRAL_AUTO (default)  3-byte elements (values modulo 2^24) in detect + describe batches while the
 *        context's PREVIOUS batch was sparse (at most 3 000 AGAST candidates per megapixel), u32 otherwise and for
 *        descriptor-only calls: a stream's batches look alike, and the sparse ones gain from the smaller image.  The
 *        choice of a call therefore depends on the call before it - a benchmark that wants one form says so:
 *   BRISK_HIP_INTEGRAL_U24 / _U32      that form for every call of the context (U24 only where it is exact: patterns
 *        whose boxes cover fewer than 2^24 / 255 pixels - every built-in one; other patterns use u32).
 * (Test / tuning builds - libbrisk_hip.so with BRISK_HIP_TUNING, include/brisk_hip_debug.h - also know BRISK_INTEGRAL_BITS=24 / 32
 * in the environment and debug bits 18 / 24, which take precedence, and report the format of the last call with
 * brisk_hip_debug_integral_bits; the release library has neither.) */
enum { BRISK_HIP_INTEGRAL_AUTO = 0, BRISK_HIP_INTEGRAL_U24 = 24, BRISK_HIP_INTEGRAL_U32 = 32 };
int brisk_hip_set_integral_format(brisk_hip_ctx* ctx, int format);
/* Host-fed form of the batch (the PCIe-fed stream): h_frames is HOST memory (pinned with hipHostMalloc /
 * hipHostRegister for full speed; pageable memory works but copies synchronously).  The frames are moved in slices of 64
 * into two device staging buffers on a copy stream while the previous slice is computed on the context's stream; the
 * results stay in HBM exactly as after brisk_hip_detect_describe_batch (brisk_hip_batch_results / _download /
 * _status).  Returns when everything is queued; brisk_hip_batch_status synchronises.
 * LIFETIME: the copy stream keeps reading h_frames after the call has returned.  The host frames must stay valid AND
 * unchanged until brisk_hip_batch_status / brisk_hip_batch_download has returned for this batch (or the next call on the
 * context has been synchronised): a caller that refills a pinned ring right after the call gets results from mixed
 * frames, silently. */
int brisk_hip_detect_describe_batch_host(brisk_hip_ctx* ctx, const brisk_hip_pattern* pat, const uint8_t* h_frames,
                                         int nframes, int w, int h, long frame_pitch, int row_pitch, int threshold,
                                         int octaves);
/* detect only / describe only variants of the batch path (roofline + stage timing) */
int brisk_hip_detect_batch(brisk_hip_ctx* ctx, const uint8_t* d_frames, int nframes, int w, int h, long frame_pitch,
                           int row_pitch, int threshold, int octaves, void* stream);
/* Device pointers of the last batch's results.  d_counts: per frame {detected, described} at
 * byte stride *count_stride (ints); keypoints [frame][kp_cap]; descriptors [frame][kp_cap][desc_pitch].  desc_pitch is the
 * pitch of the rows the LAST call wrote - read it after every call, not once: batches write 64-byte rows (more once a
 * pattern with longer descriptors was used on the context), a host-buffer brisk_hip_describe whose destination rows are
 * packed (desc_stride == descriptor size) writes slot 0's rows at that packed pitch (48 for the default pattern). */
int brisk_hip_batch_results(brisk_hip_ctx* ctx, const int** d_detected, const int** d_described, int* count_stride,
                            const brisk_hip_keypoint** d_detected_kps, const brisk_hip_keypoint** d_described_kps,
                            const uint8_t** d_desc, int* kp_cap, int* desc_pitch);
/* Copies one frame's results of the last batch to the host (synchronises). kps/desc may be NULL. */
int brisk_hip_batch_download(brisk_hip_ctx* ctx, int frame, int which /*0 detected, 1 described*/,
                             brisk_hip_keypoint* kps, int cap, int* n, uint8_t* desc, int desc_stride);
/* error / overflow flags of the last batch, OR-ed over frames (0 = clean); synchronises */
int brisk_hip_batch_status(brisk_hip_ctx* ctx, int nframes, int* overflow_flags);

/* ---- the batch path's exit to HOST memory: every frame's results in one asynchronous transfer ------------------------
 * The reference hands a call's results to the caller's std::vector<cv::KeyPoint> and descriptor cv::Mat
 * (brisk-feature-detector.cc:77-85, brisk-descriptor-extractor.cc:601-604); for a batch that is, per frame f, the rows
 * [offsets[f], offsets[f + 1]) of ONE keypoint array and ONE descriptor matrix in the caller's memory - exact prefix sums,
 * no padding rows.  The caller fills in the capacities and the five destination pointers:
 *   counts  [frames]      rows frame f HAS (detected or described keypoints)
 *   flags   [frames]      0 = clean, else the frame's rows are NOT stored: the engine's capacity flags of the frame (bit 0
 *                         candidates, bit 1 ties, bit 2 keypoints: brisk_hip_set_capacity), bit 3 / 4 as brisk_hip_batch_status,
 *                         BRISK_HIP_ROWS_CUT = the frame (and every frame behind it) did not fit rows_cap
 *   offsets [frames + 1]  first row of frame f; offsets[frames] = rows stored
 *   kps     [rows_cap]    desc [rows_cap][desc_stride] (NULL: no descriptors; bytes of a stored row behind the descriptor: 0)
 * Destinations in pinned / registered host memory (hipHostMalloc, hipHostRegister, torch pin_memory) are written by the
 * device directly, the stored rows only; pageable destinations go through a pinned buffer of the context and a host copy
 * inside brisk_hip_batch_download_wait.  4-byte aligned pointers, desc_stride a multiple of 4 and >= the descriptor size. */
#define BRISK_HIP_ROWS_CUT 0x100
typedef struct brisk_hip_batch_host_results {
  int frames_cap;          /* frames the arrays hold: >= the frames of the batch */
  int desc_stride;         /* bytes between descriptor rows */
  long long rows_cap;      /* rows kps / desc hold */
  int* counts;
  int* flags;
  long long* offsets;
  brisk_hip_keypoint* kps;
  uint8_t* desc;
} brisk_hip_batch_host_results;
/* Queues the transfer of the context's LAST batch (which: 0 detected keypoints, 1 described keypoints + descriptors) behind
 * that batch and returns: two small kernels on `stream` (hipStream_t the batch ran on; NULL = the context's stream) pack the
 * rows into a device slab, the transfer itself runs on the context's second stream (where the integral kernel runs beside the detector's
 * tail; a process has four hardware queues: a stream of its own for the transfer would share one) beside whatever the context does next -
 * the next batch may be issued at once.  *ticket names the transfer.  At most two transfers are in flight per context: a
 * third call first completes the oldest (as brisk_hip_batch_download_wait would).  `dst` (the struct) is copied; the arrays
 * it points to must stay valid until the ticket has been waited for. */
int brisk_hip_batch_download_all(brisk_hip_ctx* ctx, int which, const brisk_hip_batch_host_results* dst, void* stream,
                                 unsigned* ticket);
/* Blocks until transfer `ticket` (and every earlier one) is complete; the context's lock is not held while waiting.
 * *frames_flagged = frames whose flags[] entry is non-zero.  BRISK_HIP_OK, or - with the rows of all clean frames in place -
 * BRISK_HIP_ERR_CAPACITY (some frame hit an engine capacity or was cut) / the code brisk_hip_batch_status would give. */
int brisk_hip_batch_download_wait(brisk_hip_ctx* ctx, unsigned ticket, int* frames_flagged);
/* brisk_hip_detect_describe_batch_host followed by brisk_hip_batch_download_all(which = 1) in one call: frames from host
 * memory in, keypoints + descriptors back in host memory, everything queued when the call returns.  The transfer of
 * batch n overlaps the H2D copies and kernels of batch n + 1 (alternate two destination sets). */
int brisk_hip_detect_describe_batch_host_results(brisk_hip_ctx* ctx, const brisk_hip_pattern* pat, const uint8_t* h_frames,
                                                 int nframes, int w, int h, long frame_pitch, int row_pitch, int threshold,
                                                 int octaves, const brisk_hip_batch_host_results* dst, unsigned* ticket);

/* ---- the multi-image overloads of the reference's base classes, as ONE batch -------------------------------------------------
 * cv::FeatureDetector::detect(const vector<Mat>& images, vector<vector<KeyPoint>>& keypoints, ...) and
 * cv::DescriptorExtractor::compute(const vector<Mat>& images, vector<vector<KeyPoint>>& keypoints, vector<Mat>& descriptors), which the
 * reference's classes inherit (brisk-feature-detector.h:51, brisk-descriptor-extractor.h:54), loop over detectImpl / computeImpl;
 * here the images of a call - separate host buffers of ONE size, given as an array of pointers, row pitch `stride` - go through the
 * batch path and come back through brisk_hip_batch_download_all's destination (`dst`, `ticket`: brisk_hip_batch_download_wait).
 * _detect_images: plain detection (suppressScaleNonmaxima = true, no masks); frame f's keypoints = rows [offsets[f], offsets[f + 1]).
 * _describe_images: kps[f] / nkps[f] = the provided keypoints of image f (not modified); the rows of frame f are its border-filtered
 * keypoints with their angles and the descriptors; same_images != 0 is the caller's word (as brisk_hip_describe_same_image) that images[]
 * are the very buffers of the context's last multi-image call, unchanged: the frames are then taken from their device copies (no second
 * upload); a list that is not that list is uploaded.  images must stay valid until the ticket has been waited for (kps / nkps are
 * copied before the call returns).
 * The drop-in classes' vector overloads forward here (include/brisk/). */
int brisk_hip_detect_images(brisk_hip_ctx* ctx, const uint8_t* const* images, int nimages, int w, int h, int stride, int threshold,
                            int octaves, const brisk_hip_batch_host_results* dst, unsigned* ticket);
int brisk_hip_describe_images(brisk_hip_ctx* ctx, const brisk_hip_pattern* pat, const uint8_t* const* images, int nimages, int w, int h,
                              int stride, const brisk_hip_keypoint* const* kps, const int* nkps, int rotation_invariant,
                              int scale_invariant, int same_images, const brisk_hip_batch_host_results* dst, unsigned* ticket);

/* ---- call combining: the one-frame host calls of MANY threads as batches ------------------------------------------------
 * The reference's classes are re-entrant (detectImpl is const and builds its state per call, brisk-feature-detector.cc:77-85);
 * with a context per thread every call is ~15 kernel launches and 2 - 4 copies of its own, and the HIP runtime serialises the
 * API calls of a process - 16 threads get 3.6 x one thread.  A pool runs the calls that are inside it at the same
 * time as ONE batch: every caller copies its frame into a pinned staging slot (a CPU copy on its own thread), the first
 * caller of a group submits the group - one H2D copy, the batch kernels, one result transfer - and every caller takes its
 * own rows.  Groups close when the device can take them (two are in flight at most): batches grow with the load, a lone
 * caller is a batch of one (slower than brisk_hip_detect by the staging copy - use the pool from about four threads on, as
 * include/brisk/hip-context.h does).  All calls of a pool are thread-safe and blocking; results are bit-identical to
 * brisk_hip_detect / brisk_hip_describe.  max_batch <= 64 frames per group, max_keypoints per frame as brisk_hip_set_capacity. */
typedef struct brisk_hip_pool brisk_hip_pool;
int brisk_hip_pool_create(int device, int max_batch, int max_keypoints, brisk_hip_pool** out);
void brisk_hip_pool_destroy(brisk_hip_pool* pool);
const char* brisk_hip_pool_last_error(const brisk_hip_pool* pool); /* of the calling thread's last failed call */
/* groups run so far and the calls they carried (calls / groups = mean batch size) */
int brisk_hip_pool_stats(brisk_hip_pool* pool, unsigned long long* groups, unsigned long long* calls);
/* brisk_hip_detect (suppressScaleNonmaxima = true, no mask, no post-filter) through the pool.  *image_token (may be NULL)
 * names the device copy of this frame for a following brisk_hip_pool_describe. */
int brisk_hip_pool_detect(brisk_hip_pool* pool, const uint8_t* img, int w, int h, int stride, int threshold, int octaves,
                          brisk_hip_keypoint* out, int cap, int* n, unsigned long long* image_token);
/* brisk_hip_describe through the pool.  image_token: 0, or the token of the brisk_hip_pool_detect call that was given the
 * SAME, unchanged pixels (the caller's word, as brisk_hip_describe_same_image): the frame is then taken from its device
 * copy while the pool still holds it (a stale token is harmless: the frame is uploaded). */
int brisk_hip_pool_describe(brisk_hip_pool* pool, const brisk_hip_pattern* pat, const uint8_t* img, int w, int h, int stride,
                            brisk_hip_keypoint* kps, int* n, uint8_t* desc, int desc_stride, int rotation_invariant,
                            int scale_invariant, unsigned long long image_token);

/* Number of internal streams a batch is sliced over (1..8, default 1: measured no gain from slicing).  The slices fork from / join into the
 * caller's stream with events, so the call stays asynchronous and ordered on that stream. */
int brisk_hip_set_streams(brisk_hip_ctx* ctx, int n);

/* ---- multi-GPU: result gather of the batch path (BASELINE config 3) --------------------------------------
 * Frames are independent units (brisk-feature-detector.cc:77-85 builds all state per call): one process or host thread
 * per GPU, each with its own context, runs brisk_hip_detect_describe_batch on its shard of the frame stream - there is no
 * collective inside detect + describe.  The only exchange is this gather of the results to one rank, on RCCL directly
 * (grouped ncclSend / ncclRecv over xGMI; librccl is opened at run time, BRISK_HIP_ERR_UNSUPPORTED where it is missing).
 *   rank 0:      brisk_hip_comm_unique_id(id); pass the 128 bytes to the other ranks (file, socket, MPI, ...)
 *   every rank:  brisk_hip_comm_create(ctx, rank, world, id, &comm)         (collective: all ranks call it)
 *   per batch:   brisk_hip_detect_describe_batch(ctx, ...); brisk_hip_comm_gather_results(ctx, comm, root, ...)
 *   root:        brisk_hip_comm_wait(comm, stream or NULL) before reading the destination buffers
 * The gather is asynchronous and double-buffered: the rank's rows are packed into a slab on the batch's stream, the
 * transfer runs on the communicator's own stream beside the next batch's kernels. */
#define BRISK_HIP_COMM_ID_BYTES 128
typedef struct brisk_hip_comm brisk_hip_comm;
int brisk_hip_comm_unique_id(uint8_t* id /* BRISK_HIP_COMM_ID_BYTES */);
int brisk_hip_comm_create(brisk_hip_ctx* ctx, int rank, int world, const uint8_t* id, brisk_hip_comm** out);
void brisk_hip_comm_destroy(brisk_hip_comm* comm);
int brisk_hip_comm_rank(const brisk_hip_comm* comm);
int brisk_hip_comm_world(const brisk_hip_comm* comm);
/* Collective over the communicator: every rank contributes the DESCRIBED results of its context's last batch as fixed
 * slabs - per-frame counts [frames_max] (0 for the frames beyond its own batch), keypoints [frames_max][kpad] and
 * descriptors [frames_max][kpad][strings] (the first kpad rows of every frame; strings = descriptor bytes) - and `root`
 * receives them, rank after rank, in d_counts [world][frames_max], d_kps [world][frames_max][kpad],
 * d_desc [world][frames_max][kpad][strings] (device memory of the root's GPU; ignored on the other ranks).  frames_max,
 * kpad and strings must be the same on every rank; a frame with more than kpad keypoints is cut (its count is not: the
 * root can tell).  stream: the stream the batch ran on (NULL = the context's stream). */
int brisk_hip_comm_gather_results(brisk_hip_ctx* ctx, brisk_hip_comm* comm, int root, int frames_max, int kpad, int strings,
                                  int* d_counts, brisk_hip_keypoint* d_kps, uint8_t* d_desc, void* stream);
/* orders `stream` behind every gather issued so far on this rank (NULL: blocks the host until they are done) */
int brisk_hip_comm_wait(brisk_hip_comm* comm, void* stream);

/* ---- optional post-filter: keypoint uniformity enforcement (BASELINE config 4) ---- */
/* EnforceKeyPointUniformity (brisk/include/brisk/internal/uniformity-enforcement-inl.h:44-194, mask LUT
 * scale-space-layer-inl.h:88-97) applied to the detector's keypoints (x, y, response) in every following detect call
 * of this context (host-buffer and batch): keypoints in descending response order are accepted greedily against an
 * occupancy image at scale 15 / radius, at most max_keypoints are kept, the output is in acceptance order.
 * radius = 0 switches it off (default).  In the reference the filter is only wired into the Harris
 * ScaleSpaceFeatureDetector (scale-space-layer-inl.h:372-375), so this is an engine option, not reference behaviour of
 * BriskFeatureDetector; equal responses keep their (layer, y, x) order (the reference's std::sort is unstable). */
int brisk_hip_set_uniformity(brisk_hip_ctx* ctx, double radius, int max_keypoints);
/* KeyPointBucketing (brisk/include/brisk/internal/key-point-bucketing-inl.h:40-112; what the reference's
 * ScaleSpaceLayer uses when uniformity enforcement is off, scale-space-layer-inl.h:372-378), applied like the uniformity
 * filter to the detector's keypoints of every following detect call while uniformity is off: keypoints in descending
 * response order; with one bucket in either direction the best max_keypoints are kept, otherwise a keypoint is kept while
 * its bucket of (1 + (cols - 1) / num_buckets_u) x (1 + (rows - 1) / num_buckets_v) pixels holds fewer than
 * max_keypoints / (num_buckets_u * num_buckets_v).  Output in descending response order - except with one bucket in either
 * direction and no more than max_keypoints keypoints: the reference then leaves the vector untouched (:87-88), and so
 * does the engine (detector order).  (0, 0, *) switches it off.
 * The reference requires num_buckets_u < cols and num_buckets_v < rows (CHECK_LT, :82-83): checked per call. */
int brisk_hip_set_bucketing(brisk_hip_ctx* ctx, int num_buckets_u, int num_buckets_v, int max_keypoints);

/* ---- 16-bit image functions (not on the 8-bit detect + describe path) --------------- */
/* Halfsample16 (brisk/src/image-down-sampling.cc:56-139): dst is (w / 2) x (h / 2); Twothirdsample16 (:394-548): dst is
 * (w / 3 * 2) x (h / 3 * 2); IntegralImage16 (brisk/include/brisk/internal/integral-image.h:163-218): dst is
 * (h + 1) x (w + 1) floats.  Host buffers, strides in ELEMENTS; the reference's arithmetic bit for bit (saturating adds,
 * signed pack to 32767, float sums in the reference's order incl. its unscaled last 0..3 columns).  Images with fewer
 * than 16 (half) / 12 (two thirds) usable columns or without an output row, where the reference's loops write nothing:
 * BRISK_HIP_OK, dst untouched. */
int brisk_hip_halfsample16(brisk_hip_ctx* ctx, const uint16_t* src, int w, int h, int src_stride, uint16_t* dst, int dst_stride);
int brisk_hip_twothirdsample16(brisk_hip_ctx* ctx, const uint16_t* src, int w, int h, int src_stride, uint16_t* dst, int dst_stride);
int brisk_hip_integral_image16(brisk_hip_ctx* ctx, const uint16_t* src, int w, int h, int src_stride, float* dst, int dst_stride);

/* ---- Hamming brute-force matcher (the step after the path) ----------------------- */
/* binary-identical to cv::DMatch */
typedef struct brisk_hip_dmatch {
  int queryIdx, trainIdx, imgIdx;
  float distance;
} brisk_hip_dmatch;
/* BruteForceMatcher::knnMatchImpl -> commonKnnMatchImpl (brisk/src/brute-force-matcher.cc:54-64, 80-162) with
 * brisk::Hamming (brisk/include/brisk/internal/hamming.h:98-112: popcount of a ^ b over dim_bytes / 16 128-bit
 * words; dim_bytes 16 ... 224).  query: nq rows of dim_bytes at pitch q_pitch; train[i]: ntrain[i] rows at pitch t_pitch[i] (the
 * trainDescCollection, nimg images).  masks: NULL, or nimg pointers (each NULL or an nq x ntrain[i] u8 matrix at
 * pitch mask_pitch[i]; 0 = pair not allowed).  out: nq * k matches, row q at out + q * k, sorted by
 * (distance, imgIdx, trainIdx); out_count[q] = entries of row q (0 for a masked-out query; rows with fewer
 * than k possible matches are topped up exactly as the reference does).
 * All pointers are host pointers. */
int brisk_hip_match_knn(brisk_hip_ctx* ctx, const uint8_t* query, int nq, int q_pitch, int dim_bytes, int nimg,
                        const uint8_t* const* train, const int* ntrain, const int* t_pitch,
                        const uint8_t* const* masks, const int* mask_pitch, int k, brisk_hip_dmatch* out,
                        int* out_count);
/* BruteForceMatcher::radiusMatchImpl -> commonRadiusMatchImpl (:66-78, 164-213): every pair with
 * distance < max_distance.  out: nq rows of cap_per_query entries; out_count[q] = matches FOUND for query q
 * (only the first cap_per_query of them, in (distance, imgIdx, trainIdx) order, are stored). */
int brisk_hip_match_radius(brisk_hip_ctx* ctx, const uint8_t* query, int nq, int q_pitch, int dim_bytes, int nimg,
                           const uint8_t* const* train, const int* ntrain, const int* t_pitch,
                           const uint8_t* const* masks, const int* mask_pitch, float max_distance,
                           int cap_per_query, brisk_hip_dmatch* out, int* out_count);
/* Device-resident form used by pipelines that keep descriptors in HBM (e.g. the rows brisk_hip_batch_results
 * returns): one train set, no masks, all pointers are device pointers; asynchronous on `stream` (hipStream_t,
 * NULL = the context's stream). */
int brisk_hip_match_knn_device(brisk_hip_ctx* ctx, const uint8_t* d_query, int nq, int q_pitch, const uint8_t* d_train,
                               int nt, int t_pitch, int dim_bytes, int k, brisk_hip_dmatch* d_out, int* d_out_count,
                               void* stream);

/* ---- all frame pairs of a batch in one call ----------------------------------------------------------------------------
 * The step a stream runs after detect + describe - match every frame against the previous one, left against right - with
 * the row counts read on the device: no synchronisation, no download and no launch per pair in between.
 * A descriptor set: `frames` frames of rows in DEVICE memory; the two sides of a pair may come from one batch, from two
 * contexts (stereo) or from a caller's own device copy of earlier frames. */
typedef struct brisk_hip_desc_set {
  const uint8_t* d_desc; /* frame f's rows at d_desc + f * frame_pitch, row r at + r * row_pitch */
  const int* d_counts;   /* rows of frame f = d_counts[f * count_stride] (device memory); fewer than 2^22 */
  int count_stride;      /* in ints */
  long frame_pitch;      /* bytes */
  int row_pitch;         /* bytes, >= dim_bytes */
  int frames;
} brisk_hip_desc_set;
/* Fills *set with the DESCRIBED results of the context's last batch (the rows and counts brisk_hip_batch_results returns);
 * *dim_bytes (may be NULL) = the descriptor size of the pattern that batch used.  BRISK_HIP_ERR_ARG if the context's last
 * call described no batch.  LIFETIME: the result buffers are overwritten by the context's next batch (and may move when a
 * later call grows them), so the set is valid until then; on one stream, match-then-next-batch is safe by stream order.
 * To match across batches keep a device copy of the frames wanted and describe it with a set of your own. */
int brisk_hip_batch_desc_set(brisk_hip_ctx* ctx, brisk_hip_desc_set* set, int* dim_bytes);
/* The pairs: pair p = (query frame query_first + p * query_step, train frame train_first + p * train_step) - frame to
 * previous frame (1, 1, 0, 1), interleaved stereo (0, 2, 1, 2), two sets side by side (0, 1, 0, 1), all against a
 * keyframe (train_step = 0) - unless d_pairs is non-NULL: a DEVICE array of npairs x {query frame, train frame}. */
typedef struct brisk_hip_pair_spec {
  int npairs;
  int query_first, query_step;
  int train_first, train_step;
  const int* d_pairs;
} brisk_hip_pair_spec;
/* Pair p = (a, b): rows [p][q] of d_out / d_out_count are what brisk_hip_match_knn returns for query = the n_a rows of
 * frame a, one train image = the n_b rows of frame b, no masks, the same k: order (distance, train index), including the
 * reference's top-up when 0 < n_b < k and count 0 when n_b == 0; queryIdx = row within frame a, trainIdx = row within
 * frame b, imgIdx = b.  d_pair_rows[p] = n_a, the TRUE count: only rows q < min(n_a, rows_cap) are written, everything else
 * of d_out [npairs][rows_cap][k] and d_out_count [npairs][rows_cap] is left untouched (a cut pair shows as
 * d_pair_rows[p] > rows_cap; the entries of a row whose count is 0 are not written either).
 * cross_check != 0 (k == 1 only): row q's match t is kept only if the best match of row t of frame b among ALL rows of
 * frame a - same distance, same (distance, index) order - is q; otherwise d_out_count[p][q] = 0.
 * A frame outside its set: BRISK_HIP_ERR_ARG for the arithmetic form (checked before anything is launched); for an entry
 * of d_pairs, d_pair_rows[p] = -1 and no rows (also for a frame whose count is 2^22 or more).
 * dim_bytes 16, 32, 48 or 64, else BRISK_HIP_ERR_UNSUPPORTED (brisk_hip_match_knn_device remains for other sizes, k > 2
 * is brisk_hip_match_knn's); npairs == 0 is BRISK_HIP_OK.  Asynchronous on `stream` (hipStream_t, NULL = the context's
 * stream): issued on the batch's stream right after brisk_hip_detect_describe_batch it needs no synchronisation in between. */
int brisk_hip_match_knn_pairs_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                     const brisk_hip_pair_spec* pairs, int dim_bytes, int k, int cross_check, int rows_cap,
                                     brisk_hip_dmatch* d_out, int* d_out_count, int* d_pair_rows, void* stream);

/* Radius matching in the same form - what the reference's callers use (radiusMatch in its live demo and camera test).
 * Pair p = (a, b): row [p][q] of d_out [npairs][rows_cap][cap_per_query] / d_out_count [npairs][rows_cap] is what
 * brisk_hip_match_radius returns for query = the n_a rows of frame a, one train image = the n_b rows of frame b, no masks, the
 * same max_distance and cap_per_query: every train row with (float)distance < max_distance (strict), in (distance, trainIdx)
 * order; queryIdx = row within frame a, trainIdx = row within frame b, imgIdx = b, distance = the bit count as a float.
 * d_out_count[p][q] = matches FOUND (it may exceed cap_per_query; only the first cap_per_query are stored).
 * d_pair_rows[p] = n_a, the TRUE count: only rows q < min(n_a, rows_cap) are written; the entries behind
 * min(count, cap_per_query) of a written row and all other rows are left untouched.  n_b == 0: counts of 0 (radius matching
 * has no top-up entry).  max_distance <= 0 or NaN: all counts 0, not an error.
 * BRISK_HIP_ERR_ARG, before anything is launched: an arithmetic-form frame outside its set, npairs < 0, rows_cap < 1,
 * cap_per_query < 1, row_pitch < dim_bytes, NULL sets or outputs with npairs > 0; npairs == 0 is BRISK_HIP_OK.  An entry of
 * d_pairs outside its set, or a train count of 2^22 or more: d_pair_rows[p] = -1 and no rows, for that pair only.
 * dim_bytes 16, 32, 48 or 64, else BRISK_HIP_ERR_UNSUPPORTED.  Asynchronous on `stream` like
 * brisk_hip_match_knn_pairs_device: issued on the batch's stream after brisk_hip_detect_describe_batch it needs no
 * synchronisation.  Rows with more hits than the kernel's per-query list holds (32) take an exact, slower path inside the
 * same launch. */
int brisk_hip_match_radius_pairs_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                        const brisk_hip_pair_spec* pairs, int dim_bytes, float max_distance, int cap_per_query,
                                        int rows_cap, brisk_hip_dmatch* d_out, int* d_out_count, int* d_pair_rows, void* stream);
/* The radius sibling of brisk_hip_match_knn_device: one train set, no masks, device pointers, host counts, asynchronous on
 * `stream`; d_out [nq][cap_per_query], d_out_count [nq], as brisk_hip_match_radius writes them (imgIdx 0).  dim_bytes as
 * brisk_hip_match_radius (16 ... 224); cap_per_query >= 1. */
int brisk_hip_match_radius_device(brisk_hip_ctx* ctx, const uint8_t* d_query, int nq, int q_pitch, const uint8_t* d_train, int nt,
                                  int t_pitch, int dim_bytes, float max_distance, int cap_per_query, brisk_hip_dmatch* d_out,
                                  int* d_out_count, void* stream);

/* ---- the same two pair matchers behind a position gate -----------------------------------------------------------------
 * How the two pair forms are matched in practice: left against right inside an epipolar band (a few rows of dy, a disparity
 * range of dx), a frame against the previous one inside a search window around each keypoint, often with a limit on the
 * distance between pyramid layers.  The reference's matcher expresses this as a u8 mask per train image
 * (brisk_hip_match_knn / _radius); for the pairs of a batch the mask is a PREDICATE on the two rows' keypoints, evaluated
 * inside the kernels - and a train row that none of a wavefront's 64 neighbouring query rows may match costs neither its
 * descriptor loads nor its bit counts.
 * The keypoints that belong to the rows of a brisk_hip_desc_set: frame f's record r (28 bytes, brisk_hip_keypoint) at
 * (const char*)d_kps + f * frame_pitch + r * sizeof(brisk_hip_keypoint); DEVICE memory, d_kps and frame_pitch multiples of 4.
 * Only x, y and octave are read. */
typedef struct brisk_hip_kp_set {
  const brisk_hip_keypoint* d_kps;
  long frame_pitch; /* bytes */
} brisk_hip_kp_set;
/* query row q (keypoint Q) and train row t (keypoint T) may match iff
 *   dx_min <= T.x - Q.x <= dx_max  and  dy_min <= T.y - Q.y <= dy_max      (one IEEE fp32 subtraction each, then
 *   and (max_octave_diff < 0  or  |T.octave - Q.octave| <= max_octave_diff)   fp32 compares; no contraction)
 * -INFINITY / +INFINITY switch a bound off.  A NaN coordinate or bound makes the compare false: not allowed.
 * A stereo band: {-64, 0, -2, 2, -1}; a tracking window: {-40, 40, -40, 40, 1}; everything: {-INF, +INF, -INF, +INF, -1}. */
typedef struct brisk_hip_match_gate {
  float dx_min, dx_max, dy_min, dy_max;
  int max_octave_diff;
} brisk_hip_match_gate;
/* The DESCRIBED keypoints of the context's last batch, row for row with brisk_hip_batch_desc_set's descriptors; lifetime
 * and errors as brisk_hip_batch_desc_set. */
int brisk_hip_batch_kp_set(brisk_hip_ctx* ctx, brisk_hip_kp_set* kps);
/* brisk_hip_match_knn_pairs_device / brisk_hip_match_radius_pairs_device with the mask M[q][t] = gate(Qkp[a][q], Tkp[b][t])
 * per pair (a, b).  Everything not named here is exactly as in the ungated call of the same name: pair forms, d_pair_rows,
 * rows_cap, untouched memory, bad entries of d_pairs, descriptor sizes, error codes (all checked before anything is
 * launched), asynchronous on `stream`, no workspace.  Additional BRISK_HIP_ERR_ARG with npairs > 0: NULL query_kps /
 * train_kps / gate, a NULL or misaligned d_kps, a frame_pitch that is negative or no multiple of 4.
 * Radius: row [p][q] and its count are what brisk_hip_match_radius returns for frame a's rows, frame b's rows as the one
 *   train image and mask M: the allowed train rows with (float)d < max_distance in (distance, trainIdx) order, count =
 *   matches found.
 * k-NN (k = 1, 2): the min(k, allowed(q)) smallest (distance, trainIdx) keys among the allowed train rows;
 *   d_out_count[p][q] = that number (0: nothing allowed; entries behind the count are not written).
 *   DEVIATION FROM THE REFERENCE, on purpose: a gated row is NEVER topped up.  With a mask the reference's top-up entry
 *   (distance 2147483648.f, brute-force-matcher.cc:139-153) names the first train row that is masked or already taken - an
 *   accident nobody can use.  The gated row is brisk_hip_match_knn's row for mask M without the entries of that distance;
 *   so an all-pass gate gives the ungated call's rows except the top-up entry of 0 < n_b < k.
 * cross_check (k == 1): row q's match t is kept iff the best ALLOWED match of row t among all rows q' of frame a (M[q'][t],
 *   same (distance, index) order) is q. */
int brisk_hip_match_knn_pairs_gated_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                           const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                           const brisk_hip_match_gate* gate, const brisk_hip_pair_spec* pairs, int dim_bytes, int k,
                                           int cross_check, int rows_cap, brisk_hip_dmatch* d_out, int* d_out_count, int* d_pair_rows,
                                           void* stream);
int brisk_hip_match_radius_pairs_gated_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                              const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                              const brisk_hip_match_gate* gate, const brisk_hip_pair_spec* pairs, int dim_bytes,
                                              float max_distance, int cap_per_query, int rows_cap, brisk_hip_dmatch* d_out,
                                              int* d_out_count, int* d_pair_rows, void* stream);

/* ---- the pair matchers' exit: selected matches, packed, on the device or in HOST memory ------------------------------------
 * The four pair matchers leave padded arrays in HBM (d_out [npairs][rows_cap][per_row], d_out_count, d_pair_rows; per_row = the
 * call's k or cap_per_query).  What every consumer does first - a distance bound, Lowe's ratio test on k = 2 rows, a limit of
 * entries per row - is applied on the device, and the selected records are packed in (pair, query row, rank) order: exact
 * prefix sums, no padding, the order deterministic (stable compaction, no atomics).
 * The rule (csrc/brisk_match_select.h is its one definition).  Row (p, q) has c = d_out_count[p][q] and the stored entries
 * e[0 .. min(c, per_row)), in (distance, trainIdx) order.
 *   An entry passes iff e.distance < max_distance (strict fp32 compare; +INFINITY = no bound, NaN keeps nothing) and it is no
 *   top-up entry.  DEVIATION FROM THE REFERENCE, on purpose, the one the gated matchers make: the entry brisk_hip_match_knn's
 *   rows are topped up with when 0 < n_b < k (distance 2147483648.f, brute-force-matcher.cc:139-153) is never selected.
 *   ratio > 0: the row gives at most e[0] - iff e[0] passes and (the row has one stored entry, or e[1] is a top-up entry, or
 *     e[0].distance < ratio * e[1].distance: one fp32 multiplication, one fp32 compare, no contraction).  An ungated row with
 *     n_b == 1 and a gated row with one allowed train row therefore behave the same.  Needs per_row >= 2.
 *   ratio <= 0 or NaN (off): the leading min(stored, keep_per_row) entries that pass (a prefix: rows are sorted by distance).
 *   Rows q >= min(d_pair_rows[p], rows_cap) are never read; a pair with d_pair_rows[p] < 0 gives nothing. */
typedef struct brisk_hip_match_select {
  float max_distance; /* entry kept iff distance < max_distance */
  float ratio;        /* > 0: the ratio test; <= 0 or NaN: off */
  int keep_per_row;   /* at most this many leading entries of a row; >= 1 */
} brisk_hip_match_select;
/* flags of a pair (0 = clean); BRISK_HIP_ROWS_CUT is the fourth */
#define BRISK_HIP_PAIR_ROWS_CUT 0x1    /* d_pair_rows[p] > rows_cap: the matcher cut the pair's query rows; the matched rows are stored */
#define BRISK_HIP_PAIR_BAD 0x2         /* d_pair_rows[p] == -1 (an entry of d_pairs outside its set): nothing is stored */
#define BRISK_HIP_PAIR_ENTRIES_CUT 0x4 /* some row had count > per_row (a radius row cut by cap_per_query): what was stored is used */
/* d_out / d_out_count / d_pair_rows: what one of the four pair matchers wrote with this npairs, rows_cap and per_row.  Outputs, all
 * in caller-provided DEVICE memory:
 *   d_counts  [npairs]      matches selected for pair p
 *   d_flags   [npairs]      the bits above; BRISK_HIP_ROWS_CUT = this pair and every pair behind it did not fit matches_cap: their
 *                           counts are still reported, nothing of them is stored, their offsets stay at the total
 *   d_offsets [npairs + 1]  exclusive prefix sums of the stored counts; d_offsets[npairs] = matches stored
 *   d_matches [matches_cap] the selected records, byte-identical to the source records; nothing behind d_offsets[npairs] is written
 * d_out and d_matches 16-byte aligned, d_offsets 8-byte.  Asynchronous on `stream` (hipStream_t, NULL = the context's stream), no
 * allocation per call once the context's scratch has grown to the call's size (npairs x ceil(rows_cap / 256) sums).
 * BRISK_HIP_ERR_ARG, before anything is launched: npairs < 0, rows_cap < 1, per_row < 1, matches_cap < 0, keep_per_row < 1, a NULL
 * select, the ratio test with per_row < 2, and - with npairs > 0 - a NULL or misaligned array (d_matches may be NULL when
 * matches_cap == 0).  npairs == 0: BRISK_HIP_OK, d_offsets[0] = 0 (d_offsets NULL is then allowed too). */
int brisk_hip_select_pair_matches_device(brisk_hip_ctx* ctx, const brisk_hip_dmatch* d_out, const int* d_out_count, const int* d_pair_rows,
                                         int npairs, int rows_cap, int per_row, const brisk_hip_match_select* select, long long matches_cap,
                                         int* d_counts, int* d_flags, long long* d_offsets, brisk_hip_dmatch* d_matches, void* stream);
/* The same into HOST memory, the way brisk_hip_batch_download_all delivers keypoints and descriptors.  The caller fills in the
 * capacities and the five destination pointers (4-byte aligned, offsets 8):
 *   pair_rows [pairs]  d_pair_rows    counts [pairs]  flags [pairs]  offsets [pairs + 1]  as above    matches [matches_cap] */
typedef struct brisk_hip_pair_host_matches {
  int pairs_cap;         /* pairs the arrays hold: >= npairs */
  long long matches_cap; /* records `matches` holds */
  int* pair_rows;
  int* counts;
  int* flags;
  long long* offsets;
  brisk_hip_dmatch* matches;
} brisk_hip_pair_host_matches;
/* Queues selection + transfer and returns: the three kernels of brisk_hip_select_pair_matches_device run on `stream` (the stream
 * the matcher ran on; NULL = the context's) into a slab the context owns - d_out / d_out_count / d_pair_rows may be overwritten
 * by the next batch in stream order -, the transfer of the exact bytes runs on the context's second stream beside whatever the
 * context does next.  Pinned / registered destinations are written by the device directly; pageable ones go through a pinned
 * buffer of the context and a host copy inside brisk_hip_pair_matches_wait.  *ticket names the transfer.  Two transfers of
 * matches are in flight per context at most - slots of their own, beside the two of brisk_hip_batch_download_all: a stream that
 * downloads rows AND matches of every batch keeps two batches in flight -, a third call first completes the oldest.  `dst`
 * (the struct) is copied; its arrays must stay valid until the ticket has been waited for.  Errors as the device form's, and
 * BRISK_HIP_ERR_ARG for pairs_cap < npairs or a NULL ticket / destination array. */
int brisk_hip_pair_matches_download(brisk_hip_ctx* ctx, const brisk_hip_dmatch* d_out, const int* d_out_count, const int* d_pair_rows,
                                    int npairs, int rows_cap, int per_row, const brisk_hip_match_select* select,
                                    const brisk_hip_pair_host_matches* dst, void* stream, unsigned* ticket);
/* Blocks until transfer `ticket` (and every earlier one of matches) is complete; the context's lock is not held while waiting.
 * *pairs_flagged (may be NULL) = pairs whose flags[] entry is non-zero.  BRISK_HIP_OK, or - with every clean pair in place -
 * BRISK_HIP_ERR_CAPACITY when a pair carries BRISK_HIP_ROWS_CUT (the other flags are information, not errors). */
int brisk_hip_pair_matches_wait(brisk_hip_ctx* ctx, unsigned ticket, int* pairs_flagged);

/* ---- a batch's pair matches checked against a homography, on the device ---------------------------------------------------------
 * What survives the selection passed a descriptor test only; nothing says that a pair's matches agree with each other
 * geometrically, and one wrong match that wins a train row starts a wrong track AND takes the row from the right match (a loser
 * never falls back).  The reference judges matches by their transfer error under a homography (brisk/src/test/test-match.cc:49-126);
 * this call does it with a model estimated from the pair's own records - one call between brisk_hip_select_pair_matches_device and
 * brisk_hip_link_tracks_device, packed lists in, packed lists of the same format out.  csrc/brisk_pair_verify.h is the one
 * definition of the rule; all of its arithmetic is IEEE fp64 + - x in a fixed order, so the kept lists are reproducible bit for bit.
 * PAIRS AND RECORDS.  Pair p = (a, b) of `pairs` as the pair matchers resolve it (both forms); query / train give the frames' row
 * counts (their descriptors are not read), query_kps / train_kps the keypoints.  Its records are d_matches[d_offsets[p] ..
 * d_offsets[p + 1]), m of them.  Record j is USABLE iff 0 <= queryIdx < lim_a, 0 <= trainIdx < lim_b (lim = min(max(count, 0),
 * rows_cap), the rows that exist for the linker) and the x and y of both keypoints are finite; nothing is read from the keypoint
 * sets for any other record, which is never an inlier and never kept.
 * THE RULE.  Hypothesis h (0 <= h < hypotheses) samples four distinct records from a hash of (seed, p, h) and builds the
 * homography H, query -> train, that maps its four query points on its four train points - without a division, from the two
 * projective bases; it is INVALID if m < 4, if a sampled record is unusable or if three of the four points of a side are collinear.
 * A usable record (x, y) -> (x', y') is an INLIER iff z = (H6 x + H7 y) + H8 has the sign of the sample's first point and
 * |H (x, y, 1) - z (x', y', 1)|^2 <= max_error^2 z^2: a transfer error of at most max_error pixels in the train frame.  max_error
 * <= 0 or NaN: nothing is an inlier.  The WINNER is the valid hypothesis with the most inliers, ties to the smallest h; the model is
 * ACCEPTED iff there is one and it has at least min_inliers inliers.
 * KEPT, in the order of the input: the winner's inliers of an accepted pair; of any other pair the usable records if
 * keep_unverified != 0, else nothing.  A pair whose d_pairs entry lies outside its sets, or whose offsets are no range inside
 * [0, in_cap] (or span 2^31 records or more), is BAD: nothing of it is read or kept.
 * Not done here: essential matrices, adaptive stopping.  The refit of the model to all its inliers is a call of its own,
 * brisk_hip_refit_pair_models_device below; scenes that are no plane have brisk_hip_verify_pair_matches_epipolar_device and its own
 * refit, brisk_hip_refit_pair_models_epipolar_device, further below. */
typedef struct brisk_hip_pair_verify {
  float max_error;     /* pixels, in the train frame */
  int hypotheses;      /* 1 ... 4096 */
  int min_inliers;     /* >= 4 */
  int keep_unverified; /* pairs without an accepted model: 0 = keep nothing, else keep their usable records */
  unsigned seed;
} brisk_hip_pair_verify;
typedef struct brisk_hip_pair_model { /* 96 bytes, 8-byte aligned */
  double h[9];                        /* the winner's H, every element divided by the one of largest magnitude (the first on a tie);
                                         nine zeros without a valid hypothesis */
  int records, usable, inliers;       /* m, the usable ones, the winner's inliers */
  int hypothesis;                     /* the winner, -1: none valid */
  int valid;                          /* valid hypotheses */
  int flags;                          /* as d_out_flags[p] */
} brisk_hip_pair_model;
#define BRISK_HIP_PAIR_NO_MODEL 0x8 /* the pair has no accepted model (a BAD pair has none either) */
/* d_offsets [npairs + 1] / d_matches: the lists a selection with matches_cap = in_cap wrote for these npairs = pairs->npairs pairs
 * and this rows_cap; in_cap bounds the INPUT (d_matches holds in_cap records, no offset lies beyond it), out_cap the output.
 * Outputs, all in caller-provided DEVICE memory:
 *   d_models      [npairs]      the pairs' models
 *   d_out_counts  [npairs]      records kept for pair p
 *   d_out_flags   [npairs]      BRISK_HIP_PAIR_BAD, BRISK_HIP_PAIR_NO_MODEL; BRISK_HIP_ROWS_CUT = this pair and every pair behind it
 *                               did not fit out_cap: their counts are still reported, nothing of them is stored, their offsets stay
 *                               at the total (the cut of brisk_hip_select_pair_matches_device)
 *   d_out_offsets [npairs + 1]  exclusive prefix sums of the stored counts; d_out_offsets[npairs] = records stored
 *   d_out_matches [out_cap]     the kept records, byte-identical to the source records; nothing behind d_out_offsets[npairs] is
 *                               written.  It must not overlap d_matches.
 * Asynchronous on `stream` (hipStream_t, NULL = the context's stream), no host synchronisation, no allocation per call once the
 * context's scratch has grown to the call's size (in_cap bytes - one per input record - and npairs sums).
 * BRISK_HIP_ERR_ARG, before anything is launched: NULL pairs or verify, npairs < 0, rows_cap < 1, in_cap < 0, out_cap < 0, hypotheses
 * outside 1 ... 4096, min_inliers < 4, and - with npairs > 0 - a NULL set, a descriptor set without counts or with frames /
 * count_stride < 1, an arithmetic-form frame outside its set, the keypoint-set errors of the gated matchers, a NULL or misaligned
 * array (d_matches / d_out_matches 16-byte and NULL allowed when their capacity is 0, d_offsets / d_out_offsets / d_models 8-byte, the
 * int arrays 4-byte).  npairs == 0: BRISK_HIP_OK, d_out_offsets[0] = 0 (d_out_offsets NULL is then allowed too). */
int brisk_hip_verify_pair_matches_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                         const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                         const brisk_hip_pair_spec* pairs, int rows_cap, const long long* d_offsets,
                                         const brisk_hip_dmatch* d_matches, long long in_cap, const brisk_hip_pair_verify* verify,
                                         long long out_cap, brisk_hip_pair_model* d_models, int* d_out_counts, int* d_out_flags,
                                         long long* d_out_offsets, brisk_hip_dmatch* d_out_matches, void* stream);

/* ---- each pair's homography fitted again to all its inliers, on the device -------------------------------------------------------
 * The verifier reports the winner of its four-record hypotheses: a model that is exact for four noisy keypoints and nothing more.
 * Its kept list and the guided matchers' window centres H_p(Q) inherit that noise.  This call, between the verifier and the guided
 * matchers or the linker, fits every pair's model again to ALL its inliers by least squares and counts the inliers again, for
 * `rounds` rounds.  It reads the lists the VERIFIER read (the selection's output), not the verifier's kept lists: a least-squares
 * model recovers true matches the four-point winner scored just outside max_error, so a kept list can grow.  Its outputs have
 * exactly the verifier's formats, so the linker, the guided matchers and both exits take them unchanged.  csrc/brisk_pair_refit.h is
 * the one definition of the rule; all of its arithmetic is IEEE fp64 + - x / in a fixed order (the division is correctly rounded on
 * host and device, as the guided matchers rely on), so models and kept lists are reproducible bit for bit.
 * Pairs, records, USABLE records and BAD pairs are the verifier's.
 * THE INPUT MODEL.  Pair p has one iff it is not BAD, d_models[p].hypothesis >= 0, (d_models[p].flags & (BRISK_HIP_PAIR_BAD |
 * BRISK_HIP_PAIR_NO_MODEL)) == 0 (the guided matchers' test), the nine elements of h are finite and max_error > 0.  Only h,
 * hypothesis and flags of an input record are read.  A pair without an input model is treated as the verifier treats a pair without
 * an accepted model: it keeps its usable records if keep_unverified != 0, else nothing; flags BRISK_HIP_PAIR_NO_MODEL (and
 * BRISK_HIP_PAIR_BAD); the output model is nine zeros, hypothesis -1, inliers 0, valid 0.
 * THE SCORE of a model H is sign-free (the reported model lost its sign): a usable record PASSES iff |H (x, y, 1) - z (x', y', 1)|^2
 * <= max_error^2 z^2 with z = (H6 x + H7 y) + H8, the verifier's expressions; the INLIERS are the passers with z > 0 if those are
 * at least as many as the passers with z < 0, else the passers with z < 0.  H and -H score alike.
 * THE FIT to an inlier set of n >= 4 records: both sides are normalised (centroid to the origin, mean absolute coordinate to 1),
 * the 8 x 8 normal equations of the inhomogeneous system (h8 = 1 in normalised coordinates) are summed in one fixed order (256
 * partials by list index modulo 256, an xor butterfly inside blocks of 64, then the four blocks) and solved by elimination without
 * pivoting; the solution is denormalised and divided by its element of largest magnitude, as the verifier reports a model.  The fit
 * FAILS if a side has no extent, a pivot is not > 0 (inliers on one line, at one point) or an element of the result is not finite.
 * THE ROUNDS.  H_0 = the input model, n_0 the number of its inliers.  For r = 1 ... rounds: stop if n_(r-1) < 4 or the fit to the
 * inliers of H_(r-1) fails; if the fitted model H' has n' >= n_(r-1) inliers it REPLACES the model, else stop and keep H_(r-1).  The
 * number of inliers therefore never falls.  (Once a round returns its own inlier set, every later round fits the same set and
 * replaces the model by itself.)
 * ACCEPTED iff the pair has an input model and the final count >= min_inliers.  KEPT, in the order of the input: the final model's
 * inliers of an accepted pair; of any other pair the usable records if keep_unverified != 0, else nothing.
 * THE OUTPUT RECORD: h = the final model - the input record's nine doubles, byte for byte, when no round replaced it -, records and
 * usable as the verifier writes them, inliers = the final count, hypothesis = the input's, valid = the number of rounds that
 * replaced the model, flags = BRISK_HIP_PAIR_REFIT iff that number is > 0, plus BRISK_HIP_PAIR_NO_MODEL if not accepted (and
 * BRISK_HIP_ROWS_CUT as below).  The guided matchers read h, hypothesis and flags only: they take these records in place. */
typedef struct brisk_hip_pair_refit {
  float max_error;     /* pixels, in the train frame: the verifier's inlier threshold */
  int rounds;          /* 1 ... 8 */
  int min_inliers;     /* >= 4 */
  int keep_unverified; /* pairs without an accepted model: as brisk_hip_pair_verify */
} brisk_hip_pair_refit;
#define BRISK_HIP_PAIR_REFIT 0x10 /* at least one round replaced the input model */
/* d_offsets / d_matches / in_cap: what the VERIFIER was given for these pairs; d_models [npairs]: the models it wrote (or any
 * brisk_hip_pair_model records), DEVICE memory, 8-byte aligned.  d_out_models, d_out_counts, d_out_flags, d_out_offsets,
 * d_out_matches and out_cap: exactly the verifier's d_models ... d_out_matches - the same cut at out_cap, and nothing behind the
 * stored counts is written.  d_out_models may be the same array as d_models (a pair's record is read before it is written); no
 * other overlap is allowed.
 * Asynchronous on `stream`, no host synchronisation, no allocation once the context's scratch has the verifier's size for this in_cap
 * and npairs (it is the same scratch).  Ordered behind the context's previous call and in front of its next, like every call.
 * BRISK_HIP_ERR_ARG, before anything is launched: the verifier's errors (refit in the place of verify, min_inliers < 4 included),
 * rounds outside 1 ... 8, a misaligned d_models, a NULL d_models with npairs > 0.  npairs == 0: BRISK_HIP_OK, d_out_offsets[0] = 0. */
int brisk_hip_refit_pair_models_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                       const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                       const brisk_hip_pair_spec* pairs, int rows_cap, const long long* d_offsets,
                                       const brisk_hip_dmatch* d_matches, long long in_cap, const brisk_hip_pair_model* d_models,
                                       const brisk_hip_pair_refit* refit, long long out_cap, brisk_hip_pair_model* d_out_models,
                                       int* d_out_counts, int* d_out_flags, long long* d_out_offsets, brisk_hip_dmatch* d_out_matches,
                                       void* stream);

/* ---- a batch's pair matches checked against an epipolar geometry, on the device ---------------------------------------------------
 * A homography is the right model for a plane or a pure rotation.  Left against right, and frame against previous frame of a moving
 * camera, see a scene with depth: no homography holds there, and the verifier above keeps the dominant plane and drops true matches
 * everywhere else.  What holds is the epipolar constraint x'^T F x = 0.  This call is the verifier with that model in the
 * homography's place - the same place in the chain (select -> verify -> link), the same inputs, packed lists of the same format out.
 * csrc/brisk_pair_epipolar.h is the one definition of the rule; all of its arithmetic is IEEE fp64 + - x / in a fixed order (the
 * division is correctly rounded on host and device), so models and kept lists are reproducible bit for bit.
 * Pairs, records, USABLE records and BAD pairs are the verifier's.
 * THE RULE.  Hypothesis h (0 <= h < hypotheses) samples EIGHT distinct records from a hash of (seed, p, h).  Both sides of the
 * sample are normalised (centroid to the origin, mean absolute coordinate to 1), and F, query -> train, row-major, is the null vector
 * of the linear 8 x 9 system of the eight records, found by elimination with complete pivoting: no element is fixed to 1 beforehand,
 * so rectified stereo, where the last element of F is 0, is no special case.  F is denormalised and divided by its element of largest
 * magnitude; that F is what is scored and what is reported.  The hypothesis is INVALID if m < 8, if a sampled record is unusable, if
 * a side of the sample has no extent, if a pivot is not > 0 and finite (the eight points of a side on one axis-parallel line) or an
 * element of F is not finite.  A usable record (x, y) -> (x', y') is an INLIER iff its Sampson distance is at most max_error pixels,
 * tested without a division: with l = F (x, y, 1), l' = F^T (x', y', 1), r = (x', y', 1) . l and g = l0^2 + l1^2 + l'0^2 + l'1^2:
 * g > 0 and r^2 <= max_error^2 g.  There is no sign test.  max_error <= 0 or NaN: nothing is an inlier.  WINNER, ACCEPTED (with
 * min_inliers >= 8) and KEPT are the verifier's.
 * WHAT THE MODEL IS.  A filter: it decides which records agree with ONE epipolar geometry.  RANK 2 IS NOT ENFORCED, so the reported
 * F is the linear eight-point solution and in general has no epipoles; it is not meant for rectification or for recovering a pose.
 * Eight coplanar points (and a scene that is a plane) give a degenerate system; its null vector still vanishes on the plane's
 * records, so the plane is kept - with more random records beside it than a proper F lets through.
 * Not done here: essential matrices (no intrinsics enter), seven- or five-point samples, adaptive stopping; the refit of F to all its
 * inliers, with rank 2 enforced, is a call of its own, brisk_hip_refit_pair_models_epipolar_device below.  The second pass -
 * guided matching along epipolar lines - reads these models, or the refitted ones, in place: "a batch's pairs matched again inside a
 * band around each epipolar line" below. */
typedef struct brisk_hip_pair_epipolar_model { /* 96 bytes, 8-byte aligned.  A type of its own ON PURPOSE: brisk_hip_refit_pair_models_device
                                                  and the guided matchers read a brisk_hip_pair_model as a homography and must not be
                                                  handed an F */
  double f[9];                                 /* the winner's F, row-major, x'^T F x = 0, every element divided by the one of largest
                                                  magnitude (the first on a tie); nine zeros without a valid hypothesis */
  int records, usable, inliers;                /* m, the usable ones, the winner's inliers */
  int hypothesis;                              /* the winner, -1: none valid */
  int valid;                                   /* valid hypotheses */
  int flags;                                   /* as d_out_flags[p] */
} brisk_hip_pair_epipolar_model;
/* The arguments are brisk_hip_verify_pair_matches_device's, one for one, except that d_models holds brisk_hip_pair_epipolar_model
 * records.  `verify` is the verifier's structure, unchanged: max_error is the Sampson distance in pixels, hypotheses 1 ... 4096
 * eight-record samples, min_inliers >= 8.
 * d_offsets [npairs + 1] / d_matches: the lists a selection with matches_cap = in_cap wrote for these npairs = pairs->npairs pairs
 * and this rows_cap; in_cap bounds the INPUT (d_matches holds in_cap records, no offset lies beyond it), out_cap the output.
 * Outputs, all in caller-provided DEVICE memory:
 *   d_models      [npairs]      the pairs' models
 *   d_out_counts  [npairs]      records kept for pair p
 *   d_out_flags   [npairs]      BRISK_HIP_PAIR_BAD, BRISK_HIP_PAIR_NO_MODEL; BRISK_HIP_ROWS_CUT = this pair and every pair behind it
 *                               did not fit out_cap: their counts are still reported, nothing of them is stored, their offsets stay
 *                               at the total (the cut of brisk_hip_select_pair_matches_device)
 *   d_out_offsets [npairs + 1]  exclusive prefix sums of the stored counts; d_out_offsets[npairs] = records stored
 *   d_out_matches [out_cap]     the kept records, byte-identical to the source records; nothing behind d_out_offsets[npairs] is
 *                               written.  It must not overlap d_matches.
 * Asynchronous on `stream` (hipStream_t, NULL = the context's stream), no host synchronisation, no allocation per call once the
 * context's scratch has grown to the call's size (in_cap bytes - one per input record - and npairs sums; it is the verifier's
 * scratch).  Ordered behind the context's previous call and in front of its next, like every call.
 * BRISK_HIP_ERR_ARG, before anything is launched: NULL pairs or verify, npairs < 0, rows_cap < 1, in_cap < 0, out_cap < 0, hypotheses
 * outside 1 ... 4096, min_inliers < 8, and - with npairs > 0 - a NULL set, a descriptor set without counts or with frames /
 * count_stride < 1, an arithmetic-form frame outside its set, the keypoint-set errors of the gated matchers, a NULL or misaligned
 * array (d_matches / d_out_matches 16-byte and NULL allowed when their capacity is 0, d_offsets / d_out_offsets / d_models 8-byte, the
 * int arrays 4-byte).  npairs == 0: BRISK_HIP_OK, d_out_offsets[0] = 0 (d_out_offsets NULL is then allowed too). */
int brisk_hip_verify_pair_matches_epipolar_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                                  const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                                  const brisk_hip_pair_spec* pairs, int rows_cap, const long long* d_offsets,
                                                  const brisk_hip_dmatch* d_matches, long long in_cap, const brisk_hip_pair_verify* verify,
                                                  long long out_cap, brisk_hip_pair_epipolar_model* d_models, int* d_out_counts,
                                                  int* d_out_flags, long long* d_out_offsets, brisk_hip_dmatch* d_out_matches, void* stream);

/* ---- each pair's fundamental matrix fitted again to all its inliers, rank 2 enforced, on the device ------------------------------
 * The epipolar verifier reports the linear solution of eight noisy keypoints: exact for its sample and nothing more, and without
 * epipoles.  The band of the epipolar-guided matchers is drawn around the lines of that F.  This call stands where
 * brisk_hip_refit_pair_models_device stands in the homography branch (select -> verify_epipolar -> refit_epipolar -> epipolar-guided
 * matchers / linker / exits): it fits every pair's F again to ALL its inliers by least squares, optionally projects the result to
 * rank 2, and counts the inliers again, for `rounds` rounds.  It reads the lists the VERIFIER read, so a kept list can grow.
 * csrc/brisk_pair_epipolar_refit.h is the one definition of the rule; all of its arithmetic is IEEE fp64 + - x / in a fixed order, no
 * square root and no eigen-solver, so models and kept lists are reproducible bit for bit.
 * Pairs, records, USABLE records and BAD pairs are the verifier's.
 * THE INPUT MODEL: the test of brisk_hip_refit_pair_models_device, on f, hypothesis and flags of d_models[p].  A pair without one is
 * treated as that call treats it: BRISK_HIP_PAIR_NO_MODEL, nine zeros, hypothesis -1, inliers 0, valid 0.
 * THE SCORE of a model F: the epipolar verifier's Sampson test, Sampson distance <= max_error pixels; no sign enters.
 * THE FIT to an inlier set of n >= 8 records: both sides are normalised as in brisk_hip_refit_pair_models_device; the symmetric
 * 9 x 9 normal matrix of the rows [U X, U Y, U, V X, V Y, V, X, Y, 1] is summed in that call's fixed order and eliminated with
 * DIAGONAL pivoting: the element of F that is held at 1 is the one whose index is left last, chosen by the data, so rectified stereo
 * (the last element of F is 0) is no special case.  With rank2 != 0 the normalised solution Fn is projected to rank 2: N = Fn^T Fn,
 * the same pivoted elimination on this 3 x 3 gives e, and Fn' = Fn - (Fn e) e^T / (e . e), so Fn' e = 0: e is the epipole in the query
 * frame, and Fn' is the SVD truncation up to the error of one step of inverse iteration.  The result is denormalised and divided by
 * its element of largest magnitude.  The fit FAILS if a side has no extent, a pivot is not > 0 and finite (inliers on one
 * axis-parallel line, at one point), e . e is not finite and > 0, or an element of the result is not finite.
 * THE ROUNDS, ACCEPTED and KEPT: those of brisk_hip_refit_pair_models_device with 8 in the place of 4; the count never falls.
 * THE OUTPUT RECORD: f = the final model - the input record's nine doubles, byte for byte, when no round replaced it -, records and
 * usable as the verifier writes them, inliers = the final count, hypothesis = the input's, valid = the number of rounds that
 * replaced the model, flags = BRISK_HIP_PAIR_REFIT iff that number is > 0, plus BRISK_HIP_PAIR_NO_MODEL if not accepted (and
 * BRISK_HIP_ROWS_CUT as for the verifier).  A model that no round replaced is still the verifier's F, rank 2 NOT enforced, and its
 * record does not carry BRISK_HIP_PAIR_REFIT: the flag is how a caller knows that the record holds a refitted F, and a rank-2 one
 * if it asked for that.  The epipolar-guided matchers read f, hypothesis and flags only: they take these records in place. */
typedef struct brisk_hip_pair_epipolar_refit {
  float max_error;     /* Sampson distance in pixels: the epipolar verifier's threshold */
  int rounds;          /* 1 ... 8 */
  int min_inliers;     /* >= 8 */
  int keep_unverified; /* pairs without an accepted model: as brisk_hip_pair_verify */
  int rank2;           /* 0: the least-squares F as fitted; else its rank-2 projection */
} brisk_hip_pair_epipolar_refit;
/* The arguments, the outputs, the cut at out_cap and the BAD-pair rules are brisk_hip_refit_pair_models_device's, one for one, with
 * brisk_hip_pair_epipolar_model records: d_offsets / d_matches / in_cap are what the epipolar VERIFIER was given for these pairs,
 * d_models [npairs] the models it wrote (DEVICE memory, 8-byte aligned); d_out_models may be the same array as d_models (a pair's
 * record is read before it is written); no other overlap is allowed.
 * Asynchronous on `stream`, no host synchronisation, no allocation once the context's scratch has the verifier's size for this in_cap
 * and npairs (it is the same scratch).  Ordered behind the context's previous call and in front of its next, like every call.
 * BRISK_HIP_ERR_ARG, before anything is launched: the errors of brisk_hip_refit_pair_models_device with min_inliers < 8 in the place
 * of < 4; rounds outside 1 ... 8.  npairs == 0: BRISK_HIP_OK, d_out_offsets[0] = 0. */
int brisk_hip_refit_pair_models_epipolar_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                                const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                                const brisk_hip_pair_spec* pairs, int rows_cap, const long long* d_offsets,
                                                const brisk_hip_dmatch* d_matches, long long in_cap,
                                                const brisk_hip_pair_epipolar_model* d_models, const brisk_hip_pair_epipolar_refit* refit,
                                                long long out_cap, brisk_hip_pair_epipolar_model* d_out_models, int* d_out_counts,
                                                int* d_out_flags, long long* d_out_offsets, brisk_hip_dmatch* d_out_matches, void* stream);

/* ---- a batch's pairs matched again inside a window around each pair's model ----------------------------------------------------
 * What reaches the linker after the verification is the part of the first pass that survived the descriptor test (Lowe's ratio
 * rejects true matches on repetitive texture) AND was an inlier.  Once a pair's model is known the usual second pass is the guided
 * (by-projection) one: each query keypoint is matched again, only against the train keypoints within a few pixels of where the
 * model puts it - the position does the work the ratio test did.  These two calls are the gated matchers with the window centred at
 * H_p(Q) instead of Q; they read the verifier's d_models in place, and their output goes through the selection, the verification,
 * the linker and both exits like any pair matcher's.  csrc/brisk_match_guide.h is the one definition of the rule.
 * d_models: a DEVICE array [npairs], 8-byte aligned, indexed by PAIR p (not by frame: the keyframe form train_step = 0 has a model
 * per pair).  Only h[0..8], hypothesis and flags of a record are read; the records may be what brisk_hip_verify_pair_matches_device
 * wrote for these pairs, an earlier batch's, or the caller's own.
 * GUIDED: pair p iff d_models[p].hypothesis >= 0 and (flags & (BRISK_HIP_PAIR_BAD | BRISK_HIP_PAIR_NO_MODEL)) == 0.
 * THE CENTRE of query row q, keypoint (x, y, octave), in a guided pair: x and y converted to double, then
 *   z = (h6 x + h7 y) + h8   u = (h0 x + h1 y) + h2   v = (h3 x + h4 y) + h5   (IEEE fp64, this order, no contraction)
 *   cx = (float)(u / z)      cy = (float)(v / z)      (one correctly rounded fp64 division each, then round-to-nearest to fp32)
 * In an unguided pair with fallback != 0: cx = x, cy = y (the plain gated matcher).  The row HAS A CENTRE iff cx and cy are finite:
 * z == 0, a NaN model element, a NaN coordinate, an overflow of the conversion and an infinite model element (unless both quotients
 * stay finite) give none, and a row of an unguided pair with fallback == 0 has none.
 * THE MASK: M[q][t] = has_centre(q) and window.dx_min <= T.x - cx <= window.dx_max and window.dy_min <= T.y - cy <= window.dy_max
 * (fp32, as the gate) and the gate's octave rule between Q's and T's octaves.  The identity model gives the gated matcher's mask.
 * DEVIATION FROM THE VERIFIER, on purpose: no test of the sign of z.  The verifier's inlier rule demands that z has the sign of its
 * sample's first point; the reported model was divided by its element of largest magnitude, so that sign is lost.  The centre is
 * H's image of the point, whatever the sign of z. */
typedef struct brisk_hip_match_guide {
  brisk_hip_match_gate window; /* bounds on T - C, C the centre; max_octave_diff between Q and T as in the gate */
  int fallback;                /* a pair without a usable model: 0 = its rows match nothing, else C = Q (the plain gated matcher) */
} brisk_hip_match_guide;
/* Everything not named here is exactly as in the gated call of the same kind with the mask M above: both pair forms, d_pair_rows
 * (true counts; -1 for a bad d_pairs entry or a train count of 2^22 or more), rows_cap, memory that is never written, k-NN rows
 * holding min(k, allowed) real entries and never topped up (k = 1, 2), radius counts = matches found, descriptor sizes, error codes
 * (all checked before anything is launched), asynchronous on `stream`.  Additional BRISK_HIP_ERR_ARG with npairs > 0: a NULL or
 * misaligned d_models, a NULL guide, the gated calls' keypoint-set errors.  npairs == 0 is BRISK_HIP_OK.
 * These two calls take no cross_check argument; the cross-checked k = 1 form is a call of its own,
 * brisk_hip_match_mutual_pairs_guided_device ("the guided pair matchers' mutual forms" below). */
int brisk_hip_match_knn_pairs_guided_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                            const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                            const brisk_hip_pair_spec* pairs, const brisk_hip_pair_model* d_models,
                                            const brisk_hip_match_guide* guide, int dim_bytes, int k, int rows_cap, brisk_hip_dmatch* d_out,
                                            int* d_out_count, int* d_pair_rows, void* stream);
int brisk_hip_match_radius_pairs_guided_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                               const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                               const brisk_hip_pair_spec* pairs, const brisk_hip_pair_model* d_models,
                                               const brisk_hip_match_guide* guide, int dim_bytes, float max_distance, int cap_per_query,
                                               int rows_cap, brisk_hip_dmatch* d_out, int* d_out_count, int* d_pair_rows, void* stream);

/* ---- a batch's pairs matched again inside a band around each epipolar line -----------------------------------------------------
 * The second pass of the epipolar branch (select -> brisk_hip_verify_pair_matches_epipolar_device -> these calls -> select -> link),
 * for scenes with depth: left against right, or a moving camera.  Every query keypoint is matched again, only against the train
 * keypoints that lie within `band` pixels of its epipolar line F_p (x, y, 1), inside an optional window around the query keypoint's
 * own position (the disparity range, or the tracking window along the line), and that satisfy the gate's octave rule.  The calls
 * read the epipolar verifier's d_models in place, and their output goes through the selection, either verifier, the linker and both
 * exits like any pair matcher's.  csrc/brisk_match_epiline.h is the one definition of the rule; all of its decision arithmetic is
 * IEEE fp64 + - x and compares in a fixed order - no division, no square root -, so host and device agree bit for bit.
 * d_models: a DEVICE array [npairs] of brisk_hip_pair_epipolar_model, 8-byte aligned, indexed by PAIR p.  Only f[0..8], hypothesis
 * and flags of a record are read; the records may be the epipolar verifier's, an earlier batch's, or the caller's own.  The type is
 * the epipolar model's on purpose: a homography record does not compile in.
 * GUIDED: pair p iff d_models[p].hypothesis >= 0 and (flags & (BRISK_HIP_PAIR_BAD | BRISK_HIP_PAIR_NO_MODEL)) == 0.
 * THE LINE of query row q, keypoint (x, y, octave), in a guided pair: x and y converted to double, then step (d) of the verifier:
 *   l0 = (f0 x + f1 y) + f2   l1 = (f3 x + f4 y) + f5   l2 = (f6 x + f7 y) + f8   n = l0 l0 + l1 l1   w = (double(band) double(band)) n
 * The row HAS A LINE iff band > 0 (fp32; a NaN, zero or negative band gives none), n > 0, and n and l2 are finite.  w may be +inf:
 * a band of +INFINITY switches the band off.  A query at an epipole of a rank-2 F, a NaN or infinite model element, a NaN
 * coordinate, an overflow of n and the zero model give no line.
 * THE BAND for a train keypoint (x', y'), converted to double: r = (x' l0 + y' l1) + l2 passes iff r r <= w (closed; a NaN fails).
 * THE MASK in a guided pair: M[q][t] = has_line(q) and band(q, t) and the gate of `window` between Q and T - centred on the query
 * keypoint itself, not on a projection.  In an unguided pair with fallback != 0 the band is off and the mask is the plain gate's;
 * with fallback == 0 no row matches anything.
 * Rectified stereo, F = s [0 0 0; 0 0 -1; 0 1 0], gives the gated matcher's mask with dy in [-band, band].  With band == the
 * verifier's max_error every allowed (q, t) of finite coordinates is a Sampson inlier of that F under the verifier's rule (n <= g). */
typedef struct brisk_hip_match_epipolar_guide {
  brisk_hip_match_gate window; /* bounds on T - Q; max_octave_diff between Q and T as in the gate.  All-pass: the band alone */
  float band;                  /* pixels on either side of the epipolar line */
  int fallback;                /* a pair without a usable model: 0 = its rows match nothing, else the plain gated matcher of `window` */
} brisk_hip_match_epipolar_guide;
/* Everything not named here is exactly as in the guided call of the same kind above, with the mask M of this section: both pair
 * forms, d_pair_rows, rows_cap, memory that is never written, k-NN rows holding min(k, allowed) real entries and never topped up
 * (k = 1, 2), radius counts = matches found, the four descriptor sizes, no cross_check argument (the cross-checked k = 1 form is
 * brisk_hip_match_mutual_pairs_epipolar_guided_device below), asynchronous on `stream`, no workspace.
 * BRISK_HIP_ERR_ARG before anything is launched: the guided calls' list - with npairs > 0 a NULL or misaligned d_models, a NULL
 * guide, the gated calls' keypoint-set errors.  npairs == 0 is BRISK_HIP_OK. */
int brisk_hip_match_knn_pairs_epipolar_guided_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                                     const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                                     const brisk_hip_pair_spec* pairs, const brisk_hip_pair_epipolar_model* d_models,
                                                     const brisk_hip_match_epipolar_guide* guide, int dim_bytes, int k, int rows_cap,
                                                     brisk_hip_dmatch* d_out, int* d_out_count, int* d_pair_rows, void* stream);
int brisk_hip_match_radius_pairs_epipolar_guided_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                                        const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                                        const brisk_hip_pair_spec* pairs, const brisk_hip_pair_epipolar_model* d_models,
                                                        const brisk_hip_match_epipolar_guide* guide, int dim_bytes, float max_distance,
                                                        int cap_per_query, int rows_cap, brisk_hip_dmatch* d_out, int* d_out_count,
                                                        int* d_pair_rows, void* stream);

/* ---- the guided pair matchers' mutual forms: k = 1 with the cross check ---------------------------------------------------------
 * The second pass has no ratio test left - the window or the band replaced it -, so mutuality is the one descriptor-side safeguard
 * that remains; these two calls are the guided k-NN calls for k = 1 with the first-pass matchers' fused cross check.  Stated once,
 * for both guides: pair p = (a, b), M[q][t] the mask of the guided section in question (the window around the centre above, or the
 * band and the window of the epipolar section), exactly as that section defines it - guided pairs, fallback pairs, rows without a
 * centre or a line, window, octave rule, band.
 * FORWARD: for q < min(n_a, rows_cap), f(q) is the allowed train row of smallest key (distance, t): the record the guided k-NN call
 * writes for k = 1.
 * BACKWARD: for t = f(q), g(t) is the row q' among ALL n_a rows of frame a - also those at or beyond rows_cap - with M[q'][t] true and
 * the smallest key (distance, q').
 * KEPT iff g(t) == q: the row holds the guided k = 1 record byte for byte, count 1.  Otherwise the count is 0 and the row's record
 * is not written.
 * The backward mask is the SAME predicate as the forward one, read from the train side - the centre of q' is still H_p(q'), the
 * difference still T - C; the band is still T against the line of q'.  It is not an inverse model, so the identity model, and an
 * unguided pair with fallback != 0, give exactly brisk_hip_match_knn_pairs_gated_device with gate = window, k = 1, cross_check = 1
 * (the epipolar form with band = +INFINITY: for the rows that have a line).
 * Everything else is what the gated call with cross_check = 1 does: d_pair_rows holds the true count, -1 for a bad d_pairs entry or
 * for n_a or n_b of 2^22 or more (the backward keys index frame a too); n_b == 0, and an unguided pair with fallback == 0, give counts
 * of 0; nothing behind the counts or beyond `rows` is written; asynchronous on `stream`, no workspace, no synchronisation with the
 * host.  d_out is [npairs][rows_cap][1].  The arguments are the guided k-NN calls' without k, and so are the errors, all checked
 * before anything is launched; npairs == 0 is BRISK_HIP_OK; dim_bytes 16, 32, 48 or 64.
 * The rule's two backward predicates are brisk_guide_train_row (csrc/brisk_match_guide.h) and brisk_epiguide_train_row
 * (csrc/brisk_match_epiline.h).  Measured on one MI355X (tools/bench_match_pairs.py --guided --mutual, profiles/match_mutual_pairs.json):
 * 2.10 times the guided k = 1 call's time, where the gated call's cross check costs 2.18 times the gated call's. */
int brisk_hip_match_mutual_pairs_guided_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                               const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                               const brisk_hip_pair_spec* pairs, const brisk_hip_pair_model* d_models,
                                               const brisk_hip_match_guide* guide, int dim_bytes, int rows_cap, brisk_hip_dmatch* d_out,
                                               int* d_out_count, int* d_pair_rows, void* stream);
int brisk_hip_match_mutual_pairs_epipolar_guided_device(brisk_hip_ctx* ctx, const brisk_hip_desc_set* query, const brisk_hip_desc_set* train,
                                                        const brisk_hip_kp_set* query_kps, const brisk_hip_kp_set* train_kps,
                                                        const brisk_hip_pair_spec* pairs, const brisk_hip_pair_epipolar_model* d_models,
                                                        const brisk_hip_match_epipolar_guide* guide, int dim_bytes, int rows_cap,
                                                        brisk_hip_dmatch* d_out, int* d_out_count, int* d_pair_rows, void* stream);

/* ---- a batch's pair matches linked into feature tracks, on the device ----------------------------------------------------------
 * What every consumer of a frame-to-previous-frame matcher does next: "row q of frame i matched row t of frame i - 1" becomes
 * tracks - which keypoints are the same point seen again, since when, which tracks are long enough to use.  An integer problem
 * with an exact answer; csrc/brisk_track_link.h is the one definition of the rule.
 * THE CHAIN: `nodes` >= 1 frames in time order.  Node i has n_i = d_node_rows[i * node_rows_stride] rows (DEVICE memory); with a
 * brisk_hip_desc_set and the frames first + i * step: d_node_rows = d_counts + first * count_stride, node_rows_stride = step *
 * count_stride (a mono stream: step 1; one camera of an interleaved stereo stream: step 2).  Only the rows r < lim_i =
 * min(max(n_i, 0), rows_cap) exist.  Pair p (0 <= p < nodes - 1) has node p + 1 as query and node p as train - what the pair spec
 * {nodes - 1, first + step, step, first, step, NULL} gives the matchers - and its matches are the records
 * d_matches[d_offsets[p] .. d_offsets[p + 1]) as brisk_hip_select_pair_matches_device writes them: in (query row, rank) order, a
 * pair cut at matches_cap with an empty range.  (The d_pairs form of a pair spec is no chain.)
 * THE RULE.  Record j of pair p is a PROPOSAL iff it is the first record of its query row (j is the first of the pair's range, or
 * record j - 1 has another queryIdx), 0 <= queryIdx < lim_{p+1}, 0 <= trainIdx < lim_p, and the bit pattern of its distance, read
 * as u32, is <= 0x7F800000 (no NaN, no sign bit).  Every other record is ignored (and counted): a row proposes with its best entry
 * only, and a row that loses does not fall back to its second.  Among the proposals for one train row t the smallest 64-bit key
 * (distance bits << 32 | queryIdx) WINS - for such floats the bit order is the numeric order, ties go to the smaller query row:
 * the winner q gets prev[p + 1][q] = t, every other row of node p + 1 and every row of node 0 gets -1.  (Cross-checked k = 1 lists:
 * every proposal wins.)  If one query row's records are not contiguous in a list, the result for that row is unspecified; every
 * access stays inside the arrays.
 * A row with prev == -1 is a HEAD, a row with prev >= 0 an interior row: its track is its predecessor's, its age its predecessor's
 * + 1.  A head of node 0 with a seed d_track[r] >= 0 continues that track at age d_age[r]; every other head STARTS a track at age
 * 0, numbered first_new + the starting heads before it in (node, row) order.  Track numbers are 64-bit.
 * SPLITTING: a chain split at node m into two calls gives the numbers and ages of the single call when the second call's node 0 is
 * the first call's node m, seeded with that call's track / age rows of node m and with its next_new. */
typedef struct brisk_hip_track_seed {
  const long long* d_track;      /* [rows_cap] DEVICE: the track row r of node 0 continues, < 0 = none; NULL (with d_age) = no seeds */
  const int* d_age;              /* [rows_cap] DEVICE: its age */
  long long first_new;           /* the first number this call may give ... */
  const long long* d_first_new;  /* ... taken from this DEVICE word instead when non-NULL (the previous call's d_summary: no synchronisation) */
} brisk_hip_track_seed;
/* Outputs, all in caller-provided DEVICE memory, padded like the matchers' arrays: d_prev [nodes][rows_cap] int, d_track
 * [nodes][rows_cap] long long, d_age [nodes][rows_cap] int - only rows r < lim_i are written, everything else is left untouched -
 * and d_summary, eight long long:
 *   [0] next_new, the first number the next call may give   [1] tracks started   [2] links (winners)   [3] proposals that lost
 *   [4] records ignored   [5] observations (the sum of lim_i)   [6] 0   [7] 0
 * seed NULL = no seeds, first_new 0.  The seed arrays must not overlap this call's outputs, with one exception: d_first_new may
 * be this call's own d_summary (it is read before the summary is written).
 * Asynchronous on `stream` (hipStream_t, NULL = the context's stream), no host synchronisation, no allocation per call once the
 * context's scratch has grown to the call's size (a 64-bit claim word per row of the chain, cleared by the call itself, and
 * nodes x ceil(rows_cap / 256) sums).  BRISK_HIP_ERR_ARG, before anything is launched: nodes < 1, rows_cap < 1, node_rows_stride < 1,
 * a NULL array (d_offsets and d_matches may be NULL when nodes == 1: there are no pairs and every row is a head; a seed needs both
 * of d_track and d_age or neither), a misaligned array (d_matches 16-byte, the long long arrays 8-byte, the int arrays 4-byte). */
int brisk_hip_link_tracks_device(brisk_hip_ctx* ctx, const int* d_node_rows, int node_rows_stride, int nodes, int rows_cap,
                                 const long long* d_offsets, const brisk_hip_dmatch* d_matches, const brisk_hip_track_seed* seed,
                                 int* d_prev, long long* d_track, int* d_age, long long* d_summary, void* stream);
/* Packs the tracks worth keeping.  A track PIECE is a head and the rows that follow it in this call; it is LISTED iff (the age of
 * its last row + 1) >= min_len - a continued track counts its length before the call.  Listed pieces are stored in (node, row)
 * order of their heads, each piece's observations in node order: exact prefix sums, stable compaction, no atomics.
 *   d_list_track   [tracks_cap]      the piece's track number
 *   d_list_len     [tracks_cap]      the age of its last row + 1
 *   d_list_offsets [tracks_cap + 1]  exclusive prefix sums of the in-call observation counts
 *   d_list_obs     [obs_cap]         the observations
 *   d_summary      four long long:   pieces listed, their observations, pieces stored, flags
 * The first piece that does not fit tracks_cap or obs_cap is cut together with every piece behind it (the cut
 * brisk_hip_select_pair_matches_device makes): the true counts are still reported, nothing of the cut pieces is stored,
 * d_list_offsets[stored] = the observations stored, BRISK_HIP_TRACKS_CUT is set in the flags.  Nothing behind the stored counts is
 * written.  d_prev / d_track / d_age: what brisk_hip_link_tracks_device wrote for this chain.  Asynchronous and allocation-free
 * like it (scratch: 16 bytes per row of the chain).  BRISK_HIP_ERR_ARG, before anything is launched: the chain's errors, min_len <
 * 1, a negative capacity, a NULL or misaligned array (d_list_obs 8-byte; it may be NULL when obs_cap == 0, d_list_track and
 * d_list_len when tracks_cap == 0). */
typedef struct brisk_hip_track_obs {
  int node, row;
} brisk_hip_track_obs;
#define BRISK_HIP_TRACKS_CUT 0x1
int brisk_hip_list_tracks_device(brisk_hip_ctx* ctx, const int* d_node_rows, int node_rows_stride, int nodes, int rows_cap,
                                 const int* d_prev, const long long* d_track, const int* d_age, int min_len, long long tracks_cap,
                                 long long obs_cap, long long* d_list_track, int* d_list_len, long long* d_list_offsets,
                                 brisk_hip_track_obs* d_list_obs, long long* d_summary, void* stream);

/* ---- the tracker's exit: the listed tracks with their keypoints, on the device or in HOST memory -----------------------------
 * What a host consumer of tracks needs per track - its number, its length, the image positions it was seen at - and nothing else:
 * the observations of a list are resolved to their keypoints on the device, and only the listed tracks cross the link.
 * csrc/brisk_track_points.h is the one definition of the rule.  Point i of a list is observation i of d_list_obs; its kp is the 28
 * bytes at
 *   (const char*)kps->d_kps + (size_t)(kp_first + node * kp_step) * kps->frame_pitch + (size_t)row * 28
 * copied as dwords (NaN payloads and every bit of class_id survive; all address arithmetic is 64-bit).  An observation with node
 * outside [0, nodes) or row outside [0, lim_node) gets 28 zero bytes, and nothing is read from kps for it.  The caller vouches that
 * the frames kp_first + i * kp_step, 0 <= i < nodes, exist in kps and hold lim_i records each (a brisk_hip_kp_set carries no frame
 * count).  With the chain of a descriptor set's frames first + i * step and brisk_hip_batch_kp_set: kp_first = first, kp_step =
 * step. */
typedef struct brisk_hip_track_point { /* 36 bytes, 4-byte aligned */
  int node, row;                       /* the observation, as brisk_hip_track_obs */
  brisk_hip_keypoint kp;               /* byte-identical to the source record */
} brisk_hip_track_point;
/* Device form: the points of a list that brisk_hip_list_tracks_device wrote with this obs_cap.  Writes d_points[0 ..
 * d_list_offsets[stored]), stored = d_list_summary[2] read on the device, nothing behind it; asynchronous on `stream`, no scratch,
 * no allocation.  Like every call of the context it is ordered behind the context's previous call and in front of its next,
 * whichever streams those use: the keypoints and the node rows usually are the last batch's buffers, which the next batch
 * overwrites.  BRISK_HIP_ERR_ARG, before anything is launched: the chain's errors, obs_cap < 0, a NULL d_list_offsets /
 * d_list_summary, a NULL d_list_obs / d_points with obs_cap > 0, d_list_* arrays that are not 8-byte aligned, a d_points that is not
 * 4-byte aligned, NULL kps, a NULL or misaligned d_kps, a frame_pitch that is negative or no multiple of 4, kp_first < 0 or
 * kp_first + (nodes - 1) * kp_step < 0. */
int brisk_hip_track_points_device(brisk_hip_ctx* ctx, const int* d_node_rows, int node_rows_stride, int nodes, int rows_cap,
                                  const long long* d_list_offsets, const brisk_hip_track_obs* d_list_obs, const long long* d_list_summary,
                                  long long obs_cap, const brisk_hip_kp_set* kps, int kp_first, int kp_step, brisk_hip_track_point* d_points,
                                  void* stream);
/* The listed tracks in HOST memory, the way brisk_hip_pair_matches_download delivers matches.  The caller fills in the capacities and
 * the five destination pointers (summary, track and offsets 8-byte aligned, len and points 4-byte; track and len may be NULL when
 * tracks_cap == 0, points when points_cap == 0). */
typedef struct brisk_hip_host_tracks {
  long long tracks_cap, points_cap;
  long long* summary;            /* [4]: pieces listed, their observations, pieces stored, flags (as list_tracks' d_summary) */
  long long* track;              /* [tracks_cap] */
  int* len;                      /* [tracks_cap] */
  long long* offsets;            /* [tracks_cap + 1] */
  brisk_hip_track_point* points; /* [points_cap] */
} brisk_hip_host_tracks;
/* Queues list + points + transfer and returns: the six kernels of brisk_hip_list_tracks_device (tracks_cap, obs_cap = points_cap)
 * and the points kernel run on `stream` (the stream brisk_hip_link_tracks_device ran on; NULL = the context's) into a slab the
 * context owns - d_prev / d_track / d_age and the keypoints may be overwritten by the next batch in stream order -, the transfer
 * runs on the context's second stream.  The exact bytes that cross: summary[0 .. 4), track / len [0, stored), offsets [0, stored],
 * points [0, offsets[stored]); nothing behind them in the caller's arrays is written.  Pinned / registered / managed / device
 * destinations are written by the device directly; pageable ones go through a pinned buffer of the context and a host copy inside
 * brisk_hip_tracks_wait.  *ticket names the transfer.  Two transfers of tracks are in flight per context at most - slots of their
 * own, beside those of brisk_hip_batch_download_all and brisk_hip_pair_matches_download: a stream that downloads rows, matches AND
 * tracks of every batch keeps two batches in flight -, a third call first completes the oldest.  `dst` (the struct) is copied; its
 * arrays must stay valid until the ticket has been waited for.  BRISK_HIP_ERR_ARG, before anything is launched (*ticket = 0): the
 * errors of brisk_hip_list_tracks_device (capacities: dst's) and of the device form's kps / kp_first / kp_step, NULL dst or
 * ticket, a NULL or misaligned destination array. */
int brisk_hip_tracks_download(brisk_hip_ctx* ctx, const int* d_node_rows, int node_rows_stride, int nodes, int rows_cap,
                              const int* d_prev, const long long* d_track, const int* d_age, int min_len, const brisk_hip_kp_set* kps,
                              int kp_first, int kp_step, const brisk_hip_host_tracks* dst, void* stream, unsigned* ticket);
/* Blocks until transfer `ticket` (and every earlier one of tracks) is complete; the context's lock is not held while waiting.
 * *cut (may be NULL) = 1 when the list was cut, else 0.  BRISK_HIP_OK, or - with every stored piece in place -
 * BRISK_HIP_ERR_CAPACITY when the summary's flags carry BRISK_HIP_TRACKS_CUT.  An unknown ticket: BRISK_HIP_ERR_ARG. */
int brisk_hip_tracks_wait(brisk_hip_ctx* ctx, unsigned ticket, int* cut);

/* ---- per-stage timing: HIP events recorded on the launch stream around every kernel of the batch path ---- */
int brisk_hip_profile_enable(brisk_hip_ctx* ctx, int enable);       /* resets the accumulated calls */
int brisk_hip_profile_stages(void);                                 /* number of stages */
const char* brisk_hip_profile_stage_name(int stage);
/* average milliseconds per stage over the calls since enable/read (at most the last 64); synchronises */
int brisk_hip_profile_read(brisk_hip_ctx* ctx, float* avg_ms, int* calls);
/* frames handled by each timed kernel launch (= frames of the first stream slice of the last batch) */
int brisk_hip_profile_frames_per_launch(brisk_hip_ctx* ctx);

/* The box's own streaming ceiling, measured with the engine's float4 kernels over two buffers of `bytes` each:
 * a device-to-device copy (read + write bytes per second) and a read-only pass.  Reported by bench.py next to the
 * roofline numbers (the spec peak is never reached by any kernel). */
int brisk_hip_stream_ceiling(brisk_hip_ctx* ctx, size_t bytes, double* copy_GBps, double* read_GBps);
/* identifies the kernel sources this library was built from (hash); committed PMC traffic data names the revision
 * it was measured on */
const char* brisk_hip_kernel_revision(void);

#ifdef __cplusplus
}
#endif
#endif /* BRISK_HIP_H_ */
