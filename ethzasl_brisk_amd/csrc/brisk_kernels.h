// brisk_kernels.h - host-visible launch interface of brisk_kernels.hip
#pragma once
#include <hip/hip_runtime.h>

#include "brisk_common.h"
#include "brisk_match_gate.h"
#include "brisk_match_epiline.h"
#include "brisk_match_guide.h"
#include "brisk_match_select.h"
#include "brisk_pair_verify.h"
#include "brisk_pair_refit.h"
#include "brisk_pair_epipolar.h"
#include "brisk_pair_epipolar_refit.h"
#include "brisk_track_link.h"
#include "brisk_track_points.h"

#define BRISK_DETECT_TILE_W 64
#ifndef BRISK_DETECT_ROWS_PER_THREAD
#define BRISK_DETECT_ROWS_PER_THREAD 4
#endif
#define BRISK_DETECT_TILE_H (16 * BRISK_DETECT_ROWS_PER_THREAD)

struct BriskTileTable {
  int first_tile[BRISK_MAX_LAYERS + 1];
  int tiles_x[BRISK_MAX_LAYERS];
  int total_tiles;
};

// per-batch device buffers of the detector (arrays over frame slots)
struct BriskDetectBuffers {
  uint8_t* pyr;                  // [slots][pyr_elems]
  uint16_t* smap;                // [slots][pyr_elems]
  BriskCand* cand;               // [slots][cand_cap]
  uint8_t* blocks;               // [slots][cand_cap][64] score blocks of the candidates
  int* tie_idx;                  // [slots][BRISK_MAX_LAYERS][tie_cap]
  unsigned* keys;                // [slots][2 * cand_cap]
  BriskFrameCounters* counters;  // [slots]
  BriskKeyPoint* kp_out;         // [slots][kp_cap]
  uint32_t* bandsum;             // [slots][nbands][istride] column sums of band_h-row bands of layer 0 (for the integral)
  int band_h;                    // 96 after the detector's pyramid (k_pyramid_fused), 64 after the descriptor-only layer-0 kernel
  int istride;                   // integral / bandsum row stride (elements)
  int cand_cap, tie_cap, kp_cap;
};

struct BriskDescribeBuffers {
  uint32_t* integral;  // [slots][iframe_elems] (frame pitch in 4-byte units whatever the element size)
  int istride;         // integral row stride (elements)
  int ibits;           // element size of the integral image of this call, every frame alike: 32, or 24 = 3-byte elements (values
                       // modulo 2^24, row pitch istride * 3 bytes: a quarter less to write and to fetch; BriskPatternDev::int24_ok).
                       // k_describe is instantiated for one of the two per launch: the choice is per CALL (brisk_capi.hip,
                       // integral_format), never per frame
  long iframe_elems;
  BriskKeyPoint* dkp;  // [slots][kp_cap] filtered keypoints (angle filled in)
  int* dscale;         // [slots][kp_cap]
  int* dperm;          // [slots][kp_cap] processing order of the keypoints (spatially sorted, L2 locality)
  uint4* drec;         // [slots][kp_cap] the keypoints in processing order: {x, y, angle (float bits), scale | index << 8}
  uint8_t* desc;       // [slots][kp_cap][desc_pitch]
  int desc_pitch;
  int* dp_work;        // [slots][dp_work_stride] work area of the multi-workgroup keypoint preparation (brisk_dp_work_ints)
  long dp_work_stride;
};
long brisk_dp_work_ints(int kp_cap);

// Optional per-stage timing with HIP events on the launch stream (bench.py roofline leg).
#define BRISK_PROF_STAGES 9
#define BRISK_PROF_MAX_CALLS 64
struct BriskProfiler {
  bool on = false;
  int calls = 0;                                                   // calls recorded since the last reset
  hipEvent_t ev[BRISK_PROF_MAX_CALLS][BRISK_PROF_STAGES + 1] = {};  // created lazily
  bool used[BRISK_PROF_MAX_CALLS][BRISK_PROF_STAGES + 1] = {};
  // the integral image kernel of a detect + describe batch runs on the side stream: its own event pair
  hipEvent_t side_ev[BRISK_PROF_MAX_CALLS][2] = {};
  bool side_used[BRISK_PROF_MAX_CALLS] = {};
  bool created = false;
};
// stage ids
enum { BRISK_STG_PYRAMID = 0, BRISK_STG_DETECT, BRISK_STG_CLASSIFY, BRISK_STG_TIES, BRISK_STG_FINALIZE,
       BRISK_STG_POSTFILTER /* uniformity enforcement / bucketing (empty interval when both are off) */,
       BRISK_STG_INTEGRAL, BRISK_STG_DESC_PREPARE, BRISK_STG_DESCRIBE };
const char* brisk_stage_name(int i);
void brisk_prof_begin_call(BriskProfiler* P);
void brisk_prof_mark(BriskProfiler* P, int slot, hipStream_t s);  // slot k = start of stage k (k == stages: end)
void brisk_prof_mark_side(BriskProfiler* P, int which, hipStream_t side);  // 0 / 1 = before / after the side-stream kernel
void brisk_prof_destroy(BriskProfiler* P);

// detect + describe in one batch: the integral image runs on `side` beside the detector's latency-bound tail
struct BriskOverlap {
  hipStream_t side;
  hipEvent_t fork, join;
  const BriskDescribeBuffers* Dd;
};
int brisk_device_cus();  // compute units of the current device (cached)
// frames: u8 images, frame f at frames + f*frame_pitch, row pitch row_pitch (device memory)
void brisk_launch_detect(const BriskGeom& G, const BriskTileTable& T, const BriskDetectBuffers& B, int nframes,
                         const uint8_t* frames, long frame_pitch, int row_pitch, const uint8_t* mask,
                         long mask_frame_pitch, int mask_row_pitch, hipStream_t s, BriskProfiler* prof,
                         const BriskOverlap* ov = nullptr);
// zeroes what the previous batch (geometry Gprev, nframes frames) left in the score-state map
void brisk_launch_smap_clear(const BriskGeom& Gprev, const BriskDetectBuffers& B, int nframes, hipStream_t s);
// ComputeScale: pyramid + the provided-keypoint walk for one frame (d_in: n_in keypoints in device memory)
void brisk_launch_compute_scale(const BriskGeom& G, const BriskDetectBuffers& B, const uint8_t* frame, int row_pitch,
                                const BriskKeyPoint* d_in, int n_in, int suppress, hipStream_t s);
// only stages layer 0 (descriptor-only calls)
void brisk_launch_layer0_only(const BriskGeom& G, const BriskDetectBuffers& B, int nframes, const uint8_t* frames,
                              long frame_pitch, int row_pitch, hipStream_t s);
// integral image of layer 0 from the band sums the pyramid kernel left (brisk_kernels.hip)
void brisk_launch_integral(const BriskGeom& G, const uint8_t* pyr, const uint32_t* bandsum, uint32_t* integral, int istride,
                           long iframe_elems, int band_h, int nframes, hipStream_t s, int ibits = 32,
                           BriskFrameCounters* counters = nullptr);
// sum of the batch's candidate counts -> *host_word (pinned, mapped): candidates in bits 0-39, frames in bits 40-63
void brisk_launch_publish_single(const BriskFrameCounters* counters, const BriskKeyPoint* kps, const uint8_t* desc, int which, int max_kp,
                                 int dev_pitch, int expect, uint8_t* host, unsigned o_cnt, unsigned o_kp, unsigned o_desc, int* done,
                                 unsigned seq, hipStream_t s);
void brisk_launch_batch_density(const BriskFrameCounters* counters, int nframes, int cand_cap, long long* host_word, hipStream_t s);
// kp_in: [slots][kp_cap]; n_in: per-frame counts at byte stride n_in_stride
void brisk_launch_describe(const BriskGeom& G, const BriskPatternDev& P, const BriskDetectBuffers& B,
                           const BriskDescribeBuffers& Dd, int nframes, const BriskKeyPoint* kp_in, const int* n_in,
                           long n_in_stride, hipStream_t s, BriskProfiler* prof, const BriskOverlap* ov = nullptr,
                           int n_in_max = -1 /* largest per-frame count if the host knows it, else -1 */);

// ---- the batch path's exit to host memory (brisk_export.hip) ----
struct BriskExportSlab {  // device memory: what k_export_egress writes to the host, in the host's layout
  int* counts;            // [frames]
  int* flags;             // [frames]
  long long* offsets;     // [frames + 1]
  uint32_t* kps;          // [rows_cap][7]
  uint32_t* desc;         // [rows_cap][desc_stride / 4]
};
// counts / flags / exact prefix sums of the last batch's rows (which: 0 detected, 1 described) and the rows themselves
// -> slab, on the batch's stream
void brisk_launch_export_pack(const BriskFrameCounters* counters, const BriskKeyPoint* kps, const uint8_t* desc, int kp_cap, int dev_pitch,
                              int strings, int nframes, int which, long long rows_cap, int desc_stride, int cut_flag,
                              const BriskExportSlab& S, hipStream_t s);
// slab -> host memory the device can write (pinned / registered): the stored rows only
void brisk_launch_export_egress(const BriskExportSlab& S, int nframes, int desc_stride, int* h_counts, int* h_flags, long long* h_offsets,
                                void* h_kps, void* h_desc, hipStream_t s);

// streaming probe (brisk_hip_stream_ceiling): mode 0 copies `bytes` from a to b with 16-byte loads/stores, mode 1 only reads a
void brisk_launch_stream_probe(const void* a, void* b, size_t bytes, int mode, hipStream_t s);

// ---- Hamming brute-force matcher (brisk_match.hip) ----
struct BriskDMatch {  // binary-identical to cv::DMatch
  int queryIdx, trainIdx, imgIdx;
  float distance;
};
void brisk_launch_match_dist(const uint8_t* query, int q_pitch, int q0, int nqb, const uint8_t* train, int t_pitch, int nt,
                             int words, const uint8_t* mask, long mask_pitch, uint16_t* dist, long dist_pitch,
                             hipStream_t s);
void brisk_launch_match_masked_out(const uint8_t* mask, long mask_pitch, int q0, int nqb, const int* img_start,
                                   const int* has_mask, int nimg, int* masked, hipStream_t s);
void brisk_launch_match_knn(const uint16_t* dist, long dist_pitch, int q0, int nqb, int nt, const int* img_start, int nimg,
                            const int* masked, int k, BriskDMatch* out, int* out_count, hipStream_t s);
void brisk_launch_match_radius(const uint16_t* dist, long dist_pitch, int q0, int nqb, int nt, const int* img_start,
                               int nimg, const int* masked, float max_distance, int cap, BriskDMatch* out, int* out_count,
                               int dim_bytes, hipStream_t s);
// k <= 2, one train set, no masks: fused distance + top-2 kernel; false = not covered, use the matrix path
bool brisk_launch_match_knn_fused(const uint8_t* query, int q_pitch, int nq, const uint8_t* train, int t_pitch, int nt,
                                  int words32, int k, BriskDMatch* out, int* out_count, hipStream_t s);

// the frame pairs of a batch in one launch (k <= 2, no masks, descriptors of 16 / 32 / 48 / 64 bytes); the structs mirror
// brisk_hip_desc_set / brisk_hip_pair_spec
struct BriskDescSet {
  const uint8_t* desc;
  const int* counts;
  int count_stride;  // ints
  long frame_pitch;  // bytes
  int row_pitch;     // bytes
  int frames;
};
struct BriskPairSpec {
  int npairs, query_first, query_step, train_first, train_step;
  const int* pairs;  // device: npairs x {query frame, train frame}, or null
};
bool brisk_launch_match_knn_pairs(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int words32, int k, bool cross,
                                  int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s);

// radius matching in the same forms (cap_per_query entries per row, the count = matches found): the pairs of a batch, and one
// query set against one train set with host counts (false = not covered, use brisk_launch_match_dist + brisk_launch_match_radius)
bool brisk_launch_match_radius_pairs(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int words32, float max_distance,
                                     int cap, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s);
bool brisk_launch_match_radius_fused(const uint8_t* query, int q_pitch, int nq, const uint8_t* train, int t_pitch, int nt, int words32,
                                     float max_distance, int cap, BriskDMatch* out, int* out_count, hipStream_t s);

// the same two pair matchers behind a position gate (brisk_match_gate.h) evaluated on the keypoints that belong to the rows; a gated
// k-NN row holds real matches only (min(k, allowed rows) entries, no top-up).  BriskKpSet mirrors brisk_hip_kp_set
struct BriskKpSet {
  const char* kps;   // frame f's record r (BriskKeyPoint, 4-byte aligned) at kps + f * frame_pitch + r * sizeof(BriskKeyPoint)
  long frame_pitch;  // bytes
};
bool brisk_launch_match_knn_pairs_gated(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                        const BriskMatchGate& gate, const BriskPairSpec& P, int words32, int k, bool cross, int rows_cap,
                                        BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s);
bool brisk_launch_match_radius_pairs_gated(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                           const BriskMatchGate& gate, const BriskPairSpec& P, int words32, float max_distance, int cap,
                                           int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s);

// the gated matchers with the window centred where pair p's model models[p] puts the query keypoint (brisk_match_guide.h): k-NN
// without the cross check, and radius.  models: device, [npairs], indexed by PAIR
bool brisk_launch_match_knn_pairs_guided(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                         const BriskPairModel* models, const BriskMatchGuide& guide, const BriskPairSpec& P, int words32, int k,
                                         int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s);
bool brisk_launch_match_radius_pairs_guided(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                            const BriskPairModel* models, const BriskMatchGuide& guide, const BriskPairSpec& P, int words32,
                                            float max_distance, int cap, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows,
                                            hipStream_t s);

// the gated matchers behind the band around the query keypoint's epipolar line under pair p's model models[p]
// (brisk_match_epiline.h): k-NN without the cross check, and radius.  models: device, [npairs], indexed by PAIR
bool brisk_launch_match_knn_pairs_epiline(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                          const BriskPairEpipolarModel* models, const BriskMatchEpiGuide& guide, const BriskPairSpec& P,
                                          int words32, int k, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s);
bool brisk_launch_match_radius_pairs_epiline(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                             const BriskPairEpipolarModel* models, const BriskMatchEpiGuide& guide, const BriskPairSpec& P,
                                             int words32, float max_distance, int cap, int rows_cap, BriskDMatch* out, int* out_count,
                                             int* pair_rows, hipStream_t s);

// the two guided k-NN forms for k = 1 WITH the cross check: a row's match is kept iff the guide's mask, asked from the train side over
// ALL rows of the query frame, gives the row back (brisk_guide_train_row / brisk_epiguide_train_row).  out: [npairs][rows_cap][1]
bool brisk_launch_match_mutual_pairs_guided(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                            const BriskPairModel* models, const BriskMatchGuide& guide, const BriskPairSpec& P, int words32,
                                            int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s);
bool brisk_launch_match_mutual_pairs_epiline(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                             const BriskPairEpipolarModel* models, const BriskMatchEpiGuide& guide, const BriskPairSpec& P,
                                             int words32, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s);

// ---- the pair matchers' exit: selected matches, packed (brisk_match_export.hip; the rule: brisk_match_select.h) ----
// flags of a pair (mirror BRISK_HIP_PAIR_* / BRISK_HIP_ROWS_CUT of brisk_hip.h)
enum { BRISK_PAIR_ROWS_CUT = 1, BRISK_PAIR_BAD = 2, BRISK_PAIR_ENTRIES_CUT = 4, BRISK_PAIR_NO_MODEL = 8, BRISK_PAIR_REFIT = 0x10, BRISK_PAIR_MATCHES_CUT = 0x100 };
int brisk_match_export_blocks_per_pair(int rows_cap);
// out / out_count / pair_rows: what a pair matcher wrote.  blk [npairs * blocks_per_pair] long long and blk_over (ints, as many):
// scratch.  counts / flags [npairs], offsets [npairs + 1], matches [matches_cap] (16-byte aligned, like out); rows_copy: NULL or
// [npairs], a copy of pair_rows
void brisk_launch_pair_select(const BriskDMatch* out, const int* out_count, const int* pair_rows, int npairs, int rows_cap, int per_row,
                              const BriskMatchSelect& sel, long long* blk, int* blk_over, long long matches_cap, int* counts, int* flags,
                              long long* offsets, BriskDMatch* matches, int* rows_copy, hipStream_t s);
// packed results -> host memory the device can write: the stored matches only
void brisk_launch_pair_select_egress(const int* s_rows, const int* s_counts, const int* s_flags, const long long* s_offsets,
                                     const BriskDMatch* s_matches, int npairs, int* h_rows, int* h_counts, int* h_flags, long long* h_offsets,
                                     void* h_matches, hipStream_t s);

// ---- a batch's pair matches checked against a homography (brisk_pair_verify.hip; the rule: brisk_pair_verify.h) ----
// offsets [npairs + 1] / matches [in_cap]: the packed lists of the selection; pair p as the pair matchers resolve P.  Scratch: keep
// [in_cap] bytes (one per input record), kept [npairs] long long.  models / counts / flags [npairs], out_offsets [npairs + 1], out
// [out_cap] (16-byte aligned, like matches).  BRISK_PAIR_NO_MODEL: a pair without an accepted model
void brisk_launch_pair_verify(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK, const BriskPairSpec& P,
                              int rows_cap, const long long* offsets, const BriskDMatch* matches, long long in_cap, const BriskPairVerify& V,
                              unsigned char* keep, long long* kept, long long out_cap, BriskPairModel* models, int* counts, int* flags,
                              long long* out_offsets, BriskDMatch* out, hipStream_t s);
// the verifier with the eight-point epipolar model in the homography's place (the rule: brisk_pair_epipolar.h): its arguments, its
// scratch and its two packing kernels; models [npairs] are BriskPairEpipolarModel records
void brisk_launch_pair_epipolar(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK, const BriskPairSpec& P,
                                int rows_cap, const long long* offsets, const BriskDMatch* matches, long long in_cap, const BriskPairVerify& V,
                                unsigned char* keep, long long* kept, long long out_cap, BriskPairEpipolarModel* models, int* counts, int* flags,
                                long long* out_offsets, BriskDMatch* out, hipStream_t s);
// the pairs' models fitted again to all their inliers (the rule: brisk_pair_refit.h): the verifier's arguments, with the models it
// wrote (in_models [npairs]; models may be the same array) in the place of its sampler.  BRISK_PAIR_REFIT: a round replaced the model
void brisk_launch_pair_refit(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK, const BriskPairSpec& P,
                             int rows_cap, const long long* offsets, const BriskDMatch* matches, long long in_cap,
                             const BriskPairModel* in_models, const BriskPairRefit& R, unsigned char* keep, long long* kept, long long out_cap,
                             BriskPairModel* models, int* counts, int* flags, long long* out_offsets, BriskDMatch* out, hipStream_t s);
// the same for the epipolar verifier's models (the rule: brisk_pair_epipolar_refit.h): F fitted again to all its inliers, rank 2
// enforced if R.rank2
void brisk_launch_pair_epipolar_refit(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                      const BriskPairSpec& P, int rows_cap, const long long* offsets, const BriskDMatch* matches, long long in_cap,
                                      const BriskPairEpipolarModel* in_models, const BriskPairEpipolarRefit& R, unsigned char* keep,
                                      long long* kept, long long out_cap, BriskPairEpipolarModel* models, int* counts, int* flags,
                                      long long* out_offsets, BriskDMatch* out, hipStream_t s);

// ---- a batch's pair matches linked into feature tracks (brisk_track.hip; the rule: brisk_track_link.h) ----
enum { BRISK_TRACK_C_LINKS = 0, BRISK_TRACK_C_LOST = 1, BRISK_TRACK_C_IGNORED = 2, BRISK_TRACK_COUNTERS = 4 };  // the link call's counters
enum { BRISK_TRACK_LIST_CUT = 1 };  // flag bit 0 of the list's summary (mirrors BRISK_HIP_TRACKS_CUT)
int brisk_track_blocks_per_node(int rows_cap);
// node i has node_rows[i * stride] rows; offsets [nodes] / matches: the packed lists of the nodes - 1 pairs (pair p: query node p + 1,
// train node p).  Scratch: claims [nodes * rows_cap] (cleared here), blk [nodes * blocks_per_node], counters [BRISK_TRACK_COUNTERS],
// words [1].  seed_track / seed_age [rows_cap] or both NULL; d_first_new NULL = first_new.  prev / track / age [nodes][rows_cap],
// summary [8]
void brisk_launch_track_link(const int* node_rows, long long stride, int nodes, int rows_cap, const long long* offsets, const BriskDMatch* matches,
                             const long long* seed_track, const int* seed_age, long long first_new, const long long* d_first_new,
                             unsigned long long* claims, long long* blk, unsigned long long* counters, long long* words, int* prev,
                             long long* track, int* age, long long* summary, hipStream_t s);
// prev / track / age: what brisk_launch_track_link wrote for this chain.  Scratch: next, len [nodes * rows_cap] ints, piece as many
// long long, blk_pieces / blk_obs [nodes * blocks_per_node], words [2].  list_track / list_len [tracks_cap], list_offsets
// [tracks_cap + 1], list_obs [obs_cap] x {int node, int row}, summary [4]
void brisk_launch_track_list(const int* node_rows, long long stride, int nodes, int rows_cap, const int* prev, const long long* track,
                             const int* age, int min_len, long long tracks_cap, long long obs_cap, int* next, int* len, long long* piece,
                             long long* blk_pieces, long long* blk_obs, long long* words, long long* list_track, int* list_len,
                             long long* list_offsets, void* list_obs, long long* summary, hipStream_t s);

// ---- the tracker's exit: the listed tracks with their keypoints (brisk_track_export.hip; the rule: brisk_track_points.h) ----
// list_offsets / list_obs / list_summary: what brisk_launch_track_list wrote with this obs_cap.  kps: frame f's record r (28 bytes) at
// kps + f * frame_pitch + r * 28, node i = frame kp_first + i * kp_step.  points [obs_cap] x 36 bytes: {node, row, keypoint}; only
// the points of the stored observations are written
void brisk_launch_tracklist_points(const int* node_rows, long long stride, int nodes, int rows_cap, const long long* list_offsets,
                                   const void* list_obs, const long long* list_summary, long long obs_cap, const void* kps, long long frame_pitch,
                                   int kp_first, int kp_step, void* points, hipStream_t s);
// packed lists (each array 16-byte aligned) -> host memory the device can write: the summary and the stored prefixes only
void brisk_launch_tracklist_egress(const long long* s_summary, const long long* s_track, const int* s_len, const long long* s_offsets,
                                   const void* s_points, long long tracks_cap, long long points_cap, long long* h_summary, long long* h_track,
                                   int* h_len, long long* h_offsets, void* h_points, hipStream_t s);

// ---- uniformity enforcement / keypoint bucketing (brisk_uniformity.hip): optional post-filters of the detector's keypoints ----
void brisk_launch_bucketing(BriskKeyPoint* kp, BriskFrameCounters* counters, int* order, BriskKeyPoint* tmp, int kp_cap, int rows,
                            int cols, int nbu, int nbv, int max_keypoints, int nframes, hipStream_t s);
void brisk_launch_uniformity(BriskKeyPoint* kp, BriskFrameCounters* counters, int* order, BriskKeyPoint* tmp, uint8_t* occ,
                             long occ_frame, int ow, int kp_cap, float scaling, int max_keypoints, int nframes, hipStream_t s);

// ---- 16-bit image functions (brisk_image16.hip); strides in elements ----
void brisk_launch_halfsample16(const uint16_t* src, int sstride, int w, int h, uint16_t* dst, int dstride, hipStream_t s);
void brisk_launch_twothirdsample16(const uint16_t* src, int sstride, int w, int h, uint16_t* dst, int dstride, hipStream_t s);
// rowsum: w x h floats of scratch; out: (h + 1) x (w + 1) floats at row stride ostride
void brisk_launch_integral16(const uint16_t* src, int sstride, int w, int h, float* rowsum, float* out, int ostride, hipStream_t s);
