// brisk_track_export.hip - the tracker's exit (brisk_hip_track_points_device, brisk_hip_tracks_download).
//
// brisk_hip_list_tracks_device leaves the tracks worth keeping in HBM: numbers, lengths, offsets and (node, row) observations.  What
// a host consumer wants of them - per track its number, its length and the image positions it was seen at - is resolved here on the
// device (the rule: brisk_track_points.h), and only the listed tracks cross the link:
//   k_tracklist_points  one lane per OUTPUT dword: point i = observation i and the 28 bytes of its keypoint.  The 36-byte records
//                       are written as one run of coalesced dword stores; the keypoint reads are scattered by nature (consecutive
//                       observations of a track lie in different frames).  The number of observations is read on the device.
//   k_tracklist_egress  packed slab -> host memory, the exact bytes only (on the context's egress stream)
#include <hip/hip_runtime.h>

#include "brisk_common.h"
#include "brisk_kernels.h"
#include "brisk_export_copy.h"
#include "brisk_track_points.h"

#define TX_THREADS 256
#define TX_MAX_BLOCKS 1024  // the grid-stride loop takes the rest

// pieces stored = summary[2], observations stored = list_offsets[pieces stored]: kept inside what the arrays hold
__device__ __forceinline__ long long tx_clamp(long long v, long long cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

__global__ void __launch_bounds__(TX_THREADS) k_tracklist_points(const int* __restrict__ node_rows, long long stride, int nodes, int rows_cap,
                                                                 const long long* __restrict__ list_offsets, const int2* __restrict__ list_obs,
                                                                 const long long* __restrict__ list_summary, long long obs_cap,
                                                                 const uint32_t* __restrict__ kp_words, long long frame_pitch, int kp_first,
                                                                 int kp_step, uint32_t* __restrict__ points) {
  const long long stored = list_summary[2];
  if (stored < 0) return;
  const long long words = tx_clamp(list_offsets[stored], obs_cap) * BRISK_TRACK_POINT_WORDS;
  const long long first = (long long)blockIdx.x * TX_THREADS;
  if (first >= words) return;
  for (long long g = first + threadIdx.x; g < words; g += (long long)gridDim.x * TX_THREADS) {
    const long long i = g / BRISK_TRACK_POINT_WORDS;
    const int w = (int)(g - i * BRISK_TRACK_POINT_WORDS);
    const int2 o = list_obs[i];
    points[g] = brisk_track_point_word(node_rows, stride, nodes, rows_cap, kp_words, frame_pitch, kp_first, kp_step, o.x, o.y, w);
  }
}

// summary [4], track / len [0, stored), offsets [0, stored], points [0, offsets[stored]): nothing behind them is written
__global__ void __launch_bounds__(TX_THREADS) k_tracklist_egress(const uint32_t* __restrict__ s_summary, const uint32_t* __restrict__ s_track,
                                                                 const uint32_t* __restrict__ s_len, const uint32_t* __restrict__ s_offsets,
                                                                 const uint32_t* __restrict__ s_points, long long tracks_cap,
                                                                 long long points_cap, uint32_t* h_summary, uint32_t* h_track, uint32_t* h_len,
                                                                 uint32_t* h_offsets, uint32_t* h_points) {
  const long gt = (long)blockIdx.x * blockDim.x + threadIdx.x, gn = (long)gridDim.x * blockDim.x;
  const long long stored = tx_clamp(reinterpret_cast<const long long*>(s_summary)[2], tracks_cap);
  const long long npoints = tx_clamp(reinterpret_cast<const long long*>(s_offsets)[stored], points_cap);
  ex_copy_words(h_summary, s_summary, 8, gt, gn);
  ex_copy_words(h_track, s_track, stored * 2, gt, gn);
  ex_copy_words(h_len, s_len, stored, gt, gn);
  ex_copy_words(h_offsets, s_offsets, (stored + 1) * 2, gt, gn);
  ex_copy_words(h_points, s_points, npoints * BRISK_TRACK_POINT_WORDS, gt, gn);
}

void brisk_launch_tracklist_points(const int* node_rows, long long stride, int nodes, int rows_cap, const long long* list_offsets,
                                   const void* list_obs, const long long* list_summary, long long obs_cap, const void* kps, long long frame_pitch,
                                   int kp_first, int kp_step, void* points, hipStream_t s) {
  if (obs_cap <= 0) return;  // (nothing can be stored)
  const long long blocks = (obs_cap * BRISK_TRACK_POINT_WORDS + TX_THREADS - 1) / TX_THREADS;
  hipLaunchKernelGGL(k_tracklist_points, dim3((unsigned)(blocks < TX_MAX_BLOCKS ? blocks : TX_MAX_BLOCKS)), dim3(TX_THREADS), 0, s, node_rows,
                     stride, nodes, rows_cap, list_offsets, static_cast<const int2*>(list_obs), list_summary, obs_cap,
                     static_cast<const uint32_t*>(kps), frame_pitch, kp_first, kp_step, static_cast<uint32_t*>(points));
}

void brisk_launch_tracklist_egress(const long long* s_summary, const long long* s_track, const int* s_len, const long long* s_offsets,
                                   const void* s_points, long long tracks_cap, long long points_cap, long long* h_summary, long long* h_track,
                                   int* h_len, long long* h_offsets, void* h_points, hipStream_t s) {
  // the link bounds this kernel, not the chip (brisk_launch_export_egress): few workgroups, the CUs stay with the next batch
  hipLaunchKernelGGL(k_tracklist_egress, dim3(48), dim3(TX_THREADS), 0, s, reinterpret_cast<const uint32_t*>(s_summary),
                     reinterpret_cast<const uint32_t*>(s_track), reinterpret_cast<const uint32_t*>(s_len),
                     reinterpret_cast<const uint32_t*>(s_offsets), static_cast<const uint32_t*>(s_points), tracks_cap, points_cap,
                     reinterpret_cast<uint32_t*>(h_summary), reinterpret_cast<uint32_t*>(h_track), reinterpret_cast<uint32_t*>(h_len),
                     reinterpret_cast<uint32_t*>(h_offsets), static_cast<uint32_t*>(h_points));
}
