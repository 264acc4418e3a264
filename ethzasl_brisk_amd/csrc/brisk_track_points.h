// The point rule of brisk_hip_track_points_device / brisk_hip_tracks_download: how the observations of a track list (what
// brisk_hip_list_tracks_device writes) become points - the observation and the keypoint it names, 36 bytes.  `__host__ __device__`:
// the kernel of brisk_track_export.hip and the CPU test program tests/cpp/test_track_points.cc run the SAME code.  No function here
// is a CPU fallback of the product.
//
// Point i of a list is observation i = (node, row).  Its record is 9 dwords: node, row, then the 7 dwords of the keypoint at
//   (const char*)kps + (kp_first + node * kp_step) * frame_pitch + row * 28
// copied as dwords (NaN payloads and every bit of class_id survive); all address arithmetic is 64-bit.  An observation with node
// outside [0, nodes) or row outside [0, lim_node) - lim_node = brisk_track_lim of that node's count - gets 7 zero dwords, and
// nothing is read for it: neither the count of a node that does not exist nor a keypoint.
#pragma once
#include <stdint.h>

#include "brisk_track_link.h"

#define BRISK_TRACK_KP_WORDS 7                              // dwords of a keypoint record (28 bytes)
#define BRISK_TRACK_POINT_WORDS (2 + BRISK_TRACK_KP_WORDS)  // dwords of a point: node, row, the keypoint

// whether observation (node, row) names a keypoint; node_rows[i * stride] = rows of node i, read for a node of the chain only
BRISK_TRACK_HD bool brisk_track_point_exists(const int* node_rows, long long stride, int nodes, int rows_cap, int node, int row) {
  if (node < 0 || node >= nodes || row < 0) return false;
  return row < brisk_track_lim(node_rows[node * stride], rows_cap);
}

// index of the first dword of the keypoint of (node, row) in the keypoint set (frame_pitch: bytes, a multiple of 4)
BRISK_TRACK_HD long long brisk_track_point_kp_word(long long frame_pitch, int kp_first, int kp_step, int node, int row) {
  const long long frame = (long long)kp_first + (long long)node * (long long)kp_step;
  return (frame * frame_pitch + (long long)row * (4 * BRISK_TRACK_KP_WORDS)) >> 2;
}

// dword w (0 <= w < BRISK_TRACK_POINT_WORDS) of the point of observation (node, row); kp_words: the keypoint set as dwords
BRISK_TRACK_HD uint32_t brisk_track_point_word(const int* node_rows, long long stride, int nodes, int rows_cap, const uint32_t* kp_words,
                                               long long frame_pitch, int kp_first, int kp_step, int node, int row, int w) {
  if (w == 0) return (uint32_t)node;
  if (w == 1) return (uint32_t)row;
  if (!brisk_track_point_exists(node_rows, stride, nodes, rows_cap, node, row)) return 0u;
  return kp_words[brisk_track_point_kp_word(frame_pitch, kp_first, kp_step, node, row) + (w - 2)];
}
