// The position gate of the gated pair matchers (brisk_hip_match_knn_pairs_gated_device / brisk_hip_match_radius_pairs_gated_device):
// query row q (keypoint Q) and train row t (keypoint T) may match iff
//   dx_min <= T.x - Q.x <= dx_max  and  dy_min <= T.y - Q.y <= dy_max  and  (max_octave_diff < 0 or |T.octave - Q.octave| <= max_octave_diff)
// `__host__ __device__`: the kernels of brisk_match.hip and the CPU test program tests/cpp/test_match_gate.cc run the SAME code.
// No function here is a CPU fallback of the product.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BRISK_GATE_HD __host__ __device__ inline
#else
#define BRISK_GATE_HD inline
#endif

struct BriskMatchGate {  // mirrors brisk_hip_match_gate
  float dx_min, dx_max, dy_min, dy_max;
  int max_octave_diff;
};

// What a lane keeps of ITS keypoint while the other side's keypoints pass by: the position, and the octaves the other side may have.
// |o' - o| <= m  <=>  o - m <= o' <= o + m in exact arithmetic; the two ends are clamped to the int range, which changes nothing
// for an int o'.  m < 0 (octaves off): the whole range.
struct BriskGateLane {
  float x, y;
  int o_lo, o_hi;
};
BRISK_GATE_HD BriskGateLane brisk_gate_lane(const BriskMatchGate& g, float x, float y, int octave) {
  BriskGateLane l;
  l.x = x;
  l.y = y;
  const long long lo = (long long)octave - g.max_octave_diff, hi = (long long)octave + g.max_octave_diff;
  l.o_lo = g.max_octave_diff < 0 || lo < -2147483647LL - 1 ? (int)(-2147483647LL - 1) : (int)lo;
  l.o_hi = g.max_octave_diff < 0 || hi > 2147483647LL ? 2147483647 : (int)hi;
  return l;
}
// the two differences (one IEEE fp32 subtraction each; the build has no contraction) against the bounds: fp32 compares, so a NaN
// coordinate or bound makes the pair impossible and -INFINITY / +INFINITY switch a bound off
BRISK_GATE_HD bool brisk_gate_position(const BriskMatchGate& g, float qx, float qy, float tx, float ty) {
  const float dx = tx - qx, dy = ty - qy;
  return dx >= g.dx_min && dx <= g.dx_max && dy >= g.dy_min && dy <= g.dy_max;
}
// the lane holds the QUERY keypoint, (tx, ty, toct) is the train row passing by
BRISK_GATE_HD bool brisk_gate_query_lane(const BriskMatchGate& g, const BriskGateLane& q, float tx, float ty, int toct) {
  return brisk_gate_position(g, q.x, q.y, tx, ty) && toct >= q.o_lo && toct <= q.o_hi;
}
// the lane holds the TRAIN keypoint (the cross check's backward scan), (qx, qy, qoct) is the query row passing by
BRISK_GATE_HD bool brisk_gate_train_lane(const BriskMatchGate& g, const BriskGateLane& t, float qx, float qy, int qoct) {
  return brisk_gate_position(g, qx, qy, t.x, t.y) && qoct >= t.o_lo && qoct <= t.o_hi;
}
// the predicate as the header states it: M[q][t]
BRISK_GATE_HD bool brisk_gate_allows(const BriskMatchGate& g, float qx, float qy, int qoct, float tx, float ty, int toct) {
  return brisk_gate_query_lane(g, brisk_gate_lane(g, qx, qy, qoct), tx, ty, toct);
}
