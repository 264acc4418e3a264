// The guide of the guided pair matchers (brisk_hip_match_knn_pairs_guided_device / brisk_hip_match_radius_pairs_guided_device):
// brisk_match_gate.h's window, centred where the PAIR'S MODEL puts the query keypoint instead of at the keypoint itself.
// `__host__ __device__`: the kernels of brisk_match.hip and the CPU test program tests/cpp/test_match_guide.cc run the SAME code.
// No function here is a CPU fallback of the product.
//
// Pair p has the model record M = d_models[p] (brisk_hip_pair_model).  Only h[0..8], hypothesis and flags of a record are read: the
// records may be what brisk_hip_verify_pair_matches_device wrote for this batch, an earlier batch's, or the caller's own.
//   GUIDED    iff M.hypothesis >= 0 and (M.flags & (BRISK_HIP_PAIR_BAD | BRISK_HIP_PAIR_NO_MODEL)) == 0.
//   CENTRE    of query row q, keypoint (x, y, octave), in a guided pair: x and y converted to double, then - the parenthesised order
//             of brisk_verify_z / brisk_verify_inlier, no contraction -
//               z = (h6 x + h7 y) + h8    u = (h0 x + h1 y) + h2    v = (h3 x + h4 y) + h5
//               cx = (float)(u / z)       cy = (float)(v / z)
//             one IEEE fp64 division each, then the round-to-nearest conversion to fp32.  The division is correctly rounded on both
//             sides (the device build has no fast-math and no reciprocal approximation), so host, device and NumPy float64 agree bit
//             for bit.  In an unguided pair with fallback != 0 the centre is the keypoint itself: cx = x, cy = y, its own bits.
//   HAS A CENTRE iff brisk_verify_finite(cx) && brisk_verify_finite(cy).  z == 0, a NaN model element, a NaN coordinate, an overflow
//             of the conversion and an infinite model element (unless the quotients stay finite: an infinite z alone gives 0) all
//             give none; a row of an unguided pair with fallback == 0 has none.
//   THE MASK  M[q][t] = has_centre(q) && brisk_gate_position(window, cx, cy, T.x, T.y) && brisk_gate_lane's octave rule between Q's
//             and T's octaves: the gate with the lane's position replaced by the centre.  The identity model gives the gated
//             matcher's mask.
// DEVIATION FROM THE VERIFIER, on purpose: no test of the sign of z.  The verifier's inlier rule demands that z has the sign of its
// sample's first point; the reported model was divided by its element of largest magnitude, which loses that sign.  The centre is
// H's image of the point, whatever the sign of z.
#pragma once
#include "brisk_match_gate.h"
#include "brisk_pair_verify.h"

struct BriskMatchGuide {  // mirrors brisk_hip_match_guide
  BriskMatchGate window;  // bounds on T - C; max_octave_diff between Q and T
  int fallback;           // a pair without a usable model: 0 = its rows match nothing, else C = Q
};

// BRISK_HIP_PAIR_BAD | BRISK_HIP_PAIR_NO_MODEL: a record with one of them carries no model
#define BRISK_GUIDE_NO_MODEL_FLAGS (0x2 | 0x8)

BRISK_GATE_HD bool brisk_guide_guided(int hypothesis, int flags) { return hypothesis >= 0 && (flags & BRISK_GUIDE_NO_MODEL_FLAGS) == 0; }

struct BriskGuideCentre {
  float x, y;
  bool has;
};
// H is read in a guided pair only
BRISK_GATE_HD BriskGuideCentre brisk_guide_centre(bool guided, int fallback, const BriskHomography& H, float x, float y) {
  BriskGuideCentre c;
  c.x = x;
  c.y = y;
  if (guided) {
    const double xd = (double)x, yd = (double)y;
    const double z = brisk_verify_z(H, xd, yd);
    const double u = (H.h0 * xd + H.h1 * yd) + H.h2;
    const double v = (H.h3 * xd + H.h4 * yd) + H.h5;
    c.x = (float)(u / z);
    c.y = (float)(v / z);
  }
  c.has = (guided || fallback != 0) && brisk_verify_finite(c.x) && brisk_verify_finite(c.y);
  return c;
}
// what a lane keeps of ITS query keypoint while the train keypoints pass by: the centre and the octaves a train row may have.
// false: the row has no centre and matches nothing
BRISK_GATE_HD bool brisk_guide_lane(const BriskMatchGuide& g, bool guided, const BriskHomography& H, float x, float y, int octave,
                                    BriskGateLane& L) {
  const BriskGuideCentre c = brisk_guide_centre(guided, g.fallback, H, x, y);
  L = brisk_gate_lane(g.window, c.x, c.y, octave);
  return c.has;
}
// the lane holds the TRAIN keypoint (the mutual form's backward scan: t = brisk_gate_lane(window, T.x, T.y, T.octave)); the query row
// passing by comes as what brisk_guide_centre made of it - has-centre and the centre - with its own octave.  The SAME predicate as
// brisk_guide_lane + brisk_gate_query_lane, read from the other side: the difference is still T - C, the model is not inverted
BRISK_GATE_HD bool brisk_guide_train_row(const BriskMatchGate& window, const BriskGateLane& t, bool has, float cx, float cy, int qoct) {
  return has && brisk_gate_train_lane(window, t, cx, cy, qoct);
}
// the predicate as the header states it: M[q][t]
BRISK_GATE_HD bool brisk_guide_allows(const BriskMatchGuide& g, bool guided, const BriskHomography& H, float qx, float qy, int qoct, float tx,
                                      float ty, int toct) {
  BriskGateLane L;
  const bool has = brisk_guide_lane(g, guided, H, qx, qy, qoct, L);
  return has && brisk_gate_query_lane(g.window, L, tx, ty, toct);
}
