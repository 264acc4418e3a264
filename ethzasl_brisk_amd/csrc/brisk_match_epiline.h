// The guide of the epipolar-guided pair matchers (brisk_hip_match_knn_pairs_epipolar_guided_device /
// brisk_hip_match_radius_pairs_epipolar_guided_device): a train keypoint may match a query keypoint iff it lies within `band` pixels
// of the query keypoint's epipolar line under the PAIR'S MODEL F, inside brisk_match_gate.h's window around the query keypoint itself
// (the disparity range or tracking window along the line), and the gate's octave rule holds.
// `__host__ __device__`: the kernels of brisk_match.hip and the CPU test program tests/cpp/test_match_epiline.cc run the SAME code.
// No function here is a CPU fallback of the product.
//
// All decision arithmetic is IEEE fp64 + - x and compares in the parenthesised order written below: no contraction (the build has
// none), no division, no square root, no library call.  Host, device and a NumPy float64 restatement agree bit for bit.
//
// Pair p has the model record M = d_models[p] (brisk_hip_pair_epipolar_model).  Only f[0..8], hypothesis and flags of a record are
// read: the records may be what brisk_hip_verify_pair_matches_epipolar_device wrote for this batch, an earlier batch's, or the
// caller's own.
//   GUIDED    iff M.hypothesis >= 0 and (M.flags & (BRISK_HIP_PAIR_BAD | BRISK_HIP_PAIR_NO_MODEL)) == 0: brisk_guide_guided.
//   THE LINE  of query row q, keypoint (x, y, octave), in a guided pair: x and y converted to double, then step (d) of
//             brisk_pair_epipolar.h exactly -
//               l0 = (f0 x + f1 y) + f2    l1 = (f3 x + f4 y) + f5    l2 = (f6 x + f7 y) + f8
//               n = l0 l0 + l1 l1          b2 = double(band) * double(band)          w = b2 * n
//   HAS A LINE iff band > 0 (an fp32 compare: a NaN, zero or negative band gives none) and n > 0 and n and l2 are finite (v - v == 0).
//             w may be +inf: a band of +INFINITY switches the band off, as an infinite bound does in the gate.  A query at an
//             epipole of a rank-2 F (l = 0), a NaN or infinite model element, a NaN coordinate, an overflow of n and the zero model
//             all give no line.
//   THE BAND  for a train keypoint (x', y'), converted to double: r = (x' l0 + y' l1) + l2; it passes iff r r <= w.  A NaN fails;
//             the interval is closed.  (r^2 <= band^2 (l0^2 + l1^2): the point's distance to the line, without a division.)
//   THE MASK  in a guided pair: M[q][t] = has_line(q) && band(q, t) && the gate's predicate of `window` between Q and T - the window
//             is centred on the query keypoint itself, not on a projection.  In an unguided pair with fallback != 0 the band is off
//             and the mask is the plain gate's; with fallback == 0 no row matches anything.
// Two consequences, both exact.  RECTIFIED STEREO REDUCES TO THE GATE: with F = s [0 0 0; 0 0 -1; 0 1 0], s a power of two,
// coordinates whose difference is exact in fp32 and window.dy = -+inf, the mask is the gate's with dy in [-band, band].  THE BAND
// LIES INSIDE THE SAMPSON TEST: n <= g of brisk_epipolar_inlier, r and thr2 are computed identically, so every (q, t) the band
// allows with band == max_error and finite coordinates is an inlier of that F under brisk_pair_epipolar.h (d).
#pragma once
#include "brisk_match_gate.h"
#include "brisk_match_guide.h"
#include "brisk_pair_epipolar.h"

struct BriskMatchEpiGuide {  // mirrors brisk_hip_match_epipolar_guide
  BriskMatchGate window;     // bounds on T - Q; max_octave_diff between Q and T
  float band;                // pixels on either side of the epipolar line
  int fallback;              // a pair without a usable model: 0 = its rows match nothing, else the plain gate of `window`
};

struct BriskEpiLine {
  double l0, l1, l2;  // F (x, y, 1)
  double w;           // band^2 (l0^2 + l1^2)
};
// the line of (x, y) under F and the band; false: the row has no line (E is still written: what the test program prints)
BRISK_GATE_HD bool brisk_epiguide_line(float band, const BriskFundamental& F, float x, float y, BriskEpiLine& E) {
  const double xd = (double)x, yd = (double)y;
  E.l0 = (F.f0 * xd + F.f1 * yd) + F.f2;
  E.l1 = (F.f3 * xd + F.f4 * yd) + F.f5;
  E.l2 = (F.f6 * xd + F.f7 * yd) + F.f8;
  const double n = E.l0 * E.l0 + E.l1 * E.l1;
  const double b2 = (double)band * (double)band;
  E.w = b2 * n;
  return band > 0.0f && n > 0.0 && brisk_epipolar_finite(n) && brisk_epipolar_finite(E.l2);
}
BRISK_GATE_HD bool brisk_epiguide_band(const BriskEpiLine& E, float tx, float ty) {
  const double r = ((double)tx * E.l0 + (double)ty * E.l1) + E.l2;
  return r * r <= E.w;
}

// what a lane keeps of ITS query keypoint while the train keypoints pass by: the gate's lane (its own position, the octaves a train
// row may have) and the line.  The line is read in a guided pair only
struct BriskEpiLane {
  BriskGateLane gate;
  BriskEpiLine line;
};
// F is read in a guided pair only.  false: the row matches nothing - no line in a guided pair, no fallback in an unguided one
BRISK_GATE_HD bool brisk_epiguide_lane(const BriskMatchEpiGuide& g, bool guided, const BriskFundamental& F, float x, float y, int octave,
                                       BriskEpiLane& L) {
  L.gate = brisk_gate_lane(g.window, x, y, octave);
  L.line = BriskEpiLine{0.0, 0.0, 0.0, 0.0};
  if (guided) return brisk_epiguide_line(g.band, F, x, y, L.line);
  return g.fallback != 0;
}
// the lane holds the QUERY keypoint, (tx, ty, toct) is the train row passing by; `guided`: the band is on
BRISK_GATE_HD bool brisk_epiguide_query_lane(const BriskMatchGate& window, bool guided, const BriskGateLane& q, const BriskEpiLine& E, float tx,
                                             float ty, int toct) {
  return (!guided || brisk_epiguide_band(E, tx, ty)) && brisk_gate_query_lane(window, q, tx, ty, toct);
}
// the lane holds the TRAIN keypoint (the mutual form's backward scan: t = brisk_gate_lane(window, T.x, T.y, T.octave)); the query row
// passing by comes as what brisk_epiguide_lane made of it - `has` and the line E - with its own keypoint.  The SAME predicate as
// brisk_epiguide_query_lane behind has, read from the other side: the band is still the train point against the QUERY's line
BRISK_GATE_HD bool brisk_epiguide_train_row(const BriskMatchGate& window, bool guided, const BriskGateLane& t, bool has, const BriskEpiLine& E,
                                            float qx, float qy, int qoct) {
  return has && (!guided || brisk_epiguide_band(E, t.x, t.y)) && brisk_gate_train_lane(window, t, qx, qy, qoct);
}
// the predicate as the header states it: M[q][t]
BRISK_GATE_HD bool brisk_epiguide_allows(const BriskMatchEpiGuide& g, bool guided, const BriskFundamental& F, float qx, float qy, int qoct,
                                         float tx, float ty, int toct) {
  BriskEpiLane L;
  const bool has = brisk_epiguide_lane(g, guided, F, qx, qy, qoct, L);
  return has && brisk_epiguide_query_lane(g.window, guided, L.gate, L.line, tx, ty, toct);
}
