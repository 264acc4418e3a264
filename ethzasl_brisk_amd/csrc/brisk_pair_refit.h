// The refit rule of brisk_hip_refit_pair_models_device: a pair's homography (what brisk_hip_verify_pair_matches_device reports - a
// model that is exact for four noisy keypoints and nothing more) fitted again to ALL its inliers by least squares, the inliers
// counted again, for `rounds` rounds.  `__host__ __device__`: k_refit_models (brisk_pair_verify.hip) and the CPU test program
// tests/cpp/test_pair_refit.cc run the SAME code.  No function here is a CPU fallback of the product.
//
// All arithmetic is IEEE fp64 + - x / in the parenthesised order written below (the build has no contraction, no fast-math and no
// reciprocal approximation: the division is correctly rounded, as brisk_match_guide.h relies on), no square root, no library call;
// host, device and a NumPy float64 restatement agree bit for bit.  A pair's records, USABLE records and BAD pairs are those of
// brisk_pair_verify.h; thr2 = double(max_error)^2.
//   (1) the input model.  Pair p HAS ONE iff it is not BAD, brisk_guide_guided(hypothesis, flags) holds for its input record, the
//       record's nine elements are finite and max_error > 0.  A pair without one is treated as the verifier treats a pair without
//       an accepted model: (f) with NO_MODEL, the output model nine zeros, hypothesis -1, inliers 0, valid 0.
//   (2) the score of a model H, sign-free (the reported model lost its sign).  A usable record PASSES iff brisk_verify_within holds
//       with z = brisk_verify_z; npos = the passers with z > 0, nneg those with z < 0.  The INLIERS are the passers with z > 0 if
//       npos >= nneg, else those with z < 0 (z == 0 or NaN: never an inlier).  H and -H score alike.
//   (3) the fit to an inlier set S, n = |S| >= 4.
//       SUMS.  Every sum over S is taken in one order: lane l of 256 starts at +0.0 and adds the terms of the inlier records with
//       list index j = l (mod 256) in ascending j; the 256 partials combine by v = v + v[lane ^ off], off = 32, 16, 8, 4, 2, 1, inside
//       each block of 64 lanes, then ((W0 + W1) + W2) + W3 over the four blocks.
//       NORMALISATION.  (cx, cy, cu, cv) = the sums of (x, y, x', y') / double(n).  a = sum|x - cx| + sum|y - cy| and a' alike on the
//       train side (|v| = v < 0 ? -v : v; two sums each, then one addition); the fit FAILS unless a > 0 and a' > 0.  k = double(2 n) / a,
//       k' alike.  X = (x - cx) k, Y = (y - cy) k, U = (x' - cu) k', V = (y' - cv) k'.
//       NORMAL EQUATIONS of the rows [X Y 1 0 0 0 -XU -YU | U] and [0 0 0 X Y 1 -XV -YV | V] (h8 = 1): the 22 sums of
//       brisk_refit_terms, placed by brisk_refit_system (negation is exact; the element sum 1 is double(n)).
//       SOLVE.  Elimination without pivoting in column order k = 0 .. 7: the fit FAILS unless the pivot a_kk > 0; for each row i > k
//       ascending f = a_ik / a_kk, then a_ij = a_ij - f a_kj for j = k + 1 .. 7 ascending, then b_i = b_i - f b_k.  Back substitution for
//       i = 7 .. 0: s = b_i; s = s - a_ij x_j for j = i + 1 .. 7 ascending; x_i = s / a_ii.
//       DENORMALISATION, multiplied through by k' (no further division).  With the rows (g0 g1 g2) of the normalised solution
//       (x0 x1 x2), (x3 x4 x5), (x6 x7 1): G0 = g0 k, G1 = g1 k, G2 = g2 - (G0 cx + G1 cy); then row 0 + (k' cu) row 2, row 1 + (k' cv)
//       row 2, k' row 2.  The fit FAILS if one of the nine elements is not finite.
//       THE FITTED MODEL is brisk_verify_report of these nine: what is scored in the next step IS what is reported (the report of a
//       reported model is the model itself, bit for bit).
//   (4) the rounds.  H_0 = the input model, S_0 its inliers, n_0 = |S_0|.  For r = 1 .. rounds: stop if n_(r-1) < 4 or the fit to
//       S_(r-1) fails; H' = the fitted model, S' its inliers, n' = |S'|; if n' >= n_(r-1), H' REPLACES the model, else stop and keep
//       H_(r-1).  A round with S' = S_(r-1) is a fixed point: every later round computes the same H' and replaces again, so the
//       kernel stops there and counts the remaining rounds as replacing.
//   (5) ACCEPTED iff the pair has an input model and the final count >= min_inliers.  Kept: (f) of the verifier with the final
//       model's inliers.
//   (6) the output record: h = the final model - the input record's nine doubles, byte for byte, when no round replaced it -,
//       records / usable as the verifier writes them, inliers = the final count, hypothesis = the input's, valid = the number of
//       rounds that replaced the model, flags = BRISK_HIP_PAIR_REFIT if that number is > 0, plus NO_MODEL if not accepted.
#pragma once
#include "brisk_match_guide.h"
#include "brisk_pair_verify.h"

#define BRISK_REFIT_MAX_ROUNDS 8
#define BRISK_REFIT_LANES 256  // the lanes of the sums' order
#define BRISK_REFIT_SUMS 22    // the sums of the normal equations
#define BRISK_REFIT_PAIR_REFIT 0x10  // BRISK_HIP_PAIR_REFIT

struct BriskPairRefit {  // mirrors brisk_hip_pair_refit
  float max_error;
  int rounds, min_inliers, keep_unverified;
};

BRISK_VERIFY_HD bool brisk_refit_finite(double v) { return (v - v) == 0.0; }

// (1) for a pair that is not BAD
BRISK_VERIFY_HD bool brisk_refit_has_model(const double* h, int hypothesis, int flags, float max_error) {
  bool ok = brisk_guide_guided(hypothesis, flags) && brisk_verify_threshold_on(max_error);
#pragma unroll
  for (int i = 0; i < 9; ++i) ok = ok && brisk_refit_finite(h[i]);
  return ok;
}

// (2) a usable record: 0 = it does not pass (or z is 0 or NaN), +1 / -1 = it passes with z > 0 / z < 0.  (A NaN x gives 0.)
BRISK_VERIFY_HD int brisk_refit_pass(const BriskHomography& H, double thr2, double x, double y, double xt, double yt) {
  const double z = brisk_verify_z(H, x, y);
  const bool within = brisk_verify_within(H, z, thr2, x, y, xt, yt);
  return within ? (z > 0.0 ? 1 : (z < 0.0 ? -1 : 0)) : 0;
}
// the sign whose passers are the inliers, and their number
BRISK_VERIFY_HD int brisk_refit_sign(int npos, int nneg) { return npos >= nneg ? 1 : -1; }
BRISK_VERIFY_HD int brisk_refit_count(int npos, int nneg) { return npos >= nneg ? npos : nneg; }

// (3) both sides' centroids and scales
struct BriskRefitNorm {
  double cx, cy, cu, cv, k, kt;
};
BRISK_VERIFY_HD double brisk_refit_abs(double v) { return v < 0.0 ? -v : v; }
// s: the sums of (x, y, x', y')
BRISK_VERIFY_HD void brisk_refit_centroids(const double* s, int n, BriskRefitNorm& N) {
  const double dn = (double)n;
  N.cx = s[0] / dn;
  N.cy = s[1] / dn;
  N.cu = s[2] / dn;
  N.cv = s[3] / dn;
}
// a record's terms of the spread sums: |x - cx|, |y - cy|, |x' - cu|, |y' - cv|
BRISK_VERIFY_HD void brisk_refit_spread_terms(const BriskRefitNorm& N, double x, double y, double xt, double yt, double* t) {
  t[0] = brisk_refit_abs(x - N.cx);
  t[1] = brisk_refit_abs(y - N.cy);
  t[2] = brisk_refit_abs(xt - N.cu);
  t[3] = brisk_refit_abs(yt - N.cv);
}
// s: the four spread sums; false = a side has no extent
BRISK_VERIFY_HD bool brisk_refit_scales(const double* s, int n, BriskRefitNorm& N) {
  const double a = s[0] + s[1], at = s[2] + s[3];
  const double dn2 = (double)(2 * (long long)n);
  N.k = dn2 / a;
  N.kt = dn2 / at;
  return a > 0.0 && at > 0.0;
}
// a record's 22 terms of the normal equations
BRISK_VERIFY_HD void brisk_refit_terms(const BriskRefitNorm& N, double x, double y, double xt, double yt, double* t) {
  const double X = (x - N.cx) * N.k, Y = (y - N.cy) * N.k, U = (xt - N.cu) * N.kt, V = (yt - N.cv) * N.kt;
  const double XU = X * U, YU = Y * U, XV = X * V, YV = Y * V, W = U * U + V * V;
  t[0] = X * X;
  t[1] = X * Y;
  t[2] = Y * Y;
  t[3] = X;
  t[4] = Y;
  t[5] = XU;
  t[6] = YU;
  t[7] = U;
  t[8] = XV;
  t[9] = YV;
  t[10] = V;
  t[11] = X * XU;
  t[12] = X * YU;
  t[13] = Y * YU;
  t[14] = X * XV;
  t[15] = X * YV;
  t[16] = Y * YV;
  t[17] = t[0] * W;
  t[18] = t[1] * W;
  t[19] = t[2] * W;
  t[20] = X * W;
  t[21] = Y * W;
}
// the augmented system a[8][9], row after row, from the 22 sums s
BRISK_VERIFY_HD void brisk_refit_system(const double* s, int n, double* a) {
  const double dn = (double)n;
  const double rows[8][9] = {{s[0], s[1], s[3], 0.0, 0.0, 0.0, -s[11], -s[12], s[5]},
                             {s[1], s[2], s[4], 0.0, 0.0, 0.0, -s[12], -s[13], s[6]},
                             {s[3], s[4], dn, 0.0, 0.0, 0.0, -s[5], -s[6], s[7]},
                             {0.0, 0.0, 0.0, s[0], s[1], s[3], -s[14], -s[15], s[8]},
                             {0.0, 0.0, 0.0, s[1], s[2], s[4], -s[15], -s[16], s[9]},
                             {0.0, 0.0, 0.0, s[3], s[4], dn, -s[8], -s[9], s[10]},
                             {-s[11], -s[12], -s[5], -s[14], -s[15], -s[8], s[17], s[18], -s[20]},
                             {-s[12], -s[13], -s[6], -s[15], -s[16], -s[9], s[18], s[19], -s[21]}};
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j) a[i * 9 + j] = rows[i][j];
}
// a[8][9] is overwritten; x[8]; false = a pivot is not > 0 (x is then not to be used)
BRISK_VERIFY_HD bool brisk_refit_solve(double* a, double* x) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double piv = a[k * 9 + k];
    ok = ok && piv > 0.0;
#pragma unroll
    for (int i = k + 1; i < 8; ++i) {
      const double f = a[i * 9 + k] / piv;
#pragma unroll
      for (int j = k + 1; j < 9; ++j) a[i * 9 + j] = a[i * 9 + j] - f * a[k * 9 + j];
    }
  }
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    double s = a[i * 9 + 8];
#pragma unroll
    for (int j = i + 1; j < 8; ++j) s = s - a[i * 9 + j] * x[j];
    x[i] = s / a[i * 9 + i];
  }
  return ok;
}
// the normalised solution x[8] -> the fitted model (reported); false = an element is not finite
BRISK_VERIFY_HD bool brisk_refit_denormalise(const double* x, const BriskRefitNorm& N, BriskHomography& H) {
  const double g00 = x[0] * N.k, g01 = x[1] * N.k, g02 = x[2] - (g00 * N.cx + g01 * N.cy);
  const double g10 = x[3] * N.k, g11 = x[4] * N.k, g12 = x[5] - (g10 * N.cx + g11 * N.cy);
  const double g20 = x[6] * N.k, g21 = x[7] * N.k, g22 = 1.0 - (g20 * N.cx + g21 * N.cy);
  const double pu = N.kt * N.cu, pv = N.kt * N.cv;
  const BriskHomography R{g00 + pu * g20, g01 + pu * g21, g02 + pu * g22, g10 + pv * g20, g11 + pv * g21,
                          g12 + pv * g22, N.kt * g20,     N.kt * g21,     N.kt * g22};
  double v[9];
  brisk_verify_report(R, v);
  H = BriskHomography{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
  return brisk_refit_finite(R.h0) && brisk_refit_finite(R.h1) && brisk_refit_finite(R.h2) && brisk_refit_finite(R.h3) &&
         brisk_refit_finite(R.h4) && brisk_refit_finite(R.h5) && brisk_refit_finite(R.h6) && brisk_refit_finite(R.h7) &&
         brisk_refit_finite(R.h8);
}
// the 22 sums of an inlier set of n records -> the fitted model; a: 72 doubles of work space; false = the fit fails
BRISK_VERIFY_HD bool brisk_refit_fit(const double* s, int n, const BriskRefitNorm& N, double* a, BriskHomography& H) {
  double x[8];
  brisk_refit_system(s, n, a);
  const bool solved = brisk_refit_solve(a, x);
  const bool finite = brisk_refit_denormalise(x, N, H);
  return solved && finite;
}

// (4) does the fitted model with n1 inliers replace the model with n0?
BRISK_VERIFY_HD bool brisk_refit_replaces(int n1, int n0) { return n1 >= n0; }
// (5)
BRISK_VERIFY_HD bool brisk_refit_accepted(bool has_model, int count, int min_inliers) { return has_model && count >= min_inliers; }
