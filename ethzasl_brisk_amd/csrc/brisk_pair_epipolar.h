// The rule of brisk_hip_verify_pair_matches_epipolar_device: which records of a pair's packed match list agree with ONE epipolar
// geometry x'^T F x = 0, query -> train, estimated from the records themselves.  brisk_pair_verify.h's homography is right for a
// plane or a pure rotation; left against right and frame against previous frame of a moving camera see depth, and there the
// constraint that holds is the epipolar one.  The model is the LINEAR eight-point one: F is the null vector of the 8 x 9 system of
// eight records, found by elimination with complete pivoting.  RANK 2 IS NOT ENFORCED: the call is a filter that decides which
// records agree with one epipolar geometry, not an estimator of F (eight coplanar points give a degenerate system whose null vector
// still vanishes on the plane's records: the plane is kept).  `__host__ __device__`: k_epipolar_ransac (brisk_pair_verify.hip) and
// the CPU test program tests/cpp/test_pair_epipolar.cc run the SAME code.  No function here is a CPU fallback of the product.
//
// All arithmetic is IEEE fp64 + - x / in the parenthesised order written below (the build has no contraction; the division is
// correctly rounded on host and device, as brisk_pair_refit.h relies on), no square root, no library call: host, device and a NumPy
// float64 restatement agree bit for bit.  No element of F is fixed to 1 beforehand, so rectified stereo (F's last element is 0)
// is no special case.
//
// Pairs, records, USABLE records, BAD pairs, mix and the pair's seed are brisk_pair_verify.h's.  |v| = v < 0 ? -v : v; finite(v):
// v - v == 0.
//   (b) the sample of hypothesis h: EIGHT distinct record indices.  For k = 0..7: r_k = (u64(mix(pair_seed + 8 h + k)) * (m - k))
//       >> 32, then the indices chosen before are walked in ascending order and r_k grows by one for each that is <= r_k (the
//       verifier's (b) with eight draws).  The hypothesis is INVALID if m < 8, if a sampled record is unusable, or if (c) fails.
//   (c) the model.
//       normalisation, per sample and per side: cx = (((x0 + x1) + x2) + ... + x7) / 8.0, cy alike; a = (|x0 - cx| + ... + |x7 -
//       cx|) + (|y0 - cy| + ... + |y7 - cy|), each sum in index order.  The side fails unless a > 0.  k = 16.0 / a, X = (x - cx) k,
//       Y = (y - cy) k; the train side gives U, V and cu, cv, k'.
//       the system: row i = [U X, U Y, U, V X, V Y, V, X, Y, 1] of sampled record i (F row-major).
//       the null vector: for s = 0..7: the element of largest magnitude among rows s..7, columns s..8 - rows ascending, inside a
//       row columns ascending, the scan starts from 0.0 and only a strictly larger magnitude replaces; the model fails unless that
//       magnitude is > 0 and finite; its row and its column are swapped into position s (the column in all eight rows); for the
//       rows i > s ascending: f = a_is / a_ss, a_ij = a_ij - f a_sj for j = s + 1..8.  Then z_8 = 1 and for i = 7..0: t = +0.0, t = t
//       + a_ij z_j for j = i + 1..8 ascending, z_i = (-t) / a_ii.  z_j belongs to the column that stands at position j; the column
//       left at position 8 is the FREE one.
//       denormalisation F = T'^T Fn T: per row i of Fn: G_i0 = f_i0 k, G_i1 = f_i1 k, G_i2 = f_i2 - (G_i0 cx + G_i1 cy); then
//       F_0j = k' G_0j, F_1j = k' G_1j, F_2j = G_2j - (F_0j cu + F_1j cv).  The model fails if an element is not finite.
//       THE MODEL is brisk_verify_report of these nine ((g) of the verifier: every element divided by the one of largest
//       magnitude): what is scored is what is reported.
//   (d) the score, the Sampson distance tested without a division.  For a usable record (x, y) -> (x', y'): l0 = (F0 x + F1 y) +
//       F2, l1 = (F3 x + F4 y) + F5, l2 = (F6 x + F7 y) + F8; r = (x' l0 + y' l1) + l2; m0 = (F0 x' + F3 y') + F6, m1 = (F1 x' + F4 y')
//       + F7; g = ((l0 l0 + l1 l1) + m0 m0) + m1 m1.  INLIER iff g > 0 and r r <= thr2 g, thr2 = double(max_error)^2.  No sign test.
//       max_error <= 0 or NaN: no record is an inlier of anything.
//   (e), (f) winner, ACCEPTED and KEPT: the verifier's, with min_inliers >= 8.
// A system is exactly singular before step 8 - all points of a side equal, or on one line parallel to an axis (a coordinate that
// is the same in all eight points makes three columns zero) - and then gives no model; eight points on another line leave
// rounding residue in the last pivots and give a model like any other, which few records agree with.
#pragma once
#include "brisk_pair_verify.h"

#if defined(__clang__)
#define BRISK_EPIPOLAR_UNROLL _Pragma("unroll")
#define BRISK_EPIPOLAR_HD BRISK_VERIFY_HD __attribute__((always_inline))
#else
#define BRISK_EPIPOLAR_UNROLL
#define BRISK_EPIPOLAR_HD BRISK_VERIFY_HD
#endif

#define BRISK_EPIPOLAR_MIN_SAMPLE 8

struct BriskPairEpipolarModel {  // mirrors brisk_hip_pair_epipolar_model; the layout of BriskPairModel (k_verify_offsets reads the flags)
  double f[9];
  int records, usable, inliers, hypothesis, valid, flags;
};

// named members, row-major: nothing indexes a model dynamically, so it stays in registers
struct BriskFundamental {
  double f0, f1, f2, f3, f4, f5, f6, f7, f8;
};

BRISK_VERIFY_HD double brisk_epipolar_abs(double v) { return v < 0.0 ? -v : v; }
BRISK_VERIFY_HD bool brisk_epipolar_finite(double v) { return (v - v) == 0.0; }

// (b) m >= 8.  idx in draw order.  The indices chosen so far are kept sorted by one pass of min / max per draw
BRISK_EPIPOLAR_HD void brisk_epipolar_sample(uint32_t pair_seed, int h, int m, int (&idx)[8]) {
  const uint32_t base = pair_seed + 8u * (uint32_t)h;
  uint32_t sorted[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  BRISK_EPIPOLAR_UNROLL
  for (int k = 0; k < 8; ++k) {
    uint32_t r = (uint32_t)(((uint64_t)brisk_verify_mix(base + (uint32_t)k) * (uint64_t)(uint32_t)(m - k)) >> 32);
    BRISK_EPIPOLAR_UNROLL
    for (int c = 0; c < 8; ++c)
      if (c < k && sorted[c] <= r) ++r;
    idx[k] = (int)r;
    uint32_t v = r;
    BRISK_EPIPOLAR_UNROLL
    for (int c = 0; c < 8; ++c)
      if (c < k) {
        const uint32_t lo = sorted[c] < v ? sorted[c] : v;
        v = sorted[c] < v ? v : sorted[c];
        sorted[c] = lo;
      }
    sorted[k] = v;
  }
}

// one side of the normalisation: the eight coordinates -> centroid and scale; false: the side has no extent
BRISK_EPIPOLAR_HD bool brisk_epipolar_norm(const double (&x)[8], const double (&y)[8], double& cx, double& cy, double& k) {
  cx = (((((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]) + x[6]) + x[7]) / 8.0;
  cy = (((((((y[0] + y[1]) + y[2]) + y[3]) + y[4]) + y[5]) + y[6]) + y[7]) / 8.0;
  double ax = brisk_epipolar_abs(x[0] - cx), ay = brisk_epipolar_abs(y[0] - cy);
  BRISK_EPIPOLAR_UNROLL
  for (int i = 1; i < 8; ++i) {
    ax = ax + brisk_epipolar_abs(x[i] - cx);
    ay = ay + brisk_epipolar_abs(y[i] - cy);
  }
  const double a = ax + ay;
  k = 16.0 / a;
  return a > 0.0;
}

// step S of the elimination.  Every index below is a constant once the loops are unrolled (S is a template argument so that the
// bounds are constants too): the swaps are compare-selects, the matrix stays in registers.  false: the model fails
template <int S>
BRISK_EPIPOLAR_HD bool brisk_epipolar_step(double (&a)[8][9], int (&perm)[9]) {
  double best = 0.0;
  int pr = S, pc = S;
  BRISK_EPIPOLAR_UNROLL
  for (int i = S; i < 8; ++i) {
    BRISK_EPIPOLAR_UNROLL
    for (int j = S; j < 9; ++j) {
      const double v = brisk_epipolar_abs(a[i][j]);
      const bool more = v > best;
      best = more ? v : best;
      pr = more ? i : pr;
      pc = more ? j : pc;
    }
  }
  if (!(best > 0.0) || !brisk_epipolar_finite(best)) return false;
  // row pr <-> row S (the columns in front of S are not read again)
  BRISK_EPIPOLAR_UNROLL
  for (int j = S; j < 9; ++j) {
    double top = a[S][j];
    BRISK_EPIPOLAR_UNROLL
    for (int i = S + 1; i < 8; ++i) {
      const double v = a[i][j];
      a[i][j] = i == pr ? a[S][j] : v;
      top = i == pr ? v : top;
    }
    a[S][j] = top;
  }
  // column pc <-> column S, in every row (the rows above S carry it into the back substitution)
  BRISK_EPIPOLAR_UNROLL
  for (int i = 0; i < 8; ++i) {
    double left = a[i][S];
    BRISK_EPIPOLAR_UNROLL
    for (int j = S + 1; j < 9; ++j) {
      const double v = a[i][j];
      a[i][j] = j == pc ? a[i][S] : v;
      left = j == pc ? v : left;
    }
    a[i][S] = left;
  }
  {
    int left = perm[S];
    BRISK_EPIPOLAR_UNROLL
    for (int j = S + 1; j < 9; ++j) {
      const int v = perm[j];
      perm[j] = j == pc ? perm[S] : v;
      left = j == pc ? v : left;
    }
    perm[S] = left;
  }
  BRISK_EPIPOLAR_UNROLL
  for (int i = S + 1; i < 8; ++i) {
    const double f = a[i][S] / a[S][S];
    BRISK_EPIPOLAR_UNROLL
    for (int j = S + 1; j < 9; ++j) a[i][j] = a[i][j] - f * a[S][j];
  }
  return true;
}

// row I of the back substitution
template <int I>
BRISK_EPIPOLAR_HD void brisk_epipolar_back(const double (&a)[8][9], double (&z)[9]) {
  double t = 0.0;
  BRISK_EPIPOLAR_UNROLL
  for (int j = I + 1; j < 9; ++j) t = t + a[I][j] * z[j];
  z[I] = (-t) / a[I][I];
}

// the null vector of a (destroyed) -> fn, in the columns' own order; free_col: the column left free.  false: the model fails
BRISK_EPIPOLAR_HD bool brisk_epipolar_null(double (&a)[8][9], double (&fn)[9], int& free_col) {
  int perm[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
  free_col = -1;
  if (!brisk_epipolar_step<0>(a, perm)) return false;
  if (!brisk_epipolar_step<1>(a, perm)) return false;
  if (!brisk_epipolar_step<2>(a, perm)) return false;
  if (!brisk_epipolar_step<3>(a, perm)) return false;
  if (!brisk_epipolar_step<4>(a, perm)) return false;
  if (!brisk_epipolar_step<5>(a, perm)) return false;
  if (!brisk_epipolar_step<6>(a, perm)) return false;
  if (!brisk_epipolar_step<7>(a, perm)) return false;
  double z[9];
  z[8] = 1.0;
  brisk_epipolar_back<7>(a, z);
  brisk_epipolar_back<6>(a, z);
  brisk_epipolar_back<5>(a, z);
  brisk_epipolar_back<4>(a, z);
  brisk_epipolar_back<3>(a, z);
  brisk_epipolar_back<2>(a, z);
  brisk_epipolar_back<1>(a, z);
  brisk_epipolar_back<0>(a, z);
  // the column permutation undone: fn[perm[j]] = z[j]
  BRISK_EPIPOLAR_UNROLL
  for (int c = 0; c < 9; ++c) {
    double v = 0.0;
    BRISK_EPIPOLAR_UNROLL
    for (int j = 0; j < 9; ++j) v = perm[j] == c ? z[j] : v;
    fn[c] = v;
  }
  free_col = perm[8];
  return true;
}

// (c) false: the sample gives no model (F is then not to be used)
BRISK_EPIPOLAR_HD bool brisk_epipolar_model(const BriskVerifyPoints (&p)[8], BriskFundamental& F, int& free_col) {
  double x[8], y[8], u[8], v[8];
  BRISK_EPIPOLAR_UNROLL
  for (int i = 0; i < 8; ++i) {
    x[i] = p[i].x;
    y[i] = p[i].y;
    u[i] = p[i].xt;
    v[i] = p[i].yt;
  }
  free_col = -1;
  double cx, cy, k, cu, cv, kt;
  const bool ok_q = brisk_epipolar_norm(x, y, cx, cy, k);
  const bool ok_t = brisk_epipolar_norm(u, v, cu, cv, kt);
  if (!ok_q || !ok_t) return false;
  double a[8][9];
  BRISK_EPIPOLAR_UNROLL
  for (int i = 0; i < 8; ++i) {
    const double X = (x[i] - cx) * k, Y = (y[i] - cy) * k, U = (u[i] - cu) * kt, V = (v[i] - cv) * kt;
    a[i][0] = U * X;
    a[i][1] = U * Y;
    a[i][2] = U;
    a[i][3] = V * X;
    a[i][4] = V * Y;
    a[i][5] = V;
    a[i][6] = X;
    a[i][7] = Y;
    a[i][8] = 1.0;
  }
  double fn[9];
  if (!brisk_epipolar_null(a, fn, free_col)) return false;
  double g[9];
  BRISK_EPIPOLAR_UNROLL
  for (int i = 0; i < 3; ++i) {
    g[3 * i] = fn[3 * i] * k;
    g[3 * i + 1] = fn[3 * i + 1] * k;
    g[3 * i + 2] = fn[3 * i + 2] - (g[3 * i] * cx + g[3 * i + 1] * cy);
  }
  double d[9];
  bool finite = true;
  BRISK_EPIPOLAR_UNROLL
  for (int j = 0; j < 3; ++j) {
    d[j] = kt * g[j];
    d[3 + j] = kt * g[3 + j];
    d[6 + j] = g[6 + j] - (d[j] * cu + d[3 + j] * cv);
  }
  BRISK_EPIPOLAR_UNROLL
  for (int i = 0; i < 9; ++i) finite = finite && brisk_epipolar_finite(d[i]);
  if (!finite) return false;
  double out[9];
  brisk_verify_report(BriskHomography{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8]}, out);
  F = BriskFundamental{out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], out[8]};
  return true;
}

// (d) for a USABLE record, with the threshold on.  (A NaN x - how the kernels mark an unusable record in LDS - gives a NaN r and false.)
BRISK_VERIFY_HD bool brisk_epipolar_inlier(const BriskFundamental& F, double thr2, double x, double y, double xt, double yt) {
  const double l0 = (F.f0 * x + F.f1 * y) + F.f2;
  const double l1 = (F.f3 * x + F.f4 * y) + F.f5;
  const double l2 = (F.f6 * x + F.f7 * y) + F.f8;
  const double r = (xt * l0 + yt * l1) + l2;
  const double m0 = (F.f0 * xt + F.f3 * yt) + F.f6;
  const double m1 = (F.f1 * xt + F.f4 * yt) + F.f7;
  const double g = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
  return g > 0.0 && r * r <= thr2 * g;
}
