// The refit rule of brisk_hip_refit_pair_models_epipolar_device: a pair's fundamental matrix (what
// brisk_hip_verify_pair_matches_epipolar_device reports - the linear solution of eight noisy keypoints, exact for its sample and
// nothing more, rank 2 not enforced) fitted again to ALL its inliers by least squares, optionally projected to rank 2, the inliers
// counted again, for `rounds` rounds.  `__host__ __device__`: k_refit_epipolar (brisk_pair_verify.hip) and the CPU test program
// tests/cpp/test_pair_epipolar_refit.cc run the SAME code.  No function here is a CPU fallback of the product.
//
// All arithmetic is IEEE fp64 + - x / in the parenthesised order written below (the build has no contraction, no fast-math and no
// reciprocal approximation: the division is correctly rounded), compares only, no square root, no library call; host, device and a
// NumPy float64 restatement agree bit for bit.  A pair's records, USABLE records and BAD pairs are those of brisk_pair_verify.h;
// thr2 = double(max_error)^2; finite(v): v - v == 0.
//   (1) the input model.  brisk_refit_has_model applied to f, hypothesis and flags of the epipolar record: pair p HAS ONE iff it is
//       not BAD, brisk_guide_guided(hypothesis, flags) holds, the nine elements are finite and max_error > 0.  A pair without one is
//       treated as brisk_pair_refit.h (1) treats it: NO_MODEL, the output model nine zeros, hypothesis -1, inliers 0, valid 0.
//   (2) the score of a model F: a usable record is an INLIER iff brisk_epipolar_inlier holds (the Sampson test of
//       brisk_pair_epipolar.h (d); F and -F score alike, there is no sign).  n = the number of inliers.
//   (3) the fit to an inlier set S, n = |S| >= 8.
//       SUMS.  Every sum over S is taken in the order of brisk_pair_refit.h (3): lane l of 256 starts at +0.0 and adds the terms of
//       the inlier records with list index j = l (mod 256) in ascending j; the 256 partials combine by v = v + v[lane ^ off], off =
//       32, 16, 8, 4, 2, 1, inside each block of 64 lanes, then ((W0 + W1) + W2) + W3 over the four blocks.  In how many sweeps
//       over the records a kernel takes the sums does not enter: every sum has its own order.
//       NORMALISATION.  brisk_refit_centroids, brisk_refit_spread_terms and brisk_refit_scales of brisk_pair_refit.h: the centroids
//       (cx, cy, cu, cv), the scales k = double(2 n) / a and k' alike; the fit FAILS if a side has no extent (a > 0 and a' > 0 do
//       not both hold).  X = (x - cx) k, Y = (y - cy) k, U = (x' - cu) k', V = (y' - cv) k'.
//       NORMAL MATRIX.  A record's row is a = [U X, U Y, U, V X, V Y, V, X, Y, 1] (F row-major; the four products rounded once).  M is
//       the symmetric 9 x 9 matrix of the sums of t_ij = a_i a_j, i <= j - term number 9 i - i (i - 1) / 2 + (j - i), 45 of them -
//       each product rounded once.  a_8 = 1, so t_i8 = a_i exactly, and the (8, 8) element is double(n) (the sum of n ones).  SHARED
//       expressions, equal bit for bit: t_26 = U X = a_0 = t_08, t_27 = U Y = a_1 = t_18, t_56 = V X = a_3 = t_38, t_57 = V Y = a_4 =
//       t_48.  Terms that are merely the same monomial are NOT shared and may differ in the last bit: t_05 = (U X) V and t_23 =
//       U (V X), t_15 and t_24, t_06 = (U X) X and t_26 X, t_01 = (U X)(U Y) and t_22 t_67, and their like.
//       SOLVE: brisk_epirefit_null<9>.  The elimination runs on the full symmetric matrix with DIAGONAL pivoting, no null
//       space and no fixed element chosen beforehand.  For s = 0 .. D - 2: the largest diagonal element among positions s .. D - 1
//       - scanned ascending from 0.0, only a strictly larger value replaces; the fit FAILS unless that value is > 0 and finite; its
//       row and its column are swapped into position s (the row in all columns, the column in all rows); for the rows i > s
//       ascending (the last row included): f = a_is / a_ss, a_ij = a_ij - f a_sj for j = s + 1 .. D - 1 ascending.  Then z_(D-1) = 1
//       and for i = D - 2 .. 0: t = +0.0, t = t + a_ij z_j for j = i + 1 .. D - 1 ascending, z_i = (-t) / a_ii (brisk_epipolar_back).
//       z_j belongs to the index that stands at position j; the index left at position D - 1 is the FREE one.  The result minimises
//       |A f|^2 with the free element held at 1: the analogue of brisk_pair_refit.h's h8 = 1, the element chosen by the data, so
//       rectified stereo (the last element of F is 0) is no special case.
//       RANK 2, if rank2 != 0, in normalised coordinates.  N = Fn^T Fn, N_ij = (F_0i F_0j + F_1i F_1j) + F_2i F_2j (all nine computed:
//       N_ij and N_ji are the same bits); brisk_epirefit_null<3> (two steps, the free element 1) gives e; the fit FAILS if a
//       pivot is not > 0 and finite.  w_i = (F_i0 e0 + F_i1 e1) + F_i2 e2, q = (e0 e0 + e1 e1) + e2 e2; the fit FAILS unless q is
//       finite and > 0; Fn'_ij = Fn_ij - (w_i e_j) / q.  Then Fn' e = 0 up to rounding: e is the epipole in the query frame, and Fn'
//       is the SVD truncation of Fn up to the error of one step of inverse iteration.
//       DENORMALISATION, the expressions of brisk_epipolar_model: per row i of Fn: G_i0 = f_i0 k, G_i1 = f_i1 k, G_i2 = f_i2 - (G_i0 cx
//       + G_i1 cy); then F_0j = k' G_0j, F_1j = k' G_1j, F_2j = G_2j - (F_0j cu + F_1j cv).  The fit FAILS if an element is not finite.
//       THE FITTED MODEL is brisk_verify_report of these nine: what is scored in the next step IS what is reported.
//   (4) the rounds: brisk_pair_refit.h (4) with 8 in the place of 4.  F_0 = the input model, S_0 its inliers.  For r = 1 .. rounds:
//       stop if n_(r-1) < 8 or the fit to S_(r-1) fails; F' = the fitted model, S' its inliers, n' = |S'|; if n' >= n_(r-1), F'
//       REPLACES the model, else stop and keep F_(r-1).  A round with S' = S_(r-1) is a fixed point: every later round computes the
//       same F' and replaces again, so the kernel stops there and counts the remaining rounds as replacing.
//   (5) ACCEPTED iff the pair has an input model and the final count >= min_inliers (>= 8).  Kept: (f) of the verifier with the final
//       model's inliers.
//   (6) the output record: f = the final model - the input record's nine doubles, byte for byte, when no round replaced it -,
//       records / usable as the verifier writes them, inliers = the final count, hypothesis = the input's, valid = the number of
//       rounds that replaced the model, flags = BRISK_HIP_PAIR_REFIT if that number is > 0, plus NO_MODEL if not accepted.
//       A MODEL THAT NO ROUND REPLACED IS STILL THE VERIFIER'S UNENFORCED F, and its record does not carry BRISK_HIP_PAIR_REFIT: the
//       flag is how a caller knows that the record holds a refitted F - and a rank-2 one, if it asked for that.
#pragma once
#include "brisk_pair_epipolar.h"
#include "brisk_pair_refit.h"

#define BRISK_EPIREFIT_TERMS 45  // t_ij, i <= j; the last one is not summed: M_88 = double(n)
#define BRISK_EPIREFIT_SUMS 44
#define BRISK_EPIREFIT_SWEEP 15  // the sums a kernel lane carries at a time: sweeps of 15, 15 and 14

struct BriskPairEpipolarRefit {  // mirrors brisk_hip_pair_epipolar_refit
  float max_error;
  int rounds, min_inliers, keep_unverified, rank2;
};

// what the solve works in - LDS in the kernel: every dynamic index of the rule goes into this memory, none into a local array
struct BriskEpirefitWork {
  double s[BRISK_EPIREFIT_SUMS];  // the sums
  double a[81];                   // M, then the eliminated system
  double n3[9];                   // N = Fn^T Fn
  double z[9];                    // the solution by position
  double fn[9];                   // the normalised F
  double e[3];
  int perm[9];  // the index that stands at each position
};

// (3) a record's row a
BRISK_VERIFY_HD void brisk_epirefit_row(const BriskRefitNorm& N, double x, double y, double xt, double yt, double (&a)[9]) {
  const double X = (x - N.cx) * N.k, Y = (y - N.cy) * N.k, U = (xt - N.cu) * N.kt, V = (yt - N.cv) * N.kt;
  a[0] = U * X;
  a[1] = U * Y;
  a[2] = U;
  a[3] = V * X;
  a[4] = V * Y;
  a[5] = V;
  a[6] = X;
  a[7] = Y;
  a[8] = 1.0;
}
BRISK_VERIFY_HD constexpr int brisk_epirefit_term(int i, int j) { return (9 * i - (i * (i - 1)) / 2) + (j - i); }  // i <= j
// the terms number K0 .. K0 + CNT - 1 of a record (every index is a constant once the loops are unrolled)
template <int K0, int CNT>
BRISK_EPIPOLAR_HD void brisk_epirefit_terms(const double (&a)[9], double (&t)[CNT]) {
  BRISK_EPIPOLAR_UNROLL
  for (int i = 0; i < 9; ++i) {
    BRISK_EPIPOLAR_UNROLL
    for (int j = i; j < 9; ++j) {
      const int k = brisk_epirefit_term(i, j) - K0;
      if (k >= 0 && k < CNT) t[k] = a[i] * a[j];
    }
  }
}
// M from the 44 sums s
BRISK_EPIPOLAR_HD void brisk_epirefit_system(const double* s, int n, double* a) {
  BRISK_EPIPOLAR_UNROLL
  for (int i = 0; i < 9; ++i)
    BRISK_EPIPOLAR_UNROLL
    for (int j = i; j < 9; ++j) {
      const int k = brisk_epirefit_term(i, j);
      const double v = k < BRISK_EPIREFIT_SUMS ? s[k] : (double)n;
      a[i * 9 + j] = v;
      a[j * 9 + i] = v;
    }
}
// the diagonally pivoted elimination of a [D x D] (destroyed) -> z [D] by position, perm [D]; false = a pivot is not > 0 and finite.
// The steps and the rows run in loops, with dynamic indices into a (the kernel's LDS); inside a step every loop over a row's or a
// column's D elements is unrolled over registers with constant indices: the D loads of a row are in flight together, where a
// rolled loop would wait for each (one lane solves, so the memory's latency is the solve's time)
template <int D>
BRISK_EPIPOLAR_HD bool brisk_epirefit_null(double* a, double* z, int* perm) {
  BRISK_EPIPOLAR_UNROLL
  for (int j = 0; j < D; ++j) perm[j] = j;
  for (int s = 0; s < D - 1; ++s) {
    double diag[D];
    BRISK_EPIPOLAR_UNROLL
    for (int i = 0; i < D; ++i) diag[i] = a[i * D + i];
    double best = 0.0;
    int at = s;
    BRISK_EPIPOLAR_UNROLL
    for (int i = 0; i < D; ++i) {  // (positions s .. D - 1, ascending)
      const bool more = i >= s && diag[i] > best;
      best = more ? diag[i] : best;
      at = more ? i : at;
    }
    if (!(best > 0.0) || !brisk_epipolar_finite(best)) return false;
    double u[D], w[D];
    BRISK_EPIPOLAR_UNROLL
    for (int j = 0; j < D; ++j) {  // row at <-> row s
      u[j] = a[s * D + j];
      w[j] = a[at * D + j];
    }
    BRISK_EPIPOLAR_UNROLL
    for (int j = 0; j < D; ++j) {
      a[at * D + j] = u[j];
      a[s * D + j] = w[j];
    }
    BRISK_EPIPOLAR_UNROLL
    for (int i = 0; i < D; ++i) {  // column at <-> column s, in every row
      u[i] = a[i * D + s];
      w[i] = a[i * D + at];
    }
    BRISK_EPIPOLAR_UNROLL
    for (int i = 0; i < D; ++i) {
      a[i * D + at] = u[i];
      a[i * D + s] = w[i];
    }
    const int ps = perm[s], pa = perm[at];
    perm[at] = ps;
    perm[s] = pa;
    BRISK_EPIPOLAR_UNROLL
    for (int j = 0; j < D; ++j) u[j] = a[s * D + j];  // the pivot row
    const double piv = a[s * D + s];
    for (int i = s + 1; i < D; ++i) {
      BRISK_EPIPOLAR_UNROLL
      for (int j = 0; j < D; ++j) w[j] = a[i * D + j];
      const double f = a[i * D + s] / piv;
      BRISK_EPIPOLAR_UNROLL
      for (int j = 0; j < D; ++j)
        if (j > s) a[i * D + j] = w[j] - f * u[j];
    }
  }
  double zz[D];
  zz[D - 1] = 1.0;
  BRISK_EPIPOLAR_UNROLL
  for (int i = D - 2; i >= 0; --i) {
    double t = 0.0;
    BRISK_EPIPOLAR_UNROLL
    for (int j = i + 1; j < D; ++j) t = t + a[i * D + j] * zz[j];
    zz[i] = (-t) / a[i * D + i];
  }
  BRISK_EPIPOLAR_UNROLL
  for (int j = 0; j < D; ++j) z[j] = zz[j];
  return true;
}
// the rank-2 step on W.fn, in place; false = the fit fails
BRISK_VERIFY_HD bool brisk_epirefit_rank2(BriskEpirefitWork& W) {
  double* fn = W.fn;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) W.n3[i * 3 + j] = (fn[i] * fn[j] + fn[3 + i] * fn[3 + j]) + fn[6 + i] * fn[6 + j];
  if (!brisk_epirefit_null<3>(W.n3, W.z, W.perm)) return false;
  for (int j = 0; j < 3; ++j) W.e[W.perm[j]] = W.z[j];
  const double e0 = W.e[0], e1 = W.e[1], e2 = W.e[2];
  const double q = (e0 * e0 + e1 * e1) + e2 * e2;
  if (!(q > 0.0) || !brisk_epipolar_finite(q)) return false;
  for (int i = 0; i < 3; ++i) {
    const double w = (fn[3 * i] * e0 + fn[3 * i + 1] * e1) + fn[3 * i + 2] * e2;
    fn[3 * i] = fn[3 * i] - (w * e0) / q;
    fn[3 * i + 1] = fn[3 * i + 1] - (w * e1) / q;
    fn[3 * i + 2] = fn[3 * i + 2] - (w * e2) / q;
  }
  return true;
}
// W.s: the 44 sums of an inlier set of n records -> the fitted model (reported); free_index: the element held at 1, -1 when the
// solve fails.  false = the fit fails (F is then not to be used)
BRISK_VERIFY_HD bool brisk_epirefit_fit(int n, const BriskRefitNorm& N, int rank2, BriskEpirefitWork& W, BriskFundamental& F, int& free_index) {
  free_index = -1;
  F = BriskFundamental{0., 0., 0., 0., 0., 0., 0., 0., 0.};
  brisk_epirefit_system(W.s, n, W.a);
  if (!brisk_epirefit_null<9>(W.a, W.z, W.perm)) return false;
  free_index = W.perm[8];
  for (int j = 0; j < 9; ++j) W.fn[W.perm[j]] = W.z[j];
  if (rank2 != 0 && !brisk_epirefit_rank2(W)) return false;
  double g[9], d[9];
  BRISK_EPIPOLAR_UNROLL
  for (int i = 0; i < 3; ++i) {
    g[3 * i] = W.fn[3 * i] * N.k;
    g[3 * i + 1] = W.fn[3 * i + 1] * N.k;
    g[3 * i + 2] = W.fn[3 * i + 2] - (g[3 * i] * N.cx + g[3 * i + 1] * N.cy);
  }
  bool finite = true;
  BRISK_EPIPOLAR_UNROLL
  for (int j = 0; j < 3; ++j) {
    d[j] = N.kt * g[j];
    d[3 + j] = N.kt * g[3 + j];
    d[6 + j] = g[6 + j] - (d[j] * N.cu + d[3 + j] * N.cv);
  }
  BRISK_EPIPOLAR_UNROLL
  for (int i = 0; i < 9; ++i) finite = finite && brisk_epipolar_finite(d[i]);
  if (!finite) return false;
  double out[9];
  brisk_verify_report(BriskHomography{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8]}, out);
  F = BriskFundamental{out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], out[8]};
  return true;
}
