// The verification rule of brisk_hip_verify_pair_matches_device: which records of a pair's packed match list (what
// brisk_hip_select_pair_matches_device writes) agree with ONE homography query -> train, estimated from the records themselves.
// The reference judges matches this way (brisk/src/test/test-match.cc:49-126: every matched point goes through H_1to2 and the
// matches whose transfer error exceeds a threshold are counted); here the model is not given but searched among `hypotheses`
// four-record samples.  `__host__ __device__`: the kernels of brisk_pair_verify.hip and the CPU test program
// tests/cpp/test_pair_verify.cc run the SAME code.  No function here is a CPU fallback of the product.
//
// All arithmetic is IEEE fp64 + - x in the parenthesised order written below (the build has no contraction); the decision path
// has no division, no square root and no library call, so host, device and a NumPy float64 restatement agree bit for bit.
//
// Pair p has m records.  Record j is USABLE iff 0 <= queryIdx < lim_a, 0 <= trainIdx < lim_b (lim = brisk_track_lim(count,
// rows_cap), the rows that exist for the linker) and the x and y of both keypoints are finite; its point pair is (x, y) -> (x', y'),
// the four floats converted to double.  An unusable record is never an inlier and never kept; its keypoints are not read.
//   (a) mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on u32.
//   (b) the sample of hypothesis h: four DISTINCT record indices.  For k = 0..3: r_k = (u64(mix(mix(mix(seed ^ 0x9E3779B9) + p)
//       + 4 h + k)) * (m - k)) >> 32, then the indices chosen before are walked in ascending order and r_k grows by one for each
//       that is <= r_k.  The hypothesis is INVALID if m < 4, if a sampled record is unusable, or if (c) fails.
//   (c) the model.  For the four points (x, y, 1) of one side: d, d0, d1, d2 = the determinants of Cramer's rule for
//       [p0 p1 p2] lambda = p3 (brisk_verify_det3: a sum of three 2x2 differences).  The side fails unless each of the four is
//       < 0 or > 0 (zero: three collinear points; NaN).  Its basis is M = [d0 p0 | d1 p1 | d2 p2], and H = B adj(A) with A the
//       query side's basis and B the train side's: every element (b0 c0 + b1 c1) + b2 c2.  No division.
//   (d) the score.  z_ref = z of sample point 0.  A usable record is an INLIER iff z = (H6 x + H7 y) + H8 has z * z_ref > 0 and,
//       with ex = ((H0 x + H1 y) + H2) - z x' and ey alike, (ex ex + ey ey) <= thr2 (z z), thr2 = double(max_error)^2.
//       max_error <= 0 or NaN: no record is an inlier of anything.
//   (e) the winner: the valid hypothesis with the most inliers, ties to the smallest h - the largest key count << 32 | ~h.  The
//       model is ACCEPTED iff a valid hypothesis exists and its count >= min_inliers.
//   (f) kept: an accepted pair keeps the winner's inliers; any other pair its usable records if keep_unverified, else nothing.
//   (g) the reported model: the winner's H, every element divided by the element of largest magnitude (the first on a tie; left
//       as it is when no element has a magnitude > 0).  The only division, outside the decision path.
// Coordinates up to 8191 in magnitude keep every intermediate below 2^280.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BRISK_VERIFY_HD __host__ __device__ inline
#else
#define BRISK_VERIFY_HD inline
#endif

#define BRISK_VERIFY_MAX_HYPOTHESES 4096
#define BRISK_VERIFY_MIN_SAMPLE 4

struct BriskPairVerify {  // mirrors brisk_hip_pair_verify
  float max_error;
  int hypotheses, min_inliers, keep_unverified;
  unsigned seed;
};

struct BriskPairModel {  // mirrors brisk_hip_pair_model
  double h[9];
  int records, usable, inliers, hypothesis, valid, flags;
};

// named members: nothing indexes a model dynamically, so it stays in registers
struct BriskHomography {
  double h0, h1, h2, h3, h4, h5, h6, h7, h8;
};

struct BriskVerifyPoints {  // one record's point pair
  double x, y, xt, yt;
};

BRISK_VERIFY_HD uint32_t brisk_verify_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// what every hypothesis of pair p starts from
BRISK_VERIFY_HD uint32_t brisk_verify_pair_seed(unsigned seed, int p) {
  return brisk_verify_mix(brisk_verify_mix((uint32_t)seed ^ 0x9E3779B9u) + (uint32_t)p);
}

// finite: x - x is 0 (an infinity or a NaN gives NaN); one fp32 subtraction, no library call
BRISK_VERIFY_HD bool brisk_verify_finite(float x) { return (x - x) == 0.0f; }

BRISK_VERIFY_HD bool brisk_verify_index_ok(int query, int train, int lim_a, int lim_b) {
  return query >= 0 && query < lim_a && train >= 0 && train < lim_b;
}

BRISK_VERIFY_HD bool brisk_verify_coords_ok(float x, float y, float xt, float yt) {
  return brisk_verify_finite(x) && brisk_verify_finite(y) && brisk_verify_finite(xt) && brisk_verify_finite(yt);
}

// (b) m >= 4.  i0 .. i3 in draw order (point 0 gives z_ref)
BRISK_VERIFY_HD void brisk_verify_sample(uint32_t pair_seed, int h, int m, int& i0, int& i1, int& i2, int& i3) {
  const uint32_t base = pair_seed + 4u * (uint32_t)h;
  const uint32_t r0 = (uint32_t)(((uint64_t)brisk_verify_mix(base) * (uint64_t)(uint32_t)m) >> 32);
  uint32_t r1 = (uint32_t)(((uint64_t)brisk_verify_mix(base + 1u) * (uint64_t)(uint32_t)(m - 1)) >> 32);
  uint32_t r2 = (uint32_t)(((uint64_t)brisk_verify_mix(base + 2u) * (uint64_t)(uint32_t)(m - 2)) >> 32);
  uint32_t r3 = (uint32_t)(((uint64_t)brisk_verify_mix(base + 3u) * (uint64_t)(uint32_t)(m - 3)) >> 32);
  if (r0 <= r1) ++r1;
  const uint32_t a1 = r0 < r1 ? r0 : r1, b1 = r0 < r1 ? r1 : r0;  // the two chosen, ascending
  if (a1 <= r2) ++r2;
  if (b1 <= r2) ++r2;
  // the three chosen, ascending
  const uint32_t a2 = r2 < a1 ? r2 : a1, c2 = r2 > b1 ? r2 : b1, b2 = r2 < a1 ? a1 : (r2 > b1 ? b1 : r2);
  if (a2 <= r3) ++r3;
  if (b2 <= r3) ++r3;
  if (c2 <= r3) ++r3;
  i0 = (int)r0;
  i1 = (int)r1;
  i2 = (int)r2;
  i3 = (int)r3;
}

// | ax bx cx |
// | ay by cy |  developed along the row of ones: three 2x2 differences, summed left to right
// | 1  1  1  |
BRISK_VERIFY_HD double brisk_verify_det3(double ax, double ay, double bx, double by, double cx, double cy) {
  const double m0 = bx * cy - cx * by;
  const double m1 = cx * ay - ax * cy;
  const double m2 = ax * by - bx * ay;
  return (m0 + m1) + m2;
}

BRISK_VERIFY_HD bool brisk_verify_nonzero(double d) { return d < 0.0 || d > 0.0; }

// one side's projective basis [d0 p0 | d1 p1 | d2 p2], column after column: (m00 m10 m20) is the first column
struct BriskVerifyBasis {
  double m00, m10, m20, m01, m11, m21, m02, m12, m22;
};
BRISK_VERIFY_HD bool brisk_verify_basis(double x0, double y0, double x1, double y1, double x2, double y2, double x3, double y3,
                                        BriskVerifyBasis& M) {
  const double d = brisk_verify_det3(x0, y0, x1, y1, x2, y2);
  const double d0 = brisk_verify_det3(x3, y3, x1, y1, x2, y2);
  const double d1 = brisk_verify_det3(x0, y0, x3, y3, x2, y2);
  const double d2 = brisk_verify_det3(x0, y0, x1, y1, x3, y3);
  M.m00 = d0 * x0;
  M.m10 = d0 * y0;
  M.m20 = d0;
  M.m01 = d1 * x1;
  M.m11 = d1 * y1;
  M.m21 = d1;
  M.m02 = d2 * x2;
  M.m12 = d2 * y2;
  M.m22 = d2;
  return brisk_verify_nonzero(d) && brisk_verify_nonzero(d0) && brisk_verify_nonzero(d1) && brisk_verify_nonzero(d2);
}

// (c) false: the sample gives no model (H is then not to be used)
BRISK_VERIFY_HD bool brisk_verify_model(const BriskVerifyPoints& p0, const BriskVerifyPoints& p1, const BriskVerifyPoints& p2,
                                        const BriskVerifyPoints& p3, BriskHomography& H) {
  BriskVerifyBasis A, B;
  const bool ok_a = brisk_verify_basis(p0.x, p0.y, p1.x, p1.y, p2.x, p2.y, p3.x, p3.y, A);
  const bool ok_b = brisk_verify_basis(p0.xt, p0.yt, p1.xt, p1.yt, p2.xt, p2.yt, p3.xt, p3.yt, B);
  // adj(A): element (i, j) is the cofactor of A's element (j, i)
  const double c00 = A.m11 * A.m22 - A.m12 * A.m21;
  const double c01 = A.m02 * A.m21 - A.m01 * A.m22;
  const double c02 = A.m01 * A.m12 - A.m02 * A.m11;
  const double c10 = A.m12 * A.m20 - A.m10 * A.m22;
  const double c11 = A.m00 * A.m22 - A.m02 * A.m20;
  const double c12 = A.m02 * A.m10 - A.m00 * A.m12;
  const double c20 = A.m10 * A.m21 - A.m11 * A.m20;
  const double c21 = A.m01 * A.m20 - A.m00 * A.m21;
  const double c22 = A.m00 * A.m11 - A.m01 * A.m10;
  H.h0 = (B.m00 * c00 + B.m01 * c10) + B.m02 * c20;
  H.h1 = (B.m00 * c01 + B.m01 * c11) + B.m02 * c21;
  H.h2 = (B.m00 * c02 + B.m01 * c12) + B.m02 * c22;
  H.h3 = (B.m10 * c00 + B.m11 * c10) + B.m12 * c20;
  H.h4 = (B.m10 * c01 + B.m11 * c11) + B.m12 * c21;
  H.h5 = (B.m10 * c02 + B.m11 * c12) + B.m12 * c22;
  H.h6 = (B.m20 * c00 + B.m21 * c10) + B.m22 * c20;
  H.h7 = (B.m20 * c01 + B.m21 * c11) + B.m22 * c21;
  H.h8 = (B.m20 * c02 + B.m21 * c12) + B.m22 * c22;
  return ok_a && ok_b;
}

BRISK_VERIFY_HD double brisk_verify_z(const BriskHomography& H, double x, double y) { return (H.h6 * x + H.h7 * y) + H.h8; }

// thr2 = double(max_error)^2; meaningful for max_error > 0 only (brisk_verify_threshold_on)
BRISK_VERIFY_HD bool brisk_verify_threshold_on(float max_error) { return max_error > 0.0f; }
BRISK_VERIFY_HD double brisk_verify_thr2(float max_error) { return (double)max_error * (double)max_error; }

// (d) for a USABLE record, with the threshold on.  (A NaN x - how the kernels mark an unusable record in LDS - gives a NaN z and false.)
// the error test alone, z = brisk_verify_z(H, x, y) (brisk_pair_refit.h scores with it too)
BRISK_VERIFY_HD bool brisk_verify_within(const BriskHomography& H, double z, double thr2, double x, double y, double xt, double yt) {
  const double ex = ((H.h0 * x + H.h1 * y) + H.h2) - z * xt;
  const double ey = ((H.h3 * x + H.h4 * y) + H.h5) - z * yt;
  return (ex * ex + ey * ey) <= thr2 * (z * z);
}
BRISK_VERIFY_HD bool brisk_verify_inlier(const BriskHomography& H, double z_ref, double thr2, double x, double y, double xt, double yt) {
  const double z = brisk_verify_z(H, x, y);
  const bool within = brisk_verify_within(H, z, thr2, x, y, xt, yt);
  return z * z_ref > 0.0 && within;
}

// (e) 0 = an invalid hypothesis (a valid one has ~h != 0: h < 2^32 - 1)
BRISK_VERIFY_HD unsigned long long brisk_verify_key(bool valid, int count, int h) {
  return valid ? (((unsigned long long)(unsigned)count << 32) | (unsigned long long)(~(uint32_t)h)) : 0ull;
}
BRISK_VERIFY_HD int brisk_verify_key_hypothesis(unsigned long long key) { return key ? (int)(~(uint32_t)(key & 0xFFFFFFFFull)) : -1; }
BRISK_VERIFY_HD int brisk_verify_key_count(unsigned long long key) { return (int)(key >> 32); }
BRISK_VERIFY_HD bool brisk_verify_accepted(unsigned long long key, int min_inliers) {
  return key != 0ull && brisk_verify_key_count(key) >= min_inliers;
}

// (f)
BRISK_VERIFY_HD bool brisk_verify_keeps(bool accepted, bool usable, bool inlier, int keep_unverified) {
  return usable && (accepted ? inlier : keep_unverified != 0);
}

// (g) out[9]
BRISK_VERIFY_HD void brisk_verify_report(const BriskHomography& H, double* out) {
  const double v[9] = {H.h0, H.h1, H.h2, H.h3, H.h4, H.h5, H.h6, H.h7, H.h8};
  double best = 0.0, scale = 0.0;
  for (int i = 0; i < 9; ++i) {
    const double a = v[i] < 0.0 ? -v[i] : v[i];
    if (a > best) {
      best = a;
      scale = v[i];
    }
  }
  for (int i = 0; i < 9; ++i) out[i] = best > 0.0 ? v[i] / scale : v[i];
}
