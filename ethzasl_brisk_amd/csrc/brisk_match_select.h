// The selection rule of brisk_hip_select_pair_matches_device / brisk_hip_pair_matches_download: which of the leading entries of one
// row of a pair matcher's output (d_out [npairs][rows_cap][per_row], d_out_count [npairs][rows_cap]) are delivered.
// `__host__ __device__`: the kernels of brisk_match_export.hip and the CPU test program tests/cpp/test_match_select.cc run the SAME
// code.  No function here is a CPU fallback of the product.
//
// A row's stored entries are e[0 .. min(count, per_row)), in (distance, trainIdx) order.
//   An entry passes iff  e.distance < max_distance  (strict fp32 compare: +INFINITY = no bound, NaN keeps nothing)  and its distance
//   is not the reference's top-up value 2147483648.f (brute-force-matcher.cc:139-153).  DEVIATION FROM THE REFERENCE, on purpose, the
//   same one the gated matchers make: a top-up entry names a train row nobody chose and is never delivered.
//   ratio > 0 (the ratio test; <= 0 or NaN: off): the row gives at most e[0] - iff e[0] passes and either the row has one stored
//     entry, or e[1] is a top-up entry ("no second neighbour"), or  e[0].distance < ratio * e[1].distance  (one fp32 multiplication,
//     one fp32 compare; the build has no contraction).
//   ratio off: the leading entries among the first min(stored, keep_per_row) that pass; the row is sorted by distance, so they are
//     a prefix - the rule stops at the first entry that does not pass.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BRISK_SELECT_HD __host__ __device__ inline
#else
#define BRISK_SELECT_HD inline
#endif

#define BRISK_MATCH_TOPUP_DISTANCE 2147483648.f

struct BriskMatchSelect {  // mirrors brisk_hip_match_select
  float max_distance;
  float ratio;
  int keep_per_row;
};

// entries a row stores: the matchers write min(count, per_row) of the `count` they found (a negative count: none)
BRISK_SELECT_HD int brisk_select_stored(int count, int per_row) { return count < 0 ? 0 : (count < per_row ? count : per_row); }

BRISK_SELECT_HD bool brisk_select_ratio_on(const BriskMatchSelect& s) { return s.ratio > 0.0f; }

BRISK_SELECT_HD bool brisk_select_passes(const BriskMatchSelect& s, float distance) {
  return distance < s.max_distance && distance != BRISK_MATCH_TOPUP_DISTANCE;
}

// Number of LEADING entries of a row that are delivered (0 ... min(stored, keep_per_row); 0 or 1 with the ratio test).
// dist(i): the distance of stored entry i - called for i < stored only, and only for the entries the rule has to look at.
template <class Dist>
BRISK_SELECT_HD int brisk_select_row(const BriskMatchSelect& s, int stored, Dist dist) {
  if (stored < 1) return 0;
  if (brisk_select_ratio_on(s)) {
    const float d0 = dist(0);
    if (!brisk_select_passes(s, d0)) return 0;
    if (stored == 1) return 1;
    const float d1 = dist(1);
    if (d1 == BRISK_MATCH_TOPUP_DISTANCE) return 1;
    const float bound = s.ratio * d1;
    return d0 < bound ? 1 : 0;
  }
  const int lim = stored < s.keep_per_row ? stored : s.keep_per_row;
  int n = 0;
  while (n < lim && brisk_select_passes(s, dist(n))) ++n;
  return n;
}
