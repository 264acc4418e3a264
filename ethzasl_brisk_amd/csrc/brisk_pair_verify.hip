// brisk_pair_verify.hip - a batch's pair matches checked against a homography (brisk_hip_verify_pair_matches_device).
//
// Between the selection and the linker: the packed lists brisk_hip_select_pair_matches_device leaves in HBM hold whatever survived
// a descriptor test.  brisk_pair_verify.h is the one definition of the rule that decides which of a pair's records agree with ONE
// homography estimated from the records themselves; the output has the selection's format, so the linker and both exits read it
// unchanged.
//   k_verify_ransac   one workgroup per pair, a lane = a hypothesis: the lane builds its H in registers from its four sampled
//                     records, the workgroup streams the pair's records through LDS ({x, y, x', y'} floats, VF_CHUNK a chunk;
//                     every lane reads the SAME LDS address per step: a broadcast, no cross-lane traffic in the loop).  The
//                     winner = the largest key count << 32 | ~h, reduced by wave shuffles and one LDS step.  A last sweep, lane =
//                     record, writes a keep byte per record and the pair's kept count; then the model record.
//                     LOOP ORDER: the pass over 256 hypotheses is the OUTER loop, the chunk the inner one.  A lane then carries
//                     one H and one count at a time (with the chunk outside, every lane would have to carry - or rebuild per
//                     chunk - the models of all its up to 16 passes).  A pair of one chunk (m <= VF_CHUNK, the usual case: the
//                     lists hold a few dozen records a pair) is staged ONCE and stays in LDS for every pass and for the last
//                     sweep; only a longer pair restages its chunks per pass: 1 024 record resolutions against 256 x 1 024 scores.
//   k_epipolar_ransac brisk_hip_verify_pair_matches_epipolar_device (the rule: brisk_pair_epipolar.h): k_verify_ransac with the
//                     eight-point model in the homography's place
//   k_refit_models    brisk_hip_refit_pair_models_device (the rule: brisk_pair_refit.h) in k_verify_ransac's place: one workgroup
//                     per pair, the same staging; lane = record scores the pair's model and adds the partials of the least-squares
//                     sums, wave shuffles plus one LDS step combine them in the rule's order, one lane solves the 8 x 8 system in
//                     LDS; then the keep bytes, the kept count and the model record.
//   k_refit_epipolar  brisk_hip_refit_pair_models_epipolar_device (the rule: brisk_pair_epipolar_refit.h): k_refit_models with the
//                     fundamental matrix in the homography's place - the 44 sums of the 9 x 9 normal matrix in three sweeps of at
//                     most 15 over the chunk in LDS, one lane solves the 9 x 9 system and the 3 x 3 one of the rank-2 step in LDS
// The four share the record helpers (VfPair, vf_resolve, vf_stage), the record writer and the two kernels that pack the result;
// k_verify_ransac and the two refits also the pair's resolution (vf_pair, vf_pair_frames), the reductions and the keep sweep, which
// k_epipolar_ransac writes out for the reason given at that kernel:
//   k_verify_offsets  one workgroup: exclusive prefix sums of the kept counts, counts / flags / offsets, the cut at out_cap (the
//                     chunked scan and the cut of k_pair_select_offsets, brisk_match_export.hip)
//   k_verify_scatter  one workgroup per pair: stable compaction of the kept records in chunks of 256 - a ballot per wave, the wave
//                     totals in LDS, 16-byte loads and stores, no atomics
#include <hip/hip_runtime.h>

#include "brisk_common.h"
#include "brisk_kernels.h"
#include "brisk_track_link.h"

#define VF_THREADS 256
#define VF_WAVES (VF_THREADS / 64)
#define VF_CHUNK 1024          // records staged in LDS at a time (16 bytes each)
#define VF_OFF_THREADS 1024    // the offsets workgroup

// a pair's records: [begin, begin + m) of the packed list.  false: the offsets do not describe a range inside [0, in_cap] of at
// most 2^31 - 1 records - the pair is BAD, nothing of it is read
__device__ __forceinline__ bool vf_range(const long long* __restrict__ offsets, int p, long long in_cap, long long& begin, int& m) {
  const long long b = offsets[p], e = offsets[p + 1];
  begin = b;
  m = 0;
  if (b < 0 || e < b || e > in_cap || e - b > 0x7FFFFFFFll) return false;
  m = (int)(e - b);
  return true;
}

__device__ __forceinline__ double (&vf_coefficients(BriskPairModel& M))[9] { return M.h; }
__device__ __forceinline__ double (&vf_coefficients(BriskPairEpipolarModel& M))[9] { return M.f; }

// the pair's output record, by one lane.  have false: the nine coefficients are zeros.  (c is ONE array and `have` a value: a
// caller that selected between two local arrays by pointer would force both into scratch)
template <class Model>
__device__ __forceinline__ void vf_write_model(Model* dst, const double (&c)[9], bool have, int records, int usable, int inliers, int hypothesis,
                                               int valid, int flags) {
  Model M;
  double (&out)[9] = vf_coefficients(M);
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] = have ? c[i] : 0.0;
  M.records = records;
  M.usable = usable;
  M.inliers = inliers;
  M.hypothesis = hypothesis;
  M.valid = valid;
  M.flags = flags;
  *dst = M;
}

// pair blockIdx.x as its workgroup sees it: its frames, the records [begin, begin + m) in nchunks chunks, the row limits and the
// keypoint bases of the two frames
struct VfPair {
  long long begin;
  int fa, fb, m, nchunks, lim_a, lim_b;
  const char *qk, *tk;
};

// the pair, as the pair matchers resolve it: frames, records, chunks.  false: its offsets or its frames are out of range - nothing
// is kept, nothing of the pair is read, thread 0 has written kept[p] = 0 and the BAD record, and the workgroup returns
template <class Model>
__device__ __forceinline__ bool vf_pair(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P,
                                        const long long* __restrict__ offsets, long long in_cap, long long* __restrict__ kept, Model* models,
                                        VfPair& pr) {
  const int p = blockIdx.x;
  if (P.pairs) {
    pr.fa = P.pairs[2 * (long)p];
    pr.fb = P.pairs[2 * (long)p + 1];
  } else {
    pr.fa = P.query_first + p * P.query_step;
    pr.fb = P.train_first + p * P.train_step;
  }
  const bool range_ok = vf_range(offsets, p, in_cap, pr.begin, pr.m);
  const bool frames_ok = pr.fa >= 0 && pr.fa < Q.frames && pr.fb >= 0 && pr.fb < T.frames;
  pr.nchunks = (pr.m + VF_CHUNK - 1) / VF_CHUNK;
  pr.lim_a = pr.lim_b = 0;  // until vf_pair_frames: no record is usable, no keypoint is read
  pr.qk = pr.tk = nullptr;
  if (range_ok && frames_ok) return true;
  if (threadIdx.x == 0) {
    kept[p] = 0;
    const double none[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    vf_write_model(models + p, none, false, pr.m, 0, 0, -1, 0, BRISK_PAIR_BAD | BRISK_PAIR_NO_MODEL);
  }
  return false;
}

// the row limits and the keypoint bases of a pair vf_pair accepted.  (Behind the kernel's `return`, not inside vf_pair: there
// these loads land in a block of their own, and what the kernel loads next waits for them - one memory latency more per pair)
__device__ __forceinline__ void vf_pair_frames(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                               int rows_cap, VfPair& pr) {
  pr.lim_a = brisk_track_lim(Q.counts[(long)pr.fa * Q.count_stride], rows_cap);
  pr.lim_b = brisk_track_lim(T.counts[(long)pr.fb * T.count_stride], rows_cap);
  pr.qk = QK.kps + (long)pr.fa * QK.frame_pitch;
  pr.tk = TK.kps + (long)pr.fb * TK.frame_pitch;
}

__device__ __forceinline__ const float* vf_kp(const char* kps, int r) {
  return reinterpret_cast<const float*>(kps + (long)r * (long)sizeof(BriskKeyPoint));  // x, y lead the record
}

// record j of the pair's list -> its point pair; false = unusable (nothing is read from the keypoint sets then)
__device__ __forceinline__ bool vf_resolve(const BriskDMatch* __restrict__ matches, const VfPair& pr, int j, float4& pt) {
  const int4 rec = *reinterpret_cast<const int4*>(matches + (pr.begin + j));  // {queryIdx, trainIdx, imgIdx, distance}
  if (!brisk_verify_index_ok(rec.x, rec.y, pr.lim_a, pr.lim_b)) return false;
  const float* q = vf_kp(pr.qk, rec.x);
  const float* t = vf_kp(pr.tk, rec.y);
  pt = make_float4(q[0], q[1], t[0], t[1]);
  return brisk_verify_coords_ok(pt.x, pt.y, pt.z, pt.w);
}

__device__ __forceinline__ BriskVerifyPoints vf_points(const float4& pt) {
  return BriskVerifyPoints{(double)pt.x, (double)pt.y, (double)pt.z, (double)pt.w};
}

// chunk c of the pair -> LDS, resolved once by coalesced lanes; an unusable record is marked by a NaN x
__device__ __forceinline__ void vf_stage(float4* __restrict__ lds, const BriskDMatch* __restrict__ matches, const VfPair& pr, int c) {
  const int n = min(VF_CHUNK, pr.m - c * VF_CHUNK);
  for (int i = threadIdx.x; i < n; i += VF_THREADS) {
    float4 pt;
    if (!vf_resolve(matches, pr, c * VF_CHUNK + i, pt)) pt = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
    lds[i] = pt;
  }
}

// f(record as staged, its list index) for the pair's records, lane = record: lane l sees the indices j = l (mod 256), ascending.  A
// pair of one chunk is resident in LDS; a longer one restages chunk after chunk
template <class F>
__device__ __forceinline__ void vf_each(float4* __restrict__ pts, const BriskDMatch* __restrict__ matches, const VfPair& pr, F f) {
  for (int c = 0; c < pr.nchunks; ++c) {
    if (pr.nchunks > 1) {
      __syncthreads();  // (the chunk before is read)
      vf_stage(pts, matches, pr, c);
      __syncthreads();
    }
    const int n = min(VF_CHUNK, pr.m - c * VF_CHUNK);
    for (int i = threadIdx.x; i < n; i += VF_THREADS) f(pts[i], c * VF_CHUNK + i);
  }
}

// N sums of the workgroup in the refit rule's order: the lanes' partials through the xor butterfly of their wave, the four waves'
// totals through LDS (rows of W >= N), ((W0 + W1) + W2) + W3; every lane gets every sum.  red is free again behind the call
template <int N, class V, int W>
__device__ __forceinline__ void vf_block_sums(V (&v)[N], V (*red)[W], int lane, int wave) {
  static_assert(N <= W && VF_WAVES == 4, "a row holds a wave's sums; the order is written out for four waves");
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] + __shfl_xor(v[i], off, 64);
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) red[wave][i] = v[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  __syncthreads();
}

// the last sweep, lane = record: a keep byte per record; e = {kept, usable} of the pair, on every lane.  inlier(record as staged):
// the final model's verdict on a usable record (an unusable one is not asked: brisk_verify_keeps is `usable && ...`, so its
// verdict changes nothing - the refit, whose brisk_refit_pass takes the NaN mark, shares the sweep on that ground)
template <class Inlier, int W>
__device__ __forceinline__ void vf_keep_sweep(float4* __restrict__ pts, const BriskDMatch* __restrict__ matches, const VfPair& pr,
                                              unsigned char* __restrict__ keep, int (*red)[W], int lane, int wave, bool accepted,
                                              int keep_unverified, int (&e)[2], Inlier inlier) {
  e[0] = e[1] = 0;
  vf_each(pts, matches, pr, [&](const float4& r, int j) {
    const bool usable = r.x == r.x;
    const bool inl = accepted && usable && inlier(r);
    const bool k = brisk_verify_keeps(accepted, usable, inl, keep_unverified);
    keep[pr.begin + j] = k ? 1 : 0;
    e[0] += k ? 1 : 0;
    e[1] += usable ? 1 : 0;
  });
  vf_block_sums(e, red, lane, wave);
}

// the model of hypothesis h of a pair with m >= 4 records, and z_ref; false = invalid
__device__ __forceinline__ bool vf_hypothesis(const BriskDMatch* __restrict__ matches, const VfPair& pr, uint32_t pair_seed, int h,
                                              BriskHomography& H, double& z_ref) {
  const int m = pr.m;
  int i0, i1, i2, i3;
  brisk_verify_sample(pair_seed, h, m, i0, i1, i2, i3);
  float4 a, b, c, d;
  // (every index is below m by construction; a draw that is not - it cannot happen - would make the hypothesis invalid, not a read)
  if ((unsigned)i0 >= (unsigned)m || (unsigned)i1 >= (unsigned)m || (unsigned)i2 >= (unsigned)m || (unsigned)i3 >= (unsigned)m) return false;
  bool ok = vf_resolve(matches, pr, i0, a);
  ok = ok && vf_resolve(matches, pr, i1, b);
  ok = ok && vf_resolve(matches, pr, i2, c);
  ok = ok && vf_resolve(matches, pr, i3, d);
  if (!ok) return false;
  ok = brisk_verify_model(vf_points(a), vf_points(b), vf_points(c), vf_points(d), H);
  z_ref = brisk_verify_z(H, (double)a.x, (double)a.y);
  return ok;
}

__global__ void __launch_bounds__(VF_THREADS) k_verify_ransac(BriskDescSet Q, BriskDescSet T, BriskKpSet QK, BriskKpSet TK, BriskPairSpec P,
                                                              int rows_cap, const long long* __restrict__ offsets,
                                                              const BriskDMatch* __restrict__ matches, long long in_cap, BriskPairVerify V,
                                                              unsigned char* __restrict__ keep, long long* __restrict__ kept,
                                                              BriskPairModel* __restrict__ models) {
  __shared__ float4 pts[VF_CHUNK];
  __shared__ unsigned long long wkey[VF_WAVES];
  __shared__ double win[10];  // the winner's H and z_ref
  __shared__ int wsum[VF_WAVES][2];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  VfPair pr;
  if (!vf_pair(Q, T, P, offsets, in_cap, kept, models, pr)) return;
  vf_pair_frames(Q, T, QK, TK, rows_cap, pr);
  const uint32_t pair_seed = brisk_verify_pair_seed(V.seed, p);
  const bool thr_on = brisk_verify_threshold_on(V.max_error);
  const double thr2 = brisk_verify_thr2(V.max_error);

  if (pr.nchunks == 1) vf_stage(pts, matches, pr, 0);  // stays for every pass and the last sweep
  __syncthreads();

  // ---- the hypotheses: passes of 256 outside, chunks inside ----
  unsigned long long best = 0ull;
  int nvalid = 0;
  if (pr.m >= BRISK_VERIFY_MIN_SAMPLE) {
    const int npass = (V.hypotheses + VF_THREADS - 1) / VF_THREADS;
    for (int pass = 0; pass < npass; ++pass) {
      const int h = pass * VF_THREADS + tid;
      BriskHomography H;
      double z_ref = 0.0;
      bool valid = false;
      if (h < V.hypotheses) valid = vf_hypothesis(matches, pr, pair_seed, h, H, z_ref);
      if (!valid) H = BriskHomography{0., 0., 0., 0., 0., 0., 0., 0., 0.};
      const bool score = valid && thr_on;
      int count = 0;
      for (int c = 0; c < pr.nchunks; ++c) {
        if (pr.nchunks > 1) {
          __syncthreads();  // (the chunk before is read)
          vf_stage(pts, matches, pr, c);
          __syncthreads();
        }
        const int n = min(VF_CHUNK, pr.m - c * VF_CHUNK);
        if (score)
          for (int i = 0; i < n; ++i) {
            const float4 r = pts[i];  // one address for the whole wave: a broadcast
            count += brisk_verify_inlier(H, z_ref, thr2, (double)r.x, (double)r.y, (double)r.z, (double)r.w) ? 1 : 0;
          }
      }
      const unsigned long long key = brisk_verify_key(valid, count, h);
      best = key > best ? key : best;
      nvalid += valid ? 1 : 0;
    }
  }
  // ---- the winner: wave shuffles, one LDS step; the number of valid hypotheses rides along ----
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, 64);
    best = o > best ? o : best;
    nvalid += __shfl_xor(nvalid, off, 64);
  }
  if (lane == 0) { wkey[wave] = best; wsum[wave][0] = nvalid; }
  __syncthreads();
  best = 0ull;
  nvalid = 0;
#pragma unroll
  for (int w = 0; w < VF_WAVES; ++w) {
    const unsigned long long o = wkey[w];
    best = o > best ? o : best;
    nvalid += wsum[w][0];
  }
  const bool accepted = brisk_verify_accepted(best, V.min_inliers);
  const int hwin = brisk_verify_key_hypothesis(best);
  __syncthreads();  // (wsum is written again below)
  if (tid == 0) {
    BriskHomography H{0., 0., 0., 0., 0., 0., 0., 0., 0.};
    double z_ref = 0.0;
    if (hwin >= 0) vf_hypothesis(matches, pr, pair_seed, hwin, H, z_ref);  // the same arithmetic again
    win[0] = H.h0; win[1] = H.h1; win[2] = H.h2; win[3] = H.h3; win[4] = H.h4; win[5] = H.h5; win[6] = H.h6; win[7] = H.h7; win[8] = H.h8;
    win[9] = z_ref;
  }
  __syncthreads();
  const BriskHomography W{win[0], win[1], win[2], win[3], win[4], win[5], win[6], win[7], win[8]};
  const double w_ref = win[9];

  int e[2];  // kept, usable
  vf_keep_sweep(pts, matches, pr, keep, wsum, lane, wave, accepted, V.keep_unverified, e, [&](const float4& r) {
    return brisk_verify_inlier(W, w_ref, thr2, (double)r.x, (double)r.y, (double)r.z, (double)r.w);
  });
  if (tid == 0) {
    kept[p] = e[0];
    double h[9];
    brisk_verify_report(W, h);
    vf_write_model(models + p, h, hwin >= 0, pr.m, e[1], brisk_verify_key_count(best), hwin, nvalid, accepted ? 0 : BRISK_PAIR_NO_MODEL);
  }
}

// ---- the refit (brisk_pair_refit.h) ----
// One workgroup per pair, lane = record for the score and for the sums' partials; every lane carries the same model, inlier sign
// and count (what the reductions and the LDS broadcast of the fitted model give every lane alike), so the round loop is uniform.
// No inlier set is stored: a pass evaluates a record's membership again from the model (some twenty flops).  Lane 0 solves the 8 x 8
// system in LDS.  in_models may be models: every lane has read its pair's record before the first barrier, lane 0 writes behind the last
__global__ void __launch_bounds__(VF_THREADS) k_refit_models(BriskDescSet Q, BriskDescSet T, BriskKpSet QK, BriskKpSet TK, BriskPairSpec P,
                                                             int rows_cap, const long long* __restrict__ offsets,
                                                             const BriskDMatch* __restrict__ matches, long long in_cap,
                                                             const BriskPairModel* in_models, BriskPairRefit R, unsigned char* __restrict__ keep,
                                                             long long* __restrict__ kept, BriskPairModel* models) {
  __shared__ float4 pts[VF_CHUNK];
  __shared__ double red[VF_WAVES][BRISK_REFIT_SUMS];
  __shared__ int ired[VF_WAVES][BRISK_REFIT_SUMS];
  __shared__ double sys[72];  // the augmented system
  __shared__ double fit[10];  // the fitted model; [9] != 0: the fit failed
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  VfPair pr;
  if (!vf_pair(Q, T, P, offsets, in_cap, kept, models, pr)) return;
  vf_pair_frames(Q, T, QK, TK, rows_cap, pr);
  const double thr2 = brisk_verify_thr2(R.max_error);

  // the input record: one address for the whole workgroup
  double hin[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) hin[i] = in_models[p].h[i];
  const int in_hypothesis = in_models[p].hypothesis;
  const bool has_model = brisk_refit_has_model(hin, in_hypothesis, in_models[p].flags, R.max_error);

  if (pr.nchunks == 1) vf_stage(pts, matches, pr, 0);  // stays for every pass
  __syncthreads();

  BriskHomography H{hin[0], hin[1], hin[2], hin[3], hin[4], hin[5], hin[6], hin[7], hin[8]};
  int sign = 0, n = 0, replaced = 0;  // sign 0: nothing is an inlier
  if (has_model) {
    int c[2] = {0, 0};
    vf_each(pts, matches, pr, [&](const float4& r, int) {
      const int s = brisk_refit_pass(H, thr2, (double)r.x, (double)r.y, (double)r.z, (double)r.w);
      c[0] += s > 0 ? 1 : 0;
      c[1] += s < 0 ? 1 : 0;
    });
    vf_block_sums(c, ired, lane, wave);
    sign = brisk_refit_sign(c[0], c[1]);
    n = brisk_refit_count(c[0], c[1]);
    for (int round = 1; round <= R.rounds && n >= BRISK_VERIFY_MIN_SAMPLE; ++round) {
      BriskRefitNorm N;
      double s4[4] = {0.0, 0.0, 0.0, 0.0};
      vf_each(pts, matches, pr, [&](const float4& r, int) {
        const double x = (double)r.x, y = (double)r.y, xt = (double)r.z, yt = (double)r.w;
        const bool in = brisk_refit_pass(H, thr2, x, y, xt, yt) == sign;
        s4[0] = s4[0] + (in ? x : 0.0);
        s4[1] = s4[1] + (in ? y : 0.0);
        s4[2] = s4[2] + (in ? xt : 0.0);
        s4[3] = s4[3] + (in ? yt : 0.0);
      });
      vf_block_sums(s4, red, lane, wave);
      brisk_refit_centroids(s4, n, N);
#pragma unroll
      for (int i = 0; i < 4; ++i) s4[i] = 0.0;
      vf_each(pts, matches, pr, [&](const float4& r, int) {
        const double x = (double)r.x, y = (double)r.y, xt = (double)r.z, yt = (double)r.w;
        const bool in = brisk_refit_pass(H, thr2, x, y, xt, yt) == sign;
        double t[4];
        brisk_refit_spread_terms(N, x, y, xt, yt, t);
#pragma unroll
        for (int i = 0; i < 4; ++i) s4[i] = s4[i] + (in ? t[i] : 0.0);
      });
      vf_block_sums(s4, red, lane, wave);
      if (!brisk_refit_scales(s4, n, N)) break;
      double s22[BRISK_REFIT_SUMS];
#pragma unroll
      for (int i = 0; i < BRISK_REFIT_SUMS; ++i) s22[i] = 0.0;
      vf_each(pts, matches, pr, [&](const float4& r, int) {
        const double x = (double)r.x, y = (double)r.y, xt = (double)r.z, yt = (double)r.w;
        const bool in = brisk_refit_pass(H, thr2, x, y, xt, yt) == sign;
        double t[BRISK_REFIT_SUMS];
        brisk_refit_terms(N, x, y, xt, yt, t);
#pragma unroll
        for (int i = 0; i < BRISK_REFIT_SUMS; ++i) s22[i] = s22[i] + (in ? t[i] : 0.0);
      });
      vf_block_sums(s22, red, lane, wave);
      if (tid == 0) {  // the solve: one lane, in LDS
        BriskHomography F;
        const bool ok = brisk_refit_fit(s22, n, N, sys, F);
        fit[0] = F.h0; fit[1] = F.h1; fit[2] = F.h2; fit[3] = F.h3; fit[4] = F.h4; fit[5] = F.h5; fit[6] = F.h6; fit[7] = F.h7; fit[8] = F.h8;
        fit[9] = ok ? 0.0 : 1.0;
      }
      __syncthreads();
      const BriskHomography F{fit[0], fit[1], fit[2], fit[3], fit[4], fit[5], fit[6], fit[7], fit[8]};
      const bool failed = fit[9] != 0.0;
      __syncthreads();  // (fit is written again in the next round)
      if (failed) break;
      // the fitted model's score; d: the records whose membership differs from the present set's, per candidate sign
      int d[4] = {0, 0, 0, 0};
      vf_each(pts, matches, pr, [&](const float4& r, int) {
        const double x = (double)r.x, y = (double)r.y, xt = (double)r.z, yt = (double)r.w;
        const bool in = brisk_refit_pass(H, thr2, x, y, xt, yt) == sign;
        const int s = brisk_refit_pass(F, thr2, x, y, xt, yt);
        d[0] += s > 0 ? 1 : 0;
        d[1] += s < 0 ? 1 : 0;
        d[2] += (s > 0) != in ? 1 : 0;
        d[3] += (s < 0) != in ? 1 : 0;
      });
      vf_block_sums(d, ired, lane, wave);
      const int n1 = brisk_refit_count(d[0], d[1]), sign1 = brisk_refit_sign(d[0], d[1]);
      if (!brisk_refit_replaces(n1, n)) break;
      H = F;
      sign = sign1;
      n = n1;
      ++replaced;
      if ((sign1 > 0 ? d[2] : d[3]) == 0) {  // a fixed point: every round left fits the same set again
        replaced = R.rounds;
        break;
      }
    }
  }
  const bool accepted = brisk_refit_accepted(has_model, n, R.min_inliers);

  int e[2];  // kept, usable
  vf_keep_sweep(pts, matches, pr, keep, ired, lane, wave, accepted, R.keep_unverified, e, [&](const float4& r) {
    return brisk_refit_pass(H, thr2, (double)r.x, (double)r.y, (double)r.z, (double)r.w) == sign;
  });
  if (tid == 0) {
    kept[p] = e[0];
    const double hout[9] = {H.h0, H.h1, H.h2, H.h3, H.h4, H.h5, H.h6, H.h7, H.h8};
    double h[9];  // the input's nine doubles, byte for byte, when no round replaced them
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = replaced > 0 ? hout[i] : hin[i];
    vf_write_model(models + p, h, has_model, pr.m, e[1], n, has_model ? in_hypothesis : -1, replaced,
                   (replaced > 0 ? BRISK_PAIR_REFIT : 0) | (accepted ? 0 : BRISK_PAIR_NO_MODEL));
  }
}

// kept[p] (the pairs' kept counts) -> exclusive prefix sums in place; per pair: count, flags (the model record's too), offset.  The
// first pair with records that does not fit out_cap and every pair behind it are cut: their counts are reported, their offsets
// stay at the total stored.
__global__ void __launch_bounds__(VF_OFF_THREADS) k_verify_offsets(long long* kept, int npairs, long long out_cap, BriskPairModel* models,
                                                                  int* __restrict__ counts, int* __restrict__ flags,
                                                                  long long* __restrict__ offsets) {
  __shared__ long long part[VF_OFF_THREADS / 64];
  __shared__ int red[VF_OFF_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long n = npairs;
  const long long per = (n + VF_OFF_THREADS - 1) / VF_OFF_THREADS;
  const long long i0 = min(tid * per, n), i1 = min(i0 + per, n);
  long long sum = 0;
  for (long long i = i0; i < i1; ++i) sum += kept[i];
  // exclusive scan of the threads' sums: inside the wave, then over the 16 wave totals
  long long incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const long long v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  long long base = incl - sum, total = 0;
  for (int w = 0; w < VF_OFF_THREADS / 64; ++w) {
    const long long v = part[w];
    base += w < wave ? v : 0;
    total += v;
  }
  for (long long i = i0; i < i1; ++i) {
    const long long v = kept[i];
    kept[i] = base;
    base += v;
  }
  __syncthreads();  // (the prefixes of all pairs are in place)
  auto first_of = [&](int p) { return p < npairs ? kept[p] : total; };
  int cutp = npairs;
  for (int p = tid; p < npairs; p += VF_OFF_THREADS) {
    const long long o = first_of(p), c = first_of(p + 1) - o;
    if (c > 0 && o + c > out_cap) cutp = min(cutp, p);
  }
  for (int off = 32; off > 0; off >>= 1) cutp = min(cutp, __shfl_xor(cutp, off, 64));
  if (lane == 0) red[wave] = cutp;
  __syncthreads();
  for (int w = 0; w < VF_OFF_THREADS / 64; ++w) cutp = min(cutp, red[w]);
  const long long stop = first_of(cutp);
  for (int p = tid; p < npairs; p += VF_OFF_THREADS) {
    const long long o = first_of(p), c = first_of(p + 1) - o;
    const int fl = models[p].flags | (p >= cutp ? BRISK_PAIR_MATCHES_CUT : 0);
    models[p].flags = fl;
    counts[p] = (int)c;  // (a pair has fewer than 2^31 records)
    flags[p] = fl;
    offsets[p] = p >= cutp ? stop : o;
  }
  if (tid == 0) offsets[npairs] = stop;
}

__global__ void __launch_bounds__(VF_THREADS) k_verify_scatter(const long long* __restrict__ offsets, const BriskDMatch* __restrict__ matches,
                                                               long long in_cap, const unsigned char* __restrict__ keep,
                                                               const int* __restrict__ counts, const int* __restrict__ flags,
                                                               const long long* __restrict__ out_offsets, long long out_cap,
                                                               BriskDMatch* __restrict__ out) {
  __shared__ int part[2][VF_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (counts[p] == 0 || (flags[p] & (BRISK_PAIR_MATCHES_CUT | BRISK_PAIR_BAD))) return;  // (a bad pair has no keep bytes)
  long long begin;
  int m;
  if (!vf_range(offsets, p, in_cap, begin, m)) return;
  const uint4* src = reinterpret_cast<const uint4*>(matches);
  uint4* dst = reinterpret_cast<uint4*>(out);
  long long pos = out_offsets[p];
  for (int c0 = 0, it = 0; c0 < m; c0 += VF_THREADS, ++it) {
    const int i = c0 + tid;
    const bool k = i < m && keep[begin + i] != 0;
    const unsigned long long b = __ballot(k);
    if (lane == 0) part[it & 1][wave] = __popcll(b);
    __syncthreads();  // (one barrier a chunk: the totals alternate between two rows)
    int before = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (int w = 0; w < VF_WAVES; ++w) {
      const int v = part[it & 1][w];
      before += w < wave ? v : 0;
      all += v;
    }
    if (k && pos + before < out_cap) dst[pos + before] = src[begin + i];  // (always inside while the arrays did not change between the passes)
    pos += all;
  }
}

// ---- the epipolar verifier (brisk_pair_epipolar.h) ----
// the model of hypothesis h of a pair with m >= 8 records; false = invalid
__device__ __forceinline__ bool vf_epipolar_hypothesis(const BriskDMatch* __restrict__ matches, const VfPair& pr, uint32_t pair_seed, int h,
                                                       BriskFundamental& F) {
  int idx[8];
  brisk_epipolar_sample(pair_seed, h, pr.m, idx);
  BriskVerifyPoints pt[8];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    // (every index is below m by construction; a draw that is not - it cannot happen - would make the hypothesis invalid, not a read)
    ok = ok && (unsigned)idx[k] < (unsigned)pr.m && vf_resolve(matches, pr, idx[k], r);
    pt[k] = vf_points(r);
  }
  if (!ok) return false;
  int free_col;
  return brisk_epipolar_model(pt, F, free_col);
}

// k_verify_ransac with the eight-point model in the homography's place: one workgroup per pair, a lane = a hypothesis, the pass
// over 256 hypotheses outside, the chunk inside, the same staging, key reduction and keep sweep; k_verify_offsets and
// k_verify_scatter pack the result (BriskPairEpipolarModel has BriskPairModel's layout).  What is new is the solve: the lane keeps
// its 8 x 9 system in registers - brisk_epipolar_step indexes it with constants only, the row and column swaps of the complete
// pivoting are compare-selects - so nothing goes to scratch.  The registers of one wave per SIMD are there for it: a workgroup is
// four waves, one per SIMD, and the 16 KB chunk leaves room for nine more workgroups on the CU that the registers do not.
// At 256 VGPRs the order of the solve's instructions follows the text AROUND the pass loop: with vf_pair, a winner function
// or vf_keep_sweep in it the loop came out in another order and the call 0.5 - 1 us slower.  So this kernel carries its own
// prologue and sweep (and, like k_verify_ransac, its winner), and shares the record helpers, the record writer and the packing.
__global__ void __launch_bounds__(VF_THREADS) k_epipolar_ransac(BriskDescSet Q, BriskDescSet T, BriskKpSet QK, BriskKpSet TK, BriskPairSpec P,
                                                                int rows_cap, const long long* __restrict__ offsets,
                                                                const BriskDMatch* __restrict__ matches, long long in_cap, BriskPairVerify V,
                                                                unsigned char* __restrict__ keep, long long* __restrict__ kept,
                                                                BriskPairEpipolarModel* __restrict__ models) {
  __shared__ float4 pts[VF_CHUNK];
  __shared__ unsigned long long wkey[VF_WAVES];
  __shared__ double win[9];  // the winner's F
  __shared__ int wsum[2][VF_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the pair: vf_pair and vf_pair_frames, written out
  VfPair pr;
  if (P.pairs) {
    pr.fa = P.pairs[2 * (long)p];
    pr.fb = P.pairs[2 * (long)p + 1];
  } else {
    pr.fa = P.query_first + p * P.query_step;
    pr.fb = P.train_first + p * P.train_step;
  }
  const bool range_ok = vf_range(offsets, p, in_cap, pr.begin, pr.m);
  const bool frames_ok = pr.fa >= 0 && pr.fa < Q.frames && pr.fb >= 0 && pr.fb < T.frames;
  if (!range_ok || !frames_ok) {  // nothing is kept, nothing of the pair is read
    if (tid == 0) {
      kept[p] = 0;
      const double none[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
      vf_write_model(models + p, none, false, pr.m, 0, 0, -1, 0, BRISK_PAIR_BAD | BRISK_PAIR_NO_MODEL);
    }
    return;
  }
  pr.lim_a = brisk_track_lim(Q.counts[(long)pr.fa * Q.count_stride], rows_cap);
  pr.lim_b = brisk_track_lim(T.counts[(long)pr.fb * T.count_stride], rows_cap);
  pr.qk = QK.kps + (long)pr.fa * QK.frame_pitch;
  pr.tk = TK.kps + (long)pr.fb * TK.frame_pitch;
  pr.nchunks = (pr.m + VF_CHUNK - 1) / VF_CHUNK;
  const uint32_t pair_seed = brisk_verify_pair_seed(V.seed, p);
  const bool thr_on = brisk_verify_threshold_on(V.max_error);
  const double thr2 = brisk_verify_thr2(V.max_error);

  if (pr.nchunks == 1) vf_stage(pts, matches, pr, 0);  // stays for every pass and the last sweep
  __syncthreads();

  // ---- the hypotheses: passes of 256 outside, chunks inside; the pass behind the last one is the winner's, on every lane ----
  unsigned long long best = 0ull;
  int nvalid = 0, hwin = -1;
  bool accepted = false;
  BriskFundamental W{0., 0., 0., 0., 0., 0., 0., 0., 0.};
  const int npass = pr.m >= BRISK_EPIPOLAR_MIN_SAMPLE ? (V.hypotheses + VF_THREADS - 1) / VF_THREADS : 0;
  for (int pass = 0; pass <= npass; ++pass) {
    const bool last = pass == npass;
    if (last) {
      // the winner: wave shuffles, one LDS step; the number of valid hypotheses rides along
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
        nvalid += __shfl_xor(nvalid, off, 64);
      }
      if (lane == 0) { wkey[wave] = best; wsum[0][wave] = nvalid; }
      __syncthreads();
      best = 0ull;
      nvalid = 0;
#pragma unroll
      for (int w = 0; w < VF_WAVES; ++w) {
        const unsigned long long o = wkey[w];
        best = o > best ? o : best;
        nvalid += wsum[0][w];
      }
      accepted = brisk_verify_accepted(best, V.min_inliers);
      hwin = brisk_verify_key_hypothesis(best);
      if (hwin < 0) break;
    }
    // (the winner's model is the same arithmetic again, by lane 0 alone: one instance of the solve in the kernel's code)
    const int h = last ? hwin : pass * VF_THREADS + tid;
    BriskFundamental F{0., 0., 0., 0., 0., 0., 0., 0., 0.};
    bool valid = false;
    if (last ? tid == 0 : h < V.hypotheses) valid = vf_epipolar_hypothesis(matches, pr, pair_seed, h, F);
    if (!valid) F = BriskFundamental{0., 0., 0., 0., 0., 0., 0., 0., 0.};
    if (last) {
      if (tid == 0) {
        win[0] = F.f0; win[1] = F.f1; win[2] = F.f2; win[3] = F.f3; win[4] = F.f4; win[5] = F.f5; win[6] = F.f6; win[7] = F.f7; win[8] = F.f8;
      }
      break;
    }
    const bool score = valid && thr_on;
    int count = 0;
    for (int c = 0; c < pr.nchunks; ++c) {
      if (pr.nchunks > 1) {
        __syncthreads();  // (the chunk before is read)
        vf_stage(pts, matches, pr, c);
        __syncthreads();
      }
      const int n = min(VF_CHUNK, pr.m - c * VF_CHUNK);
      if (score)
        for (int i = 0; i < n; ++i) {
          const float4 r = pts[i];  // one address for the whole wave: a broadcast
          count += brisk_epipolar_inlier(F, thr2, (double)r.x, (double)r.y, (double)r.z, (double)r.w) ? 1 : 0;
        }
    }
    const unsigned long long key = brisk_verify_key(valid, count, h);
    best = key > best ? key : best;
    nvalid += valid ? 1 : 0;
  }
  __syncthreads();  // (win is written; wsum is written again below)
  if (hwin >= 0) W = BriskFundamental{win[0], win[1], win[2], win[3], win[4], win[5], win[6], win[7], win[8]};

  // ---- the last sweep: lane = record ----
  int nkept = 0, nusable = 0;
  for (int c = 0; c < pr.nchunks; ++c) {
    if (pr.nchunks > 1) {
      __syncthreads();
      vf_stage(pts, matches, pr, c);
      __syncthreads();
    }
    const int n = min(VF_CHUNK, pr.m - c * VF_CHUNK);
    for (int i = tid; i < n; i += VF_THREADS) {
      const float4 r = pts[i];
      const bool usable = r.x == r.x;
      const bool inl = accepted && usable && brisk_epipolar_inlier(W, thr2, (double)r.x, (double)r.y, (double)r.z, (double)r.w);
      const bool k = brisk_verify_keeps(accepted, usable, inl, V.keep_unverified);
      keep[pr.begin + (long long)c * VF_CHUNK + i] = k ? 1 : 0;
      nkept += k ? 1 : 0;
      nusable += usable ? 1 : 0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    nkept += __shfl_xor(nkept, off, 64);
    nusable += __shfl_xor(nusable, off, 64);
  }
  if (lane == 0) { wsum[0][wave] = nkept; wsum[1][wave] = nusable; }
  __syncthreads();
  if (tid == 0) {
    nkept = nusable = 0;
#pragma unroll
    for (int w = 0; w < VF_WAVES; ++w) { nkept += wsum[0][w]; nusable += wsum[1][w]; }
    kept[p] = nkept;
    const double f[9] = {W.f0, W.f1, W.f2, W.f3, W.f4, W.f5, W.f6, W.f7, W.f8};  // (zeros without a valid hypothesis)
    vf_write_model(models + p, f, true, pr.m, nusable, brisk_verify_key_count(best), hwin, nvalid, accepted ? 0 : BRISK_PAIR_NO_MODEL);
  }
}

// ---- the epipolar refit (brisk_pair_epipolar_refit.h) ----
// one sweep of the normal matrix's sums: the terms K0 .. K0 + CNT - 1 of the pair's inliers under F, lane = record, combined in the
// rule's order; lane 0 leaves them in W.s.  A lane carries CNT running sums, not 44: k_refit_models' 22 already take 252 VGPRs.  The
// order inside each sum is the rule's, so the number of sweeps changes no bit
template <int K0, int CNT>
__device__ __forceinline__ void vf_epirefit_sweep(float4* __restrict__ pts, const BriskDMatch* __restrict__ matches, const VfPair& pr,
                                                  const BriskFundamental& F, double thr2, const BriskRefitNorm& N,
                                                  double (*red)[BRISK_EPIREFIT_SWEEP], BriskEpirefitWork& W, int lane, int wave) {
  double s[CNT];
#pragma unroll
  for (int i = 0; i < CNT; ++i) s[i] = 0.0;
  vf_each(pts, matches, pr, [&](const float4& r, int) {
    const double x = (double)r.x, y = (double)r.y, xt = (double)r.z, yt = (double)r.w;
    const bool in = brisk_epipolar_inlier(F, thr2, x, y, xt, yt);
    double a[9], t[CNT];
    brisk_epirefit_row(N, x, y, xt, yt, a);
    brisk_epirefit_terms<K0, CNT>(a, t);
#pragma unroll
    for (int i = 0; i < CNT; ++i) s[i] = s[i] + (in ? t[i] : 0.0);
  });
  vf_block_sums(s, red, lane, wave);
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < CNT; ++i) W.s[K0 + i] = s[i];
}

// k_refit_models with the fundamental matrix in the homography's place: one workgroup per pair, the same staging, lane = record for
// the score and for the sums' partials, every lane carries the same model and count, so the round loop is uniform.  The 44 sums of
// the 9 x 9 normal matrix are taken in three sweeps over the chunk that stays in LDS; lane 0 solves the 9 x 9 and the 3 x 3 system
// in LDS (BriskEpirefitWork: every dynamic index goes there).  in_models may be models: every lane has read its pair's record
// before the first barrier, lane 0 writes behind the last
__global__ void __launch_bounds__(VF_THREADS) k_refit_epipolar(BriskDescSet Q, BriskDescSet T, BriskKpSet QK, BriskKpSet TK, BriskPairSpec P,
                                                               int rows_cap, const long long* __restrict__ offsets,
                                                               const BriskDMatch* __restrict__ matches, long long in_cap,
                                                               const BriskPairEpipolarModel* in_models, BriskPairEpipolarRefit R,
                                                               unsigned char* __restrict__ keep, long long* __restrict__ kept,
                                                               BriskPairEpipolarModel* models) {
  __shared__ float4 pts[VF_CHUNK];
  __shared__ double red[VF_WAVES][BRISK_EPIREFIT_SWEEP];
  __shared__ int ired[VF_WAVES][2];
  __shared__ BriskEpirefitWork work;
  __shared__ double fit[10];  // the fitted model; [9] != 0: the fit failed
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  VfPair pr;
  if (!vf_pair(Q, T, P, offsets, in_cap, kept, models, pr)) return;
  vf_pair_frames(Q, T, QK, TK, rows_cap, pr);
  const double thr2 = brisk_verify_thr2(R.max_error);

  // the input record: one address for the whole workgroup
  double fin[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) fin[i] = in_models[p].f[i];
  const int in_hypothesis = in_models[p].hypothesis;
  const bool has_model = brisk_refit_has_model(fin, in_hypothesis, in_models[p].flags, R.max_error);

  if (pr.nchunks == 1) vf_stage(pts, matches, pr, 0);  // stays for every pass
  __syncthreads();

  BriskFundamental F{fin[0], fin[1], fin[2], fin[3], fin[4], fin[5], fin[6], fin[7], fin[8]};
  int n = 0, replaced = 0;
  if (has_model) {
    int c[2] = {0, 0};
    vf_each(pts, matches, pr, [&](const float4& r, int) {
      c[0] += brisk_epipolar_inlier(F, thr2, (double)r.x, (double)r.y, (double)r.z, (double)r.w) ? 1 : 0;
    });
    vf_block_sums(c, ired, lane, wave);
    n = c[0];
    for (int round = 1; round <= R.rounds && n >= BRISK_EPIPOLAR_MIN_SAMPLE; ++round) {
      BriskRefitNorm N;
      double s4[4] = {0.0, 0.0, 0.0, 0.0};
      vf_each(pts, matches, pr, [&](const float4& r, int) {
        const double x = (double)r.x, y = (double)r.y, xt = (double)r.z, yt = (double)r.w;
        const bool in = brisk_epipolar_inlier(F, thr2, x, y, xt, yt);
        s4[0] = s4[0] + (in ? x : 0.0);
        s4[1] = s4[1] + (in ? y : 0.0);
        s4[2] = s4[2] + (in ? xt : 0.0);
        s4[3] = s4[3] + (in ? yt : 0.0);
      });
      vf_block_sums(s4, red, lane, wave);
      brisk_refit_centroids(s4, n, N);
#pragma unroll
      for (int i = 0; i < 4; ++i) s4[i] = 0.0;
      vf_each(pts, matches, pr, [&](const float4& r, int) {
        const double x = (double)r.x, y = (double)r.y, xt = (double)r.z, yt = (double)r.w;
        const bool in = brisk_epipolar_inlier(F, thr2, x, y, xt, yt);
        double t[4];
        brisk_refit_spread_terms(N, x, y, xt, yt, t);
#pragma unroll
        for (int i = 0; i < 4; ++i) s4[i] = s4[i] + (in ? t[i] : 0.0);
      });
      vf_block_sums(s4, red, lane, wave);
      if (!brisk_refit_scales(s4, n, N)) break;
      vf_epirefit_sweep<0, BRISK_EPIREFIT_SWEEP>(pts, matches, pr, F, thr2, N, red, work, lane, wave);
      vf_epirefit_sweep<BRISK_EPIREFIT_SWEEP, BRISK_EPIREFIT_SWEEP>(pts, matches, pr, F, thr2, N, red, work, lane, wave);
      vf_epirefit_sweep<2 * BRISK_EPIREFIT_SWEEP, BRISK_EPIREFIT_SUMS - 2 * BRISK_EPIREFIT_SWEEP>(pts, matches, pr, F, thr2, N, red, work, lane,
                                                                                                 wave);
      if (tid == 0) {  // the solve: one lane, in LDS (it wrote work.s itself)
        BriskFundamental G;
        int free_index;
        const bool ok = brisk_epirefit_fit(n, N, R.rank2, work, G, free_index);
        fit[0] = G.f0; fit[1] = G.f1; fit[2] = G.f2; fit[3] = G.f3; fit[4] = G.f4; fit[5] = G.f5; fit[6] = G.f6; fit[7] = G.f7; fit[8] = G.f8;
        fit[9] = ok ? 0.0 : 1.0;
      }
      __syncthreads();
      const BriskFundamental G{fit[0], fit[1], fit[2], fit[3], fit[4], fit[5], fit[6], fit[7], fit[8]};
      const bool failed = fit[9] != 0.0;
      __syncthreads();  // (fit is written again in the next round)
      if (failed) break;
      // the fitted model's score; d[1]: the records whose membership differs from the present set's
      int d[2] = {0, 0};
      vf_each(pts, matches, pr, [&](const float4& r, int) {
        const double x = (double)r.x, y = (double)r.y, xt = (double)r.z, yt = (double)r.w;
        const bool in = brisk_epipolar_inlier(F, thr2, x, y, xt, yt);
        const bool in1 = brisk_epipolar_inlier(G, thr2, x, y, xt, yt);
        d[0] += in1 ? 1 : 0;
        d[1] += in1 != in ? 1 : 0;
      });
      vf_block_sums(d, ired, lane, wave);
      if (!brisk_refit_replaces(d[0], n)) break;
      F = G;
      n = d[0];
      ++replaced;
      if (d[1] == 0) {  // a fixed point: every round left fits the same set again
        replaced = R.rounds;
        break;
      }
    }
  }
  const bool accepted = brisk_refit_accepted(has_model, n, R.min_inliers);

  int e[2];  // kept, usable
  vf_keep_sweep(pts, matches, pr, keep, ired, lane, wave, accepted, R.keep_unverified, e, [&](const float4& r) {
    return brisk_epipolar_inlier(F, thr2, (double)r.x, (double)r.y, (double)r.z, (double)r.w);
  });
  if (tid == 0) {
    kept[p] = e[0];
    const double fout[9] = {F.f0, F.f1, F.f2, F.f3, F.f4, F.f5, F.f6, F.f7, F.f8};
    double f[9];  // the input's nine doubles, byte for byte, when no round replaced them
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = replaced > 0 ? fout[i] : fin[i];
    vf_write_model(models + p, f, has_model, pr.m, e[1], n, has_model ? in_hypothesis : -1, replaced,
                   (replaced > 0 ? BRISK_PAIR_REFIT : 0) | (accepted ? 0 : BRISK_PAIR_NO_MODEL));
  }
}

// what the three calls end in: the kept counts -> counts, flags (the model records' too) and offsets, then the kept records packed
static void vf_launch_pack(int np, const long long* offsets, const BriskDMatch* matches, long long in_cap, const unsigned char* keep,
                           long long* kept, long long out_cap, BriskPairModel* models, int* counts, int* flags, long long* out_offsets,
                           BriskDMatch* out, hipStream_t s) {
  hipLaunchKernelGGL(k_verify_offsets, dim3(1), dim3(VF_OFF_THREADS), 0, s, kept, np, out_cap, models, counts, flags, out_offsets);
  hipLaunchKernelGGL(k_verify_scatter, dim3(np), dim3(VF_THREADS), 0, s, offsets, matches, in_cap, keep, counts, flags, out_offsets, out_cap,
                     out);
}

void brisk_launch_pair_verify(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK, const BriskPairSpec& P,
                              int rows_cap, const long long* offsets, const BriskDMatch* matches, long long in_cap, const BriskPairVerify& V,
                              unsigned char* keep, long long* kept, long long out_cap, BriskPairModel* models, int* counts, int* flags,
                              long long* out_offsets, BriskDMatch* out, hipStream_t s) {
  hipLaunchKernelGGL(k_verify_ransac, dim3(P.npairs), dim3(VF_THREADS), 0, s, Q, T, QK, TK, P, rows_cap, offsets, matches, in_cap, V, keep,
                     kept, models);
  vf_launch_pack(P.npairs, offsets, matches, in_cap, keep, kept, out_cap, models, counts, flags, out_offsets, out, s);
}

void brisk_launch_pair_refit(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK, const BriskPairSpec& P,
                             int rows_cap, const long long* offsets, const BriskDMatch* matches, long long in_cap,
                             const BriskPairModel* in_models, const BriskPairRefit& R, unsigned char* keep, long long* kept, long long out_cap,
                             BriskPairModel* models, int* counts, int* flags, long long* out_offsets, BriskDMatch* out, hipStream_t s) {
  hipLaunchKernelGGL(k_refit_models, dim3(P.npairs), dim3(VF_THREADS), 0, s, Q, T, QK, TK, P, rows_cap, offsets, matches, in_cap, in_models, R,
                     keep, kept, models);
  vf_launch_pack(P.npairs, offsets, matches, in_cap, keep, kept, out_cap, models, counts, flags, out_offsets, out, s);
}

void brisk_launch_pair_epipolar_refit(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                      const BriskPairSpec& P, int rows_cap, const long long* offsets, const BriskDMatch* matches, long long in_cap,
                                      const BriskPairEpipolarModel* in_models, const BriskPairEpipolarRefit& R, unsigned char* keep,
                                      long long* kept, long long out_cap, BriskPairEpipolarModel* models, int* counts, int* flags,
                                      long long* out_offsets, BriskDMatch* out, hipStream_t s) {
  hipLaunchKernelGGL(k_refit_epipolar, dim3(P.npairs), dim3(VF_THREADS), 0, s, Q, T, QK, TK, P, rows_cap, offsets, matches, in_cap, in_models,
                     R, keep, kept, models);
  vf_launch_pack(P.npairs, offsets, matches, in_cap, keep, kept, out_cap, reinterpret_cast<BriskPairModel*>(models), counts, flags, out_offsets,
                 out, s);
}

void brisk_launch_pair_epipolar(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK, const BriskPairSpec& P,
                                int rows_cap, const long long* offsets, const BriskDMatch* matches, long long in_cap, const BriskPairVerify& V,
                                unsigned char* keep, long long* kept, long long out_cap, BriskPairEpipolarModel* models, int* counts, int* flags,
                                long long* out_offsets, BriskDMatch* out, hipStream_t s) {
  static_assert(sizeof(BriskPairEpipolarModel) == sizeof(BriskPairModel) && offsetof(BriskPairEpipolarModel, flags) == offsetof(BriskPairModel, flags),
                "k_verify_offsets reads and writes the flags of either record");
  hipLaunchKernelGGL(k_epipolar_ransac, dim3(P.npairs), dim3(VF_THREADS), 0, s, Q, T, QK, TK, P, rows_cap, offsets, matches, in_cap, V, keep,
                     kept, models);
  vf_launch_pack(P.npairs, offsets, matches, in_cap, keep, kept, out_cap, reinterpret_cast<BriskPairModel*>(models), counts, flags, out_offsets,
                 out, s);
}
