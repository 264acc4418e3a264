// brisk_match.hip - Hamming brute-force matcher kernels (the step after the detect + describe path).
//
// Replaces brisk::BruteForceMatcher::commonKnnMatchImpl / commonRadiusMatchImpl
// (brisk/src/brute-force-matcher.cc:80-213) with brisk::Hamming (brisk/include/brisk/internal/hamming.h:98-112)
// as the distance: popcount of a ^ b over size / 16 128-bit words.  Integer work, HBM/L2-bound, no MFMA.
//
// Matrix path (any descriptor size up to 224 bytes, several train images, masks):
//   k_match_dist        u16 distance matrix of a block of queries against all train descriptors (all train images
//                       concatenated in image order); 0xFFFF = the reference's INT_MAX (masked pair)
//   k_match_masked_out  the queries that every image's mask forbids
//   k_match_knn         one wave per query: k rounds of "first minimum" selection, as the reference does
//   k_match_radius      one wave per query: distance histogram in LDS, then stable placement by (distance, image,
//                       train index)
//
// Register-row path (descriptors of 16, 32, 48 or 64 bytes, one train set, no masks, no distance matrix): 64 queries per
// workgroup, one per lane with its descriptor in registers; each wave walks a slice of the train rows through wave-uniform
// (scalar) loads and XORs them against the lane's registers.  A candidate is one packed key, distance << 22 | train row.
// The shared pieces, each written once: mp_resolve (a workgroup's pair, counts, frame pointers, alignment), mp_load_row and
// m_dist (a row into registers, a register row against a memory row), the scans mp_scan / mrp_scan and their gated forms
// mpg_scan / mrpg_scan (chosen once per slice by mp_scan_slice / mrp_body), m_top2 and m_merge (the two smallest keys, and
// the per-wave lists of a workgroup merged through LDS), m_dispatch_words and mp_launch_pairs on the host.
//   k_match_knn_fused           k <= 2, one query set against one train set, 16 waves per workgroup
//   k_match_knn_pairs[_gated]   k <= 2 for the frame pairs of a batch in one launch (mp_body), with the cross check fused;
//                               gated: only rows whose keypoints pass brisk_match_gate.h's predicate, no top-up entry
//   k_guided_knn_pairs          the gated k-NN kernel (no cross check) with the window centred where the pair's model puts the
//                               lane's query keypoint (brisk_match_guide.h): a per-lane fp64 prologue in front of the same scan
//   k_guided_radius_pairs       the gated radius kernel, guided the same way
//   k_epiline_knn_pairs, k_epiline_radius_pairs
//                               the gated kernels (no cross check) behind the band around the lane's epipolar line under the
//                               pair's model (brisk_match_epiline.h): the line is made per lane in front of the same scan, the
//                               band is three fp64 multiplies per passing row beside the gate's compares
//   k_mutual_centre_knn, k_mutual_line_knn
//                               the two guided k-NN kernels for k = 1 WITH the cross check: the backward scan asks the guide's mask from
//                               the train side, the centres / lines of the query rows passing by made 64 at a time, one per lane, and
//                               handed round by v_readlane (mpm_scan)
//   k_match_radius_pairs[_gated], k_match_radius_pairs_one
//                               radius matching in the same shape (mrp_body): hits collected in a short LDS list per
//                               query and ranked; a query with more hits than the list holds is redone by one wave
//                               with k_match_radius' histogram and placement (mrp_dense)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "brisk_kernels.h"

#define MT_THREADS 256
#define MT_QTILE 32
#define MT_MAXWORDS_LONG 28  // descriptors up to 224 bytes (generateKernel at small pattern scales); BRISK's own are 48 and 64 (8 x u64)

// grid: (ceil(nt / 256), ceil(nqb / MT_QTILE)); thread = one train descriptor, loop over the query tile in LDS
template <int MT_MAXWORDS>
__global__ void __launch_bounds__(MT_THREADS) k_match_dist(const uint8_t* __restrict__ query, int q_pitch, int q0, int nqb,
                                                           const uint8_t* __restrict__ train, int t_pitch, int nt,
                                                           int words /* u64 per descriptor */,
                                                           const uint8_t* __restrict__ mask, long mask_pitch,
                                                           uint16_t* __restrict__ dist, long dist_pitch) {
  __shared__ unsigned long long qs[MT_QTILE][MT_MAXWORDS];
  const int t = blockIdx.x * MT_THREADS + threadIdx.x;
  const int qt0 = blockIdx.y * MT_QTILE;
  for (int i = threadIdx.x; i < MT_QTILE * words; i += MT_THREADS) {
    const int q = i / words, w = i % words;
    unsigned long long v = 0;
    if (qt0 + q < nqb) {
      const uint8_t* p = query + (long)(q0 + qt0 + q) * q_pitch + w * 8;
      for (int b = 0; b < 8; ++b) v |= (unsigned long long)p[b] << (8 * b);  // (no alignment assumption on the rows)
    }
    qs[q][w] = v;
  }
  __syncthreads();
  if (t >= nt) return;
  unsigned long long tv[MT_MAXWORDS];
#pragma unroll
  for (int w = 0; w < MT_MAXWORDS; ++w) {
    tv[w] = 0;
    if (w < words) {
      const uint8_t* p = train + (long)t * t_pitch + w * 8;
      unsigned long long v = 0;
      for (int b = 0; b < 8; ++b) v |= (unsigned long long)p[b] << (8 * b);
      tv[w] = v;
    }
  }
  const int nq = min(MT_QTILE, nqb - qt0);
  for (int q = 0; q < nq; ++q) {
    int d = 0;
#pragma unroll
    for (int w = 0; w < MT_MAXWORDS; ++w)
      if (w < words) d += __popcll(tv[w] ^ qs[q][w]);
    if (mask && mask[(long)(q0 + qt0 + q) * mask_pitch + t] == 0) d = 0xFFFF;
    dist[(long)(qt0 + q) * dist_pitch + t] = (uint16_t)d;
  }
}

// masked-out queries (OpenCV DescriptorMatcher::isMaskedOut: `outCount == masks.size()`): EVERY image has a non-empty
// mask whose row for this query is all zero - the query can match nothing anywhere.
// grid: nqb blocks of 64 threads; img_start[nimg + 1] are the offsets of the images in the concatenated train set,
// has_mask[i] != 0 if image i has a mask.
__global__ void __launch_bounds__(64) k_match_masked_out(const uint8_t* __restrict__ mask, long mask_pitch, int q0,
                                                         const int* __restrict__ img_start, const int* __restrict__ has_mask,
                                                         int nimg, int* __restrict__ masked) {
  const int q = blockIdx.x, lane = threadIdx.x;
  int out = nimg > 0 ? 1 : 0;
  for (int i = 0; i < nimg && out; ++i) {
    if (!has_mask[i]) { out = 0; break; }  // no mask, or no train descriptors (an empty cv::Mat): not counted
    bool any = false;
    for (int t = img_start[i] + lane; t < img_start[i + 1]; t += 64) any |= mask[(long)(q0 + q) * mask_pitch + t] != 0;
    if (__any(any)) out = 0;
  }
  if (lane == 0) masked[q] = out;
}

// (img_start == nullptr: a single train image [0, nt))
__device__ __forceinline__ int mt_image_of(const int* img_start, int nimg, int t) {
  if (!img_start) return 0;
  int i = 0;
  while (i + 1 < nimg && t >= img_start[i + 1]) ++i;
  return i;
}

// one wave per query; out row = (q0 + q) * k
__global__ void __launch_bounds__(64) k_match_knn(const uint16_t* __restrict__ dist, long dist_pitch, int q0, int nt,
                                                  const int* __restrict__ img_start, int nimg, const int* __restrict__ masked,
                                                  int k, BriskDMatch* __restrict__ out, int* __restrict__ out_count) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const uint16_t* row = dist + (long)q * dist_pitch;
  BriskDMatch* orow = out + (long)(q0 + q) * k;
  if (masked && masked[q]) {
    if (lane == 0) out_count[q0 + q] = 0;
    return;
  }
  int last_nonempty = -1;
  if (!img_start) last_nonempty = nt > 0 ? 0 : -1;
  else
    for (int i = 0; i < nimg; ++i)
      if (img_start[i + 1] > img_start[i]) last_nonempty = i;
  int count = 0;
  unsigned long long last = 0;
  bool have_last = false;
  for (int kk = 0; kk < k; ++kk) {
    // first minimum over (distance, concatenated index) = the reference's minMaxLoc per image + strict '<' across
    // images.  The reference overwrites a selected entry with INT_MAX; selections come in strictly increasing
    // (distance, index) order, so "the smallest key above the previous selection" is the same thing without a write.
    unsigned long long best = ~0ull;
    for (int t = lane; t < nt; t += 64) {
      const unsigned long long key = ((unsigned long long)row[t] << 32) | (unsigned)t;
      if ((!have_last || key > last) && key < best) best = key;
    }
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o < best ? o : best;
    }
    const unsigned d = (unsigned)(best >> 32);
    if (nt == 0 || d >= 0xFFFFu) break;  // nothing real left
    const int t = (int)(best & 0xFFFFFFFFu);
    if (lane == 0) {
      const int img = mt_image_of(img_start, nimg, t);
      BriskDMatch m;
      m.queryIdx = q0 + q; m.trainIdx = t - (img_start ? img_start[img] : 0); m.imgIdx = img; m.distance = (float)d;
      orow[count] = m;
    }
    last = best;
    have_last = true;
    ++count;
  }
  // reference quirk (brute-force-matcher.cc:139-153): with every entry at INT_MAX the comparison
  // `minVal < bestMatch.distance` still succeeds (2147483647.0 < FLT_MAX, and again against float(INT_MAX) =
  // 2147483648), so the remaining k - count slots are filled with {train 0 of the LAST non-empty image, 2147483648.f}
  if (last_nonempty >= 0 && lane == 0) {
    for (int c = count; c < k; ++c) {
      BriskDMatch m;
      m.queryIdx = q0 + q; m.trainIdx = 0; m.imgIdx = last_nonempty; m.distance = 2147483648.0f;
      orow[c] = m;
    }
  }
  if (last_nonempty >= 0) count = k;
  if (lane == 0) out_count[q0 + q] = count;
}

// one wave per query.  out row = (q0 + q) * cap, at most cap matches are stored, out_count = matches found.
#define MR_BINS 1793  // distances 0 ... 8 x 224 bytes (BRISK's own descriptors: 0 ... 512; the prefix below only walks the first 513 bins then)
__global__ void __launch_bounds__(64) k_match_radius(const uint16_t* __restrict__ dist, long dist_pitch, int q0, int nt,
                                                     const int* __restrict__ img_start, int nimg,
                                                     const int* __restrict__ masked, float max_distance, int cap,
                                                     BriskDMatch* __restrict__ out, int* __restrict__ out_count, int nbins) {
  __shared__ int bins[MR_BINS + 1];
  const int q = blockIdx.x, lane = threadIdx.x;
  const uint16_t* row = dist + (long)q * dist_pitch;
  BriskDMatch* orow = out + (long)(q0 + q) * cap;
  if (masked && masked[q]) {
    if (lane == 0) out_count[q0 + q] = 0;
    return;
  }
  for (int b = lane; b <= nbins; b += 64) bins[b] = 0;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  for (int t = lane; t < nt; t += 64) {
    const unsigned d = row[t];
    if (d != 0xFFFFu && (float)d < max_distance) atomicAdd(&bins[d], 1);
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) {  // exclusive prefix over the nbins (513 for a 64-byte descriptor) distance values
    int acc = 0;
    for (int b = 0; b < nbins; ++b) { const int c = bins[b]; bins[b] = acc; acc += c; }
    bins[nbins] = acc;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const int total = bins[nbins];
  // stable placement: chunks of 64 train entries in order; inside a chunk equal distances keep lane order
  for (int t0 = 0; t0 < nt; t0 += 64) {
    const int t = t0 + lane;
    unsigned d = 0xFFFFu;
    if (t < nt) d = row[t];
    const bool hit = d != 0xFFFFu && (float)d < max_distance;
    unsigned long long todo = __ballot(hit);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned dsel = __shfl(d, leader, 64);
      const unsigned long long same = __ballot(hit && d == dsel);
      const int base = bins[dsel];
      if (hit && d == dsel) {
        const int pos = base + __popcll(same & ((1ull << lane) - 1ull));
        if (pos < cap) {
          const int img = mt_image_of(img_start, nimg, t);
          BriskDMatch m;
          m.queryIdx = q0 + q; m.trainIdx = t - (img_start ? img_start[img] : 0); m.imgIdx = img; m.distance = (float)d;
          orow[pos] = m;
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (lane == leader) bins[dsel] = base + __popcll(same);
      __builtin_amdgcn_s_waitcnt(0);
      __builtin_amdgcn_wave_barrier();
      todo &= ~same;
    }
  }
  if (lane == 0) out_count[q0 + q] = total;
}

// ------------------------------------------------------------------------------------------------
// The register-row path: what its kernels share.
// ------------------------------------------------------------------------------------------------
#define MF_WAVES 16
#define MF_IDX_BITS 22
#define MF_IDX_MASK ((1u << MF_IDX_BITS) - 1)
#define MF_NO_KEY 0xFFFFFFFFu
#ifndef MP_WAVES
// waves of a pair workgroup = slices of the train rows.  8, not k_match_knn_fused's 16: a CU holds ONE workgroup of 16 waves (71 VGPRs
// with the 32-key merge unrolled: 7 waves per SIMD) but four of 8 (39 VGPRs), and with several resident the prologue (pair and
// count look-ups, the query row) and the LDS merge of one are covered by the scans of the others (measured both)
#define MP_WAVES 8
#endif

// rows of 4-byte aligned base and pitches are read as words, others byte by byte (no alignment assumption on a caller's rows)
__device__ __forceinline__ bool m_aligned(const void* base, long frame_pitch, int row_pitch) {
  return (((uintptr_t)base | (unsigned long)frame_pitch | (unsigned)row_pitch) & 3) == 0;
}
template <int W32>
__device__ __forceinline__ void mp_load_row(const uint8_t* p, bool aligned, unsigned (&v)[W32]) {
  if (aligned) {
    const unsigned* p32 = reinterpret_cast<const unsigned*>(p);
#pragma unroll
    for (int w = 0; w < W32; ++w) v[w] = p32[w];
  } else {
#pragma unroll
    for (int w = 0; w < W32; ++w)
      v[w] = (unsigned)p[4 * w] | ((unsigned)p[4 * w + 1] << 8) | ((unsigned)p[4 * w + 2] << 16) | ((unsigned)p[4 * w + 3] << 24);
  }
}
// Hamming distance of a register row to the row at tp (wave-uniform in the scans: scalar loads, v_xor + v_bcnt with accumulate)
template <int W32, bool ALIGNED>
__device__ __forceinline__ unsigned m_dist(const unsigned (&qv)[W32], const uint8_t* tp) {
  unsigned d = 0;
  if (ALIGNED) {
    const unsigned* tp32 = reinterpret_cast<const unsigned*>(tp);
#pragma unroll
    for (int w = 0; w < W32; ++w) d += __popc(qv[w] ^ tp32[w]);
  } else {
#pragma unroll
    for (int w = 0; w < W32; ++w) {
      const unsigned tv = (unsigned)tp[4 * w] | ((unsigned)tp[4 * w + 1] << 8) | ((unsigned)tp[4 * w + 2] << 16) | ((unsigned)tp[4 * w + 3] << 24);
      d += __popc(qv[w] ^ tv);
    }
  }
  return d;
}
__device__ __forceinline__ unsigned m_key(unsigned d, int t) { return (d << MF_IDX_BITS) | (unsigned)t; }
__device__ __forceinline__ void m_key_to(unsigned key, BriskDMatch& m) {
  m.trainIdx = (int)(key & MF_IDX_MASK);
  m.distance = (float)(key >> MF_IDX_BITS);
}
// (b1, b2): the two smallest keys seen
__device__ __forceinline__ void m_top2(unsigned& b1, unsigned& b2, unsigned key) {
  b2 = min(b2, max(b1, key));
  b1 = min(b1, key);
}
// the lane's two smallest keys over the partial lists of the WAVES waves
template <int WAVES>
__device__ __forceinline__ void m_merge(const unsigned (&part)[WAVES][2][64], int lane, unsigned& m1, unsigned& m2) {
#pragma unroll
  for (int w = 0; w < WAVES; ++w)
#pragma unroll
    for (int i = 0; i < 2; ++i) m_top2(m1, m2, part[w][i][lane]);
}
// rows [t0, t1) of one frame (wave-uniform addresses) against the lane's descriptor: the two smallest keys
template <int W32, bool ALIGNED>
__device__ __forceinline__ void mp_scan(const unsigned (&qv)[W32], const uint8_t* rows, int pitch, int t0, int t1, unsigned& b1,
                                        unsigned& b2) {
  for (int t = t0; t < t1; ++t) m_top2(b1, b2, m_key(m_dist<W32, ALIGNED>(qv, rows + (long)t * pitch), t));
}

// ------------------------------------------------------------------------------------------------
// k-NN for k <= 2, one query set against one train set (the frame-to-frame / frame-to-map case): MF_WAVES waves, wave w scans
// the w-th slice of the train set; the MF_WAVES partial top-2 lists of a query are merged through LDS.
// ------------------------------------------------------------------------------------------------
template <int W32>
__global__ void __launch_bounds__(MF_WAVES * 64) k_match_knn_fused(const uint8_t* __restrict__ query, int q_pitch, int nq,
                                                                    const uint8_t* __restrict__ train, int t_pitch, int nt,
                                                                    int k, BriskDMatch* __restrict__ out,
                                                                    int* __restrict__ out_count) {
  __shared__ unsigned part[MF_WAVES][2][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * 64 + lane;
  unsigned qv[W32];
  mp_load_row<W32>(query + (long)min(q, nq - 1) * q_pitch, false, qv);
  const int per = (nt + MF_WAVES - 1) / MF_WAVES;
  const int t0 = __builtin_amdgcn_readfirstlane(wave * per), t1 = min(nt, t0 + per);
  unsigned b1 = MF_NO_KEY, b2 = MF_NO_KEY;
  if (m_aligned(train, 0, t_pitch)) mp_scan<W32, true>(qv, train, t_pitch, t0, t1, b1, b2);
  else mp_scan<W32, false>(qv, train, t_pitch, t0, t1, b1, b2);
  part[wave][0][lane] = b1;
  part[wave][1][lane] = b2;
  __syncthreads();
  if (wave == 0 && q < nq) {
    unsigned m1 = MF_NO_KEY, m2 = MF_NO_KEY;
    m_merge<MF_WAVES>(part, lane, m1, m2);
    BriskDMatch* orow = out + (long)q * k;
    BriskDMatch m;
    m.queryIdx = q; m.imgIdx = 0;
    m_key_to(m1, m);
    orow[0] = m;
    if (k > 1) {
      m_key_to(m2, m);
      orow[1] = m;
    }
    out_count[q] = k;
  }
}

// ------------------------------------------------------------------------------------------------
// The frame pairs of a batch in one launch: grid (ceil(rows_cap / 64), pairs), MP_WAVES waves.  Everything a pair needs is
// resolved on the device.
// ------------------------------------------------------------------------------------------------
// row 0 of frame f.  (An expression on the kernel's own argument wherever it is used, not a pointer kept in MpPair: with the
// pointer handed on through the struct the compiler no longer takes the row loads of the radius scans for scalar loads.)
__device__ __forceinline__ const uint8_t* mp_frame(const BriskDescSet& S, int f) { return S.desc + (long)f * S.frame_pitch; }
struct MpPair {
  int a, b;      // query frame of Q, train frame of T
  int n_a, n_b;  // their row counts
  int rows;      // min(n_a, rows_cap): the query rows that are matched
  bool q_aligned, t_aligned;
};
// the workgroup finds pair p (arithmetic form or the caller's list), reads the two row counts from the sets' count arrays and
// reports the pair in pair_rows (-1: no such frames, or more rows than the keys hold; back_keys: keys index frame a's rows
// too).  false: nothing to do for this workgroup - a bad pair, or its 64 rows lie beyond `rows`
__device__ __forceinline__ bool mp_resolve(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int p, bool back_keys,
                                           int rows_cap, int* __restrict__ pair_rows, MpPair& R) {
  if (P.pairs) {
    R.a = P.pairs[2 * (long)p];
    R.b = P.pairs[2 * (long)p + 1];
  } else {
    R.a = P.query_first + p * P.query_step;
    R.b = P.train_first + p * P.train_step;
  }
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (R.a < 0 || R.a >= Q.frames || R.b < 0 || R.b >= T.frames) {  // (a bad entry of the caller's list; the arithmetic form is checked on the host)
    if (first) pair_rows[p] = -1;
    return false;
  }
  R.n_a = max(0, Q.counts[(long)R.a * Q.count_stride]);
  R.n_b = max(0, T.counts[(long)R.b * T.count_stride]);
  if (R.n_b >= (1 << MF_IDX_BITS) || (back_keys && R.n_a >= (1 << MF_IDX_BITS))) {  // (the keys hold 22 index bits)
    if (first) pair_rows[p] = -1;
    return false;
  }
  if (first) pair_rows[p] = R.n_a;
  R.rows = min(R.n_a, rows_cap);
  R.q_aligned = m_aligned(Q.desc, Q.frame_pitch, Q.row_pitch);
  R.t_aligned = m_aligned(T.desc, T.frame_pitch, T.row_pitch);
  return (int)blockIdx.x * 64 < R.rows;
}

// The position gate (brisk_match_gate.h): the mask of a pair is the gate's predicate on the two rows' keypoints, whose records lie
// row for row with the descriptors.  MpGate: the gate and the records of a pair's two frames.
struct MpGate {
  BriskMatchGate g;
  const char* qk;
  const char* tk;
};
__device__ __forceinline__ const BriskKeyPoint* mp_kp(const char* kps, int r) {
  return reinterpret_cast<const BriskKeyPoint*>(kps + (long)r * (long)sizeof(BriskKeyPoint));
}
// The guide (brisk_match_guide.h): the lane of query keypoint kp in a pair whose model record is *M - the gate's lane with the position
// replaced by the centre H(kp).  A workgroup is one pair, so M is wave-uniform (scalar loads, once per workgroup); the fp64 work is
// per lane and done before the scan, which keeps the lane alone: the nine model words and the temporaries are dead in the row loop.
// false: the row has no centre.
__device__ __forceinline__ bool mpu_lane(const BriskPairModel* __restrict__ M, bool guided, const BriskMatchGate& window, int fallback,
                                         const BriskKeyPoint* kp, BriskGateLane& L) {
  const BriskHomography H{M->h[0], M->h[1], M->h[2], M->h[3], M->h[4], M->h[5], M->h[6], M->h[7], M->h[8]};
  const BriskMatchGuide U{window, fallback};
  return brisk_guide_lane(U, guided, H, kp->x, kp->y, kp->octave, L);
}
// The kinds of guide of mp_body / mrp_body, and the model record each reads
#define MP_GUIDE_NONE 0
#define MP_GUIDE_CENTRE 1  // brisk_match_guide.h: the window centred at H(kp)
#define MP_GUIDE_LINE 2    // brisk_match_epiline.h: the window at kp itself, and the band around F kp
template <int GUIDE>
using MpModelOf = std::conditional_t<GUIDE == MP_GUIDE_LINE, BriskPairEpipolarModel, BriskPairModel>;
// The epipolar guide: the lane of query keypoint kp in a pair whose model record is *M - the gate's own lane and the line F kp with
// the band's bound w.  M is wave-uniform as in mpu_lane; what stays live across the scan is the lane and four doubles.
// false: the row matches nothing.
__device__ __forceinline__ bool mpe_lane(const BriskPairEpipolarModel* __restrict__ M, bool guided, const BriskMatchGate& window, float band,
                                         int fallback, const BriskKeyPoint* kp, BriskEpiLane& L) {
  const BriskFundamental F{M->f[0], M->f[1], M->f[2], M->f[3], M->f[4], M->f[5], M->f[6], M->f[7], M->f[8]};
  const BriskMatchEpiGuide U{window, band, fallback};
  return brisk_epiguide_lane(U, guided, F, kp->x, kp->y, kp->octave, L);
}

// The gated scans.  The keypoint of the wave-uniform row comes through the same scalar loads as the row itself, MPG_CHUNK records
// ahead of the rows they belong to (one wait for the chunk, not one per row); the predicate is a handful of VALU compares whose
// result lives in a lane mask.  A row that NO lane of the wave may match is left without its descriptor loads and popcounts: a
// uniform branch on the mask.  `on`: the lane takes part at all.
// ok[i]: this lane may match row tc + i; live[i]: the lanes of the wave that may.  The ballots are taken for the whole chunk BEFORE
// the first branch (a ballot is not moved below a branch), so the chunk's keypoint loads and compares stay together in front of
// its rows instead of one load and wait in front of each.  (No scheduling barrier between the loads and the compares: with one
// the compiler no longer takes the loop's loads - the descriptor rows included - for scalar loads.)
// SWAP (the cross check): the roles swap - the lane holds the train side's keypoint, the row passing by is a query row.
// LINE (the epipolar guide, never with SWAP): the row must also lie in the band around the lane's line *E when `band` (wave-uniform:
// the pair is guided) is set.
#define MPG_CHUNK 4
template <bool SWAP, bool LINE = false>
__device__ __forceinline__ void mpg_allowed(const BriskMatchGate& g, const BriskGateLane& L, bool on, const char* kps, int tc, int t1,
                                            bool (&ok)[MPG_CHUNK], unsigned long long (&live)[MPG_CHUNK], const BriskEpiLine* E = nullptr,
                                            bool band = false) {
#pragma unroll
  for (int i = 0; i < MPG_CHUNK; ++i) {
    const BriskKeyPoint* kp = mp_kp(kps, min(tc + i, t1 - 1));
    const bool pass = LINE   ? brisk_epiguide_query_lane(g, band, L, *E, kp->x, kp->y, kp->octave)
                      : SWAP ? brisk_gate_train_lane(g, L, kp->x, kp->y, kp->octave)
                             : brisk_gate_query_lane(g, L, kp->x, kp->y, kp->octave);
    ok[i] = on && tc + i < t1 && pass;
    live[i] = __ballot(ok[i]);
  }
}
// mp_scan behind the gate: the two smallest keys among the allowed rows
template <int W32, bool ALIGNED, bool SWAP, bool LINE = false>
__device__ __forceinline__ void mpg_scan(const unsigned (&qv)[W32], const uint8_t* rows, int pitch, int t0, int t1, const BriskMatchGate& g,
                                         const BriskGateLane& L, bool on, const char* kps, unsigned& b1, unsigned& b2,
                                         const BriskEpiLine* E = nullptr, bool band = false) {
  for (int tc = t0; tc < t1; tc += MPG_CHUNK) {
    bool ok[MPG_CHUNK];
    unsigned long long live[MPG_CHUNK];
    mpg_allowed<SWAP, LINE>(g, L, on, kps, tc, t1, ok, live, E, band);
#pragma unroll
    for (int i = 0; i < MPG_CHUNK; ++i) {
      if (live[i] == 0) continue;  // wave-uniform
      const int t = tc + i;
      const unsigned d = m_dist<W32, ALIGNED>(qv, rows + (long)t * pitch);
      m_top2(b1, b2, ok[i] ? m_key(d, t) : MF_NO_KEY);
    }
  }
}

// this wave's slice of the n rows of one frame against the lane's descriptor: the two smallest keys.  GATE: `self` is the lane's
// own keypoint, kps the records of the rows passing by; `guided` (the guided kernels): the lane as mpu_lane made it, instead of self's;
// LINE: `guided` and *E are what mpe_lane made, `band` as in mpg_allowed
template <int W32, bool GATE, bool SWAP, bool LINE = false>
__device__ __forceinline__ void mp_scan_slice(const unsigned (&v)[W32], const uint8_t* rows, int pitch, bool aligned, int n, int wave,
                                              const BriskMatchGate& g, const BriskKeyPoint* self, bool on, const char* kps, unsigned& b1,
                                              unsigned& b2, const BriskGateLane* guided = nullptr, const BriskEpiLine* E = nullptr,
                                              bool band = false) {
  const int per = (n + MP_WAVES - 1) / MP_WAVES;
  const int t0 = __builtin_amdgcn_readfirstlane(wave * per), t1 = min(n, t0 + per);
  if (GATE) {
    const BriskGateLane L = guided ? *guided : brisk_gate_lane(g, self->x, self->y, self->octave);
    if (aligned) mpg_scan<W32, true, SWAP, LINE>(v, rows, pitch, t0, t1, g, L, on, kps, b1, b2, E, band);
    else mpg_scan<W32, false, SWAP, LINE>(v, rows, pitch, t0, t1, g, L, on, kps, b1, b2, E, band);
  } else {
    if (aligned) mp_scan<W32, true>(v, rows, pitch, t0, t1, b1, b2);  // (batch results: 4-byte aligned rows at pitch 64)
    else mp_scan<W32, false>(v, rows, pitch, t0, t1, b1, b2);         // (a caller's set whose base, frame pitch or row pitch is not)
  }
}

// The backward scan of the mutual guided forms (k_mutual_centre_knn, k_mutual_line_knn).  The lane holds train row f(q) and its
// keypoint's lane TL; the rows passing by are QUERY rows, and the guide's mask needs what the model makes of each of them: its centre,
// or its line.  The wave makes them 64 at a time - lane i stages row base + i with the forward scan's own brisk_guide_centre /
// brisk_epiguide_lane, one fp64 prologue per 64 scanned rows - and the row loop reads record j out of lane j's registers with
// v_readlane (j is the loop's scalar counter).  A readlane writes SGPRs: the predicate's compares take the centre as scalar operands,
// exactly as mpg_scan's take the keypoint its scalar loads brought, and nothing of the staging goes through LDS - an LDS table would
// return to VGPRs and count on lgkmcnt beside the descriptor rows' scalar loads, whose out-of-order return forces every wait to 0.
// has-centre / has-line is one ballot per block, kept as a lane mask.  mpg_scan's chunks, ballots before the first branch and the
// live == 0 skip are kept: a query row that no lane may match costs its readlanes and compares only.
__device__ __forceinline__ float mpm_readlane(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }
__device__ __forceinline__ double mpm_readlane(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}
// rows [t0, t1) of frame a (wave-uniform) against the lane's train row tv: the smallest key (distance, q') among the rows whose mask
// allows the lane's train keypoint.  kps: frame a's keypoints; M, guided, fallback, band: as the forward scan's mpu_lane / mpe_lane
template <int W32, bool ALIGNED, int GUIDE>
__device__ __forceinline__ void mpm_scan(const unsigned (&tv)[W32], const uint8_t* rows, int pitch, int t0, int t1, const BriskMatchGate& g,
                                         const BriskGateLane& TL, bool on, const char* kps, const MpModelOf<GUIDE>* __restrict__ M, bool guided,
                                         int fallback, float band, int lane, unsigned& best) {
  for (int base = t0; base < t1; base += 64) {
    const int nblk = min(64, t1 - base);  // (wave-uniform)
    const BriskKeyPoint* kp = mp_kp(kps, base + min(lane, nblk - 1));
    float sx, sy;  // the centre, or the keypoint itself (the line form's window stays there)
    const int so = kp->octave;
    BriskEpiLine sl = {};
    bool shas;
    if constexpr (GUIDE == MP_GUIDE_LINE) {
      BriskEpiLane L;
      shas = mpe_lane(M, guided, g, band, fallback, kp, L);
      sx = kp->x;
      sy = kp->y;
      sl = L.line;
    } else {
      const BriskHomography H{M->h[0], M->h[1], M->h[2], M->h[3], M->h[4], M->h[5], M->h[6], M->h[7], M->h[8]};
      const BriskGuideCentre c = brisk_guide_centre(guided, fallback, H, kp->x, kp->y);
      sx = c.x;
      sy = c.y;
      shas = c.has;
    }
    const unsigned long long has = __ballot(shas);
    for (int jc = 0; jc < nblk; jc += MPG_CHUNK) {
      bool ok[MPG_CHUNK];
      unsigned long long live[MPG_CHUNK];
#pragma unroll
      for (int i = 0; i < MPG_CHUNK; ++i) {
        const int j = min(jc + i, nblk - 1);
        const bool hj = (has >> j) & 1;
        const float x = mpm_readlane(sx, j), y = mpm_readlane(sy, j);
        const int o = __builtin_amdgcn_readlane(so, j);
        bool pass;
        if constexpr (GUIDE == MP_GUIDE_LINE) {
          BriskEpiLine E = {};
          if (guided) E = BriskEpiLine{mpm_readlane(sl.l0, j), mpm_readlane(sl.l1, j), mpm_readlane(sl.l2, j), mpm_readlane(sl.w, j)};
          pass = brisk_epiguide_train_row(g, guided, TL, hj, E, x, y, o);
        } else {
          pass = brisk_guide_train_row(g, TL, hj, x, y, o);
        }
        ok[i] = on && jc + i < nblk && pass;
        live[i] = __ballot(ok[i]);
      }
#pragma unroll
      for (int i = 0; i < MPG_CHUNK; ++i) {
        if (live[i] == 0) continue;  // wave-uniform
        const int t = base + jc + i;
        const unsigned d = m_dist<W32, ALIGNED>(tv, rows + (long)t * pitch);
        best = min(best, ok[i] ? m_key(d, t) : MF_NO_KEY);
      }
    }
  }
}

// k-NN of a pair: k_match_knn_fused's scheme with MP_WAVES waves.
// CROSS (k == 1): the forward match t of row q is kept only if the best match of row t of frame b among ALL rows of frame a is q.
// Fused: once the forward keys are merged, lane q takes row t of frame b into its registers and the waves scan frame a the same
// way (top-1) - the same work as a role-swapped launch, without a scratch buffer of backward keys and without any hand-off
// between workgroups.
// GATE: a lane the gate forbids keeps MF_NO_KEY, so a row holds min(k, allowed rows) REAL matches and is never topped up; in the
// cross check a lane without a forward match takes no part.
// GUIDE (with GATE): `gate` is the guide's window, centred by models[p] (mpu_lane); a lane whose row has no centre
// takes no part, and a pair without a usable model and without the fallback has empty rows.  GUIDE == MP_GUIDE_LINE: the window stays
// at the lane's own keypoint, and the lane carries its epipolar line under models[p] and `band` (mpe_lane).
// GUIDE with CROSS (the mutual forms, k == 1): the backward scan asks the SAME mask from the train side - row q' of frame a may claim the
// lane's train row iff the guide allows (q', t) - through mpm_scan, which makes the centres / lines of the rows passing by on the way.
template <int W32, bool CROSS, bool GATE, int GUIDE = MP_GUIDE_NONE>
__device__ __forceinline__ void mp_body(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int pair0, int k, int rows_cap,
                                        BriskDMatch* __restrict__ out, int* __restrict__ out_count, int* __restrict__ pair_rows,
                                        const BriskKpSet& QK, const BriskKpSet& TK, const BriskMatchGate& gate,
                                        const MpModelOf<GUIDE>* __restrict__ models = nullptr, int fallback = 0, float band = 0.f) {
  __shared__ unsigned part[MP_WAVES][2][64];
  __shared__ unsigned fwd[64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = pair0 + blockIdx.y;
  MpPair R;
  if (!mp_resolve(Q, T, P, p, CROSS, rows_cap, pair_rows, R)) return;
  const int q = blockIdx.x * 64 + lane;
  BriskDMatch* orow = out + ((long)p * rows_cap + q) * k;
  int* ocnt = out_count + (long)p * rows_cap + q;
  const bool guided = GUIDE && brisk_guide_guided(models[p].hypothesis, models[p].flags);  // (wave-uniform)
  if (R.n_b == 0 || (GUIDE && !guided && fallback == 0)) {  // nothing to match against: empty rows (the reference tops up only when some train image has rows)
    if (wave == 0 && q < R.rows) *ocnt = 0;
    return;
  }
  const uint8_t* qrows = mp_frame(Q, R.a);
  const uint8_t* trows = mp_frame(T, R.b);
  const char* qk = GATE ? QK.kps + (long)R.a * QK.frame_pitch : nullptr;
  const char* tk = GATE ? TK.kps + (long)R.b * TK.frame_pitch : nullptr;
  unsigned b1 = MF_NO_KEY, b2 = MF_NO_KEY;
  {
    unsigned qv[W32];
    mp_load_row<W32>(qrows + (long)min(q, R.rows - 1) * Q.row_pitch, R.q_aligned, qv);
    if constexpr (GUIDE == MP_GUIDE_LINE) {
      BriskEpiLane L;
      const bool has = mpe_lane(models + p, guided, gate, band, fallback, mp_kp(qk, min(q, R.rows - 1)), L);
      mp_scan_slice<W32, GATE, false, true>(qv, trows, T.row_pitch, R.t_aligned, R.n_b, wave, gate, nullptr, q < R.rows && has, tk, b1, b2, &L.gate,
                                            &L.line, guided);
    } else if constexpr (GUIDE == MP_GUIDE_CENTRE) {
      BriskGateLane L;
      const bool has = mpu_lane(models + p, guided, gate, fallback, mp_kp(qk, min(q, R.rows - 1)), L);
      mp_scan_slice<W32, GATE, false>(qv, trows, T.row_pitch, R.t_aligned, R.n_b, wave, gate, nullptr, q < R.rows && has, tk, b1, b2, &L);
    } else {
      mp_scan_slice<W32, GATE, false>(qv, trows, T.row_pitch, R.t_aligned, R.n_b, wave, gate, GATE ? mp_kp(qk, min(q, R.rows - 1)) : nullptr,
                                      q < R.rows, tk, b1, b2);
    }
  }
  part[wave][0][lane] = b1;
  part[wave][1][lane] = b2;
  __syncthreads();
  unsigned m1 = MF_NO_KEY, m2 = MF_NO_KEY;
  if (wave == 0) m_merge<MP_WAVES>(part, lane, m1, m2);
  bool keep = true;
  if (CROSS) {
    if (wave == 0) fwd[lane] = m1;
    __syncthreads();  // (also: wave 0 has read part[] before anybody writes it again)
    const unsigned f = fwd[lane];
    const bool has = !GATE || f != MF_NO_KEY;  // (ungated, n_b >= 1: every lane has a real forward match; the gate may have left none)
    const int t = has ? (int)(f & MF_IDX_MASK) : 0;
    unsigned tv[W32];
    mp_load_row<W32>(trows + (long)t * T.row_pitch, R.t_aligned, tv);
    unsigned c1 = MF_NO_KEY, c2 = MF_NO_KEY;
    // ALL rows q' of frame a, also those beyond rows_cap
    if constexpr (GUIDE != MP_GUIDE_NONE) {  // the guide's mask from the train side: mpm_scan
      const BriskKeyPoint* tkp = mp_kp(tk, t);
      const BriskGateLane TL = brisk_gate_lane(gate, tkp->x, tkp->y, tkp->octave);
      const int per = (R.n_a + MP_WAVES - 1) / MP_WAVES;
      const int t0 = __builtin_amdgcn_readfirstlane(wave * per), t1 = min(R.n_a, t0 + per);
      if (R.q_aligned) mpm_scan<W32, true, GUIDE>(tv, qrows, Q.row_pitch, t0, t1, gate, TL, has, qk, models + p, guided, fallback, band, lane, c1);
      else mpm_scan<W32, false, GUIDE>(tv, qrows, Q.row_pitch, t0, t1, gate, TL, has, qk, models + p, guided, fallback, band, lane, c1);
    } else {
      mp_scan_slice<W32, GATE, true>(tv, qrows, Q.row_pitch, R.q_aligned, R.n_a, wave, gate, GATE ? mp_kp(tk, t) : nullptr, has, qk, c1, c2);
    }
    part[wave][0][lane] = c1;
    __syncthreads();
    if (wave == 0) {
      unsigned best = MF_NO_KEY;
#pragma unroll
      for (int w = 0; w < MP_WAVES; ++w) best = min(best, part[w][0][lane]);
      keep = has && (int)(best & MF_IDX_MASK) == q;
    }
  }
  if (wave == 0 && q < R.rows) {
    int n = 0;
    if (keep && (!GATE || m1 != MF_NO_KEY)) {
      BriskDMatch m;
      m.queryIdx = q; m.imgIdx = R.b;
      m_key_to(m1, m);
      orow[0] = m;
      n = 1;
      if (k > 1 && (!GATE || m2 != MF_NO_KEY)) {  // (gated: a second entry only where a second row is allowed)
        if (m2 != MF_NO_KEY) {
          m_key_to(m2, m);
        } else {  // n_b < k: the reference's top-up entry (k_match_knn above; brute-force-matcher.cc:139-153)
          m.trainIdx = 0; m.distance = 2147483648.0f;
        }
        orow[1] = m;
        n = 2;
      }
    }
    *ocnt = n;
  }
}

template <int W32, bool CROSS>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_knn_pairs(const BriskDescSet Q, const BriskDescSet T, const BriskPairSpec P,
                                                                    int pair0, int k, int rows_cap, BriskDMatch* __restrict__ out,
                                                                    int* __restrict__ out_count, int* __restrict__ pair_rows) {
  mp_body<W32, CROSS, false>(Q, T, P, pair0, k, rows_cap, out, out_count, pair_rows, BriskKpSet(), BriskKpSet(), BriskMatchGate());
}
template <int W32, bool CROSS>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_knn_pairs_gated(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                          const BriskKpSet TK, const BriskMatchGate gate,
                                                                          const BriskPairSpec P, int pair0, int k, int rows_cap,
                                                                          BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                          int* __restrict__ pair_rows) {
  mp_body<W32, CROSS, true>(Q, T, P, pair0, k, rows_cap, out, out_count, pair_rows, QK, TK, gate);
}
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_guided_knn_pairs(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                     const BriskKpSet TK, const BriskPairModel* __restrict__ models,
                                                                     const BriskMatchGuide guide, const BriskPairSpec P, int pair0, int k,
                                                                     int rows_cap, BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                     int* __restrict__ pair_rows) {
  mp_body<W32, false, true, MP_GUIDE_CENTRE>(Q, T, P, pair0, k, rows_cap, out, out_count, pair_rows, QK, TK, guide.window, models, guide.fallback);
}
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_epiline_knn_pairs(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                      const BriskKpSet TK, const BriskPairEpipolarModel* __restrict__ models,
                                                                      const BriskMatchEpiGuide guide, const BriskPairSpec P, int pair0, int k,
                                                                      int rows_cap, BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                      int* __restrict__ pair_rows) {
  mp_body<W32, false, true, MP_GUIDE_LINE>(Q, T, P, pair0, k, rows_cap, out, out_count, pair_rows, QK, TK, guide.window, models, guide.fallback,
                                           guide.band);
}
// the mutual guided forms: the guided / epipolar-guided k-NN kernel for k = 1 with the cross check fused (mp_body's CROSS with a guide)
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_mutual_centre_knn(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                      const BriskKpSet TK, const BriskPairModel* __restrict__ models,
                                                                      const BriskMatchGuide guide, const BriskPairSpec P, int pair0, int rows_cap,
                                                                      BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                      int* __restrict__ pair_rows) {
  mp_body<W32, true, true, MP_GUIDE_CENTRE>(Q, T, P, pair0, 1, rows_cap, out, out_count, pair_rows, QK, TK, guide.window, models, guide.fallback);
}
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_mutual_line_knn(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                    const BriskKpSet TK, const BriskPairEpipolarModel* __restrict__ models,
                                                                    const BriskMatchEpiGuide guide, const BriskPairSpec P, int pair0, int rows_cap,
                                                                    BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                    int* __restrict__ pair_rows) {
  mp_body<W32, true, true, MP_GUIDE_LINE>(Q, T, P, pair0, 1, rows_cap, out, out_count, pair_rows, QK, TK, guide.window, models, guide.fallback,
                                          guide.band);
}

// ------------------------------------------------------------------------------------------------
// Radius matching in mp_body's shape.  No distance matrix: a hit ((float)d < max_distance, brute-force-matcher.cc:203-207) bumps
// its query's counter in LDS and, while the query's short LDS list has room, drops its packed key there.  Keys are unique per
// train row, so the order of collection does not matter:
//   sparse rows (count <= MRP_LIST): MP_WAVES threads per query rank the keys of the list against each other and store those
//       of rank < cap at their rank - (distance, trainIdx) order;
//   dense rows (the list overflowed): one wave per such query runs k_match_radius' algorithm with the distances recomputed on
//       the fly (lane = train row, the query wave-uniform): histogram over the distances below the threshold, exclusive prefix,
//       stable placement in train order.  Second phase of the same workgroup: nothing between the phases leaves the CU.
// The counter holds the number FOUND in both cases.
// ------------------------------------------------------------------------------------------------
#ifndef MRP_LIST
#define MRP_LIST 32  // keys per query held in LDS (8 KiB per workgroup); a row with more hits takes the dense path
#endif
#define MRP_BINS 513                    // distances 0 ... 512 (descriptors of at most 64 bytes)
#define MRP_PER ((MRP_BINS + 63) / 64)  // bins per lane in the prefix

// a hit of the lane's query: counted, and listed while the list has room
__device__ __forceinline__ void mrp_hit(unsigned key, int* cnt, unsigned (*list)[64], int lane) {
  const int slot = atomicAdd(&cnt[lane], 1);
  if (slot < MRP_LIST) list[slot][lane] = key;
}
// rows [t0, t1) of one frame (wave-uniform addresses) against the lane's descriptor: hits (d < thr) into the lane's counter and list
template <int W32, bool ALIGNED>
__device__ __forceinline__ void mrp_scan(const unsigned (&qv)[W32], const uint8_t* rows, int pitch, int t0, int t1, unsigned thr,
                                         int* cnt, unsigned (*list)[64], int lane) {
  for (int t = t0; t < t1; ++t) {
    const unsigned d = m_dist<W32, ALIGNED>(qv, rows + (long)t * pitch);
    if (d < thr) mrp_hit(m_key(d, t), cnt, list, lane);
  }
}
// mrp_scan behind the gate (mpg_scan's loop)
template <int W32, bool ALIGNED, bool LINE = false>
__device__ __forceinline__ void mrpg_scan(const unsigned (&qv)[W32], const uint8_t* rows, int pitch, int t0, int t1, unsigned thr,
                                          const BriskMatchGate& g, const BriskGateLane& L, bool on, const char* kps, int* cnt,
                                          unsigned (*list)[64], int lane, const BriskEpiLine* E = nullptr, bool band = false) {
  for (int tc = t0; tc < t1; tc += MPG_CHUNK) {
    bool ok[MPG_CHUNK];
    unsigned long long live[MPG_CHUNK];
    mpg_allowed<false, LINE>(g, L, on, kps, tc, t1, ok, live, E, band);
#pragma unroll
    for (int i = 0; i < MPG_CHUNK; ++i) {
      if (live[i] == 0) continue;  // wave-uniform
      const int t = tc + i;
      const unsigned d = m_dist<W32, ALIGNED>(qv, rows + (long)t * pitch);
      if (ok[i] && d < thr) mrp_hit(m_key(d, t), cnt, list, lane);
    }
  }
}
// the dense path's distance of train row t (one per lane) to the wave's query; GATE: a row the gate forbids is no hit (thr);
// LINE: nor is a row outside the band around the query's line *E (wave-uniform) when `band` is set
template <int W32, bool ALIGNED, bool GATE, bool LINE = false>
__device__ __forceinline__ unsigned mrp_dense_dist(const unsigned (&uq)[W32], const uint8_t* trows, int t_pitch, int t, unsigned thr,
                                                   const MpGate& G, const BriskGateLane& QL, const BriskEpiLine* E = nullptr, bool band = false) {
  if (LINE) {
    const BriskKeyPoint* kp = mp_kp(G.tk, t);
    if (!brisk_epiguide_query_lane(G.g, band, QL, *E, kp->x, kp->y, kp->octave)) return thr;
  } else if (GATE) {
    const BriskKeyPoint* kp = mp_kp(G.tk, t);
    if (!brisk_gate_query_lane(G.g, QL, kp->x, kp->y, kp->octave)) return thr;
  }
  return m_dist<W32, ALIGNED>(uq, trows + (long)t * t_pitch);
}
// one wave, one query with more than MRP_LIST hits.  bins: thr + 1 ints of this wave's own
template <int W32, bool ALIGNED, bool GATE, bool LINE = false>
__device__ __forceinline__ void mrp_dense(int* bins, const unsigned (&uq)[W32], const uint8_t* trows, int t_pitch, int n_b, unsigned thr,
                                          int cap, int lane, int q, int img, BriskDMatch* __restrict__ orow, const MpGate& G,
                                          const BriskGateLane& QL, const BriskEpiLine* E = nullptr, bool band = false) {
  for (int b = lane; b <= (int)thr; b += 64) bins[b] = 0;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  for (int t = lane; t < n_b; t += 64) {
    const unsigned d = mrp_dense_dist<W32, ALIGNED, GATE, LINE>(uq, trows, t_pitch, t, thr, G, QL, E, band);
    if (d < thr) atomicAdd(&bins[d], 1);
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  {  // exclusive prefix over the thr (<= 513) bins: MRP_PER consecutive bins per lane, a scan of the lane sums in between
    int loc[MRP_PER], sum = 0;
#pragma unroll
    for (int i = 0; i < MRP_PER; ++i) {
      const int b = lane * MRP_PER + i;
      loc[i] = b < (int)thr ? bins[b] : 0;
      sum += loc[i];
    }
    int incl = sum;
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    int acc = incl - sum;
#pragma unroll
    for (int i = 0; i < MRP_PER; ++i) {
      const int b = lane * MRP_PER + i;
      if (b < (int)thr) bins[b] = acc;
      acc += loc[i];
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  // stable placement (k_match_radius): chunks of 64 train rows in order; inside a chunk equal distances keep lane order.  A bin's
  // base only grows: a hit whose bin has reached cap is never stored and takes no part
  for (int t0 = 0; t0 < n_b; t0 += 64) {
    const int t = t0 + lane;
    unsigned d = thr;
    if (t < n_b) d = mrp_dense_dist<W32, ALIGNED, GATE, LINE>(uq, trows, t_pitch, t, thr, G, QL, E, band);
    const bool hit = d < thr && bins[d] < cap;
    unsigned long long todo = __ballot(hit);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned dsel = __shfl(d, leader, 64);
      const unsigned long long same = __ballot(hit && d == dsel);
      const int base = bins[dsel];
      if (hit && d == dsel) {
        const int pos = base + __popcll(same & ((1ull << lane) - 1ull));
        if (pos < cap) {
          BriskDMatch m;
          m.queryIdx = q; m.trainIdx = t; m.imgIdx = img; m.distance = (float)d;
          orow[pos] = m;
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (lane == leader) bins[dsel] = base + __popcll(same);
      __builtin_amdgcn_s_waitcnt(0);
      __builtin_amdgcn_wave_barrier();
      todo &= ~same;
    }
  }
}

// the workgroup's 64 query rows [blockIdx.x * 64, ...) of `rows` against the n_b train rows; out / out_count: row 0 of this query set
// GUIDE (with GATE): G.g is the guide's window, centred by the pair's model record *model (mpu_lane); MP_GUIDE_LINE: the window stays at
// the query keypoint and the rows pass the band around its line under *model (mpe_lane)
template <int W32, bool GATE = false, int GUIDE = MP_GUIDE_NONE>
__device__ __forceinline__ void mrp_body(const uint8_t* qrows, int q_pitch, bool q_aligned, int rows, const uint8_t* trows, int t_pitch,
                                         bool t_aligned, int n_b, float max_distance, int cap, int img, BriskDMatch* __restrict__ out,
                                         int* __restrict__ out_count, const MpGate& G = MpGate(),
                                         const MpModelOf<GUIDE>* __restrict__ model = nullptr, bool guided = false, int fallback = 0,
                                         float band = 0.f) {
  __shared__ int cnt[64];
  __shared__ unsigned list[MRP_LIST][64];
  __shared__ int bins[MP_WAVES][MRP_BINS + 3];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int q = blockIdx.x * 64 + lane;
  // d is an integer: (float)d < max_distance <=> d < ceil(max_distance); nothing hits for max_distance <= 0 or NaN, and no
  // distance exceeds 32 * W32
  const unsigned thr = max_distance > 0.f ? (unsigned)fminf(ceilf(max_distance), (float)(32 * W32 + 1)) : 0u;
  if (n_b == 0 || thr == 0) {  // (radius matching has no top-up entry)
    if (wave == 0 && q < rows) out_count[q] = 0;
    return;
  }
  if (wave == 0) cnt[lane] = 0;
  __syncthreads();
  {
    unsigned qv[W32];
    mp_load_row<W32>(qrows + (long)min(q, rows - 1) * q_pitch, q_aligned, qv);
    const unsigned thr_lane = q < rows ? thr : 0u;  // (the lanes behind the last row collect nothing)
    const int per = (n_b + MP_WAVES - 1) / MP_WAVES;
    const int t0 = wave * per, t1 = min(n_b, t0 + per);
    if (GATE) {
      const BriskKeyPoint* kp = mp_kp(G.qk, min(q, rows - 1));
      bool on = q < rows;
      if constexpr (GUIDE == MP_GUIDE_LINE) {
        BriskEpiLane L;
        on = mpe_lane(model, guided, G.g, band, fallback, kp, L) && on;
        if (t_aligned) mrpg_scan<W32, true, true>(qv, trows, t_pitch, t0, t1, thr, G.g, L.gate, on, G.tk, cnt, list, lane, &L.line, guided);
        else mrpg_scan<W32, false, true>(qv, trows, t_pitch, t0, t1, thr, G.g, L.gate, on, G.tk, cnt, list, lane, &L.line, guided);
      } else {
        BriskGateLane L;
        if (GUIDE) on = mpu_lane(model, guided, G.g, fallback, kp, L) && on;
        else L = brisk_gate_lane(G.g, kp->x, kp->y, kp->octave);
        if (t_aligned) mrpg_scan<W32, true>(qv, trows, t_pitch, t0, t1, thr, G.g, L, on, G.tk, cnt, list, lane);
        else mrpg_scan<W32, false>(qv, trows, t_pitch, t0, t1, thr, G.g, L, on, G.tk, cnt, list, lane);
      }
    } else {
      if (t_aligned) mrp_scan<W32, true>(qv, trows, t_pitch, t0, t1, thr_lane, cnt, list, lane);
      else mrp_scan<W32, false>(qv, trows, t_pitch, t0, t1, thr_lane, cnt, list, lane);
    }
  }
  __syncthreads();
  {  // counts of all rows; sparse rows: MP_WAVES threads per query, each ranks every MP_WAVES-th key of the list
    const int ql = threadIdx.x / MP_WAVES, sub = threadIdx.x % MP_WAVES;
    const int qq = blockIdx.x * 64 + ql;
    if (qq < rows) {
      const int c = cnt[ql];
      if (sub == 0) out_count[qq] = c;
      if (c <= MRP_LIST) {
        BriskDMatch* orow = out + (long)qq * cap;
        for (int j = sub; j < c; j += MP_WAVES) {
          const unsigned key = list[j][ql];
          int rank = 0;
          for (int i = 0; i < c; ++i) rank += list[i][ql] < key ? 1 : 0;
          if (rank < cap) {
            BriskDMatch m;
            m.queryIdx = qq; m.trainIdx = (int)(key & ((1u << MF_IDX_BITS) - 1)); m.imgIdx = img; m.distance = (float)(key >> MF_IDX_BITS);
            orow[rank] = m;
          }
        }
      }
    }
  }
  for (int ql = wave; ql < 64; ql += MP_WAVES) {  // dense rows: one wave each
    const int qq = blockIdx.x * 64 + ql;
    if (qq >= rows) break;
    if (cnt[ql] <= MRP_LIST) continue;
    unsigned uq[W32];
    mp_load_row<W32>(qrows + (long)qq * q_pitch, q_aligned, uq);
    if constexpr (GUIDE == MP_GUIDE_LINE) {  // (the model is read again, as below; the query's line is wave-uniform)
      BriskEpiLane QE;
      if (!mpe_lane(model, guided, G.g, band, fallback, mp_kp(G.qk, qq), QE)) continue;  // (cannot be: a row without a line has no hits)
      if (t_aligned)
        mrp_dense<W32, true, GATE, true>(bins[wave], uq, trows, t_pitch, n_b, thr, cap, lane, qq, img, out + (long)qq * cap, G, QE.gate, &QE.line, guided);
      else
        mrp_dense<W32, false, GATE, true>(bins[wave], uq, trows, t_pitch, n_b, thr, cap, lane, qq, img, out + (long)qq * cap, G, QE.gate, &QE.line, guided);
    } else {
      BriskGateLane QL = {};
      if (GATE) {
        const BriskKeyPoint* kp = mp_kp(G.qk, qq);  // (wave-uniform)
        if (GUIDE) {  // (the model is read again: a rare path, and nothing of it stays live across the scan)
          if (!mpu_lane(model, guided, G.g, fallback, kp, QL)) continue;  // (cannot be: a row without a centre has no hits)
        } else {
          QL = brisk_gate_lane(G.g, kp->x, kp->y, kp->octave);
        }
      }
      if (t_aligned) mrp_dense<W32, true, GATE>(bins[wave], uq, trows, t_pitch, n_b, thr, cap, lane, qq, img, out + (long)qq * cap, G, QL);
      else mrp_dense<W32, false, GATE>(bins[wave], uq, trows, t_pitch, n_b, thr, cap, lane, qq, img, out + (long)qq * cap, G, QL);
    }
  }
}

template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_radius_pairs(const BriskDescSet Q, const BriskDescSet T, const BriskPairSpec P,
                                                                       int pair0, float max_distance, int cap, int rows_cap,
                                                                       BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                       int* __restrict__ pair_rows) {
  const int p = pair0 + blockIdx.y;
  MpPair R;
  if (!mp_resolve(Q, T, P, p, false, rows_cap, pair_rows, R)) return;
  mrp_body<W32>(mp_frame(Q, R.a), Q.row_pitch, R.q_aligned, R.rows, mp_frame(T, R.b), T.row_pitch, R.t_aligned, R.n_b, max_distance, cap, R.b,
                out + (long)p * rows_cap * cap, out_count + (long)p * rows_cap);
}
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_radius_pairs_gated(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                             const BriskKpSet TK, const BriskMatchGate gate,
                                                                             const BriskPairSpec P, int pair0, float max_distance, int cap,
                                                                             int rows_cap, BriskDMatch* __restrict__ out,
                                                                             int* __restrict__ out_count, int* __restrict__ pair_rows) {
  const int p = pair0 + blockIdx.y;
  MpPair R;
  if (!mp_resolve(Q, T, P, p, false, rows_cap, pair_rows, R)) return;
  const MpGate G{gate, QK.kps + (long)R.a * QK.frame_pitch, TK.kps + (long)R.b * TK.frame_pitch};
  mrp_body<W32, true>(mp_frame(Q, R.a), Q.row_pitch, R.q_aligned, R.rows, mp_frame(T, R.b), T.row_pitch, R.t_aligned, R.n_b, max_distance, cap, R.b,
                      out + (long)p * rows_cap * cap, out_count + (long)p * rows_cap, G);
}
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_guided_radius_pairs(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                        const BriskKpSet TK, const BriskPairModel* __restrict__ models,
                                                                        const BriskMatchGuide guide, const BriskPairSpec P, int pair0,
                                                                        float max_distance, int cap, int rows_cap,
                                                                        BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                        int* __restrict__ pair_rows) {
  const int p = pair0 + blockIdx.y;
  MpPair R;
  if (!mp_resolve(Q, T, P, p, false, rows_cap, pair_rows, R)) return;
  const bool guided = brisk_guide_guided(models[p].hypothesis, models[p].flags);  // (wave-uniform)
  const int n_b = guided || guide.fallback != 0 ? R.n_b : 0;  // a pair without a usable model and without the fallback: empty rows
  const MpGate G{guide.window, QK.kps + (long)R.a * QK.frame_pitch, TK.kps + (long)R.b * TK.frame_pitch};
  mrp_body<W32, true, MP_GUIDE_CENTRE>(mp_frame(Q, R.a), Q.row_pitch, R.q_aligned, R.rows, mp_frame(T, R.b), T.row_pitch, R.t_aligned, n_b, max_distance,
                                       cap, R.b, out + (long)p * rows_cap * cap, out_count + (long)p * rows_cap, G, models + p, guided, guide.fallback);
}
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_epiline_radius_pairs(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                         const BriskKpSet TK, const BriskPairEpipolarModel* __restrict__ models,
                                                                         const BriskMatchEpiGuide guide, const BriskPairSpec P, int pair0,
                                                                         float max_distance, int cap, int rows_cap,
                                                                         BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                         int* __restrict__ pair_rows) {
  const int p = pair0 + blockIdx.y;
  MpPair R;
  if (!mp_resolve(Q, T, P, p, false, rows_cap, pair_rows, R)) return;
  const bool guided = brisk_guide_guided(models[p].hypothesis, models[p].flags);  // (wave-uniform)
  const int n_b = guided || guide.fallback != 0 ? R.n_b : 0;  // a pair without a usable model and without the fallback: empty rows
  const MpGate G{guide.window, QK.kps + (long)R.a * QK.frame_pitch, TK.kps + (long)R.b * TK.frame_pitch};
  mrp_body<W32, true, MP_GUIDE_LINE>(mp_frame(Q, R.a), Q.row_pitch, R.q_aligned, R.rows, mp_frame(T, R.b), T.row_pitch, R.t_aligned, n_b, max_distance,
                                     cap, R.b, out + (long)p * rows_cap * cap, out_count + (long)p * rows_cap, G, models + p, guided, guide.fallback,
                                     guide.band);
}
// one query set against one train set, counts from the host (brisk_hip_match_radius_device); grid ceil(nq / 64)
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_radius_pairs_one(const uint8_t* __restrict__ query, int q_pitch, int nq,
                                                                           const uint8_t* __restrict__ train, int t_pitch, int nt,
                                                                           float max_distance, int cap, BriskDMatch* __restrict__ out,
                                                                           int* __restrict__ out_count) {
  mrp_body<W32>(query, q_pitch, m_aligned(query, 0, q_pitch), nq, train, t_pitch, m_aligned(train, 0, t_pitch), nt, max_distance, cap, 0, out,
                out_count);
}

// ------------------------------------------------------------------------------------------------
// Launches of the register-row path.  The brisk_launch_* functions return false when the case is not covered (the descriptor
// size, or what each states): the caller uses the distance-matrix path or reports it.
// ------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, W32>) for the descriptor sizes the kernels are built for: 16, 32, 48, 64 bytes
template <class F>
static bool m_dispatch_words(int words32, F&& f) {
  switch (words32) {
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 12: f(std::integral_constant<int, 12>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    default: return false;
  }
  return true;
}
// launch(grid, first pair) for grid (ceil(rows_cap / 64), pairs), 65535 pairs at a time (what grid.y holds)
template <class F>
static void mp_launch_pairs(int npairs, int rows_cap, F&& launch) {
  for (int p0 = 0; p0 < npairs; p0 += 65535) launch(dim3((rows_cap + 63) / 64, min(65535, npairs - p0)), p0);
}

bool brisk_launch_match_knn_fused(const uint8_t* query, int q_pitch, int nq, const uint8_t* train, int t_pitch, int nt,
                                  int words32, int k, BriskDMatch* out, int* out_count, hipStream_t s) {
  if (k < 1 || k > 2 || nt < k || nt >= (1 << MF_IDX_BITS) || nq <= 0) return false;
  return m_dispatch_words(words32, [&](auto W) {
    hipLaunchKernelGGL(k_match_knn_fused<decltype(W)::value>, dim3((nq + 63) / 64), dim3(MF_WAVES * 64), 0, s, query, q_pitch, nq, train,
                       t_pitch, nt, k, out, out_count);
  });
}
bool brisk_launch_match_knn_pairs(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int words32, int k, bool cross,
                                  int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    constexpr int W32 = decltype(W)::value;
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      if (cross) hipLaunchKernelGGL((k_match_knn_pairs<W32, true>), grid, dim3(MP_WAVES * 64), 0, s, Q, T, P, p0, k, rows_cap, out, out_count, pair_rows);
      else hipLaunchKernelGGL((k_match_knn_pairs<W32, false>), grid, dim3(MP_WAVES * 64), 0, s, Q, T, P, p0, k, rows_cap, out, out_count, pair_rows);
    });
  });
}
bool brisk_launch_match_knn_pairs_gated(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                        const BriskMatchGate& gate, const BriskPairSpec& P, int words32, int k, bool cross, int rows_cap,
                                        BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    constexpr int W32 = decltype(W)::value;
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      if (cross)
        hipLaunchKernelGGL((k_match_knn_pairs_gated<W32, true>), grid, dim3(MP_WAVES * 64), 0, s, Q, T, QK, TK, gate, P, p0, k, rows_cap, out, out_count, pair_rows);
      else
        hipLaunchKernelGGL((k_match_knn_pairs_gated<W32, false>), grid, dim3(MP_WAVES * 64), 0, s, Q, T, QK, TK, gate, P, p0, k, rows_cap, out, out_count, pair_rows);
    });
  });
}
bool brisk_launch_match_radius_pairs(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int words32, float max_distance,
                                     int cap, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      hipLaunchKernelGGL(k_match_radius_pairs<decltype(W)::value>, grid, dim3(MP_WAVES * 64), 0, s, Q, T, P, p0, max_distance, cap, rows_cap, out,
                         out_count, pair_rows);
    });
  });
}
bool brisk_launch_match_radius_pairs_gated(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                           const BriskMatchGate& gate, const BriskPairSpec& P, int words32, float max_distance, int cap,
                                           int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      hipLaunchKernelGGL(k_match_radius_pairs_gated<decltype(W)::value>, grid, dim3(MP_WAVES * 64), 0, s, Q, T, QK, TK, gate, P, p0, max_distance, cap,
                         rows_cap, out, out_count, pair_rows);
    });
  });
}
bool brisk_launch_match_knn_pairs_guided(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                         const BriskPairModel* models, const BriskMatchGuide& guide, const BriskPairSpec& P, int words32, int k,
                                         int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      hipLaunchKernelGGL(k_guided_knn_pairs<decltype(W)::value>, grid, dim3(MP_WAVES * 64), 0, s, Q, T, QK, TK, models, guide, P, p0, k, rows_cap, out,
                         out_count, pair_rows);
    });
  });
}
bool brisk_launch_match_radius_pairs_guided(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                            const BriskPairModel* models, const BriskMatchGuide& guide, const BriskPairSpec& P, int words32,
                                            float max_distance, int cap, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows,
                                            hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      hipLaunchKernelGGL(k_guided_radius_pairs<decltype(W)::value>, grid, dim3(MP_WAVES * 64), 0, s, Q, T, QK, TK, models, guide, P, p0, max_distance,
                         cap, rows_cap, out, out_count, pair_rows);
    });
  });
}
bool brisk_launch_match_knn_pairs_epiline(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                          const BriskPairEpipolarModel* models, const BriskMatchEpiGuide& guide, const BriskPairSpec& P,
                                          int words32, int k, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      hipLaunchKernelGGL(k_epiline_knn_pairs<decltype(W)::value>, grid, dim3(MP_WAVES * 64), 0, s, Q, T, QK, TK, models, guide, P, p0, k, rows_cap, out,
                         out_count, pair_rows);
    });
  });
}
bool brisk_launch_match_radius_pairs_epiline(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                             const BriskPairEpipolarModel* models, const BriskMatchEpiGuide& guide, const BriskPairSpec& P,
                                             int words32, float max_distance, int cap, int rows_cap, BriskDMatch* out, int* out_count,
                                             int* pair_rows, hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      hipLaunchKernelGGL(k_epiline_radius_pairs<decltype(W)::value>, grid, dim3(MP_WAVES * 64), 0, s, Q, T, QK, TK, models, guide, P, p0, max_distance,
                         cap, rows_cap, out, out_count, pair_rows);
    });
  });
}
bool brisk_launch_match_mutual_pairs_guided(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                            const BriskPairModel* models, const BriskMatchGuide& guide, const BriskPairSpec& P, int words32,
                                            int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      hipLaunchKernelGGL(k_mutual_centre_knn<decltype(W)::value>, grid, dim3(MP_WAVES * 64), 0, s, Q, T, QK, TK, models, guide, P, p0, rows_cap, out,
                         out_count, pair_rows);
    });
  });
}
bool brisk_launch_match_mutual_pairs_epiline(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                             const BriskPairEpipolarModel* models, const BriskMatchEpiGuide& guide, const BriskPairSpec& P,
                                             int words32, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  return m_dispatch_words(words32, [&](auto W) {
    mp_launch_pairs(P.npairs, rows_cap, [&](dim3 grid, int p0) {
      hipLaunchKernelGGL(k_mutual_line_knn<decltype(W)::value>, grid, dim3(MP_WAVES * 64), 0, s, Q, T, QK, TK, models, guide, P, p0, rows_cap, out,
                         out_count, pair_rows);
    });
  });
}
// (also not covered: nt >= 2^22)
bool brisk_launch_match_radius_fused(const uint8_t* query, int q_pitch, int nq, const uint8_t* train, int t_pitch, int nt, int words32,
                                     float max_distance, int cap, BriskDMatch* out, int* out_count, hipStream_t s) {
  if (nq <= 0 || nt < 0 || nt >= (1 << MF_IDX_BITS) || cap < 1) return false;
  return m_dispatch_words(words32, [&](auto W) {
    hipLaunchKernelGGL(k_match_radius_pairs_one<decltype(W)::value>, dim3((nq + 63) / 64), dim3(MP_WAVES * 64), 0, s, query, q_pitch, nq, train, t_pitch,
                       nt, max_distance, cap, out, out_count);
  });
}

void brisk_launch_match_dist(const uint8_t* query, int q_pitch, int q0, int nqb, const uint8_t* train, int t_pitch, int nt,
                             int words, const uint8_t* mask, long mask_pitch, uint16_t* dist, long dist_pitch,
                             hipStream_t s) {
  if (nt <= 0 || nqb <= 0) return;
  const dim3 grid((nt + MT_THREADS - 1) / MT_THREADS, (nqb + MT_QTILE - 1) / MT_QTILE);
  if (words <= 8)
    hipLaunchKernelGGL(k_match_dist<8>, grid, dim3(MT_THREADS), 0, s, query, q_pitch, q0, nqb, train, t_pitch, nt, words, mask,
                       mask_pitch, dist, dist_pitch);
  else
    hipLaunchKernelGGL(k_match_dist<MT_MAXWORDS_LONG>, grid, dim3(MT_THREADS), 0, s, query, q_pitch, q0, nqb, train, t_pitch, nt,
                       words, mask, mask_pitch, dist, dist_pitch);
}
void brisk_launch_match_masked_out(const uint8_t* mask, long mask_pitch, int q0, int nqb, const int* img_start,
                                   const int* has_mask, int nimg, int* masked, hipStream_t s) {
  if (nqb <= 0) return;
  hipLaunchKernelGGL(k_match_masked_out, dim3(nqb), dim3(64), 0, s, mask, mask_pitch, q0, img_start, has_mask, nimg, masked);
}
void brisk_launch_match_knn(const uint16_t* dist, long dist_pitch, int q0, int nqb, int nt, const int* img_start, int nimg,
                            const int* masked, int k, BriskDMatch* out, int* out_count, hipStream_t s) {
  if (nqb <= 0) return;
  hipLaunchKernelGGL(k_match_knn, dim3(nqb), dim3(64), 0, s, dist, dist_pitch, q0, nt, img_start, nimg, masked, k, out,
                     out_count);
}
void brisk_launch_match_radius(const uint16_t* dist, long dist_pitch, int q0, int nqb, int nt, const int* img_start,
                               int nimg, const int* masked, float max_distance, int cap, BriskDMatch* out, int* out_count,
                               int dim_bytes, hipStream_t s) {
  if (nqb <= 0) return;
  hipLaunchKernelGGL(k_match_radius, dim3(nqb), dim3(64), 0, s, dist, dist_pitch, q0, nt, img_start, nimg, masked,
                     max_distance, cap, out, out_count, min(dim_bytes * 8 + 1, MR_BINS));
}
