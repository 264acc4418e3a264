// brisk_track.hip - a batch's pair matches linked into feature tracks (brisk_hip_link_tracks_device, brisk_hip_list_tracks_device).
//
// The packed lists brisk_hip_select_pair_matches_device leaves in HBM say "row q of frame i matched row t of frame i - 1".  The
// rule that turns them into tracks is brisk_track_link.h; these kernels apply it to a chain of `nodes` frames:
//   k_track_init          one lane per row, blockIdx.y = node: claim word cleared, prev = -1; the call's counters cleared
//   k_track_propose       one lane per record, blockIdx.y = pair: one no-return 64-bit atomicMin per proposal on its train row's claim
//   k_track_resolve       the same records again: the proposal whose key IS the claim writes prev; links / losers / ignored counted
//   k_track_count         starting heads per workgroup of rows
//   k_track_offsets       one workgroup: exclusive prefix sums of the workgroup sums (the pattern of k_pair_select_offsets), first_new
//                         taken from the device word or the argument, the summary
//   k_track_number        the count pass again, a scan inside the workgroup: every head takes its number (or its seed) and WALKS
//                         its chain along the claim words, leaving track and age on every row (O(observations) stores; the longest
//                         track of the call is nodes - 1 dependent loads)
// and pack the pieces worth keeping, in (node, row) order of their heads, by stable compaction:
//   k_track_list_init     forward pointers = -1, piece words = -1, piece lengths = 0
//   k_track_list_next     next[i - 1][prev[i][r]] = r
//   k_track_list_walk     every head walks its chain: the rows learn their head, the head its length and whether it is listed;
//                         listed pieces and their observations summed per workgroup
//   k_track_list_offsets  one workgroup: the prefix sums of both, the cut at tracks_cap / obs_cap found to the piece, the summary
//   k_track_list_heads    the scan inside the workgroup: number, length, offset and first observation of every stored piece
//   k_track_list_obs      one lane per interior row: its observation at (offset of its head's piece) + (nodes behind the head)
// No atomics in the numbering or the packing: the order is the rows' order.
#include <hip/hip_runtime.h>

#include "brisk_common.h"
#include "brisk_kernels.h"

#define TK_ROWS 256      // rows (or records) = lanes of a workgroup of the row passes
#define TK_THREADS 1024  // the offsets workgroups

// exclusive prefix of v over the workgroup's THREADS lanes (part: THREADS / 64 words of LDS, free again on return); *total = the sum
template <int THREADS>
__device__ __forceinline__ long long tk_scan(long long v, long long* part, long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const long long u = __shfl_up(incl, off, 64);
    if (lane >= off) incl += u;
  }
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  long long base = incl - v, tot = 0;
  for (int w = 0; w < THREADS / 64; ++w) {
    const long long u = part[w];
    base += w < wave ? u : 0;
    tot += u;
  }
  __syncthreads();
  *total = tot;
  return base;
}

__device__ __forceinline__ long long tk_wave_sum(long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int tk_lim(const int* __restrict__ node_rows, long long stride, int node, int rows_cap) {
  return brisk_track_lim(node_rows[node * stride], rows_cap);
}

// ---- link ---------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(TK_ROWS) k_track_init(const int* __restrict__ node_rows, long long stride, int n0, int rows_cap,
                                                        unsigned long long* __restrict__ claims, int* __restrict__ prev,
                                                        unsigned long long* __restrict__ counters) {
  const int node = n0 + blockIdx.y, r = blockIdx.x * TK_ROWS + threadIdx.x;
  if (node == 0 && blockIdx.x == 0 && threadIdx.x < BRISK_TRACK_COUNTERS) counters[threadIdx.x] = 0;
  if (r >= tk_lim(node_rows, stride, node, rows_cap)) return;
  const long long idx = (long long)node * rows_cap + r;
  claims[idx] = BRISK_TRACK_NO_CLAIM;
  prev[idx] = -1;
}

// record j of pair p (range [o0, o1)): true and *key, *q, *t iff it is a proposal
__device__ __forceinline__ bool tk_proposal(const BriskDMatch* __restrict__ matches, long long o0, long long j, int lim_q, int lim_t,
                                            unsigned long long* key, int* q, int* t) {
  const uint4 rec = reinterpret_cast<const uint4*>(matches)[j];
  const int before = j > o0 ? matches[j - 1].queryIdx : 0;
  *q = (int)rec.x;
  *t = (int)rec.y;
  *key = brisk_track_key(rec.w, *q);
  return brisk_track_proposes(brisk_track_first_of_row(j, o0, *q, before), *q, *t, rec.w, lim_q, lim_t);
}

__global__ void __launch_bounds__(TK_ROWS) k_track_propose(const int* __restrict__ node_rows, long long stride, int p0, int rows_cap,
                                                           const long long* __restrict__ offsets, const BriskDMatch* __restrict__ matches,
                                                           unsigned long long* __restrict__ claims) {
  const int p = p0 + blockIdx.y;
  const long long o0 = offsets[p], o1 = offsets[p + 1];
  if (o0 + (long long)blockIdx.x * TK_ROWS >= o1) return;
  const int lim_t = tk_lim(node_rows, stride, p, rows_cap), lim_q = tk_lim(node_rows, stride, p + 1, rows_cap);
  for (long long j = o0 + (long long)blockIdx.x * TK_ROWS + threadIdx.x; j < o1; j += (long long)gridDim.x * TK_ROWS) {
    unsigned long long key;
    int q, t;
    if (tk_proposal(matches, o0, j, lim_q, lim_t, &key, &q, &t)) atomicMin(&claims[(long long)p * rows_cap + t], key);
  }
}

__global__ void __launch_bounds__(TK_ROWS) k_track_resolve(const int* __restrict__ node_rows, long long stride, int p0, int rows_cap,
                                                           const long long* __restrict__ offsets, const BriskDMatch* __restrict__ matches,
                                                           const unsigned long long* __restrict__ claims, int* __restrict__ prev,
                                                           unsigned long long* __restrict__ counters) {
  const int p = p0 + blockIdx.y;
  const long long o0 = offsets[p], o1 = offsets[p + 1];
  if (o0 + (long long)blockIdx.x * TK_ROWS >= o1) return;
  const int lim_t = tk_lim(node_rows, stride, p, rows_cap), lim_q = tk_lim(node_rows, stride, p + 1, rows_cap);
  long long links = 0, lost = 0, ignored = 0;
  for (long long j = o0 + (long long)blockIdx.x * TK_ROWS + threadIdx.x; j < o1; j += (long long)gridDim.x * TK_ROWS) {
    unsigned long long key;
    int q, t;
    if (!tk_proposal(matches, o0, j, lim_q, lim_t, &key, &q, &t)) {
      ++ignored;
    } else if (brisk_track_wins(claims[(long long)p * rows_cap + t], key)) {
      prev[(long long)(p + 1) * rows_cap + q] = t;
      ++links;
    } else {
      ++lost;
    }
  }
  // (integer sums: the order of the additions does not show)
  links = tk_wave_sum(links);
  lost = tk_wave_sum(lost);
  ignored = tk_wave_sum(ignored);
  if ((threadIdx.x & 63) == 0) {
    if (links) atomicAdd(&counters[BRISK_TRACK_C_LINKS], (unsigned long long)links);
    if (lost) atomicAdd(&counters[BRISK_TRACK_C_LOST], (unsigned long long)lost);
    if (ignored) atomicAdd(&counters[BRISK_TRACK_C_IGNORED], (unsigned long long)ignored);
  }
}

// whether row (node, r) - r below the node's rows - starts a track
__device__ __forceinline__ bool tk_starts(const int* __restrict__ prev, const long long* __restrict__ seed_track, int node, int r,
                                          long long idx) {
  const bool seeded = node == 0 && seed_track != nullptr;
  return brisk_track_starts(prev[idx], node, seeded, seeded ? seed_track[r] : -1);
}

__global__ void __launch_bounds__(TK_ROWS) k_track_count(const int* __restrict__ node_rows, long long stride, int n0, int rows_cap,
                                                         const int* __restrict__ prev, const long long* __restrict__ seed_track,
                                                         long long* __restrict__ blk) {
  __shared__ long long part[TK_ROWS / 64];
  const int node = n0 + blockIdx.y, r = blockIdx.x * TK_ROWS + threadIdx.x;
  const int lim = tk_lim(node_rows, stride, node, rows_cap);
  const long long idx = (long long)node * rows_cap + r;
  long long total;
  tk_scan<TK_ROWS>(r < lim && tk_starts(prev, seed_track, node, r, idx) ? 1 : 0, part, &total);
  if (threadIdx.x == 0) blk[(long long)node * gridDim.x + blockIdx.x] = total;
}

// blk [nblk] -> exclusive prefix sums in place; words[0] = first_new (read BEFORE the summary is written: d_first_new may be the
// summary's own first word, one call feeding the next)
__global__ void __launch_bounds__(TK_THREADS) k_track_offsets(long long* blk, long long nblk, const int* __restrict__ node_rows,
                                                              long long stride, int nodes, int rows_cap, long long first_new,
                                                              const long long* d_first_new, const unsigned long long* __restrict__ counters,
                                                              long long* __restrict__ words, long long* summary) {
  __shared__ long long part[TK_THREADS / 64];
  const int tid = threadIdx.x;
  const long long per = (nblk + TK_THREADS - 1) / TK_THREADS;
  const long long i0 = min(tid * per, nblk), i1 = min(i0 + per, nblk);
  long long sum = 0, obs = 0, started, observations;
  for (long long i = i0; i < i1; ++i) sum += blk[i];
  for (int n = tid; n < nodes; n += TK_THREADS) obs += tk_lim(node_rows, stride, n, rows_cap);
  long long base = tk_scan<TK_THREADS>(sum, part, &started);
  tk_scan<TK_THREADS>(obs, part, &observations);
  for (long long i = i0; i < i1; ++i) {
    const long long v = blk[i];
    blk[i] = base;
    base += v;
  }
  if (tid == 0) {
    const long long first = d_first_new ? *d_first_new : first_new;
    const long long links = (long long)counters[BRISK_TRACK_C_LINKS], lost = (long long)counters[BRISK_TRACK_C_LOST],
                    ignored = (long long)counters[BRISK_TRACK_C_IGNORED];
    words[0] = first;
    summary[0] = first + started;
    summary[1] = started;
    summary[2] = links;
    summary[3] = lost;
    summary[4] = ignored;
    summary[5] = observations;
    summary[6] = 0;
    summary[7] = 0;
  }
}

__global__ void __launch_bounds__(TK_ROWS) k_track_number(const int* __restrict__ node_rows, long long stride, int n0, int nodes, int rows_cap,
                                                          const int* __restrict__ prev, const unsigned long long* __restrict__ claims,
                                                          const long long* __restrict__ seed_track, const int* __restrict__ seed_age,
                                                          const long long* __restrict__ blk, const long long* __restrict__ words,
                                                          long long* __restrict__ track, int* __restrict__ age) {
  __shared__ long long part[TK_ROWS / 64];
  int node = n0 + blockIdx.y;
  const int r = blockIdx.x * TK_ROWS + threadIdx.x;
  const int lim = tk_lim(node_rows, stride, node, rows_cap);
  if ((int)blockIdx.x * TK_ROWS >= lim) return;
  long long idx = (long long)node * rows_cap + r;
  const bool head = r < lim && brisk_track_is_head(prev[idx]);
  const bool starts = r < lim && tk_starts(prev, seed_track, node, r, idx);
  long long total;
  const long long rank = tk_scan<TK_ROWS>(starts ? 1 : 0, part, &total);
  if (!head) return;
  long long id;
  int a = 0;
  if (starts) {
    id = words[0] + blk[(long long)node * gridDim.x + blockIdx.x] + rank;
  } else {  // a seeded head of node 0
    id = seed_track[r];
    a = seed_age[r];
  }
  // the walk: the claim word of a row names the row of the next node that won it
  for (;;) {
    track[idx] = id;
    age[idx] = a;
    if (node + 1 >= nodes) break;
    const int q = brisk_track_next_row(claims[idx]);
    if (q < 0 || q >= rows_cap) break;  // (a claim holds a query row below its node's rows: the second test never fires)
    ++node;
    ++a;
    idx = (long long)node * rows_cap + q;
  }
}

void brisk_launch_track_link(const int* node_rows, long long stride, int nodes, int rows_cap, const long long* offsets, const BriskDMatch* matches,
                             const long long* seed_track, const int* seed_age, long long first_new, const long long* d_first_new,
                             unsigned long long* claims, long long* blk, unsigned long long* counters, long long* words, int* prev,
                             long long* track, int* age, long long* summary, hipStream_t s) {
  const int bpn = brisk_track_blocks_per_node(rows_cap);
  // grid (workgroups per node, nodes), 65535 nodes at a time (what grid.y holds)
  for (int n0 = 0; n0 < nodes; n0 += 65535)
    hipLaunchKernelGGL(k_track_init, dim3(bpn, min(65535, nodes - n0)), dim3(TK_ROWS), 0, s, node_rows, stride, n0, rows_cap, claims, prev,
                       counters);
  for (int p0 = 0; p0 < nodes - 1; p0 += 65535)
    hipLaunchKernelGGL(k_track_propose, dim3(bpn, min(65535, nodes - 1 - p0)), dim3(TK_ROWS), 0, s, node_rows, stride, p0, rows_cap, offsets,
                       matches, claims);
  for (int p0 = 0; p0 < nodes - 1; p0 += 65535)
    hipLaunchKernelGGL(k_track_resolve, dim3(bpn, min(65535, nodes - 1 - p0)), dim3(TK_ROWS), 0, s, node_rows, stride, p0, rows_cap, offsets,
                       matches, claims, prev, counters);
  for (int n0 = 0; n0 < nodes; n0 += 65535)
    hipLaunchKernelGGL(k_track_count, dim3(bpn, min(65535, nodes - n0)), dim3(TK_ROWS), 0, s, node_rows, stride, n0, rows_cap, prev, seed_track,
                       blk);
  hipLaunchKernelGGL(k_track_offsets, dim3(1), dim3(TK_THREADS), 0, s, blk, (long long)nodes * bpn, node_rows, stride, nodes, rows_cap, first_new,
                     d_first_new, counters, words, summary);
  for (int n0 = 0; n0 < nodes; n0 += 65535)
    hipLaunchKernelGGL(k_track_number, dim3(bpn, min(65535, nodes - n0)), dim3(TK_ROWS), 0, s, node_rows, stride, n0, nodes, rows_cap, prev,
                       claims, seed_track, seed_age, blk, words, track, age);
}

// ---- list ---------------------------------------------------------------------------------------------------------------------
// piece [nodes][rows_cap] long long: an interior row's head (node * rows_cap + row) once k_track_list_walk has reached it; a head's
// own word: its piece's length (the age of its last row + 1) until k_track_list_heads replaces it by the piece's offset (-1 = not stored)

__global__ void __launch_bounds__(TK_ROWS) k_track_list_init(const int* __restrict__ node_rows, long long stride, int n0, int rows_cap,
                                                             int* __restrict__ next, int* __restrict__ len, long long* __restrict__ piece) {
  const int node = n0 + blockIdx.y, r = blockIdx.x * TK_ROWS + threadIdx.x;
  if (r >= tk_lim(node_rows, stride, node, rows_cap)) return;
  const long long idx = (long long)node * rows_cap + r;
  next[idx] = -1;
  len[idx] = 0;
  piece[idx] = -1;
}

__global__ void __launch_bounds__(TK_ROWS) k_track_list_next(const int* __restrict__ node_rows, long long stride, int n0, int rows_cap,
                                                             const int* __restrict__ prev, int* __restrict__ next) {
  const int node = n0 + blockIdx.y, r = blockIdx.x * TK_ROWS + threadIdx.x;  // (n0 >= 1: node 0 has no predecessor)
  if (r >= tk_lim(node_rows, stride, node, rows_cap)) return;
  const int t = prev[(long long)node * rows_cap + r];
  if (t >= 0 && t < tk_lim(node_rows, stride, node - 1, rows_cap)) next[(long long)(node - 1) * rows_cap + t] = r;
}

__global__ void __launch_bounds__(TK_ROWS) k_track_list_walk(const int* __restrict__ node_rows, long long stride, int n0, int nodes,
                                                             int rows_cap, const int* __restrict__ prev, const int* __restrict__ age,
                                                             const int* __restrict__ next, int min_len, int* __restrict__ len,
                                                             long long* __restrict__ piece, long long* __restrict__ blk_pieces,
                                                             long long* __restrict__ blk_obs) {
  __shared__ long long part[TK_ROWS / 64];
  const int node = n0 + blockIdx.y, r = blockIdx.x * TK_ROWS + threadIdx.x;
  const long long blk = (long long)node * gridDim.x + blockIdx.x;
  const int lim = tk_lim(node_rows, stride, node, rows_cap);
  if ((int)blockIdx.x * TK_ROWS >= lim) {
    if (threadIdx.x == 0) { blk_pieces[blk] = 0; blk_obs[blk] = 0; }
    return;
  }
  const long long head = (long long)node * rows_cap + r;
  int n = 0;
  if (r < lim && brisk_track_is_head(prev[head])) {
    long long idx = head;
    int at = node;
    n = 1;
    while (at + 1 < nodes) {
      const int q = next[idx];
      if (q < 0) break;  // (next holds rows below their node's rows only: k_track_list_next)
      ++at;
      ++n;
      idx = (long long)at * rows_cap + q;
      piece[idx] = head;
    }
    const int last_age = age[idx];
    piece[head] = (long long)last_age + 1;
    if (!brisk_track_listed(last_age, min_len)) n = 0;
    len[head] = n;
  }
  long long pieces, obs;
  tk_scan<TK_ROWS>(n > 0 ? 1 : 0, part, &pieces);
  tk_scan<TK_ROWS>(n, part, &obs);
  if (threadIdx.x == 0) { blk_pieces[blk] = pieces; blk_obs[blk] = obs; }
}

// both arrays of workgroup sums -> exclusive prefix sums in place.  The first piece that does not fit tracks_cap or obs_cap is cut
// with every piece behind it: the prefixes grow, so it lies in the first workgroup whose END does not fit, and that workgroup's
// rows are scanned here once more.  words[0] = pieces stored, words[1] = observations stored.
__global__ void __launch_bounds__(TK_THREADS) k_track_list_offsets(long long* blk_pieces, long long* blk_obs, long long nblk, int bpn,
                                                                   const int* __restrict__ node_rows, long long stride, int rows_cap,
                                                                   const int* __restrict__ len, long long tracks_cap, long long obs_cap,
                                                                   long long* __restrict__ words, long long* __restrict__ summary,
                                                                   long long* __restrict__ list_offsets) {
  __shared__ long long part[TK_THREADS / 64];
  __shared__ long long red[TK_THREADS / 64];
  __shared__ long long cut[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long per = (nblk + TK_THREADS - 1) / TK_THREADS;
  const long long i0 = min(tid * per, nblk), i1 = min(i0 + per, nblk);
  long long sp = 0, so = 0, pieces, obs;
  for (long long i = i0; i < i1; ++i) { sp += blk_pieces[i]; so += blk_obs[i]; }
  long long bp = tk_scan<TK_THREADS>(sp, part, &pieces);
  long long bo = tk_scan<TK_THREADS>(so, part, &obs);
  long long cutb = nblk;
  for (long long i = i0; i < i1; ++i) {
    const long long vp = blk_pieces[i], vo = blk_obs[i];
    blk_pieces[i] = bp;
    blk_obs[i] = bo;
    bp += vp;
    bo += vo;
    if (vp > 0 && (bp > tracks_cap || bo > obs_cap)) cutb = min(cutb, i);
  }
  for (int off = 32; off > 0; off >>= 1) cutb = min(cutb, __shfl_xor(cutb, off, 64));
  if (lane == 0) red[wave] = cutb;
  __syncthreads();  // (and the prefixes of all workgroups are in place)
  for (int w = 0; w < TK_THREADS / 64; ++w) cutb = min(cutb, red[w]);
  long long stored = pieces, stored_obs = obs;
  if (cutb < nblk) {  // (the same for every lane)
    const int node = (int)(cutb / bpn), r = (int)(cutb % bpn) * TK_ROWS + tid;
    const int n = tid < TK_ROWS && r < tk_lim(node_rows, stride, node, rows_cap) ? len[(long long)node * rows_cap + r] : 0;
    long long t;
    const long long rank = blk_pieces[cutb] + tk_scan<TK_THREADS>(n > 0 ? 1 : 0, part, &t);
    const long long off = blk_obs[cutb] + tk_scan<TK_THREADS>(n, part, &t);
    const bool fails = n > 0 && (rank + 1 > tracks_cap || off + n > obs_cap);
    // the first lane that fails (rows are in lane order): ballots of the waves, in wave order
    const unsigned long long b = __ballot(fails);
    if (lane == 0) red[wave] = b ? (long long)(wave * 64 + __ffsll((long long)b) - 1) : (long long)TK_THREADS;
    __syncthreads();
    long long firstlane = TK_THREADS;
    for (int w = 0; w < TK_THREADS / 64; ++w) firstlane = min(firstlane, red[w]);
    if (tid == firstlane) { cut[0] = rank; cut[1] = off; }
    __syncthreads();
    stored = cut[0];
    stored_obs = cut[1];
  }
  if (tid == 0) {
    words[0] = stored;
    words[1] = stored_obs;
    summary[0] = pieces;
    summary[1] = obs;
    summary[2] = stored;
    summary[3] = stored < pieces ? BRISK_TRACK_LIST_CUT : 0;
    list_offsets[stored] = stored_obs;
  }
}

__global__ void __launch_bounds__(TK_ROWS) k_track_list_heads(const int* __restrict__ node_rows, long long stride, int n0, int rows_cap,
                                                              const int* __restrict__ prev, const long long* __restrict__ track,
                                                              const int* __restrict__ len, const long long* __restrict__ blk_pieces,
                                                              const long long* __restrict__ blk_obs, const long long* __restrict__ words,
                                                              long long* __restrict__ piece, long long* __restrict__ list_track,
                                                              int* __restrict__ list_len, long long* __restrict__ list_offsets,
                                                              int2* __restrict__ list_obs) {
  __shared__ long long part[TK_ROWS / 64];
  const int node = n0 + blockIdx.y, r = blockIdx.x * TK_ROWS + threadIdx.x;
  const long long blk = (long long)node * gridDim.x + blockIdx.x;
  const int lim = tk_lim(node_rows, stride, node, rows_cap);
  if ((int)blockIdx.x * TK_ROWS >= lim) return;
  const long long idx = (long long)node * rows_cap + r;
  const bool head = r < lim && brisk_track_is_head(prev[idx]);
  const int n = head ? len[idx] : 0;
  long long t;
  const long long rank = blk_pieces[blk] + tk_scan<TK_ROWS>(n > 0 ? 1 : 0, part, &t);
  const long long off = blk_obs[blk] + tk_scan<TK_ROWS>(n, part, &t);
  if (!head) return;
  if (n > 0 && rank < words[0] && off + n <= words[1]) {  // (the second test is the first's: both hold for a stored piece)
    list_track[rank] = track[idx];
    list_len[rank] = (int)piece[idx];
    list_offsets[rank] = off;
    list_obs[off] = make_int2(node, r);
    piece[idx] = off;
  } else {
    piece[idx] = -1;
  }
}

__global__ void __launch_bounds__(TK_ROWS) k_track_list_obs(const int* __restrict__ node_rows, long long stride, int n0, int rows_cap,
                                                            const int* __restrict__ prev, const long long* __restrict__ piece,
                                                            const long long* __restrict__ words, long long cells, int2* __restrict__ list_obs) {
  const int node = n0 + blockIdx.y, r = blockIdx.x * TK_ROWS + threadIdx.x;  // (n0 >= 1: the rows of node 0 are heads)
  if (r >= tk_lim(node_rows, stride, node, rows_cap)) return;
  const long long idx = (long long)node * rows_cap + r;
  if (brisk_track_is_head(prev[idx])) return;
  const long long head = piece[idx];
  if (head < 0 || head >= cells) return;  // (a row no head's walk reached: a prev that names no row)
  const long long off = piece[head];
  if (off < 0) return;                    // (its piece is not stored)
  const long long pos = off + (node - head / rows_cap);
  if (pos >= off && pos < words[1]) list_obs[pos] = make_int2(node, r);
}

int brisk_track_blocks_per_node(int rows_cap) { return (rows_cap + TK_ROWS - 1) / TK_ROWS; }

void brisk_launch_track_list(const int* node_rows, long long stride, int nodes, int rows_cap, const int* prev, const long long* track,
                             const int* age, int min_len, long long tracks_cap, long long obs_cap, int* next, int* len, long long* piece,
                             long long* blk_pieces, long long* blk_obs, long long* words, long long* list_track, int* list_len,
                             long long* list_offsets, void* list_obs, long long* summary, hipStream_t s) {
  const int bpn = brisk_track_blocks_per_node(rows_cap);
  int2* obs = static_cast<int2*>(list_obs);
  for (int n0 = 0; n0 < nodes; n0 += 65535)
    hipLaunchKernelGGL(k_track_list_init, dim3(bpn, min(65535, nodes - n0)), dim3(TK_ROWS), 0, s, node_rows, stride, n0, rows_cap, next, len,
                       piece);
  for (int n0 = 1; n0 < nodes; n0 += 65535)
    hipLaunchKernelGGL(k_track_list_next, dim3(bpn, min(65535, nodes - n0)), dim3(TK_ROWS), 0, s, node_rows, stride, n0, rows_cap, prev, next);
  for (int n0 = 0; n0 < nodes; n0 += 65535)
    hipLaunchKernelGGL(k_track_list_walk, dim3(bpn, min(65535, nodes - n0)), dim3(TK_ROWS), 0, s, node_rows, stride, n0, nodes, rows_cap, prev,
                       age, next, min_len, len, piece, blk_pieces, blk_obs);
  hipLaunchKernelGGL(k_track_list_offsets, dim3(1), dim3(TK_THREADS), 0, s, blk_pieces, blk_obs, (long long)nodes * bpn, bpn, node_rows, stride,
                     rows_cap, len, tracks_cap, obs_cap, words, summary, list_offsets);
  for (int n0 = 0; n0 < nodes; n0 += 65535)
    hipLaunchKernelGGL(k_track_list_heads, dim3(bpn, min(65535, nodes - n0)), dim3(TK_ROWS), 0, s, node_rows, stride, n0, rows_cap, prev, track,
                       len, blk_pieces, blk_obs, words, piece, list_track, list_len, list_offsets, obs);
  for (int n0 = 1; n0 < nodes; n0 += 65535)
    hipLaunchKernelGGL(k_track_list_obs, dim3(bpn, min(65535, nodes - n0)), dim3(TK_ROWS), 0, s, node_rows, stride, n0, rows_cap, prev, piece,
                       words, (long long)nodes * rows_cap, obs);
}
