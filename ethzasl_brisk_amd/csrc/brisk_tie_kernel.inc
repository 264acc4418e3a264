// brisk_tie_kernel.inc - body of k_tie_resolve, included three times by brisk_kernels.hip (TR_KERNEL_NAME, TR_KERNEL_MASKS,
// TR_KERNEL_PAIR = two ties per wave, round 5):
// the large-batch form must stay at 96 VGPRs at most (see there), which the precomputed-mask form of the static step exceeds.
__device__ __noinline__ void TR_SORT_NAME(const BriskCand* C, int* list, int n, int h, unsigned* gkey, unsigned* gci, unsigned* pool,
                                            unsigned* wsum) {
  const int tid = threadIdx.x, nthreads = blockDim.x, wave = tid >> 6, lane = tid & 63;
  unsigned* cnt32 = pool;            // [4096]
  unsigned* rowstart = pool + 4096;  // [8192]
  int* wlist = list;
  #pragma unroll 1
  for (int i = tid; i < 4096; i += nthreads) cnt32[i] = 0;
  __syncthreads();
  #pragma unroll 1
  for (int j = tid; j < n; j += nthreads) {
    const unsigned y = (C[list[j]].key >> 13) & 0x1FFFu;
    atomicAdd(&cnt32[y >> 1], (y & 1) ? 0x10000u : 1u);
  }
  __syncthreads();
  {  // exclusive prefix over the 8192 rows: a contiguous stretch of rows per thread, wave scan, wave totals
    const int rpt = (8192 + nthreads - 1) / nthreads;
    const int r0 = min(tid * rpt, 8192), r1 = min(r0 + rpt, 8192);
    unsigned local = 0;
    #pragma unroll 1
    for (int r = r0; r < r1; ++r) local += (cnt32[r >> 1] >> (16 * (r & 1))) & 0xFFFFu;
    const unsigned incl = (unsigned)wave_inclusive_scan((int)local);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned base = incl - local;
    #pragma unroll 1
    for (int q = 0; q < wave; ++q) base += wsum[q];
    #pragma unroll 1
    for (int r = r0; r < r1; ++r) {
      rowstart[r] = base;
      base += (cnt32[r >> 1] >> (16 * (r & 1))) & 0xFFFFu;
    }
  }
  __syncthreads();
  #pragma unroll 1
  for (int i = tid; i < 4096; i += nthreads) cnt32[i] = 0;
  __syncthreads();
  #pragma unroll 1
  for (int j = tid; j < n; j += nthreads) {
    const int ci = list[j];
    const unsigned key = C[ci].key;
    const unsigned y = (key >> 13) & 0x1FFFu;
    const unsigned old = atomicAdd(&cnt32[y >> 1], (y & 1) ? 0x10000u : 1u);
    const unsigned pos = rowstart[y] + ((old >> (16 * (y & 1))) & 0xFFFFu);
    gkey[pos] = key;
    gci[pos] = (unsigned)ci;
  }
  // (the buckets are read by other waves of this workgroup: stores acknowledged, then the barrier; L1-bypassing loads)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  #pragma unroll 1
  for (int y = wave; y < h; y += (nthreads >> 6)) {
    const int b0 = (int)rowstart[y], nb = (int)((cnt32[y >> 1] >> (16 * (y & 1))) & 0xFFFFu);
    #pragma unroll 1
    for (int e0 = 0; e0 < nb; e0 += 64) {
      const bool mine = e0 + lane < nb;
      const unsigned myk = mine ? __hip_atomic_load(&gkey[b0 + e0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      const int ci = mine ? (int)__hip_atomic_load(&gci[b0 + e0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
      int r = 0;
      #pragma unroll 1
      for (int i0 = 0; i0 < nb; i0 += 64) {  // 64 keys of the bucket per load, handed round by lane broadcasts
        const unsigned kk = (i0 + lane < nb) ? __hip_atomic_load(&gkey[b0 + i0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xFFFFFFFFu;
#pragma unroll 8
        for (int t = 0; t < 64; ++t) r += ((unsigned)__builtin_amdgcn_readlane((int)kk, t) < myk) ? 1 : 0;
      }
      // (read by the workgroup of the layer above, possibly on another XCD: through memory, like the score-state map)
      if (mine) __hip_atomic_store(&wlist[b0 + r], ci, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

__global__ void __launch_bounds__(TR_THREADS) TR_KERNEL_NAME(BriskGeom G, uint8_t* pyr, uint16_t* smap, BriskCand* cand,
                                                             BriskFrameCounters* counters, const int* tie_idx,
                                                             const uint8_t* blocks, unsigned* gscratch, int cand_cap,
                                                             int tie_cap, int nframes, int lpw, int persist, int pair_min, int nbands) {
  BRISK_CHAIN_SETPRIO();
  constexpr int masks = TR_KERNEL_MASKS;
  constexpr int TR_NW = TR_KERNEL_PAIR ? 2 : 1;  // ties a wave decides at a time (one per half wave in the pair form)
  __shared__ uint8_t kp5s[TR_WAVES * TR_NW][32];
  __shared__ uint16_t win[TR_WAVES * TR_NW][TR_WIN * TR_WIN + 1];  // per-wave window(s) of the tie(s) being decided
  // the four TR_CHUNK-sized arrays as ONE block of LDS: the raster sort of a layer beyond the on-chip capacity
  // (tie_sort_large) uses all of it for its row tables (4096 words of row counters + 8192 row offsets) before any of
  // them holds live data
  constexpr int TR_SK = TR_CHUNK > TR_THREADS ? TR_CHUNK : TR_THREADS;
  struct TiePool {
    unsigned skey[TR_SK];
    int sorder[TR_CHUNK];      // candidate index of the tie with raster rank r
    unsigned sxyd[TR_CHUNK];   // its key (layer, y, x)
    int vals_ci[TR_CHUNK];     // candidate index of the tie (unsorted order)
    unsigned pad[(TR_SK + 3 * TR_CHUNK) < 12288 ? 12288 - (TR_SK + 3 * TR_CHUNK) : 1];
  };
  __shared__ TiePool tp;
  __shared__ unsigned wsum[TR_WAVES];
  unsigned (&skey)[TR_SK] = tp.skey;
  int (&sorder)[TR_CHUNK] = tp.sorder;
  unsigned (&sxyd)[TR_CHUNK] = tp.sxyd;
  unsigned* const pool = reinterpret_cast<unsigned*>(&tp);
  __shared__ int vals[TR_WAVES * TR_NW][40];
  int (&vals_ci)[TR_CHUNK] = tp.vals_ci;
  __shared__ __attribute__((aligned(16))) uint16_t sfpm[TR_CHUNK];   // e3 footprint mask of the tie with raster rank r
  // (pair form) first rank of the chunk in row y - 4 or below it, y the row of rank r: where the search for pending ties of its
  // window starts; during the raster sort: next member of the same row bucket
#if TR_KERNEL_MASKS
  __shared__ uint16_t sback[TR_CHUNK];
#endif
  __shared__ __attribute__((aligned(16))) uint16_t sneed[TR_CHUNK];  // rows of the layer below the tie with raster rank r waits for (brisk_tie_rows_needed; 0 = none)
  __shared__ unsigned below_bm[TR_BM_WORDS];  // cells of this layer that a tie of the layer below can touch
  __shared__ int ticket_s, abort_s, seen_s, nsel_s;
  (void)&nsel_s;
  int* const tstat = reinterpret_cast<int*>(skey);               // after the sort: decision of rank r (0 = pending)
  unsigned* const sfpxy = reinterpret_cast<unsigned*>(vals_ci);  // after the sort: footprint anchor of rank r
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nthreads = blockDim.x, dwaves = (nthreads >> 6) - 1;  // deciding waves; the last wave writes the decisions to memory
  // the lane's slot of the cache replay (lanes 0-7: the 8 probe values, lanes 32-56: the 5x5 raw block) and which of the
  // slot pixel's 24 neighbours can act on it: constants of the lane (brisk_state_masks)
#if TR_KERNEL_PAIR
  // pair form: every half wave holds one tie's 32 slots - the 8 probes and the 24 block pixels around the centre (the
  // centre's raw value is the candidate's own D: no replay)
  const int tslot = ((lane & 31) < 8) ? (lane & 31) : ((lane & 31) < 20 ? (lane & 31) : (lane & 31) + 1);
#else
  const int tslot = (lane < 8) ? lane : (lane >= 32 && lane < 57) ? lane - 24 : -1;
#endif
  // (one register: bits 0-24 the act mask, bits 25-29 the index of the neighbour that is the candidate itself, 31 = none)
  unsigned tam = 0;
  if (masks && tslot >= 0) {
    int tsx, tsy;
    bool town;
    unsigned am, ns;
    brisk_tie_slot_offset(tslot, &tsx, &tsy, &town);
    brisk_state_masks(tsx, tsy, town, &am, &ns);
    const unsigned notself = ~ns & 0x1FFEFFFu;  // (bit 12 is the pixel itself: never a neighbour)
    tam = am | ((notself ? (unsigned)(31 - __builtin_clz(notself)) : 31u) << 25);
  }
  const int nl = G.nlayers;
  const int ngroups = (nl + lpw - 1) / lpw;  // tickets per frame, `lpw` consecutive layers each
  // Row bands (pair form, calls of one or two frames, one layer per ticket): a layer's ties are dealt to nbands workgroups by
  // image row - a frame is ready in the time of its largest layer, and that layer's 30 decisions in flight are what bounds it.  Band b
  // only ever waits for band b - 1 (a pending tie of its window above its first row: read from the score-state map, where the other
  // band's writer wave puts the decision) and for the layer below; tickets are (layer, band) in ascending order.
  const int nb_k = (TR_KERNEL_PAIR && lpw == 1) ? min(max(nbands, 1), BRISK_TIE_MAX_BANDS) : 1;
  const int tpf = ngroups * nb_k;  // tickets per frame
  // persist: the grid is one workgroup per CU and a workgroup draws ticket after ticket (frames whose layers differ a lot
  // in ties - 4K: 23 ... 1026 per layer - then balance by themselves; a ticket still only waits for tickets drawn before it)
  for (;;) {
  __syncthreads();  // (the previous ticket's use of the on-chip arrays and of ticket_s is over)
  if (tid == 0) {
    abort_s = 0;
    if (nframes >= 8) {  // one ticket counter per XCD residue: frames g * 8 + xcd, layer groups in ascending order
      const int xcd = blockIdx.x & 7;
      const int t = atomicAdd(&counters[xcd].tie_ticket, 1);
      ticket_s = ((t / tpf) * 8 + xcd) * tpf + t % tpf;
    } else {
      ticket_s = atomicAdd(&counters[0].tie_ticket, 1);
    }
  }
  __syncthreads();
  const int frame = ticket_s / tpf, l0 = ((ticket_s % tpf) / nb_k) * lpw, l1 = min(l0 + lpw, nl), band = (ticket_s % tpf) % nb_k;
  if (frame >= nframes) return;
  if (counters[frame].low_score) {  // the frame runs the ordered path: nothing to resolve, nobody waits for this ticket
    if (!persist) return;
    continue;
  }
  const BriskCand* C = cand + (long)frame * cand_cap;
  // a frame whose candidate or tie list overflowed is reported as an error and its result discarded; its map holds
  // tie candidates that are in no list, which nobody would ever decide: do not wait for them
  const bool skip_frame = (counters[frame].overflow & 3) != 0;
  // Safety net of the waits below (a wait that cannot end must not hang the GPU): a wait may legitimately last as long
  // as all raster-earlier work of the frame - a frame of 150 k ties that all depend on each other decides one tie per
  // 4 us, and the layer above waits at its front for most of that -, so the bound is 0.5 s + 20 us per tie of the frame
  // on the 100 MHz wall clock, not a spin count.
  long long wait_budget = 50000000ll;
  for (int q = 0; q < nl; ++q) {
    const long long nq = min(counters[frame].ntie[q], tie_cap);
    wait_budget += nq * 2000ll;
    // (a layer beyond the on-chip capacity is first put into raster order through global scratch: O(n), at most a
    // row's width of steps per tie)
    if (nq > TR_CHUNK) wait_budget += nq * 2000ll;
  }
  for (int l = l0; l < l1; ++l) {
  int* const my_prog = (band == 0) ? &counters[frame].tie_prog[l] : &counters[frame].tie_prog_b[l * (BRISK_TIE_MAX_BANDS - 1) + band - 1];
  const int n_all = min(counters[frame].ntie[l], tie_cap);
  // (a layer beyond the on-chip capacity is not cut: band 0 takes all of it, the others report done)
  const bool banded = nb_k > 1 && n_all <= TR_CHUNK;
  const int rows_pb = (G.L[l].h + nb_k - 1) / nb_k;
  const int y0b = banded ? band * rows_pb : 0, y1b = banded ? y0b + rows_pb : 0x7FFFFFFF;  // this workgroup's rows of the layer
  (void)y1b;
  int n = n_all;
  TR_STAMP(tid == 0, l, 0)
  __syncthreads();  // (the previous layer's use of the on-chip arrays is over)
  if (n == 0 || skip_frame || (!banded && band > 0)) {
    if (tid == 0) __hip_atomic_fetch_max(my_prog, TR_PROG_DONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    continue;
  }
  if (n > TR_CHUNK) {
    // raster order in O(n) through global scratch (this layer's share: the ties of all layers together are at most the
    // candidates), before the per-layer state below is built: the tie kernel must stay at 104 VGPRs
    int off = 0;
    for (int q = 0; q < l; ++q) off += min(counters[frame].ntie[q], tie_cap);
    unsigned* gk = gscratch + (long)frame * cand_cap * 2 + off;
    TR_SORT_NAME(C, const_cast<int*>(tie_idx + ((long)frame * BRISK_MAX_LAYERS + l) * tie_cap), n, G.L[l].h, gk, gk + cand_cap, pool, wsum);
    // the list was rewritten in place: the workgroup of the layer above reads it (for its bitmap) only after this flag
    if (tid == 0) __hip_atomic_fetch_or(&counters[frame].tie_sorted, 1 << l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0) { seen_s = 0; nsel_s = 0; }
  const BriskLayerView L = make_view(G, pyr, smap, frame, l);
  const bool last = (l == nl - 1);
  const bool float_patch = last || G.single_layer;
  const bool touch2x2 = last && !G.single_layer;
  const int* list = tie_idx + ((long)frame * BRISK_MAX_LAYERS + l) * tie_cap;
  // the layer below is either this workgroup's previous layer (complete) or another workgroup's (in progress)
  const bool below_elsewhere = (l == l0) && (l > 0);
  const int* below_prog = below_elsewhere ? &counters[frame].tie_prog[l - 1] : nullptr;
  // (the layer below in bands: its progress is that of its first band that is not done, and at least that band's first row)
  const bool below_banded = below_elsewhere && nb_k > 1 && min(counters[frame].ntie[l > 0 ? l - 1 : 0], tie_cap) <= TR_CHUNK;
  const int rows_pb_below = (G.L[l > 0 ? l - 1 : 0].h + nb_k - 1) / nb_k;
  int below_band = 0;  // (wave-uniform, monotone)
  const bool below_is_octave = ((l - 1) & 1) == 0;
  int seen = below_elsewhere ? 0 : TR_PROG_DONE;  // last observed progress of the layer below (wave-uniform, monotone)
  // Most ties do not depend on the layer below at all: only a tie of the layer below that passes touches this layer,
  // and only inside its 4x4 footprint.  A coarse bitmap of this layer's cells within reach of such a footprint (the
  // tie's 5x5 block is 2 pixels wide on each side) tells which ties have to wait for the layer below.
  int bm_shift = 3;
  while (((L.w >> bm_shift) + 1) * ((L.h >> bm_shift) + 1) > TR_BM_WORDS * 32) ++bm_shift;
  const int bm_w = (L.w >> bm_shift) + 1;
  if (below_elsewhere) {
    for (int i = tid; i < TR_BM_WORDS; i += nthreads) below_bm[i] = 0;
    __syncthreads();
    const int nb = min(counters[frame].ntie[l - 1], tie_cap);
    const int* listb = tie_idx + ((long)frame * BRISK_MAX_LAYERS + l - 1) * tie_cap;
    if (nb > TR_CHUNK) {  // that list is rewritten in raster order by its workgroup (tie_sort_large): not before it is done
      long long t0 = 0;
      for (int spin = 0; !(__hip_atomic_load(&counters[frame].tie_sorted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (1 << (l - 1))); ++spin) {
        if (__hip_atomic_load(&abort_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
        __builtin_amdgcn_s_sleep(8);
        if ((spin & 255) == 255) {
          const long long now = (long long)wall_clock64();
          if (!t0) t0 = now;
          else if (now - t0 > wait_budget) { __hip_atomic_store(&abort_s, 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break; }
        }
      }
    }
    for (int j = tid; j < nb; j += nthreads) {
      const BriskCand* c = &C[__hip_atomic_load(&listb[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)];
      if (!c->fp_mask) continue;
      const int x0 = max((int)c->fp_x0 - 2, 0) >> bm_shift, x1 = min((int)c->fp_x0 + 5, L.w - 1) >> bm_shift;
      const int y0 = max((int)c->fp_y0 - 2, 0) >> bm_shift, y1 = min((int)c->fp_y0 + 5, L.h - 1) >> bm_shift;
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) atomicOr(&below_bm[(y * bm_w + x) >> 5], 1u << ((y * bm_w + x) & 31));
    }
    // (the barriers of the sort below order the bitmap before its first use)
  }

  // ---- raster order of the layer's ties
  const bool on_chip = n <= TR_CHUNK;
#if !TR_KERNEL_MASKS || defined(TR_OLD_SORT)
  // (the large-batch form keeps the count-all ranking: its layers are small where batches are large, and the bucket form's
  // extra scalar state takes it from 96 to 109 VGPRs - SGPR spill lanes - which it cannot afford, see brisk_kernels.hip)
  if (on_chip) {
    for (int j = tid; j < n; j += nthreads) {
      const int ci = list[j];
      vals_ci[j] = ci;
      skey[j] = C[ci].key;
    }
    __syncthreads();
    for (int j = tid; j < n; j += nthreads) {
      const unsigned k = skey[j];
      int r = 0;
      for (int q = 0; q < n; ++q) r += (skey[q] < k) ? 1 : 0;
      sorder[r] = vals_ci[j];
      sxyd[r] = k;
    }
    __syncthreads();
  }
#else
  if (on_chip) {
    // Rank of a key = keys of smaller row buckets + smaller keys of its own bucket, whose members hang on a linked list
    // (round 5, as in k_finalize: counting ALL smaller keys per key took n LDS reads per thread - 58 of the 290 us of one
    // 4K frame's largest layer, 1 026 ties, were spent before its first decision).  The bucket tables borrow the arrays
    // that only hold live data after the sort.
    constexpr int TR_NB = TR_CHUNK >= 2048 ? 1024 : TR_CHUNK >= 1024 ? 512 : TR_CHUNK >= 256 ? 128 : 32;
    int* const bhead = reinterpret_cast<int*>(sneed);   // [TR_NB] last member of the bucket (-1: empty)
    int* const bstart = reinterpret_cast<int*>(sfpm);   // [TR_NB] members, then keys in smaller buckets
    uint16_t* const bnext = sback;                      // next member of the same bucket (0xFFFF: none)
    static_assert(TR_CHUNK * sizeof(uint16_t) >= TR_NB * sizeof(int), "bucket tables");
    #pragma unroll 1
    for (int b = tid; b < TR_NB; b += nthreads) { bhead[b] = -1; bstart[b] = 0; }
    if (banded) __syncthreads();  // (nsel_s = 0 is visible)
    #pragma unroll 1
    for (int j = tid; j < n_all; j += nthreads) {
      const int ci = list[j];
      const unsigned key = C[ci].key;
      int pos = j;
      if (banded) {  // this band's ties only (in any order: they are ranked below)
        const int y = (int)((key >> 13) & 0x1FFF);
        pos = (y >= y0b && y < y1b) ? atomicAdd(&nsel_s, 1) : -1;
      }
      if (pos >= 0) { vals_ci[pos] = ci; skey[pos] = key; }
    }
    int shift = 0;
    #pragma unroll 1
    while ((G.L[l].h >> shift) >= TR_NB) ++shift;
    __syncthreads();
    if (banded) n = nsel_s;
    if (n == 0) {  // (no tie of the layer in this band's rows)
      if (tid == 0) __hip_atomic_fetch_max(my_prog, TR_PROG_DONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    #pragma unroll 1
    for (int j = tid; j < n; j += nthreads) {
      const int b = (int)((skey[j] >> 13) & 0x1FFF) >> shift;
      atomicAdd(&bstart[b], 1);
      bnext[j] = (uint16_t)atomicExch(&bhead[b], j);
    }
    __syncthreads();
    {  // exclusive prefix over the buckets: a contiguous stretch per thread, wave scan, wave totals
      const int per = (TR_NB + nthreads - 1) / nthreads;
      const int b0 = min(tid * per, TR_NB), b1 = min(b0 + per, TR_NB);
      int local = 0;
      #pragma unroll 1
      for (int b = b0; b < b1; ++b) local += bstart[b];
      const int incl = wave_inclusive_scan(local);
      if (lane == 63) wsum[wave] = (unsigned)incl;
      __syncthreads();
      int base = incl - local;
      #pragma unroll 1
      for (int q = 0; q < wave; ++q) base += (int)wsum[q];
      #pragma unroll 1
      for (int b = b0; b < b1; ++b) {
        const int t = bstart[b];
        bstart[b] = base;
        base += t;
      }
    }
    __syncthreads();
    #pragma unroll 1
    for (int j = tid; j < n; j += nthreads) {
      const unsigned k = skey[j];
      const int b = (int)((k >> 13) & 0x1FFF) >> shift;
      int r = bstart[b];
      #pragma unroll 1
      for (int q = bhead[b]; q >= 0; q = (bnext[q] == 0xFFFFu) ? -1 : (int)bnext[q]) r += (skey[q] < k) ? 1 : 0;
      sorder[r] = vals_ci[j];
      sxyd[r] = k;
    }
    __syncthreads();
  }
#endif
  // (a layer beyond the on-chip capacity was put into raster order at the top of the layer loop: tie_sort_large)

  uint16_t* wl = win[wave * TR_NW];
  (void)wl;
  for (int c0 = 0; c0 < n; c0 += TR_CHUNK) {
    const int nc = min(TR_CHUNK, n - c0);
    if (!on_chip) {
      __syncthreads();
      for (int r = tid; r < nc; r += nthreads) {
        const int ci = __hip_atomic_load(&list[c0 + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (rewritten above: not from L1)
        sorder[r] = ci;
        sxyd[r] = C[ci].key;
      }
      __syncthreads();
    }
#define TR_NEED(key_, need_)                                                                                     \
  {                                                                                                              \
    const int x_ = (int)((key_) & 0x1FFF), y_ = (int)(((key_) >> 13) & 0x1FFF);                                  \
    const int cell_ = (y_ >> bm_shift) * bm_w + (x_ >> bm_shift);                                                \
    need_ = (below_elsewhere && ((below_bm[cell_ >> 5] >> (cell_ & 31)) & 1u)) ? brisk_tie_rows_needed(y_, below_is_octave) : 0; \
  }
    // (measured and dropped, round 5: the writer wave alone reading the progress of the layer below from memory and handing
    // it on through LDS - the deciding waves no longer pay an L2 round trip per poll, but see the progress a writer pass
    // later: one 1080p frame 120 -> 132 us, one 4K frame 289 -> 296 us, batches unchanged)
#define TR_POLL(need_)                                                                                           \
  if (seen < need_) {                                                                                            \
    seen = max(seen, __hip_atomic_load(&seen_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));                \
    if (seen < need_) {                                                                                          \
      if (!below_banded) {                                                                                       \
        seen = __hip_atomic_load(below_prog, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                        \
      } else {                                                                                                   \
        for (;;) {                                                                                               \
          const int* pw_ = below_band ? &counters[frame].tie_prog_b[(l - 1) * (BRISK_TIE_MAX_BANDS - 1) + below_band - 1] : below_prog;  \
          const int p_ = __hip_atomic_load(pw_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                     \
          if (p_ == TR_PROG_DONE && below_band + 1 < nb_k) { ++below_band; continue; }                           \
          seen = max(seen, (p_ == TR_PROG_DONE) ? TR_PROG_DONE : max(p_, below_band * rows_pb_below));           \
          break;                                                                                                 \
        }                                                                                                        \
      }                                                                                                          \
      if (lane == 0) __hip_atomic_fetch_max(&seen_s, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      \
    }                                                                                                            \
  }
    // everything the decision loop needs besides the smap window goes on chip: footprints by rank, decisions, the rows
    // of the layer below that must be done before the tie's window is read (round 5: was two dependent LDS reads per tie)
    for (int r = tid; r < nc; r += nthreads) {
      const BriskCand* c = &C[sorder[r]];
      sfpxy[r] = (unsigned)(uint16_t)c->fp_x0 | ((unsigned)(uint16_t)c->fp_y0 << 16);
      sfpm[r] = c->fp_mask;
      tstat[r] = 0;
      int need_r;
      TR_NEED(sxyd[r], need_r)
      sneed[r] = (uint16_t)need_r;
#if TR_KERNEL_PAIR
      {
        const unsigned kr = sxyd[r], y4 = max((int)((kr >> 13) & 0x1FFF) - 4, 0);
        const unsigned kb = (kr & 0xFC000000u) | (y4 << 13);
        int a = 0, b = r;
        while (a < b) {
          const int m = (a + b) >> 1;
          if (sxyd[m] < kb) a = m + 1; else b = m;
        }
        sback[r] = (uint16_t)a;
      }
#endif
    }
    __syncthreads();
    // Round-robin over the raster-sorted ties: neighbouring ties (which depend on each other) run on different
    // waves back to back.  The only thing a tie needs from raster-earlier ties of its 9x9 window is their
    // decision, which is exchanged through LDS (tstat); the window itself and the 5x5 score block of a wave's
    // NEXT tie are prefetched into registers while the current one is decided.
#if TR_KERNEL_PAIR
    // ---- two ties per wave (round 5), for layers of at least pair_min ties: half wave h decides rank j0 + h * dwaves.  The window read, the search for pending
    // earlier ties and the static step of the cache replay - three quarters of a decision's 4.25 us - run for both ties in
    // the same instructions (the single form keeps 33 of 64 lanes busy); every half then takes its decision the moment ITS
    // pending ties are decided, inside the polling loop: the other half may still be waiting - possibly for THIS half's
    // decision, or for a wave that waits for it -, so neither ever holds the other's decision back.  An iteration takes
    // 6.0 us instead of 4.4 (the pair waits for the later of two sets of pending ties, and for the layer below up to the later
    // tie's rows), which the small layers at the top of the pyramid - two or three iterations in all - do not win back.
    {
      // (experiments: bits 16.. of pair_min select how ranks are dealt - 0: halves dwaves apart, 1: adjacent ranks in one wave)
      const bool paired = nc >= (pair_min & 0xFFFF);
      const int pmode = pair_min >> 16;
      const int wmul = (paired && pmode == 1) ? 2 : 1, jstep = paired ? 2 * dwaves : dwaves;
      const int hoffv = (lane >> 5) ? (paired ? (pmode == 1 ? 1 : dwaves) : TR_CHUNK) : 0;  // this half's rank offset (beyond the chunk: no tie)
      const int half = lane >> 5, hl = lane & 31;
      uint16_t* wlh = win[wave * 2 + half];
      uint8_t* kph = kp5s[wave * 2 + half];
      int* valh = vals[wave * 2 + half];
      int j0 = (wave < dwaves) ? wave * wmul : nc;
      // the lane's three window entries (hl, hl + 32, hl + 64) as offsets + 4, four bits each: x0 y0 x1 y1 x2 y2
      const unsigned woff = (unsigned)(hl % TR_WIN) | ((unsigned)(hl / TR_WIN) << 4) | ((unsigned)((hl + 32) % TR_WIN) << 8) |
                            ((unsigned)((hl + 32) / TR_WIN) << 12) | ((unsigned)(min(hl + 64, TR_WIN * TR_WIN - 1) % TR_WIN) << 16) |
                            ((unsigned)(min(hl + 64, TR_WIN * TR_WIN - 1) / TR_WIN) << 20);
      TR_STAMP(tid == 0, l, 1)
#ifdef TR_TIMING
      int tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      long long tlast = (long long)wall_clock64();
#endif
      unsigned pw0 = 0, pw1 = 0, pw2 = 0, pkb = 0;
      bool pvalid = false;
#define TRP_LOADWIN(jj_, a0_, a1_, a2_)                                                                          \
  {                                                                                                              \
    const unsigned k_ = sxyd[min((jj_) + hoffv, nc - 1)];                                                        \
    const int cx_ = k_ & 0x1FFF, cy_ = (k_ >> 13) & 0x1FFF;                                                      \
    const int qx0_ = cx_ + (int)(woff & 15u) - 4, qy0_ = cy_ + (int)((woff >> 4) & 15u) - 4;                      \
    const int qx1_ = cx_ + (int)((woff >> 8) & 15u) - 4, qy1_ = cy_ + (int)((woff >> 12) & 15u) - 4;              \
    const int qx2_ = cx_ + (int)((woff >> 16) & 15u) - 4, qy2_ = cy_ + (int)((woff >> 20) & 15u) - 4;             \
    a0_ = smap_load_fresh(L.smap, (long)min(max(qy0_, 0), L.h - 1) * L.stride + min(max(qx0_, 0), L.w - 1));     \
    a1_ = smap_load_fresh(L.smap, (long)min(max(qy1_, 0), L.h - 1) * L.stride + min(max(qx1_, 0), L.w - 1));     \
    a2_ = smap_load_fresh(L.smap, (long)min(max(qy2_, 0), L.h - 1) * L.stride + min(max(qx2_, 0), L.w - 1));     \
    if (qx0_ < 0 || qy0_ < 0 || qx0_ >= L.w || qy0_ >= L.h) a0_ = 0;                                            \
    if (qx1_ < 0 || qy1_ < 0 || qx1_ >= L.w || qy1_ >= L.h) a1_ = 0;                                            \
    if (qx2_ < 0 || qy2_ < 0 || qx2_ >= L.w || qy2_ >= L.h) a2_ = 0;                                            \
  }
      // rows of the layer below both ties of the pair need (the later one's: a slight over-wait for the earlier)
#define TRP_NEED(jj_, need_)                                                                                     \
  {                                                                                                              \
    const int nh_ = ((jj_) + hoffv < nc) ? (int)sneed[min((jj_) + hoffv, nc - 1)] : 0;                           \
    need_ = max(__builtin_amdgcn_readlane(nh_, 0), __builtin_amdgcn_readlane(nh_, 32));                          \
  }
#define TRP_TRY_PREFETCH(jj_)                                                                                    \
  {                                                                                                              \
    int need_;                                                                                                   \
    TRP_NEED(jj_, need_)                                                                                         \
    TR_POLL(need_)                                                                                               \
    pvalid = seen >= need_;                                                                                      \
    if (pvalid) TRP_LOADWIN(jj_, pw0, pw1, pw2)                                                                  \
    pkb = blocks[((long)frame * cand_cap + sorder[min((jj_) + hoffv, nc - 1)]) * 64 + min(hl, 24)];              \
  }
      if (j0 < nc) TRP_TRY_PREFETCH(j0)
      while (j0 < nc) {
        unsigned v0 = pw0, v1 = pw1, v2 = pw2;
        const unsigned kb = pkb;
        const bool valid = pvalid;
        const int jme = j0 + hoffv;
        const bool hv = jme < nc;  // this half has a tie
        const unsigned key = sxyd[min(jme, nc - 1)];
        const int cx = key & 0x1FFF, cy = (key >> 13) & 0x1FFF;
        {
          const int jn = min(j0 + jstep, nc - 1);  // (the last prefetch of a wave is redundant, never out of range)
          TRP_TRY_PREFETCH(jn)
        }
        TR_T(2)
        if (!valid) {  // pipeline front: wait for the layer below, then read the windows
          int need;
          TRP_NEED(j0, need)
          long long t0 = 0;
          for (int spin = 0; seen < need; ++spin) {
            TR_POLL(need)
            if (seen >= need || __hip_atomic_load(&abort_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
            __builtin_amdgcn_s_sleep(8);
            if ((spin & 255) == 255) {
              const long long now = (long long)wall_clock64();
              if (!t0) t0 = now;
              else if (now - t0 > wait_budget) break;
            }
          }
          if (seen < need) __hip_atomic_store(&abort_s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (the layer below: never observed)
          TRP_LOADWIN(j0, v0, v1, v2)
        }
        TR_T(7)
        // the windows as they were read (ties that were pending then show status TIE) and the score blocks go to LDS
        wlh[hl] = (uint16_t)v0;
        wlh[hl + 32] = (uint16_t)v1;
        if (hl + 64 < TR_WIN * TR_WIN) wlh[hl + 64] = (uint16_t)v2;
        if (hl < 25) kph[hl] = (uint8_t)kb;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int centre = BRISK_SM_D(wlh[4 * TR_WIN + 4]);
        // raster-earlier ties of the window (entries 0..39 of the 81) that were pending: where their decisions will
        // appear.  Entry hl on every lane, entry hl + 32 on the half's first eight lanes.
        int lo0 = -1, lo1 = -1;
        {
          const bool p0 = hv && BRISK_SM_D(v0) && BRISK_SM_STATUS(v0) == BRISK_ST_TIE;
          const bool p1 = hv && hl < 8 && BRISK_SM_D(v1) && BRISK_SM_STATUS(v1) == BRISK_ST_TIE;
          if (p0 || p1) {  // both searches in one loop: their LDS reads overlap
            const unsigned k0 = ((unsigned)l << 26) | ((unsigned)(cy + (int)((woff >> 4) & 15u) - 4) << 13) | (unsigned)(cx + (int)(woff & 15u) - 4);
            const unsigned k1 = ((unsigned)l << 26) | ((unsigned)(cy + (int)((woff >> 12) & 15u) - 4) << 13) | (unsigned)(cx + (int)((woff >> 8) & 15u) - 4);
            const int back = sback[min(jme, nc - 1)];  // (the window's rows start at cy - 4)
            int a0 = p0 ? back : 0, b0 = p0 ? jme : 0, a1 = p1 ? back : 0, b1 = p1 ? jme : 0;
            while (a0 < b0 || a1 < b1) {
              const int m0 = (a0 + b0) >> 1, m1 = (a1 + b1) >> 1;
              const unsigned s0 = sxyd[m0], s1 = sxyd[m1];
              if (a0 < b0) { if (s0 < k0) a0 = m0 + 1; else b0 = m0; }
              if (a1 < b1) { if (s1 < k1) a1 = m1 + 1; else b1 = m1; }
            }
            // (a pending raster-earlier tie of the window is always in this chunk: earlier chunks are complete and the
            // window was read after they were)
            const bool f0 = p0 && a0 < jme && sxyd[a0] == k0, f1 = p1 && a1 < jme && sxyd[a1] == k1;
            // a pending tie above this band's first row belongs to the band above: its decision comes through the map (-2)
            const bool x0 = p0 && !f0 && banded && (int)((k0 >> 13) & 0x1FFF) < y0b, x1 = p1 && !f1 && banded && (int)((k1 >> 13) & 0x1FFF) < y0b;
            if ((p0 && !f0 && !x0) || (p1 && !f1 && !x1)) __hip_atomic_store(&abort_s, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (never observed)
            lo0 = f0 ? a0 : (x0 ? -2 : -1);
            lo1 = f1 ? a1 : (x1 ? -2 : -1);
          }
        }
        TR_T(3)
        // everything of the cache replay that does not depend on those decisions, before waiting for them
        unsigned spk = BRISK_SS_FINAL, sdyn = 0;
        int tsx = 0, tsy = 0;
        {
          bool town;
          brisk_tie_slot_offset(tslot, &tsx, &tsy, &town);
          const unsigned selfi = tam >> 25;
          if (hv)
            spk = brisk_tie_slot_static_m(L, float_patch, touch2x2, cx, cy, tslot, tsx, tsy, tam & 0x1FFFFFFu, ~(selfi < 25 ? (1u << selfi) : 0u), wlh,
                                          cx - 4, cy - 4, TR_WIN, kph, &sdyn);
        }
        TR_T(5)
        // decisions: a half resolves and publishes as soon as every pending tie of ITS window is decided
        bool done = !hv;
        long long t0 = 0;
        for (int spin = 0;; ++spin) {
          int st0 = 1, st1 = 1;
          if (!done) {
            if (lo0 >= 0) st0 = __hip_atomic_load(&tstat[lo0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) & 3;
            if (lo1 >= 0) st1 = __hip_atomic_load(&tstat[lo1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) & 3;
            if (lo0 == -2 || lo1 == -2) {  // the band above: PASS / FAIL appears in the score-state map (TIE: still pending)
              if (lo0 == -2) {
                const unsigned v = smap_load_fresh(L.smap, (long)(cy + (int)((woff >> 4) & 15u) - 4) * L.stride + cx + (int)(woff & 15u) - 4);
                st0 = (BRISK_SM_STATUS(v) == BRISK_ST_TIE) ? 0 : (int)BRISK_SM_STATUS(v);
              }
              if (lo1 == -2) {
                const unsigned v = smap_load_fresh(L.smap, (long)(cy + (int)((woff >> 12) & 15u) - 4) * L.stride + cx + (int)((woff >> 8) & 15u) - 4);
                st1 = (BRISK_SM_STATUS(v) == BRISK_ST_TIE) ? 0 : (int)BRISK_SM_STATUS(v);
              }
            }
          }
          const unsigned long long rb = __ballot(done || (st0 && st1));
          const bool half_ready = (unsigned)(rb >> (32 * half)) == 0xFFFFFFFFu;
          if (half_ready && !done) {
            TR_T(4)
            if (lo0 != -1) wlh[hl] = (uint16_t)((v0 & ~0x3000u) | ((unsigned)st0 << 12));
            if (lo1 != -1) wlh[hl + 32] = (uint16_t)((v1 & ~0x3000u) | ((unsigned)st1 << 12));
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // the open events with the decisions in
            valh[tslot] = brisk_tie_slot_resolve(L, spk, sdyn, cx, cy, centre, tslot, wlh, cx - 4, cy - 4, TR_WIN, kph);
            if (hl == 0) valh[8 + 12] = centre;  // (the block's centre: the candidate's own value)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // the eight neighbours of the tie list on the half's first eight lanes
            const bool nb_ok = (hl >= 8) || brisk_tie_neighbour_ok(centre, &valh[0], &valh[8], hl);
            const bool pass = (unsigned)(__ballot(nb_ok) >> (32 * half)) == 0xFFFFFFFFu;
            const int dec = pass ? (int)BRISK_ST_PASS : (int)BRISK_ST_FAIL;
            // the decision goes to LDS only (other waves - and the other half - spin on it); the writer wave takes it to memory
            if (hl == 0) __hip_atomic_store(&tstat[jme], dec, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            done = true;
            TR_T(0)
#ifdef TR_TIMING
            if (half == 0 || !(rb & 1)) tacc[1] += 1;  // passes through the resolve step (1 or 2 per pair)
#endif
          }
          if (__all(done)) break;
          if (__hip_atomic_load(&abort_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
          __builtin_amdgcn_s_sleep(1);
          if ((spin & 4095) == 4095) {  // (the other waves may themselves be waiting for the layer below)
            const long long now = (long long)wall_clock64();
            if (!t0) t0 = now;
            else if (now - t0 > wait_budget) break;
          }
        }
        if (!__all(done) && !__hip_atomic_load(&abort_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
          __hip_atomic_store(&abort_s, 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (never observed)
        __builtin_amdgcn_wave_barrier();
        TR_T(4)
#ifdef TR_TIMING
        tacc[6] += 1;
#endif
        TR_STAMP(tid == 0 && j0 == 0, l, 2)
        j0 += jstep;
      }
#ifdef TR_TIMING
      if (lane == 0 && wave < dwaves)
        for (int i = 0; i < 8; ++i) atomicAdd(&counters[frame].tphase[i], tacc[i]);
#endif
#undef TRP_TRY_PREFETCH
#undef TRP_NEED
#undef TRP_LOADWIN
    }
#else
    {
    int j = (wave < dwaves) ? wave : nc;
    TR_STAMP(tid == 0, l, 1)
#ifdef TR_TIMING
    int tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long tlast = (long long)wall_clock64();
#endif
    unsigned pw0 = 0, pw1 = 0, pkb = 0;
    bool pvalid = false;
#define TR_PREFETCH(jj)                                                                                          \
  {                                                                                                              \
    const unsigned k_ = sxyd[jj];                                                                                \
    const int cx_ = k_ & 0x1FFF, cy_ = (k_ >> 13) & 0x1FFF;                                                      \
    const int e1_ = min(lane + 64, TR_WIN * TR_WIN - 1);                                                         \
    const int qx0_ = cx_ + lane % TR_WIN - 4, qy0_ = cy_ + lane / TR_WIN - 4;                                    \
    const int qx1_ = cx_ + e1_ % TR_WIN - 4, qy1_ = cy_ + e1_ / TR_WIN - 4;                                      \
    pw0 = smap_load_fresh(L.smap, (long)min(max(qy0_, 0), L.h - 1) * L.stride + min(max(qx0_, 0), L.w - 1));     \
    pw1 = smap_load_fresh(L.smap, (long)min(max(qy1_, 0), L.h - 1) * L.stride + min(max(qx1_, 0), L.w - 1));     \
    if (qx0_ < 0 || qy0_ < 0 || qx0_ >= L.w || qy0_ >= L.h) pw0 = 0;                                            \
    if (qx1_ < 0 || qy1_ < 0 || qx1_ >= L.w || qy1_ >= L.h) pw1 = 0;                                            \
  }
#define TR_PREFETCH_BLOCK(jj) pkb = blocks[((long)frame * cand_cap + sorder[jj]) * 64 + min(lane, 24)];
    // the window may only be read once the layer below is past the rows that can touch it
#define TR_TRY_PREFETCH(jj)                                                                                      \
  {                                                                                                              \
    int need_;                                                                                                   \
    need_ = sneed[jj];                                                                                           \
    TR_POLL(need_)                                                                                               \
    TR_T(1)                                                                                                      \
    pvalid = seen >= need_;                                                                                      \
    if (pvalid) TR_PREFETCH(jj)                                                                                  \
    TR_PREFETCH_BLOCK(jj)                                                                                        \
  }
    if (j < nc) TR_TRY_PREFETCH(j)
    while (j < nc) {
      unsigned v0 = pw0;
      unsigned v1 = pw1;
      const unsigned kb = pkb;
      const bool valid = pvalid;
      const unsigned key = sxyd[j];
      const int cx = key & 0x1FFF, cy = (key >> 13) & 0x1FFF;
      {
        const int jn = min(j + dwaves, nc - 1);  // (the last prefetch of a wave is redundant, never out of range)
        TR_TRY_PREFETCH(jn)
      }
      TR_T(2)
      if (!valid) {  // pipeline front: wait for the layer below, then read the window
        const int need = sneed[j];
        long long t0 = 0;
        for (int spin = 0; seen < need; ++spin) {
          TR_POLL(need)
          if (seen >= need || __hip_atomic_load(&abort_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
          __builtin_amdgcn_s_sleep(8);
          if ((spin & 255) == 255) {
            const long long now = (long long)wall_clock64();
            if (!t0) t0 = now;
            else if (now - t0 > wait_budget) break;
          }
        }
        if (seen < need) __hip_atomic_store(&abort_s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (the layer below: never observed)
        const unsigned s0 = pw0, s1 = pw1;  // keep the next tie's prefetch
        TR_PREFETCH(j)
        v0 = pw0; v1 = pw1;
        pw0 = s0; pw1 = s1;
      }
      TR_T(7)
      // the window as it was read (ties that were pending then show status TIE) and the score block go to LDS
      wl[lane] = (uint16_t)v0;
      if (lane + 64 < TR_WIN * TR_WIN) wl[lane + 64] = (uint16_t)v1;
      if (lane < 25) kp5s[wave * TR_NW][lane] = (uint8_t)kb;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int centre = BRISK_SM_D(wl[4 * TR_WIN + 4]);
      // lanes 0-7: the 8 probe values, lanes 32-56: the 5x5 raw block (vals[8..32])
      int slot_v = (lane < 8) ? lane : (lane >= 32 && lane < 57) ? lane - 24 : -1;
#if TR_KERNEL_LIST
      // (opaque to the compiler: what the static step derives from the slot - the pixel's offsets in the window and in the
      // block, for either form - is worked out per tie instead of living in registers across all loops of the kernel:
      // 104 -> 90 VGPRs, the bound is 96)
      asm volatile("" : "+v"(slot_v));
#endif
      const int slot = slot_v;
      // raster-earlier ties of the window (entries 0..39 of the 81) that were pending: where their decisions will appear
      int lo = -1;
      {
        const int dy = lane / TR_WIN - 4, dx = lane % TR_WIN - 4;
        if (lane < 40 && BRISK_SM_D(v0) && BRISK_SM_STATUS(v0) == BRISK_ST_TIE) {
          const unsigned k2 = ((unsigned)l << 26) | ((unsigned)(cy + dy) << 13) | (unsigned)(cx + dx);
          int hi = j;
          lo = 0;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sxyd[mid] < k2) lo = mid + 1; else hi = mid;
          }
          // (a pending raster-earlier tie of the window is always in this chunk: earlier chunks are complete and the
          // window was read after they were)
          if (!(lo < j && sxyd[lo] == k2)) {
            __hip_atomic_store(&abort_s, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (never observed)
            lo = -1;
          }
        }
      }
      TR_T(3)
      // everything of the cache replay that does not depend on those decisions, before waiting for them
      unsigned spk = BRISK_SS_FINAL, sdyn = 0;
#if TR_KERNEL_LIST
      // the window's candidates that can act (entries 0 ... 40 with a score, the tie itself among them): a short list is
      // walked entry by entry (brisk_state_static_list, all lanes: the entry's value is lane e's v0), a long one - all-tie
      // images reach 41 - takes the unrolled loop over the pixel's 24 neighbours
      const unsigned long long clist = __ballot(lane <= BRISK_TIE_WIN_SELF && BRISK_SM_D(v0) != 0);
      const bool by_list = __builtin_popcountll(clist) <= BRISK_TIE_LIST_CAP;
      if (by_list) spk = brisk_tie_slot_static_list(L, float_patch, touch2x2, cx, cy, slot, wl, kp5s[wave * TR_NW], clist, v0, &sdyn);
#else
      const bool by_list = false;
#endif
      if (slot >= 0 && !by_list) {
        if (masks) {
          int tsx, tsy;
          bool town;
          brisk_tie_slot_offset(slot, &tsx, &tsy, &town);
          const unsigned selfi = tam >> 25;
          spk = brisk_tie_slot_static_m(L, float_patch, touch2x2, cx, cy, slot, tsx, tsy, tam & 0x1FFFFFFu, ~(selfi < 25 ? (1u << selfi) : 0u), wl, cx - 4,
                                        cy - 4, TR_WIN, kp5s[wave * TR_NW], &sdyn);
        }
        else spk = brisk_tie_slot_static(L, float_patch, touch2x2, cx, cy, slot, wl, cx - 4, cy - 4, TR_WIN, kp5s[wave * TR_NW], &sdyn);
      }
      TR_T(5)
      if (lo >= 0) {
        int st = 0;
        long long t0 = 0;
        for (int spin = 0;; ++spin) {
          st = __hip_atomic_load(&tstat[lo], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) & 3;
          if (st || __hip_atomic_load(&abort_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
          __builtin_amdgcn_s_sleep(1);
          if ((spin & 4095) == 4095) {  // (the other wave may itself be waiting for the layer below)
            const long long now = (long long)wall_clock64();
            if (!t0) t0 = now;
            else if (now - t0 > wait_budget) break;
          }
        }
        if (!st && !__hip_atomic_load(&abort_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) __hip_atomic_store(&abort_s, 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (never observed)
        if (st) wl[lane] = (uint16_t)((v0 & ~0x3000u) | ((unsigned)st << 12));
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      TR_T(4)
      // the open events with the decisions in
      if (slot >= 0)
        vals[wave * TR_NW][slot] = brisk_tie_slot_resolve(L, spk, sdyn, cx, cy, centre, slot, wl, cx - 4, cy - 4, TR_WIN, kp5s[wave * TR_NW]);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // the eight neighbours of the tie list on eight lanes (a serial walk on one lane costs ~70 dependent LDS reads)
      const bool nb_ok = (lane >= 8) || brisk_tie_neighbour_ok(centre, &vals[wave * TR_NW][0], &vals[wave * TR_NW][8], lane);
      const bool pass = __all(nb_ok);
      const int dec = pass ? (int)BRISK_ST_PASS : (int)BRISK_ST_FAIL;
      // the decision goes to LDS only (other waves spin on it); the writer wave takes it to memory
      if (lane == 0) __hip_atomic_store(&tstat[j], dec, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      __builtin_amdgcn_wave_barrier();
      TR_T(0)
#ifdef TR_TIMING
      tacc[6] += 1;
#endif
      TR_STAMP(tid == 0 && j == 0, l, 2)
      j += dwaves;
    }
#ifdef TR_TIMING
    if (lane == 0 && wave < dwaves)
      for (int i = 0; i < 8; ++i) atomicAdd(&counters[frame].tphase[i], tacc[i]);
#endif
    }
#endif  // TR_KERNEL_PAIR
    TR_STAMP(tid == 0, l, 3)
    // ---- writer wave: decisions -> score-state map, candidate status, touches on the layer above; a tie counts as
    // done for the layer above once these are performed; the progress is the row of the first tie that is not done.
    // The deciding waves never wait for a memory write this way (an agent-scope atomic takes microseconds).
    if (wave == dwaves) {
      int w = 0, row_pub = -1;
      long long t0 = 0;
      for (int idle = 0; w < nc;) {
        const int i = w + lane;
        const int st = (i < nc) ? __hip_atomic_load(&tstat[i], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) : 0;
        const bool todo = (st & 3) && !(st & TR_DONE_BIT);
        if (todo) {
          const unsigned key = sxyd[i];
          const int cx = key & 0x1FFF, cy = (key >> 13) & 0x1FFF;
          const bool pass = (st & 3) == (int)BRISK_ST_PASS;
          if (pass) smap_xor(L.smap, (long)cy * L.stride + cx, 0x3000u);  // TIE (10b) -> PASS (01b)
          else smap_or(L.smap, (long)cy * L.stride + cx, 0x1000u);       // TIE (10b) -> FAIL (11b)
          cand[(long)frame * cand_cap + sorder[i]].status = (uint8_t)(st & 3);
          const unsigned fpm = (pass && !last) ? (unsigned)sfpm[i] : 0u;
          if (fpm) {
            const int fx = (int16_t)(sfpxy[i] & 0xFFFFu), fy = (int16_t)(sfpxy[i] >> 16);
            const BriskLayerView La = make_view(G, pyr, smap, frame, l + 1);
            for (int b = 0; b < 16; ++b)
              if (fpm & (1u << b)) smap_or(La.smap, (long)(fy + (b >> 2)) * La.stride + fx + (b & 3), BRISK_SM_TOUCH);
          }
        }
        if (__any(todo)) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (todo) __hip_atomic_fetch_or(&tstat[i], TR_DONE_BIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        const unsigned long long decided = __ballot((i < nc) && (st & 3));
        const int lead = (~decided == 0ull) ? 64 : __builtin_ctzll(~decided);
        if (lead) {
          w += lead;
          idle = 0;
          if (lane == 0 && !last && w < nc) {
            const int row = (int)((sxyd[w] >> 13) & 0x1FFF);
            if (row > row_pub) __hip_atomic_fetch_max(my_prog, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          if (w < nc) row_pub = max(row_pub, (int)((sxyd[w] >> 13) & 0x1FFF));
        } else {
          if ((++idle & 4095) == 0) {  // (the deciding waves may be waiting for the layer below)
            const long long now = (long long)wall_clock64();
            if (idle == 4096) t0 = now;
            else if (now - t0 > wait_budget) {  // (never observed)
              __hip_atomic_store(&abort_s, 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              break;
            }
          }
          __builtin_amdgcn_s_sleep(2);
        }
      }
    }
#undef TR_TRY_PREFETCH
#undef TR_POLL
#undef TR_NEED
#undef TR_PREFETCH_BLOCK
#undef TR_PREFETCH
    // the touches are agent-scope atomics and the readers use L1-bypassing loads: completion of the atomics (vmcnt) +
    // the workgroup barrier is all the ordering the next chunk and the progress word need
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TR_STAMP(lane == 0 && wave == dwaves, l, 4)
    __syncthreads();
    TR_STAMP(tid == 0, l, 5)
    if (tid == 0 && !last) {
      const int c1 = c0 + nc;
      const int row = (c1 < n) ? (int)((C[__hip_atomic_load(&list[c1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)].key >> 13) & 0x1FFF) : TR_PROG_DONE;
      __hip_atomic_fetch_max(my_prog, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  }  // layers of this ticket
  __syncthreads();
  if (tid == 0 && abort_s) atomicOr(&counters[frame].overflow, 8 | (abort_s << 8));  // a wait ran into its bound: reported as an error (bits 8-10: which wait)
  if (!persist) return;
  }  // tickets of this workgroup
}
