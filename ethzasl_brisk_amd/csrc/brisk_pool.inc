// brisk_pool.inc - cross-thread call combining for the one-frame host calls (included at the end of brisk_capi.hip: it
// uses that file's static helpers).
//
// The reference's classes are re-entrant (BriskFeatureDetector::detectImpl is const and builds its state per call,
// brisk/src/brisk-feature-detector.cc:77-85): N host threads may call detect() / compute() at once.  With one engine
// context per thread that is N x 15 kernel launches and N x 4 copies per frame pair - and the HIP runtime serialises the
// API calls of a process (round 6, profiles/r06_threads_limiter.txt: hipLaunchKernel 4.6 -> 26 us, hipMemcpyAsync 29 -> 73 us
// from 1 to 8 threads; kernels of different streams overlap 1.9-fold at most), so 16 threads reach 3.6 x one thread.
//
// A pool turns calls that are in the engine AT THE SAME TIME into batches: a call copies its frame into a pinned staging
// slot of the group that is forming (a CPU copy: no runtime call, no lock), the group's first member submits the whole
// group - one H2D copy, the batch kernels, one result transfer (brisk_hip_batch_download_all) - and every member copies
// its own rows out.  Only group leaders talk to the runtime.  A group closes when one of the pool's BRISK_POOL_CTX engine
// contexts is free to take it (one group per context: a small batch is latency-bound, four of them overlap on the chip):
// batches grow with the load, a lone caller is a group of one.
// A detect() call returns a token for the device copy of its frame; a describe() call that presents the token (the
// caller's word that the pixels are the same: brisk::hip::ScopedSameImage) takes the frame from there - one D2D copy
// instead of a second trip over the link.
#include <atomic>
#include <condition_variable>

#define BRISK_POOL_CTX 8      // at most; a pool uses `nctx` engine contexts (4): one group runs per context, the groups of different contexts overlap on the device
#define BRISK_POOL_GROUPS 12  // group buffers: nctx on the device, one forming, the others being read out / holding retained frames

namespace {
struct PoolKey {
  int kind = 0;  // 1 detect, 2 describe
  int w = 0, h = 0, threshold = 0, octaves = 0, rot = 0, scl = 0;
  const brisk_hip_pattern* pat = nullptr;
  bool operator==(const PoolKey& o) const {
    return kind == o.kind && w == o.w && h == o.h && threshold == o.threshold && octaves == o.octaves && rot == o.rot && scl == o.scl && pat == o.pat;
  }
};
enum { PG_FREE = 0, PG_FORMING, PG_CLOSED, PG_DONE, PG_PREP /* being sized by the thread that opens it */ };
struct PoolGroup {
  int state = PG_FREE;
  PoolKey key;
  int n = 0, copied = 0, readers = 0;
  unsigned gen = 0;          // counts the uses of this buffer: a token names (buffer, gen, slot)
  unsigned long long seq = 0;  // submission order
  int ci = 0;                  // the context that runs it
  std::condition_variable done_cv;  // the members wait here for the group's results (the pool's own variable wakes everybody)
  int rc = BRISK_HIP_OK;
  std::string err;
  // staging (pinned host) and device frames, [maxb] slots of `frame_bytes`
  PinnedBuf h_frames;
  DeviceBuf d_frames;
  size_t frame_bytes = 0;    // bytes per slot of the current use (dpitch * h)
  int dpitch = 0;
  std::vector<const uint8_t*> src_dev;  // describe: per member, the retained device copy of its frame (null: the frame was staged)
  // describe: provided keypoints (pinned), [maxb][kin_cap]
  PinnedBuf h_kin, h_nin;
  int kin_cap = 0;           // rows per slot of h_kin
  hipEvent_t copied_ev = nullptr;  // the group's frames are on the device
  // results (pinned)
  brisk_hip_batch_host_results res{};
  int res_stride_cap = 0;
  PinnedBuf res_mem;
};
}  // namespace

struct brisk_hip_pool {
  int device = 0, maxb = 16;
  brisk_hip_ctx* ctx[BRISK_POOL_CTX] = {};
  bool busy[BRISK_POOL_CTX] = {};
  int nctx = 4;
  int kp_cap = 0;
  std::mutex mu;
  std::condition_variable cv;
  PoolGroup g[BRISK_POOL_GROUPS];
  int forming = -1;        // index of the group that accepts members
  unsigned long long next_seq = 1, submit_seq = 1;  // groups are submitted to the device in the order they closed
  hipStream_t copy = nullptr;
  long long rows_per_group = 0;
  unsigned long long stat_groups = 0, stat_frames = 0;  // groups / member calls run so far
  // wall time per phase, summed over calls (tools: brisk_hip_debug_pool_phases): 0 until the call has joined a group, 1 staging
  // copies, 2 leader: until a context is free and the members have staged, 3 leader: copies queued, 4 leader: batch queued,
  // 5 leader: until the results are in host memory, 6 member: until the group is done, 7 whole call
  std::atomic<long long> phase_ns[8];
  brisk_hip_pool() { for (auto& a : phase_ns) a.store(0); }
};
struct PoolClock {
  brisk_hip_pool* P;
  std::chrono::steady_clock::time_point t;
  explicit PoolClock(brisk_hip_pool* p) : P(p), t(std::chrono::steady_clock::now()) {}
  void lap(int phase) {
    const auto n = std::chrono::steady_clock::now();
    P->phase_ns[phase].fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(n - t).count(), std::memory_order_relaxed);
    t = n;
  }
};
// the calling thread's last pool error (a pool is shared by many threads: one string per pool would be a race)
static thread_local std::string tl_pool_err;

static inline unsigned long long pool_token(int gi, unsigned gen, int slot) {
  return ((unsigned long long)(gen & 0xFFFFFFu) << 16) | ((unsigned long long)(gi + 1) << 8) | (unsigned long long)slot;
}

// (pool->mu held) a group buffer sized for this use; the buffers grow, never shrink
static int pool_prepare_group(brisk_hip_pool* P, std::unique_lock<std::mutex>& lk, PoolGroup& G, const PoolKey& key, int kin_need) {
  const int dpitch = brisk_align_up(key.w, 64);
  const size_t fb = (size_t)dpitch * key.h;
  if (hipSetDevice(P->device) != hipSuccess) return BRISK_HIP_ERR_HIP;
  if (fb * P->maxb > G.d_frames.cap) {  // (the second of the pair)
    // The buffer is FREE: every group that used it is done.  But a describe group that closed and has not reached the
    // device yet may still name frames in it (a token): its copies must be queued before the buffer goes away.
    while (P->submit_seq != P->next_seq) P->cv.wait(lk);
    G.h_frames.reset();
    G.d_frames.reset();
    if (G.h_frames.grow(fb * P->maxb, 256) != hipSuccess || G.d_frames.grow(fb * P->maxb, 256) != hipSuccess) return BRISK_HIP_ERR_HIP;
  }
  if (key.kind == 2 && kin_need > G.kin_cap) {
    const int cap = ((kin_need > 4096 ? kin_need : 4096) + 1023) / 1024 * 1024;
    G.kin_cap = 0;
    if (G.h_kin.grow(sizeof(brisk_hip_keypoint) * (size_t)cap * P->maxb) != hipSuccess) return BRISK_HIP_ERR_HIP;
    G.kin_cap = cap;
  }
  if (G.h_nin.grow(sizeof(int) * (size_t)P->maxb) != hipSuccess) return BRISK_HIP_ERR_HIP;
  const int rstride = key.kind == 2 ? key.pat->host.strings : 4;  // descriptor rows packed at the descriptor size
  if (!G.res_mem.p || rstride > G.res_stride_cap) {
    G.res_stride_cap = rstride > 64 ? rstride : 64;
    const SlabLayout LY = export_layout(P->maxb, P->rows_per_group, G.res_stride_cap);
    if (G.res_mem.grow(LY.bytes()) != hipSuccess) return BRISK_HIP_ERR_HIP;
    G.res = export_at(LY, G.res_mem.as<uint8_t>(), P->maxb, rstride, P->rows_per_group);
  }
  G.res.desc_stride = rstride;
  G.key = key;
  G.frame_bytes = fb;
  G.dpitch = dpitch;
  G.n = 0; G.copied = 0; G.readers = 0;
  G.gen = (G.gen + 1) & 0xFFFFFFu;
  if (!G.gen) G.gen = 1;
  G.rc = BRISK_HIP_OK;
  G.err.clear();
  G.src_dev.assign(P->maxb, nullptr);
  G.state = PG_FORMING;
  return BRISK_HIP_OK;
}

// descriptor-only batch on frames resident in HBM (the pool's describe groups): the n-frame form of describe_host.
// d_kp_in / d_n_in of the context hold the provided keypoints (kp_cap rows per frame) and their counts.
static int describe_batch_locked(brisk_hip_ctx* ctx, const brisk_hip_pattern* pat, const uint8_t* d_frames, int nframes, int w, int h,
                                 long frame_pitch, int row_pitch, int rot, int scl, int n_in_max, hipStream_t s) {
  make_geometry(w, h, 20, 0, &ctx->G, &ctx->T);  // only layer 0 is needed
  ctx->G.debug_flags = dbg_flags(ctx);
  if (pat->host.strings > ctx->desc_pitch) ctx->desc_pitch = brisk_align_up(pat->host.strings, 16);
  // (ensure_buffers ran before the keypoints were uploaded: brisk_pool_submit)
  if (ctx->dirty_frames > 0) {
    brisk_launch_smap_clear(ctx->dirtyG, ctx->B, ctx->dirty_frames, s);
    ctx->dirty_frames = 0;
  }
  HIPCHK(ctx, hipMemsetAsync(ctx->B.counters, 0, sizeof(BriskFrameCounters) * (size_t)nframes, s));
  ctx->img_cache.valid = false;
  ctx->last_l0_ext = nullptr;
  BriskDetectBuffers Bd = ctx->B;
  brisk_prof_begin_call(&ctx->prof);
  brisk_prof_mark(&ctx->prof, BRISK_STG_PYRAMID, s);
  brisk_launch_layer0_only(ctx->G, ctx->B, nframes, d_frames, frame_pitch, row_pitch, s);
  Bd.band_h = 64;
  brisk_prof_mark(&ctx->prof, BRISK_STG_DETECT, s);
  BriskPatternDev Pd = pat->dev;
  Pd.rotation_invariant = rot ? 1 : 0;
  Pd.scale_invariant = scl ? 1 : 0;
  BriskDescribeBuffers Dd = ctx->D;
  integral_format(ctx, pat, false, &Dd.ibits);
  brisk_launch_describe(ctx->G, Pd, Bd, Dd, nframes, ctx->d_kp_in.as<BriskKeyPoint>(), ctx->d_n_in.as<int>(), sizeof(int), s, &ctx->prof, nullptr, n_in_max);
  if (ctx->prof.on) ctx->prof.calls++;
  HIPCHK(ctx, hipGetLastError());
  ctx->last_nframes = nframes;
  ctx->last_has_desc = true;
  ctx->last_desc_pitch = Dd.desc_pitch;
  ctx->last_strings = pat->host.strings;
  return BRISK_HIP_OK;
}

// The leader's part, step 1 - IN THE ORDER THE GROUPS CLOSED (pool_run holds that order): the group's frames onto the device.
// The copy stream is one for the whole pool, so a describe group's device-to-device copies out of another group's buffer are
// queued before the copy that refills that buffer.  Nothing else of a submission is ordered between groups.
static int pool_submit_copies(brisk_hip_pool* P, PoolGroup& G) {
  brisk_hip_ctx* ctx = P->ctx[G.ci];
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCHK(ctx, hipSetDevice(P->device));
  if (!G.copied_ev) HIPCHK(ctx, hipEventCreateWithFlags(&G.copied_ev, hipEventDisableTiming));
  if (G.key.kind == 1) {
    // one copy for the whole group (staging slots are contiguous)
    HIPCHK(ctx, hipMemcpyAsync(G.d_frames.p, G.h_frames.p, G.frame_bytes * (size_t)G.n, hipMemcpyHostToDevice, P->copy));
  } else {
    // describe: retained device copies (D2D) or staged frames (H2D); runs of staged slots go as one copy
    for (int i = 0; i < G.n;) {
      uint8_t* dst = G.d_frames.as<uint8_t>() + (size_t)i * G.frame_bytes;
      if (G.src_dev[i]) {
        HIPCHK(ctx, hipMemcpyAsync(dst, G.src_dev[i], G.frame_bytes, hipMemcpyDeviceToDevice, P->copy));
        ++i;
      } else {
        int j = i + 1;
        while (j < G.n && !G.src_dev[j]) ++j;
        HIPCHK(ctx, hipMemcpyAsync(dst, G.h_frames.as<uint8_t>() + (size_t)i * G.frame_bytes, G.frame_bytes * (size_t)(j - i), hipMemcpyHostToDevice, P->copy));
        i = j;
      }
    }
  }
  HIPCHK(ctx, hipEventRecord(G.copied_ev, P->copy));
  return BRISK_HIP_OK;
}

// step 2 (any order between groups): the batch on the group's context and the transfer of its results; returns the ticket
static int pool_submit_batch(brisk_hip_pool* P, PoolGroup& G, unsigned* ticket) {
  brisk_hip_ctx* ctx = P->ctx[G.ci];
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIPCHK(ctx, hipSetDevice(P->device));
  const PoolKey& K = G.key;
  hipStream_t s = ctx->stream;
  if (K.kind == 1) {
    HIPCHK(ctx, hipStreamWaitEvent(s, G.copied_ev, 0));
    // (the batch reads the frames where they are: the group's buffer is not touched again before the group is done)
    int rc = run_batch(ctx, nullptr, G.d_frames.as<uint8_t>(), G.n, K.w, K.h, (long)G.frame_bytes, G.dpitch, K.threshold, K.octaves, nullptr, 0, 0, s, true,
                       false, 0.0, 0x7FFFFFFF, false, BRISK_LOWER_THRESHOLD, nullptr);
    if (rc) return rc;
    return download_all_locked(ctx, 0, &G.res, s, ticket, true, true);
  }
  int nmax = 0;
  for (int i = 0; i < G.n; ++i) nmax = G.h_nin.as<int>()[i] > nmax ? G.h_nin.as<int>()[i] : nmax;
  if (nmax > ctx->kp_cap) return fail(ctx, BRISK_HIP_ERR_CAPACITY, "more keypoints than the pool's capacity");
  if (int rcp = check_pattern_device(ctx, K.pat)) return rcp;
  BriskGeom Gd;
  BriskTileTable Td;
  make_geometry(K.w, K.h, 20, 0, &Gd, &Td);
  if (K.pat->host.strings > ctx->desc_pitch) ctx->desc_pitch = brisk_align_up(K.pat->host.strings, 16);
  int rc = ensure_buffers(ctx, G.n, Gd);
  if (rc) return rc;
  if (workspace_acquire(ctx, s)) return fail(ctx, BRISK_HIP_ERR_HIP, "hipStreamWaitEvent failed");
  WorkspaceGuard guard(ctx, s);
  // the provided keypoints into the context's own buffers: on the compute stream, behind the kernels that still read them
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_n_in.p, G.h_nin.p, sizeof(int) * (size_t)G.n, hipMemcpyHostToDevice, s));
  if (nmax > 0)
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_kp_in.p, sizeof(BriskKeyPoint) * (size_t)ctx->B.kp_cap, G.h_kin.p, sizeof(brisk_hip_keypoint) * (size_t)G.kin_cap,
                                 sizeof(brisk_hip_keypoint) * (size_t)nmax, (size_t)G.n, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipStreamWaitEvent(s, G.copied_ev, 0));
  rc = describe_batch_locked(ctx, K.pat, G.d_frames.as<uint8_t>(), G.n, K.w, K.h, (long)G.frame_bytes, G.dpitch, K.rot, K.scl, nmax, s);
  if (rc) return rc;
  if (guard.release()) return fail(ctx, BRISK_HIP_ERR_HIP, "hipEventRecord failed");
  return download_all_locked(ctx, 1, &G.res, s, ticket, true, true);
}

// Joins (or opens) the group of `key`, stages the caller's frame (unless `token` names a retained device copy), lets the
// group's leader run it and waits for the group; on return *gi / *slot name the caller's rows in the group's results and
// the caller must call pool_leave() when it has copied them out.
static int pool_run(brisk_hip_pool* P, const PoolKey& key, const uint8_t* img, int stride, unsigned long long token, const brisk_hip_keypoint* kin,
                    int nin, int* gi_out, int* slot_out) {
  PoolClock clk(P), whole(P);
  std::unique_lock<std::mutex> lk(P->mu);
  int gi = -1;
  for (;;) {
    if (P->forming >= 0) {
      PoolGroup& F = P->g[P->forming];
      if (F.state == PG_FORMING && F.key == key && F.n < P->maxb && (key.kind != 2 || nin <= F.kin_cap)) { gi = P->forming; break; }
      P->cv.wait(lk);  // another kind of call is forming (or the group is full): it closes as soon as the device takes it
      continue;
    }
    int f = -1;
    for (int i = 0; i < BRISK_POOL_GROUPS; ++i)
      if (P->g[i].state == PG_FREE) { f = i; break; }
    if (f < 0) { P->cv.wait(lk); continue; }
    P->g[f].state = PG_PREP;  // (the preparation may wait: nobody else takes this buffer or opens another group meanwhile)
    P->forming = f;
    const int rc = pool_prepare_group(P, lk, P->g[f], key, nin);
    if (rc) {
      P->g[f].state = PG_FREE;
      P->forming = -1;
      P->cv.notify_all();
      tl_pool_err = "pool: allocation of a group's buffers failed";
      return rc;
    }
    gi = f;
    break;
  }
  PoolGroup& G = P->g[gi];
  const int slot = G.n++;
  const bool leader = slot == 0;
  G.readers++;
  // A retained frame is taken only while its buffer still carries that use (the generation).  Its ADDRESS is fixed here, under the
  // lock: by the time the leader queues the copy the buffer may have been prepared for another use - of another frame size - whose
  // own copies are queued behind this group's (one forming group at a time, one copy stream), so the bytes are still there.
  const uint8_t* retained = nullptr;
  if (token && key.kind == 2) {
    const int sg = (int)((token >> 8) & 0xFF) - 1, sslot = (int)(token & 0xFF);
    if (sg >= 0 && sg < BRISK_POOL_GROUPS && sg != gi) {
      const PoolGroup& S = P->g[sg];
      // (FREE is fine: the frames stay in the buffer until it is prepared for another use, which changes the generation)
      if (S.state != PG_FORMING && S.state != PG_PREP && S.gen == (unsigned)((token >> 16) & 0xFFFFFFu) && sslot < S.n && S.key.w == key.w &&
          S.key.h == key.h && S.key.kind == 1 && S.rc == BRISK_HIP_OK)
        retained = S.d_frames.as<uint8_t>() + (size_t)sslot * S.frame_bytes;
    }
  }
  G.src_dev[slot] = retained;
  if (key.kind == 2) G.h_nin.as<int>()[slot] = nin;
  lk.unlock();
  clk.lap(0);
  // staging: plain CPU copies into pinned memory, every member on its own thread
  if (!retained) {
    uint8_t* dst = G.h_frames.as<uint8_t>() + (size_t)slot * G.frame_bytes;
    if (stride == G.dpitch) memcpy(dst, img, (size_t)G.dpitch * (key.h - 1) + key.w);
    else for (int y = 0; y < key.h; ++y) memcpy(dst + (size_t)y * G.dpitch, img + (size_t)y * stride, (size_t)key.w);
  }
  if (key.kind == 2 && nin > 0) memcpy(G.h_kin.as<brisk_hip_keypoint>() + (size_t)slot * G.kin_cap, kin, sizeof(brisk_hip_keypoint) * (size_t)nin);
  clk.lap(1);
  lk.lock();
  G.copied++;
  if (leader) {
    // close when a context is free to take the group; members keep joining until then
    int ci = -1;
    for (;;) {
      for (int c = 0; c < P->nctx && ci < 0; ++c)
        if (!P->busy[c]) ci = c;
      if (ci >= 0) break;
      P->cv.wait(lk);
    }
    P->busy[ci] = true;
    G.ci = ci;
    G.state = PG_CLOSED;
    G.seq = P->next_seq++;
    P->forming = -1;
    P->cv.notify_all();                                   // (callers of another kind may open their group now)
    while (G.copied < G.n) P->cv.wait(lk);                 // members still staging
    while (P->submit_seq != G.seq) P->cv.wait(lk);         // the groups' copies are queued in the order the groups closed
    P->stat_groups++;
    P->stat_frames += (unsigned long long)G.n;
    lk.unlock();
    clk.lap(2);
    unsigned ticket = 0;
    brisk_hip_ctx* ctx = P->ctx[ci];
    int rc = pool_submit_copies(P, G);
    lk.lock();
    P->submit_seq++;
    P->cv.notify_all();
    lk.unlock();
    clk.lap(3);
    if (!rc) rc = pool_submit_batch(P, G, &ticket);
    clk.lap(4);
    std::string err;
    if (rc) err = brisk_hip_last_error(ctx);
    if (!rc) {
      int flagged = 0;
      rc = brisk_hip_batch_download_wait(ctx, ticket, &flagged);
      if (rc == BRISK_HIP_ERR_CAPACITY) rc = BRISK_HIP_OK;  // per-frame flags: every member looks at its own
      if (rc) err = brisk_hip_last_error(ctx);
    }
    clk.lap(5);
    lk.lock();
    G.rc = rc;
    G.err = err;
    G.state = PG_DONE;
    P->busy[ci] = false;
    G.done_cv.notify_all();
    P->cv.notify_all();
  } else {
    if (G.state == PG_CLOSED && G.copied == G.n) P->cv.notify_all();  // (the leader is waiting for the last member's copy)
    while (G.state != PG_DONE) G.done_cv.wait(lk);
    clk.lap(6);
  }
  whole.lap(7);
  *gi_out = gi;
  *slot_out = slot;
  const int rc = G.rc;
  if (rc) tl_pool_err = G.err;
  return rc;
}

static void pool_leave(brisk_hip_pool* P, int gi) {
  std::lock_guard<std::mutex> lk(P->mu);
  PoolGroup& G = P->g[gi];
  if (--G.readers == 0) {
    // (the device frames stay where they are: a token is honoured until the buffer is prepared for another use.  A
    // buffer whose frames a forming describe group refers to cannot be prepared meanwhile: only one group forms at a
    // time, and the describe group's copies are queued - on the one copy stream - before the next use's)
    G.state = PG_FREE;
    P->cv.notify_all();
  }
}

static int pool_member_status(brisk_hip_pool* P, const PoolGroup& G, int slot) {
  const int fl = G.res.flags[slot];
  if (!fl) return BRISK_HIP_OK;
  if (fl & BRISK_HIP_ROWS_CUT) { tl_pool_err = "pool: the group's result rows were exhausted (brisk_hip_pool_create: max_keypoints)"; return BRISK_HIP_ERR_CAPACITY; }
  brisk_hip_ctx* ctx = P->ctx[G.ci];
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int rc = overflow_to_rc(ctx, fl);
  tl_pool_err = ctx->err;
  return rc;
}

extern "C" {

int brisk_hip_pool_create(int device, int max_batch, int max_keypoints, brisk_hip_pool** out) {
  if (!out) return BRISK_HIP_ERR_ARG;
  *out = nullptr;
  if (max_batch < 1 || max_batch > 64 || max_keypoints < 16) return BRISK_HIP_ERR_ARG;
  brisk_hip_pool* P = new brisk_hip_pool();
  P->device = device;
  P->maxb = max_batch;
  P->kp_cap = max_keypoints;
  if (const char* e = tuning_env("BRISK_POOL_CONTEXTS")) P->nctx = atoi(e) < 1 ? 1 : (atoi(e) > BRISK_POOL_CTX ? BRISK_POOL_CTX : atoi(e));  // experiments
  for (int c = 0; c < P->nctx; ++c) {
    int rc = brisk_hip_create(device, &P->ctx[c]);
    if (!rc) rc = brisk_hip_set_capacity(P->ctx[c], 4 * max_keypoints > 65536 ? 4 * max_keypoints : 65536, max_keypoints);
    if (rc) {
      for (int k = 0; k <= c; ++k) brisk_hip_destroy(P->ctx[k]);
      delete P;
      return rc;
    }
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&P->copy, hipStreamNonBlocking) != hipSuccess) {
    brisk_hip_pool_destroy(P);
    return BRISK_HIP_ERR_HIP;
  }
  // rows of a group's result buffers: every member may return a quarter of the capacity on average
  P->rows_per_group = (long long)max_batch * (max_keypoints / 4 > 4096 ? max_keypoints / 4 : 4096);
  *out = P;
  return BRISK_HIP_OK;
}

void brisk_hip_pool_destroy(brisk_hip_pool* P) {
  if (!P) return;
  (void)hipSetDevice(P->device);
  (void)hipDeviceSynchronize();
  for (PoolGroup& G : P->g)  // (the groups' buffers go with the pool, below)
    if (G.copied_ev) (void)hipEventDestroy(G.copied_ev);
  if (P->copy) (void)hipStreamDestroy(P->copy);
  for (brisk_hip_ctx* c : P->ctx) if (c) brisk_hip_destroy(c);
  delete P;
}

int brisk_hip_pool_stats(brisk_hip_pool* P, unsigned long long* groups, unsigned long long* calls) {
  if (!P) return BRISK_HIP_ERR_ARG;
  std::lock_guard<std::mutex> lk(P->mu);
  if (groups) *groups = P->stat_groups;
  if (calls) *calls = P->stat_frames;
  return BRISK_HIP_OK;
}

#ifdef BRISK_HIP_TUNING
// seconds per phase summed over all calls so far (PoolClock above); out holds 8 doubles
int brisk_hip_debug_pool_phases(brisk_hip_pool* P, double* out) {
  if (!P || !out) return BRISK_HIP_ERR_ARG;
  for (int i = 0; i < 8; ++i) out[i] = 1e-9 * (double)P->phase_ns[i].load(std::memory_order_relaxed);
  return BRISK_HIP_OK;
}
#endif

const char* brisk_hip_pool_last_error(const brisk_hip_pool* P) { return P ? tl_pool_err.c_str() : "null pool"; }

int brisk_hip_pool_detect(brisk_hip_pool* P, const uint8_t* img, int w, int h, int stride, int threshold, int octaves,
                          brisk_hip_keypoint* out, int cap, int* n, unsigned long long* image_token) {
  if (!P || !img || !n || cap < 0 || (cap > 0 && !out)) return BRISK_HIP_ERR_ARG;
  *n = 0;
  if (image_token) *image_token = 0;
  if (w <= 0 || h <= 0 || w > 8191 || h > 8191 || stride < w || octaves < 0 || 2 * octaves > BRISK_MAX_LAYERS) return BRISK_HIP_ERR_ARG;
  if (threshold < 1 || threshold > 255) return BRISK_HIP_ERR_THRESHOLD;
  PoolKey key;
  key.kind = 1; key.w = w; key.h = h; key.threshold = threshold; key.octaves = octaves;
  int gi = -1, slot = -1;
  int rc = pool_run(P, key, img, stride, 0ull, nullptr, 0, &gi, &slot);
  if (gi < 0) return rc;
  PoolGroup& G = P->g[gi];
  if (!rc) rc = pool_member_status(P, G, slot);
  if (!rc) {
    const long long a = G.res.offsets[slot], cnt = G.res.offsets[slot + 1] - a;
    *n = (int)cnt;
    if (cnt > cap) {
      tl_pool_err = "output keypoint buffer too small";
      rc = BRISK_HIP_ERR_CAPACITY;
    } else if (cnt > 0) {
      memcpy(out, G.res.kps + a, sizeof(brisk_hip_keypoint) * (size_t)cnt);
    }
    if (image_token) *image_token = pool_token(gi, G.gen, slot);
  }
  pool_leave(P, gi);
  return rc;
}

int brisk_hip_pool_describe(brisk_hip_pool* P, const brisk_hip_pattern* pat, const uint8_t* img, int w, int h, int stride,
                            brisk_hip_keypoint* kps, int* n, uint8_t* desc, int desc_stride, int rotation_invariant,
                            int scale_invariant, unsigned long long image_token) {
  if (!P || !pat || !img || !n || *n < 0 || (*n > 0 && (!kps || !desc))) return BRISK_HIP_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 8191 || h > 8191 || stride < w) return BRISK_HIP_ERR_ARG;
  const int strings = pat->host.strings;
  if (*n > 0 && desc_stride < strings) return BRISK_HIP_ERR_ARG;
  if (*n > P->kp_cap) return BRISK_HIP_ERR_CAPACITY;
  PoolKey key;
  key.kind = 2; key.w = w; key.h = h; key.pat = pat; key.rot = rotation_invariant ? 1 : 0; key.scl = scale_invariant ? 1 : 0;
  const int nin = *n;
  int gi = -1, slot = -1;
  int rc = pool_run(P, key, img, stride, image_token, kps, nin, &gi, &slot);
  if (gi < 0) return rc;
  PoolGroup& G = P->g[gi];
  if (!rc) rc = pool_member_status(P, G, slot);
  if (!rc) {
    const long long a = G.res.offsets[slot], cnt = G.res.offsets[slot + 1] - a;
    *n = (int)cnt;
    if (cnt > 0) {
      memcpy(kps, G.res.kps + a, sizeof(brisk_hip_keypoint) * (size_t)cnt);
      const int rs = G.res.desc_stride;
      const uint8_t* src = G.res.desc + (size_t)a * rs;
      if (rs == desc_stride && strings == rs) memcpy(desc, src, (size_t)cnt * rs);
      else for (long long i = 0; i < cnt; ++i) memcpy(desc + (size_t)i * desc_stride, src + (size_t)i * rs, (size_t)strings);
    }
  }
  pool_leave(P, gi);
  return rc;
}

}  // extern "C"
