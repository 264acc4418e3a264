// brisk_transfer.h - host code only: the asynchronous transfers to host memory behind brisk_hip_batch_download_all,
// brisk_hip_pair_matches_download and brisk_hip_tracks_download - the slot of one transfer, the ring of two an exit keeps in flight,
// tickets and waits.
// (No device compiler output depends on this file: build.kernel_revision() leaves it out, like brisk_capi.hip.)
// A context is not known here: the calls are given its device, its error string and its lock.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <string>

#include "../../include/brisk_hip.h"
#include "brisk_hostmem.h"

static int transfer_fail(std::string& err, int code, const std::string& msg) { err = msg; return code; }
#define TRANSFER_HIPCHK(err, call)                                                                                        \
  do {                                                                                                                    \
    hipError_t e_ = (call);                                                                                               \
    if (e_ != hipSuccess) return transfer_fail(err, BRISK_HIP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Can the device write to this address?  Pinned / registered host memory, managed and device memory: yes (through the
// device-side alias the runtime reports); pageable host memory: no - the transfer then lands in the slot's pinned bounce
// buffer and the wait copies it out.
static bool device_can_write(const void* p, void** dev) {
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof a);
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // (an unregistered pointer is an error on older runtimes, hipMemoryTypeUnregistered on newer ones)
    return false;
  }
  if (a.type != hipMemoryTypeHost && a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged && a.type != hipMemoryTypeUnified)
    return false;
  *dev = a.devicePointer ? a.devicePointer : const_cast<void*>(p);
  return true;
}
// Can it write every destination array a transfer fills (`required`; the others become null)?  Then each p becomes its device-side
// alias; no at the first array out of reach.  known_pinned: the arrays come from hipHostMalloc - no pointer query is made.
struct HostDst {
  void* p;
  bool required;
};
template <size_t N>
static bool device_can_write_all(HostDst (&d)[N], bool known_pinned = false) {
  if (known_pinned) return true;
  for (HostDst& x : d) {
    void* dev = nullptr;
    if (x.required && !device_can_write(x.p, &dev)) return false;
    x.p = dev;
  }
  return true;
}

// One transfer: pack kernels fill `slab` on the batch's stream (`packed` behind them), an egress kernel on a second stream moves
// the exact bytes to the host (`done` behind it).  Arrays: the exit's destination struct (brisk_hip_batch_host_results,
// brisk_hip_pair_host_matches) or a struct around it (the tracks exit's TrackTransfer); its int array `flags` has one entry per
// frame / pair / list, nonzero = flagged.
template <class Arrays>
struct TransferSlot {
  DeviceBuf slab;
  PinnedBuf bounce;  // staging for destinations the device cannot write (pageable memory)
  hipEvent_t packed = nullptr, done = nullptr;
  bool done_valid = false;  // `done` has been recorded: the slab is in use until it fires
  bool pending = false;     // the transfer has not been completed by a wait yet
  bool use_bounce = false;
  unsigned ticket = 0;
  int n = 0;     // frames / pairs of the transfer
  Arrays dst{};  // the caller's destinations
  Arrays wr{};   // where the host finds what the egress kernel wrote (the caller's arrays, or the bounce buffer)
  int rc = BRISK_HIP_OK, flagged = 0;
  std::string msg;
};

// The egress kernel of slot E has finished (the context's lock held): counts the flagged entries and completes the slot.  The
// exit's own part: copy_out(E) moves its arrays out of the bounce buffer to E.dst; status(E, flags_or) - called when something is
// flagged, E.flagged set, flags_or the OR of all flags - turns flags into E.rc and E.msg.
template <class Slot, class CopyOut, class Status>
static void transfer_finish(Slot& E, CopyOut copy_out, Status status) {
  int flagged = 0, flags_or = 0;
  for (int i = 0; i < E.n; ++i)
    if (E.wr.flags[i]) { ++flagged; flags_or |= E.wr.flags[i]; }
  if (E.use_bounce) copy_out(E);
  E.pending = false;
  E.flagged = flagged;
  E.rc = BRISK_HIP_OK;
  E.msg.clear();
  if (flagged) status(E, flags_or);
}

// The two slots of one exit and its ticket sequence.  Two, so that a stream keeps two batches in flight: the transfer of one runs
// beside the kernels of the next.  Each exit has its own ring (a stream that downloads rows, matches AND tracks still keeps two
// batches in flight) and its own tickets.  Every call is made with the context's lock held; finish(slot) is the exit's transfer_finish.
template <class Arrays>
struct TransferRing {
  using Slot = TransferSlot<Arrays>;
  Slot slots[2];
  unsigned seq = 0;  // the last ticket issued

  // *out = the slot of the next transfer, its slab holding `slab_bytes`: free of its previous occupant, the events created
  template <class Finish>
  int open(size_t slab_bytes, std::string& err, Finish finish, Slot** out) {
    Slot& E = slots[(seq + 1) & 1];
    if (!E.packed) {
      TRANSFER_HIPCHK(err, hipEventCreateWithFlags(&E.packed, hipEventDisableTiming));
      TRANSFER_HIPCHK(err, hipEventCreateWithFlags(&E.done, hipEventDisableTiming));
    }
    if (E.pending) {  // a third transfer in flight: complete the oldest first
      TRANSFER_HIPCHK(err, hipEventSynchronize(E.done));
      finish(E);
    }
    if (slab_bytes > E.slab.cap) {
      if (E.done_valid) TRANSFER_HIPCHK(err, hipEventSynchronize(E.done));
      TRANSFER_HIPCHK(err, E.slab.grow(slab_bytes));
    }
    *out = &E;
    return BRISK_HIP_OK;
  }
  // the egress kernel of E is queued on `es`, E.dst / E.wr are set: `done` behind it, the transfer in flight under a new ticket
  int close(Slot& E, hipStream_t es, bool use_bounce, int n, std::string& err, unsigned* ticket) {
    TRANSFER_HIPCHK(err, hipEventRecord(E.done, es));
    E.done_valid = true;
    E.pending = true;
    E.use_bounce = use_bounce;
    E.n = n;
    E.ticket = ++seq;
    if (!E.ticket) E.ticket = ++seq;  // (0 is never a ticket)
    *ticket = E.ticket;
    return BRISK_HIP_OK;
  }
  // Completes the transfers up to `ticket`, oldest first, and reports `ticket`'s outcome.  The lock is held through `lk` and
  // released while the host waits for the device.  name: the head of the messages.
  template <class Finish>
  int wait(int device, std::string& err, std::unique_lock<std::mutex>& lk, unsigned ticket, int* flagged, Finish finish, const char* name) {
    if (flagged) *flagged = 0;
    if (hipSetDevice(device) != hipSuccess) return transfer_fail(err, BRISK_HIP_ERR_HIP, "hipSetDevice failed");
    for (int pass = 0; pass < 2; ++pass) {
      Slot* E = nullptr;
      for (Slot& X : slots)
        if (X.pending && (int)(X.ticket - ticket) <= 0 && (!E || (int)(X.ticket - E->ticket) < 0)) E = &X;
      if (!E) break;
      const unsigned t = E->ticket;
      hipEvent_t ev = E->done;
      lk.unlock();
      const hipError_t e = hipEventSynchronize(ev);
      lk.lock();
      if (e != hipSuccess) return transfer_fail(err, BRISK_HIP_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
      if (E->pending && E->ticket == t) finish(*E);  // (unless another thread completed it meanwhile)
    }
    for (Slot& X : slots)
      if (X.ticket == ticket && ticket != 0 && !X.pending) {
        if (flagged) *flagged = X.flagged;
        if (X.rc) err = X.msg;
        return X.rc;
      }
    return transfer_fail(err, BRISK_HIP_ERR_ARG, std::string(name) + ": unknown ticket (never issued on this context, or two later transfers have replaced it)");
  }
  void destroy_events() {  // (with the context, once the device is idle; the buffers go with their owners)
    for (Slot& E : slots) {
      if (E.packed) hipEventDestroy(E.packed);
      if (E.done) hipEventDestroy(E.done);
    }
  }
};
