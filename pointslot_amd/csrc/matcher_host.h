// The matcher handle as the host side of the library sees it, and what the calls that run on it share: match_host.hip owns the
// handle; search_host.hip, kfsearch_host.hip, tri_host.hip, bow_host.hip and kfdb_host.hip run their calls on it.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <stdint.h>
#include <vector>
#include "frame_host.h"
#include "ps_common.h"
#include "search_side.h"   // al, Arena, ptr and the searched side

struct ps_matcher {
  std::mutex mu;              // calls on one handle are serialised (a handle may be shared by threads)
  int device = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_buf = nullptr;   // one growable device arena
  size_t d_bytes = 0;
  uint8_t* h_buf = nullptr;   // pinned staging of the same size
  size_t h_bytes = 0;
  uint8_t* d_wide = nullptr;  // second arena, only for the wide re-run of search problems whose windows overflowed the candidate store
  size_t d_wide_bytes = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the kernels of the last brute-force / projection / triangulation / bag-of-words call (ps_matcher_last_kernel_ms)
  float last_kernel_ms = 0;
};

// grow both arenas / the second arena to at least that many bytes (contents are lost); PS_OK or PS_ERR_HIP
int psm_ensure(ps_matcher* m, size_t need);
int psm_ensure_wide(ps_matcher* m, size_t bytes);

// The kernels of a call, between the two events ps_matcher_last_kernel_ms reads: begin, the launches, end (which also reports a failed
// launch); psm_kernels_ms once the call's read-back has synchronised the stream.
inline int psm_kernels_begin(ps_matcher* m) { PS_HIP(hipEventRecord(m->ev0, m->stream)); return PS_OK; }
inline int psm_kernels_end(ps_matcher* m) { PS_HIP(hipEventRecord(m->ev1, m->stream)); PS_HIP(hipGetLastError()); return PS_OK; }
inline int psm_kernels_ms(ps_matcher* m) { PS_HIP(hipEventElapsedTime(&m->last_kernel_ms, m->ev0, m->ev1)); return PS_OK; }

// The frame-backed problems of one call and the whole protocol around frame_stage.  A call declares every problem it launches with
// add(): either that queues a staging job, or it returns false, the caller packs the side from the host arrays (side_pack) and the
// whole input is uploaded.  Only when every declared problem is staged does upload() leave the skip ranges out - so a searched side
// is uploaded or staged, never neither.
struct FrameUse {
  std::vector<ps_frame*> of;        // per problem, nullptr = host arrays
  std::vector<ps_frame*> uniq;      // the handles, each once in locking order
  std::vector<float> grid;          // [nprob][4]: what the handles said when the call looked
  bool any() const { return !uniq.empty(); }
  int init(ps_matcher* m, ps_frame* const* frames, int nprob, const char* what);   // frames may be nullptr; what: the call's name in error texts
  int check(int p, int train_n, const char* what);                                  // train_n against problem p's handle; fills grid
  template <typename Prob> void grid_into(Prob& d, int p, const ps_proj_train& T) const {   // problem p's grid parameters: the handle's over the caller's
    const float own[4] = {T.min_x, T.min_y, T.grid_w_inv, T.grid_h_inv}, *g = of[p] ? &grid[(size_t)p * 4] : own;
    d.min_x = g[0]; d.min_y = g[1]; d.gw_inv = g[2]; d.gh_inv = g[3];
  }
  bool staged(int p, int n) const { return of[p] && n > 0; }
  // declares problem p (device slot `slot`): n features at t_off, its grid at grid_off; true: staged from its handle
  bool add(int p, int slot, int n, int32_t t_off, int32_t grid_off) {
    if (staged(p, n)) jobs.push_back(FrameStageJob{of[p]->slab, n, t_off, grid_off, slot});
    else needs_host = true;
    return staged(p, n);
  }
  // The job slots, last of the input side, and the status slots on the read-back side: they exist only in a call that uses a handle.
  // Both return where the arena stands behind them.
  size_t reserve_jobs(Arena& a, int nslot) { nslots = nslot; o_jobs = any() ? a.take(sizeof(FrameStageJob) * nslot) : 0; return a.off; }
  size_t reserve_status(Arena& a) { o_status = any() ? a.take((size_t)nslots * 4) : 0; return a.off; }
  int upload(ps_matcher* m, uint8_t* H, uint8_t* D, size_t in_bytes, const SideSkip& skip);   // H -> D: [0, in_bytes) whole, or without `skip`
  int stage(ps_matcher* m, uint8_t* D, const SideOff& o);   // behind the upload: the slabs' sides land where host arrays would have
  // after the read-back: the slab did not hold the frame the caller described for the problem in `slot`
  bool stale(const uint8_t* H, int slot) const { return any() && reinterpret_cast<const int32_t*>(H + o_status)[slot] != 0; }
 private:
  std::vector<FrameStageJob> jobs;
  bool needs_host = false;
  int nslots = 0; size_t o_jobs = 0, o_status = 0;   // the slots of reserve_jobs / reserve_status
};

// PS_ERR_INVALID for a stale handle; more < 0: no "(and N more)", n < 0: the count is not named
int frame_stale_error(const char* what, int p, long more, int n);
