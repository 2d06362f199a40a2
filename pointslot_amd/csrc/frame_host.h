// The frame handle as the host side of the library sees it: frame_host.hip owns it, match_host.hip consumes it.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include "frame_plan.h"

struct ps_frame {
  std::mutex mu;                  // event bookkeeping; a publish holds it while it queues, a consumer while it queues its staging copy
  int device = 0;
  int capacity = 0;
  int n = 0;                      // keypoints of the last publish, as the publisher stated them
  int prev_n = 0;                 // the most the slab has held since it was last cleared behind n
  float grid[4] = {0, 0, 0, 0};   // mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv of the last publish
  bool published = false;
  hipStream_t stream = nullptr;
  hipEvent_t ev_ready = nullptr;  // recorded behind every publish; consumers' streams wait on it
  hipEvent_t ev_src = nullptr;    // the extractor's stream as of ps_frame_publish_orb
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;   // around the last publish (ps_frame_last_publish_ms)
  // "last use": one event per consumer (a matcher handle) that has read the slab.  A consumer that finds no slot of its own takes
  // the oldest one and first makes its stream wait on the event there, so waiting on all slots still covers every earlier reader.
  static const int USES = 8;
  hipEvent_t ev_use[USES] = {};
  const void* user[USES] = {};
  unsigned long long use_seq[USES] = {};
  unsigned long long seq = 0;
  uint8_t* d_slab = nullptr;
  size_t slab_bytes = 0;
  uint8_t* h_stage = nullptr;     // pinned: keypoints | u_right | descriptors of ps_frame_publish_host, uploaded in one piece
  size_t stage_bytes = 0;
  uint8_t* d_stage = nullptr;     // where that upload lands (inside the slab)
  FrameSlab slab = {};
};

// The frames of one search call, each once.  begin: locks them (in address order) and makes `st` wait for their publishes;
// end: records "last use" on `st` for `consumer` and unlocks.  Between the two the caller queues its frame_stage launch.
int psf_consume_begin(ps_frame* const* uniq, int n, hipStream_t st);
int psf_consume_end(ps_frame* const* uniq, int n, const void* consumer, hipStream_t st, bool record);

// what ps_frame_publish_orb needs of an extractor handle (orb_host.hip)
struct PsOrbView {
  const ps_keypoint* d_kps; const uint8_t* d_desc; const int32_t* d_counts; const float* d_uright;
  int kp_cap, max_batch, device, planned;
  hipStream_t stream;
};
extern "C" int psk_orb_view(ps_orb* h, PsOrbView* v);
