// Device-side descriptors of the frame handle (ps_frame): the slab a published frame lives in, one publish job, one staging job.
#pragma once
#include <stdint.h>
#include "../../include/pointslot_hip.h"
#include "match_plan.h"

#define PS_FRAME_NCELL (PS_GRID_COLS * PS_GRID_ROWS)
#define PS_FRAME_MAX_N 32767          // a candidate key's index field (match_kernels.hip) holds 15 bits
#define PS_FRAME_PUB_THREADS 256      // frame_publish: 4 waves, each owns a contiguous quarter of the keypoints
#define PS_FRAME_PUB_WAVES (PS_FRAME_PUB_THREADS / 64)
#define PS_FRAME_PUB_BATCH 16         // frames per frame_publish launch (jobs travel by value in the kernel arguments)

// header of a slab, written by frame_publish
struct FrameHdr {
  int32_t n;          // keypoints the slab holds
  int32_t mismatch;   // the publisher's n differed from the extractor's count (ps_frame_publish_orb)
  int32_t pad[2];
};

// device pointers into one frame's slab (all 16-byte aligned)
struct FrameSlab {
  FrameHdr* hdr;
  float* x; float* y; int32_t* octave; float* angle; float* u_right;
  uint8_t* desc;                      // [n][32]
  int32_t* cell_off;                  // [PS_FRAME_NCELL + 1]
  int32_t* cell_idx;                  // [capacity]; entries beyond cell_off[NCELL] are zero up to n
};

struct FramePubJob {
  FrameSlab dst;
  const ps_keypoint* kps;             // AoS source: the staged host upload or the extractor's output rows
  const float* u_right;               // nullptr: monocular, all -1
  const uint8_t* desc;                // 16-byte aligned
  const int32_t* count;               // nullptr, or the device-side keypoint count n is clamped to
  int32_t n, prev_n, capacity, pad;
  float min_x, min_y, gw_inv, gh_inv;
};
struct FramePubBatch { FramePubJob job[PS_FRAME_PUB_BATCH]; };

// frame_stage: the train side of one problem, copied from a slab to where the search kernels read it in the matcher's arena
struct FrameStageJob {
  FrameSlab src;
  int32_t nt, t_off, grid_off, prob;
};
struct FrameStageDst {
  float* tx; float* ty; int32_t* toct; float* tang; float* tur; uint8_t* tdesc;   // tang may be nullptr (the fuse search has none)
  int32_t* cell_off; int32_t* cell_idx;                                           // both may be nullptr (a consumer without the grid: tri_match)
  int32_t* status;                    // per problem: non-zero where the slab does not hold the frame the caller described
};
