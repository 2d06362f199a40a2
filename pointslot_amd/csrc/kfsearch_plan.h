// Device-side descriptors of the keyframe projection searches (kfsearch_kernels.hip): ps_kf_search and ps_search_by_sim3.
// Every search of a batch - one ps_kf_search problem, or one direction of a ps_search_by_sim3 problem - is one KsJob.
#pragma once
#include <stdint.h>
#include "match_plan.h"

#define PS_KS_MAX_N 8191        // features per searched side: the index field of a candidate key holds 13 bits
#define PS_KS_MAX_NQ 32768      // points per problem
#define PS_KS_CAP 32            // candidates kept per query in the everyday store (only those that can ever be taken are kept)
#define PS_KS_CAP_WIDE 1024     // ... in the store of the re-run of the problems that overflowed the first one (10 position bits)
#define PS_KS_IDXB 13

// kind: 0 SearchByProjection(pKF, Scw, ..)   ordered, gates z / image (exclusive) / distance / viewing angle, levels [l-1, l]
//       1 Fuse(pKF, Scw, ..)                 independent, the same gates
//       2 SearchByProjection(F, pKF, ..)     ordered, gates image (inclusive) / distance, levels [l-1, l+1], rotation histogram
//       3 one direction of SearchBySim3      independent, two-step transform, gates z / image (exclusive) / distance of the camera-frame point
struct KsJob {
  int32_t t_off, nt;           // searched side
  int32_t q_off, nq;           // points
  int32_t grid_off;            // into cell_off (COLS*ROWS+1 entries per job); cell_idx shares t_off
  int32_t c_off, cap;          // ordered kinds: first query's slot in the candidate store, and the store's row length
  int32_t kind;
  float min_x, min_y, gw_inv, gh_inv;
  float R[9], t[3], ow[3];
  float R2[9], t2[3];          // kind 3: sR21 / t21 (or sR12 / t12) applied to R X + t
  float fx, fy, cx, cy;
  float bounds[4];             // mnMinX, mnMaxX, mnMinY, mnMaxY
  float scale[8];
  float log_scale;
  int32_t n_levels;
  float th;
  int32_t th_dist;
  int32_t check_ori;
  int32_t pad;
};

// the two jobs of one Sim3 problem, for the agreement pass
struct KsPair { int32_t q1_off, n1, q2_off, n2; };

struct KsArrays {
  const KsJob* job;
  // searched side
  const float* tx; const float* ty; const int32_t* toct; const float* tang; const uint8_t* tdesc; const uint8_t* tocc;
  const int32_t* cell_off; const int32_t* cell_idx;
  // points
  const uint8_t* qvalid; const float* qpos; const float* qnormal; const float* qmin; const float* qmax; const uint8_t* qdesc;
  const float* qang;
  // outputs / work
  int32_t* best_idx; int32_t* best_dist;     // per query (independent kinds)
  uint32_t* cand; int32_t* ncand; uint32_t* qtop;   // per query (ordered kinds): kept candidates, their number, the smallest key
  int32_t* match; int32_t* nmatch;           // per train slot / per job (ordered kinds)
  int32_t* overflow;                         // per job: queries that kept more candidates than the store's row holds
  // Sim3 agreement
  const KsPair* pair; int32_t* match12; int32_t* nfound;
};
