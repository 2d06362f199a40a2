// Device-side descriptors of the keyframe database (kfdb_kernels.hip): the forward store and the arrays of one add / query / score call.
#pragma once
#include <stdint.h>
#define PS_KFDB_MAX_WORDS 8191      // words of a stored or a query BowVector: the query's ids live in LDS (32 KB)
#define PS_KFDB_MAX_CAPACITY 4096   // live keyframes: kfdb_list sorts the sharing slots of a query in LDS (12 B per slot)

// The forward store.  A slot holds one keyframe: its BowVector as two rows (ids ascending; values), its length, the serial of
// its add (monotone over the life of the database, 0 = free slot), the caller's id and the model of KeyFrame::mRelocScore.
struct KfdbStore {
  int32_t* ids;        // [capacity][stride]
  double* vals;        // [capacity][stride]
  int32_t* len;        // [capacity]; 0 for a free slot
  uint32_t* serial;    // [capacity]
  int64_t* kfid;       // [capacity]
  float* reloc;        // [capacity]
  int32_t stride;      // max_words rounded up to 64
  int32_t high;        // slots in use lie in [0, high)
};

// ps_kfdb_add: entry e goes to slot[e]; its vector is src_id / src_val [off[e], off[e] + n[e])
struct KfdbAddArrays {
  KfdbStore S;
  const int32_t* slot; const int32_t* off; const int32_t* n;
  const uint32_t* serial; const int64_t* kfid;
  const int32_t* src_id; const double* src_val;
};

// one query of a ps_kfdb_query call; its BowVector is qid / qval [off, off + n)
struct KfdbQuery {
  int32_t off, n, mode;
  int32_t excl;        // mode 1: first word of its exclusion bitmask (bit s: slot s is a connected keyframe); -1: none
};
struct KfdbQueryArrays {
  KfdbStore S;
  const KfdbQuery* q;
  const int32_t* qid; const double* qval;
  const uint32_t* excl;
  const int32_t* order;          // workgroup o of kfdb_list serves query order[o]: the nloop mode-1 queries, then the mode-0 queries in array order
  int32_t nq, nloop, out_stride;
  int32_t spw;                   // slots per wave of kfdb_count
  int32_t* words;                // [nq][high] common words (0: shares none, or excluded)
  int32_t* lcw;                  // [nq][high] least common word
  float* score;                  // [nq][high] fresh score where words > min_common_words
  int32_t* maxw;                 // [nq], zeroed before the call
  int64_t* share_id; int32_t* share_words; float* share_score;   // [nq][out_stride]
  int32_t* nshare; int32_t* mincw;                               // [nq]
};

// ps_kfdb_score: the query against the named slots (-1: unknown id, NaN)
struct KfdbScoreArrays {
  KfdbStore S;
  const int32_t* qid; const double* qval; int32_t qn;
  const int32_t* slot; int32_t n;
  double* out;
};
