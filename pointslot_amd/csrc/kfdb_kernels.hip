// Kernels of the keyframe database (include/pointslot_hip.h: ps_kfdb): KeyFrameDatabase::DetectLoopCandidates /
// DetectRelocalizationCandidates up to the scored sharing list (src/KeyFrameDatabase.cc:77-140, :200-254 of the reference) and
// L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) over a forward store: one row of word ids and
// one row of values per keyframe, no inverted file.  Everything here is integer counting, one double sum in a fixed order and
// float compares: the results are the reference's bit for bit (the file is compiled with -ffp-contract=off).
//   kfdb_count : one wave per (query, slot).  The query's ids sit in LDS; the lanes take the slot's ids 64 at a time and
//                binary-search them; a ballot gives the chunk's hits.  words = the popcounts; the least common word = the first
//                hit; an integer atomicMax per query gives maxCommonWords.  Reads ids only.
//   kfdb_score : minCommonWords from that maximum, on the device.  One wave per slot that passes: the same intersection, now
//                with the two values of every hit; the terms are added in ascending word order by ONE accumulator (the set bits
//                of the ballot walked with a lane read) - the order of the additions is part of the result.
//   kfdb_list  : one workgroup per query: the sharing slots sorted by (least common word, serial) in LDS - the order in which the
//                reference's walk over the inverted file meets them first - and the output lists.  reloc_score as relocalisation
//                query q of a call sees it is the score of the last relocalisation query up to q that scored the slot, else
//                the stored value: every query resolves that by itself from the scores of the call, so the queries of a call
//                run side by side and still see what the earlier ones left.
//   kfdb_commit: the stored reloc_score after the call: per slot the score of the last relocalisation query that scored it.
#include <hip/hip_runtime.h>
#include "kfdb_plan.h"

#define KFDB_T 256                 // 4 waves.  A workgroup of kfdb_count loads the query once for 4 * spw slots, spw per wave (1 for
                                   // a small call, so that there are enough waves to hide the LDS searches; 4 for a batch)
#define KFDB_LIST_T 1024

extern __shared__ int32_t kfdb_q[];    // the query's word ids, ascending

// position of e in q[0, n) or -1
__device__ inline int kfdb_find(const int32_t* q, int n, int32_t e) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (q[mid] < e) lo = mid + 1; else hi = mid;
  }
  return lo < n && q[lo] == e ? lo : -1;
}

__device__ inline void kfdb_load_query(const int32_t* src, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) kfdb_q[i] = src[i];
  __syncthreads();
}

// one wave: the number of words of ids[0, len) that the query holds, and the least of them (-1: none); len is wave-uniform
__device__ inline int kfdb_wave_count(int qn, const int32_t* ids, int len, int lane, int& least) {
  int words = 0;
  least = -1;
  for (int c = 0; c < len; c += 64) {
    const int i = c + lane;
    const int32_t e = i < len ? ids[i] : -1;
    const unsigned long long hits = __ballot(i < len && kfdb_find(kfdb_q, qn, e) >= 0);
    if (hits && least < 0) least = __shfl(e, __ffsll((long long)hits) - 1);
    words += __popcll(hits);
  }
  return words;
}

// lane l's value of v, l wave-uniform: two register reads, no trip through LDS
__device__ inline double kfdb_lane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// one wave: the sum of L1Scoring::score before its `-score/2.0`: fabs(vi - wi) - fabs(vi) - fabs(wi) over the common words in
// ascending word id, one addition after the other (vi the query's value).  Every lane returns the sum.
__device__ inline double kfdb_wave_sum(int qn, const double* qval, const int32_t* ids, const double* vals, int len, int lane) {
  double acc = 0;
  int32_t e_next = lane < len ? ids[lane] : -1;
  double w_next = lane < len ? vals[lane] : 0.0;
  for (int c = 0; c < len; c += 64) {
    const int i = c + lane;
    const int32_t e = e_next;
    const double wi = w_next;
    if (i + 64 < len) { e_next = ids[i + 64]; w_next = vals[i + 64]; }            // the next chunk is on its way during the sum
    const int pos = i < len ? kfdb_find(kfdb_q, qn, e) : -1;
    double term = 0;
    if (pos >= 0) {
      const double vi = qval[pos];
      term = fabs(vi - wi) - fabs(vi) - fabs(wi);
    }
    unsigned long long hits = __ballot(pos >= 0);
    while (hits) {                                  // ascending lanes = ascending word ids
      acc += kfdb_lane(term, __ffsll((long long)hits) - 1);
      hits &= hits - 1;
    }
  }
  return acc;
}

__device__ inline int kfdb_min_common(int max_common) { return (int)((float)max_common * 0.8f); }   // `int minCommonWords = maxCommonWords*0.8f;`

__global__ __launch_bounds__(256) void kfdb_put(KfdbAddArrays A) {
  const int e = blockIdx.x, s = A.slot[e], n = A.n[e];
  const size_t row = (size_t)s * A.S.stride, off = (size_t)A.off[e];
  for (int i = threadIdx.x; i < n; i += 256) {
    A.S.ids[row + i] = A.src_id[off + i];
    A.S.vals[row + i] = A.src_val[off + i];
  }
  if (threadIdx.x == 0) { A.S.len[s] = n; A.S.serial[s] = A.serial[e]; A.S.kfid[s] = A.kfid[e]; A.S.reloc[s] = 0.f; }
}

__global__ __launch_bounds__(KFDB_T) void kfdb_count(KfdbQueryArrays A) {
  const int qi = blockIdx.y, high = A.S.high;
  const KfdbQuery Q = A.q[qi];
  kfdb_load_query(A.qid + Q.off, Q.n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int most = 0;
  for (int k = 0; k < A.spw; k++) {
    const int s = (blockIdx.x * A.spw + k) * 4 + wave;        // wave-uniform
    if (s >= high) break;
    int len = A.S.len[s];
    if (Q.excl >= 0 && ((A.excl[Q.excl + (s >> 5)] >> (s & 31)) & 1u)) len = 0;   // spConnectedKeyFrames: never listed, never counted
    int least;
    const int words = kfdb_wave_count(Q.n, A.S.ids + (size_t)s * A.S.stride, len, lane, least);
    if (lane == 0) { A.words[(size_t)qi * high + s] = words; A.lcw[(size_t)qi * high + s] = least; }
    most = max(most, words);
  }
  if (lane == 0 && most > 0) atomicMax(&A.maxw[qi], most);
}

__global__ __launch_bounds__(KFDB_T) void kfdb_score(KfdbQueryArrays A) {
  const int qi = blockIdx.y, high = A.S.high;
  const int mincw = kfdb_min_common(A.maxw[qi]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.x * 4 + wave;
  const int pass = s < high && A.words[(size_t)qi * high + s] > mincw;
  if (!__syncthreads_or(pass)) return;               // nothing to score here: leave before loading the query
  const KfdbQuery Q = A.q[qi];
  kfdb_load_query(A.qid + Q.off, Q.n);
  if (!pass) return;
  const size_t row = (size_t)s * A.S.stride;
  const double acc = kfdb_wave_sum(Q.n, A.qval + Q.off, A.S.ids + row, A.S.vals + row, A.S.len[s], lane);
  if (lane == 0) A.score[(size_t)qi * high + s] = (float)(-acc / 2.0);            // `float si = mpVoc->score(...)`
}

// pKF->mRelocScore of slot s as the relocalisation query at place o of order[] reads it after its own scoring stage: what the last
// relocalisation query up to o that scored the slot wrote (`pKFi->mRelocScore = si`), else the value stored before the call
__device__ inline float kfdb_reloc_seen(const KfdbQueryArrays& A, int o, int s) {
  for (; o >= A.nloop; o--) {
    const int qi = A.order[o];
    if (A.words[(size_t)qi * A.S.high + s] > kfdb_min_common(A.maxw[qi])) return A.score[(size_t)qi * A.S.high + s];
  }
  return A.S.reloc[s];
}

__global__ __launch_bounds__(KFDB_LIST_T) void kfdb_list(KfdbQueryArrays A) {
  __shared__ unsigned long long key[PS_KFDB_MAX_CAPACITY];
  __shared__ int32_t slot[PS_KFDB_MAX_CAPACITY];
  __shared__ int cnt;
  const int tid = threadIdx.x, high = A.S.high;
  const int o = blockIdx.x;                        // order[]: the loop queries, then the relocalisation queries in array order
  const int qi = A.order[o];
  const int mode = A.q[qi].mode;
  const int mincw = kfdb_min_common(A.maxw[qi]);
  const int32_t* W = A.words + (size_t)qi * high;
  const int32_t* L = A.lcw + (size_t)qi * high;
  const float* SC = A.score + (size_t)qi * high;
  if (tid == 0) cnt = 0;
  __syncthreads();
  for (int s = tid; s < high; s += KFDB_LIST_T) {
    const int w = W[s];
    if (w <= 0) continue;
    const int p = atomicAdd(&cnt, 1);
    key[p] = ((unsigned long long)(uint32_t)L[s] << 32) | A.S.serial[s];
    slot[p] = s;
  }
  __syncthreads();
  const int n = cnt;
  int np = 1;
  while (np < n) np <<= 1;
  for (int i = n + tid; i < np; i += KFDB_LIST_T) { key[i] = ~0ull; slot[i] = -1; }
  __syncthreads();
  for (int k = 2; k <= np; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < np; i += KFDB_LIST_T) {
        const int x = i ^ j;
        if (x > i) {
          const unsigned long long a = key[i], b = key[x];
          if ((a > b) == ((i & k) == 0)) {
            key[i] = b; key[x] = a;
            const int32_t t = slot[i]; slot[i] = slot[x]; slot[x] = t;
          }
        }
      }
      __syncthreads();
    }
  const size_t out = (size_t)qi * A.out_stride;
  for (int i = tid; i < n; i += KFDB_LIST_T) {
    const int s = slot[i], w = W[s];
    A.share_id[out + i] = A.S.kfid[s];
    A.share_words[out + i] = w;
    A.share_score[out + i] = mode == 0 ? kfdb_reloc_seen(A, o, s) : (w > mincw ? SC[s] : 0.f);
  }
  if (tid == 0) { A.nshare[qi] = n; A.mincw[qi] = mincw; }
}

__global__ __launch_bounds__(256) void kfdb_commit(KfdbQueryArrays A) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < A.S.high && A.nq > A.nloop) A.S.reloc[s] = kfdb_reloc_seen(A, A.nq - 1, s);
}

__global__ __launch_bounds__(KFDB_T) void kfdb_score_slots(KfdbScoreArrays A) {
  kfdb_load_query(A.qid, A.qn);
  const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= A.n) return;
  const int s = A.slot[e];
  if (s < 0) { if (lane == 0) A.out[e] = __longlong_as_double(0x7FF8000000000000ll); return; }
  const size_t row = (size_t)s * A.S.stride;
  const double acc = kfdb_wave_sum(A.qn, A.qval, A.S.ids + row, A.S.vals + row, A.S.len[s], lane);
  if (lane == 0) A.out[e] = -acc / 2.0;
}

extern "C" void psk_kfdb_put_launch(const KfdbAddArrays* A, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(kfdb_put, dim3(n), dim3(256), 0, st, *A);
}

// lds_words: the longest query of the call
extern "C" void psk_kfdb_query_launch(const KfdbQueryArrays* A, int lds_words, hipStream_t st) {
  const size_t lds = (size_t)(lds_words > 0 ? lds_words : 1) * 4;
  const int per = 4 * A->spw;
  hipLaunchKernelGGL(kfdb_count, dim3((A->S.high + per - 1) / per, A->nq), dim3(KFDB_T), lds, st, *A);
  hipLaunchKernelGGL(kfdb_score, dim3((A->S.high + 3) / 4, A->nq), dim3(KFDB_T), lds, st, *A);
  hipLaunchKernelGGL(kfdb_list, dim3(A->nq), dim3(KFDB_LIST_T), 0, st, *A);
  if (A->nloop < A->nq) hipLaunchKernelGGL(kfdb_commit, dim3((A->S.high + 255) / 256), dim3(256), 0, st, *A);
}

extern "C" void psk_kfdb_score_launch(const KfdbScoreArrays* A, hipStream_t st) {
  if (A->n > 0) hipLaunchKernelGGL(kfdb_score_slots, dim3((A->n + 3) / 4), dim3(KFDB_T), (size_t)(A->qn > 0 ? A->qn : 1) * 4, st, *A);
}
