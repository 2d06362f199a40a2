// CDNA4 kernels of the bag-of-words calls: TemplatedVocabulary::transform (/root/reference/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:
// 1133-1200, :1224-1265) for a batch of frames and ORBmatcher::SearchByBoW (/root/reference/src/ORBmatcher.cc:280-410, :646-781).
//   bow_walk   : a 16-lane row per feature, four features per wave.  Lane c of the row loads child c of the node the feature
//                stands on (32 bytes as two 16-byte loads; a sibling group is one contiguous run) and the row takes a DPP minimum
//                of distance << 20 | c - least distance, earliest child, which is what the strict `d < best_d` (:1250) leaves.
//                Nodes with more than 16 children take further passes over the row.  Beside the descriptor a lane loads the
//                16-byte slot of its child (id, children, word, weight); the winner's slot is passed round the row, so a level
//                is one round trip to memory.  Every level waits for the one above it, so the kernel lives on the number of rows
//                in flight, not on arithmetic: it keeps no LDS and few registers, and a workgroup is four independent waves.
//   bow_vector : one workgroup per frame.  Bitonic sort of the word ids in LDS, run heads by comparison with the left neighbour,
//                run lengths by binary search, value = count * weight (TF_IDF, TF: the weights are floats and the counts below
//                2^13, so the product equals the reference's repeated double addition exactly) or the weight (IDF, BINARY), the
//                L1 norm as a tree sum, the division.
//   bow_search : one wave per (problem, vocabulary node present on both sides).  The features of side a in the node are walked one
//                after the other - the skip rule makes that order part of the result - and the candidates of side b are spread
//                over the lanes in chunks of 64 (the first chunk stays in registers).  The taken bits of the node sit in LDS, one word per 32 candidates.  Two wave
//                minimums: the best as distance << 16 | position (first of least distance), then the least distance among the
//                others.
//   bow_commit : one workgroup per problem: rotation histogram, ComputeThreeMaxima, the matches outside the three bins removed,
//                the count.
// Everything is integer or evaluated as written (contraction off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bow_plan.h"
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int bow_hamming256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// unsigned minimum over the 16 lanes of a DPP row; every lane of the row receives it.  All lanes of the wave must be active.
__device__ __forceinline__ uint32_t bow_row_min_u32(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
  return v;
}
__device__ __forceinline__ uint32_t bow_wave_min_u32(uint32_t v) {
  v = bow_row_min_u32(v);
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  return min(min(a, b), min(c, d));
}

__global__ __launch_bounds__(256) void bow_walk(BowTransformArrays A) {
  const int c = threadIdx.x & 15;
  const int g = blockIdx.x * 16 + (threadIdx.x >> 4);   // the row's feature slot; the 16 slots of a workgroup belong to one frame
  const BowFrame F = A.frame[A.feat_frame[blockIdx.x]];
  const int i = g - F.f_off;
  bool live = i < F.n;
  uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
  if (live) {
    const uint4* q = reinterpret_cast<const uint4*>(A.desc + (size_t)g * 32);
    q0 = q[0]; q1 = q[1];
  }
  const int nid_level = A.tree.L - F.levelsup;
  int cur = 0, level = 0, nid = nid_level <= 0 ? 0 : -1;
  int off = 0, cnt = A.tree.root_cnt, word = -1;
  float weight = 0.f;
  const int4* slots = reinterpret_cast<const int4*>(A.tree.slot);
  while (__any(live)) {   // wave-uniform: the rows of a wave may stand at different depths, a finished row idles through the minimum
    uint32_t key = 0xFFFFFFFFu;
    int4 mine = make_int4(0, 0, 0, 0);                            // the slot of this lane's best child
    if (live) {
      for (int c0 = 0; c0 < cnt; c0 += 16) {
        if (c0 + c < cnt) {
          const uint4* d = reinterpret_cast<const uint4*>(A.tree.child_desc + (size_t)(off + c0 + c) * 32);
          const int4 s = slots[off + c0 + c];
          const uint32_t kk = ((uint32_t)bow_hamming256(q0, q1, d[0], d[1]) << 20) | (uint32_t)(c0 + c);
          if (kk < key) { key = kk; mine = s; }
        }
      }
    }
    const uint32_t win = bow_row_min_u32(key);
    const int src = (int)(win & 15u);                             // the lane of the row that looked at the winner
    const int w_id = __shfl(mine.x, src, 16), w_off = __shfl(mine.y, src, 16), w_cnt = __shfl(mine.z, src, 16), w_wt = __shfl(mine.w, src, 16);
    if (live) {
      cur = w_id;
      level++;
      if (level == nid_level) nid = cur;
      if (w_cnt == 0) { word = w_off; weight = __int_as_float(w_wt); live = false; }
      else { off = w_off; cnt = w_cnt; }
    }
  }
  if (c == 0 && i < F.n) {
    const bool stopped = !(weight > 0.0f);                        // `if(w > 0)` (:1163, :1191)
    A.word[g] = stopped ? -1 : word;
    A.node[g] = stopped ? -1 : (nid >= 0 ? nid : cur);            // a leaf above the asked level: the leaf itself (modelling choice)
  }
}

#define BOW_VEC_T 256
__global__ __launch_bounds__(BOW_VEC_T) void bow_vector(BowTransformArrays A) {
  __shared__ uint32_t key[PS_BOW_MAX_N + 1];
  __shared__ int s_cnt[BOW_VEC_T + 1];
  __shared__ double s_sum[BOW_VEC_T];
  const BowFrame F = A.frame[blockIdx.x];
  const int tid = threadIdx.x, n = F.n;
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += BOW_VEC_T) {
    const int w = i < n ? A.word[F.f_off + i] : -1;
    key[i] = w < 0 ? 0xFFFFFFFFu : (uint32_t)w;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += BOW_VEC_T) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint32_t a = key[lo], b = key[hi];
        const bool up = (lo & k) == 0;
        if ((a > b) == up) { key[lo] = b; key[hi] = a; }
      }
      __syncthreads();
    }
  }
  // every thread owns a contiguous chunk of the sorted keys; a run's head is the key that differs from its left neighbour
  const int ch = (P + BOW_VEC_T - 1) / BOW_VEC_T;
  const int b0 = tid * ch, b1 = min(b0 + ch, P);
  int heads = 0;
  for (int i = b0; i < b1; i++) heads += (key[i] != 0xFFFFFFFFu && (i == 0 || key[i] != key[i - 1])) ? 1 : 0;
  s_cnt[tid + 1] = heads;
  if (tid == 0) s_cnt[0] = 0;
  __syncthreads();
  if (tid == 0) for (int t = 0; t < BOW_VEC_T; t++) s_cnt[t + 1] += s_cnt[t];
  __syncthreads();
  int pos = s_cnt[tid];
  const int first = pos;
  double sum = 0.0;
  for (int i = b0; i < b1; i++) {
    const uint32_t kk = key[i];
    if (kk == 0xFFFFFFFFu || (i > 0 && kk == key[i - 1])) continue;
    int lo = i, hi = P;                                           // the first index behind the run
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (key[mid] == kk) lo = mid; else hi = mid; }
    const double w = (double)A.tree.word_weight[kk];
    const double v = A.tree.weighting <= 1 ? (double)(hi - i) * w : w;   // TF_IDF, TF: addWeight; IDF, BINARY: addIfNotExist
    A.bow_id[F.f_off + pos] = (int32_t)kk;
    A.bow_val[F.f_off + pos] = v;
    sum += fabs(v);
    pos++;
  }
  s_sum[tid] = sum;
  __syncthreads();
  for (int s = BOW_VEC_T >> 1; s > 0; s >>= 1) {
    if (tid < s) s_sum[tid] += s_sum[tid + s];
    __syncthreads();
  }
  const double norm = s_sum[0];
  if (norm > 0.0)
    for (int p = first; p < pos; p++) A.bow_val[F.f_off + p] = __ddiv_rn(A.bow_val[F.f_off + p], norm);
  if (tid == 0) A.bow_n[blockIdx.x] = s_cnt[BOW_VEC_T];
}

// A whole wave per (problem, node) item.  16-lane rows (four items per wave) were measured beside it: 0.196 against 0.244 ms for
// 512 problems of 2000 x 2000 features, but 0.080 against 0.049 ms for one problem - the tracking thread's call.
__global__ __launch_bounds__(256) void bow_search(BowSearchArrays A) {
  constexpr int W = 64, G = 256 / W;
  __shared__ uint32_t taken_s[G][(PS_BOW_MAX_N + 64) / 32];
  const int grp = threadIdx.x / W, lane = threadIdx.x % W;
  const int it = blockIdx.x * G + grp;
  if (it >= A.nitems) return;                                     // a whole wave or row; the kernel has no workgroup barrier
  const BowSItem I = A.item[it];
  const BowSProb P = A.prob[I.prob];
  volatile uint32_t* taken = taken_s[grp];
  const int nb = I.b1 - I.b0;
  // bit k: candidate k of the node is not admitted - taken by an earlier feature of a, or (mode 1) without a point
  for (int w = lane; w < (nb + 31) / 32; w += W) taken[w] = 0;
  __builtin_amdgcn_wave_barrier();
  if (P.mode == 1)
    for (int k = lane; k < nb; k += W)
      if (A.hasp[P.b_off + A.lst[I.b0 + k]] == 0) atomicOr(&taken_s[grp][k >> 5], 1u << (k & 31));
  // the first chunk's candidates stay in registers: most nodes hold fewer than that
  uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
  if (lane < nb) {
    const uint4* d = reinterpret_cast<const uint4*>(A.desc + (size_t)(P.b_off + A.lst[I.b0 + lane]) * 32);
    r0 = d[0]; r1 = d[1];
  }
  const uint32_t none = (256u << 16) | 0xFFFFu;
  for (int ia = I.a0; ia < I.a1; ia++) {
    const int fa = A.lst[ia];
    if (!A.hasp[P.a_off + fa]) continue;                          // !pMP || pMP->isBad(): uniform over the item's lanes
    const uint4* q = reinterpret_cast<const uint4*>(A.desc + (size_t)(P.a_off + fa) * 32);
    const uint4 q0 = q[0], q1 = q[1];
    __builtin_amdgcn_wave_barrier();
    uint32_t best = none, second = 256;                           // of this lane's candidates, in ascending position
    for (int k0 = 0; k0 < nb; k0 += W) {
      const int k = k0 + lane;
      if (k < nb && !((taken[k >> 5] >> (k & 31)) & 1u)) {
        uint32_t dist;
        if (k0 == 0) dist = (uint32_t)bow_hamming256(q0, q1, r0, r1);
        else {
          const uint4* d = reinterpret_cast<const uint4*>(A.desc + (size_t)(P.b_off + A.lst[I.b0 + k]) * 32);
          dist = (uint32_t)bow_hamming256(q0, q1, d[0], d[1]);
        }
        const uint32_t kk = (dist << 16) | (uint32_t)k;
        if (kk < best) { second = min(second, best >> 16); best = kk; }
        else if (dist < second) second = dist;
      }
    }
    const uint32_t gbest = bow_wave_min_u32(best);                // least distance, first position
    const uint32_t gsecond = bow_wave_min_u32(best == gbest ? second : (best >> 16));
    const uint32_t d1 = gbest >> 16;
    const bool near = P.mode == 0 ? d1 <= 50u : d1 < 50u;         // TH_LOW: `<=` at :350, `<` at :724
    if (near && (float)d1 < P.nn_ratio * (float)gsecond) {
      const int pos = (int)(gbest & 0xFFFFu);
      if (lane == 0) {
        const int fb = A.lst[I.b0 + pos];
        taken[pos >> 5] = taken[pos >> 5] | (1u << (pos & 31));
        if (P.mode == 0) A.match[(size_t)P.out_off + fb] = fa; else A.match[(size_t)P.out_off + fa] = fb;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

#define BOW_COMMIT_T 256
__device__ __forceinline__ int bow_rot_bin(float a1, float a2) {
  float rot = a1 - a2;
  if (rot < 0.0f) rot += 360.0f;
  int bin = (int)roundf(rot * (30.0f / 360.0f));
  if (bin == 30) bin = 0;
  return bin < 0 ? 0 : (bin > 29 ? 29 : bin);   // (angles outside [0, 360) would trip the reference's assert)
}

__global__ __launch_bounds__(BOW_COMMIT_T) void bow_commit(BowSearchArrays A) {
  __shared__ int hist[30];
  __shared__ int s_nm;
  const BowSProb P = A.prob[blockIdx.x];
  const int tid = threadIdx.x;
  if (tid < 30) hist[tid] = 0;
  if (tid == 0) s_nm = 0;
  __syncthreads();
  int nm = 0;
  for (int e = tid; e < P.out_n; e += BOW_COMMIT_T) {
    const int m = A.match[(size_t)P.out_off + e];
    if (m < 0) continue;
    nm++;
    if (P.check_ori) {
      const int ia = P.mode == 0 ? m : e, ib = P.mode == 0 ? e : m;
      atomicAdd(&hist[bow_rot_bin(A.ang[P.a_off + ia], A.ang[P.b_off + ib])], 1);
    }
  }
  __syncthreads();
  if (P.check_ori) {   // ComputeThreeMaxima (ORBmatcher.cc:2658-2699)
    int i1 = -1, i2 = -1, i3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < 30; i++) {
      const int s = hist[i];
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
      else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { i3 = -1; }
    for (int e = tid; e < P.out_n; e += BOW_COMMIT_T) {
      const int m = A.match[(size_t)P.out_off + e];
      if (m < 0) continue;
      const int ia = P.mode == 0 ? m : e, ib = P.mode == 0 ? e : m;
      const int b = bow_rot_bin(A.ang[P.a_off + ia], A.ang[P.b_off + ib]);
      if (b != i1 && b != i2 && b != i3) { A.match[(size_t)P.out_off + e] = -1; nm--; }
    }
  }
  if (nm) atomicAdd(&s_nm, nm);
  __syncthreads();
  if (tid == 0) A.nmatch[blockIdx.x] = s_nm;
}

}  // namespace

extern "C" void psk_bow_transform_launch(const BowTransformArrays* A, int nframes, hipStream_t st) {
  if (A->nblocks16 > 0) hipLaunchKernelGGL(bow_walk, dim3(A->nblocks16), dim3(256), 0, st, *A);
  if (nframes > 0) hipLaunchKernelGGL(bow_vector, dim3(nframes), dim3(BOW_VEC_T), 0, st, *A);
}

extern "C" void psk_bow_search_launch(const BowSearchArrays* A, hipStream_t st) {
  if (A->nitems > 0) hipLaunchKernelGGL(bow_search, dim3((A->nitems + 3) / 4), dim3(256), 0, st, *A);
  if (A->nprob > 0) hipLaunchKernelGGL(bow_commit, dim3(A->nprob), dim3(BOW_COMMIT_T), 0, st, *A);
}
