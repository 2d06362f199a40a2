// CDNA4 kernels for the loop-closure and relocalisation projection matchers (ps_kf_search, ps_search_by_sim3):
//   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)              /root/reference/src/ORBmatcher.cc:413-526   kind 0
//   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)                       :1262-1385                                  kind 1
//   ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)  :2529-2656                                  kind 2
//   ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)           :1387-1611                                  kind 3, twice
// with KeyFrame::GetFeaturesInArea (/root/reference/src/KeyFrame.cc:665-704) / Frame::GetFeaturesInArea (Frame.cc:1808-1861) as the
// candidate generator.  Every search of a batch is one KsJob (kfsearch_plan.h).
//   ks_search  : one wave per point, as fuse_search - the float projection and the gates are wave-uniform, the lanes walk the grid
//                window in the reference's order (ix, then iy, then cell order).  Independent kinds (1, 3): "first strict minimum" =
//                wave minimum of (distance, traversal position).  Order-dependent kinds (0, 2): the candidates that can ever be
//                taken - free at entry, distance <= th_dist - are stored in traversal order as keys
//                dist << 23 | position << 13 | train index, with their number and the smallest key.
//   ks_resolve : one wave per order-dependent job - the points in order over an LDS bitmap of the slots given away by this call;
//                a point whose smallest key is still free takes it without touching memory, otherwise its list is rescanned.
//                Kind 2: rotation histogram with the overload's own factor 1.0f / HISTO_LENGTH, ComputeThreeMaxima, reset (-2).
//   ks_agree   : the agreement pass of SearchBySim3 (:1595-1608) on the two directions' results, which never leave the device.
// Float expressions are evaluated as written (-ffp-contract=off); cv::Mat products, Mat::dot and cv::norm accumulate in double.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kfsearch_plan.h"
#include "match_device.h"

namespace {

constexpr uint32_t KS_IDXM = (1u << PS_KS_IDXB) - 1u;
constexpr uint32_t KS_NONE = 0xFFFFFFFFu;

// No LDS, 42 VGPRs, no scratch (two descriptors, the window bounds, the projection): eight waves per SIMD fit; the kernel is latency
// bound (three dependent loads per 64 candidates) and lives on that occupancy.
__global__ __launch_bounds__(256) void ks_search(KsArrays A) {
  const KsJob& J = A.job[blockIdx.y];     // by reference: a private copy indexed by the level (J.scale[lvl]) would live in scratch memory
  const int qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (qi >= J.nq) return;
  const int q = J.q_off + qi;
  const int kind = J.kind;
  const bool ordered = kind == 0 || kind == 2;
  bool ok = A.qvalid[q] != 0;
  const float X = A.qpos[3 * q], Y = A.qpos[3 * q + 1], Z = A.qpos[3 * q + 2];
  float xc = __fadd_rn(dot3_f(&J.R[0], X, Y, Z), J.t[0]);
  float yc = __fadd_rn(dot3_f(&J.R[3], X, Y, Z), J.t[1]);
  float zc = __fadd_rn(dot3_f(&J.R[6], X, Y, Z), J.t[2]);
  float dist3D;
  if (kind == 3) {
    // p3Dc2 = sR21 * p3Dc1 + t21: a second rounded step, and the distance is that of the camera-frame point (:1445, :1464)
    const float x2 = __fadd_rn(dot3_f(&J.R2[0], xc, yc, zc), J.t2[0]);
    const float y2 = __fadd_rn(dot3_f(&J.R2[3], xc, yc, zc), J.t2[1]);
    const float z2 = __fadd_rn(dot3_f(&J.R2[6], xc, yc, zc), J.t2[2]);
    xc = x2; yc = y2; zc = z2;
    dist3D = (float)sqrt(__dadd_rn(__dadd_rn(__dmul_rn((double)xc, (double)xc), __dmul_rn((double)yc, (double)yc)), __dmul_rn((double)zc, (double)zc)));
  } else {
    const float p0 = __fsub_rn(X, J.ow[0]), p1 = __fsub_rn(Y, J.ow[1]), p2 = __fsub_rn(Z, J.ow[2]);
    dist3D = (float)sqrt(__dadd_rn(__dadd_rn(__dmul_rn((double)p0, (double)p0), __dmul_rn((double)p1, (double)p1)), __dmul_rn((double)p2, (double)p2)));
    if (kind != 2) {   // viewing angle (:477, :1327); the relocalisation overload has no such gate
      const double dotn = __dadd_rn(__dadd_rn(__dmul_rn((double)p0, (double)A.qnormal[3 * q]), __dmul_rn((double)p1, (double)A.qnormal[3 * q + 1])),
                                    __dmul_rn((double)p2, (double)A.qnormal[3 * q + 2]));
      if (dotn < __dmul_rn(0.5, (double)dist3D)) ok = false;
    }
  }
  const float invz = __fdiv_rn(1.0f, zc);   // 1/z, 1.0/z and 1.0f/z are the same float
  float u, v;
  if (kind == 2) {
    // no depth-sign gate; fx*xc*invzc+cx associates as ((fx*xc)*invzc)+cx; inclusive bounds (:2561-2567).  A non-finite u or v
    // (z == 0) counts as outside the image.
    u = __fadd_rn(__fmul_rn(__fmul_rn(J.fx, xc), invz), J.cx);
    v = __fadd_rn(__fmul_rn(__fmul_rn(J.fy, yc), invz), J.cy);
    if (!(u >= J.bounds[0] && u <= J.bounds[1] && v >= J.bounds[2] && v <= J.bounds[3])) ok = false;
  } else {
    if (zc < 0.0f) ok = false;
    u = __fadd_rn(__fmul_rn(J.fx, __fmul_rn(xc, invz)), J.cx);
    v = __fadd_rn(__fmul_rn(J.fy, __fmul_rn(yc, invz)), J.cy);
    if (!(u >= J.bounds[0] && u < J.bounds[1] && v >= J.bounds[2] && v < J.bounds[3])) ok = false;   // KeyFrame::IsInImage
  }
  const float maxd = A.qmax[q], mind = A.qmin[q];
  if (dist3D < __fmul_rn(0.8f, mind) || dist3D > __fmul_rn(1.2f, maxd)) ok = false;
  uint32_t best = KS_NONE;       // independent: distance << 20 | traversal position; ordered: the candidate key
  int bestj = -1;
  int count = 0;                 // ordered: candidates kept so far
  if (ok && J.nt > 0) {
    const float ratio = __fdiv_rn(maxd, dist3D);
    int lvl = (int)ceil(__ddiv_rn(log((double)ratio), (double)J.log_scale));
    lvl = lvl < 0 ? 0 : (lvl >= J.n_levels ? J.n_levels - 1 : lvl);
    const int lo = lvl - 1, hi = kind == 2 ? lvl + 1 : lvl;
    const float r = __fmul_rn(J.th, J.scale[lvl]);
    const int nMinCellX = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(u, J.min_x), r), J.gw_inv)));
    const int nMaxCellX = min(PS_GRID_COLS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(u, J.min_x), r), J.gw_inv)));
    const int nMinCellY = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(v, J.min_y), r), J.gh_inv)));
    const int nMaxCellY = min(PS_GRID_ROWS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(v, J.min_y), r), J.gh_inv)));
    if (nMinCellX < PS_GRID_COLS && nMaxCellX >= 0 && nMinCellY < PS_GRID_ROWS && nMaxCellY >= 0) {
      const uint4* qd = reinterpret_cast<const uint4*>(A.qdesc + (size_t)q * 32);
      const uint4 a0 = qd[0], a1 = qd[1];
      const int32_t* coff = A.cell_off + J.grid_off;
      const int cap = J.cap;
      uint32_t* row = ordered ? A.cand + ((size_t)J.c_off + qi) * cap : nullptr;
      int scanned = 0;
      for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
        const int b = coff[ix * PS_GRID_ROWS + nMinCellY], e = coff[ix * PS_GRID_ROWS + nMaxCellY + 1];
        for (int k0 = b; k0 < e; k0 += 64) {
          const int k = k0 + lane;
          bool pass = false;
          int j = 0;
          uint32_t dist = 0;
          if (k < e) {
            j = A.cell_idx[J.t_off + k];
            const int t = J.t_off + j;
            const float ex = __fsub_rn(A.tx[t], u), ey = __fsub_rn(A.ty[t], v);
            const int oc = A.toct[t];
            pass = fabsf(ex) < r && fabsf(ey) < r && oc >= lo && oc <= hi;
            if (pass && ordered && A.tocc[t]) pass = false;          // vpMatched[idx] / mvpMapPoints[i2] at entry
            if (pass) {
              const uint4* td = reinterpret_cast<const uint4*>(A.tdesc + (size_t)t * 32);
              dist = (uint32_t)hamming256(a0, a1, td[0], td[1]);
              if (ordered && (int)dist > J.th_dist) pass = false;    // can never be taken
            }
          }
          if (ordered) {
            const unsigned long long pm = __builtin_amdgcn_ballot_w64(pass);
            const int pos = count + __popcll(pm & ((1ull << lane) - 1ull));
            if (pass) {
              const uint32_t key = (dist << 23) | ((uint32_t)min(pos, PS_KS_CAP_WIDE - 1) << PS_KS_IDXB) | (uint32_t)j;
              if (pos < cap) row[pos] = key;
              if (key < best) best = key;
            }
            count += __popcll(pm);
          } else if (pass) {
            const uint32_t key = (dist << 20) | (uint32_t)min(scanned + (k - k0), 0xFFFFF);
            if (key < best) { best = key; bestj = j; }
          }
          scanned += 64;
        }
      }
    }
  }
  const uint32_t bk = wave_min_u32(best);
  if (ordered) {
    if (lane == 0) {
      if (count > J.cap) { atomicAdd(&A.overflow[blockIdx.y], 1); count = J.cap; }
      A.ncand[q] = count;
      A.qtop[q] = bk;
    }
  } else {
    int out_idx = -1, out_dist = 256;
    if (bk != KS_NONE) {
      out_dist = (int)(bk >> 20);
      const unsigned long long holder = __builtin_amdgcn_ballot_w64(best == bk);
      const int bj = __builtin_amdgcn_readlane(bestj, __ffsll((long long)holder) - 1);
      if (out_dist <= J.th_dist) out_idx = bj;
    }
    if (lane == 0) { A.best_idx[q] = out_idx; A.best_dist[q] = out_dist; }
  }
}

// LDS: 1 KB bitmap (8192 slots) + 8 KB bins + the histogram = 9.1 KB per workgroup of one wave (of the CU's 160 KB); 14 VGPRs.
__global__ __launch_bounds__(64) void ks_resolve(KsArrays A) {
  __shared__ uint32_t taken[(PS_KS_MAX_N + 32) / 32];   // slots given away by this call (those occupied at entry never reach the lists)
  __shared__ uint8_t bin_of[PS_KS_MAX_N + 1];
  __shared__ int hist[32];
  __shared__ int s_removed;
  const KsJob J = A.job[blockIdx.x];
  if (!(J.kind == 0 || J.kind == 2)) return;
  const int lane = threadIdx.x;
  int32_t* match = A.match + J.t_off;
  for (int w = lane; w < (PS_KS_MAX_N + 32) / 32; w += 64) taken[w] = 0;
  if (lane < 32) hist[lane] = 0;
  if (lane == 0) s_removed = 0;
  for (int j = lane; j < J.nt; j += 64) match[j] = -1;
  __syncthreads();
  int nm = 0;
  for (int q0 = 0; q0 < J.nq; q0 += 64) {
    const bool qin = q0 + lane < J.nq;
    const int nc = qin ? A.ncand[J.q_off + q0 + lane] : 0;
    const uint32_t top = qin ? A.qtop[J.q_off + q0 + lane] : KS_NONE;
    unsigned long long pend = __builtin_amdgcn_ballot_w64(nc > 0);
    while (pend) {                                   // the points that have a candidate at all, in order
      const int i = __ffsll((long long)pend) - 1;
      pend &= pend - 1;
      uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)top, i);
      const uint32_t j0 = key & KS_IDXM;
      if ((taken[j0 >> 5] >> (j0 & 31)) & 1u) {
        // its best candidate went to an earlier point: the smallest key of its list that is still free
        const int nci = __builtin_amdgcn_readlane(nc, i);
        const uint32_t* row = A.cand + ((size_t)J.c_off + q0 + i) * J.cap;
        uint32_t m = KS_NONE;
        for (int c = lane; c < nci; c += 64) {
          const uint32_t k = row[c];
          const uint32_t jj = k & KS_IDXM;
          if (!((taken[jj >> 5] >> (jj & 31)) & 1u) && k < m) m = k;
        }
        key = wave_min_u32(m);
      }
      if (key == KS_NONE) continue;
      if (lane == 0) {
        const uint32_t j = key & KS_IDXM;
        taken[j >> 5] |= 1u << (j & 31);
        match[j] = q0 + i;
      }
      nm++;
      __syncthreads();
    }
  }
  __syncthreads();
  if (J.kind == 2 && J.check_ori) {
    const float factor = 1.0f / 30;                  // 1.0f / HISTO_LENGTH, as this overload writes it (:2541): bins 0 .. 12
    for (int j = lane; j < J.nt; j += 64) {
      const int qi = match[j];
      if (qi >= 0) {
        float rot = __fsub_rn(A.qang[J.q_off + qi], A.tang[J.t_off + j]);
        if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
        int bin = (int)roundf(__fmul_rn(rot, factor));
        if (bin == 30) bin = 0;
        if (!(bin >= 0 && bin < 30)) bin = 0;        // angles outside [0, 360): the reference's assert; here the bin stays inside the table
        atomicAdd(&hist[bin], 1);
        bin_of[j] = (uint8_t)bin;
      }
    }
    __syncthreads();
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < 30; i++) {
      const int s = hist[i];
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
      else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { i2 = -1; i3 = -1; }
    else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) { i3 = -1; }
    int removed = 0;
    for (int j = lane; j < J.nt; j += 64) {
      if (match[j] >= 0) {
        const int b = bin_of[j];
        if (b != i1 && b != i2 && b != i3) { match[j] = -2; removed++; }
      }
    }
    if (removed) atomicAdd(&s_removed, removed);
    __syncthreads();
    nm -= s_removed;
  }
  if (lane == 0) A.nmatch[blockIdx.x] = nm;
}

// 4 bytes of LDS, 10 VGPRs.
__global__ __launch_bounds__(256) void ks_agree(KsArrays A) {
  __shared__ int s_n;
  const KsPair P = A.pair[blockIdx.x];
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int n = 0;
  for (int i1 = threadIdx.x; i1 < P.n1; i1 += 256) {
    const int idx2 = A.best_idx[P.q1_off + i1];
    int r = -1;
    if (idx2 >= 0 && idx2 < P.n2 && A.best_idx[P.q2_off + idx2] == i1) { r = idx2; n++; }
    A.match12[P.q1_off + i1] = r;
  }
  if (n) atomicAdd(&s_n, n);
  __syncthreads();
  if (threadIdx.x == 0) A.nfound[blockIdx.x] = s_n;
}

}  // namespace

// max_nq >= 1.  npair > 0: the jobs are the two directions of npair Sim3 problems, and the agreement pass follows.
extern "C" void psk_ks_launch(const KsArrays* arrays, int njobs, int max_nq, int any_ordered, int npair, hipStream_t st) {
  const KsArrays A = *arrays;
  hipLaunchKernelGGL(ks_search, dim3((max_nq + 3) / 4, njobs), dim3(256), 0, st, A);
  if (any_ordered) hipLaunchKernelGGL(ks_resolve, dim3(njobs), dim3(64), 0, st, A);
  if (npair > 0) hipLaunchKernelGGL(ks_agree, dim3(npair), dim3(256), 0, st, A);
}
