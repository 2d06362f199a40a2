// CDNA4 kernels of ps_create_new_map_points: LocalMapping::CreateNewMapPoints (/root/reference/src/LocalMapping.cc:414-707) for
// a batch of keyframes - ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:783-979) against every neighbour and the
// per-match triangulation with its gates (LocalMapping.cc:519-684).
//   tri_match  : a wave takes 64 consecutive features of keyframe 1 against one neighbour.  The search is one wave per feature,
//                one feature after the other: the lanes stride over the neighbour's features of the same vocabulary node; the
//                winner is a wave-min of distance << 20 | ~index (least distance, then the HIGHEST index: the reference's
//                `dist > bestDist` lets a later equal distance replace the earlier one, ORBmatcher.cc:865) and goes to the lane
//                of that feature.  The triangulation is then one lane per feature, the wave's 64 winners at once (a few
//                hundred FP64 operations each; done wave-uniformly per feature it was more than half of the kernel's time).
//   tri_commit : one workgroup per keyframe 1, k barrier-separated rounds.  vbMatched2 (ORBmatcher.cc:803) is read at :852 and
//                never written, so a feature's partner does not depend on the other features; the only state that travels
//                from one neighbour to the next is the slot of keyframe 1 that a created point fills (LocalMapping.cc:693,
//                read at ORBmatcher.cc:826-830).  The round drops the matches of filled slots, applies the rotation histogram
//                to what is left, turns "would create" into "created" and sets the slot's bit in LDS.
// Float expressions are evaluated as written (contraction off); cv::Mat products, Mat::dot and cv::norm accumulate in double.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tri_plan.h"
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int tri_hamming256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// wave-wide unsigned minimum on DPP lanes, as in match_kernels.hip.  All 64 lanes must be active.
__device__ __forceinline__ uint32_t tri_wave_min_u32(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  return min(min(a, b), min(c, d));
}

// a . b of float vectors the way Mat::dot / cv::gemm / cv::norm form it: products and sum in double
__device__ __forceinline__ double tri_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return (double)a0 * (double)b0 + (double)a1 * (double)b1 + (double)a2 * (double)b2;
}

// the baseline gate of a stereo / RGB-D system (LocalMapping.cc:463-475): the neighbour is skipped as a whole
__device__ __forceinline__ bool tri_neighbour_skipped(const TriProb& P, const TriKf& K1, const TriKf& K2) {
  if (!P.triangulate) return false;
  const float b0 = K2.ow[0] - K1.ow[0], b1 = K2.ow[1] - K1.ow[1], b2 = K2.ow[2] - K1.ow[2];
  const float baseline = (float)sqrt(tri_dot3(b0, b1, b2, b0, b1, b2));
  return baseline < K2.mb;
}

// Right singular vector of the least singular value of the 4 x 4 float matrix A, in FP64: one-sided Jacobi on the four columns
// (the rotations that make the columns orthogonal, accumulated in V; the shortest column's V column is the answer).  The loops
// are unrolled so that both matrices stay in registers.
__device__ __forceinline__ void tri_null_vector(const float (&Af)[4][4], double (&out)[4]) {
  double a[4][4], v[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) { a[r][c] = (double)Af[r][c]; v[r][c] = r == c ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; p++) {
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) { alpha += a[r][p] * a[r][p]; beta += a[r][q] * a[r][q]; gamma += a[r][p] * a[r][q]; }
        if (gamma != 0.0 && fabs(gamma) > 1e-15 * sqrt(alpha * beta)) {
          rotated = true;
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const double ap = a[r][p], aq = a[r][q];
            a[r][p] = c * ap - s * aq; a[r][q] = s * ap + c * aq;
            const double vp = v[r][p], vq = v[r][q];
            v[r][p] = c * vp - s * vq; v[r][q] = s * vp + c * vq;
          }
        }
      }
    }
    if (!rotated) break;
  }
  double least = 0.0;
  out[0] = v[0][0]; out[1] = v[1][0]; out[2] = v[2][0]; out[3] = v[3][0];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const double n2 = a[0][c] * a[0][c] + a[1][c] * a[1][c] + a[2][c] * a[2][c] + a[3][c] * a[3][c];
    if (c == 0 || n2 < least) { least = n2; out[0] = v[0][c]; out[1] = v[1][c]; out[2] = v[2][c]; out[3] = v[3][c]; }
  }
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:711-727): mvKeys, not mvKeysUn
__device__ __forceinline__ void tri_unproject_stereo(const TriArrays& A, const TriKf& K, int i, float (&X)[3]) {
  const float z = A.depth[K.f_off + i];
  const float u = K.raw_off >= 0 ? A.xraw[K.raw_off + i] : A.x[K.f_off + i];
  const float v = K.raw_off >= 0 ? A.yraw[K.raw_off + i] : A.y[K.f_off + i];
  const float x = (u - K.cx) * z * K.invfx;
  const float y = (v - K.cy) * z * K.invfy;
  // Twc.rowRange(0,3).colRange(0,3) * x3Dc + Twc.rowRange(0,3).col(3): Rwc = Rcw^T, the last column is the camera centre
  X[0] = (float)tri_dot3(K.rcw[0], K.rcw[3], K.rcw[6], x, y, z) + K.ow[0];
  X[1] = (float)tri_dot3(K.rcw[1], K.rcw[4], K.rcw[7], x, y, z) + K.ow[1];
  X[2] = (float)tri_dot3(K.rcw[2], K.rcw[5], K.rcw[8], x, y, z) + K.ow[2];
}

// the reprojection gate of one keyframe (LocalMapping.cc:611-666); mbf is mpCurrentKeyFrame's for both keyframes, as written there
__device__ __forceinline__ bool tri_reprojection_fails(const TriKf& K, const float (&X)[3], float z, float kx, float ky, float kur, int oct, float mbf) {
  const float sigma2 = K.sigma2[oct & 7];
  const float x = (float)(tri_dot3(K.rcw[0], K.rcw[1], K.rcw[2], X[0], X[1], X[2]) + (double)K.tcw[0]);
  const float y = (float)(tri_dot3(K.rcw[3], K.rcw[4], K.rcw[5], X[0], X[1], X[2]) + (double)K.tcw[1]);
  const float invz = (float)__ddiv_rn(1.0, (double)z);
  const float u = K.fx * x * invz + K.cx;
  const float v = K.fy * y * invz + K.cy;
  const float ex = u - kx, ey = v - ky;
  if (!(kur >= 0)) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
  const float u_r = u - mbf * invz;
  const float er = u_r - kur;
  return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// LocalMapping.cc:519-684 for the pair (i1, i2): the status (see ps_tri_problem) and, where a point was formed, the point
__device__ int tri_point(const TriArrays& A, const TriProb& P, const TriKf& K1, const TriKf& K2, int i1, int i2, float (&X)[3]) {
  const int t1 = K1.f_off + i1, t2 = K2.f_off + i2;
  const float kx1 = A.x[t1], ky1 = A.y[t1], kur1 = A.ur[t1], kx2 = A.x[t2], ky2 = A.y[t2], kur2 = A.ur[t2];
  const int oct1 = A.oct[t1], oct2 = A.oct[t2];
  const bool st1 = kur1 >= 0, st2 = kur2 >= 0;
  const float xn1x = (kx1 - K1.cx) * K1.invfx, xn1y = (ky1 - K1.cy) * K1.invfy;
  const float xn2x = (kx2 - K2.cx) * K2.invfx, xn2y = (ky2 - K2.cy) * K2.invfy;
  float r1[3], r2[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {   // ray = Rwc * xn
    r1[c] = (float)tri_dot3(K1.rcw[c], K1.rcw[3 + c], K1.rcw[6 + c], xn1x, xn1y, 1.0f);
    r2[c] = (float)tri_dot3(K2.rcw[c], K2.rcw[3 + c], K2.rcw[6 + c], xn2x, xn2y, 1.0f);
  }
  const float cosRays = (float)__ddiv_rn(tri_dot3(r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]),
                                         sqrt(tri_dot3(r1[0], r1[1], r1[2], r1[0], r1[1], r1[2])) * sqrt(tri_dot3(r2[0], r2[1], r2[2], r2[0], r2[1], r2[2])));
  float cosStereo = cosRays + 1.0f;
  float cosStereo1 = cosStereo, cosStereo2 = cosStereo;
  // modelling choice: the cosine of the stereo parallax in FP64, rounded once
  if (st1) cosStereo1 = (float)cos(2.0 * atan2((double)__fdiv_rn(K1.mb, 2.0f), (double)A.depth[t1]));
  else if (st2) cosStereo2 = (float)cos(2.0 * atan2((double)__fdiv_rn(K2.mb, 2.0f), (double)A.depth[t2]));
  cosStereo = cosStereo2 < cosStereo1 ? cosStereo2 : cosStereo1;

  X[0] = X[1] = X[2] = 0.f;
  if (cosRays < cosStereo && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
    float M[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const float a0 = c < 3 ? K1.rcw[c] : K1.tcw[0], a1 = c < 3 ? K1.rcw[3 + c] : K1.tcw[1], a2 = c < 3 ? K1.rcw[6 + c] : K1.tcw[2];
      const float b0 = c < 3 ? K2.rcw[c] : K2.tcw[0], b1 = c < 3 ? K2.rcw[3 + c] : K2.tcw[1], b2 = c < 3 ? K2.rcw[6 + c] : K2.tcw[2];
      M[0][c] = xn1x * a2 - a0; M[1][c] = xn1y * a2 - a1;
      M[2][c] = xn2x * b2 - b0; M[3][c] = xn2y * b2 - b1;
    }
    // modelling choice: the null vector in FP64 on the float entries of A, the division in FP64, one rounding per coordinate
    double nv[4];
    tri_null_vector(M, nv);
    if ((float)nv[3] == 0.f) return 4;
    X[0] = (float)__ddiv_rn(nv[0], nv[3]); X[1] = (float)__ddiv_rn(nv[1], nv[3]); X[2] = (float)__ddiv_rn(nv[2], nv[3]);
  } else if (st1 && cosStereo1 < cosStereo2) {
    tri_unproject_stereo(A, K1, i1, X);
  } else if (st2 && cosStereo2 < cosStereo1) {
    tri_unproject_stereo(A, K2, i2, X);
  } else {
    return 3;
  }
  const float z1 = (float)(tri_dot3(K1.rcw[6], K1.rcw[7], K1.rcw[8], X[0], X[1], X[2]) + (double)K1.tcw[2]);
  if (z1 <= 0) return 5;
  const float z2 = (float)(tri_dot3(K2.rcw[6], K2.rcw[7], K2.rcw[8], X[0], X[1], X[2]) + (double)K2.tcw[2]);
  if (z2 <= 0) return 6;
  if (tri_reprojection_fails(K1, X, z1, kx1, ky1, kur1, oct1, K1.mbf)) return 7;
  if (tri_reprojection_fails(K2, X, z2, kx2, ky2, kur2, oct2, K1.mbf)) return 8;
  const float n10 = X[0] - K1.ow[0], n11 = X[1] - K1.ow[1], n12 = X[2] - K1.ow[2];
  const float n20 = X[0] - K2.ow[0], n21 = X[1] - K2.ow[1], n22 = X[2] - K2.ow[2];
  const float dist1 = (float)sqrt(tri_dot3(n10, n11, n12, n10, n11, n12));
  const float dist2 = (float)sqrt(tri_dot3(n20, n21, n22, n20, n21, n22));
  if (dist1 == 0 || dist2 == 0) return 9;
  const float ratioDist = __fdiv_rn(dist2, dist1);
  const float ratioOctave = __fdiv_rn(K1.scale[oct1 & 7], K2.scale[oct2 & 7]);
  if (ratioDist * P.ratio_factor < ratioOctave || ratioDist > ratioOctave * P.ratio_factor) return 10;
  return 0;
}

__global__ __launch_bounds__(256) void tri_match(TriArrays A) {
  const TriPair& R = A.pair[blockIdx.x];
  const TriProb& P = A.prob[R.prob];
  const int lane = threadIdx.x & 63;
  const int base = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 64;   // the wave's 64 consecutive features of keyframe 1
  if (base >= P.n1) return;
  const TriKf& K1 = A.kf[P.kf1];
  const TriKf& K2 = A.kf[R.kf2];
  const int mine = base + lane;                                  // the feature this lane triangulates and stores
  const size_t o = (size_t)R.out_off + mine;
  if (tri_neighbour_skipped(P, K1, K2)) {
    if (mine < P.n1) { A.match[o] = -1; A.status[o] = 11; A.x3d[3 * o] = 0.f; A.x3d[3 * o + 1] = 0.f; A.x3d[3 * o + 2] = 0.f; }
    return;
  }
  // the epipole in the neighbour's image (ORBmatcher.cc:789-796)
  const float c2x = (float)tri_dot3(K2.rcw[0], K2.rcw[1], K2.rcw[2], K1.ow[0], K1.ow[1], K1.ow[2]) + K2.tcw[0];
  const float c2y = (float)tri_dot3(K2.rcw[3], K2.rcw[4], K2.rcw[5], K1.ow[0], K1.ow[1], K1.ow[2]) + K2.tcw[1];
  const float c2z = (float)tri_dot3(K2.rcw[6], K2.rcw[7], K2.rcw[8], K1.ow[0], K1.ow[1], K1.ow[2]) + K2.tcw[2];
  const float invz = __fdiv_rn(1.0f, c2z);
  const float ex = K2.fx * c2x * invz + K2.cx;
  const float ey = K2.fy * c2y * invz + K2.cy;
  const float* F = R.f12;
  int my_best = -1, my_status = 1;
  const int count = P.n1 - base < 64 ? P.n1 - base : 64;
  for (int q = 0; q < count; q++) {   // ---- the search: the whole wave on one feature of keyframe 1 at a time (wave-uniform) ----
    const int t1 = K1.f_off + base + q;
    const float kx1 = A.x[t1], ky1 = A.y[t1];
    const bool st1 = A.ur[t1] >= 0;
    const int node = A.aux[t1];
    int status = 1, best2 = -1;
    if (A.occ[t1]) status = 2;
    else if (node >= 0 && !(P.only_stereo && !st1)) {
      // the epipolar line of kp1 in the neighbour's image (CheckDistEpipolarLine, :261-278)
      const float la = kx1 * F[0] + ky1 * F[3] + F[6];
      const float lb = kx1 * F[1] + ky1 * F[4] + F[7];
      const float lc = kx1 * F[2] + ky1 * F[5] + F[8];
      const float den = la * la + lb * lb;
      const uint4* qd = reinterpret_cast<const uint4*>(A.desc + (size_t)t1 * 32);
      const uint4 a0 = qd[0], a1 = qd[1];
      const int b = A.node_off[R.node_off + node], e = A.node_off[R.node_off + node + 1];
      uint32_t best = 0xFFFFFFFFu;   // distance << 20 | (0xFFFFF - index): the minimum is the least distance at the highest index
      for (int k0 = b; k0 < e; k0 += 64) {
        const int k = k0 + lane;
        if (k < e) {
          const int j = A.aux[K2.f_off + k];
          const int t2 = K2.f_off + j;
          const bool st2 = A.ur[t2] >= 0;
          bool pass = A.occ[t2] == 0 && !(P.only_stereo && !st2);
          uint32_t dist = 256;
          if (pass) {
            const uint4* td = reinterpret_cast<const uint4*>(A.desc + (size_t)t2 * 32);
            dist = (uint32_t)tri_hamming256(a0, a1, td[0], td[1]);
            pass = dist <= 50;                                   // TH_LOW
          }
          if (pass) {
            const float kx2 = A.x[t2], ky2 = A.y[t2];
            const int oct2 = A.oct[t2] & 7;
            if (!st1 && !st2) {
              const float dx = ex - kx2, dy = ey - ky2;
              if (dx * dx + dy * dy < 100.0f * K2.scale[oct2]) pass = false;
            }
            const float num = la * kx2 + lb * ky2 + lc;
            if (den == 0) pass = false;
            else if (!((double)__fdiv_rn(num * num, den) < 3.84 * (double)K2.sigma2[oct2])) pass = false;
          }
          if (pass) best = min(best, (dist << 20) | (uint32_t)(0xFFFFF - j));
        }
      }
      best = tri_wave_min_u32(best);
      if (best != 0xFFFFFFFFu) best2 = 0xFFFFF - (int)(best & 0xFFFFF);
    }
    if (lane == q) { my_best = best2; my_status = status; }
  }
  if (mine >= P.n1) return;
  // ---- the triangulation: one lane per feature, 64 winners of the wave at once ----
  float X[3] = {0.f, 0.f, 0.f};
  if (my_best >= 0 && P.triangulate) my_status = tri_point(A, P, K1, K2, mine, my_best, X);
  A.match[o] = my_best;
  if (P.triangulate) { A.status[o] = (uint8_t)my_status; A.x3d[3 * o] = X[0]; A.x3d[3 * o + 1] = X[1]; A.x3d[3 * o + 2] = X[2]; }
}

#define TRI_COMMIT_T 256
__device__ __forceinline__ int tri_rot_bin(float a1, float a2) {
  float rot = a1 - a2;
  if (rot < 0.0f) rot += 360.0f;
  int bin = (int)roundf(rot * (30.0f / 360.0f));
  if (bin == 30) bin = 0;
  return bin < 0 ? 0 : (bin > 29 ? 29 : bin);   // (angles outside [0, 360) would trip the reference's assert)
}

__global__ __launch_bounds__(TRI_COMMIT_T) void tri_commit(TriArrays A) {
  __shared__ uint32_t occ[(PS_TRI_MAX_N + 32) / 32];
  __shared__ int hist[30];
  __shared__ int s_nm, s_new;
  const TriProb& P = A.prob[blockIdx.x];
  const TriKf& K1 = A.kf[P.kf1];
  const int tid = threadIdx.x, n1 = P.n1;
  // the occupied slots of keyframe 1 as bits (a thread owns whole words)
  for (int w = tid; w < (n1 + 31) / 32; w += TRI_COMMIT_T) {
    uint32_t bits = 0;
    for (int b = 0; b < 32 && w * 32 + b < n1; b++) bits |= A.occ[K1.f_off + w * 32 + b] ? (1u << b) : 0u;
    occ[w] = bits;
  }
  if (tid == 0) s_new = 0;
  __syncthreads();
  for (int r = 0; r < P.k; r++) {
    const TriPair& R = A.pair[P.first_pair + r];
    const TriKf& K2 = A.kf[R.kf2];
    const size_t o = (size_t)R.out_off;
    if (tid < 30) hist[tid] = 0;
    if (tid == 0) s_nm = 0;
    __syncthreads();
    if (tri_neighbour_skipped(P, K1, K2)) {   // uniform; tri_match has marked the neighbour
      if (tid == 0) A.nmatch[P.first_pair + r] = 0;
      continue;
    }
    int nm = 0, nnew = 0;
    for (int i = tid; i < n1; i += TRI_COMMIT_T) {
      int m = A.match[o + i];
      if (P.chain && ((occ[i >> 5] >> (i & 31)) & 1u)) {   // a point sits in the slot, possibly one of an earlier neighbour (ORBmatcher.cc:826-830)
        if (m >= 0) A.match[o + i] = -1;
        m = -1;
        if (P.triangulate) A.status[o + i] = 2;
      }
      if (m >= 0) {
        nm++;
        if (P.check_ori) atomicAdd(&hist[tri_rot_bin(A.ang[K1.f_off + i], A.ang[K2.f_off + m])], 1);
      }
    }
    __syncthreads();
    int i1 = -1, i2 = -1, i3 = -1;
    if (P.check_ori) {   // ComputeThreeMaxima (ORBmatcher.cc:2658-2699)
      int max1 = 0, max2 = 0, max3 = 0;
      for (int i = 0; i < 30; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
      }
      if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
      else if ((float)max3 < 0.1f * (float)max1) { i3 = -1; }
    }
    for (int i = tid; i < n1; i += TRI_COMMIT_T) {
      const int m = A.match[o + i];
      if (m < 0) continue;
      if (P.check_ori) {
        const int b = tri_rot_bin(A.ang[K1.f_off + i], A.ang[K2.f_off + m]);
        if (b != i1 && b != i2 && b != i3) {
          A.match[o + i] = -1;
          if (P.triangulate) A.status[o + i] = 1;
          nm--;
          continue;
        }
      }
      if (P.triangulate && A.status[o + i] == 0) {   // mpCurrentKeyFrame->AddMapPoint(pMP, idx1) (LocalMapping.cc:693)
        nnew++;
        if (P.chain) atomicOr(&occ[i >> 5], 1u << (i & 31));
      }
    }
    if (nm) atomicAdd(&s_nm, nm);
    if (nnew) atomicAdd(&s_new, nnew);
    __syncthreads();
    if (tid == 0) A.nmatch[P.first_pair + r] = s_nm;
    __syncthreads();
  }
  if (tid == 0) A.nnew[blockIdx.x] = s_new;
}

}  // namespace

// Two launches whatever the batch holds.
extern "C" void psk_tri_launch(const TriArrays* arrays, int nprob, int npairs, int max_n1, hipStream_t st) {
  if (npairs > 0 && max_n1 > 0) hipLaunchKernelGGL(tri_match, dim3(npairs, (max_n1 + 255) / 256), dim3(256), 0, st, *arrays);
  hipLaunchKernelGGL(tri_commit, dim3(nprob), dim3(TRI_COMMIT_T), 0, st, *arrays);
}
