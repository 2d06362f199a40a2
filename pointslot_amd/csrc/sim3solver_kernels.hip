// CDNA4 kernel of the loop-closure Sim3 solver (ps_sim3_ransac): every hypothesis of every candidate pair of a batch in one launch.
//   Sim3Solver::iterate's draw (/root/reference/src/Sim3Solver.cc:164-178), ComputeSim3 (:227-338), CheckInliers / Project /
//   FromCameraToImage (:341-424), with DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50).
// A block serves PS_S3_HB hypotheses of one problem (grid = hypothesis blocks x problems, ragged through the problem table):
//   model stage : one lane per hypothesis - the three indices in closed form, Horn's closed-form model, parked in LDS (and written out)
//   check stage : the correspondences are staged once per block and tile in LDS as SoA (with their own projections, which no
//                 hypothesis changes); each wave owns a quarter of the block's hypotheses and sweeps (hypothesis, 64 correspondences)
//                 pairs, one correspondence per lane: the 64-bit ballot is the mask word, its popcount the running count.
// Float expressions are evaluated as written (-ffp-contract=off); cv::Mat products, Mat::dot and cv::norm accumulate in double.  The
// eigenvector is that of the float32 N, by cyclic Jacobi in FP64.  The readings of OpenCV-internal steps: DESIGN.md 4j.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <float.h>
#include "sim3solver_plan.h"
#include "match_device.h"

namespace {

// DUtils::Random::RandomInt(0, size - 1) on the raw rand() value r (RAND_MAX = 2^31 - 1)
__device__ __forceinline__ int s3_randint(int r, int size) { return (int)(((double)r / 2147483648.0) * (double)size); }

__device__ __forceinline__ double s3_dot3(const float* a, float x, float y, float z) {
  return (double)a[0] * (double)x + (double)a[1] * (double)y + (double)a[2] * (double)z;
}

// One Jacobi rotation in the (P, Q) plane of the symmetric A (both triangles kept) and of the eigenvector columns V.
template <int P, int Q> __device__ __forceinline__ void s3_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = 0.5 * (A[Q][Q] - A[P][P]) / apq;
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c), h = t * apq;
  A[P][P] -= h; A[Q][Q] += h; A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k != P && k != Q) {
      const double g = A[k][P], e = A[k][Q];
      const double gp = g - s * (e + g * tau), eq = e + s * (g - e * tau);
      A[k][P] = gp; A[P][k] = gp; A[k][Q] = eq; A[Q][k] = eq;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double g = V[k][P], e = V[k][Q];
    V[k][P] = g - s * (e + g * tau); V[k][Q] = e + s * (g - e * tau);
  }
}

// ComputeSim3 on the three correspondences a[i], b[i] (camera 1 / camera 2): s, R, t12 into m[13]; sR12 / t12 / sR21 / t21 into T[24]
__device__ void s3_model(const float (&P1)[3][3], const float (&P2)[3][3], int fix_scale, float* m, float* T) {
  // P[r][i]: coordinate r of point i.  Centroid: cv::reduce sums in float; C / 3 = float(double(C) * (1.0 / 3.0))
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    O1[r] = (float)((double)((P1[r][0] + P1[r][1]) + P1[r][2]) * (1.0 / 3.0));
    O2[r] = (float)((double)((P2[r][0] + P2[r][1]) + P2[r][2]) * (1.0 / 3.0));
#pragma unroll
    for (int i = 0; i < 3; i++) { Pr1[r][i] = P1[r][i] - O1[r]; Pr2[r][i] = P2[r][i] - O2[r]; }
  }
  float M[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) M[r][c] = (float)s3_dot3(Pr2[r], Pr1[c][0], Pr1[c][1], Pr1[c][2]);
  const double m00 = M[0][0], m01 = M[0][1], m02 = M[0][2], m10 = M[1][0], m11 = M[1][1], m12 = M[1][2], m20 = M[2][0], m21 = M[2][1], m22 = M[2][2];
  const float N11 = (float)(m00 + m11 + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02), N14 = (float)(m01 - m10);
  const float N22 = (float)(m00 - m11 - m22), N23 = (float)(m01 + m10), N24 = (float)(m20 + m02);
  const float N33 = (float)(-m00 + m11 - m22), N34 = (float)(m12 + m21), N44 = (float)(-m00 - m11 + m22);
  double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 16; sweep++) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
    if (off <= 1e-40 * dia) break;
    s3_rotate<0, 1>(A, V); s3_rotate<0, 2>(A, V); s3_rotate<0, 3>(A, V);
    s3_rotate<1, 2>(A, V); s3_rotate<1, 3>(A, V); s3_rotate<2, 3>(A, V);
  }
  double q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]}, best = A[0][0];
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (A[k][k] > best) { best = A[k][k]; q[0] = V[0][k]; q[1] = V[1][k]; q[2] = V[2][k]; q[3] = V[3][k]; }
  if (q[0] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  const float e0 = (float)q[0], e1 = (float)q[1], e2 = (float)q[2], e3 = (float)q[3];
  // ang = atan2(norm(vec), evec(0, 0)); vec = 2 * ang * vec / norm(vec): one scale (2 ang) * (1 / norm) on double(vec), rounded once.
  // A zero imaginary part gives 0 * inf = NaN, as in the reference: every later comparison is false.
  const double nrm = sqrt((double)e1 * (double)e1 + (double)e2 * (double)e2 + (double)e3 * (double)e3);
  const double ang = atan2(nrm, (double)e0);
  const double a = (2.0 * ang) * (1.0 / nrm);
  const float v0 = (float)((double)e1 * a), v1 = (float)((double)e2 * a), v2 = (float)((double)e3 * a);
  // cv::Rodrigues on a float vector: in double, R = c I + (1 - c) r r^T + s [r]x, rounded to float
  float R[3][3];
  {
    double rx = v0, ry = v1, rz = v2;
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[r][c] = r == c ? 1.f : 0.f;
    } else {
      const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
      rx *= it; ry *= it; rz *= it;
      const double rv[3] = {rx, ry, rz};
      const double cr[3][3] = {{0.0, -rz, ry}, {rz, 0.0, -rx}, {-ry, rx, 0.0}};
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) R[r][k] = (float)((c * (r == k ? 1.0 : 0.0) + c1 * (rv[r] * rv[k])) + s * cr[r][k]);
    }
  }
  float s12 = 1.0f;
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const float p3 = (float)s3_dot3(R[r], Pr2[0][i], Pr2[1][i], Pr2[2][i]);
        nom += (double)Pr1[r][i] * (double)p3;
        den += (double)(p3 * p3);
      }
    s12 = (float)(nom / den);
  }
  m[0] = s12;
  const double sd = (double)s12, inv = 1.0 / (double)s12;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float t = (float)((double)O1[r] - sd * s3_dot3(R[r], O2[0], O2[1], O2[2]));
    m[10 + r] = t; T[9 + r] = t;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      m[1 + 3 * r + c] = R[r][c];
      T[3 * r + c] = (float)((double)R[r][c] * sd);          // sR12
      T[12 + 3 * r + c] = (float)((double)R[c][r] * inv);    // sR21
    }
  }
#pragma unroll
  for (int r = 0; r < 3; r++) T[21 + r] = (float)(-s3_dot3(&T[12 + 3 * r], T[9], T[10], T[11]));
}

// 30 KB of LDS per block (the tile and the block's models), 256 threads: two blocks per CU by LDS.  The model stage is FP64 on one
// wave; the check stage is float with three double dot products per projection.
__global__ __launch_bounds__(256) void s3_ransac(S3Arrays A) {
  __shared__ float sx[12][PS_S3_TILE];          // x1 (0..2), x2 (3..5), u1 v1 (6, 7), u2 v2 (8, 9), gate1, gate2
  __shared__ float smod[24][PS_S3_HB];          // sR12, t12, sR21, t21 per hypothesis
  __shared__ int scnt[PS_S3_HB];
  const S3Prob& P = A.prob[blockIdx.y];
  const int n = P.n, h0 = blockIdx.x * PS_S3_HB;
  if (h0 >= P.nhyp) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nh = min(PS_S3_HB, P.nhyp - h0);
  if (tid < nh) {
    const int hg = P.h_off + h0 + tid;
    // the draw without replacement over 0 .. n - 1 (pick, move the back element into the slot, pop) after one, two removals
    const int r0 = s3_randint(A.draws[3 * hg], n), r1 = s3_randint(A.draws[3 * hg + 1], n - 1), r2 = s3_randint(A.draws[3 * hg + 2], n - 2);
    const int i0 = r0;
    const int i1 = r1 == r0 ? n - 1 : r1;
    const int back = (n - 2 == r0) ? n - 1 : n - 2;          // the back element at the second removal
    const int i2 = r2 == r1 ? back : (r2 == r0 ? n - 1 : r2);
    const int idx[3] = {i0, i1, i2};
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const size_t c = (size_t)(P.c_off + idx[i]) * 3;
#pragma unroll
      for (int r = 0; r < 3; r++) { P1[r][i] = A.x1[c + r]; P2[r][i] = A.x2[c + r]; }
    }
    float m[PS_S3_MODEL], T[24];
    s3_model(P1, P2, P.fix_scale, m, T);
#pragma unroll
    for (int k = 0; k < PS_S3_MODEL; k++) A.model[(size_t)hg * PS_S3_MODEL + k] = m[k];
#pragma unroll
    for (int k = 0; k < 24; k++) smod[k][tid] = T[k];
  }
  if (tid < PS_S3_HB) scnt[tid] = 0;
  const float fx1 = P.k1[0], fy1 = P.k1[1], cx1 = P.k1[2], cy1 = P.k1[3], fx2 = P.k2[0], fy2 = P.k2[1], cx2 = P.k2[2], cy2 = P.k2[3];
  for (int base = 0; base < n; base += PS_S3_TILE) {
    const int nt = min(PS_S3_TILE, n - base);
    __syncthreads();                            // the models are parked / the previous tile is done with
    for (int i = tid; i < nt; i += 256) {
      const size_t c = (size_t)(P.c_off + base + i);
      const float X1 = A.x1[3 * c], Y1 = A.x1[3 * c + 1], Z1 = A.x1[3 * c + 2], X2 = A.x2[3 * c], Y2 = A.x2[3 * c + 1], Z2 = A.x2[3 * c + 2];
      sx[0][i] = X1; sx[1][i] = Y1; sx[2][i] = Z1; sx[3][i] = X2; sx[4][i] = Y2; sx[5][i] = Z2;
      const float iz1 = 1.0f / Z1, iz2 = 1.0f / Z2;            // FromCameraToImage: no positivity test
      sx[6][i] = fx1 * (X1 * iz1) + cx1; sx[7][i] = fy1 * (Y1 * iz1) + cy1;
      sx[8][i] = fx2 * (X2 * iz2) + cx2; sx[9][i] = fy2 * (Y2 * iz2) + cy2;
      sx[10][i] = A.gate1[c]; sx[11][i] = A.gate2[c];
    }
    __syncthreads();
    const int nsub = (nt + 63) >> 6;
    for (int h = wave; h < nh; h += 4) {
      float T[24];
#pragma unroll
      for (int k = 0; k < 24; k++) T[k] = smod[k][h];
      int count = 0;
      for (int sub = 0; sub < nsub; sub++) {
        const int i = sub * 64 + lane;
        bool in = false;
        if (i < nt) {
          const float X1 = sx[0][i], Y1 = sx[1][i], Z1 = sx[2][i], X2 = sx[3][i], Y2 = sx[4][i], Z2 = sx[5][i];
          // Project(mvX3Dc2, T12, K1) against mvP1im1
          const float ax = dot3_f(&T[0], X2, Y2, Z2) + T[9], ay = dot3_f(&T[3], X2, Y2, Z2) + T[10], az = dot3_f(&T[6], X2, Y2, Z2) + T[11];
          const float ia = 1.0f / az;
          const float d0 = sx[6][i] - (fx1 * (ax * ia) + cx1), d1 = sx[7][i] - (fy1 * (ay * ia) + cy1);
          const float err1 = (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
          // Project(mvX3Dc1, T21, K2) against mvP2im2
          const float bx = dot3_f(&T[12], X1, Y1, Z1) + T[21], by = dot3_f(&T[15], X1, Y1, Z1) + T[22], bz = dot3_f(&T[18], X1, Y1, Z1) + T[23];
          const float ib = 1.0f / bz;
          const float g0 = (fx2 * (bx * ib) + cx2) - sx[8][i], g1 = (fy2 * (by * ib) + cy2) - sx[9][i];
          const float err2 = (float)((double)g0 * (double)g0 + (double)g1 * (double)g1);
          in = err1 < sx[10][i] && err2 < sx[11][i];
        }
        const unsigned long long word = __ballot(in);
        count += __popcll(word);
        if (P.m_off >= 0 && lane == 0) A.mask[(size_t)P.m_off + (size_t)(h0 + h) * P.nwords + (base >> 6) + sub] = word;
      }
      if (lane == 0) scnt[h] += count;          // hypothesis h belongs to this wave alone
    }
  }
  __syncthreads();
  if (tid < nh) A.inliers[P.h_off + h0 + tid] = scnt[tid];
}

}  // namespace

extern "C" void psk_s3_launch(const S3Arrays* arrays, int nprob, int max_hyp, hipStream_t st) {
  const S3Arrays A = *arrays;
  hipLaunchKernelGGL(s3_ransac, dim3((max_hyp + PS_S3_HB - 1) / PS_S3_HB, nprob), dim3(256), 0, st, A);
}
