// Device-side descriptors of the batched Horn RANSAC (sim3solver_kernels.hip): ps_sim3_ransac.  A problem is one candidate keyframe
// pair: n correspondences in the two camera frames, nhyp hypotheses of three raw rand() values each.
#pragma once
#include <stdint.h>

#define PS_S3_MAX_N 32767       // correspondences per problem
#define PS_S3_MAX_HYP 4096      // hypotheses per problem
#define PS_S3_HB 64             // hypotheses per block: one lane each in the model stage
#define PS_S3_TILE 512          // correspondences staged in LDS at a time (a multiple of 64)
#define PS_S3_MODEL 13          // s, R row-major, t

struct S3Prob {
  int32_t n, nhyp;
  int32_t c_off;                // first correspondence in x1 / x2 / gate1 / gate2
  int32_t h_off;                // first hypothesis in draws / inliers / model
  int32_t nwords;               // ceil(n / 64): mask words per hypothesis
  int32_t fix_scale;
  int64_t m_off;                // first mask word
  float k1[4], k2[4];           // fx, fy, cx, cy of keyframe 1 / 2
};

struct S3Arrays {
  const S3Prob* prob;
  const float* x1; const float* x2;          // [..][3] camera-frame points
  const float* gate1; const float* gate2;    // mvnMaxError1 / 2 as floats (already truncated)
  const int32_t* draws;                      // [..][3]
  int32_t* inliers;                          // per hypothesis
  float* model;                              // [..][13]
  unsigned long long* mask;                  // per hypothesis nwords words
};
