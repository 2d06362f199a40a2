// Device-side descriptors of ps_create_new_map_points (tri_kernels.hip): LocalMapping::CreateNewMapPoints' epipolar search and
// triangulation for a batch of keyframes, each with its ordered neighbours.
#pragma once
#include <stdint.h>
#define PS_TRI_MAX_N 8191      // features per keyframe: tri_commit keeps one occupied bit per feature of keyframe 1 in LDS
#define PS_TRI_MAX_K 32        // neighbours per keyframe (the reference asks for 10, 20 in the monocular setting)

// one keyframe as the kernels read it; its features are the slice [f_off, f_off + n) of the concatenated feature arrays
struct TriKf {
  int32_t f_off, n;
  int32_t raw_off;             // slice of xraw / yraw (mvKeys), -1: the same as x / y
  int32_t pad;
  float rcw[9], tcw[3], ow[3];
  float fx, fy, cx, cy, invfx, invfy, mb, mbf;
  float scale[8], sigma2[8];
};
struct TriProb {
  int32_t kf1;                 // index into kf
  int32_t first_pair, k, n1;
  int32_t only_stereo, check_ori, triangulate, chain;
  float ratio_factor;
  int32_t pad[3];
};
// one (keyframe 1, neighbour) pair.  node_off: U + 1 offsets, U = distinct nodes of keyframe 1; bucket c lists the features of
// the neighbour that sit in keyframe 1's c-th node, ascending, inside the neighbour's slice of `aux`
struct TriPair {
  int32_t prob, kf2, node_off, out_off;
  float f12[9];
  int32_t pad[3];
};
struct TriArrays {
  const TriProb* prob; const TriPair* pair; const TriKf* kf;
  const float* x; const float* y; const int32_t* oct; const float* ang; const float* ur; const float* depth;
  const float* xraw; const float* yraw;
  const uint8_t* desc; const uint8_t* occ;
  const int32_t* aux;          // keyframe 1: the feature's node as an index into the keyframe's distinct nodes (-1: none); neighbour: the bucket lists
  const int32_t* node_off;
  int32_t* match; int32_t* nmatch; float* x3d; uint8_t* status; int32_t* nnew;
};
