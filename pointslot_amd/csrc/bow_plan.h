// Device-side descriptors of the bag-of-words calls (bow_kernels.hip): the vocabulary tree, ps_bow_transform and ps_search_by_bow.
#pragma once
#include <stdint.h>
#define PS_BOW_MAX_N 8191        // features per frame / per side: the BowVector sort and the taken bits of a node live in LDS

// One child slot of the tree.  The children of a node are the run [off, off + child_cnt) of slot / child_desc: a sibling group is
// contiguous and 32-byte aligned, in child-list order (record order).  A slot says everything the descent needs once it has
// chosen that child, so a level costs one round trip to memory: the 16 lanes of a row fetch descriptor and slot of "their" child
// side by side, and the winner's slot travels inside the row.  The root's children start at slot 0.
struct BowSlot {
  int32_t id;                    // NodeId of the child
  int32_t off_or_word;           // inner node: first slot of its children; leaf: its WordId
  int32_t child_cnt;             // 0: a leaf
  float weight;
};
struct BowTree {
  const BowSlot* slot;           // [nodes - 1]
  const uint8_t* child_desc;     // [nodes - 1][32] descriptor per child slot
  const float* word_weight;      // [words]
  int32_t root_cnt;              // children of the root
  int32_t L, weighting, nodes, words;
};
// one frame of a transform call; its features are the slice [f_off, f_off + n) of desc / word / node, its BowVector at most n
// entries from the same offset of bow_id / bow_val
struct BowFrame {
  int32_t f_off, n, levelsup, pad;
};
struct BowTransformArrays {
  BowTree tree;
  const BowFrame* frame;
  const uint8_t* desc;
  const int32_t* feat_frame;     // per block of 16 features: the frame (features of a frame start at a multiple of 16)
  int32_t* word; int32_t* node;
  int32_t* bow_id; double* bow_val; int32_t* bow_n;
  int32_t nblocks16;
};

// one search problem; side a's features are [a_off, a_off + a_n) of desc / ang / hasp, side b's [b_off, ..)
struct BowSProb {
  int32_t a_off, a_n, b_off, b_n;
  int32_t mode, check_ori;
  float nn_ratio;
  int32_t out_off, out_n;        // match slice: mode 0 b_n entries, mode 1 a_n entries
  int32_t pad[3];
};
// one vocabulary node present on both sides of a problem: the features of a in it are lst[a0 .. a1) (ascending indices into the
// side), those of b lst[b0 .. b1)
struct BowSItem {
  int32_t prob, a0, a1, b0, b1, pad[3];
};
struct BowSearchArrays {
  const BowSProb* prob; const BowSItem* item;
  const uint8_t* desc; const float* ang; const uint8_t* hasp;
  const int32_t* lst;
  int32_t* match; int32_t* nmatch;
  int32_t nitems, nprob;
};
