// ORB_SLAM2::ORBVocabulary (/root/reference/include/ORBVocabulary.h: DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) on the
// C-ABI: the members Frame::ComputeBoW, KeyFrame::ComputeBoW, System's loader and KeyFrameDatabase-shaped callers use.
// DBoW2::BowVector / FeatureVector are the std::map types they are in the reference (BowVector.h, FeatureVector.h).
#pragma once
#include <cmath>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/pointslot_hip.h"
#include "slotcv.h"

namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
typedef unsigned int NodeId;
class BowVector : public std::map<WordId, WordValue> {};
class FeatureVector : public std::map<NodeId, std::vector<unsigned int>> {};
}  // namespace DBoW2

namespace ORB_SLAM2 {

class ORBVocabulary {
 public:
  explicit ORBVocabulary(int device = 0) : device_(device) {}
  ~ORBVocabulary() { clear(); }
  ORBVocabulary(const ORBVocabulary&) = delete;

  // TemplatedVocabulary::loadFromBinaryFile (TemplatedVocabulary.h:1343-1384); false where the reference would read garbage
  bool loadFromBinaryFile(const std::string& filename) {
    clear();
    if (ps_vocabulary_load_binary(device_, filename.c_str(), &v_) != PS_OK) return false;
    return ps_matcher_create(device_, &m_) == PS_OK;
  }
  // from records in file order (ps_vocabulary_create)
  bool create(int k, int L, int scoring, int weighting, int nnodes, const int32_t* parent, const uint8_t* desc, const float* weight, const uint8_t* is_leaf) {
    clear();
    if (ps_vocabulary_create(device_, k, L, scoring, weighting, nnodes, parent, desc, weight, is_leaf, &v_) != PS_OK) return false;
    return ps_matcher_create(device_, &m_) == PS_OK;
  }
  unsigned int size() const {
    int32_t words = 0;
    if (v_) ps_vocabulary_info(v_, nullptr, nullptr, nullptr, &words);
    return (unsigned int)words;
  }
  bool empty() const { return size() == 0; }
  const ps_vocabulary* handle() const { return v_; }
  int device() const { return device_; }

  // transform(features, BowVector&, FeatureVector&, levelsup) (:1133-1200).  features: one 1 x 32 CV_8U row per keypoint
  // (Converter::toDescriptorVector), or the descriptor matrix itself.  matcher: the handle whose stream runs the call; nullptr:
  // one the vocabulary keeps (calls on it are serialised).
  void transform(const std::vector<pscv::Mat>& features, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup, ps_matcher* matcher = nullptr) const {
    std::vector<uint8_t> rows(features.size() * 32 + 32, 0);
    for (std::size_t i = 0; i < features.size(); i++) std::memcpy(&rows[i * 32], features[i].ptr<uint8_t>(0), 32);
    transformRows(rows.data(), (int)features.size(), v, fv, levelsup, matcher);
  }
  void transform(const pscv::Mat& descriptors, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup, ps_matcher* matcher = nullptr) const {
    std::vector<uint8_t> rows((std::size_t)descriptors.rows * 32 + 32, 0);
    for (int i = 0; i < descriptors.rows; i++) std::memcpy(&rows[(std::size_t)i * 32], descriptors.ptr<uint8_t>(i), 32);
    transformRows(rows.data(), descriptors.rows, v, fv, levelsup, matcher);
  }
  // the struct-level batch call: many frames at once (include/pointslot_hip.h: ps_bow_problem)
  void transform(ps_bow_problem* frames, int n, ps_matcher* matcher = nullptr) const {
    if (n <= 0) return;
    if (!v_) throw std::runtime_error("ORBVocabulary: no vocabulary loaded");
    if (ps_bow_transform(matcher ? matcher : m_, v_, frames, n) != PS_OK) throw std::runtime_error(std::string("ps_bow_transform: ") + ps_last_error());
  }

  // L1Scoring::score (ScoringObject.cpp:23-68) on the host: 1 - 0.5 * |v1 - v2|_1 of two L1-normalised vectors, accumulated over
  // the words both hold, in ascending word order
  double score(const DBoW2::BowVector& v1, const DBoW2::BowVector& v2) const {
    double acc = 0;
    auto a = v1.begin();
    auto b = v2.begin();
    while (a != v1.end() && b != v2.end()) {
      if (a->first < b->first) a = v1.lower_bound(b->first);
      else if (b->first < a->first) b = v2.lower_bound(a->first);
      else { acc += std::fabs(a->second - b->second) - std::fabs(a->second) - std::fabs(b->second); ++a; ++b; }
    }
    return -acc / 2.0;
  }

 private:
  void clear() {
    if (m_) ps_matcher_destroy(m_);
    if (v_) ps_vocabulary_destroy(v_);
    m_ = nullptr; v_ = nullptr;
  }
  void transformRows(const uint8_t* rows, int n, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup, ps_matcher* matcher) const {
    v.clear();
    fv.clear();
    if (!v_ || n <= 0) return;                                  // `if(empty()) return;` (:1140)
    std::vector<int32_t> word((std::size_t)n), node((std::size_t)n), id((std::size_t)n);
    std::vector<double> val((std::size_t)n);
    ps_bow_problem p = ps_bow_problem{};
    p.n = n; p.desc = rows; p.levelsup = levelsup; p.word = word.data(); p.node = node.data(); p.bow_id = id.data(); p.bow_val = val.data();
    transform(&p, 1, matcher);
    for (int i = 0; i < p.bow_n; i++) v.insert(v.end(), std::make_pair((DBoW2::WordId)id[i], val[i]));
    for (int i = 0; i < n; i++)                                  // addFeature in feature order
      if (node[i] >= 0) fv[(DBoW2::NodeId)node[i]].push_back((unsigned int)i);
  }
  int device_ = 0;
  ps_vocabulary* v_ = nullptr;
  ps_matcher* m_ = nullptr;
};

}  // namespace ORB_SLAM2
