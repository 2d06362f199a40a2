// ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:41-310 of the reference) on the C-ABI: add, erase,
// clear, DetectLoopCandidates and DetectRelocalizationCandidates under the reference's signatures, as templates over KeyFrame- /
// Frame-shaped types: mnId, mBowVec (DBoW2::BowVector), and on a keyframe GetConnectedKeyFrames() -> std::set<KeyFrame*> and
// GetBestCovisibilityKeyFrames(int) -> std::vector<KeyFrame*>.  `typedef KeyFrameDatabaseT<KeyFrame> KeyFrameDatabase;` gives the
// reference's class.  The store and the search run on the device (ps_kfdb_query); the covisibility stage is the library's
// host-only ps_kfdb_select, fed from the caller's covisibility graph.  mMutex guards the database as in the reference: the
// search part of a query holds it, the covisibility stage does not.
// Limits the reference does not have: `capacity` live keyframes (at most 4096) and `max_words` words per stored BowVector; an add
// beyond either throws.  KeyFrame::mRelocScore is modelled by the database (0 at add; include/pointslot_hip.h).
#pragma once
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>
#include "ORBVocabulary.h"

namespace ORB_SLAM2 {

template <class KeyFrameT>
class KeyFrameDatabaseT {
 public:
  explicit KeyFrameDatabaseT(const ORBVocabulary& voc, int capacity = 4096, int max_words = 2048) : mpVoc(&voc) {
    if (ps_kfdb_create(voc.device(), capacity, max_words, &db_) != PS_OK || ps_matcher_create(voc.device(), &m_) != PS_OK) {
      const std::string why = ps_last_error();
      release();
      throw std::runtime_error("KeyFrameDatabase: " + why);
    }
  }
  ~KeyFrameDatabaseT() { release(); }
  KeyFrameDatabaseT(const KeyFrameDatabaseT&) = delete;
  KeyFrameDatabaseT& operator=(const KeyFrameDatabaseT&) = delete;

  // void add(KeyFrame* pKF)                                                                                                  :41-47
  void add(KeyFrameT* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    std::vector<int32_t> id;
    std::vector<double> val;
    unpack(pKF->mBowVec, id, val);
    const int64_t kid = (int64_t)pKF->mnId;
    const int32_t* pid = id.data();
    const double* pval = val.data();
    const int32_t n = (int32_t)id.size();
    if (ps_kfdb_add(db_, m_, &kid, &pid, &pval, &n, 1, nullptr) != PS_OK) throw std::runtime_error(std::string("KeyFrameDatabase::add: ") + ps_last_error());
    mKeyFrames[kid] = pKF;
  }
  // void erase(KeyFrame* pKF)                                                                                                :49-68
  void erase(KeyFrameT* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    const int64_t kid = (int64_t)pKF->mnId;
    const auto it = mKeyFrames.find(kid);
    if (it == mKeyFrames.end() || it->second != pKF) return;
    ps_kfdb_erase(db_, &kid, 1);
    mKeyFrames.erase(it);
  }
  // void clear()                                                                                                             :70-74
  void clear() {
    std::unique_lock<std::mutex> lock(mMutex);
    ps_kfdb_clear(db_);
    mKeyFrames.clear();
  }
  std::size_t size() const { return mKeyFrames.size(); }
  ps_kfdb* handle() { return db_; }
  ps_matcher* matcher() { return m_; }

  // std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore)                                               :77-198
  std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore) {
    std::vector<int64_t> connected;
    for (KeyFrameT* c : pKF->GetConnectedKeyFrames()) connected.push_back((int64_t)c->mnId);
    return detect(pKF->mBowVec, 1, minScore, connected);
  }
  // std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F)                                                          :200-310
  template <class FrameT>
  std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F) {
    return detect(F->mBowVec, 0, 0.f, std::vector<int64_t>());
  }
  // mpORBVocabulary->score(CurrentBowVec, pKF->mBowVec) for stored keyframes, on the device: LoopClosing::DetectLoop's minScore loop
  // (src/LoopClosing.cc:127-141).  A keyframe that is not stored gives NaN.
  std::vector<double> score(const DBoW2::BowVector& v, const std::vector<KeyFrameT*>& vpKFs) {
    std::unique_lock<std::mutex> lock(mMutex);
    std::vector<int32_t> id;
    std::vector<double> val, out(vpKFs.size());
    unpack(v, id, val);
    std::vector<int64_t> ids;
    for (KeyFrameT* k : vpKFs) ids.push_back((int64_t)k->mnId);
    const int rc = ps_kfdb_score(db_, m_, id.data(), val.data(), (int)id.size(), ids.data(), (int)ids.size(), out.data());
    if (rc != PS_OK && rc != PS_ERR_INVALID) throw std::runtime_error(std::string("KeyFrameDatabase::score: ") + ps_last_error());
    return out;
  }

 protected:
  const ORBVocabulary* mpVoc;
  std::mutex mMutex;

 private:
  static void unpack(const DBoW2::BowVector& v, std::vector<int32_t>& id, std::vector<double>& val) {
    id.clear(); val.clear();
    for (const auto& kv : v) { id.push_back((int32_t)kv.first); val.push_back(kv.second); }
  }
  std::vector<KeyFrameT*> detect(const DBoW2::BowVector& bow, int mode, float minScore, const std::vector<int64_t>& connected) {
    std::vector<int32_t> id;
    std::vector<double> val;
    unpack(bow, id, val);
    std::vector<int64_t> share_id;
    std::vector<int32_t> share_words;
    std::vector<float> share_score;
    std::vector<KeyFrameT*> listed;
    ps_kfdb_query_problem p = ps_kfdb_query_problem{};
    {
      std::unique_lock<std::mutex> lock(mMutex);
      const std::size_t room = mKeyFrames.size() + 1;
      share_id.resize(room); share_words.resize(room); share_score.resize(room);
      p.n = (int32_t)id.size(); p.bow_id = id.data(); p.bow_val = val.data(); p.mode = mode;
      p.nexcluded = (int32_t)connected.size(); p.excluded = connected.data();
      p.share_id = share_id.data(); p.share_words = share_words.data(); p.share_score = share_score.data();
      if (ps_kfdb_query(db_, m_, &p, 1) != PS_OK) throw std::runtime_error(std::string("KeyFrameDatabase: ") + ps_last_error());
      for (int i = 0; i < p.nshare; i++) listed.push_back(mKeyFrames[share_id[i]]);
    }
    if (p.nshare == 0) return std::vector<KeyFrameT*>();
    std::vector<int64_t> neigh((std::size_t)p.nshare * 10, 0), cand((std::size_t)p.nshare);
    std::vector<int32_t> neigh_n((std::size_t)p.nshare, 0);
    for (int i = 0; i < p.nshare; i++) {
      if (!(share_words[i] > p.min_common_words)) continue;
      const std::vector<KeyFrameT*> vpNeighs = listed[i]->GetBestCovisibilityKeyFrames(10);
      for (std::size_t k = 0; k < vpNeighs.size() && k < 10; k++) neigh[(std::size_t)i * 10 + neigh_n[i]++] = (int64_t)vpNeighs[k]->mnId;
    }
    int32_t ncand = 0;
    if (ps_kfdb_select(mode, minScore, share_id.data(), share_words.data(), share_score.data(), p.nshare, p.min_common_words, neigh.data(), neigh_n.data(),
                       cand.data(), &ncand) != PS_OK)
      throw std::runtime_error(std::string("KeyFrameDatabase: ") + ps_last_error());
    std::map<int64_t, KeyFrameT*> at;
    for (int i = 0; i < p.nshare; i++) at[share_id[i]] = listed[i];
    std::vector<KeyFrameT*> out;
    for (int i = 0; i < ncand; i++) out.push_back(at[cand[i]]);
    return out;
  }
  void release() {
    if (m_) ps_matcher_destroy(m_);
    if (db_) ps_kfdb_destroy(db_);
    m_ = nullptr; db_ = nullptr;
  }
  ps_kfdb* db_ = nullptr;
  ps_matcher* m_ = nullptr;
  std::map<int64_t, KeyFrameT*> mKeyFrames;     // the stored keyframes by mnId
};

}  // namespace ORB_SLAM2
