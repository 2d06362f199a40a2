// ORB_SLAM2::Sim3Solver (/root/reference/include/Sim3Solver.h, src/Sim3Solver.cc) on the C-ABI, as a template over the caller's
// KeyFrame / MapPoint types: any types with the reference's member names compile (KeyFrame: GetMapPointMatches, GetRotation,
// GetTranslation, mvKeysUn, mvLevelSigma2, fx, fy, cx, cy - the entries of mK; MapPoint: isBad, GetIndexInKeyFrame, GetWorldPos).
// The constructor is the reference's (:38-113, with its skip rules and mvnIndices1).  ps_sim3_ransac evaluates all mRansacMaxIts
// hypotheses of a solver - PrepareBatch: of every live candidate of a loop query in one call - and iterate() only walks the cached
// counts: it returns the model, vbInliers over mN1, nInliers and bNoMore exactly as :141-208, with mnIterations carried between calls.
// The draws: 3 x mRansacMaxIts raw values are taken from the source of draws (std::rand by default, as the reference uses) when a
// solver is prepared, not lazily, so the global rand() order across solvers differs from the reference's.
#pragma once
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/pointslot_hip.h"
#include "slotcv.h"

namespace ORB_SLAM2 {

template <class KeyFrameT, class MapPointT>
class Sim3Solver {
 public:
  typedef std::function<int()> DrawSource;

  // handle: the matcher handle the call runs on (ORBmatcher::handle()); nullptr: the solver creates one of its own when it prepares
  Sim3Solver(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12, const bool bFixScale = true,
             ps_matcher* handle = nullptr, DrawSource draws = DrawSource())
      : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale), h_(handle), draws_(draws) {
    std::vector<MapPointT*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = (int)vpMatched12.size();
    const pscv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation(), Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
    for (int i1 = 0; i1 < mN1; i1++) {
      if (!vpMatched12[i1]) continue;
      MapPointT* pMP1 = vpKeyFrameMP1[i1];
      MapPointT* pMP2 = vpMatched12[i1];
      if (!pMP1) continue;
      if (pMP1->isBad() || pMP2->isBad()) continue;
      const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
      if (indexKF1 < 0 || indexKF2 < 0) continue;
      const float sigmaSquare1 = pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave];
      const float sigmaSquare2 = pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave];
      // mvnMaxError1 / 2 are std::vector<size_t>: the double 9.210 * sigma2 is truncated, and compared as a float
      mvnMaxError1.push_back((float)(size_t)(9.210 * sigmaSquare1));
      mvnMaxError2.push_back((float)(size_t)(9.210 * sigmaSquare2));
      mvnIndices1.push_back(i1);
      ToCamera(Rcw1, tcw1, pMP1->GetWorldPos(), mvX3Dc1);
      ToCamera(Rcw2, tcw2, pMP2->GetWorldPos(), mvX3Dc2);
    }
    mK1[0] = pKF1->fx; mK1[1] = pKF1->fy; mK1[2] = pKF1->cx; mK1[3] = pKF1->cy;
    mK2[0] = pKF2->fx; mK2[1] = pKF2->fy; mK2[2] = pKF2->cx; mK2[3] = pKF2->cy;
    SetRansacParameters();
  }
  ~Sim3Solver() { if (own_) ps_matcher_destroy(own_); }
  Sim3Solver(const Sim3Solver&) = delete;
  Sim3Solver& operator=(const Sim3Solver&) = delete;

  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    mRansacProb = probability; mRansacMinInliers = minInliers;
    N = (int)mvnIndices1.size();
    if (ps_sim3_ransac_iterations(probability, minInliers, maxIterations, N, &mRansacMaxIts) != PS_OK) throw std::runtime_error(ps_last_error());
    mnIterations = 0;
    prepared_ = false;
  }

  // Evaluates all mRansacMaxIts hypotheses of all live (N >= mRansacMinInliers), un-prepared solvers in one ps_sim3_ransac, on the
  // first live solver's handle.  An un-prepared solver prepares itself at its first iterate.
  static void PrepareBatch(const std::vector<Sim3Solver*>& vpSolvers) {
    std::vector<Sim3Solver*> todo;
    for (Sim3Solver* s : vpSolvers)
      if (s && !s->prepared_ && s->Live()) todo.push_back(s);
    if (todo.empty()) return;
    std::vector<ps_sim3_ransac_problem> probs(todo.size());
    for (size_t k = 0; k < todo.size(); k++) {
      Sim3Solver& S = *todo[k];
      const int nh = S.mRansacMaxIts, nw = (S.N + 63) / 64;
      S.draws3_.resize((size_t)3 * nh);
      for (int32_t& d : S.draws3_) d = S.draws_ ? S.draws_() : std::rand();
      S.inliers_.assign(nh, 0); S.model_.assign((size_t)13 * nh, 0.f); S.mask_.assign((size_t)nh * nw, 0);
      ps_sim3_ransac_problem& p = probs[k];
      p = ps_sim3_ransac_problem{};
      p.n = S.N; p.x3dc1 = S.mvX3Dc1.data(); p.x3dc2 = S.mvX3Dc2.data(); p.max_err1 = S.mvnMaxError1.data(); p.max_err2 = S.mvnMaxError2.data();
      for (int c = 0; c < 4; c++) { p.k1[c] = S.mK1[c]; p.k2[c] = S.mK2[c]; }
      p.fix_scale = S.mbFixScale ? 1 : 0; p.nhyp = nh; p.draws = S.draws3_.data(); p.min_inliers = S.mRansacMinInliers;
      p.inliers = S.inliers_.data(); p.model = S.model_.data(); p.mask = S.mask_.data();
    }
    if (ps_sim3_ransac(todo[0]->Handle(), probs.data(), (int)probs.size()) != PS_OK) throw std::runtime_error(ps_last_error());
    for (Sim3Solver* s : todo) s->prepared_ = true;
  }

  pscv::Mat find(std::vector<bool>& vbInliers12, int& nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
  }

  pscv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    if (!Live()) {   // N < mRansacMinInliers (fewer than three correspondences: the reference's draw is undefined)
      bNoMore = true;
      return pscv::Mat();
    }
    if (!prepared_) PrepareBatch(std::vector<Sim3Solver*>(1, this));
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
      const int h = mnIterations;
      nCurrentIterations++;
      mnIterations++;
      const int mnInliersi = inliers_[h];
      if (mnInliersi >= mnBestInliers) {
        Take(h);
        if (mnInliersi > mRansacMinInliers) {
          nInliers = mnInliersi;
          const uint64_t* w = &mask_[(size_t)h * ((N + 63) / 64)];
          for (int i = 0; i < N; i++)
            if ((w[i >> 6] >> (i & 63)) & 1) vbInliers[mvnIndices1[i]] = true;
          return mBestT12.clone();
        }
      }
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return pscv::Mat();
  }

  pscv::Mat GetEstimatedRotation() { return mBestRotation.clone(); }
  pscv::Mat GetEstimatedTranslation() { return mBestTranslation.clone(); }
  float GetEstimatedScale() { return mBestScale; }

  // what the constructor kept, for a binding that wants to look (the reference keeps them protected)
  int N = 0, mN1 = 0;
  std::vector<size_t> mvnIndices1;
  std::vector<float> mvX3Dc1, mvX3Dc2, mvnMaxError1, mvnMaxError2;   // [N][3], [N][3], [N], [N]
  int mnIterations, mnBestInliers;
  int mRansacMinInliers = 6, mRansacMaxIts = 300;
  double mRansacProb = 0.99;
  ps_matcher* Handle() {
    if (h_) return h_;
    if (!own_ && ps_matcher_create(0, &own_) != PS_OK) throw std::runtime_error(std::string("ps_matcher_create: ") + ps_last_error());
    return own_;
  }

 private:
  bool Live() const { return N >= mRansacMinInliers && N >= 3; }
  // Rcw * X3Dw + tcw (:96, :99): the product's three terms and their sum in double, rounded, then the float addition
  static void ToCamera(const pscv::Mat& R, const pscv::Mat& t, const pscv::Mat& X, std::vector<float>& out) {
    for (int r = 0; r < 3; r++) {
      const float p = (float)((double)R.at<float>(r, 0) * (double)X.at<float>(0) + (double)R.at<float>(r, 1) * (double)X.at<float>(1) +
                              (double)R.at<float>(r, 2) * (double)X.at<float>(2));
      out.push_back(p + t.at<float>(r));
    }
  }
  // hypothesis h becomes the best one: mBestT12 = [s R | t] with every entry of s R = float(double(R) * double(s)) (ORBmatcher::Sim3Pair)
  void Take(int h) {
    const float* m = &model_[(size_t)13 * h];
    mnBestInliers = inliers_[h];
    mBestScale = m[0];
    mBestRotation = pscv::Mat(3, 3, pscv::CV_32F); mBestTranslation = pscv::Mat(3, 1, pscv::CV_32F); mBestT12 = pscv::Mat(4, 4, pscv::CV_32F);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) {
        mBestRotation.at<float>(r, c) = m[1 + 3 * r + c];
        mBestT12.at<float>(r, c) = (float)((double)m[1 + 3 * r + c] * (double)m[0]);
      }
      mBestTranslation.at<float>(r) = m[10 + r];
      mBestT12.at<float>(r, 3) = m[10 + r];
      mBestT12.at<float>(3, r) = 0.f;
    }
    mBestT12.at<float>(3, 3) = 1.f;
  }

  bool mbFixScale;
  float mK1[4], mK2[4];
  pscv::Mat mBestT12, mBestRotation, mBestTranslation;
  float mBestScale = 0.f;
  ps_matcher* h_ = nullptr;
  ps_matcher* own_ = nullptr;
  DrawSource draws_;
  bool prepared_ = false;
  std::vector<int32_t> draws3_;
  std::vector<int32_t> inliers_;
  std::vector<float> model_;
  std::vector<uint64_t> mask_;
};

}  // namespace ORB_SLAM2
