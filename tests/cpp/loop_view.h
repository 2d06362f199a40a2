// Test scaffolding, NOT the reference's data model: the members of KeyFrame, Frame and MapPoint
// (/root/reference/include/{KeyFrame,Frame,MapPoint}.h) that the loop-closure and relocalisation matchers - SearchBySim3,
// SearchByProjection(pKF, Scw, ..), Fuse(pKF, Scw, ..) and SearchByProjection(CurrentFrame, pKF, ..) - read or write, under the
// reference's own names, so that the reference-signature templates of pointslot_amd/host/ORBmatcher.h can be instantiated without
// OpenCV / the rest of ORB_SLAM2.  Mutexes and bookkeeping are left out.
#pragma once
#include <cmath>
#include <map>
#include <set>
#include <vector>
#include "frame_view.h"

namespace ORB_SLAM2 {

struct LoopKeyFrame;

struct LoopMapPoint : MapPoint {
  cv::Mat mNormalVector;
  float mfMinDistance = 0.f, mfMaxDistance = 0.f;          // protected in the reference: a binding makes them readable
  std::map<LoopKeyFrame*, std::size_t> mObservations;
  LoopMapPoint() : mNormalVector(3, 1, cv::CV_32F) {}
  cv::Mat GetNormal() const { return mNormalVector.clone(); }
  float GetMinDistanceInvariance() const { return 0.8f * mfMinDistance; }
  float GetMaxDistanceInvariance() const { return 1.2f * mfMaxDistance; }
  void AddObservation(LoopKeyFrame* pKF, std::size_t idx) {
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs++;
  }
  int GetIndexInKeyFrame(LoopKeyFrame* pKF) const {
    const auto it = mObservations.find(pKF);
    return it == mObservations.end() ? -1 : (int)it->second;
  }
};

struct LoopKeyFrame {
  int N = 0;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;
  cv::Mat mDescriptors;
  std::vector<std::vector<std::vector<std::size_t>>> mGrid;   // [mnGridCols][mnGridRows], private in the reference
  int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
  float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0;
  std::vector<float> mvScaleFactors;
  float mfLogScaleFactor = 0;
  int mnScaleLevels = 0;
  cv::Mat Rcw, tcw;
  std::vector<LoopMapPoint*> mvpMapPoints;

  LoopKeyFrame() : Rcw(3, 3, cv::CV_32F), tcw(3, 1, cv::CV_32F) {}
  cv::Mat GetRotation() { return Rcw.clone(); }
  cv::Mat GetTranslation() { return tcw.clone(); }
  LoopMapPoint* GetMapPoint(const std::size_t& idx) { return mvpMapPoints[idx]; }
  std::vector<LoopMapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  std::set<LoopMapPoint*> GetMapPoints() {                                           // KeyFrame.cc:261-275
    std::set<LoopMapPoint*> s;
    for (LoopMapPoint* p : mvpMapPoints)
      if (p && !p->isBad()) s.insert(p);
    return s;
  }
  void AddMapPoint(LoopMapPoint* pMP, const std::size_t& idx) { mvpMapPoints[idx] = pMP; }
  void AssignFeaturesToGrid() {                                                      // Frame.cc:1636-1656, copied by KeyFrame::KeyFrame
    mGrid.assign(FRAME_GRID_COLS, std::vector<std::vector<std::size_t>>(FRAME_GRID_ROWS));
    for (int i = 0; i < N; i++) {
      const int gx = (int)std::round((mvKeysUn[i].pt.x - mnMinX) * mfGridElementWidthInv);
      const int gy = (int)std::round((mvKeysUn[i].pt.y - mnMinY) * mfGridElementHeightInv);
      if (gx < 0 || gx >= FRAME_GRID_COLS || gy < 0 || gy >= FRAME_GRID_ROWS) continue;
      mGrid[gx][gy].push_back(i);
    }
  }
};

struct LoopFrame : Frame {
  float mfLogScaleFactor = 0;
  int mnScaleLevels = 0;
};

}  // namespace ORB_SLAM2
