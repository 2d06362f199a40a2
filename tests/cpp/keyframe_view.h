// Test scaffolding, NOT the reference's data model: a plain struct carrying exactly the members of KeyFrame
// (/root/reference/include/KeyFrame.h) that ORBmatcher::SearchForTriangulation and LocalMapping::CreateNewMapPoints read, under
// the reference's own names - so that the reference-signature template of pointslot_amd/host/ORBmatcher.h can be instantiated
// and exercised without OpenCV / DBoW2 / the rest of ORB_SLAM2.  Mutexes and bookkeeping are left out.
#pragma once
#include <map>
#include <vector>
#include "frame_view.h"

namespace ORB_SLAM2 {

struct KeyFrame {
  long unsigned int mnId = 0;
  int N = 0;
  std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
  std::vector<float> mvuRight, mvDepth;
  cv::Mat mDescriptors;
  std::map<unsigned int, std::vector<unsigned int>> mFeatVec;   // DBoW2::FeatureVector: node id -> features, ascending
  std::vector<MapPoint*> mvpMapPoints;
  float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mbf = 0, mb = 0;
  std::vector<float> mvScaleFactors, mvLevelSigma2;
  cv::Mat Rcw, tcw, Ow;

  KeyFrame() : Rcw(3, 3, cv::CV_32F), tcw(3, 1, cv::CV_32F), Ow(3, 1, cv::CV_32F) {}
  MapPoint* GetMapPoint(const std::size_t& idx) { return mvpMapPoints[idx]; }
  cv::Mat GetRotation() { return Rcw.clone(); }
  cv::Mat GetTranslation() { return tcw.clone(); }
  cv::Mat GetCameraCenter() { return Ow.clone(); }
};

}  // namespace ORB_SLAM2
