// Test scaffolding, NOT the reference's data model: the members of KeyFrame and Frame (/root/reference/include/{KeyFrame,Frame}.h)
// that ComputeBoW and ORBmatcher::SearchByBoW read or write, under the reference's own names, on top of the types of
// keyframe_view.h / frame_view.h - so that the reference-signature templates of pointslot_amd/host/ORBmatcher.h and
// ORBVocabulary.h can be instantiated without OpenCV / DBoW2 / the rest of ORB_SLAM2.
#pragma once
#include <vector>
#include "keyframe_view.h"
#include "ORBVocabulary.h"

namespace ORB_SLAM2 {

struct BowKeyFrame : KeyFrame {
  DBoW2::BowVector mBowVec;
  DBoW2::FeatureVector mFeatVec;          // (hides the plain map of keyframe_view.h: the DBoW2 type, as in the reference)
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  // KeyFrame::ComputeBoW (KeyFrame.cc:114-123)
  void ComputeBoW(const ORBVocabulary& voc) {
    if (mBowVec.empty() || mFeatVec.empty()) voc.transform(mDescriptors, mBowVec, mFeatVec, 4);
  }
};

struct BowFrame : Frame {
  DBoW2::BowVector mBowVec;
  DBoW2::FeatureVector mFeatVec;
  // Frame::ComputeBoW (Frame.cc:2040-2047)
  void ComputeBoW(const ORBVocabulary& voc) {
    if (mBowVec.empty()) voc.transform(mDescriptors, mBowVec, mFeatVec, 4);
  }
};

}  // namespace ORB_SLAM2
