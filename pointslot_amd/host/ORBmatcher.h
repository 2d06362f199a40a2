// ORB_SLAM2::ORBmatcher hot members (/root/reference/include/ORBmatcher.h:47-118) on the C-ABI.  The reference's
// methods take Frame& and write MapPoint* into it; Frame / MapPoint are outside the hot path and are not rebuilt.  Two
// layers: (i) the reference's own signatures as templates over the caller's Frame / MapPoint types (the marshalling of
// INTEGRATION.md section 2 and the pointer write-back, tested on tests/cpp/frame_view.h), (ii) underneath, methods that
// take the ps_*_problem structs directly for callers that already keep their data as arrays.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/pointslot_hip.h"
#include "slotcv.h"

namespace ORB_SLAM2 {

class ORBmatcher {
 public:
  static const int TH_LOW = 50, TH_HIGH = 100, TH_HIGH_FORDYNAMIC = 130, RADIUS_FORDYNAMIC = 5, HISTO_LENGTH = 30;

  ORBmatcher(float nnratio = 0.6, bool checkOri = true, int device = 0) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {
    if (ps_matcher_create(device, &h_) != PS_OK) throw std::runtime_error(std::string("ps_matcher_create: ") + ps_last_error());
  }
  ~ORBmatcher() { ps_matcher_destroy(h_); }
  ORBmatcher(const ORBmatcher&) = delete;

  // Computes the Hamming distance between two ORB descriptors (ORBmatcher.cc:2704-2720).  A single pair stays on the
  // host (same SWAR arithmetic); the bulk form is DescriptorDistanceMatrix.
  static int DescriptorDistance(const pscv::Mat& a, const pscv::Mat& b) {
    const int32_t* pa = a.ptr<int32_t>();
    const int32_t* pb = b.ptr<int32_t>();
    int dist = 0;
    for (int i = 0; i < 8; i++, pa++, pb++) {
      unsigned int v = *pa ^ *pb;
      v = v - ((v >> 1) & 0x55555555);
      v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
      dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
    }
    return dist;
  }
  void DescriptorDistanceMatrix(const pscv::Mat& q, const pscv::Mat& t, std::vector<uint16_t>& out) {
    out.resize((size_t)q.rows * t.rows);
    if (ps_hamming_matrix(h_, q.data, q.rows, t.data, t.rows, out.data()) != PS_OK) throw std::runtime_error(ps_last_error());
  }

  // SearchByBruceMatching(LastFrame, CurrentFrame, nLastOrder, nCurrenOrder, matches) for a batch of objects:
  // fills ps_bf_problem::query_of_train / nmatches (see include/pointslot_hip.h).  Returns the summed match count.
  int SearchByBruceMatching(std::vector<ps_bf_problem>& objects) {
    if (objects.empty()) return 0;
    if (ps_match_bruteforce(h_, objects.data(), (int)objects.size(), mfNNratio, mbCheckOrientation ? 1 : 0) != PS_OK)
      throw std::runtime_error(ps_last_error());
    int n = 0;
    for (const ps_bf_problem& o : objects) n += o.nmatches;
    return n;
  }

  // The three SearchByProjection overloads; the caller fills ps_proj_problem from its Frame.
  // th_dist / ratio_test / check_orientation are set here from the overload being emulated.
  static void ConfigureProjectionFrame(ps_proj_problem& p, float nnratio, bool checkOri) {   // (Frame& cur, const Frame& last, th, bMono)
    p.frame_mode = 1; p.th_dist = TH_HIGH; p.ratio_test = 0; p.nn_ratio = nnratio; p.check_orientation = checkOri ? 1 : 0; p.use_bbox = 0;
  }
  static void ConfigureProjectionPoints(ps_proj_problem& p, float nnratio) {                 // (Frame& F, const vector<MapPoint*>&, th)
    p.frame_mode = 0; p.th_dist = TH_HIGH; p.ratio_test = 1; p.nn_ratio = nnratio; p.check_orientation = 0; p.use_bbox = 0;
  }
  static void ConfigureProjectionObject(ps_proj_problem& p, float nnratio) {                 // (Frame& F, nOrder, const vector<MapObjectPoint*>&, th)
    p.frame_mode = 0; p.th_dist = TH_HIGH_FORDYNAMIC; p.ratio_test = 1; p.nn_ratio = nnratio; p.check_orientation = 0; p.use_bbox = 1;
  }
  // frame: nullptr, or the frame handle the train side of p comes from (ps_search_by_projection_frames)
  int SearchByProjectionFrame(ps_proj_problem& p, ps_frame* frame = nullptr) { ConfigureProjectionFrame(p, mfNNratio, mbCheckOrientation); return run(p, frame); }
  int SearchByProjectionPoints(ps_proj_problem& p, ps_frame* frame = nullptr) { ConfigureProjectionPoints(p, mfNNratio); return run(p, frame); }
  int SearchByProjectionObject(ps_proj_problem& p) { ConfigureProjectionObject(p, mfNNratio); return run(p); }
  // already-configured problems (possibly of different overloads / matcher settings) in one call; returns the summed match count
  int SearchByProjectionBatch(ps_proj_problem* p, int n) {
    if (n <= 0) return 0;
    if (ps_search_by_projection(h_, p, n) != PS_OK) throw std::runtime_error(ps_last_error());
    int total = 0;
    for (int i = 0; i < n; i++) total += p[i].nmatches;
    return total;
  }
  // ... with the train side of problem i taken from frames[i] where that is non-null
  int SearchByProjectionBatch(ps_proj_problem* p, ps_frame* const* frames, int n) {
    if (n <= 0) return 0;
    if (ps_search_by_projection_frames(h_, p, frames, n) != PS_OK) throw std::runtime_error(ps_last_error());
    int total = 0;
    for (int i = 0; i < n; i++) total += p[i].nmatches;
    return total;
  }
  // the search half of Fuse on caller-filled problems (include/pointslot_hip.h: ps_fuse_problem); frames as above, or nullptr
  void FuseSearch(ps_fuse_problem* p, ps_frame* const* frames, int n) {
    if (n <= 0) return;
    if ((frames ? ps_fuse_search_frames(h_, p, frames, n) : ps_fuse_search(h_, p, n)) != PS_OK) throw std::runtime_error(ps_last_error());
  }
  // LocalMapping::CreateNewMapPoints on caller-filled problems (include/pointslot_hip.h: ps_tri_problem): SearchForTriangulation
  // against every neighbour and the triangulation gates.  kf1_frames: nullptr, or per problem the frame handle keyframe 1's keys
  // and descriptors come from.  Returns the points created over all problems.
  int CreateNewMapPoints(ps_tri_problem* p, ps_frame* const* kf1_frames, int n) {
    if (n <= 0) return 0;
    if ((kf1_frames ? ps_create_new_map_points_frames(h_, p, kf1_frames, n) : ps_create_new_map_points(h_, p, n)) != PS_OK) throw std::runtime_error(ps_last_error());
    int total = 0;
    for (int i = 0; i < n; i++) total += *p[i].nnew;
    return total;
  }
  // both SearchByBoW overloads on caller-filled problems (include/pointslot_hip.h: ps_bow_search_problem; mode, nn_ratio and
  // check_orientation are the caller's, so one call may mix overloads and settings).  Returns the summed match count.
  int SearchByBoWBatch(ps_bow_search_problem* p, int n) {
    if (n <= 0) return 0;
    if (ps_search_by_bow(h_, p, n) != PS_OK) throw std::runtime_error(ps_last_error());
    int total = 0;
    for (int i = 0; i < n; i++) total += p[i].nmatches;
    return total;
  }
  // the loop-closure / relocalisation projection matchers on caller-filled problems (include/pointslot_hip.h: ps_kf_search_problem;
  // mode, th_dist and check_orientation are the caller's, so one call may mix the three members).  frames: nullptr, or per problem
  // the frame handle the searched side comes from.  Returns the summed match count.
  int KfSearchBatch(ps_kf_search_problem* p, ps_frame* const* frames, int n) {
    if (n <= 0) return 0;
    if ((frames ? ps_kf_search_frames(h_, p, frames, n) : ps_kf_search(h_, p, n)) != PS_OK) throw std::runtime_error(ps_last_error());
    int total = 0;
    for (int i = 0; i < n; i++) total += p[i].nmatches;
    return total;
  }
  // SearchBySim3 on caller-filled problems (ps_sim3_problem); frames1 / frames2: nullptr, or per problem the handles of keyframe 1 / 2
  int SearchBySim3Batch(ps_sim3_problem* p, ps_frame* const* frames1, ps_frame* const* frames2, int n) {
    if (n <= 0) return 0;
    if (((frames1 || frames2) ? ps_search_by_sim3_frames(h_, p, frames1, frames2, n) : ps_search_by_sim3(h_, p, n)) != PS_OK) throw std::runtime_error(ps_last_error());
    int total = 0;
    for (int i = 0; i < n; i++) total += p[i].nfound;
    return total;
  }
  // The decomposition of a Sim3 pose at ORBmatcher.cc:422-426 / :1271-1275 as ONE stated model (cv::MatExpr division by a scalar is
  // OpenCV-internal): the dot product of row 0 in double, scw = its root rounded to float, every entry of Rcw and tcw =
  // float(double(entry) * (1.0 / double(scw))), Ow = -Rcw^T tcw with the products and their sum in double, rounded once.
  // (pointslot_amd.matcher.decompose_scw is the same model.)
  template <class MatT> static void DecomposeScw(const MatT& Scw, float rcw[9], float tcw[3], float ow[3]) {
    double dot = 0.0;
    for (int c = 0; c < 3; c++) dot += (double)Scw.template at<float>(0, c) * (double)Scw.template at<float>(0, c);
    const float scw = (float)std::sqrt(dot);
    const double inv = 1.0 / (double)scw;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) rcw[3 * r + c] = (float)((double)Scw.template at<float>(r, c) * inv);
      tcw[r] = (float)((double)Scw.template at<float>(r, 3) * inv);
    }
    for (int r = 0; r < 3; r++) ow[r] = (float)(-((double)rcw[r] * (double)tcw[0] + (double)rcw[3 + r] * (double)tcw[1] + (double)rcw[6 + r] * (double)tcw[2]));
  }
  // sR12 = s12 * R12, sR21 = (1.0 / s12) * R12.t(), t21 = -sR21 * t12 (ORBmatcher.cc:1404-1406) as ONE stated model: every entry of
  // sR12 = float(double(R12) * double(s12)), of sR21 = float(double(R12^T) * (1.0 / double(s12))), t21 with the products and their
  // sum in double, negated, rounded once.  (pointslot_amd.matcher.sim3_pair is the same model.)
  template <class MatT> static void Sim3Pair(float s12, const MatT& R12, const MatT& t12, float sr12[9], float t12o[3], float sr21[9], float t21[3]) {
    const double s = (double)s12, inv = 1.0 / (double)s12;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) {
        sr12[3 * r + c] = (float)((double)R12.template at<float>(r, c) * s);
        sr21[3 * r + c] = (float)((double)R12.template at<float>(c, r) * inv);
      }
      t12o[r] = t12.template at<float>(r);
    }
    for (int r = 0; r < 3; r++) t21[r] = (float)(-((double)sr21[3 * r] * (double)t12o[0] + (double)sr21[3 * r + 1] * (double)t12o[1] + (double)sr21[3 * r + 2] * (double)t12o[2]));
  }
  ps_matcher* handle() { return h_; }   // (kernel time of the last call: ps_matcher_last_kernel_ms)
  static float RadiusByViewingCos(const float& viewCos) { return viewCos > 0.998 ? 2.5f : 4.0f; }   // ORBmatcher.cc:252-258

  // ------------------------------------------------------------------------------------------------------------------
  // The reference's own signatures (/root/reference/include/ORBmatcher.h:47-103) as templates over the caller's Frame /
  // MapPoint / MapObjectPoint types: any type with the reference's member names compiles (Frame.h: N, mvKeys, mvKeysUn,
  // mvuRight, mDescriptors, mvpMapPoints, mvbOutlier, mGrid, mnMinX.., mfGridElementWidthInv.., mTcw, fx.., mbf, mb,
  // mvScaleFactors, and the per-object mvObjKeys / mvObjKeysUn / mvuObjKeysRight / mvObjPointsDescriptors /
  // mvpMapObjectPoints / mvbObjKeysOutlier / mvObjKeysGrid / isInBBox).  Each does what INTEGRATION.md section 2 lists:
  // gather the fields the reference reads into a ps_proj_problem / ps_bf_problem, one C-ABI call, pointer write-back.
  // A Frame type with a member `ps_frame* mpDeviceFrame` (not in the reference; detected at compile time) that is non-null
  // has its train side on the device already: the two overloads that search into the frame's own keypoints then build no host
  // CSR and pack no train arrays - only mvpMapPoints' occupancy travels.  (The object overload searches into one object's
  // key set, which a frame handle does not hold.)
  // ------------------------------------------------------------------------------------------------------------------

  // int SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th)            ORBmatcher.cc:68-155
  template <class FrameT, class MapPointT>
  int SearchByProjection(FrameT& F, const std::vector<MapPointT*>& vpMapPoints, const float th) {
    TrainSide T;
    T.frame = deviceFrameOf(F);
    if (T.frame) fillTrainOnDevice(T, (int)F.mvKeysUn.size()); else fillTrain(T, F.mvKeysUn, F.mvuRight, F.mDescriptors, F.mGrid, F);
    for (size_t j = 0; j < F.mvpMapPoints.size(); j++) T.occupied[j] = (F.mvpMapPoints[j] && F.mvpMapPoints[j]->Observations() > 0) ? 1 : 0;
    return searchPoints(T, F, vpMapPoints, th, false, [&](int j, MapPointT* p) { F.mvpMapPoints[j] = p; });
  }

  // int SearchByProjection(Frame &F, const size_t &nOrder, const vector<MapObjectPoint*> &vpMapPoints, const float th)   :157-248
  template <class FrameT, class MapObjectPointT>
  int SearchByProjection(FrameT& F, const std::size_t& nOrder, const std::vector<MapObjectPointT*>& vpMapPoints, const float th) {
    if (F.mvDetectionObjects[nOrder] == NULL) throw std::runtime_error("SearchByProjection: no detection at nOrder");   // assert(0) in the reference
    TrainSide T;
    fillTrain(T, F.mvObjKeysUn[nOrder], F.mvuObjKeysRight[nOrder], F.mvObjPointsDescriptors[nOrder], F.mvObjKeysGrid[nOrder], F);
    T.in_bbox.assign(T.n, 0);
    for (int j = 0; j < T.n; j++) {
      T.in_bbox[j] = F.isInBBox(nOrder, F.mvObjKeysUn[nOrder][j].pt.x, F.mvObjKeysUn[nOrder][j].pt.y) ? 1 : 0;
      T.occupied[j] = (F.mvpMapObjectPoints[nOrder][j] && F.mvpMapObjectPoints[nOrder][j]->Observations() > 0) ? 1 : 0;
    }
    return searchPoints(T, F, vpMapPoints, th, true, [&](int j, MapObjectPointT* p) { F.mvpMapObjectPoints[nOrder][j] = p; });
  }

  // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)               :1613-1756
  template <class FrameT>
  int SearchByProjection(FrameT& CurrentFrame, const FrameT& LastFrame, const float th, const bool bMono) {
    TrainSide T;
    T.frame = deviceFrameOf(CurrentFrame);
    if (T.frame) fillTrainOnDevice(T, (int)CurrentFrame.mvKeysUn.size());
    else fillTrain(T, CurrentFrame.mvKeysUn, CurrentFrame.mvuRight, CurrentFrame.mDescriptors, CurrentFrame.mGrid, CurrentFrame);
    for (size_t j = 0; j < CurrentFrame.mvpMapPoints.size(); j++)
      T.occupied[j] = (CurrentFrame.mvpMapPoints[j] && CurrentFrame.mvpMapPoints[j]->Observations() > 0) ? 1 : 0;
    const int nq = LastFrame.N;
    std::vector<uint8_t> qvalid(nq, 0), qobs(nq, 0), qdesc((size_t)nq * 32, 0);
    std::vector<float> qxw((size_t)nq * 3, 0.f), qang(nq, 0.f);
    std::vector<int32_t> qoct(nq, 0);
    for (int i = 0; i < nq; i++) {
      auto* pMP = LastFrame.mvpMapPoints[i];
      qoct[i] = LastFrame.mvKeys[i].octave; qang[i] = LastFrame.mvKeysUn[i].angle;
      if (!pMP || LastFrame.mvbOutlier[i]) continue;
      qvalid[i] = 1; qobs[i] = pMP->Observations() > 0 ? 1 : 0;
      const pscv::Mat x3Dw = pMP->GetWorldPos();
      for (int c = 0; c < 3; c++) qxw[3 * (size_t)i + c] = x3Dw.template at<float>(c);
      const pscv::Mat d = pMP->GetDescriptor();
      std::memcpy(&qdesc[(size_t)i * 32], d.template ptr<uint8_t>(), 32);
    }
    ps_proj_problem p = ps_proj_problem{};
    T.bind(p.train);
    p.nq = nq; p.q_valid = qvalid.data(); p.q_desc = qdesc.data(); p.q_observed = qobs.data(); p.q_angle = qang.data();
    p.q_xw = qxw.data(); p.q_octave = qoct.data(); p.mono = bMono ? 1 : 0;
    copyPose(CurrentFrame.mTcw, p.tcw); copyPose(LastFrame.mTcw, p.tlw);
    p.fx = CurrentFrame.fx; p.fy = CurrentFrame.fy; p.cx = CurrentFrame.cx; p.cy = CurrentFrame.cy; p.mbf = CurrentFrame.mbf; p.mb = CurrentFrame.mb;
    p.bounds[0] = CurrentFrame.mnMinX; p.bounds[1] = CurrentFrame.mnMaxX; p.bounds[2] = CurrentFrame.mnMinY; p.bounds[3] = CurrentFrame.mnMaxY;
    for (int l = 0; l < 8; l++) p.scale_factors[l] = l < (int)CurrentFrame.mvScaleFactors.size() ? CurrentFrame.mvScaleFactors[l] : 1.f;
    p.th = th;
    std::vector<int32_t> match((size_t)std::max(T.n, 1), -1);
    p.match_of_train = match.data();
    const int n = SearchByProjectionFrame(p, T.frame);
    for (int j = 0; j < T.n; j++) {
      if (match[j] >= 0) CurrentFrame.mvpMapPoints[j] = LastFrame.mvpMapPoints[match[j]];
      else if (match[j] == -2) CurrentFrame.mvpMapPoints[j] = NULL;   // assigned, then reset by the rotation check (:1742-1750)
    }
    return n;
  }

  // int SearchByBruceMatching(const Frame& LastFrame, const Frame& CurrentFrame, const int &nLastOrder, const int &nCurrenOrder,
  //                           vector<MapObjectPoint *> &vpMapObjectPointMatches)                                          :2043-2155
  template <class FrameT, class MapObjectPointT>
  int SearchByBruceMatching(const FrameT& LastFrame, const FrameT& CurrentFrame, const int& nLastOrder, const int& nCurrenOrder,
                            std::vector<MapObjectPointT*>& vpMapObjectPointMatches) {
    const std::vector<MapObjectPointT*>& vpMapLast = LastFrame.mvpMapObjectPoints[nLastOrder];
    const int nq = (int)vpMapLast.size(), nt = (int)CurrentFrame.mvObjKeysUn[nCurrenOrder].size();
    vpMapObjectPointMatches.assign(CurrentFrame.mvpMapObjectPoints[nCurrenOrder].size(), static_cast<MapObjectPointT*>(NULL));
    std::vector<uint8_t> qvalid(std::max(nq, 1), 0);
    std::vector<float> qang(std::max(nq, 1), 0.f), tang(std::max(nt, 1), 0.f);
    for (int i = 0; i < nq; i++) {
      MapObjectPointT* pMP = vpMapLast[i];
      qvalid[i] = (pMP && !pMP->isBad() && !LastFrame.mvbObjKeysOutlier[nLastOrder][i]) ? 1 : 0;
      qang[i] = LastFrame.mvObjKeysUn[nLastOrder][i].angle;
    }
    for (int j = 0; j < nt; j++) tang[j] = CurrentFrame.mvObjKeys[nCurrenOrder][j].angle;
    std::vector<uint8_t> qd = rows32(LastFrame.mvObjPointsDescriptors[nLastOrder], nq), td = rows32(CurrentFrame.mvObjPointsDescriptors[nCurrenOrder], nt);
    std::vector<int32_t> qot(std::max(nt, 1), -1);
    std::vector<ps_bf_problem> pr(1);
    pr[0] = ps_bf_problem{qd.data(), qang.data(), qvalid.data(), nq, td.data(), tang.data(), nt, qot.data(), 0};
    if (nq == 0 || nt == 0) return 0;
    const int n = SearchByBruceMatching(pr);
    for (int j = 0; j < nt && j < (int)vpMapObjectPointMatches.size(); j++)
      if (qot[j] >= 0) vpMapObjectPointMatches[j] = vpMapLast[qot[j]];
    return n;
  }

  // int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs,
  //                            const bool bOnlyStereo)                                                                     :783-979
  // over a KeyFrame-shaped type (KeyFrame.h: N, mvKeys, mvKeysUn, mvuRight, mvDepth, mDescriptors, mFeatVec, GetMapPoint,
  // GetRotation, GetTranslation, GetCameraCenter, fx .. invfy, mb, mbf, mvScaleFactors, mvLevelSigma2; tests/cpp/keyframe_view.h).
  // The node of a feature comes from walking the caller's mFeatVec.  A type with a non-null `ps_frame* mpDeviceFrame` has the keys
  // and descriptors of pKF1 on the device already.
  template <class KeyFrameT, class MatT>
  int SearchForTriangulation(KeyFrameT* pKF1, KeyFrameT* pKF2, MatT F12, std::vector<std::pair<std::size_t, std::size_t>>& vMatchedPairs,
                             const bool bOnlyStereo) {
    TriSide S1, S2;
    ps_frame* frame = deviceFrameOf(*pKF1);
    ps_tri_problem p = ps_tri_problem{};
    fillTriSide(S1, *pKF1, p.kf1, frame != nullptr);
    ps_tri_keyframe k2 = ps_tri_keyframe{};
    fillTriSide(S2, *pKF2, k2, false);
    float f12[9];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) f12[3 * r + c] = F12.template at<float>(r, c);
    std::vector<int32_t> match((std::size_t)std::max(p.kf1.n, 1), -1);
    int32_t nmatches = 0, nnew = 0;
    p.k = 1; p.kf2 = &k2; p.f12 = f12;
    p.only_stereo = bOnlyStereo ? 1 : 0; p.check_orientation = mbCheckOrientation ? 1 : 0; p.triangulate = 0; p.chain = 0;
    p.match = match.data(); p.nmatches = &nmatches; p.nnew = &nnew;
    CreateNewMapPoints(&p, frame ? &frame : nullptr, 1);
    vMatchedPairs.clear();
    vMatchedPairs.reserve(nmatches);
    for (int i = 0; i < p.kf1.n; i++)
      if (match[i] >= 0) vMatchedPairs.push_back(std::make_pair((std::size_t)i, (std::size_t)match[i]));
    return nmatches;
  }

  // int SearchByBoW(KeyFrame *pKF, Frame &F, std::vector<MapPoint*> &vpMapPointMatches)                                    :280-410
  // over KeyFrame- and Frame-shaped types (KeyFrame.h: N, mvKeysUn, mDescriptors, mFeatVec, GetMapPointMatches; Frame.h: N, mvKeys,
  // mDescriptors, mFeatVec; tests/cpp/bow_view.h).  mFeatVec is what ORBVocabulary::transform filled (ComputeBoW).
  template <class KeyFrameT, class FrameT, class MapPointT, class = typename std::enable_if<!std::is_pointer<FrameT>::value>::type>
  int SearchByBoW(KeyFrameT* pKF, FrameT& F, std::vector<MapPointT*>& vpMapPointMatches) {
    const std::vector<MapPointT*> vpMapPointsKF = pKF->GetMapPointMatches();
    vpMapPointMatches.assign((std::size_t)F.N, static_cast<MapPointT*>(NULL));
    BowSide A, B;
    ps_bow_search_problem p = ps_bow_search_problem{};
    fillBowSide(A, p.a, pKF->N, pKF->mDescriptors, pKF->mvKeysUn, pKF->mFeatVec, &vpMapPointsKF);
    fillBowSide(B, p.b, F.N, F.mDescriptors, F.mvKeys, F.mFeatVec, (const std::vector<MapPointT*>*)nullptr);
    std::vector<int32_t> match((std::size_t)std::max(F.N, 1), -1);
    p.mode = 0; p.nn_ratio = mfNNratio; p.check_orientation = mbCheckOrientation ? 1 : 0; p.match = match.data();
    SearchByBoWBatch(&p, 1);
    for (int j = 0; j < F.N; j++)
      if (match[j] >= 0) vpMapPointMatches[j] = vpMapPointsKF[match[j]];
    return p.nmatches;
  }

  // int SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint*> &vpMatches12)                                   :646-781
  template <class KeyFrameT, class MapPointT>
  int SearchByBoW(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12) {
    const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    vpMatches12.assign(vpMapPoints1.size(), static_cast<MapPointT*>(NULL));
    BowSide A, B;
    ps_bow_search_problem p = ps_bow_search_problem{};
    fillBowSide(A, p.a, pKF1->N, pKF1->mDescriptors, pKF1->mvKeysUn, pKF1->mFeatVec, &vpMapPoints1);
    fillBowSide(B, p.b, pKF2->N, pKF2->mDescriptors, pKF2->mvKeysUn, pKF2->mFeatVec, &vpMapPoints2);
    std::vector<int32_t> match((std::size_t)std::max(pKF1->N, 1), -1);
    p.mode = 1; p.nn_ratio = mfNNratio; p.check_orientation = mbCheckOrientation ? 1 : 0; p.match = match.data();
    SearchByBoWBatch(&p, 1);
    for (int i = 0; i < pKF1->N && i < (int)vpMatches12.size(); i++)
      if (match[i] >= 0) vpMatches12[i] = vpMapPoints2[match[i]];
    return p.nmatches;
  }

  // ------------------------------------------------------------------------------------------------------------------
  // The loop-closure and relocalisation members, over KeyFrame- / Frame- / MapPoint-shaped types (tests/cpp/loop_view.h).
  // KeyFrame: N, mvKeysUn, mvuRight, mDescriptors, mGrid[ix][iy], mnMinX .. mnMaxY, mfGridElementWidthInv / HeightInv, fx .. cy,
  // mvScaleFactors, mfLogScaleFactor, mnScaleLevels, GetRotation, GetTranslation, GetMapPoint, GetMapPoints, GetMapPointMatches,
  // AddMapPoint.  MapPoint: isBad, GetWorldPos, GetNormal, GetDescriptor, AddObservation, GetIndexInKeyFrame and mfMinDistance /
  // mfMaxDistance (protected in the reference, and Get{Min,Max}DistanceInvariance return them scaled: PredictScale needs them as
  // they are, so a binding makes them readable).  mGrid is private in the reference's KeyFrame as well.
  // ------------------------------------------------------------------------------------------------------------------

  // int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)   :413-526
  template <class KeyFrameT, class MatT, class MapPointT>
  int SearchByProjection(KeyFrameT* pKF, MatT Scw, const std::vector<MapPointT*>& vpPoints, std::vector<MapPointT*>& vpMatched, int th) {
    TrainSide T;
    fillKfTrain(T, *pKF);
    for (int j = 0; j < T.n && j < (int)vpMatched.size(); j++) T.occupied[j] = vpMatched[j] ? 1 : 0;
    std::set<MapPointT*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
    spAlreadyFound.erase(static_cast<MapPointT*>(NULL));
    PointSide Q;
    for (MapPointT* pMP : vpPoints) Q.add(pMP, !pMP->isBad() && !spAlreadyFound.count(pMP), true, 0.f);
    ps_kf_search_problem p = ps_kf_search_problem{};
    p.mode = 0;
    DecomposeScw(Scw, p.rcw, p.tcw, p.ow);
    std::vector<int32_t> match((std::size_t)std::max(T.n, 1), -1);
    p.match_of_train = match.data(); p.th = (float)th;
    runKfSearch(p, T, Q, *pKF);
    for (int j = 0; j < T.n && j < (int)vpMatched.size(); j++)
      if (match[j] >= 0) vpMatched[j] = vpPoints[match[j]];
    return p.nmatches;
  }

  // int Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th, vector<MapPoint*> &vpReplacePoint)            :1262-1385
  // with the map surgery of :1369-1379 in candidate order
  template <class KeyFrameT, class MatT, class MapPointT>
  int Fuse(KeyFrameT* pKF, MatT Scw, const std::vector<MapPointT*>& vpPoints, float th, std::vector<MapPointT*>& vpReplacePoint) {
    TrainSide T;
    fillKfTrain(T, *pKF);
    const auto spAlreadyFound = pKF->GetMapPoints();
    PointSide Q;
    for (MapPointT* pMP : vpPoints) Q.add(pMP, !pMP->isBad() && !spAlreadyFound.count(pMP), true, 0.f);
    ps_kf_search_problem p = ps_kf_search_problem{};
    p.mode = 1;
    DecomposeScw(Scw, p.rcw, p.tcw, p.ow);
    const int nq = (int)vpPoints.size();
    std::vector<int32_t> bi((std::size_t)std::max(nq, 1), -1), bd((std::size_t)std::max(nq, 1), 256);
    p.best_idx = bi.data(); p.best_dist = bd.data(); p.th = th;
    runKfSearch(p, T, Q, *pKF);
    int nFused = 0;
    for (int iMP = 0; iMP < nq; iMP++) {
      if (bi[iMP] < 0) continue;
      MapPointT* pMP = vpPoints[iMP];
      MapPointT* pMPinKF = pKF->GetMapPoint(bi[iMP]);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF;
      } else {
        pMP->AddObservation(pKF, bi[iMP]);
        pKF->AddMapPoint(pMP, bi[iMP]);
      }
      nFused++;
    }
    return nFused;
  }

  // int SearchByProjection(Frame &CurrentFrame, KeyFrame* pKF, const set<MapPoint*> &sAlreadyFound, const float th, const int ORBdist)   :2529-2656
  // A Frame type with a non-null `ps_frame* mpDeviceFrame` is searched on the device: relocalisation runs this once per candidate keyframe.
  template <class FrameT, class KeyFrameT, class MapPointT>
  int SearchByProjection(FrameT& CurrentFrame, KeyFrameT* pKF, const std::set<MapPointT*>& sAlreadyFound, const float th, const int ORBdist) {
    TrainSide T;
    T.frame = deviceFrameOf(CurrentFrame);
    if (T.frame) fillTrainOnDevice(T, (int)CurrentFrame.mvKeysUn.size());
    else fillTrain(T, CurrentFrame.mvKeysUn, CurrentFrame.mvuRight, CurrentFrame.mDescriptors, CurrentFrame.mGrid, CurrentFrame);
    for (std::size_t j = 0; j < CurrentFrame.mvpMapPoints.size(); j++) T.occupied[j] = CurrentFrame.mvpMapPoints[j] ? 1 : 0;
    const auto vpMPs = pKF->GetMapPointMatches();
    PointSide Q;
    for (std::size_t i = 0; i < vpMPs.size(); i++) {
      auto* pMP = vpMPs[i];
      Q.add(pMP, pMP && !pMP->isBad() && !sAlreadyFound.count(pMP), false, pKF->mvKeysUn[i].angle);
    }
    ps_kf_search_problem p = ps_kf_search_problem{};
    p.mode = 2; p.th_dist = ORBdist; p.check_orientation = mbCheckOrientation ? 1 : 0;
    // Rcw, tcw of mTcw and Ow = -Rcw^T tcw (:2533-2535: a transposed operand, products and sum in double)
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) p.rcw[3 * r + c] = CurrentFrame.mTcw.template at<float>(r, c);
      p.tcw[r] = CurrentFrame.mTcw.template at<float>(r, 3);
    }
    for (int r = 0; r < 3; r++)
      p.ow[r] = (float)(-((double)p.rcw[r] * (double)p.tcw[0] + (double)p.rcw[3 + r] * (double)p.tcw[1] + (double)p.rcw[6 + r] * (double)p.tcw[2]));
    std::vector<int32_t> match((std::size_t)std::max(T.n, 1), -1);
    p.match_of_train = match.data(); p.th = th;
    runKfSearch(p, T, Q, CurrentFrame);
    for (int j = 0; j < T.n; j++) {
      if (match[j] >= 0) CurrentFrame.mvpMapPoints[j] = vpMPs[match[j]];
      else if (match[j] == -2) CurrentFrame.mvpMapPoints[j] = NULL;   // assigned, then reset by the rotation check (:2642-2652)
    }
    return p.nmatches;
  }

  // int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12,
  //                  const cv::Mat &t12, const float th)                                                                   :1387-1611
  template <class KeyFrameT, class MapPointT, class MatT>
  int SearchBySim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12, const float& s12, const MatT& R12, const MatT& t12, const float th) {
    const auto vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    const int N1 = (int)vpMapPoints1.size(), N2 = (int)vpMapPoints2.size();
    TrainSide T1, T2;
    fillKfTrain(T1, *pKF1); fillKfTrain(T2, *pKF2);
    PointSide Q1, Q2;
    for (auto* pMP : vpMapPoints1) Q1.add(pMP, pMP && !pMP->isBad(), false, 0.f);
    for (auto* pMP : vpMapPoints2) Q2.add(pMP, pMP && !pMP->isBad(), false, 0.f);
    std::vector<uint8_t> already1((std::size_t)std::max(N1, 1), 0), already2((std::size_t)std::max(N2, 1), 0);
    for (int i = 0; i < N1; i++) {
      MapPointT* pMP = vpMatches12[i];
      if (!pMP) continue;
      already1[i] = 1;
      const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
      if (idx2 >= 0 && idx2 < N2) already2[idx2] = 1;
    }
    ps_sim3_problem p = ps_sim3_problem{};
    fillSim3Side(p.kf1, T1, Q1, already1, *pKF1);
    fillSim3Side(p.kf2, T2, Q2, already2, *pKF2);
    p.fx = pKF1->fx; p.fy = pKF1->fy; p.cx = pKF1->cx; p.cy = pKF1->cy;     // keyframe 1's, for both directions (:1390-1393)
    Sim3Pair(s12, R12, t12, p.sr12, p.t12, p.sr21, p.t21);
    p.th = th;
    std::vector<int32_t> m12((std::size_t)std::max(N1, 1), -1);
    p.match12 = m12.data();
    ps_frame* f1 = deviceFrameOf(*pKF1);
    ps_frame* f2 = deviceFrameOf(*pKF2);
    SearchBySim3Batch(&p, f1 ? &f1 : nullptr, f2 ? &f2 : nullptr, 1);
    for (int i1 = 0; i1 < N1; i1++)
      if (m12[i1] >= 0) vpMatches12[i1] = vpMapPoints2[m12[i1]];
    return p.nfound;
  }

 protected:
  // one side of SearchByBoW as ps_bow_side's arrays; points == nullptr: the Frame side of the first overload
  struct BowSide {
    std::vector<float> angle;
    std::vector<int32_t> node;
    std::vector<uint8_t> desc, has_point;
  };
  template <class KeysT, class FeatVecT, class MapPointT>
  static void fillBowSide(BowSide& S, ps_bow_side& s, int n, const pscv::Mat& descriptors, const KeysT& keys, const FeatVecT& featVec,
                          const std::vector<MapPointT*>* points) {
    const int m = std::max(n, 1);
    S.angle.assign(m, 0.f); S.node.assign(m, -1); S.has_point.assign(m, 0);
    for (int i = 0; i < n; i++) {
      S.angle[i] = keys[i].angle;
      if (points && (std::size_t)i < points->size()) S.has_point[i] = ((*points)[i] && !(*points)[i]->isBad()) ? 1 : 0;
    }
    for (const auto& nodeAndFeatures : featVec)
      for (const auto i : nodeAndFeatures.second)
        if ((std::size_t)i < (std::size_t)n) S.node[i] = (int32_t)nodeAndFeatures.first;
    S.desc = rows32(descriptors, n);
    s.n = n; s.desc = S.desc.data(); s.angle = S.angle.data(); s.node = S.node.data(); s.has_point = points ? S.has_point.data() : nullptr;
  }
  // one KeyFrame as ps_tri_keyframe's arrays
  struct TriSide {
    std::vector<float> x, y, xr, yr, angle, ur, depth;
    std::vector<int32_t> octave, node;
    std::vector<uint8_t> desc, occupied;
  };
  template <class KeyFrameT>
  static void fillTriSide(TriSide& S, KeyFrameT& KF, ps_tri_keyframe& k, bool on_device) {
    const int n = KF.N, m = std::max(n, 1);
    S.x.resize(m); S.y.resize(m); S.xr.resize(m); S.yr.resize(m); S.angle.resize(m); S.ur.resize(m); S.depth.resize(m); S.octave.resize(m);
    S.node.assign(m, -1); S.occupied.assign(m, 0);
    for (int i = 0; i < n; i++) {
      S.x[i] = KF.mvKeysUn[i].pt.x; S.y[i] = KF.mvKeysUn[i].pt.y; S.octave[i] = KF.mvKeysUn[i].octave; S.angle[i] = KF.mvKeysUn[i].angle;
      S.xr[i] = KF.mvKeys[i].pt.x; S.yr[i] = KF.mvKeys[i].pt.y; S.ur[i] = KF.mvuRight[i]; S.depth[i] = KF.mvDepth[i];
      S.occupied[i] = KF.GetMapPoint(i) ? 1 : 0;
    }
    for (const auto& nodeAndFeatures : KF.mFeatVec)
      for (const auto i : nodeAndFeatures.second)
        if ((std::size_t)i < (std::size_t)n) S.node[i] = (int32_t)nodeAndFeatures.first;
    S.desc = rows32(KF.mDescriptors, n);
    k.n = n;
    if (!on_device) { k.x = S.x.data(); k.y = S.y.data(); k.octave = S.octave.data(); k.angle = S.angle.data(); k.u_right = S.ur.data(); k.desc = S.desc.data(); }
    k.x_raw = S.xr.data(); k.y_raw = S.yr.data(); k.depth = S.depth.data(); k.node = S.node.data(); k.occupied = S.occupied.data();
    const auto R = KF.GetRotation(), t = KF.GetTranslation(), O = KF.GetCameraCenter();
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) k.rcw[3 * r + c] = R.template at<float>(r, c);
      k.tcw[r] = t.template at<float>(r); k.ow[r] = O.template at<float>(r);
    }
    k.fx = KF.fx; k.fy = KF.fy; k.cx = KF.cx; k.cy = KF.cy; k.invfx = KF.invfx; k.invfy = KF.invfy; k.mb = KF.mb; k.mbf = KF.mbf;
    for (int l = 0; l < 8; l++) {
      k.scale_factors[l] = l < (int)KF.mvScaleFactors.size() ? KF.mvScaleFactors[l] : 1.f;
      k.level_sigma2[l] = l < (int)KF.mvLevelSigma2.size() ? KF.mvLevelSigma2[l] : 1.f;
    }
  }
  // the "train" half of a windowed search: mvKeysUn-like keys, mvuRight, descriptors and the 64 x 48 grid of the frame (or of
  // one of its objects) as the arrays of ps_proj_train
  struct TrainSide {
    int n = 0;
    std::vector<float> x, y, angle, ur;
    std::vector<int32_t> octave, cell_off, cell_idx;
    std::vector<uint8_t> desc, occupied, in_bbox;
    float min_x = 0, min_y = 0, gw = 0, gh = 0;
    ps_frame* frame = nullptr;   // non-null: everything but occupied / in_bbox is in this handle, the vectors above stay empty
    void bind(ps_proj_train& t) const {
      t.n = n; t.x = x.data(); t.y = y.data(); t.octave = octave.data(); t.angle = angle.data(); t.u_right = ur.data(); t.desc = desc.data();
      t.occupied = occupied.data(); t.in_bbox = in_bbox.empty() ? nullptr : in_bbox.data(); t.cell_off = cell_off.data(); t.cell_idx = cell_idx.data();
      t.min_x = min_x; t.min_y = min_y; t.grid_w_inv = gw; t.grid_h_inv = gh;
    }
  };
  static std::vector<uint8_t> rows32(const pscv::Mat& m, int n) {
    std::vector<uint8_t> out((size_t)std::max(n, 1) * 32, 0);
    for (int i = 0; i < n && i < m.rows; i++) std::memcpy(&out[(size_t)i * 32], m.ptr<uint8_t>(i), 32);
    return out;
  }
  template <class MatT> static void copyPose(const MatT& Tcw, float* out16) {
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) out16[4 * r + c] = Tcw.template at<float>(r, c);
  }
  // ps_frame* mpDeviceFrame of the caller's Frame type, nullptr for a type without the member
  template <class T, class = void> struct HasDeviceFrame : std::false_type {};
  template <class T> struct HasDeviceFrame<T, std::void_t<decltype(std::declval<const T&>().mpDeviceFrame)>> : std::true_type {};
  template <class FrameT> static ps_frame* deviceFrameOf(const FrameT& F) {
    if constexpr (HasDeviceFrame<FrameT>::value) return F.mpDeviceFrame; else return nullptr;
  }
  static void fillTrainOnDevice(TrainSide& T, int n) { T.n = n; T.occupied.assign(std::max(n, 1), 0); }
  template <class KeysT, class GridT, class FrameT>
  static void fillTrain(TrainSide& T, const KeysT& keysUn, const std::vector<float>& uRight, const pscv::Mat& descriptors, const GridT& grid, const FrameT& F) {
    const int n = (int)keysUn.size();
    T.n = n;
    T.x.resize(std::max(n, 1)); T.y.resize(std::max(n, 1)); T.angle.resize(std::max(n, 1)); T.ur.resize(std::max(n, 1)); T.octave.resize(std::max(n, 1));
    T.occupied.assign(std::max(n, 1), 0);
    for (int j = 0; j < n; j++) {
      T.x[j] = keysUn[j].pt.x; T.y[j] = keysUn[j].pt.y; T.angle[j] = keysUn[j].angle; T.octave[j] = keysUn[j].octave; T.ur[j] = uRight[j];
    }
    T.desc = rows32(descriptors, n);
    const int GC = 64, GR = 48;   // FRAME_GRID_COLS / FRAME_GRID_ROWS (Frame.h:40-41)
    T.cell_off.assign(GC * GR + 1, 0);
    T.cell_idx.clear();
    for (int ix = 0; ix < GC; ix++)
      for (int iy = 0; iy < GR; iy++) {
        T.cell_off[ix * GR + iy] = (int32_t)T.cell_idx.size();
        for (std::size_t k : grid[ix][iy]) T.cell_idx.push_back((int32_t)k);
      }
    T.cell_off[GC * GR] = (int32_t)T.cell_idx.size();
    T.cell_idx.resize(std::max<size_t>(T.cell_idx.size(), (size_t)std::max(n, 1)), 0);
    T.min_x = F.mnMinX; T.min_y = F.mnMinY; T.gw = F.mfGridElementWidthInv; T.gh = F.mfGridElementHeightInv;
  }
  // the two map-point overloads share everything but the window (r * scale[level] and levels [l-1, l] for map points; 5 px and
  // [l-1, l+1] for object points, ORBmatcher.cc:92-93 / :182) and the threshold
  template <class FrameT, class PointT, class Assign>
  int searchPoints(TrainSide& T, const FrameT& F, const std::vector<PointT*>& pts, const float th, bool object, Assign assign) {
    const int nq = (int)pts.size();
    std::vector<uint8_t> qvalid(std::max(nq, 1), 0), qobs(std::max(nq, 1), 0), qdesc((size_t)std::max(nq, 1) * 32, 0);
    std::vector<float> qu(std::max(nq, 1), 0.f), qv(std::max(nq, 1), 0.f), qur(std::max(nq, 1), 0.f), rad(std::max(nq, 1), 0.f), rer(std::max(nq, 1), 0.f);
    std::vector<int32_t> minl(std::max(nq, 1), 0), maxl(std::max(nq, 1), 0);
    const bool bFactor = th != 1.0;
    for (int i = 0; i < nq; i++) {
      PointT* pMP = pts[i];
      if (!pMP->mbTrackInView || pMP->isBad()) continue;
      const int nPredictedLevel = pMP->mnTrackScaleLevel;
      float r = RadiusByViewingCos(pMP->mTrackViewCos);
      if (bFactor) r *= th;
      qvalid[i] = 1; qobs[i] = pMP->Observations() > 0 ? 1 : 0;
      qu[i] = pMP->mTrackProjX; qv[i] = pMP->mTrackProjY; qur[i] = pMP->mTrackProjXR;
      rer[i] = r * F.mvScaleFactors[nPredictedLevel];
      rad[i] = object ? (float)RADIUS_FORDYNAMIC : rer[i];
      minl[i] = nPredictedLevel - 1; maxl[i] = object ? nPredictedLevel + 1 : nPredictedLevel;
      const pscv::Mat d = pMP->GetDescriptor();
      std::memcpy(&qdesc[(size_t)i * 32], d.template ptr<uint8_t>(), 32);
    }
    ps_proj_problem p = ps_proj_problem{};
    T.bind(p.train);
    p.nq = nq; p.q_valid = qvalid.data(); p.q_desc = qdesc.data(); p.q_observed = qobs.data();
    p.q_u = qu.data(); p.q_v = qv.data(); p.q_ur = qur.data(); p.q_radius = rad.data(); p.q_radius_er = rer.data();
    p.q_min_level = minl.data(); p.q_max_level = maxl.data();
    for (int l = 0; l < 8; l++) p.scale_factors[l] = l < (int)F.mvScaleFactors.size() ? F.mvScaleFactors[l] : 1.f;
    p.th = th;
    std::vector<int32_t> match((size_t)std::max(T.n, 1), -1);
    p.match_of_train = match.data();
    if (nq == 0) return 0;
    const int n = object ? SearchByProjectionObject(p) : SearchByProjectionPoints(p, T.frame);
    for (int j = 0; j < T.n; j++)
      if (match[j] >= 0) assign(j, pts[match[j]]);
    return n;
  }

  // the projected points of a ps_kf_search problem / the per-slot map points of a ps_sim3_side
  struct PointSide {
    std::vector<uint8_t> valid, desc;
    std::vector<float> pos, normal, mind, maxd, angle;
    template <class MapPointT> void add(MapPointT* pMP, bool ok, bool withNormal, float ang) {
      const std::size_t i = valid.size();
      valid.push_back(ok ? 1 : 0); angle.push_back(ang);
      desc.resize((i + 1) * 32, 0); pos.resize((i + 1) * 3, 0.f); normal.resize((i + 1) * 3, 0.f);
      mind.push_back(0.f); maxd.push_back(1.f);
      if (!ok) return;
      const pscv::Mat X = pMP->GetWorldPos();
      for (int c = 0; c < 3; c++) pos[3 * i + c] = X.template at<float>(c);
      if (withNormal) {
        const pscv::Mat Pn = pMP->GetNormal();
        for (int c = 0; c < 3; c++) normal[3 * i + c] = Pn.template at<float>(c);
      }
      mind[i] = pMP->mfMinDistance; maxd[i] = pMP->mfMaxDistance;
      const pscv::Mat d = pMP->GetDescriptor();
      std::memcpy(&desc[i * 32], d.template ptr<uint8_t>(), 32);
    }
    void pad() {   // (never hand out a null data() for an empty side)
      if (valid.empty()) { valid.assign(1, 0); desc.assign(32, 0); pos.assign(3, 0.f); normal.assign(3, 0.f); mind.assign(1, 0.f); maxd.assign(1, 1.f); angle.assign(1, 0.f); }
    }
  };
  // a keyframe as the searched side: on the device already (mpDeviceFrame) or packed from mvKeysUn / mDescriptors / mGrid
  template <class KeyFrameT> static void fillKfTrain(TrainSide& T, KeyFrameT& KF) {
    T.frame = deviceFrameOf(KF);
    if (T.frame) fillTrainOnDevice(T, (int)KF.mvKeysUn.size()); else fillTrain(T, KF.mvKeysUn, KF.mvuRight, KF.mDescriptors, KF.mGrid, KF);
  }
  template <class ViewT> static void fillView(const ViewT& V, float bounds[4], float scale[8], float& logScale, int32_t& nLevels) {
    bounds[0] = (float)V.mnMinX; bounds[1] = (float)V.mnMaxX; bounds[2] = (float)V.mnMinY; bounds[3] = (float)V.mnMaxY;
    for (int l = 0; l < 8; l++) scale[l] = l < (int)V.mvScaleFactors.size() ? V.mvScaleFactors[l] : 1.f;
    logScale = V.mfLogScaleFactor; nLevels = V.mnScaleLevels;
  }
  // V: the KeyFrame / Frame being searched into (intrinsics, bounds, scale tables)
  template <class ViewT> void runKfSearch(ps_kf_search_problem& p, TrainSide& T, PointSide& Q, const ViewT& V) {
    T.bind(p.train);
    p.nq = (int)Q.valid.size();
    Q.pad();
    p.q_valid = Q.valid.data(); p.q_pos = Q.pos.data(); p.q_normal = Q.normal.data(); p.q_min_dist = Q.mind.data(); p.q_max_dist = Q.maxd.data();
    p.q_desc = Q.desc.data(); p.q_angle = Q.angle.data();
    p.fx = V.fx; p.fy = V.fy; p.cx = V.cx; p.cy = V.cy;
    fillView(V, p.bounds, p.scale_factors, p.log_scale_factor, p.n_levels);
    ps_frame* frame = T.frame;
    KfSearchBatch(&p, frame ? &frame : nullptr, 1);
  }
  template <class KeyFrameT> static void fillSim3Side(ps_sim3_side& s, TrainSide& T, PointSide& Q, std::vector<uint8_t>& already, KeyFrameT& KF) {
    T.bind(s.train);
    Q.pad();
    s.has_point = Q.valid.data(); s.pos = Q.pos.data(); s.min_dist = Q.mind.data(); s.max_dist = Q.maxd.data(); s.point_desc = Q.desc.data();
    s.already = already.data();
    const auto R = KF.GetRotation(), t = KF.GetTranslation();
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) s.rcw[3 * r + c] = R.template at<float>(r, c);
      s.tcw[r] = t.template at<float>(r);
    }
    fillView(KF, s.bounds, s.scale_factors, s.log_scale_factor, s.n_levels);
  }

  int run(ps_proj_problem& p, ps_frame* frame = nullptr) {
    if ((frame ? ps_search_by_projection_frames(h_, &p, &frame, 1) : ps_search_by_projection(h_, &p, 1)) != PS_OK) throw std::runtime_error(ps_last_error());
    return p.nmatches;
  }
  ps_matcher* h_ = nullptr;
  float mfNNratio;
  bool mbCheckOrientation;
};

}  // namespace ORB_SLAM2
