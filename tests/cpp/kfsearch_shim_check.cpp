// The loop-closure and relocalisation members of the host shim (pointslot_amd/host/ORBmatcher.h) - SearchByProjection(pKF, Scw, ..),
// Fuse(pKF, Scw, ..), SearchByProjection(CurrentFrame, pKF, ..) and SearchBySim3 - instantiated on the view types of
// tests/cpp/loop_view.h: every reference-signature template must leave the pointers the struct-level call (ps_kf_search /
// ps_search_by_sim3 on problems packed here by hand) says it should, the relocalisation one also with the frame taken from a
// frame handle (`ps_frame* mpDeviceFrame`).  Prints one line per check and a final JSON summary; exit code 0 iff every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>
#include "loop_view.h"
#include "ORBmatcher.h"

using namespace ORB_SLAM2;

namespace {
struct DevLoopFrame : LoopFrame { ps_frame* mpDeviceFrame = nullptr; };

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
  double uni(double a, double b) { return a + (b - a) * uni(); }
  int below(int n) { return (int)(uni() * n); }
  double normal() { return std::sqrt(-2 * std::log(1 - uni())) * std::cos(6.283185307179586 * uni()); }
};
const float FX = 721.5377f, FY = 721.5377f, CX = 609.5593f, CY = 172.854f;
const int W = 1241, H = 376, NPTS = 320;
int g_fail = 0, g_checks = 0;
void check(bool ok, const char* what, const char* detail = "") {
  g_checks++;
  if (!ok) g_fail++;
  std::printf("%s %s %s\n", ok ? "ok  " : "FAIL", what, detail);
}

struct World { std::vector<float> X; std::vector<std::vector<uint8_t>> desc; std::vector<int> oct; std::vector<float> ang; };

std::vector<uint8_t> noisy(const std::vector<uint8_t>& d0, Rng& rng, int flips) {
  std::vector<uint8_t> d = d0;
  for (int f = rng.below(flips + 1); f > 0; f--) d[rng.below(32)] ^= (uint8_t)(1u << rng.below(8));
  return d;
}

// a camera at O looking along +z with a small yaw: the world points it sees become its features, in an order of its own;
// seen[i] = the world point behind feature i
template <class ViewT>
void seeWorld(ViewT& K, const World& Wd, Rng& rng, double yaw, const float O[3], float R[9], float t[3], std::vector<int>& seen) {
  K.fx = FX; K.fy = FY; K.cx = CX; K.cy = CY;
  K.mnMinX = 0; K.mnMinY = 0; K.mnMaxX = W; K.mnMaxY = H;
  K.mfGridElementWidthInv = 64.f / W; K.mfGridElementHeightInv = 48.f / H;
  K.mvScaleFactors.assign(8, 1.f);
  for (int l = 1; l < 8; l++) K.mvScaleFactors[l] = (float)(K.mvScaleFactors[l - 1] * 1.2);
  K.mfLogScaleFactor = std::log(1.2f); K.mnScaleLevels = 8;
  const float c = (float)std::cos(yaw), s = (float)std::sin(yaw);
  const float Rv[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
  for (int r = 0; r < 3; r++) {
    for (int q = 0; q < 3; q++) R[3 * r + q] = Rv[3 * r + q];
    t[r] = -(Rv[3 * r] * O[0] + Rv[3 * r + 1] * O[1] + Rv[3 * r + 2] * O[2]);
  }
  std::vector<int> order(NPTS);
  for (int i = 0; i < NPTS; i++) order[i] = i;
  for (int i = NPTS - 1; i > 0; i--) std::swap(order[i], order[rng.below(i + 1)]);
  std::vector<std::vector<uint8_t>> rows;
  for (int p : order) {
    const float* X = &Wd.X[3 * p];
    float pc[3];
    for (int r = 0; r < 3; r++) pc[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
    if (pc[2] < 1.f) continue;
    const float u = FX * pc[0] / pc[2] + CX + (float)(0.5 * rng.normal()), v = FY * pc[1] / pc[2] + CY + (float)(0.5 * rng.normal());
    if (u < 5 || u > W - 25 || v < 5 || v > H - 5) continue;
    cv::KeyPoint k; k.pt.x = u; k.pt.y = v; k.octave = Wd.oct[p]; k.angle = std::fmod(Wd.ang[p] + (float)(3.0 * rng.normal()) + 360.f, 360.f);
    K.mvKeysUn.push_back(k); K.mvuRight.push_back(-1.f);
    rows.push_back(noisy(Wd.desc[p], rng, 12));
    seen.push_back(p);
  }
  K.N = (int)K.mvKeysUn.size();
  K.mDescriptors.create(K.N, 32, cv::CV_8U);
  for (int i = 0; i < K.N; i++) std::memcpy(K.mDescriptors.template ptr<uint8_t>(i), rows[i].data(), 32);
  K.AssignFeaturesToGrid();
}

void makeKeyFrame(LoopKeyFrame& K, const World& Wd, Rng& rng, double yaw, float ox, float oz, std::vector<int>& seen) {
  const float O[3] = {ox, 0.f, oz};
  float R[9], t[3];
  seeWorld(K, Wd, rng, yaw, O, R, t, seen);
  for (int r = 0; r < 3; r++) {
    for (int q = 0; q < 3; q++) K.Rcw.at<float>(r, q) = R[3 * r + q];
    K.tcw.at<float>(r) = t[r];
  }
  K.mvpMapPoints.assign(K.N, nullptr);
}

// the searched side and the points packed by hand, independently of the shim's own marshalling
struct PackedTrain {
  std::vector<float> x, y, ang; std::vector<int32_t> oct, coff, cidx; std::vector<uint8_t> desc, occ;
  ps_proj_train t;
  template <class ViewT> explicit PackedTrain(ViewT& K) {
    for (int i = 0; i < K.N; i++) {
      x.push_back(K.mvKeysUn[i].pt.x); y.push_back(K.mvKeysUn[i].pt.y); ang.push_back(K.mvKeysUn[i].angle); oct.push_back(K.mvKeysUn[i].octave);
      desc.insert(desc.end(), K.mDescriptors.template ptr<uint8_t>(i), K.mDescriptors.template ptr<uint8_t>(i) + 32);
    }
    occ.assign(K.N, 0);
    for (int ix = 0; ix < 64; ix++)
      for (int iy = 0; iy < 48; iy++) {
        coff.push_back((int32_t)cidx.size());
        for (std::size_t k : K.mGrid[ix][iy]) cidx.push_back((int32_t)k);
      }
    coff.push_back((int32_t)cidx.size());
    cidx.resize(K.N + 1, 0);
    t = ps_proj_train{};
    t.n = K.N; t.x = x.data(); t.y = y.data(); t.octave = oct.data(); t.angle = ang.data(); t.desc = desc.data(); t.occupied = occ.data();
    t.cell_off = coff.data(); t.cell_idx = cidx.data();
    t.min_x = (float)K.mnMinX; t.min_y = (float)K.mnMinY; t.grid_w_inv = K.mfGridElementWidthInv; t.grid_h_inv = K.mfGridElementHeightInv;
  }
};
struct PackedPoints {
  std::vector<uint8_t> valid, desc; std::vector<float> pos, nor, mind, maxd, ang;
  void add(LoopMapPoint* p, bool ok, float angle) {
    valid.push_back(ok); ang.push_back(angle);
    for (int c = 0; c < 3; c++) { pos.push_back(ok ? p->mWorldPos.at<float>(c) : 0.f); nor.push_back(ok ? p->mNormalVector.at<float>(c) : 0.f); }
    mind.push_back(ok ? p->mfMinDistance : 0.f); maxd.push_back(ok ? p->mfMaxDistance : 1.f);
    for (int b = 0; b < 32; b++) desc.push_back(ok ? p->mDescriptor.ptr<uint8_t>()[b] : 0);
  }
};
template <class ViewT> void view(ps_kf_search_problem& p, ViewT& V) {
  p.fx = V.fx; p.fy = V.fy; p.cx = V.cx; p.cy = V.cy;
  p.bounds[0] = (float)V.mnMinX; p.bounds[1] = (float)V.mnMaxX; p.bounds[2] = (float)V.mnMinY; p.bounds[3] = (float)V.mnMaxY;
  for (int l = 0; l < 8; l++) p.scale_factors[l] = V.mvScaleFactors[l];
  p.log_scale_factor = V.mfLogScaleFactor; p.n_levels = V.mnScaleLevels;
}
void points(ps_kf_search_problem& p, PackedPoints& Q) {
  p.nq = (int)Q.valid.size(); p.q_valid = Q.valid.data(); p.q_pos = Q.pos.data(); p.q_normal = Q.nor.data(); p.q_min_dist = Q.mind.data();
  p.q_max_dist = Q.maxd.data(); p.q_desc = Q.desc.data(); p.q_angle = Q.ang.data();
}
cv::Mat sim3Matrix(LoopKeyFrame& K, float s) {
  cv::Mat S(4, 4, cv::CV_32F);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) S.at<float>(r, c) = s * K.Rcw.at<float>(r, c);
    S.at<float>(r, 3) = s * K.tcw.at<float>(r);
    S.at<float>(3, r) = 0.f;
  }
  S.at<float>(3, 3) = 1.f;
  return S;
}
}  // namespace

int main() {
  Rng rng(0x51A3);
  World Wd;
  for (int p = 0; p < NPTS; p++) {
    const double z = rng.uni(5, 40);
    Wd.X.push_back((float)(rng.uni(-0.5, 0.5) * z)); Wd.X.push_back((float)(rng.uni(-0.18, 0.18) * z)); Wd.X.push_back((float)z);
    std::vector<uint8_t> d(32);
    for (auto& b : d) b = (uint8_t)rng.below(256);
    Wd.desc.push_back(d); Wd.oct.push_back(rng.below(6)); Wd.ang.push_back((float)rng.uni(0, 360));
  }
  // one map point per world point; its scale-invariance region puts the predicted level at the features' octave
  std::vector<LoopMapPoint*> mp(NPTS);
  for (int p = 0; p < NPTS; p++) {
    LoopMapPoint* m = mp[p] = new LoopMapPoint();
    const float* X = &Wd.X[3 * p];
    const float d = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    for (int c = 0; c < 3; c++) { m->mWorldPos.at<float>(c) = X[c]; m->mNormalVector.at<float>(c) = X[c] / d; }
    m->mfMaxDistance = d * (float)std::pow(1.2, Wd.oct[p] - 0.5); m->mfMinDistance = m->mfMaxDistance / (float)std::pow(1.2, 7);
    const std::vector<uint8_t> dd = noisy(Wd.desc[p], rng, 20);
    std::memcpy(m->mDescriptor.ptr<uint8_t>(), dd.data(), 32);
    m->bad = rng.uni() < 0.03;
  }
  ORBmatcher matcher(0.6f, true);
  char detail[160];

  // ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) ----
  {
    LoopKeyFrame A; std::vector<int> seen;
    makeKeyFrame(A, Wd, rng, 0.01, 0.1f, -0.5f, seen);
    std::vector<LoopMapPoint*> vpPoints(mp.begin(), mp.end()), vpMatched(A.N, nullptr);
    for (int j = 0; j < A.N; j++) if (rng.uni() < 0.15) vpMatched[j] = mp[seen[j]];
    const cv::Mat Scw = sim3Matrix(A, 0.93f);
    PackedTrain T(A); PackedPoints Q;
    std::set<LoopMapPoint*> found(vpMatched.begin(), vpMatched.end());
    for (int j = 0; j < A.N; j++) T.occ[j] = vpMatched[j] ? 1 : 0;
    for (LoopMapPoint* p : vpPoints) Q.add(p, !p->isBad() && !found.count(p), 0.f);
    ps_kf_search_problem pr = ps_kf_search_problem{};
    pr.train = T.t; pr.mode = 0; points(pr, Q); view(pr, A);
    ORBmatcher::DecomposeScw(Scw, pr.rcw, pr.tcw, pr.ow);
    pr.th = 10.f;
    std::vector<int32_t> match(A.N, -1);
    pr.match_of_train = match.data();
    matcher.KfSearchBatch(&pr, nullptr, 1);
    std::vector<LoopMapPoint*> want = vpMatched;
    for (int j = 0; j < A.N; j++) if (match[j] >= 0) want[j] = vpPoints[match[j]];
    const int n = matcher.SearchByProjection(&A, Scw, vpPoints, vpMatched, 10);
    std::snprintf(detail, sizeof detail, "(%d matches, %d features, %d points)", n, A.N, NPTS);
    check(n == pr.nmatches && vpMatched == want && n >= 10, "SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) equals the struct-level call", detail);
  }
  // ---- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) ----
  {
    LoopKeyFrame A; std::vector<int> seen;
    makeKeyFrame(A, Wd, rng, -0.01, -0.2f, 0.3f, seen);
    for (int j = 0; j < A.N; j++) if (rng.uni() < 0.3) { A.mvpMapPoints[j] = new LoopMapPoint(); A.mvpMapPoints[j]->bad = rng.uni() < 0.2; }
    for (int j = 0; j < A.N; j++) if (rng.uni() < 0.05) A.mvpMapPoints[j] = mp[seen[j]];          // already in the keyframe
    std::vector<LoopMapPoint*> vpPoints(mp.begin(), mp.end()), vpReplace(NPTS, nullptr);
    const cv::Mat Scw = sim3Matrix(A, 1.07f);
    PackedTrain T(A); PackedPoints Q;
    const std::set<LoopMapPoint*> found = A.GetMapPoints();
    for (LoopMapPoint* p : vpPoints) Q.add(p, !p->isBad() && !found.count(p), 0.f);
    ps_kf_search_problem pr = ps_kf_search_problem{};
    pr.train = T.t; pr.mode = 1; points(pr, Q); view(pr, A);
    ORBmatcher::DecomposeScw(Scw, pr.rcw, pr.tcw, pr.ow);
    pr.th = 4.f;
    std::vector<int32_t> bi(NPTS, -1), bd(NPTS, 256);
    pr.best_idx = bi.data(); pr.best_dist = bd.data();
    matcher.KfSearchBatch(&pr, nullptr, 1);
    // the map surgery replayed on a copy of the slots, in candidate order
    std::vector<LoopMapPoint*> slots = A.mvpMapPoints, wantReplace(NPTS, nullptr);
    int wantFused = 0, added = 0;
    for (int i = 0; i < NPTS; i++) {
      if (bi[i] < 0) continue;
      if (slots[bi[i]]) { if (!slots[bi[i]]->isBad()) wantReplace[i] = slots[bi[i]]; }
      else { slots[bi[i]] = vpPoints[i]; added++; }
      wantFused++;
    }
    const int n = matcher.Fuse(&A, Scw, vpPoints, 4.f, vpReplace);
    bool obs = true;
    for (int j = 0; j < A.N; j++) if (A.mvpMapPoints[j] && A.mvpMapPoints[j]->mObservations.count(&A)) obs = obs && A.mvpMapPoints[j]->GetIndexInKeyFrame(&A) == j;
    std::snprintf(detail, sizeof detail, "(%d fused: %d added, %d to replace)", n, added, wantFused - added);
    check(n == wantFused && n == pr.nmatches && vpReplace == wantReplace && A.mvpMapPoints == slots && obs && added >= 5 && wantFused - added >= 3,
          "Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) equals the struct-level call plus the map surgery in candidate order", detail);
  }
  // ---- SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) ----
  {
    LoopKeyFrame A; std::vector<int> seenA;
    makeKeyFrame(A, Wd, rng, 0.0, 0.0f, 0.0f, seenA);
    for (int i = 0; i < A.N; i++) if (rng.uni() < 0.8) A.mvpMapPoints[i] = mp[seenA[i]];
    DevLoopFrame F0; std::vector<int> seenF;
    const float O[3] = {0.25f, 0.f, 0.6f};
    float R[9], t[3];
    seeWorld(F0, Wd, rng, 0.015, O, R, t, seenF);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) F0.mTcw.at<float>(r, c) = r < 3 ? (c < 3 ? R[3 * r + c] : t[r]) : (c == 3 ? 1.f : 0.f);
    F0.mvpMapPoints.assign(F0.N, nullptr);
    for (int j = 0; j < F0.N; j++) if (rng.uni() < 0.1) F0.mvpMapPoints[j] = new LoopMapPoint();
    std::set<LoopMapPoint*> sAlreadyFound;
    for (int i = 0; i < A.N; i++) if (A.mvpMapPoints[i] && rng.uni() < 0.1) sAlreadyFound.insert(A.mvpMapPoints[i]);
    for (int ORBdist : {100, 64}) {
      DevLoopFrame F = F0;
      PackedTrain T(F); PackedPoints Q;
      for (int j = 0; j < F.N; j++) T.occ[j] = F.mvpMapPoints[j] ? 1 : 0;
      for (int i = 0; i < A.N; i++) { LoopMapPoint* p = A.mvpMapPoints[i]; Q.add(p, p && !p->isBad() && !sAlreadyFound.count(p), A.mvKeysUn[i].angle); }
      ps_kf_search_problem pr = ps_kf_search_problem{};
      pr.train = T.t; pr.mode = 2; points(pr, Q); view(pr, F);
      for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) pr.rcw[3 * r + c] = R[3 * r + c]; pr.tcw[r] = t[r]; }
      for (int r = 0; r < 3; r++) pr.ow[r] = (float)(-((double)R[r] * t[0] + (double)R[3 + r] * t[1] + (double)R[6 + r] * t[2]));
      pr.th = ORBdist == 100 ? 10.f : 3.f; pr.th_dist = ORBdist; pr.check_orientation = 1;
      std::vector<int32_t> match(F.N, -1);
      pr.match_of_train = match.data();
      matcher.KfSearchBatch(&pr, nullptr, 1);
      std::vector<MapPoint*> want = F.mvpMapPoints;
      int reset = 0;
      for (int j = 0; j < F.N; j++) { if (match[j] >= 0) want[j] = A.mvpMapPoints[match[j]]; else if (match[j] == -2) { want[j] = nullptr; reset++; } }
      const int n = matcher.SearchByProjection(F, &A, sAlreadyFound, pr.th, ORBdist);
      std::snprintf(detail, sizeof detail, "(ORBdist %d: %d matches, %d reset by the rotation check)", ORBdist, n, reset);
      check(n == pr.nmatches && F.mvpMapPoints == want && n >= 10, "SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) equals the struct-level call", detail);
      // ... and with the frame on the device
      DevLoopFrame G = F0;
      std::vector<ps_keypoint> kps(G.N);
      static_assert(sizeof(ps_keypoint) == sizeof(cv::KeyPoint), "ps_keypoint is cv::KeyPoint");
      std::memcpy(kps.data(), G.mvKeysUn.data(), sizeof(ps_keypoint) * G.N);
      ps_frame* f = nullptr;
      const bool ok = ps_frame_create(0, G.N, &f) == PS_OK &&
                      ps_frame_publish_host(f, kps.data(), G.mvuRight.data(), T.desc.data(), G.N, 0.f, 0.f, G.mfGridElementWidthInv, G.mfGridElementHeightInv) == PS_OK;
      int nd = -1;
      if (ok) { G.mpDeviceFrame = f; nd = matcher.SearchByProjection(G, &A, sAlreadyFound, pr.th, ORBdist); }
      if (f) ps_frame_destroy(f);
      check(ok && nd == n && G.mvpMapPoints == want, "... with mpDeviceFrame equals the host-array path");
    }
  }
  // ---- SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) ----
  {
    LoopKeyFrame A, B; std::vector<int> seenA, seenB;
    makeKeyFrame(A, Wd, rng, 0.0, 0.0f, 0.0f, seenA);
    makeKeyFrame(B, Wd, rng, 0.02, 1.5f, 0.4f, seenB);
    B.fx = 650.f;                                                      // never read: keyframe 1's intrinsics serve both directions
    for (int i = 0; i < A.N; i++) if (rng.uni() < 0.67) { A.mvpMapPoints[i] = mp[seenA[i]]; mp[seenA[i]]->AddObservation(&A, i); }
    // keyframe 2 holds points of its own at the same places (two maps before the loop is closed)
    for (int i = 0; i < B.N; i++) if (rng.uni() < 0.67) {
      LoopMapPoint* q = new LoopMapPoint(*mp[seenB[i]]);
      q->mObservations.clear(); q->AddObservation(&B, i);
      B.mvpMapPoints[i] = q;
    }
    // R12, t12 from the two poses (scale 1): c1 = R12 c2 + t12
    cv::Mat R12(3, 3, cv::CV_32F), t12(3, 1, cv::CV_32F);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) { float v = 0; for (int k = 0; k < 3; k++) v += A.Rcw.at<float>(r, k) * B.Rcw.at<float>(c, k); R12.at<float>(r, c) = v; }
    }
    for (int r = 0; r < 3; r++) { float v = A.tcw.at<float>(r); for (int k = 0; k < 3; k++) v -= R12.at<float>(r, k) * B.tcw.at<float>(k); t12.at<float>(r) = v; }
    std::vector<LoopMapPoint*> vpMatches12(A.N, nullptr);
    int pre = 0;
    for (int i2 = 0; i2 < B.N && pre < 15; i2++)
      for (int i1 = 0; i1 < A.N; i1++)
        if (B.mvpMapPoints[i2] && A.mvpMapPoints[i1] && seenA[i1] == seenB[i2] && !vpMatches12[i1]) { vpMatches12[i1] = B.mvpMapPoints[i2]; pre++; break; }
    PackedTrain T1(A), T2(B); PackedPoints Q1, Q2;
    for (LoopMapPoint* p : A.mvpMapPoints) Q1.add(p, p && !p->isBad(), 0.f);
    for (LoopMapPoint* p : B.mvpMapPoints) Q2.add(p, p && !p->isBad(), 0.f);
    std::vector<uint8_t> al1(A.N, 0), al2(B.N, 0);
    for (int i = 0; i < A.N; i++) if (vpMatches12[i]) { al1[i] = 1; const int j = vpMatches12[i]->GetIndexInKeyFrame(&B); if (j >= 0 && j < B.N) al2[j] = 1; }
    ps_sim3_problem pr = ps_sim3_problem{};
    auto side = [](ps_sim3_side& s, PackedTrain& T, PackedPoints& Q, std::vector<uint8_t>& al, LoopKeyFrame& K) {
      s.train = T.t; s.has_point = Q.valid.data(); s.pos = Q.pos.data(); s.min_dist = Q.mind.data(); s.max_dist = Q.maxd.data();
      s.point_desc = Q.desc.data(); s.already = al.data();
      for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) s.rcw[3 * r + c] = K.Rcw.at<float>(r, c); s.tcw[r] = K.tcw.at<float>(r); }
      s.bounds[0] = (float)K.mnMinX; s.bounds[1] = (float)K.mnMaxX; s.bounds[2] = (float)K.mnMinY; s.bounds[3] = (float)K.mnMaxY;
      for (int l = 0; l < 8; l++) s.scale_factors[l] = K.mvScaleFactors[l];
      s.log_scale_factor = K.mfLogScaleFactor; s.n_levels = K.mnScaleLevels;
    };
    side(pr.kf1, T1, Q1, al1, A); side(pr.kf2, T2, Q2, al2, B);
    pr.fx = A.fx; pr.fy = A.fy; pr.cx = A.cx; pr.cy = A.cy;
    ORBmatcher::Sim3Pair(1.0f, R12, t12, pr.sr12, pr.t12, pr.sr21, pr.t21);
    pr.th = 7.5f;
    std::vector<int32_t> m12(A.N, -1);
    pr.match12 = m12.data();
    matcher.SearchBySim3Batch(&pr, nullptr, nullptr, 1);
    std::vector<LoopMapPoint*> want = vpMatches12;
    for (int i = 0; i < A.N; i++) if (m12[i] >= 0) want[i] = B.mvpMapPoints[m12[i]];
    const int n = matcher.SearchBySim3(&A, &B, vpMatches12, 1.0f, R12, t12, 7.5f);
    std::snprintf(detail, sizeof detail, "(%d found beside %d matched at entry, %d x %d slots)", n, pre, A.N, B.N);
    check(n == pr.nfound && vpMatches12 == want && n >= 10 && pre >= 5, "SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) equals the struct-level call", detail);
  }
  std::printf("{\"checks\": %d, \"failed\": %d}\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
