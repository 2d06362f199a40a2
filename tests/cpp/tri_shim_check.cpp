// ORBmatcher::SearchForTriangulation of the host shim (pointslot_amd/host/ORBmatcher.h) on the KeyFrame-shaped type of
// tests/cpp/keyframe_view.h: the reference-signature template must return the pairs of the struct-level call on a
// ps_tri_problem packed here by hand, with and without bOnlyStereo, and with keyframe 1 taken from a frame handle
// (`ps_frame* mpDeviceFrame`).  Prints one line per check and a final JSON summary; exit code 0 iff every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include "keyframe_view.h"
#include "ORBmatcher.h"

using namespace ORB_SLAM2;

namespace {
struct DevKeyFrame : KeyFrame { ps_frame* mpDeviceFrame = nullptr; };

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
  double uni(double a, double b) { return a + (b - a) * uni(); }
  int below(int n) { return (int)(uni() * n); }
  double normal() { return std::sqrt(-2 * std::log(1 - uni())) * std::cos(6.283185307179586 * uni()); }
};
const float FX = 721.5377f, FY = 721.5377f, CX = 609.5593f, CY = 172.854f, BF = 384.38148f;
const int W = 1241, H = 376, NPTS = 260, NNODES = 10;
int g_fail = 0, g_checks = 0;
void check(bool ok, const char* what, const char* detail = "") {
  g_checks++;
  if (!ok) g_fail++;
  std::printf("%s %s %s\n", ok ? "ok  " : "FAIL", what, detail);
}

struct World { std::vector<float> X; std::vector<std::vector<uint8_t>> desc; std::vector<int> oct; std::vector<float> ang; };

// a keyframe at (cxw, 0, czw) looking along +z with a small yaw: the world points it sees, in an order of its own
void makeKeyFrame(KeyFrame& K, const World& Wd, Rng& rng, double yaw, double cxw, double czw) {
  K.fx = FX; K.fy = FY; K.cx = CX; K.cy = CY; K.invfx = 1.0f / FX; K.invfy = 1.0f / FY; K.mbf = BF; K.mb = BF / FX;
  K.mvScaleFactors.assign(8, 1.f); K.mvLevelSigma2.assign(8, 1.f);
  for (int l = 1; l < 8; l++) { K.mvScaleFactors[l] = (float)(K.mvScaleFactors[l - 1] * 1.2); K.mvLevelSigma2[l] = K.mvScaleFactors[l] * K.mvScaleFactors[l]; }
  const float c = (float)std::cos(yaw), s = (float)std::sin(yaw);
  const float R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
  const float O[3] = {(float)cxw, 0.f, (float)czw};
  for (int r = 0; r < 3; r++) {
    for (int q = 0; q < 3; q++) K.Rcw.at<float>(r, q) = R[3 * r + q];
    K.Ow.at<float>(r) = O[r];
    K.tcw.at<float>(r) = -(R[3 * r] * O[0] + R[3 * r + 1] * O[1] + R[3 * r + 2] * O[2]);
  }
  std::vector<int> order(NPTS);
  for (int i = 0; i < NPTS; i++) order[i] = i;
  for (int i = NPTS - 1; i > 0; i--) std::swap(order[i], order[rng.below(i + 1)]);
  std::vector<std::vector<uint8_t>> rows;
  for (int p : order) {
    const float* X = &Wd.X[3 * p];
    float pc[3];
    for (int r = 0; r < 3; r++) pc[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + K.tcw.at<float>(r);
    if (pc[2] < 1.f) continue;
    const float u = FX * pc[0] / pc[2] + CX + (float)(0.4 * rng.normal()), v = FY * pc[1] / pc[2] + CY + (float)(0.4 * rng.normal());
    if (u < 5 || u > W - 5 || v < 5 || v > H - 5) continue;
    cv::KeyPoint k; k.pt.x = u; k.pt.y = v; k.octave = Wd.oct[p]; k.angle = std::fmod(Wd.ang[p] + (float)(2.0 * rng.normal()) + 360.f, 360.f);
    cv::KeyPoint raw = k; raw.pt.x += 0.25f;                    // mvKeys differ from mvKeysUn
    const bool stereo = pc[2] < 25.f && rng.uni() < 0.8;
    const int i = (int)K.mvKeysUn.size();
    K.mvKeysUn.push_back(k); K.mvKeys.push_back(raw);
    K.mvDepth.push_back(stereo ? pc[2] : -1.f); K.mvuRight.push_back(stereo ? u - BF / pc[2] : -1.f);
    std::vector<uint8_t> d = Wd.desc[p];
    for (int f = rng.below(9); f > 0; f--) d[rng.below(32)] ^= (uint8_t)(1u << rng.below(8));
    rows.push_back(d);
    if (rng.uni() < 0.93) K.mFeatVec[100u + 3u * (unsigned)(rng.uni() < 0.9 ? p % NNODES : rng.below(NNODES))].push_back((unsigned)i);
    K.mvpMapPoints.push_back(rng.uni() < 0.2 ? new MapPoint() : nullptr);
  }
  K.N = (int)K.mvKeysUn.size();
  K.mDescriptors.create(K.N, 32, cv::CV_8U);
  for (int i = 0; i < K.N; i++) std::memcpy(K.mDescriptors.ptr<uint8_t>(i), rows[i].data(), 32);
}

// LocalMapping::ComputeF12 (LocalMapping.cc:804-823) in double: K1^-T [t12]x R12 K2^-1
cv::Mat computeF12(KeyFrame& A, KeyFrame& B) {
  double R1[9], R2[9], t1[3], t2[3], R12[9], t12[3];
  for (int i = 0; i < 9; i++) { R1[i] = A.Rcw.at<float>(i / 3, i % 3); R2[i] = B.Rcw.at<float>(i / 3, i % 3); }
  for (int i = 0; i < 3; i++) { t1[i] = A.tcw.at<float>(i); t2[i] = B.tcw.at<float>(i); }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R12[3 * r + c] = R1[3 * r] * R2[3 * c] + R1[3 * r + 1] * R2[3 * c + 1] + R1[3 * r + 2] * R2[3 * c + 2];
  for (int r = 0; r < 3; r++) t12[r] = -(R12[3 * r] * t2[0] + R12[3 * r + 1] * t2[1] + R12[3 * r + 2] * t2[2]) + t1[r];
  const double tx[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};
  double E[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) E[3 * r + c] = tx[3 * r] * R12[c] + tx[3 * r + 1] * R12[3 + c] + tx[3 * r + 2] * R12[6 + c];
  // K^-1 = [1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1]
  const double Ki[9] = {1.0 / FX, 0, -CX / (double)FX, 0, 1.0 / FY, -CY / (double)FY, 0, 0, 1};
  double T[9];
  cv::Mat F(3, 3, cv::CV_32F);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) T[3 * r + c] = Ki[r] * E[c] + Ki[3 + r] * E[3 + c] + Ki[6 + r] * E[6 + c];   // K1^-T E
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) F.at<float>(r, c) = (float)(T[3 * r] * Ki[c] + T[3 * r + 1] * Ki[3 + c] + T[3 * r + 2] * Ki[6 + c]);
  return F;
}

// the keyframe packed by hand, independently of the shim's own marshalling
struct Packed {
  std::vector<float> x, y, xr, yr, ang, ur, depth; std::vector<int32_t> oct, node; std::vector<uint8_t> desc, occ;
  ps_tri_keyframe k;
  explicit Packed(KeyFrame& K) {
    const int n = K.N;
    node.assign(n, -1);
    for (int i = 0; i < n; i++) {
      x.push_back(K.mvKeysUn[i].pt.x); y.push_back(K.mvKeysUn[i].pt.y); xr.push_back(K.mvKeys[i].pt.x); yr.push_back(K.mvKeys[i].pt.y);
      ang.push_back(K.mvKeysUn[i].angle); oct.push_back(K.mvKeysUn[i].octave); ur.push_back(K.mvuRight[i]); depth.push_back(K.mvDepth[i]);
      occ.push_back(K.mvpMapPoints[i] ? 1 : 0);
      desc.insert(desc.end(), K.mDescriptors.ptr<uint8_t>(i), K.mDescriptors.ptr<uint8_t>(i) + 32);
    }
    for (auto& e : K.mFeatVec) for (unsigned i : e.second) node[i] = (int32_t)e.first;
    k = ps_tri_keyframe{};
    k.n = n; k.x = x.data(); k.y = y.data(); k.x_raw = xr.data(); k.y_raw = yr.data(); k.octave = oct.data(); k.angle = ang.data();
    k.u_right = ur.data(); k.depth = depth.data(); k.desc = desc.data(); k.node = node.data(); k.occupied = occ.data();
    for (int i = 0; i < 9; i++) k.rcw[i] = K.Rcw.at<float>(i / 3, i % 3);
    for (int i = 0; i < 3; i++) { k.tcw[i] = K.tcw.at<float>(i); k.ow[i] = K.Ow.at<float>(i); }
    k.fx = K.fx; k.fy = K.fy; k.cx = K.cx; k.cy = K.cy; k.invfx = K.invfx; k.invfy = K.invfy; k.mb = K.mb; k.mbf = K.mbf;
    for (int l = 0; l < 8; l++) { k.scale_factors[l] = K.mvScaleFactors[l]; k.level_sigma2[l] = K.mvLevelSigma2[l]; }
  }
};

typedef std::vector<std::pair<std::size_t, std::size_t>> Pairs;
Pairs structLevel(ORBmatcher& matcher, KeyFrame& A, KeyFrame& B, const cv::Mat& F, bool onlyStereo, int& nm) {
  Packed pa(A), pb(B);
  ps_tri_problem p = ps_tri_problem{};
  p.kf1 = pa.k; p.k = 1; p.kf2 = &pb.k;
  float f12[9];
  for (int i = 0; i < 9; i++) f12[i] = F.at<float>(i / 3, i % 3);
  p.f12 = f12; p.only_stereo = onlyStereo; p.check_orientation = 1; p.triangulate = 0; p.chain = 0;
  std::vector<int32_t> match(A.N, -1);
  int32_t nmatches = 0, nnew = 0;
  p.match = match.data(); p.nmatches = &nmatches; p.nnew = &nnew;
  matcher.CreateNewMapPoints(&p, nullptr, 1);
  Pairs out;
  for (int i = 0; i < A.N; i++) if (match[i] >= 0) out.push_back(std::make_pair((std::size_t)i, (std::size_t)match[i]));
  nm = nmatches;
  return out;
}
}  // namespace

int main() {
  Rng rng(0x7121);
  World Wd;
  for (int p = 0; p < NPTS; p++) {
    const double z = rng.uni(5, 40);
    Wd.X.push_back((float)(rng.uni(-0.5, 0.5) * z)); Wd.X.push_back((float)(rng.uni(-0.18, 0.18) * z)); Wd.X.push_back((float)z);
    std::vector<uint8_t> d(32);
    for (auto& b : d) b = (uint8_t)rng.below(256);
    Wd.desc.push_back(d); Wd.oct.push_back(rng.below(4)); Wd.ang.push_back((float)rng.uni(0, 360));
  }
  DevKeyFrame A, B;
  makeKeyFrame(A, Wd, rng, 0.0, 0.0, 0.0);
  makeKeyFrame(B, Wd, rng, 0.01, 0.3, -1.2);
  const cv::Mat F = computeF12(A, B);
  ORBmatcher matcher(0.6f, true);
  char detail[128];
  for (int onlyStereo = 0; onlyStereo < 2; onlyStereo++) {
    int nm = 0;
    const Pairs want = structLevel(matcher, A, B, F, onlyStereo != 0, nm);
    Pairs got;
    const int n = matcher.SearchForTriangulation((KeyFrame*)&A, (KeyFrame*)&B, F, got, onlyStereo != 0);
    std::snprintf(detail, sizeof detail, "(%d pairs of %d x %d features)", n, A.N, B.N);
    check(n == nm && got == want && n == (int)got.size() && n >= 10,
          onlyStereo ? "SearchForTriangulation(pKF1, pKF2, F12, pairs, true) equals the struct-level call" : "SearchForTriangulation(pKF1, pKF2, F12, pairs, false) equals the struct-level call", detail);
  }
  {
    int nm = 0;
    const Pairs want = structLevel(matcher, A, B, F, false, nm);
    std::vector<ps_keypoint> kps(A.N);
    static_assert(sizeof(ps_keypoint) == sizeof(cv::KeyPoint), "ps_keypoint is cv::KeyPoint");
    std::memcpy(kps.data(), A.mvKeysUn.data(), sizeof(ps_keypoint) * A.N);
    std::vector<uint8_t> desc((size_t)A.N * 32);
    for (int i = 0; i < A.N; i++) std::memcpy(&desc[(size_t)i * 32], A.mDescriptors.ptr<uint8_t>(i), 32);
    ps_frame* f = nullptr;
    bool ok = ps_frame_create(0, A.N, &f) == PS_OK &&
              ps_frame_publish_host(f, kps.data(), A.mvuRight.data(), desc.data(), A.N, 0.f, 0.f, 64.f / W, 48.f / H) == PS_OK;
    Pairs got;
    int n = -1;
    if (ok) {
      A.mpDeviceFrame = f;
      n = matcher.SearchForTriangulation(&A, &B, F, got, false);
      A.mpDeviceFrame = nullptr;
    }
    if (f) ps_frame_destroy(f);
    std::snprintf(detail, sizeof detail, "(%d pairs)", n);
    check(ok && n == nm && got == want, "SearchForTriangulation with mpDeviceFrame equals the host-array path", detail);
  }
  std::printf("{\"checks\": %d, \"failed\": %d}\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
