// The C++ Sim3Solver of the host shim (pointslot_amd/host/Sim3Solver.h) instantiated on the view types of tests/cpp/loop_view.h
// (with the two members of KeyFrame the solver reads beside them): the constructor's filters and mvnIndices1, the truncated gates,
// iterate() against a walk over the struct-level call (ps_sim3_ransac on problems packed here by hand, same draws), vbInliers
// indexed through mvnIndices1 over mN1, and PrepareBatch over three solvers against three single runs.  Prints one line per check
// and a final JSON summary; exit code 0 iff every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "loop_view.h"
#include "Sim3Solver.h"

using namespace ORB_SLAM2;

namespace {
struct SolverKeyFrame : LoopKeyFrame { std::vector<float> mvLevelSigma2; };
typedef Sim3Solver<SolverKeyFrame, LoopMapPoint> Solver;

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
  double uni(double a, double b) { return a + (b - a) * uni(); }
  int below(int n) { return (int)(uni() * n); }
  double normal() { return std::sqrt(-2 * std::log(1 - uni())) * std::cos(6.283185307179586 * uni()); }
  int raw() { return (int)(next() >> 33); }   // 0 .. 2^31 - 1, as rand()
};
int g_fail = 0, g_checks = 0;
void check(bool ok, const char* what, const char* detail = "") {
  g_checks++;
  if (!ok) g_fail++;
  std::printf("%s %s %s\n", ok ? "ok  " : "FAIL", what, detail);
}

// a loop candidate: keyframe 1 at the origin, keyframe 2 a little aside, n slots in keyframe 1 each holding a map point, and for most
// slots a map point of keyframe 2's own map at the same place (some of them wrong)
struct Pair {
  SolverKeyFrame A, B;
  std::vector<std::unique_ptr<LoopMapPoint>> own;
  std::vector<LoopMapPoint*> vpMatched12;
  LoopMapPoint* point(const float* X) {
    own.emplace_back(new LoopMapPoint());
    for (int c = 0; c < 3; c++) own.back()->mWorldPos.at<float>(c) = X[c];
    return own.back().get();
  }
  Pair(uint64_t seed, int n, double wrong) {
    Rng rng(seed);
    for (SolverKeyFrame* K : {&A, &B}) {
      K->fx = 721.5377f; K->fy = 721.5377f; K->cx = 609.5593f; K->cy = 172.854f;
      K->mvLevelSigma2.assign(8, 1.f);
      for (int l = 1; l < 8; l++) K->mvLevelSigma2[l] = (float)std::pow(1.2, 2 * l);
      for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) K->Rcw.at<float>(r, c) = r == c ? 1.f : 0.f; K->tcw.at<float>(r) = 0.f; }
      K->N = n;
      K->mvKeysUn.resize(n);
      for (int i = 0; i < n; i++) K->mvKeysUn[i].octave = rng.below(8);
      K->mvpMapPoints.assign(n, nullptr);
    }
    B.fx = 718.856f; B.cx = 607.1928f;
    const float yaw = 0.05f, c = std::cos(yaw), s = std::sin(yaw);
    const float Rb[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    for (int r = 0; r < 3; r++) for (int q = 0; q < 3; q++) B.Rcw.at<float>(r, q) = Rb[3 * r + q];
    B.tcw.at<float>(0) = -0.8f; B.tcw.at<float>(1) = 0.05f; B.tcw.at<float>(2) = 0.3f;
    vpMatched12.assign(n, nullptr);
    for (int i = 0; i < n; i++) {
      const double z = rng.uni(5, 30);
      float X[3] = {(float)(rng.uni(-0.5, 0.5) * z), (float)(rng.uni(-0.2, 0.2) * z), (float)z};
      LoopMapPoint* p1 = point(X);
      A.mvpMapPoints[i] = p1; p1->AddObservation(&A, i);
      float Y[3];
      const bool bad = rng.uni() < wrong;
      for (int k = 0; k < 3; k++) Y[k] = bad ? (float)(X[k] + rng.uni(-2, 2)) : (float)(X[k] + 0.002 * z * rng.normal());
      LoopMapPoint* p2 = point(Y);
      const int j = (i * 7 + 3) % n;                       // keyframe 2 keeps its points in an order of its own
      B.mvpMapPoints[j] = p2; p2->AddObservation(&B, j);
      vpMatched12[i] = p2;
    }
  }
};

// the struct-level call on the solver's own arrays and the given draws
struct ByHand {
  std::vector<int32_t> inliers, draws; std::vector<float> model; std::vector<uint64_t> mask;
  int first = -3, best = -3, nw = 0;
  void run(ps_matcher* h, Solver& S, bool fix, const float* k1, const float* k2, Rng rng) {
    const int nh = S.mRansacMaxIts;
    nw = (S.N + 63) / 64;
    draws.resize(3 * nh);
    for (int32_t& d : draws) d = rng.raw();
    inliers.assign(nh, -1); model.assign(13 * nh, 0.f); mask.assign((size_t)nh * nw, 0);
    ps_sim3_ransac_problem p = ps_sim3_ransac_problem{};
    p.n = S.N; p.x3dc1 = S.mvX3Dc1.data(); p.x3dc2 = S.mvX3Dc2.data(); p.max_err1 = S.mvnMaxError1.data(); p.max_err2 = S.mvnMaxError2.data();
    std::memcpy(p.k1, k1, 16); std::memcpy(p.k2, k2, 16);
    p.fix_scale = fix; p.nhyp = nh; p.draws = draws.data(); p.min_inliers = S.mRansacMinInliers;
    p.inliers = inliers.data(); p.model = model.data(); p.mask = mask.data();
    if (ps_sim3_ransac(h, &p, 1) != PS_OK) std::printf("ps_sim3_ransac: %s\n", ps_last_error());
    first = p.first_success; best = p.best;
  }
};

// iterate(step) until bNoMore or a model, recorded
struct Run { int calls = 0, nInliers = 0, its = 0; bool found = false, noMore = false; std::vector<bool> vb; std::vector<float> T; float s = 0; };
Run drive(Solver& S, int step) {
  Run r;
  for (;;) {
    bool noMore; int nIn;
    cv::Mat T = S.iterate(step, noMore, r.vb, nIn);
    r.calls++;
    if (!T.empty()) {
      r.found = true; r.nInliers = nIn; r.s = S.GetEstimatedScale();
      for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.T.push_back(T.at<float>(i, j));
      break;
    }
    if (noMore) { r.noMore = true; break; }
    if (r.calls > 1000) break;
  }
  r.its = S.mnIterations;
  return r;
}
bool same(const Run& a, const Run& b) {
  return a.calls == b.calls && a.found == b.found && a.noMore == b.noMore && a.nInliers == b.nInliers && a.its == b.its && a.vb == b.vb &&
         a.T.size() == b.T.size() && (a.T.empty() || std::memcmp(a.T.data(), b.T.data(), a.T.size() * 4) == 0);
}
}  // namespace

int main() {
  ps_matcher* h = nullptr;
  if (ps_matcher_create(0, &h) != PS_OK) { std::printf("ps_matcher_create: %s\n", ps_last_error()); return 2; }
  char detail[200];
  const float k1[4] = {721.5377f, 721.5377f, 609.5593f, 172.854f}, k2[4] = {718.856f, 721.5377f, 607.1928f, 172.854f};

  // ---- the constructor's filters, mvnIndices1 and the truncated gates ----
  {
    Pair P(0x51A3, 60, 0.3);
    LoopMapPoint stray;                                     // a point keyframe 2 does not hold: GetIndexInKeyFrame < 0
    P.vpMatched12[2] = nullptr;                             // the null match
    P.A.mvpMapPoints[4] = nullptr;                          // no point in keyframe 1's slot
    P.A.mvpMapPoints[6]->bad = true; P.vpMatched12[7]->bad = true;   // a bad point on either side
    P.vpMatched12[9] = &stray;                              // index < 0 in keyframe 2
    P.A.mvpMapPoints[11]->mObservations.clear();            // index < 0 in keyframe 1
    P.vpMatched12.resize(50);                               // mN1 is the size of vpMatched12, not of the keyframe
    Solver S(&P.A, &P.B, P.vpMatched12, false, h);
    std::vector<size_t> want;
    for (int i = 0; i < 50; i++) if (i != 2 && i != 4 && i != 6 && i != 7 && i != 9 && i != 11) want.push_back(i);
    check(S.mvnIndices1 == want && S.N == 44 && S.mN1 == 50, "the null match, the missing and bad points and the index < 0 are filtered as in the reference");
    bool gates = true, below = false;
    for (int k = 0; k < S.N; k++) {
      const int i1 = (int)S.mvnIndices1[k], i2 = P.vpMatched12[i1]->GetIndexInKeyFrame(&P.B);
      const double f1 = 9.210 * P.A.mvLevelSigma2[P.A.mvKeysUn[i1].octave], f2 = 9.210 * P.B.mvLevelSigma2[P.B.mvKeysUn[i2].octave];
      gates = gates && S.mvnMaxError1[k] == (float)std::floor(f1) && S.mvnMaxError2[k] == (float)std::floor(f2);
      below = below || S.mvnMaxError1[k] < (float)f1;
      if (P.A.mvKeysUn[i1].octave == 1) gates = gates && S.mvnMaxError1[k] == 13.f;
    }
    check(gates && below, "the gates are 9.210 * sigma2 truncated to an integer (level 1 gates at 13)");
    bool cam = true;
    for (int k = 0; k < S.N; k++) {
      const LoopMapPoint* p = P.A.mvpMapPoints[S.mvnIndices1[k]];
      for (int c = 0; c < 3; c++) cam = cam && S.mvX3Dc1[3 * k + c] == p->mWorldPos.at<float>(c);   // keyframe 1 is at the origin
    }
    check(cam, "mvX3Dc1 holds the points of the kept slots in order");

    // ---- iterate(5) against the walk over the struct-level call, vbInliers through mvnIndices1 ----
    S.SetRansacParameters(0.99, 20, 300);
    ByHand B;
    B.run(h, S, 0, k1, k2, Rng(77));
    Rng src(77);
    Solver S2(&P.A, &P.B, P.vpMatched12, false, h, [&src]() { return src.raw(); });
    S2.SetRansacParameters(0.99, 20, 300);
    const Run r = drive(S2, 5);
    bool ok = B.first >= 0 && r.found && r.its == B.first + 1 && r.calls == B.first / 5 + 1 && r.nInliers == B.inliers[B.first];
    std::vector<bool> vb(50, false);
    if (B.first >= 0)
      for (int i = 0; i < S.N; i++)
        if ((B.mask[(size_t)B.first * B.nw + (i >> 6)] >> (i & 63)) & 1) vb[S.mvnIndices1[i]] = true;
    ok = ok && r.vb == vb && r.vb.size() == 50 && !r.vb[2] && !r.vb[4];
    if (ok) {
      const float* m = &B.model[13 * B.first];
      for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) ok = ok && r.T[4 * i + j] == (float)((double)m[1 + 3 * i + j] * (double)m[0]);
        ok = ok && r.T[4 * i + 3] == m[10 + i] && r.T[12 + i] == 0.f;
      }
      ok = ok && r.T[15] == 1.f && r.s == m[0];
    }
    std::snprintf(detail, sizeof detail, "(first success at %d of %d, %d inliers of %d)", B.first, S.mRansacMaxIts, r.nInliers, S.N);
    check(ok, "iterate(5) returns at the struct-level call's first success with its model; vbInliers is indexed through mvnIndices1 over mN1", detail);
    // the walk goes on after a success, and ends with bNoMore on the call that reaches mRansacMaxIts
    int calls = 0; bool noMore = false, past = true;
    while (!noMore && calls < 400) {
      std::vector<bool> v; int n;
      const int before = S2.mnIterations;
      cv::Mat T = S2.iterate(5, noMore, v, n);
      calls++;
      past = past && S2.mnIterations > before && (T.empty() || (n == B.inliers[S2.mnIterations - 1] && n > 20));
      if (noMore) past = past && S2.mnIterations == S2.mRansacMaxIts && T.empty();
    }
    check(past && noMore && S2.mnIterations == S2.mRansacMaxIts, "mnIterations survives between calls; bNoMore comes with the call that reaches mRansacMaxIts");
  }
  // ---- too few correspondences: bNoMore at once, nothing launched ----
  {
    Pair P(0x77, 12, 0.2);
    Solver S(&P.A, &P.B, P.vpMatched12, true, h);
    S.SetRansacParameters(0.99, 20, 300);
    bool noMore = false; std::vector<bool> vb; int n = -1;
    cv::Mat T = S.iterate(5, noMore, vb, n);
    check(T.empty() && noMore && n == 0 && vb.size() == 12 && S.mnIterations == 0, "N < mRansacMinInliers: bNoMore at the first call");
  }
  // ---- PrepareBatch over three solvers equals three single runs ----
  {
    Pair P0(0xA1, 150, 0.5), P1(0xA2, 64, 0.4), P2(0xA3, 15, 0.2);
    Pair* Ps[3] = {&P0, &P1, &P2};
    Run single[3], batch[3];
    for (int k = 0; k < 3; k++) {
      Rng src(900 + k);
      Solver S(&Ps[k]->A, &Ps[k]->B, Ps[k]->vpMatched12, k == 1, h, [&src]() { return src.raw(); });
      S.SetRansacParameters(0.99, 20, 300);
      single[k] = drive(S, 5);
    }
    Rng s0(900), s1(901), s2(902);
    Rng* srcs[3] = {&s0, &s1, &s2};
    std::vector<std::unique_ptr<Solver>> own;
    std::vector<Solver*> vp;
    for (int k = 0; k < 3; k++) {
      Rng* src = srcs[k];
      own.emplace_back(new Solver(&Ps[k]->A, &Ps[k]->B, Ps[k]->vpMatched12, k == 1, h, [src]() { return src->raw(); }));
      own.back()->SetRansacParameters(0.99, 20, 300);
      vp.push_back(own.back().get());
    }
    Solver::PrepareBatch(vp);
    for (int k = 0; k < 3; k++) batch[k] = drive(*vp[k], 5);
    const bool ok = same(single[0], batch[0]) && same(single[1], batch[1]) && same(single[2], batch[2]);
    std::snprintf(detail, sizeof detail, "(found %d %d %d after %d %d %d hypotheses; the third has too few correspondences)", batch[0].found, batch[1].found,
                  batch[2].found, batch[0].its, batch[1].its, batch[2].its);
    check(ok && batch[0].found && batch[1].found && !batch[2].found && batch[2].noMore && batch[2].its == 0, "PrepareBatch over three solvers equals three single runs", detail);
  }
  ps_matcher_destroy(h);
  std::printf("{\"checks\": %d, \"failed\": %d}\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
