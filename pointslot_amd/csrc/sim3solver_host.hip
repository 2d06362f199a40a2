// Host side of the loop-closure Sim3 solver: ps_sim3_ransac (sim3solver_kernels.hip) on a matcher handle - the handle's arena, pinned
// staging, one launch and one wait per call - and the host-only ps_sim3_ransac_iterations.  The call keeps no state between invocations.
#include "matcher_host.h"   // (the HIP runtime, before the plan)
#include "sim3solver_plan.h"
#include <climits>
#include <cmath>

extern "C" void psk_s3_launch(const S3Arrays*, int, int, hipStream_t);

namespace {
// what a problem costs: nothing (not launched, legal), a launch, or beyond the limits
enum { S3_IDLE = 0, S3_RUN = 1, S3_OVER = 2 };
int s3_state(const ps_sim3_ransac_problem& P) {
  if (P.n > PS_S3_MAX_N || P.nhyp > PS_S3_MAX_HYP) return S3_OVER;
  if (P.nhyp == 0 || P.n < P.min_inliers || P.n < 3) return S3_IDLE;   // (fewer than three correspondences: the reference's draw is undefined)
  return S3_RUN;
}
}  // namespace

extern "C" {
int ps_sim3_ransac(ps_matcher* m, ps_sim3_ransac_problem* probs, int nprob) {
  if (!m || nprob < 0 || (nprob > 0 && !probs)) return ps_set_error(PS_ERR_INVALID, "ps_sim3_ransac: bad argument");
  if (nprob == 0) return PS_OK;
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  std::vector<int> state(nprob);
  size_t NC = 0, NH = 0, NW = 0;
  int max_hyp = 0, nrun = 0, over = -1;
  for (int p = 0; p < nprob; p++) {
    const ps_sim3_ransac_problem& P = probs[p];
    if (P.n < 0 || P.nhyp < 0) return ps_set_error(PS_ERR_INVALID, "sim3_ransac problem %d: negative n or nhyp", p);
    const int st = state[p] = s3_state(P);
    if (st == S3_OVER && over < 0) over = p;
    if (st != S3_RUN) continue;
    if (!P.x3dc1 || !P.x3dc2 || !P.max_err1 || !P.max_err2 || !P.draws) return ps_set_error(PS_ERR_INVALID, "sim3_ransac problem %d: null input arrays", p);
    if (!P.inliers || !P.model) return ps_set_error(PS_ERR_INVALID, "sim3_ransac problem %d: null output arrays", p);
    NC += P.n; NH += P.nhyp;
    if (P.mask) NW += (size_t)P.nhyp * ((P.n + 63) / 64);
    max_hyp = std::max(max_hyp, P.nhyp);
    nrun++;
  }
  for (int p = 0; p < nprob; p++) probs[p].first_success = probs[p].best = state[p] == S3_OVER ? -2 : -1;
  if (nrun > 0) {
    Arena a;
    const size_t o_prob = a.take(sizeof(S3Prob) * nrun), o_x1 = a.take(NC * 12), o_x2 = a.take(NC * 12), o_g1 = a.take(NC * 4), o_g2 = a.take(NC * 4);
    const size_t o_draws = a.take(NH * 12), in_bytes = a.off;
    const size_t o_inl = a.take(NH * 4), o_model = a.take(NH * PS_S3_MODEL * 4), o_mask = a.take(NW * 8), out_end = a.off;
    PS_TRY(psm_ensure(m, a.off));
    uint8_t* H = m->h_buf;
    uint8_t* D = m->d_buf;
    memset(H, 0, in_bytes);
    S3Prob* hp = ptr<S3Prob>(H, o_prob);
    size_t c0 = 0, h0 = 0, w0 = 0;
    int slot = 0;
    for (int p = 0; p < nprob; p++) {
      if (state[p] != S3_RUN) continue;
      const ps_sim3_ransac_problem& P = probs[p];
      S3Prob& d = hp[slot++];
      d.n = P.n; d.nhyp = P.nhyp; d.c_off = (int32_t)c0; d.h_off = (int32_t)h0; d.nwords = (P.n + 63) / 64; d.fix_scale = P.fix_scale ? 1 : 0;
      d.m_off = P.mask ? (int64_t)w0 : -1;
      memcpy(d.k1, P.k1, 16); memcpy(d.k2, P.k2, 16);
      const size_t n = (size_t)P.n, nh = (size_t)P.nhyp;
      memcpy(H + o_x1 + c0 * 12, P.x3dc1, n * 12); memcpy(H + o_x2 + c0 * 12, P.x3dc2, n * 12);
      memcpy(H + o_g1 + c0 * 4, P.max_err1, n * 4); memcpy(H + o_g2 + c0 * 4, P.max_err2, n * 4);
      memcpy(H + o_draws + h0 * 12, P.draws, nh * 12);
      c0 += n; h0 += nh;
      if (P.mask) w0 += nh * (size_t)d.nwords;
    }
    PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
    S3Arrays A;
    A.prob = ptr<S3Prob>(D, o_prob);
    A.x1 = ptr<float>(D, o_x1); A.x2 = ptr<float>(D, o_x2); A.gate1 = ptr<float>(D, o_g1); A.gate2 = ptr<float>(D, o_g2);
    A.draws = ptr<int32_t>(D, o_draws);
    A.inliers = ptr<int32_t>(D, o_inl); A.model = ptr<float>(D, o_model); A.mask = ptr<unsigned long long>(D, o_mask);
    PS_TRY(psm_kernels_begin(m));
    psk_s3_launch(&A, nrun, max_hyp, m->stream);
    PS_TRY(psm_kernels_end(m));
    PS_HIP(hipMemcpyAsync(H + o_inl, D + o_inl, out_end - o_inl, hipMemcpyDeviceToHost, m->stream));
    PS_HIP(hipStreamSynchronize(m->stream));
    PS_TRY(psm_kernels_ms(m));
    slot = 0;
    for (int p = 0; p < nprob; p++) {
      if (state[p] != S3_RUN) continue;
      ps_sim3_ransac_problem& P = probs[p];
      const S3Prob& d = hp[slot++];
      const size_t nh = (size_t)P.nhyp;
      const int32_t* inl = ptr<int32_t>(H, o_inl) + d.h_off;
      memcpy(P.inliers, inl, nh * 4);
      memcpy(P.model, ptr<float>(H, o_model) + (size_t)d.h_off * PS_S3_MODEL, nh * PS_S3_MODEL * 4);
      if (P.mask) memcpy(P.mask, ptr<uint64_t>(H, o_mask) + d.m_off, nh * (size_t)d.nwords * 8);
      // iterate's bookkeeping (Sim3Solver.cc:184-200) over all hypotheses: `>=` lets a later tie replace the earlier best
      int best_n = 0;
      for (int h = 0; h < P.nhyp; h++) {
        if (inl[h] >= best_n) { best_n = inl[h]; P.best = h; }
        if (P.first_success < 0 && inl[h] > P.min_inliers) P.first_success = h;
      }
    }
  }
  if (over >= 0)
    return ps_set_error(PS_ERR_CAPACITY, "sim3_ransac problem %d: more than %d correspondences or more than %d hypotheses", over, PS_S3_MAX_N, PS_S3_MAX_HYP);
  return PS_OK;
}

// Sim3Solver::SetRansacParameters (Sim3Solver.cc:115-139): mRansacMaxIts for n correspondences, with its float epsilon.  A quotient
// that is not a number or does not fit an int converts as x86 does (to INT_MIN), which the clamp turns into one iteration.
int ps_sim3_ransac_iterations(double probability, int min_inliers, int max_iterations, int n, int* iterations) {
  if (!iterations || n < 0) return ps_set_error(PS_ERR_INVALID, "ps_sim3_ransac_iterations: bad argument");
  const float epsilon = (float)min_inliers / (float)n;
  int its;
  if (min_inliers == n) {
    its = 1;
  } else {
    const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
    its = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
  }
  *iterations = std::max(1, std::min(its, max_iterations));
  return PS_OK;
}
}  // extern "C"
