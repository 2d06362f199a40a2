// Host side of the loop-closure and relocalisation projection matchers: ps_kf_search, ps_search_by_sim3 (kfsearch_kernels.hip), each
// also with frame handles as the searched sides.  Both calls become one batch of jobs for ks_run.  The searched side's layout and
// packing: search_side.h; the frame-handle protocol: FrameUse (matcher_host.h).
#include "matcher_host.h"   // (the HIP runtime, before the plan: its vector types)
#include "kfsearch_plan.h"

extern "C" void psk_ks_launch(const KsArrays*, int, int, int, int, hipStream_t);

namespace {
// one search as the caller described it: a ps_kf_search problem, or one direction of a ps_search_by_sim3 problem
struct KsHostJob {
  const ps_proj_train* T = nullptr;
  ps_frame* frame = nullptr;
  int kind = 0, nq = 0;
  const uint8_t* q_valid = nullptr;
  const uint8_t* q_already = nullptr;   // Sim3: valid = has_point && !already
  const float* q_pos = nullptr; const float* q_normal = nullptr; const float* q_min = nullptr; const float* q_max = nullptr;
  const uint8_t* q_desc = nullptr; const float* q_angle = nullptr;
  const float* R = nullptr; const float* t = nullptr; const float* ow = nullptr; const float* R2 = nullptr; const float* t2 = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0;
  const float* bounds = nullptr; const float* scale = nullptr;
  float log_scale = 0, th = 0;
  int n_levels = 0, th_dist = 0, check_ori = 0;
  bool skip = false;                    // beyond the limits: not served
  int status = 0;                       // out: 0 served, 1 capacity, 2 the frame handle does not hold the frame described
  size_t t_off = 0, q_off = 0;          // out: where its results are in the buffers of KsOut
  int nmatch = 0;                       // out (ordered kinds)
};
struct KsOut { const int32_t* best_idx; const int32_t* best_dist; const int32_t* match; const int32_t* match12; const int32_t* nfound; };

bool ks_ordered(int kind) { return kind == 0 || kind == 2; }

// Packs, uploads, launches and reads back one batch of searches.  npair > 0: jobs 2p, 2p + 1 are the two directions of Sim3 problem p.
// The handle's lock is held by the caller; `out` points into the pinned staging buffer and is valid until the handle's next call.
int ks_run(ps_matcher* m, std::vector<KsHostJob>& jobs, int npair, const char* what, KsOut& out) {
  const int nj = (int)jobs.size();
  std::vector<ps_frame*> fr(nj, nullptr);
  for (int j = 0; j < nj; j++) fr[j] = jobs[j].skip ? nullptr : jobs[j].frame;
  FrameUse U;
  PS_TRY(U.init(m, fr.data(), nj, what));
  size_t NT = 0, NQ = 0, NQO = 0;
  int max_nq = 1, any_ordered = 0;
  for (int j = 0; j < nj; j++) {
    KsHostJob& J = jobs[j];
    J.t_off = NT; J.q_off = NQ;
    if (J.skip) continue;
    if (U.of[j]) PS_TRY(U.check(j, J.T->n, what));
    NT += J.T->n; NQ += J.nq;
    if (ks_ordered(J.kind)) { NQO += J.nq; any_ordered = 1; }
    max_nq = std::max(max_nq, J.nq);
  }
  Arena a;
  const size_t o_job = a.take(sizeof(KsJob) * nj), o_pair = a.take(sizeof(KsPair) * (npair > 0 ? npair : 1));
  const KsSide S = ks_side_layout(a, NT, nj);   // a fully frame-backed call uploads neither x .. desc nor the grids: S.t.skip()
  const size_t o_qvalid = a.take(NQ), o_qpos = a.take(NQ * 12), o_qnor = a.take(NQ * 12), o_qmin = a.take(NQ * 4), o_qmax = a.take(NQ * 4), o_qdesc = a.take(NQ * 32);
  const size_t o_qang = a.take(NQ * 4);
  const size_t in_bytes = U.reserve_jobs(a, nj);
  const size_t o_bi = a.take(NQ * 4), o_bd = a.take(NQ * 4), o_match = a.take(NT * 4), o_m12 = a.take(NQ * 4), o_nm = a.take((size_t)nj * 4), o_ovf = a.take((size_t)nj * 4);
  const size_t o_nf = a.take((size_t)(npair > 0 ? npair : 1) * 4), counts_end = a.off;
  const size_t out_end = U.reserve_status(a);
  const size_t o_cand = a.take(NQO * PS_KS_CAP * 4), o_ncand = a.take(NQ * 4), o_qtop = a.take(NQ * 4);
  PS_TRY(psm_ensure(m, a.off));
  uint8_t* H = m->h_buf;
  uint8_t* D = m->d_buf;
  memset(H, 0, in_bytes);
  KsJob* hj = ptr<KsJob>(H, o_job);
  size_t c0 = 0;
  for (int j = 0; j < nj; j++) {
    const KsHostJob& J = jobs[j];
    KsJob& d = hj[j];
    d.kind = J.kind; d.grid_off = j * (PS_SIDE_NCELL + 1); d.t_off = (int32_t)J.t_off; d.q_off = (int32_t)J.q_off; d.cap = PS_KS_CAP;
    if (J.skip) continue;               // nt = nq = 0: nothing is launched for it
    const ps_proj_train& T = *J.T;
    const size_t t0 = J.t_off, q0 = J.q_off;
    d.nt = T.n; d.nq = J.nq;
    U.grid_into(d, j, T);
    if (ks_ordered(J.kind)) { d.c_off = (int32_t)c0; c0 += J.nq; }
    memcpy(d.R, J.R, 36); memcpy(d.t, J.t, 12);
    if (J.ow) memcpy(d.ow, J.ow, 12);
    if (J.R2) { memcpy(d.R2, J.R2, 36); memcpy(d.t2, J.t2, 12); }
    d.fx = J.fx; d.fy = J.fy; d.cx = J.cx; d.cy = J.cy;
    memcpy(d.bounds, J.bounds, 16); memcpy(d.scale, J.scale, 32);
    d.log_scale = J.log_scale; d.n_levels = J.n_levels; d.th = J.th; d.th_dist = J.th_dist; d.check_ori = J.check_ori;
    if (!U.add(j, j, T.n, (int32_t)t0, d.grid_off)) side_pack(H, S.t, T, t0, (size_t)d.grid_off, SIDE_ANG | SIDE_GRID, true);   // (u_right: zeros)
    if (T.n > 0 && ks_ordered(J.kind)) memcpy(H + S.occ + t0, T.occupied, (size_t)T.n);
    if (J.nq > 0) {
      const size_t n = (size_t)J.nq;
      if (J.q_already) {
        uint8_t* v = H + o_qvalid + q0;
        for (size_t i = 0; i < n; i++) v[i] = J.q_valid[i] && !J.q_already[i];
      } else {
        memcpy(H + o_qvalid + q0, J.q_valid, n);
      }
      memcpy(H + o_qpos + q0 * 12, J.q_pos, n * 12); memcpy(H + o_qmin + q0 * 4, J.q_min, n * 4);
      memcpy(H + o_qmax + q0 * 4, J.q_max, n * 4); memcpy(H + o_qdesc + q0 * 32, J.q_desc, n * 32);
      if (J.q_normal) memcpy(H + o_qnor + q0 * 12, J.q_normal, n * 12);
      if (J.q_angle) memcpy(H + o_qang + q0 * 4, J.q_angle, n * 4);
    }
  }
  KsPair* hp = ptr<KsPair>(H, o_pair);
  for (int p = 0; p < npair; p++) {
    const KsHostJob& j1 = jobs[2 * p];
    const KsHostJob& j2 = jobs[2 * p + 1];
    hp[p] = j1.skip ? KsPair{0, 0, 0, 0} : KsPair{(int32_t)j1.q_off, j1.nq, (int32_t)j2.q_off, j2.nq};
  }
  PS_TRY(U.upload(m, H, D, in_bytes, S.t.skip()));
  PS_HIP(hipMemsetAsync(D + o_nm, 0, counts_end - o_nm, m->stream));   // nmatch, overflow, nfound
  PS_TRY(U.stage(m, D, S.t));
  const auto F = [D](size_t o) { return ptr<float>(D, o); };
  const auto I = [D](size_t o) { return ptr<int32_t>(D, o); };
  KsArrays A;
  A.job = ptr<KsJob>(D, o_job);
  side_arrays(A, S.t, D);
  A.tang = F(S.t.ang); A.tocc = D + S.occ;
  A.qvalid = D + o_qvalid; A.qpos = F(o_qpos); A.qnormal = F(o_qnor); A.qmin = F(o_qmin); A.qmax = F(o_qmax); A.qdesc = D + o_qdesc; A.qang = F(o_qang);
  A.best_idx = I(o_bi); A.best_dist = I(o_bd);
  A.cand = ptr<uint32_t>(D, o_cand); A.ncand = I(o_ncand); A.qtop = ptr<uint32_t>(D, o_qtop);
  A.match = I(o_match); A.nmatch = I(o_nm); A.overflow = I(o_ovf);
  A.pair = ptr<KsPair>(D, o_pair); A.match12 = I(o_m12); A.nfound = I(o_nf);
  PS_TRY(psm_kernels_begin(m));
  psk_ks_launch(&A, nj, max_nq, any_ordered, npair, m->stream);
  PS_TRY(psm_kernels_end(m));
  PS_HIP(hipMemcpyAsync(H + o_bi, D + o_bi, out_end - o_bi, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  PS_TRY(psm_kernels_ms(m));
  // An order-dependent job in which a point kept more than PS_KS_CAP candidates runs again with rows of PS_KS_CAP_WIDE in a store
  // of its own; the others keep their results.  One that overflows that too is the only one that fails.
  std::vector<int> wide;
  for (int j = 0; j < nj; j++) {
    KsHostJob& J = jobs[j];
    J.status = J.skip ? 1 : U.stale(H, j) ? 2 : 0;
    J.nmatch = ptr<int32_t>(H, o_nm)[j];
    if (J.status == 0 && ptr<int32_t>(H, o_ovf)[j] > 0) wide.push_back(j);
  }
  if (!wide.empty()) {
    std::vector<KsJob> sub(wide.size());
    size_t nq2 = 0;
    int max_nq2 = 1;
    for (size_t i = 0; i < wide.size(); i++) {
      sub[i] = hj[wide[i]];
      sub[i].c_off = (int32_t)nq2; sub[i].cap = PS_KS_CAP_WIDE;
      nq2 += sub[i].nq;
      max_nq2 = std::max(max_nq2, sub[i].nq);
    }
    Arena w;
    const size_t w_job = w.take(sizeof(KsJob) * sub.size()), w_nm = w.take(sub.size() * 4), w_ovf = w.take(sub.size() * 4), w_cand = w.take(nq2 * PS_KS_CAP_WIDE * 4);
    PS_TRY(psm_ensure_wide(m, w.off));
    uint8_t* Wd = m->d_wide;
    PS_HIP(hipMemcpyAsync(Wd + w_job, sub.data(), sizeof(KsJob) * sub.size(), hipMemcpyHostToDevice, m->stream));
    PS_HIP(hipMemsetAsync(Wd + w_nm, 0, w_cand - w_nm, m->stream));
    KsArrays A2 = A;
    A2.job = ptr<KsJob>(Wd, w_job); A2.cand = ptr<uint32_t>(Wd, w_cand); A2.nmatch = ptr<int32_t>(Wd, w_nm); A2.overflow = ptr<int32_t>(Wd, w_ovf);
    psk_ks_launch(&A2, (int)sub.size(), max_nq2, 1, 0, m->stream);
    PS_HIP(hipGetLastError());
    std::vector<int32_t> nm2(sub.size(), 0), ovf2(sub.size(), 0);
    PS_HIP(hipMemcpyAsync(H + o_match, D + o_match, NT * 4, hipMemcpyDeviceToHost, m->stream));
    PS_HIP(hipStreamSynchronize(m->stream));
    PS_HIP(hipMemcpy(nm2.data(), Wd + w_nm, sub.size() * 4, hipMemcpyDeviceToHost));
    PS_HIP(hipMemcpy(ovf2.data(), Wd + w_ovf, sub.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < wide.size(); i++) {
      jobs[wide[i]].nmatch = nm2[i];
      if (ovf2[i] > 0) jobs[wide[i]].status = 1;
    }
  }
  out.best_idx = ptr<int32_t>(H, o_bi); out.best_dist = ptr<int32_t>(H, o_bd); out.match = ptr<int32_t>(H, o_match);
  out.match12 = ptr<int32_t>(H, o_m12); out.nfound = ptr<int32_t>(H, o_nf);
  return PS_OK;
}

int ks_bad_train(const ps_proj_train& T, bool framed, bool need_occ, bool need_angle) {
  if (T.n < 0) return 1;
  if (T.n == 0 || T.n > PS_KS_MAX_N) return 0;
  if (need_occ && !T.occupied) return 1;
  if (framed) return 0;
  if (!T.x || !T.y || !T.octave || !T.desc || !T.cell_off || !T.cell_idx) return 1;
  if (need_angle && !T.angle) return 1;
  return 0;
}

// what the two calls report once every job has been served or has failed
int ks_report(const std::vector<KsHostJob>& jobs, int per_problem, const char* what) {
  int stale = -1, failed = -1;
  for (size_t j = 0; j < jobs.size(); j++) {
    if (jobs[j].status == 2 && stale < 0) stale = (int)j / per_problem;
    if (jobs[j].status == 1 && failed < 0) failed = (int)j / per_problem;
  }
  if (stale >= 0) return frame_stale_error(what, stale, -1, -1);
  if (failed >= 0)
    return ps_set_error(PS_ERR_CAPACITY, "%s problem %d: more than %d features in the searched side, more than %d points, or a point "
                        "with more than %d candidates it could take", what, failed, PS_KS_MAX_N, PS_KS_MAX_NQ, PS_KS_CAP_WIDE);
  return PS_OK;
}

int kf_search(ps_matcher* m, ps_kf_search_problem* probs, ps_frame* const* frames, int nprob) {
  if (!m || nprob < 0 || (nprob > 0 && !probs)) return ps_set_error(PS_ERR_INVALID, "ps_kf_search: bad argument");
  if (nprob == 0) return PS_OK;
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  std::vector<KsHostJob> jobs(nprob);
  for (int p = 0; p < nprob; p++) {
    const ps_kf_search_problem& P = probs[p];
    KsHostJob& J = jobs[p];
    if (P.mode < 0 || P.mode > 2) return ps_set_error(PS_ERR_INVALID, "kf_search problem %d: mode must be 0, 1 or 2", p);
    const bool ord = P.mode != 1, ori = P.mode == 2 && P.check_orientation;
    J.frame = frames ? frames[p] : nullptr;
    if (P.nq < 0 || ks_bad_train(P.train, J.frame != nullptr, ord, ori))
      return ps_set_error(PS_ERR_INVALID, "kf_search problem %d: bad searched side (occupied stays a host array)", p);
    if (P.nq > 0 && (!P.q_valid || !P.q_pos || !P.q_min_dist || !P.q_max_dist || !P.q_desc || (P.mode != 2 && !P.q_normal) || (ori && !P.q_angle)))
      return ps_set_error(PS_ERR_INVALID, "kf_search problem %d: null query arrays", p);
    if (ord ? (P.train.n > 0 && !P.match_of_train) : (P.nq > 0 && (!P.best_idx || !P.best_dist)))
      return ps_set_error(PS_ERR_INVALID, "kf_search problem %d: null output arrays", p);
    if (P.n_levels < 1 || P.n_levels > 8) return ps_set_error(PS_ERR_INVALID, "kf_search problem %d: n_levels must be 1..8", p);
    if (P.mode == 2 && (P.th_dist < 0 || P.th_dist > 255)) return ps_set_error(PS_ERR_INVALID, "kf_search problem %d: th_dist must be 0..255", p);
    J.T = &P.train; J.kind = P.mode; J.nq = P.nq;
    J.q_valid = P.q_valid; J.q_pos = P.q_pos; J.q_normal = P.mode != 2 ? P.q_normal : nullptr; J.q_min = P.q_min_dist; J.q_max = P.q_max_dist;
    J.q_desc = P.q_desc; J.q_angle = ori ? P.q_angle : nullptr;
    J.R = P.rcw; J.t = P.tcw; J.ow = P.ow;
    J.fx = P.fx; J.fy = P.fy; J.cx = P.cx; J.cy = P.cy; J.bounds = P.bounds; J.scale = P.scale_factors;
    J.log_scale = P.log_scale_factor; J.n_levels = P.n_levels; J.th = P.th;
    J.th_dist = P.mode == 2 ? P.th_dist : 50;   // TH_LOW
    J.check_ori = ori ? 1 : 0;
    J.skip = P.train.n > PS_KS_MAX_N || P.nq > PS_KS_MAX_NQ;
  }
  KsOut O;
  int rc = ks_run(m, jobs, 0, "kf_search", O);
  if (rc != PS_OK) return rc;
  for (int p = 0; p < nprob; p++) {
    ps_kf_search_problem& P = probs[p];
    const KsHostJob& J = jobs[p];
    if (J.status) { P.nmatches = -1; continue; }
    if (P.mode == 1) {
      int nf = 0;
      if (P.nq > 0) {
        memcpy(P.best_idx, O.best_idx + J.q_off, (size_t)P.nq * 4);
        memcpy(P.best_dist, O.best_dist + J.q_off, (size_t)P.nq * 4);
        for (int i = 0; i < P.nq; i++) nf += P.best_idx[i] >= 0;
      }
      P.nmatches = nf;
    } else {
      if (P.train.n > 0) memcpy(P.match_of_train, O.match + J.t_off, (size_t)P.train.n * 4);
      P.nmatches = J.nmatch;
    }
  }
  return ks_report(jobs, 1, "kf_search");
}

int search_by_sim3(ps_matcher* m, ps_sim3_problem* probs, ps_frame* const* frames1, ps_frame* const* frames2, int nprob) {
  if (!m || nprob < 0 || (nprob > 0 && !probs)) return ps_set_error(PS_ERR_INVALID, "ps_search_by_sim3: bad argument");
  if (nprob == 0) return PS_OK;
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  std::vector<KsHostJob> jobs((size_t)2 * nprob);
  for (int p = 0; p < nprob; p++) {
    const ps_sim3_problem& P = probs[p];
    const ps_sim3_side* S[2] = {&P.kf1, &P.kf2};
    ps_frame* F[2] = {frames1 ? frames1[p] : nullptr, frames2 ? frames2[p] : nullptr};
    for (int s = 0; s < 2; s++) {
      const ps_sim3_side& K = *S[s];
      if (ks_bad_train(K.train, F[s] != nullptr, false, false)) return ps_set_error(PS_ERR_INVALID, "sim3 problem %d: bad features of keyframe %d", p, s + 1);
      if (K.train.n > 0 && (!K.has_point || !K.pos || !K.min_dist || !K.max_dist || !K.point_desc || !K.already))
        return ps_set_error(PS_ERR_INVALID, "sim3 problem %d: null map-point arrays of keyframe %d", p, s + 1);
      if (K.n_levels < 1 || K.n_levels > 8) return ps_set_error(PS_ERR_INVALID, "sim3 problem %d: n_levels must be 1..8", p);
    }
    if (P.kf1.train.n > 0 && !P.match12) return ps_set_error(PS_ERR_INVALID, "sim3 problem %d: null match12", p);
    const bool skip = P.kf1.train.n > PS_KS_MAX_N || P.kf2.train.n > PS_KS_MAX_N;
    for (int s = 0; s < 2; s++) {       // direction s: the points of keyframe s + 1 into the features of the other one
      const ps_sim3_side& Q = *S[s];
      const ps_sim3_side& T = *S[1 - s];
      KsHostJob& J = jobs[(size_t)2 * p + s];
      J.T = &T.train; J.frame = F[1 - s]; J.kind = 3; J.nq = Q.train.n;
      J.q_valid = Q.has_point; J.q_already = Q.already; J.q_pos = Q.pos; J.q_min = Q.min_dist; J.q_max = Q.max_dist; J.q_desc = Q.point_desc;
      J.R = Q.rcw; J.t = Q.tcw; J.R2 = s == 0 ? P.sr21 : P.sr12; J.t2 = s == 0 ? P.t21 : P.t12;
      J.fx = P.fx; J.fy = P.fy; J.cx = P.cx; J.cy = P.cy;
      J.bounds = T.bounds; J.scale = T.scale_factors; J.log_scale = T.log_scale_factor; J.n_levels = T.n_levels;
      J.th = P.th; J.th_dist = 100;     // TH_HIGH
      J.skip = skip;
    }
  }
  KsOut O;
  int rc = ks_run(m, jobs, nprob, "sim3", O);
  if (rc != PS_OK) return rc;
  for (int p = 0; p < nprob; p++) {
    ps_sim3_problem& P = probs[p];
    KsHostJob& a = jobs[(size_t)2 * p];
    KsHostJob& b = jobs[(size_t)2 * p + 1];
    if (a.status || b.status) { a.status = b.status = std::max(a.status, b.status); P.nfound = -1; continue; }
    const size_t n1 = (size_t)P.kf1.train.n, n2 = (size_t)P.kf2.train.n;
    if (n1 > 0) memcpy(P.match12, O.match12 + a.q_off, n1 * 4);
    if (n1 > 0 && P.match1) memcpy(P.match1, O.best_idx + a.q_off, n1 * 4);
    if (n2 > 0 && P.match2) memcpy(P.match2, O.best_idx + b.q_off, n2 * 4);
    P.nfound = O.nfound[p];
  }
  return ks_report(jobs, 2, "sim3");
}
}  // namespace

extern "C" {
int ps_kf_search(ps_matcher* m, ps_kf_search_problem* probs, int nprob) { return kf_search(m, probs, nullptr, nprob); }
int ps_kf_search_frames(ps_matcher* m, ps_kf_search_problem* probs, ps_frame* const* frames, int nprob) { return kf_search(m, probs, frames, nprob); }
int ps_search_by_sim3(ps_matcher* m, ps_sim3_problem* probs, int nprob) { return search_by_sim3(m, probs, nullptr, nullptr, nprob); }
int ps_search_by_sim3_frames(ps_matcher* m, ps_sim3_problem* probs, ps_frame* const* frames1, ps_frame* const* frames2, int nprob) {
  return search_by_sim3(m, probs, frames1, frames2, nprob);
}
}  // extern "C"
