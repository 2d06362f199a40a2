// Host side of the windowed matchers of match_kernels.hip: the three ORBmatcher::SearchByProjection overloads
// (ps_search_by_projection) and the search half of ORBmatcher::Fuse (ps_fuse_search), each also with frame handles as the searched
// side.  The searched side's layout and packing: search_side.h; the frame-handle protocol: FrameUse (matcher_host.h).
#include <chrono>
#include "matcher_host.h"   // (the HIP runtime, before the plan: its vector types)
#include "match_plan.h"

static_assert(PS_SIDE_NCELL == PS_GRID_COLS * PS_GRID_ROWS, "search_side.h lays out the grid of match_plan.h");

extern "C" {
void psk_pj_launch(const PjArrays*, int, int, int, int, int, hipStream_t);
void psk_fuse_launch(const FuArrays*, int, int, hipStream_t);
}

namespace {
const int NCELL = PS_SIDE_NCELL;
// See include/pointslot_hip.h for the field mapping.  frames: nullptr, or per problem the frame handle its train side comes from.
int search_by_projection(ps_matcher* m, ps_proj_problem* probs, ps_frame* const* frames, int nprob) {
  if (!m || !probs || nprob < 1) return ps_set_error(PS_ERR_INVALID, "ps_search_by_projection: bad argument");
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  FrameUse U;
  PS_TRY(U.init(m, frames, nprob, "projection"));
  size_t NT = 0, NQ = 0;
  int max_nq = 0, max_nt = 0, any_frame = 0;
  for (int p = 0; p < nprob; p++) {
    const ps_proj_problem& P = probs[p];
    const ps_proj_train& T = P.train;
    if (U.of[p]) {
      if (T.n < 0 || P.nq < 0 || (T.n > 0 && (!T.occupied || !P.match_of_train)))
        return ps_set_error(PS_ERR_INVALID, "projection problem %d: bad train side (occupied and match_of_train stay host arrays)", p);
      PS_TRY(U.check(p, T.n, "projection"));
    } else if (T.n < 0 || T.n > 32767 || P.nq < 0 || (T.n > 0 && (!T.x || !T.y || !T.octave || !T.angle || !T.u_right || !T.desc ||
        !T.occupied || !T.cell_off || !T.cell_idx || !P.match_of_train)))
      return ps_set_error(PS_ERR_INVALID, "projection problem %d: bad train side (n <= 32767)", p);
    if (P.nq > 0 && (!P.q_valid || !P.q_desc || !P.q_observed)) return ps_set_error(PS_ERR_INVALID, "projection problem %d: null query arrays", p);
    if (P.frame_mode) {
      if (P.nq > 0 && (!P.q_xw || !P.q_octave || !P.q_angle)) return ps_set_error(PS_ERR_INVALID, "projection problem %d: frame mode needs q_xw/q_octave/q_angle", p);
      any_frame = 1;
    } else if (P.nq > 0 && (!P.q_u || !P.q_v || !P.q_ur || !P.q_radius || !P.q_radius_er || !P.q_min_level || !P.q_max_level))
      return ps_set_error(PS_ERR_INVALID, "projection problem %d: null pre-projected query arrays", p);
    if (P.use_bbox && T.n > 0 && !T.in_bbox) return ps_set_error(PS_ERR_INVALID, "projection problem %d: use_bbox without in_bbox", p);
    NT += T.n; NQ += P.nq;
    max_nq = P.nq > max_nq ? P.nq : max_nq;
    max_nt = T.n > max_nt ? T.n : max_nt;
  }
  Arena a;
  const size_t o_prob = a.take(sizeof(PjProb) * nprob);
  const PjSide S = pj_side_layout(a, NT, nprob);   // a fully frame-backed call uploads neither x .. desc nor the grids: S.t.skip()
  const size_t o_qvalid = a.take(NQ), o_qu = a.take(NQ * 4), o_qv = a.take(NQ * 4), o_qur = a.take(NQ * 4), o_qrad = a.take(NQ * 4), o_qrer = a.take(NQ * 4);
  const size_t o_qminl = a.take(NQ * 4), o_qmaxl = a.take(NQ * 4), o_qdesc = a.take(NQ * 32), o_qobs = a.take(NQ), o_qang = a.take(NQ * 4);
  const size_t o_qxw = a.take(NQ * 12), o_qoct = a.take(NQ * 4);
  const size_t in_bytes = U.reserve_jobs(a, nprob);
  const size_t o_match = a.take(NT * 4), o_nm = a.take((size_t)nprob * 4), o_ovf = a.take((size_t)nprob * 4);
  const size_t out_end = U.reserve_status(a);
  const size_t o_cand = a.take(NQ * PS_PJ_CAP * 4), o_ncand = a.take(NQ * 4), o_qbest = a.take(NQ * 4), o_qbin = a.take(NQ), o_tt = a.take(NQ * 16);
  PS_TRY(psm_ensure(m, a.off));
  uint8_t* H = m->h_buf;
  static const bool prof = getenv("PS_MATCH_PROFILE") != nullptr;   // developer switch: host-side breakdown of the call on stderr
  const auto tp0 = std::chrono::steady_clock::now();
  PjProb* hp = ptr<PjProb>(H, o_prob);
  std::vector<size_t> toff(nprob), qoff(nprob);
  for (size_t p = 0, t0 = 0, q0 = 0; p < (size_t)nprob; t0 += probs[p].train.n, q0 += probs[p].nq, p++) {
    toff[p] = t0; qoff[p] = q0;
    U.add((int)p, (int)p, probs[p].train.n, (int32_t)t0, (int32_t)p * (NCELL + 1));
  }
  // every problem fills (or zeroes) exactly its own slices of the staging buffer: independent, memcpy-bound
  ps_parallel_for(nprob, in_bytes, [&](int p) {
    const ps_proj_problem& P = probs[p];
    const ps_proj_train& T = P.train;
    const size_t t0 = toff[p], q0 = qoff[p];
    PjProb& d = hp[p];
    memset(&d, 0, sizeof(d));
    d.t_off = (int32_t)t0; d.nt = T.n; d.q_off = (int32_t)q0; d.c_off = (int32_t)q0; d.nq = P.nq; d.grid_off = p * (NCELL + 1);
    U.grid_into(d, p, T);
    d.th_dist = P.th_dist; d.ratio_test = P.ratio_test; d.nn_ratio = P.nn_ratio; d.check_ori = P.check_orientation;
    d.use_bbox = P.use_bbox; d.frame_mode = P.frame_mode;
    memcpy(d.tcw, P.tcw, 64); memcpy(d.tlw, P.tlw, 64);
    d.fx = P.fx; d.fy = P.fy; d.cx = P.cx; d.cy = P.cy; d.mbf = P.mbf; d.mb = P.mb;
    memcpy(d.bounds, P.bounds, 16); memcpy(d.scale, P.scale_factors, 32);
    d.th = P.th; d.mono = P.mono;
    if (T.n > 0) {
      const size_t n = (size_t)T.n;
      memcpy(H + S.occ + t0, T.occupied, n);
      if (T.in_bbox) memcpy(H + S.bbox + t0, T.in_bbox, n); else memset(H + S.bbox + t0, 0, n);
    }
    if (!U.staged(p, T.n)) side_pack(H, S.t, T, t0, (size_t)d.grid_off, SIDE_ANG | SIDE_UR | SIDE_GRID, false);
    if (P.nq > 0) {
      const size_t n = (size_t)P.nq;
      memcpy(H + o_qvalid + q0, P.q_valid, n); memcpy(H + o_qdesc + q0 * 32, P.q_desc, n * 32);
      memcpy(H + o_qobs + q0, P.q_observed, n);
      if (P.q_angle) memcpy(H + o_qang + q0 * 4, P.q_angle, n * 4); else memset(H + o_qang + q0 * 4, 0, n * 4);
      const size_t pre[7] = {o_qu, o_qv, o_qur, o_qrad, o_qrer, o_qminl, o_qmaxl};
      if (P.frame_mode) {
        memcpy(H + o_qxw + q0 * 12, P.q_xw, n * 12); memcpy(H + o_qoct + q0 * 4, P.q_octave, n * 4);
        for (size_t o : pre) memset(H + o + q0 * 4, 0, n * 4);
      } else {
        const void* src[7] = {P.q_u, P.q_v, P.q_ur, P.q_radius, P.q_radius_er, P.q_min_level, P.q_max_level};
        for (int k = 0; k < 7; k++) memcpy(H + pre[k] + q0 * 4, src[k], n * 4);
        memset(H + o_qxw + q0 * 12, 0, n * 12); memset(H + o_qoct + q0 * 4, 0, n * 4);
      }
    }
  });
  uint8_t* D = m->d_buf;
  const auto tp1 = std::chrono::steady_clock::now();
  PS_TRY(U.upload(m, H, D, in_bytes, S.t.skip()));
  PS_TRY(U.stage(m, D, S.t));
  if (prof) PS_HIP(hipStreamSynchronize(m->stream));
  const auto tp2 = std::chrono::steady_clock::now();
  PS_HIP(hipMemsetAsync(D + o_ovf, 0, (size_t)nprob * 4, m->stream));
  const auto F = [D](size_t o) { return ptr<float>(D, o); };
  const auto I = [D](size_t o) { return ptr<int32_t>(D, o); };
  PjArrays A;
  A.prob = ptr<PjProb>(D, o_prob);
  side_arrays(A, S.t, D);
  A.tang = F(S.t.ang); A.tur = F(S.t.ur); A.tocc = D + S.occ; A.tbbox = D + S.bbox;
  A.qvalid = D + o_qvalid; A.qu = F(o_qu); A.qv = F(o_qv); A.qur = F(o_qur); A.qrad = F(o_qrad); A.qrer = F(o_qrer);
  A.qminl = I(o_qminl); A.qmaxl = I(o_qmaxl); A.qdesc = D + o_qdesc; A.qobs = D + o_qobs; A.qang = F(o_qang);
  A.qxw = F(o_qxw); A.qoct = I(o_qoct);
  A.cand = ptr<uint32_t>(D, o_cand); A.ncand = I(o_ncand); A.match = I(o_match); A.nmatch = I(o_nm); A.overflow = I(o_ovf);
  A.qbest = I(o_qbest); A.qbin = D + o_qbin; A.ttop = ptr<uint4>(D, o_tt);
  PS_TRY(psm_kernels_begin(m));
  psk_pj_launch(&A, nprob, max_nq > 0 ? max_nq : 1, max_nt, any_frame, 0, m->stream);
  PS_TRY(psm_kernels_end(m));
  if (prof) PS_HIP(hipStreamSynchronize(m->stream));
  const auto tp3 = std::chrono::steady_clock::now();
  PS_HIP(hipMemcpyAsync(H + o_match, D + o_match, out_end - o_match, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  PS_TRY(psm_kernels_ms(m));
  const auto tp4 = std::chrono::steady_clock::now();
  if (prof) {
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "ps_search_by_projection %d problems, %.1f MB in: pack %.3f ms, upload %.3f, kernels %.3f, read-back %.3f\n", nprob, in_bytes / 1e6, ms(tp0, tp1),
            ms(tp1, tp2), ms(tp2, tp3), ms(tp3, tp4));
  }
  // Problems with a window of more than PS_PJ_CAP candidates (dense imagery, the 2 * th retry at a coarse octave) run again with
  // the wide key format - 1024 candidates per window, frames of up to 8191 features - in a compact candidate store of their own;
  // the other problems of the batch keep their results.  A problem that overflows that too (or has more features) is the only one
  // that fails: nmatches = -1, its match_of_train untouched, and the call returns PS_ERR_CAPACITY after serving the rest.
  const int32_t* ovf = ptr<int32_t>(H, o_ovf);
  std::vector<int> wide, failed, stale;
  for (int p = 0; p < nprob; p++) {
    if (U.stale(H, p)) stale.push_back(p);
    else if (ovf[p] > 0) (probs[p].train.n <= PS_PJ_WIDE_MAX_N ? wide : failed).push_back(p);
  }
  std::vector<int32_t> wide_nm(wide.size(), 0);
  if (!wide.empty()) {
    size_t nq2 = 0;
    int max_nq2 = 1, any_frame2 = 0;
    std::vector<PjProb> sub(wide.size());
    for (size_t i = 0; i < wide.size(); i++) {
      sub[i] = hp[wide[i]];
      sub[i].c_off = (int32_t)nq2;
      nq2 += probs[wide[i]].nq;
      max_nq2 = std::max(max_nq2, probs[wide[i]].nq);
      any_frame2 |= probs[wide[i]].frame_mode;
    }
    Arena w;
    const size_t w_prob = w.take(sizeof(PjProb) * sub.size()), w_nm = w.take(sub.size() * 4), w_ovf = w.take(sub.size() * 4), w_cand = w.take(nq2 * PS_PJ_CAP_WIDE * 4);
    PS_TRY(psm_ensure_wide(m, w.off));
    uint8_t* Wd = m->d_wide;
    PS_HIP(hipMemcpyAsync(Wd + w_prob, sub.data(), sizeof(PjProb) * sub.size(), hipMemcpyHostToDevice, m->stream));
    PS_HIP(hipMemsetAsync(Wd + w_ovf, 0, sub.size() * 4, m->stream));
    // (pj_project runs again on these problems: it only repeats what it wrote; the queries it invalidated stay invalid)
    PjArrays A2 = A;
    A2.prob = ptr<PjProb>(Wd, w_prob); A2.cand = ptr<uint32_t>(Wd, w_cand); A2.nmatch = ptr<int32_t>(Wd, w_nm); A2.overflow = ptr<int32_t>(Wd, w_ovf);
    psk_pj_launch(&A2, (int)sub.size(), max_nq2, max_nt, any_frame2, 1, m->stream);
    PS_HIP(hipGetLastError());
    std::vector<int32_t> ovf2(sub.size(), 0);
    PS_HIP(hipMemcpyAsync(H + o_match, D + o_match, NT * 4, hipMemcpyDeviceToHost, m->stream));
    PS_HIP(hipStreamSynchronize(m->stream));
    PS_HIP(hipMemcpy(wide_nm.data(), Wd + w_nm, sub.size() * 4, hipMemcpyDeviceToHost));
    PS_HIP(hipMemcpy(ovf2.data(), Wd + w_ovf, sub.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < wide.size(); i++)
      if (ovf2[i] > 0) { failed.push_back(wide[i]); wide_nm[i] = -1; }
  }
  for (int p = 0; p < nprob; p++) {
    ps_proj_problem& P = probs[p];
    if (std::find(failed.begin(), failed.end(), p) != failed.end() || std::find(stale.begin(), stale.end(), p) != stale.end()) { P.nmatches = -1; continue; }
    if (P.train.n > 0) memcpy(P.match_of_train, H + o_match + toff[p] * 4, (size_t)P.train.n * 4);
    P.nmatches = ptr<int32_t>(H, o_nm)[p];
  }
  for (size_t i = 0; i < wide.size(); i++)
    if (wide_nm[i] >= 0) probs[wide[i]].nmatches = wide_nm[i];
  if (!stale.empty()) return frame_stale_error("projection", stale[0], (long)stale.size() - 1, probs[stale[0]].train.n);
  if (!failed.empty())
    return ps_set_error(PS_ERR_CAPACITY, "projection problem %d (and %zu more): a search window held more than %d candidates%s", failed[0], failed.size() - 1,
                        probs[failed[0]].train.n <= PS_PJ_WIDE_MAX_N ? PS_PJ_CAP_WIDE : PS_PJ_CAP,
                        probs[failed[0]].train.n <= PS_PJ_WIDE_MAX_N ? "" : " and the frame has more features than the wide candidate store indexes (8191)");
  return PS_OK;
}

int fuse_search(ps_matcher* m, ps_fuse_problem* probs, ps_frame* const* frames, int nprob) {
  if (!m || !probs || nprob < 1) return ps_set_error(PS_ERR_INVALID, "ps_fuse_search: bad argument");
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  FrameUse U;
  PS_TRY(U.init(m, frames, nprob, "fuse"));
  size_t NT = 0, NQ = 0;
  int max_nq = 0;
  for (int p = 0; p < nprob; p++) {
    const ps_fuse_problem& P = probs[p];
    const ps_proj_train& T = P.train;
    if (U.of[p]) {
      if (T.n < 0 || P.nq < 0) return ps_set_error(PS_ERR_INVALID, "fuse problem %d: bad keyframe side", p);
      PS_TRY(U.check(p, T.n, "fuse"));
    } else if (T.n < 0 || P.nq < 0 || (T.n > 0 && (!T.x || !T.y || !T.octave || !T.u_right || !T.desc || !T.cell_off || !T.cell_idx)))
      return ps_set_error(PS_ERR_INVALID, "fuse problem %d: bad keyframe side", p);
    if (P.nq > 0 && (!P.q_valid || !P.q_pos || !P.q_normal || !P.q_min_dist || !P.q_max_dist || !P.q_desc || !P.best_idx || !P.best_dist))
      return ps_set_error(PS_ERR_INVALID, "fuse problem %d: null query arrays", p);
    if (P.n_levels < 1 || P.n_levels > 8) return ps_set_error(PS_ERR_INVALID, "fuse problem %d: n_levels must be 1..8", p);
    NT += T.n; NQ += P.nq;
    max_nq = P.nq > max_nq ? P.nq : max_nq;
  }
  if (NQ == 0) return PS_OK;
  Arena a;
  const size_t o_prob = a.take(sizeof(FuProb) * nprob);
  const SideOff S = fu_side_layout(a, NT, nprob);   // a fully frame-backed call uploads none of it: S.skip()
  const size_t o_qvalid = a.take(NQ), o_qpos = a.take(NQ * 12), o_qnor = a.take(NQ * 12), o_qmin = a.take(NQ * 4), o_qmax = a.take(NQ * 4), o_qdesc = a.take(NQ * 32);
  const size_t in_bytes = U.reserve_jobs(a, nprob);
  const size_t o_bi = a.take(NQ * 4), o_bd = a.take(NQ * 4);
  PS_TRY(psm_ensure(m, U.reserve_status(a)));
  uint8_t* H = m->h_buf;
  memset(H, 0, in_bytes);
  FuProb* hp = ptr<FuProb>(H, o_prob);
  size_t t0 = 0, q0 = 0;
  for (int p = 0; p < nprob; p++) {
    const ps_fuse_problem& P = probs[p];
    const ps_proj_train& T = P.train;
    FuProb& d = hp[p];
    d.t_off = (int32_t)t0; d.nt = T.n; d.q_off = (int32_t)q0; d.nq = P.nq; d.grid_off = p * (NCELL + 1);
    U.grid_into(d, p, T);
    memcpy(d.R, P.rcw, 36); memcpy(d.t, P.tcw, 12); memcpy(d.ow, P.ow, 12);
    d.fx = P.fx; d.fy = P.fy; d.cx = P.cx; d.cy = P.cy; d.bf = P.bf;
    memcpy(d.bounds, P.bounds, 32); memcpy(d.scale, P.scale_factors, 32); memcpy(d.inv_sigma2, P.inv_level_sigma2, 32);
    d.log_scale = P.log_scale_factor; d.n_levels = P.n_levels; d.th = P.th;
    if (!U.add(p, p, T.n, (int32_t)t0, d.grid_off)) side_pack(H, S, T, t0, (size_t)d.grid_off, SIDE_UR | SIDE_GRID, true);
    if (P.nq > 0) {
      memcpy(H + o_qvalid + q0, P.q_valid, P.nq); memcpy(H + o_qpos + q0 * 12, P.q_pos, (size_t)P.nq * 12);
      memcpy(H + o_qnor + q0 * 12, P.q_normal, (size_t)P.nq * 12); memcpy(H + o_qmin + q0 * 4, P.q_min_dist, (size_t)P.nq * 4);
      memcpy(H + o_qmax + q0 * 4, P.q_max_dist, (size_t)P.nq * 4); memcpy(H + o_qdesc + q0 * 32, P.q_desc, (size_t)P.nq * 32);
    }
    t0 += T.n; q0 += P.nq;
  }
  uint8_t* D = m->d_buf;
  PS_TRY(U.upload(m, H, D, in_bytes, S.skip()));
  PS_TRY(U.stage(m, D, S));
  const auto F = [D](size_t o) { return ptr<float>(D, o); };
  FuArrays A;
  A.prob = ptr<FuProb>(D, o_prob);
  side_arrays(A, S, D);
  A.tur = F(S.ur);
  A.qvalid = D + o_qvalid; A.qpos = F(o_qpos); A.qnormal = F(o_qnor); A.qmin = F(o_qmin); A.qmax = F(o_qmax); A.qdesc = D + o_qdesc;
  A.best_idx = ptr<int32_t>(D, o_bi); A.best_dist = ptr<int32_t>(D, o_bd);
  psk_fuse_launch(&A, nprob, max_nq, m->stream);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(H + o_bi, D + o_bi, a.off - o_bi, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  q0 = 0;
  int stale = -1;
  for (int p = 0; p < nprob; p++) {
    ps_fuse_problem& P = probs[p];
    if (U.stale(H, p)) {   // its outputs stay as the caller left them
      stale = stale < 0 ? p : stale;
    } else if (P.nq > 0) {
      memcpy(P.best_idx, H + o_bi + q0 * 4, (size_t)P.nq * 4);
      memcpy(P.best_dist, H + o_bd + q0 * 4, (size_t)P.nq * 4);
    }
    q0 += P.nq;
  }
  if (stale >= 0) return frame_stale_error("fuse", stale, -1, probs[stale].train.n);
  return PS_OK;
}
}  // namespace

extern "C" {
int ps_search_by_projection(ps_matcher* m, ps_proj_problem* probs, int nprob) { return search_by_projection(m, probs, nullptr, nprob); }
int ps_search_by_projection_frames(ps_matcher* m, ps_proj_problem* probs, ps_frame* const* frames, int nprob) { return search_by_projection(m, probs, frames, nprob); }
int ps_fuse_search(ps_matcher* m, ps_fuse_problem* probs, int nprob) { return fuse_search(m, probs, nullptr, nprob); }
int ps_fuse_search_frames(ps_matcher* m, ps_fuse_problem* probs, ps_frame* const* frames, int nprob) { return fuse_search(m, probs, frames, nprob); }
}  // extern "C"
