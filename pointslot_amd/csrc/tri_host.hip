// Host side of ps_create_new_map_points (tri_kernels.hip): LocalMapping::CreateNewMapPoints - SearchForTriangulation against every
// neighbour + the triangulation gates.  Keyframe 1 may come from a frame handle (FrameUse, matcher_host.h); x .. desc of every
// keyframe are a searched side without a grid (search_side.h).
#include "matcher_host.h"
#include "tri_plan.h"

extern "C" void psk_tri_launch(const TriArrays*, int, int, int, hipStream_t);

namespace {
// the host pointers one keyframe of a triangulation problem needs (on_device: x .. desc come from a frame handle)
bool tri_keyframe_ok(const ps_tri_keyframe& K, bool on_device) {
  if (K.n <= 0) return K.n == 0;
  if (!K.depth || !K.node || !K.occupied) return false;
  if ((K.x_raw == nullptr) != (K.y_raw == nullptr)) return false;
  return on_device || (K.x && K.y && K.octave && K.angle && K.u_right && K.desc);
}
void tri_fill_kf(TriKf& d, const ps_tri_keyframe& K, int32_t f_off, int32_t raw_off) {
  memset(&d, 0, sizeof(d));
  d.f_off = f_off; d.n = K.n; d.raw_off = raw_off;
  memcpy(d.rcw, K.rcw, 36); memcpy(d.tcw, K.tcw, 12); memcpy(d.ow, K.ow, 12);
  d.fx = K.fx; d.fy = K.fy; d.cx = K.cx; d.cy = K.cy; d.invfx = K.invfx; d.invfy = K.invfy; d.mb = K.mb; d.mbf = K.mbf;
  memcpy(d.scale, K.scale_factors, 32); memcpy(d.sigma2, K.level_sigma2, 32);
}
struct TriOff { SideOff k; size_t depth, xraw, yraw, occ; };
// the feature arrays of one keyframe into its slices of the staging buffer (skip_keys: x .. desc are staged on the device)
void tri_pack_kf(uint8_t* H, const TriOff& o, const ps_tri_keyframe& K, const TriKf& d, bool skip_keys) {
  const size_t n = (size_t)K.n, f = (size_t)d.f_off;
  if (n == 0) return;
  if (!skip_keys) {
    ps_proj_train T = {};
    T.n = K.n; T.x = K.x; T.y = K.y; T.octave = K.octave; T.angle = K.angle; T.u_right = K.u_right; T.desc = K.desc;
    side_pack(H, o.k, T, f, 0, SIDE_ANG | SIDE_UR, false);
  }
  memcpy(H + o.depth + f * 4, K.depth, n * 4); memcpy(H + o.occ + f, K.occupied, n);
  if (d.raw_off >= 0) { memcpy(H + o.xraw + (size_t)d.raw_off * 4, K.x_raw, n * 4); memcpy(H + o.yraw + (size_t)d.raw_off * 4, K.y_raw, n * 4); }
}

int create_new_map_points(ps_matcher* m, ps_tri_problem* probs, ps_frame* const* frames, int nprob) {
  if (!m || !probs || nprob < 1) return ps_set_error(PS_ERR_INVALID, "ps_create_new_map_points: bad argument");
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  FrameUse U;
  PS_TRY(U.init(m, frames, nprob, "triangulation"));
  std::vector<int> served, failed;
  for (int p = 0; p < nprob; p++) {
    const ps_tri_problem& P = probs[p];
    if (P.kf1.n < 0 || P.k < 0 || (P.k > 0 && (!P.kf2 || !P.f12 || !P.nmatches)) || !P.nnew)
      return ps_set_error(PS_ERR_INVALID, "triangulation problem %d: bad sizes or null pointers", p);
    bool beyond = P.kf1.n > PS_TRI_MAX_N || P.k > PS_TRI_MAX_K;
    for (int i = 0; i < P.k && i < PS_TRI_MAX_K; i++) {
      if (P.kf2[i].n < 0) return ps_set_error(PS_ERR_INVALID, "triangulation problem %d: neighbour %d has a negative count", p, i);
      beyond = beyond || P.kf2[i].n > PS_TRI_MAX_N;
    }
    if (beyond) { failed.push_back(p); continue; }
    if (!tri_keyframe_ok(P.kf1, U.of[p] != nullptr)) return ps_set_error(PS_ERR_INVALID, "triangulation problem %d: null arrays in keyframe 1", p);
    for (int i = 0; i < P.k; i++)
      if (!tri_keyframe_ok(P.kf2[i], false)) return ps_set_error(PS_ERR_INVALID, "triangulation problem %d: null arrays in neighbour %d", p, i);
    if (P.k > 0 && P.kf1.n > 0 && (!P.match || (P.triangulate && (!P.x3d || !P.status))))
      return ps_set_error(PS_ERR_INVALID, "triangulation problem %d: null output arrays", p);
    if (U.of[p]) PS_TRY(U.check(p, P.kf1.n, "triangulation"));
    served.push_back(p);
  }
  const int ns = (int)served.size();
  if (ns == 0)
    return ps_set_error(PS_ERR_CAPACITY, "triangulation problem %d (and %zu more): more than %d features in a keyframe or more than %d neighbours", failed[0],
                        failed.size() - 1, PS_TRI_MAX_N, PS_TRI_MAX_K);
  // the distinct nodes of every keyframe 1 (sorted): a feature's node becomes its index among them, a neighbour's features are
  // bucketed by that index
  std::vector<std::vector<int32_t>> nodes(ns);
  ps_parallel_for(ns, (size_t)ns << 16, [&](int s) {
    const ps_tri_keyframe& K = probs[served[s]].kf1;
    std::vector<int32_t>& un = nodes[s];
    for (int i = 0; i < K.n; i++) if (K.node[i] >= 0) un.push_back(K.node[i]);
    std::sort(un.begin(), un.end());
    un.erase(std::unique(un.begin(), un.end()), un.end());
  });
  std::vector<TriProb> hp(ns);
  std::vector<int32_t> kf_first(ns);
  size_t NF = 0, NR = 0, NO = 0, NN = 0, npairs = 0, nkf = 0;
  int max_n1 = 0, any_tri = 0;
  for (int s = 0; s < ns; s++) {
    const ps_tri_problem& P = probs[served[s]];
    TriProb& d = hp[s];
    memset(&d, 0, sizeof(d));
    d.kf1 = (int32_t)nkf; d.first_pair = (int32_t)npairs; d.k = P.k; d.n1 = P.kf1.n;
    d.only_stereo = P.only_stereo; d.check_ori = P.check_orientation; d.triangulate = P.triangulate; d.chain = P.chain;
    d.ratio_factor = P.ratio_factor;
    kf_first[s] = (int32_t)nkf;
    nkf += 1 + (size_t)P.k; npairs += (size_t)P.k;
    max_n1 = std::max(max_n1, P.kf1.n);
    any_tri |= P.triangulate ? 1 : 0;
  }
  std::vector<TriKf> hk(nkf);
  std::vector<TriPair> hr(npairs);
  for (int s = 0; s < ns; s++) {
    const ps_tri_problem& P = probs[served[s]];
    for (int i = -1; i < P.k; i++) {
      const ps_tri_keyframe& K = i < 0 ? P.kf1 : P.kf2[i];
      const bool raw = K.n > 0 && K.x_raw != nullptr;
      tri_fill_kf(hk[(size_t)kf_first[s] + 1 + i], K, (int32_t)NF, raw ? (int32_t)NR : -1);
      NF += (size_t)K.n;
      if (raw) NR += (size_t)K.n;
      if (i >= 0) {
        TriPair& r = hr[(size_t)hp[s].first_pair + i];
        memset(&r, 0, sizeof(r));
        r.prob = s; r.kf2 = kf_first[s] + 1 + i; r.node_off = (int32_t)NN; r.out_off = (int32_t)NO;
        memcpy(r.f12, P.f12 + 9 * (size_t)i, 36);
        NN += nodes[s].size() + 1; NO += (size_t)P.kf1.n;
      }
    }
  }
  if (NF > 0x7FFFFFFFull || NO > 0x7FFFFFFFull || NN > 0x7FFFFFFFull) return ps_set_error(PS_ERR_CAPACITY, "ps_create_new_map_points: the batch holds more than 2^31 features");
  Arena a;
  const size_t o_prob = a.take(sizeof(TriProb) * ns), o_pair = a.take(sizeof(TriPair) * npairs), o_kf = a.take(sizeof(TriKf) * nkf);
  TriOff O;
  O.k.take_keys(a, NF, SIDE_ANG | SIDE_UR);
  O.depth = a.take(NF * 4); O.xraw = a.take(NR * 4); O.yraw = a.take(NR * 4); O.occ = a.take(NF);
  const size_t o_aux = a.take(NF * 4), o_noff = a.take(NN * 4);
  const size_t in_bytes = U.reserve_jobs(a, ns);
  const size_t o_match = a.take(NO * 4), o_nm = a.take(npairs * 4), o_nnew = a.take((size_t)ns * 4);
  U.reserve_status(a);
  const size_t o_status = a.take(any_tri ? NO : 0), o_x3d = a.take(any_tri ? NO * 12 : 0);
  const size_t out_end = a.off;
  PS_TRY(psm_ensure(m, a.off));
  uint8_t* H = m->h_buf;
  memcpy(H + o_prob, hp.data(), sizeof(TriProb) * ns);
  if (npairs) memcpy(H + o_pair, hr.data(), sizeof(TriPair) * npairs);
  memcpy(H + o_kf, hk.data(), sizeof(TriKf) * nkf);
  for (int s = 0; s < ns; s++)   // keyframe 1 of a problem with neighbours; its slot is s
    if (hp[s].k > 0) U.add(served[s], s, hp[s].n1, hk[(size_t)kf_first[s]].f_off, 0);
  // every problem fills exactly its own slices of the staging buffer
  ps_parallel_for(ns, in_bytes, [&](int s) {
    const ps_tri_problem& P = probs[served[s]];
    const std::vector<int32_t>& un = nodes[s];
    const int nu = (int)un.size();
    const TriKf& d1 = hk[(size_t)kf_first[s]];
    tri_pack_kf(H, O, P.kf1, d1, U.of[served[s]] != nullptr);
    int32_t* aux1 = (int32_t*)(H + o_aux) + d1.f_off;
    for (int i = 0; i < P.kf1.n; i++) {
      const int32_t v = P.kf1.node[i];
      aux1[i] = v < 0 ? -1 : (int32_t)(std::lower_bound(un.begin(), un.end(), v) - un.begin());
    }
    std::vector<int32_t> slot(nu + 1), where;
    for (int i = 0; i < P.k; i++) {
      const ps_tri_keyframe& K = P.kf2[i];
      const TriKf& d2 = hk[(size_t)kf_first[s] + 1 + i];
      tri_pack_kf(H, O, K, d2, false);
      // the neighbour's features bucketed by keyframe 1's nodes: a counting sort, stable in the feature index
      int32_t* noff = (int32_t*)(H + o_noff) + hr[(size_t)hp[s].first_pair + i].node_off;
      int32_t* aux2 = (int32_t*)(H + o_aux) + d2.f_off;
      where.assign((size_t)K.n, -1);
      std::fill(slot.begin(), slot.end(), 0);
      for (int j = 0; j < K.n; j++) {
        const int32_t v = K.node[j];
        if (v < 0) continue;
        const auto it = std::lower_bound(un.begin(), un.end(), v);
        if (it == un.end() || *it != v) continue;
        where[j] = (int32_t)(it - un.begin());
        slot[where[j] + 1]++;
      }
      for (int c = 0; c < nu; c++) slot[c + 1] += slot[c];
      memcpy(noff, slot.data(), (size_t)(nu + 1) * 4);
      const int32_t filled = slot[nu];
      for (int j = 0; j < K.n; j++)
        if (where[j] >= 0) aux2[slot[where[j]]++] = j;
      for (int j = filled; j < K.n; j++) aux2[j] = 0;
    }
  });
  uint8_t* D = m->d_buf;
  PS_TRY(U.upload(m, H, D, in_bytes, SideSkip{{}, 0}));   // whole: the neighbours' sides are host arrays in every call
  PS_TRY(psm_kernels_begin(m));   // (the staging copy of frame-backed keyframes counts as kernel time of the call)
  PS_TRY(U.stage(m, D, O.k));
  const auto F = [D](size_t o) { return ptr<float>(D, o); };
  const auto I = [D](size_t o) { return ptr<int32_t>(D, o); };
  TriArrays A;
  A.prob = ptr<TriProb>(D, o_prob); A.pair = ptr<TriPair>(D, o_pair); A.kf = ptr<TriKf>(D, o_kf);
  A.x = F(O.k.x); A.y = F(O.k.y); A.oct = I(O.k.oct); A.ang = F(O.k.ang); A.ur = F(O.k.ur); A.desc = D + O.k.desc;
  A.depth = F(O.depth); A.xraw = F(O.xraw); A.yraw = F(O.yraw); A.occ = D + O.occ; A.aux = I(o_aux); A.node_off = I(o_noff);
  A.match = I(o_match); A.nmatch = I(o_nm); A.x3d = F(o_x3d); A.status = D + o_status; A.nnew = I(o_nnew);
  psk_tri_launch(&A, ns, (int)npairs, max_n1, m->stream);
  PS_TRY(psm_kernels_end(m));
  PS_HIP(hipMemcpyAsync(H + o_match, D + o_match, out_end - o_match, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  PS_TRY(psm_kernels_ms(m));
  int stale = -1;
  for (int s = 0; s < ns; s++) {
    ps_tri_problem& P = probs[served[s]];
    if (U.stale(H, s)) { stale = stale < 0 ? served[s] : stale; continue; }   // its outputs stay as the caller left them
    *P.nnew = ptr<int32_t>(H, o_nnew)[s];
    if (P.k == 0) continue;
    memcpy(P.nmatches, H + o_nm + (size_t)hp[s].first_pair * 4, (size_t)P.k * 4);
    const size_t o0 = (size_t)hr[(size_t)hp[s].first_pair].out_off, cnt = (size_t)P.k * (size_t)P.kf1.n;
    if (cnt == 0) continue;
    memcpy(P.match, H + o_match + o0 * 4, cnt * 4);
    if (P.triangulate) { memcpy(P.status, H + o_status + o0, cnt); memcpy(P.x3d, H + o_x3d + o0 * 12, cnt * 12); }
  }
  if (stale >= 0) return frame_stale_error("triangulation", stale, -1, probs[stale].kf1.n);
  if (!failed.empty())
    return ps_set_error(PS_ERR_CAPACITY, "triangulation problem %d (and %zu more): more than %d features in a keyframe or more than %d neighbours", failed[0],
                        failed.size() - 1, PS_TRI_MAX_N, PS_TRI_MAX_K);
  return PS_OK;
}
}  // namespace

extern "C" {
int ps_create_new_map_points(ps_matcher* m, ps_tri_problem* probs, int nprob) { return create_new_map_points(m, probs, nullptr, nprob); }
int ps_create_new_map_points_frames(ps_matcher* m, ps_tri_problem* probs, ps_frame* const* kf1_frames, int nprob) { return create_new_map_points(m, probs, kf1_frames, nprob); }
}  // extern "C"
