// Host side of the matcher C-ABI (include/pointslot_hip.h): packs the caller's per-object problems into
// one upload, launches the kernels of match_kernels.hip on the handle's stream, copies the results back.
// Replaces ORBmatcher::SearchByBruceMatching / DescriptorDistance — /root/reference/src/ORBmatcher.cc.
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <mutex>
#include <string.h>
#include <vector>
#include "frame_host.h"
#include "match_plan.h"
#include "matcher_host.h"
#include "tri_plan.h"
#include "kfsearch_plan.h"
#include "ps_common.h"

extern "C" {
void psk_bf_launch(const BfBlock*, int, const BfProb*, int, const uint8_t*, const float*, const uint8_t*, const uint8_t*,
                   const float*, uint32_t*, int32_t*, int32_t*, float, int, hipStream_t);
void psk_hamming_matrix_launch(const uint8_t*, int, const uint8_t*, int, uint16_t*, hipStream_t);
void psk_pj_launch(const PjArrays*, int, int, int, int, int, hipStream_t);
void psk_fuse_launch(const FuArrays*, int, int, hipStream_t);
void psk_distinctive_launch(const uint8_t*, const int32_t*, int32_t*, int, hipStream_t);
void psk_frame_stage_launch(const FrameStageJob*, int, const FrameStageDst*, hipStream_t);
void psk_tri_launch(const TriArrays*, int, int, int, hipStream_t);
}

namespace {
inline size_t al(size_t v) { return (v + 255) / 256 * 256; }

int ensure(ps_matcher* m, size_t need) {
  // 25 % headroom: batch sizes drift from call to call (keypoint counts), and re-allocating pinned memory costs milliseconds
  const size_t bytes = (need > m->d_bytes || need > m->h_bytes) ? al(need + need / 4) : need;
  if (bytes > m->d_bytes) {
    if (m->d_buf) hipFree(m->d_buf);
    m->d_buf = nullptr;
    PS_HIP(hipMalloc(&m->d_buf, bytes));
    if (const char* fill = getenv("PS_DEBUG_FILL")) {   // diagnostic: poison fresh device memory.  hipMemset on device memory returns before the fill has run, and it runs
      PS_HIP(hipMemset(m->d_buf, atoi(fill), bytes));                 // on the null stream, which the handle's non-blocking stream does not wait for: without the wait the fill
      PS_HIP(hipDeviceSynchronize());        // landed on top of the call's uploads now and then (r06: 2 of 50 runs of the poisoned test slice died of it)
    }
    m->d_bytes = bytes;
  }
  if (bytes > m->h_bytes) {
    if (m->h_buf) hipHostFree(m->h_buf);
    m->h_buf = nullptr;
    PS_HIP(hipHostMalloc(&m->h_buf, bytes, hipHostMallocDefault));
    m->h_bytes = bytes;
  }
  return PS_OK;
}

// The frame-backed problems of one search call (ps_search_by_projection_frames / ps_fuse_search_frames): which problems take their train
// side from a frame handle, the handles each once in locking order, and a copy of what the handles said when the call looked.
struct FrameUse {
  std::vector<ps_frame*> of;        // per problem, nullptr = host arrays
  std::vector<ps_frame*> uniq;
  std::vector<FrameStageJob> jobs;  // problems with n > 0
  std::vector<float> grid;          // [nprob][4]
  bool all_staged = false;          // no problem needs its train arrays (or an empty grid) from the host: those bytes are not uploaded
  bool any() const { return !uniq.empty(); }
};

int frame_use_init(FrameUse& U, ps_matcher* m, ps_frame* const* frames, int nprob, const char* what) {
  U.of.assign(nprob, nullptr);
  U.grid.assign((size_t)nprob * 4, 0.f);
  if (!frames) return PS_OK;
  for (int p = 0; p < nprob; p++) {
    ps_frame* f = frames[p];
    if (!f) continue;
    if (f->device != m->device) return ps_set_error(PS_ERR_INVALID, "%s problem %d: the frame handle lives on another device", what, p);
    U.of[p] = f;
    U.uniq.push_back(f);
  }
  std::sort(U.uniq.begin(), U.uniq.end());
  U.uniq.erase(std::unique(U.uniq.begin(), U.uniq.end()), U.uniq.end());
  return PS_OK;
}

// train.n against the handle, and the handle's grid parameters
int frame_use_check(FrameUse& U, int p, int train_n, const char* what) {
  ps_frame* f = U.of[p];
  std::lock_guard<std::mutex> lock(f->mu);
  if (!f->published) return ps_set_error(PS_ERR_INVALID, "%s problem %d: the frame handle has never been published", what, p);
  if (train_n != f->n) return ps_set_error(PS_ERR_INVALID, "%s problem %d: train.n = %d, the frame handle holds %d keypoints", what, p, train_n, f->n);
  memcpy(&U.grid[(size_t)p * 4], f->grid, 16);
  return PS_OK;
}

// queues frame_stage behind the call's upload: the slabs' train sides land where the host arrays would have been uploaded
int frame_use_stage(FrameUse& U, ps_matcher* m, const FrameStageJob* d_jobs, const FrameStageDst& dst) {
  int rc = psf_consume_begin(U.uniq.data(), (int)U.uniq.size(), m->stream);
  if (rc != PS_OK) return rc;
  hipError_t e = hipSuccess;
  if (!U.jobs.empty()) {
    psk_frame_stage_launch(d_jobs, (int)U.jobs.size(), &dst, m->stream);
    e = hipGetLastError();
  }
  rc = psf_consume_end(U.uniq.data(), (int)U.uniq.size(), m, m->stream, !U.jobs.empty() && e == hipSuccess);
  if (e != hipSuccess) return ps_set_error(PS_ERR_HIP, "frame_stage: %s", hipGetErrorString(e));
  return rc;
}
}  // namespace

int psm_ensure(ps_matcher* m, size_t need) { return ensure(m, need); }

extern "C" {

int ps_matcher_create(int device, ps_matcher** out) {
  if (!out) return ps_set_error(PS_ERR_INVALID, "null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ps_set_error(PS_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return ps_set_error(PS_ERR_INVALID, "bad device ordinal");
  PS_HIP(hipSetDevice(device));
  ps_matcher* m = new ps_matcher();
  m->device = device;
  hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete m; return ps_set_error(PS_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
  hipEventCreate(&m->ev0); hipEventCreate(&m->ev1);
  *out = m;
  return PS_OK;
}

int ps_matcher_last_kernel_ms(const ps_matcher* m, float* ms) {
  if (!m || !ms) return ps_set_error(PS_ERR_INVALID, "null argument");
  *ms = m->last_kernel_ms;
  return PS_OK;
}

void ps_matcher_destroy(ps_matcher* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->ev0) hipEventDestroy(m->ev0);
  if (m->ev1) hipEventDestroy(m->ev1);
  if (m->stream) { hipStreamSynchronize(m->stream); hipStreamDestroy(m->stream); }
  if (m->d_buf) hipFree(m->d_buf);
  if (m->d_wide) hipFree(m->d_wide);
  if (m->h_buf) hipHostFree(m->h_buf);
  delete m;
}

int ps_hamming_matrix(ps_matcher* m, const uint8_t* q, int nq, const uint8_t* t, int nt, uint16_t* out) {
  if (!m || !q || !t || !out || nq < 1 || nt < 1) return ps_set_error(PS_ERR_INVALID, "ps_hamming_matrix: bad argument");
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  const size_t oq = 0, ot = al((size_t)nq * 32), oo = ot + al((size_t)nt * 32), total = oo + al((size_t)nq * nt * 2);
  int rc = ensure(m, total);
  if (rc != PS_OK) return rc;
  memcpy(m->h_buf + oq, q, (size_t)nq * 32);
  memcpy(m->h_buf + ot, t, (size_t)nt * 32);
  PS_HIP(hipMemcpyAsync(m->d_buf, m->h_buf, oo, hipMemcpyHostToDevice, m->stream));
  psk_hamming_matrix_launch(m->d_buf + oq, nq, m->d_buf + ot, nt, (uint16_t*)(m->d_buf + oo), m->stream);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(m->h_buf + oo, m->d_buf + oo, (size_t)nq * nt * 2, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  memcpy(out, m->h_buf + oo, (size_t)nq * nt * 2);
  return PS_OK;
}

int ps_match_bruteforce(ps_matcher* m, ps_bf_problem* probs, int nprob, float nn_ratio, int check_orientation) {
  if (!m || !probs || nprob < 1) return ps_set_error(PS_ERR_INVALID, "ps_match_bruteforce: bad argument");
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  size_t tq = 0, tt = 0;
  std::vector<BfProb> dp(nprob);
  std::vector<BfBlock> blocks;
  for (int p = 0; p < nprob; p++) {
    ps_bf_problem& P = probs[p];
    if (P.nq < 0 || P.nt < 0 || P.nt > PS_BF_MAX_TRAIN || (P.nq > 0 && (!P.q_desc || !P.q_angle || !P.q_valid)) ||
        (P.nt > 0 && (!P.t_desc || !P.t_angle || !P.query_of_train)))
      return ps_set_error(PS_ERR_INVALID, "brute-force problem %d: bad sizes or null pointers (nt <= %d)", p, PS_BF_MAX_TRAIN);
    dp[p] = BfProb{(int32_t)tq, P.nq, (int32_t)tt, P.nt};
    if (P.nt > 0)
      for (int q0 = 0; q0 < P.nq; q0 += PS_BF_QPB)
        blocks.push_back(BfBlock{p, q0, P.nq - q0 < PS_BF_QPB ? P.nq - q0 : PS_BF_QPB, 0});
    tq += P.nq;
    tt += P.nt;
  }
  // arena layout (host staging mirrors the device arena)
  size_t off = 0;
  const size_t o_prob = off; off += al(sizeof(BfProb) * nprob);
  const size_t o_blk = off;  off += al(sizeof(BfBlock) * (blocks.size() + 1));
  const size_t o_qd = off;   off += al(tq * 32 + 32);
  const size_t o_qa = off;   off += al(tq * 4 + 4);
  const size_t o_qv = off;   off += al(tq + 1);
  const size_t o_td = off;   off += al(tt * 32 + 32);
  const size_t o_ta = off;   off += al(tt * 4 + 4);
  const size_t in_bytes = off;
  const size_t o_out = off;  off += al(tt * 4 + 4);
  const size_t o_nm = off;   off += al((size_t)nprob * 4);
  const size_t out_bytes = off - o_out;
  const size_t o_topk = off; off += al(tq * PS_BF_TOPK * 4 + 4);
  int rc = ensure(m, off);
  if (rc != PS_OK) return rc;
  uint8_t* H = m->h_buf;
  memcpy(H + o_prob, dp.data(), sizeof(BfProb) * nprob);
  if (!blocks.empty()) memcpy(H + o_blk, blocks.data(), sizeof(BfBlock) * blocks.size());
  for (int p = 0; p < nprob; p++) {
    const ps_bf_problem& P = probs[p];
    if (P.nq > 0) {
      memcpy(H + o_qd + (size_t)dp[p].q_off * 32, P.q_desc, (size_t)P.nq * 32);
      memcpy(H + o_qa + (size_t)dp[p].q_off * 4, P.q_angle, (size_t)P.nq * 4);
      memcpy(H + o_qv + (size_t)dp[p].q_off, P.q_valid, (size_t)P.nq);
    }
    if (P.nt > 0) {
      memcpy(H + o_td + (size_t)dp[p].t_off * 32, P.t_desc, (size_t)P.nt * 32);
      memcpy(H + o_ta + (size_t)dp[p].t_off * 4, P.t_angle, (size_t)P.nt * 4);
    }
  }
  uint8_t* D = m->d_buf;
  PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
  hipEventRecord(m->ev0, m->stream);
  psk_bf_launch((const BfBlock*)(D + o_blk), (int)blocks.size(), (const BfProb*)(D + o_prob), nprob, D + o_qd,
                (const float*)(D + o_qa), D + o_qv, D + o_td, (const float*)(D + o_ta), (uint32_t*)(D + o_topk),
                (int32_t*)(D + o_out), (int32_t*)(D + o_nm), nn_ratio, check_orientation, m->stream);
  hipEventRecord(m->ev1, m->stream);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(H + o_out, D + o_out, out_bytes, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  hipEventElapsedTime(&m->last_kernel_ms, m->ev0, m->ev1);
  for (int p = 0; p < nprob; p++) {
    ps_bf_problem& P = probs[p];
    if (P.nt > 0) memcpy(P.query_of_train, H + o_out + (size_t)dp[p].t_off * 4, (size_t)P.nt * 4);
    P.nmatches = ((const int32_t*)(H + o_nm))[p];
  }
  return PS_OK;
}


// The three ORBmatcher::SearchByProjection overloads (see include/pointslot_hip.h for the field mapping).  frames: nullptr, or per
// problem the frame handle its train side comes from (ps_search_by_projection_frames).
static int search_by_projection(ps_matcher* m, ps_proj_problem* probs, ps_frame* const* frames, int nprob) {
  if (!m || !probs || nprob < 1) return ps_set_error(PS_ERR_INVALID, "ps_search_by_projection: bad argument");
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  FrameUse U;
  int frc = frame_use_init(U, m, frames, nprob, "projection");
  if (frc != PS_OK) return frc;
  size_t NT = 0, NQ = 0;
  int max_nq = 0, max_nt = 0, any_frame = 0;
  const int NCELL = PS_GRID_COLS * PS_GRID_ROWS;
  for (int p = 0; p < nprob; p++) {
    const ps_proj_problem& P = probs[p];
    const ps_proj_train& T = P.train;
    if (U.of[p]) {
      if (T.n < 0 || P.nq < 0 || (T.n > 0 && (!T.occupied || !P.match_of_train)))
        return ps_set_error(PS_ERR_INVALID, "projection problem %d: bad train side (occupied and match_of_train stay host arrays)", p);
      if ((frc = frame_use_check(U, p, T.n, "projection")) != PS_OK) return frc;
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
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += al(bytes + 64); return r; };
  const size_t o_prob = take(sizeof(PjProb) * nprob);
  const size_t o_tx = take(NT * 4), o_ty = take(NT * 4), o_toct = take(NT * 4), o_tang = take(NT * 4), o_tur = take(NT * 4);
  const size_t o_tdesc = take(NT * 32), o_tocc = take(NT), o_tbb = take(NT), o_coff = take((size_t)nprob * (NCELL + 1) * 4), o_cidx = take(NT * 4);
  const size_t o_qvalid = take(NQ), o_qu = take(NQ * 4), o_qv = take(NQ * 4), o_qur = take(NQ * 4), o_qrad = take(NQ * 4), o_qrer = take(NQ * 4);
  const size_t o_qminl = take(NQ * 4), o_qmaxl = take(NQ * 4), o_qdesc = take(NQ * 32), o_qobs = take(NQ), o_qang = take(NQ * 4);
  const size_t o_qxw = take(NQ * 12), o_qoct = take(NQ * 4);
  // (the two frame-handle slots exist only in a call that uses one: the layout of every other call is what it was)
  const size_t o_jobs = U.any() ? take(sizeof(FrameStageJob) * nprob) : 0;
  const size_t in_bytes = off;
  const size_t o_match = take(NT * 4), o_nm = take((size_t)nprob * 4), o_ovf = take((size_t)nprob * 4);
  const size_t o_fst = U.any() ? take((size_t)nprob * 4) : 0;
  const size_t out_end = off;
  const size_t o_cand = take(NQ * PS_PJ_CAP * 4), o_ncand = take(NQ * 4), o_qbest = take(NQ * 4), o_qbin = take(NQ), o_tt = take(NQ * 16);
  int rc = ensure(m, off);
  if (rc != PS_OK) return rc;
  uint8_t* H = m->h_buf;
  static const bool prof = getenv("PS_MATCH_PROFILE") != nullptr;   // developer switch: host-side breakdown of the call on stderr
  const auto tp0 = std::chrono::steady_clock::now();
  PjProb* hp = (PjProb*)(H + o_prob);
  std::vector<size_t> toff(nprob), qoff(nprob);
  {
    size_t t0 = 0, q0 = 0;
    for (int p = 0; p < nprob; p++) { toff[p] = t0; qoff[p] = q0; t0 += probs[p].train.n; q0 += probs[p].nq; }
  }
  if (U.any()) {
    U.all_staged = true;
    for (int p = 0; p < nprob; p++) {
      if (U.of[p] && probs[p].train.n > 0)
        U.jobs.push_back(FrameStageJob{U.of[p]->slab, probs[p].train.n, (int32_t)toff[p], p * (NCELL + 1), p});
      else
        U.all_staged = false;
    }
    memset(H + o_jobs, 0, sizeof(FrameStageJob) * nprob);
    if (!U.jobs.empty()) memcpy(H + o_jobs, U.jobs.data(), sizeof(FrameStageJob) * U.jobs.size());
  }
  // every problem fills (or zeroes) exactly its own slices of the staging buffer: independent, memcpy-bound
  ps_parallel_for(nprob, in_bytes, [&](int p) {
    const ps_proj_problem& P = probs[p];
    const ps_proj_train& T = P.train;
    const size_t t0 = toff[p], q0 = qoff[p];
    PjProb& d = hp[p];
    memset(&d, 0, sizeof(d));
    d.t_off = (int32_t)t0; d.nt = T.n; d.q_off = (int32_t)q0; d.c_off = (int32_t)q0; d.nq = P.nq; d.grid_off = p * (NCELL + 1);
    d.min_x = T.min_x; d.min_y = T.min_y; d.gw_inv = T.grid_w_inv; d.gh_inv = T.grid_h_inv;
    if (U.of[p]) { const float* g = &U.grid[(size_t)p * 4]; d.min_x = g[0]; d.min_y = g[1]; d.gw_inv = g[2]; d.gh_inv = g[3]; }
    d.th_dist = P.th_dist; d.ratio_test = P.ratio_test; d.nn_ratio = P.nn_ratio; d.check_ori = P.check_orientation;
    d.use_bbox = P.use_bbox; d.frame_mode = P.frame_mode;
    memcpy(d.tcw, P.tcw, 64); memcpy(d.tlw, P.tlw, 64);
    d.fx = P.fx; d.fy = P.fy; d.cx = P.cx; d.cy = P.cy; d.mbf = P.mbf; d.mb = P.mb;
    memcpy(d.bounds, P.bounds, 16); memcpy(d.scale, P.scale_factors, 32);
    d.th = P.th; d.mono = P.mono;
    if (T.n > 0 && U.of[p]) {   // x .. desc and the grid are staged on the device (frame_stage)
      const size_t n = (size_t)T.n;
      memcpy(H + o_tocc + t0, T.occupied, n);
      if (T.in_bbox) memcpy(H + o_tbb + t0, T.in_bbox, n); else memset(H + o_tbb + t0, 0, n);
    } else if (T.n > 0) {
      const size_t n = (size_t)T.n, filled = (size_t)T.cell_off[NCELL];
      memcpy(H + o_tx + t0 * 4, T.x, n * 4); memcpy(H + o_ty + t0 * 4, T.y, n * 4);
      memcpy(H + o_toct + t0 * 4, T.octave, n * 4); memcpy(H + o_tang + t0 * 4, T.angle, n * 4);
      memcpy(H + o_tur + t0 * 4, T.u_right, n * 4); memcpy(H + o_tdesc + t0 * 32, T.desc, n * 32);
      memcpy(H + o_tocc + t0, T.occupied, n);
      if (T.in_bbox) memcpy(H + o_tbb + t0, T.in_bbox, n); else memset(H + o_tbb + t0, 0, n);
      memcpy(H + o_coff + (size_t)d.grid_off * 4, T.cell_off, (size_t)(NCELL + 1) * 4);
      memcpy(H + o_cidx + t0 * 4, T.cell_idx, std::min(filled, n) * 4);
      if (filled < n) memset(H + o_cidx + (t0 + filled) * 4, 0, (n - filled) * 4);
    } else {
      memset(H + o_coff + (size_t)d.grid_off * 4, 0, (size_t)(NCELL + 1) * 4);
    }
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
  if (U.all_staged) {   // everything but the train arrays and the grids
    PS_HIP(hipMemcpyAsync(D, H, o_tx, hipMemcpyHostToDevice, m->stream));
    PS_HIP(hipMemcpyAsync(D + o_tocc, H + o_tocc, o_coff - o_tocc, hipMemcpyHostToDevice, m->stream));
    PS_HIP(hipMemcpyAsync(D + o_qvalid, H + o_qvalid, in_bytes - o_qvalid, hipMemcpyHostToDevice, m->stream));
  } else {
    PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
  }
  if (U.any()) {
    FrameStageDst dst{(float*)(D + o_tx), (float*)(D + o_ty), (int32_t*)(D + o_toct), (float*)(D + o_tang), (float*)(D + o_tur), D + o_tdesc,
                      (int32_t*)(D + o_coff), (int32_t*)(D + o_cidx), (int32_t*)(D + o_fst)};
    PS_HIP(hipMemsetAsync(D + o_fst, 0, (size_t)nprob * 4, m->stream));
    if ((frc = frame_use_stage(U, m, (const FrameStageJob*)(D + o_jobs), dst)) != PS_OK) return frc;
  }
  if (prof) PS_HIP(hipStreamSynchronize(m->stream));
  const auto tp2 = std::chrono::steady_clock::now();
  PS_HIP(hipMemsetAsync(D + o_ovf, 0, (size_t)nprob * 4, m->stream));
  PjArrays A;
  A.prob = (const PjProb*)(D + o_prob);
  A.tx = (const float*)(D + o_tx); A.ty = (const float*)(D + o_ty); A.toct = (const int32_t*)(D + o_toct);
  A.tang = (const float*)(D + o_tang); A.tur = (const float*)(D + o_tur); A.tdesc = D + o_tdesc; A.tocc = D + o_tocc;
  A.tbbox = D + o_tbb; A.cell_off = (const int32_t*)(D + o_coff); A.cell_idx = (const int32_t*)(D + o_cidx);
  A.qvalid = D + o_qvalid; A.qu = (float*)(D + o_qu); A.qv = (float*)(D + o_qv); A.qur = (float*)(D + o_qur);
  A.qrad = (float*)(D + o_qrad); A.qrer = (float*)(D + o_qrer); A.qminl = (int32_t*)(D + o_qminl); A.qmaxl = (int32_t*)(D + o_qmaxl);
  A.qdesc = D + o_qdesc; A.qobs = D + o_qobs; A.qang = (const float*)(D + o_qang);
  A.qxw = (const float*)(D + o_qxw); A.qoct = (const int32_t*)(D + o_qoct);
  A.cand = (uint32_t*)(D + o_cand); A.ncand = (int32_t*)(D + o_ncand); A.match = (int32_t*)(D + o_match);
  A.nmatch = (int32_t*)(D + o_nm); A.overflow = (int32_t*)(D + o_ovf); A.qbest = (int32_t*)(D + o_qbest); A.qbin = D + o_qbin;
  A.ttop = (uint4*)(D + o_tt);
  hipEventRecord(m->ev0, m->stream);
  psk_pj_launch(&A, nprob, max_nq > 0 ? max_nq : 1, max_nt, any_frame, 0, m->stream);
  hipEventRecord(m->ev1, m->stream);
  PS_HIP(hipGetLastError());
  if (prof) PS_HIP(hipStreamSynchronize(m->stream));
  const auto tp3 = std::chrono::steady_clock::now();
  PS_HIP(hipMemcpyAsync(H + o_match, D + o_match, out_end - o_match, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  hipEventElapsedTime(&m->last_kernel_ms, m->ev0, m->ev1);
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
  const int32_t* ovf = (const int32_t*)(H + o_ovf);
  std::vector<int> wide, failed, stale;
  if (U.any())
    for (int p = 0; p < nprob; p++)
      if (((const int32_t*)(H + o_fst))[p]) stale.push_back(p);
  for (int p = 0; p < nprob; p++)
    if (ovf[p] > 0 && std::find(stale.begin(), stale.end(), p) == stale.end()) (probs[p].train.n <= PS_PJ_WIDE_MAX_N ? wide : failed).push_back(p);
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
    size_t woff = 0;
    auto wtake = [&](size_t bytes) { size_t r = woff; woff += al(bytes + 64); return r; };
    const size_t w_prob = wtake(sizeof(PjProb) * sub.size()), w_nm = wtake(sub.size() * 4), w_ovf = wtake(sub.size() * 4), w_cand = wtake(nq2 * PS_PJ_CAP_WIDE * 4);
    if (woff > m->d_wide_bytes) {
      if (m->d_wide) hipFree(m->d_wide);
      m->d_wide = nullptr; m->d_wide_bytes = 0;
      PS_HIP(hipMalloc(&m->d_wide, woff));
      m->d_wide_bytes = woff;
    }
    uint8_t* Wd = m->d_wide;
    PS_HIP(hipMemcpyAsync(Wd + w_prob, sub.data(), sizeof(PjProb) * sub.size(), hipMemcpyHostToDevice, m->stream));
    PS_HIP(hipMemsetAsync(Wd + w_ovf, 0, sub.size() * 4, m->stream));
    // (pj_project runs again on these problems: it only repeats what it wrote; the queries it invalidated stay invalid)
    PjArrays A2 = A;
    A2.prob = (const PjProb*)(Wd + w_prob); A2.cand = (uint32_t*)(Wd + w_cand); A2.nmatch = (int32_t*)(Wd + w_nm); A2.overflow = (int32_t*)(Wd + w_ovf);
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
    P.nmatches = ((const int32_t*)(H + o_nm))[p];
  }
  for (size_t i = 0; i < wide.size(); i++)
    if (wide_nm[i] >= 0) probs[wide[i]].nmatches = wide_nm[i];
  if (!stale.empty())
    return ps_set_error(PS_ERR_INVALID, "projection problem %d (and %zu more): the frame handle does not hold the %d keypoints it was published with "
                        "(the extractor's count differed from the n given to ps_frame_publish_orb)", stale[0], stale.size() - 1, probs[stale[0]].train.n);
  if (!failed.empty())
    return ps_set_error(PS_ERR_CAPACITY, "projection problem %d (and %zu more): a search window held more than %d candidates%s", failed[0], failed.size() - 1,
                        probs[failed[0]].train.n <= PS_PJ_WIDE_MAX_N ? PS_PJ_CAP_WIDE : PS_PJ_CAP,
                        probs[failed[0]].train.n <= PS_PJ_WIDE_MAX_N ? "" : " and the frame has more features than the wide candidate store indexes (8191)");
  return PS_OK;
}


int ps_search_by_projection(ps_matcher* m, ps_proj_problem* probs, int nprob) { return search_by_projection(m, probs, nullptr, nprob); }

int ps_search_by_projection_frames(ps_matcher* m, ps_proj_problem* probs, ps_frame* const* frames, int nprob) {
  return search_by_projection(m, probs, frames, nprob);
}


int ps_distinctive_descriptors(ps_matcher* m, const uint8_t* desc, const int32_t* off, int npoints, int32_t* best) {
  if (!m || !off || !best || npoints < 1) return ps_set_error(PS_ERR_INVALID, "ps_distinctive_descriptors: bad argument");
  const int total = off[npoints];
  if (total > 0 && !desc) return ps_set_error(PS_ERR_INVALID, "null descriptors");
  for (int p = 0; p < npoints; p++)
    if (off[p + 1] < off[p] || off[p + 1] - off[p] > 128) return ps_set_error(PS_ERR_CAPACITY, "point %d: 0..128 observations supported", p);
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  const size_t o_desc = 0, o_off = al((size_t)total * 32 + 32), o_best = o_off + al((size_t)(npoints + 1) * 4), end = o_best + al((size_t)npoints * 4);
  int rc = ensure(m, end);
  if (rc != PS_OK) return rc;
  if (total > 0) memcpy(m->h_buf + o_desc, desc, (size_t)total * 32);
  memcpy(m->h_buf + o_off, off, (size_t)(npoints + 1) * 4);
  PS_HIP(hipMemcpyAsync(m->d_buf, m->h_buf, o_best, hipMemcpyHostToDevice, m->stream));
  psk_distinctive_launch(m->d_buf + o_desc, (const int32_t*)(m->d_buf + o_off), (int32_t*)(m->d_buf + o_best), npoints, m->stream);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(m->h_buf + o_best, m->d_buf + o_best, (size_t)npoints * 4, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  memcpy(best, m->h_buf + o_best, (size_t)npoints * 4);
  return PS_OK;
}


static int fuse_search(ps_matcher* m, ps_fuse_problem* probs, ps_frame* const* frames, int nprob) {
  if (!m || !probs || nprob < 1) return ps_set_error(PS_ERR_INVALID, "ps_fuse_search: bad argument");
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  FrameUse U;
  int frc = frame_use_init(U, m, frames, nprob, "fuse");
  if (frc != PS_OK) return frc;
  size_t NT = 0, NQ = 0;
  int max_nq = 0;
  const int NCELL = PS_GRID_COLS * PS_GRID_ROWS;
  for (int p = 0; p < nprob; p++) {
    const ps_fuse_problem& P = probs[p];
    const ps_proj_train& T = P.train;
    if (U.of[p]) {
      if (T.n < 0 || P.nq < 0) return ps_set_error(PS_ERR_INVALID, "fuse problem %d: bad keyframe side", p);
      if ((frc = frame_use_check(U, p, T.n, "fuse")) != PS_OK) return frc;
    } else if (T.n < 0 || P.nq < 0 || (T.n > 0 && (!T.x || !T.y || !T.octave || !T.u_right || !T.desc || !T.cell_off || !T.cell_idx)))
      return ps_set_error(PS_ERR_INVALID, "fuse problem %d: bad keyframe side", p);
    if (P.nq > 0 && (!P.q_valid || !P.q_pos || !P.q_normal || !P.q_min_dist || !P.q_max_dist || !P.q_desc || !P.best_idx || !P.best_dist))
      return ps_set_error(PS_ERR_INVALID, "fuse problem %d: null query arrays", p);
    if (P.n_levels < 1 || P.n_levels > 8) return ps_set_error(PS_ERR_INVALID, "fuse problem %d: n_levels must be 1..8", p);
    NT += T.n; NQ += P.nq;
    max_nq = P.nq > max_nq ? P.nq : max_nq;
  }
  if (NQ == 0) return PS_OK;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += al(bytes + 64); return r; };
  const size_t o_prob = take(sizeof(FuProb) * nprob);
  const size_t o_tx = take(NT * 4), o_ty = take(NT * 4), o_toct = take(NT * 4), o_tur = take(NT * 4), o_tdesc = take(NT * 32);
  const size_t o_coff = take((size_t)nprob * (NCELL + 1) * 4), o_cidx = take(NT * 4);
  const size_t o_qvalid = take(NQ), o_qpos = take(NQ * 12), o_qnor = take(NQ * 12), o_qmin = take(NQ * 4), o_qmax = take(NQ * 4), o_qdesc = take(NQ * 32);
  const size_t o_jobs = U.any() ? take(sizeof(FrameStageJob) * nprob) : 0;
  const size_t in_bytes = off;
  const size_t o_bi = take(NQ * 4), o_bd = take(NQ * 4);
  const size_t o_fst = U.any() ? take((size_t)nprob * 4) : 0;
  int rc = ensure(m, off);
  if (rc != PS_OK) return rc;
  uint8_t* H = m->h_buf;
  memset(H, 0, in_bytes);
  U.all_staged = U.any();
  FuProb* hp = (FuProb*)(H + o_prob);
  size_t t0 = 0, q0 = 0;
  for (int p = 0; p < nprob; p++) {
    const ps_fuse_problem& P = probs[p];
    const ps_proj_train& T = P.train;
    FuProb& d = hp[p];
    d.t_off = (int32_t)t0; d.nt = T.n; d.q_off = (int32_t)q0; d.nq = P.nq; d.grid_off = p * (NCELL + 1);
    d.min_x = T.min_x; d.min_y = T.min_y; d.gw_inv = T.grid_w_inv; d.gh_inv = T.grid_h_inv;
    if (U.of[p]) { const float* g = &U.grid[(size_t)p * 4]; d.min_x = g[0]; d.min_y = g[1]; d.gw_inv = g[2]; d.gh_inv = g[3]; }
    memcpy(d.R, P.rcw, 36); memcpy(d.t, P.tcw, 12); memcpy(d.ow, P.ow, 12);
    d.fx = P.fx; d.fy = P.fy; d.cx = P.cx; d.cy = P.cy; d.bf = P.bf;
    memcpy(d.bounds, P.bounds, 32); memcpy(d.scale, P.scale_factors, 32); memcpy(d.inv_sigma2, P.inv_level_sigma2, 32);
    d.log_scale = P.log_scale_factor; d.n_levels = P.n_levels; d.th = P.th;
    if (U.of[p] && T.n > 0) {   // staged on the device (frame_stage)
      U.jobs.push_back(FrameStageJob{U.of[p]->slab, T.n, (int32_t)t0, p * (NCELL + 1), p});
    } else if (U.any()) {
      U.all_staged = false;
    }
    if (T.n > 0 && !U.of[p]) {
      memcpy(H + o_tx + t0 * 4, T.x, (size_t)T.n * 4); memcpy(H + o_ty + t0 * 4, T.y, (size_t)T.n * 4);
      memcpy(H + o_toct + t0 * 4, T.octave, (size_t)T.n * 4); memcpy(H + o_tur + t0 * 4, T.u_right, (size_t)T.n * 4);
      memcpy(H + o_tdesc + t0 * 32, T.desc, (size_t)T.n * 32);
      memcpy(H + o_cidx + t0 * 4, T.cell_idx, (size_t)T.cell_off[NCELL] * 4);
    }
    if (T.cell_off && !U.of[p]) memcpy(H + o_coff + (size_t)d.grid_off * 4, T.cell_off, (size_t)(NCELL + 1) * 4);
    if (P.nq > 0) {
      memcpy(H + o_qvalid + q0, P.q_valid, P.nq); memcpy(H + o_qpos + q0 * 12, P.q_pos, (size_t)P.nq * 12);
      memcpy(H + o_qnor + q0 * 12, P.q_normal, (size_t)P.nq * 12); memcpy(H + o_qmin + q0 * 4, P.q_min_dist, (size_t)P.nq * 4);
      memcpy(H + o_qmax + q0 * 4, P.q_max_dist, (size_t)P.nq * 4); memcpy(H + o_qdesc + q0 * 32, P.q_desc, (size_t)P.nq * 32);
    }
    t0 += T.n; q0 += P.nq;
  }
  uint8_t* D = m->d_buf;
  if (U.any() && !U.jobs.empty()) memcpy(H + o_jobs, U.jobs.data(), sizeof(FrameStageJob) * U.jobs.size());
  if (U.all_staged) {   // everything but the keyframe arrays and the grids
    PS_HIP(hipMemcpyAsync(D, H, o_tx, hipMemcpyHostToDevice, m->stream));
    PS_HIP(hipMemcpyAsync(D + o_qvalid, H + o_qvalid, in_bytes - o_qvalid, hipMemcpyHostToDevice, m->stream));
  } else {
    PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
  }
  if (U.any()) {
    FrameStageDst dst{(float*)(D + o_tx), (float*)(D + o_ty), (int32_t*)(D + o_toct), nullptr, (float*)(D + o_tur), D + o_tdesc,
                      (int32_t*)(D + o_coff), (int32_t*)(D + o_cidx), (int32_t*)(D + o_fst)};
    PS_HIP(hipMemsetAsync(D + o_fst, 0, (size_t)nprob * 4, m->stream));
    if ((frc = frame_use_stage(U, m, (const FrameStageJob*)(D + o_jobs), dst)) != PS_OK) return frc;
  }
  FuArrays A;
  A.prob = (const FuProb*)(D + o_prob);
  A.tx = (const float*)(D + o_tx); A.ty = (const float*)(D + o_ty); A.toct = (const int32_t*)(D + o_toct); A.tur = (const float*)(D + o_tur);
  A.tdesc = D + o_tdesc; A.cell_off = (const int32_t*)(D + o_coff); A.cell_idx = (const int32_t*)(D + o_cidx);
  A.qvalid = D + o_qvalid; A.qpos = (const float*)(D + o_qpos); A.qnormal = (const float*)(D + o_qnor); A.qmin = (const float*)(D + o_qmin);
  A.qmax = (const float*)(D + o_qmax); A.qdesc = D + o_qdesc; A.best_idx = (int32_t*)(D + o_bi); A.best_dist = (int32_t*)(D + o_bd);
  psk_fuse_launch(&A, nprob, max_nq, m->stream);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(H + o_bi, D + o_bi, off - o_bi, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  q0 = 0;
  int stale = -1;
  for (int p = 0; p < nprob; p++) {
    ps_fuse_problem& P = probs[p];
    if (U.any() && ((const int32_t*)(H + o_fst))[p]) {   // its outputs stay as the caller left them
      stale = stale < 0 ? p : stale;
    } else if (P.nq > 0) {
      memcpy(P.best_idx, H + o_bi + q0 * 4, (size_t)P.nq * 4);
      memcpy(P.best_dist, H + o_bd + q0 * 4, (size_t)P.nq * 4);
    }
    q0 += P.nq;
  }
  if (stale >= 0)
    return ps_set_error(PS_ERR_INVALID, "fuse problem %d: the frame handle does not hold the %d keypoints it was published with "
                        "(the extractor's count differed from the n given to ps_frame_publish_orb)", stale, probs[stale].train.n);
  return PS_OK;
}

int ps_fuse_search(ps_matcher* m, ps_fuse_problem* probs, int nprob) { return fuse_search(m, probs, nullptr, nprob); }

int ps_fuse_search_frames(ps_matcher* m, ps_fuse_problem* probs, ps_frame* const* frames, int nprob) {
  return fuse_search(m, probs, frames, nprob);
}


// ---- LocalMapping::CreateNewMapPoints: SearchForTriangulation against every neighbour + the triangulation gates ----
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
struct TriOff { size_t x, y, oct, ang, ur, depth, xraw, yraw, desc, occ; };
// the feature arrays of one keyframe into its slices of the staging buffer (skip_keys: x .. desc are staged on the device)
void tri_pack_kf(uint8_t* H, const TriOff& o, const ps_tri_keyframe& K, const TriKf& d, bool skip_keys) {
  const size_t n = (size_t)K.n, f = (size_t)d.f_off;
  if (n == 0) return;
  if (!skip_keys) {
    memcpy(H + o.x + f * 4, K.x, n * 4); memcpy(H + o.y + f * 4, K.y, n * 4); memcpy(H + o.oct + f * 4, K.octave, n * 4);
    memcpy(H + o.ang + f * 4, K.angle, n * 4); memcpy(H + o.ur + f * 4, K.u_right, n * 4); memcpy(H + o.desc + f * 32, K.desc, n * 32);
  }
  memcpy(H + o.depth + f * 4, K.depth, n * 4); memcpy(H + o.occ + f, K.occupied, n);
  if (d.raw_off >= 0) { memcpy(H + o.xraw + (size_t)d.raw_off * 4, K.x_raw, n * 4); memcpy(H + o.yraw + (size_t)d.raw_off * 4, K.y_raw, n * 4); }
}
}  // namespace

static int create_new_map_points(ps_matcher* m, ps_tri_problem* probs, ps_frame* const* frames, int nprob) {
  if (!m || !probs || nprob < 1) return ps_set_error(PS_ERR_INVALID, "ps_create_new_map_points: bad argument");
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  FrameUse U;
  int frc = frame_use_init(U, m, frames, nprob, "triangulation");
  if (frc != PS_OK) return frc;
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
    if (U.of[p] && (frc = frame_use_check(U, p, P.kf1.n, "triangulation")) != PS_OK) return frc;
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
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += al(bytes + 64); return r; };
  const size_t o_prob = take(sizeof(TriProb) * ns), o_pair = take(sizeof(TriPair) * npairs), o_kf = take(sizeof(TriKf) * nkf);
  TriOff O;
  O.x = take(NF * 4); O.y = take(NF * 4); O.oct = take(NF * 4); O.ang = take(NF * 4); O.ur = take(NF * 4); O.depth = take(NF * 4);
  O.xraw = take(NR * 4); O.yraw = take(NR * 4); O.desc = take(NF * 32); O.occ = take(NF);
  const size_t o_aux = take(NF * 4), o_noff = take(NN * 4);
  const size_t o_jobs = U.any() ? take(sizeof(FrameStageJob) * ns) : 0;
  const size_t in_bytes = off;
  const size_t o_match = take(NO * 4), o_nm = take(npairs * 4), o_nnew = take((size_t)ns * 4);
  const size_t o_fst = U.any() ? take((size_t)ns * 4) : 0;
  const size_t o_status = take(any_tri ? NO : 0), o_x3d = take(any_tri ? NO * 12 : 0);
  const size_t out_end = off;
  int rc = ensure(m, off);
  if (rc != PS_OK) return rc;
  uint8_t* H = m->h_buf;
  memcpy(H + o_prob, hp.data(), sizeof(TriProb) * ns);
  if (npairs) memcpy(H + o_pair, hr.data(), sizeof(TriPair) * npairs);
  memcpy(H + o_kf, hk.data(), sizeof(TriKf) * nkf);
  if (U.any()) {
    for (int s = 0; s < ns; s++)
      if (U.of[served[s]] && hp[s].n1 > 0 && hp[s].k > 0)
        U.jobs.push_back(FrameStageJob{U.of[served[s]]->slab, hp[s].n1, hk[(size_t)kf_first[s]].f_off, 0, s});
    memset(H + o_jobs, 0, sizeof(FrameStageJob) * ns);
    if (!U.jobs.empty()) memcpy(H + o_jobs, U.jobs.data(), sizeof(FrameStageJob) * U.jobs.size());
  }
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
  PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
  hipEventRecord(m->ev0, m->stream);   // (the staging copy of frame-backed keyframes counts as kernel time of the call)
  if (U.any()) {
    FrameStageDst dst{(float*)(D + O.x), (float*)(D + O.y), (int32_t*)(D + O.oct), (float*)(D + O.ang), (float*)(D + O.ur), D + O.desc,
                      nullptr, nullptr, (int32_t*)(D + o_fst)};
    PS_HIP(hipMemsetAsync(D + o_fst, 0, (size_t)ns * 4, m->stream));
    if ((frc = frame_use_stage(U, m, (const FrameStageJob*)(D + o_jobs), dst)) != PS_OK) return frc;
  }
  TriArrays A;
  A.prob = (const TriProb*)(D + o_prob); A.pair = (const TriPair*)(D + o_pair); A.kf = (const TriKf*)(D + o_kf);
  A.x = (const float*)(D + O.x); A.y = (const float*)(D + O.y); A.oct = (const int32_t*)(D + O.oct); A.ang = (const float*)(D + O.ang);
  A.ur = (const float*)(D + O.ur); A.depth = (const float*)(D + O.depth); A.xraw = (const float*)(D + O.xraw); A.yraw = (const float*)(D + O.yraw);
  A.desc = D + O.desc; A.occ = D + O.occ; A.aux = (const int32_t*)(D + o_aux); A.node_off = (const int32_t*)(D + o_noff);
  A.match = (int32_t*)(D + o_match); A.nmatch = (int32_t*)(D + o_nm); A.x3d = (float*)(D + o_x3d); A.status = D + o_status; A.nnew = (int32_t*)(D + o_nnew);
  psk_tri_launch(&A, ns, (int)npairs, max_n1, m->stream);
  hipEventRecord(m->ev1, m->stream);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(H + o_match, D + o_match, out_end - o_match, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  hipEventElapsedTime(&m->last_kernel_ms, m->ev0, m->ev1);
  int stale = -1;
  for (int s = 0; s < ns; s++) {
    ps_tri_problem& P = probs[served[s]];
    if (U.any() && ((const int32_t*)(H + o_fst))[s]) { stale = stale < 0 ? served[s] : stale; continue; }   // its outputs stay as the caller left them
    *P.nnew = ((const int32_t*)(H + o_nnew))[s];
    if (P.k == 0) continue;
    memcpy(P.nmatches, H + o_nm + (size_t)hp[s].first_pair * 4, (size_t)P.k * 4);
    const size_t o0 = (size_t)hr[(size_t)hp[s].first_pair].out_off, cnt = (size_t)P.k * (size_t)P.kf1.n;
    if (cnt == 0) continue;
    memcpy(P.match, H + o_match + o0 * 4, cnt * 4);
    if (P.triangulate) { memcpy(P.status, H + o_status + o0, cnt); memcpy(P.x3d, H + o_x3d + o0 * 12, cnt * 12); }
  }
  if (stale >= 0)
    return ps_set_error(PS_ERR_INVALID, "triangulation problem %d: the frame handle does not hold the %d keypoints it was published with "
                        "(the extractor's count differed from the n given to ps_frame_publish_orb)", stale, probs[stale].kf1.n);
  if (!failed.empty())
    return ps_set_error(PS_ERR_CAPACITY, "triangulation problem %d (and %zu more): more than %d features in a keyframe or more than %d neighbours", failed[0],
                        failed.size() - 1, PS_TRI_MAX_N, PS_TRI_MAX_K);
  return PS_OK;
}

int ps_create_new_map_points(ps_matcher* m, ps_tri_problem* probs, int nprob) { return create_new_map_points(m, probs, nullptr, nprob); }

int ps_create_new_map_points_frames(ps_matcher* m, ps_tri_problem* probs, ps_frame* const* kf1_frames, int nprob) {
  return create_new_map_points(m, probs, kf1_frames, nprob);
}

}  // extern "C"

// ---- The loop-closure and relocalisation projection matchers: ps_kf_search, ps_search_by_sim3 (kfsearch_kernels.hip) ----
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
  const int NCELL = PS_GRID_COLS * PS_GRID_ROWS;
  std::vector<ps_frame*> fr(nj, nullptr);
  for (int j = 0; j < nj; j++) fr[j] = jobs[j].skip ? nullptr : jobs[j].frame;
  FrameUse U;
  int frc = frame_use_init(U, m, fr.data(), nj, what);
  if (frc != PS_OK) return frc;
  size_t NT = 0, NQ = 0, NQO = 0;
  int max_nq = 1, any_ordered = 0;
  for (int j = 0; j < nj; j++) {
    KsHostJob& J = jobs[j];
    J.t_off = NT; J.q_off = NQ;
    if (J.skip) continue;
    if (U.of[j] && (frc = frame_use_check(U, j, J.T->n, what)) != PS_OK) return frc;
    NT += J.T->n; NQ += J.nq;
    if (ks_ordered(J.kind)) { NQO += J.nq; any_ordered = 1; }
    max_nq = std::max(max_nq, J.nq);
  }
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += al(bytes + 64); return r; };
  const size_t o_job = take(sizeof(KsJob) * nj), o_pair = take(sizeof(KsPair) * (npair > 0 ? npair : 1));
  const size_t o_tx = take(NT * 4), o_ty = take(NT * 4), o_toct = take(NT * 4), o_tang = take(NT * 4), o_tur = take(NT * 4), o_tdesc = take(NT * 32);
  const size_t o_coff = take((size_t)nj * (NCELL + 1) * 4), o_cidx = take(NT * 4);
  const size_t o_tocc = take(NT);
  const size_t o_qvalid = take(NQ), o_qpos = take(NQ * 12), o_qnor = take(NQ * 12), o_qmin = take(NQ * 4), o_qmax = take(NQ * 4), o_qdesc = take(NQ * 32);
  const size_t o_qang = take(NQ * 4);
  const size_t o_fjobs = U.any() ? take(sizeof(FrameStageJob) * nj) : 0;
  const size_t in_bytes = off;
  const size_t o_bi = take(NQ * 4), o_bd = take(NQ * 4), o_match = take(NT * 4), o_m12 = take(NQ * 4), o_nm = take((size_t)nj * 4), o_ovf = take((size_t)nj * 4);
  const size_t o_nf = take((size_t)(npair > 0 ? npair : 1) * 4), o_fst = take((size_t)nj * 4);
  const size_t out_end = off;
  const size_t o_cand = take(NQO * PS_KS_CAP * 4), o_ncand = take(NQ * 4), o_qtop = take(NQ * 4);
  int rc = ensure(m, off);
  if (rc != PS_OK) return rc;
  uint8_t* H = m->h_buf;
  uint8_t* D = m->d_buf;
  memset(H, 0, in_bytes);
  memset(H + o_fst, 0, (size_t)nj * 4);
  KsJob* hj = (KsJob*)(H + o_job);
  size_t c0 = 0;
  U.all_staged = U.any();
  for (int j = 0; j < nj; j++) {
    const KsHostJob& J = jobs[j];
    KsJob& d = hj[j];
    d.kind = J.kind; d.grid_off = j * (NCELL + 1); d.t_off = (int32_t)J.t_off; d.q_off = (int32_t)J.q_off; d.cap = PS_KS_CAP;
    if (J.skip) continue;               // nt = nq = 0: nothing is launched for it
    const ps_proj_train& T = *J.T;
    const size_t t0 = J.t_off, q0 = J.q_off;
    d.nt = T.n; d.nq = J.nq;
    d.min_x = T.min_x; d.min_y = T.min_y; d.gw_inv = T.grid_w_inv; d.gh_inv = T.grid_h_inv;
    if (U.of[j]) { const float* g = &U.grid[(size_t)j * 4]; d.min_x = g[0]; d.min_y = g[1]; d.gw_inv = g[2]; d.gh_inv = g[3]; }
    if (ks_ordered(J.kind)) { d.c_off = (int32_t)c0; c0 += J.nq; }
    memcpy(d.R, J.R, 36); memcpy(d.t, J.t, 12);
    if (J.ow) memcpy(d.ow, J.ow, 12);
    if (J.R2) { memcpy(d.R2, J.R2, 36); memcpy(d.t2, J.t2, 12); }
    d.fx = J.fx; d.fy = J.fy; d.cx = J.cx; d.cy = J.cy;
    memcpy(d.bounds, J.bounds, 16); memcpy(d.scale, J.scale, 32);
    d.log_scale = J.log_scale; d.n_levels = J.n_levels; d.th = J.th; d.th_dist = J.th_dist; d.check_ori = J.check_ori;
    if (U.of[j] && T.n > 0) {
      U.jobs.push_back(FrameStageJob{U.of[j]->slab, T.n, (int32_t)t0, d.grid_off, j});
    } else if (U.any()) {
      U.all_staged = false;
    }
    if (T.n > 0) {
      const size_t n = (size_t)T.n;
      if (!U.of[j]) {
        const size_t filled = std::min((size_t)T.cell_off[NCELL], n);
        memcpy(H + o_tx + t0 * 4, T.x, n * 4); memcpy(H + o_ty + t0 * 4, T.y, n * 4);
        memcpy(H + o_toct + t0 * 4, T.octave, n * 4); memcpy(H + o_tdesc + t0 * 32, T.desc, n * 32);
        if (T.angle) memcpy(H + o_tang + t0 * 4, T.angle, n * 4);
        memcpy(H + o_coff + (size_t)d.grid_off * 4, T.cell_off, (size_t)(NCELL + 1) * 4);
        memcpy(H + o_cidx + t0 * 4, T.cell_idx, filled * 4);
      }
      if (ks_ordered(J.kind)) memcpy(H + o_tocc + t0, T.occupied, n);
    }
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
  KsPair* hp = (KsPair*)(H + o_pair);
  for (int p = 0; p < npair; p++) {
    const KsHostJob& a = jobs[2 * p];
    const KsHostJob& b = jobs[2 * p + 1];
    hp[p] = a.skip ? KsPair{0, 0, 0, 0} : KsPair{(int32_t)a.q_off, a.nq, (int32_t)b.q_off, b.nq};
  }
  if (U.any() && !U.jobs.empty()) memcpy(H + o_fjobs, U.jobs.data(), sizeof(FrameStageJob) * U.jobs.size());
  if (U.all_staged) {   // everything but the searched sides' arrays and grids
    PS_HIP(hipMemcpyAsync(D, H, o_tx, hipMemcpyHostToDevice, m->stream));
    PS_HIP(hipMemcpyAsync(D + o_tocc, H + o_tocc, in_bytes - o_tocc, hipMemcpyHostToDevice, m->stream));
  } else {
    PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
  }
  PS_HIP(hipMemsetAsync(D + o_nm, 0, out_end - o_nm, m->stream));   // nmatch, overflow, nfound, frame status
  if (U.any()) {
    FrameStageDst dst{(float*)(D + o_tx), (float*)(D + o_ty), (int32_t*)(D + o_toct), (float*)(D + o_tang), (float*)(D + o_tur), D + o_tdesc,
                      (int32_t*)(D + o_coff), (int32_t*)(D + o_cidx), (int32_t*)(D + o_fst)};
    if ((frc = frame_use_stage(U, m, (const FrameStageJob*)(D + o_fjobs), dst)) != PS_OK) return frc;
  }
  KsArrays A;
  A.job = (const KsJob*)(D + o_job);
  A.tx = (const float*)(D + o_tx); A.ty = (const float*)(D + o_ty); A.toct = (const int32_t*)(D + o_toct); A.tang = (const float*)(D + o_tang);
  A.tdesc = D + o_tdesc; A.tocc = D + o_tocc; A.cell_off = (const int32_t*)(D + o_coff); A.cell_idx = (const int32_t*)(D + o_cidx);
  A.qvalid = D + o_qvalid; A.qpos = (const float*)(D + o_qpos); A.qnormal = (const float*)(D + o_qnor); A.qmin = (const float*)(D + o_qmin);
  A.qmax = (const float*)(D + o_qmax); A.qdesc = D + o_qdesc; A.qang = (const float*)(D + o_qang);
  A.best_idx = (int32_t*)(D + o_bi); A.best_dist = (int32_t*)(D + o_bd);
  A.cand = (uint32_t*)(D + o_cand); A.ncand = (int32_t*)(D + o_ncand); A.qtop = (uint32_t*)(D + o_qtop);
  A.match = (int32_t*)(D + o_match); A.nmatch = (int32_t*)(D + o_nm); A.overflow = (int32_t*)(D + o_ovf);
  A.pair = (const KsPair*)(D + o_pair); A.match12 = (int32_t*)(D + o_m12); A.nfound = (int32_t*)(D + o_nf);
  hipEventRecord(m->ev0, m->stream);
  psk_ks_launch(&A, nj, max_nq, any_ordered, npair, m->stream);
  hipEventRecord(m->ev1, m->stream);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(H + o_bi, D + o_bi, out_end - o_bi, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  hipEventElapsedTime(&m->last_kernel_ms, m->ev0, m->ev1);
  const int32_t* ovf = (const int32_t*)(H + o_ovf);
  const int32_t* nm = (const int32_t*)(H + o_nm);
  const int32_t* fst = (const int32_t*)(H + o_fst);
  // An order-dependent job in which a point kept more than PS_KS_CAP candidates runs again with rows of PS_KS_CAP_WIDE in a store
  // of its own; the others keep their results.  One that overflows that too is the only one that fails.
  std::vector<int> wide;
  for (int j = 0; j < nj; j++) {
    KsHostJob& J = jobs[j];
    J.status = J.skip ? 1 : (U.any() && fst[j]) ? 2 : 0;
    J.nmatch = nm[j];
    if (J.status == 0 && ovf[j] > 0) wide.push_back(j);
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
    size_t woff = 0;
    auto wtake = [&](size_t bytes) { size_t r = woff; woff += al(bytes + 64); return r; };
    const size_t w_job = wtake(sizeof(KsJob) * sub.size()), w_nm = wtake(sub.size() * 4), w_ovf = wtake(sub.size() * 4), w_cand = wtake(nq2 * PS_KS_CAP_WIDE * 4);
    if (woff > m->d_wide_bytes) {
      if (m->d_wide) hipFree(m->d_wide);
      m->d_wide = nullptr; m->d_wide_bytes = 0;
      PS_HIP(hipMalloc(&m->d_wide, woff));
      m->d_wide_bytes = woff;
    }
    uint8_t* Wd = m->d_wide;
    PS_HIP(hipMemcpyAsync(Wd + w_job, sub.data(), sizeof(KsJob) * sub.size(), hipMemcpyHostToDevice, m->stream));
    PS_HIP(hipMemsetAsync(Wd + w_nm, 0, w_cand - w_nm, m->stream));
    KsArrays A2 = A;
    A2.job = (const KsJob*)(Wd + w_job); A2.cand = (uint32_t*)(Wd + w_cand); A2.nmatch = (int32_t*)(Wd + w_nm); A2.overflow = (int32_t*)(Wd + w_ovf);
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
  out.best_idx = (const int32_t*)(H + o_bi); out.best_dist = (const int32_t*)(H + o_bd); out.match = (const int32_t*)(H + o_match);
  out.match12 = (const int32_t*)(H + o_m12); out.nfound = (const int32_t*)(H + o_nf);
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
  if (stale >= 0)
    return ps_set_error(PS_ERR_INVALID, "%s problem %d: the frame handle does not hold the keypoints it was published with "
                        "(the extractor's count differed from the n given to ps_frame_publish_orb)", what, stale);
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
