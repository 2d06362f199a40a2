// Host side of the matcher C-ABI (include/pointslot_hip.h): the matcher handle and its arenas, the frame-handle protocol every
// windowed matcher shares (FrameUse, matcher_host.h), and the calls without a search window - the Hamming matrix, brute-force
// matching (match_kernels.hip) and the distinctive descriptors.  The windowed matchers: search_host.hip (projection, fuse),
// kfsearch_host.hip (loop closure, relocalisation, Sim3), tri_host.hip (CreateNewMapPoints).
// Replaces ORBmatcher::SearchByBruceMatching / DescriptorDistance — /root/reference/src/ORBmatcher.cc.
#include "matcher_host.h"   // (the HIP runtime, before the plan: its vector types)
#include "match_plan.h"

extern "C" {
void psk_bf_launch(const BfBlock*, int, const BfProb*, int, const uint8_t*, const float*, const uint8_t*, const uint8_t*,
                   const float*, uint32_t*, int32_t*, int32_t*, float, int, hipStream_t);
void psk_hamming_matrix_launch(const uint8_t*, int, const uint8_t*, int, uint16_t*, hipStream_t);
void psk_distinctive_launch(const uint8_t*, const int32_t*, int32_t*, int, hipStream_t);
void psk_frame_stage_launch(const FrameStageJob*, int, const FrameStageDst*, hipStream_t);
}

int psm_ensure(ps_matcher* m, size_t need) {
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

int psm_ensure_wide(ps_matcher* m, size_t bytes) {
  if (bytes <= m->d_wide_bytes) return PS_OK;
  if (m->d_wide) hipFree(m->d_wide);
  m->d_wide = nullptr; m->d_wide_bytes = 0;
  PS_HIP(hipMalloc(&m->d_wide, bytes));
  if (const char* fill = getenv("PS_DEBUG_FILL")) {   // diagnostic, as in psm_ensure: the fill has landed before the handle's stream uses the buffer
    PS_HIP(hipMemset(m->d_wide, atoi(fill), bytes));
    PS_HIP(hipDeviceSynchronize());
  }
  m->d_wide_bytes = bytes;
  return PS_OK;
}

int FrameUse::init(ps_matcher* m, ps_frame* const* frames, int nprob, const char* what) {
  of.assign(nprob, nullptr);
  grid.assign((size_t)nprob * 4, 0.f);
  if (!frames) return PS_OK;
  for (int p = 0; p < nprob; p++) {
    ps_frame* f = frames[p];
    if (!f) continue;
    if (f->device != m->device) return ps_set_error(PS_ERR_INVALID, "%s problem %d: the frame handle lives on another device", what, p);
    of[p] = f;
    uniq.push_back(f);
  }
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  return PS_OK;
}

int FrameUse::check(int p, int train_n, const char* what) {
  ps_frame* f = of[p];
  std::lock_guard<std::mutex> lock(f->mu);
  if (!f->published) return ps_set_error(PS_ERR_INVALID, "%s problem %d: the frame handle has never been published", what, p);
  if (train_n != f->n) return ps_set_error(PS_ERR_INVALID, "%s problem %d: train.n = %d, the frame handle holds %d keypoints", what, p, train_n, f->n);
  memcpy(&grid[(size_t)p * 4], f->grid, 16);
  return PS_OK;
}

int FrameUse::upload(ps_matcher* m, uint8_t* H, uint8_t* D, size_t in_bytes, const SideSkip& skip) {
  if (any()) {
    memset(H + o_jobs, 0, sizeof(FrameStageJob) * nslots);
    if (!jobs.empty()) memcpy(H + o_jobs, jobs.data(), sizeof(FrameStageJob) * jobs.size());
  }
  size_t lo = 0;
  if (any() && !needs_host)   // everything but the staged arrays and grids
    for (int i = 0; i < skip.n; lo = skip.r[i++].hi)
      PS_HIP(hipMemcpyAsync(D + lo, H + lo, skip.r[i].lo - lo, hipMemcpyHostToDevice, m->stream));
  PS_HIP(hipMemcpyAsync(D + lo, H + lo, in_bytes - lo, hipMemcpyHostToDevice, m->stream));
  return PS_OK;
}

int FrameUse::stage(ps_matcher* m, uint8_t* D, const SideOff& o) {
  if (!any()) return PS_OK;
  const FrameStageDst dst = side_stage_dst<FrameStageDst>(o, D, ptr<int32_t>(D, o_status));
  PS_HIP(hipMemsetAsync(D + o_status, 0, (size_t)nslots * 4, m->stream));
  PS_TRY(psf_consume_begin(uniq.data(), (int)uniq.size(), m->stream));
  hipError_t e = hipSuccess;
  if (!jobs.empty()) {
    psk_frame_stage_launch(ptr<const FrameStageJob>(D, o_jobs), (int)jobs.size(), &dst, m->stream);
    e = hipGetLastError();
  }
  const int rc = psf_consume_end(uniq.data(), (int)uniq.size(), m, m->stream, !jobs.empty() && e == hipSuccess);
  if (e != hipSuccess) return ps_set_error(PS_ERR_HIP, "frame_stage: %s", hipGetErrorString(e));
  return rc;
}

int frame_stale_error(const char* what, int p, long more, int n) {
  char and_more[40] = "", count[16] = "";
  if (more >= 0) snprintf(and_more, sizeof and_more, " (and %ld more)", more);
  if (n >= 0) snprintf(count, sizeof count, "%d ", n);
  return ps_set_error(PS_ERR_INVALID, "%s problem %d%s: the frame handle does not hold the %skeypoints it was published with "
                      "(the extractor's count differed from the n given to ps_frame_publish_orb)", what, p, and_more, count);
}

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
  PS_TRY(psm_ensure(m, total));
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
  PS_TRY(psm_ensure(m, off));
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
  PS_TRY(psm_kernels_begin(m));
  psk_bf_launch((const BfBlock*)(D + o_blk), (int)blocks.size(), (const BfProb*)(D + o_prob), nprob, D + o_qd,
                (const float*)(D + o_qa), D + o_qv, D + o_td, (const float*)(D + o_ta), (uint32_t*)(D + o_topk),
                (int32_t*)(D + o_out), (int32_t*)(D + o_nm), nn_ratio, check_orientation, m->stream);
  PS_TRY(psm_kernels_end(m));
  PS_HIP(hipMemcpyAsync(H + o_out, D + o_out, out_bytes, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  PS_TRY(psm_kernels_ms(m));
  for (int p = 0; p < nprob; p++) {
    ps_bf_problem& P = probs[p];
    if (P.nt > 0) memcpy(P.query_of_train, H + o_out + (size_t)dp[p].t_off * 4, (size_t)P.nt * 4);
    P.nmatches = ((const int32_t*)(H + o_nm))[p];
  }
  return PS_OK;
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
  PS_TRY(psm_ensure(m, end));
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
}  // extern "C"
