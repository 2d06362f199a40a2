// Host side of the frame handle (include/pointslot_hip.h, ps_frame): a stereo Frame's search-relevant state kept in HBM between the
// calls that search into it - what Frame::Frame leaves in mvKeysUn, mvuRight, mDescriptors and mGrid
// (/root/reference/src/Frame.cc:709-722, 1636-1656).  Kernels: frame_kernels.hip; the consumers are in match_host.hip.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "frame_host.h"
#include "ps_common.h"

extern "C" {
void psk_frame_publish_launch(const FramePubBatch*, int, hipStream_t);
}

namespace {
inline size_t al(size_t v) { return (v + 255) / 256 * 256; }
inline size_t al16(size_t v) { return (v + 15) / 16 * 16; }

// `st` waits for everything that still reads or writes the slab of `f` (f->mu held)
int wait_for_slab(ps_frame* f, hipStream_t st) {
  if (f->published) PS_HIP(hipStreamWaitEvent(st, f->ev_ready, 0));   // (a batch publish may have run on another handle's stream)
  for (int i = 0; i < ps_frame::USES; i++)
    if (f->user[i]) PS_HIP(hipStreamWaitEvent(st, f->ev_use[i], 0));
  return PS_OK;
}

void fill_job(FramePubJob& J, const ps_frame* f, const ps_keypoint* kps, const float* ur, const uint8_t* desc, const int32_t* count, int n,
              float min_x, float min_y, float gw_inv, float gh_inv) {
  J.dst = f->slab; J.kps = kps; J.u_right = ur; J.desc = desc; J.count = count;
  J.n = n; J.prev_n = f->prev_n; J.capacity = f->capacity; J.pad = 0;
  J.min_x = min_x; J.min_y = min_y; J.gw_inv = gw_inv; J.gh_inv = gh_inv;
}

void published(ps_frame* f, int n, float min_x, float min_y, float gw_inv, float gh_inv) {
  f->n = n; f->prev_n = n; f->published = true;
  f->grid[0] = min_x; f->grid[1] = min_y; f->grid[2] = gw_inv; f->grid[3] = gh_inv;
}
}  // namespace

int psf_consume_begin(ps_frame* const* uniq, int n, hipStream_t st) {
  for (int i = 0; i < n; i++) {
    uniq[i]->mu.lock();
    hipError_t e = uniq[i]->published ? hipStreamWaitEvent(st, uniq[i]->ev_ready, 0) : hipSuccess;
    if (!uniq[i]->published || e != hipSuccess) {
      for (int k = 0; k <= i; k++) uniq[k]->mu.unlock();
      if (e != hipSuccess) return ps_set_error(PS_ERR_HIP, "hipStreamWaitEvent: %s", hipGetErrorString(e));
      return ps_set_error(PS_ERR_INVALID, "frame handle %d of the call has never been published", i);
    }
  }
  return PS_OK;
}

int psf_consume_end(ps_frame* const* uniq, int n, const void* consumer, hipStream_t st, bool record) {
  hipError_t err = hipSuccess;
  for (int i = 0; i < n; i++) {
    ps_frame* f = uniq[i];
    if (record) {
      int slot = -1;
      for (int k = 0; k < ps_frame::USES && slot < 0; k++) if (f->user[k] == consumer) slot = k;
      for (int k = 0; k < ps_frame::USES && slot < 0; k++) if (!f->user[k]) slot = k;
      if (slot < 0) {
        slot = 0;
        for (int k = 1; k < ps_frame::USES; k++) if (f->use_seq[k] < f->use_seq[slot]) slot = k;
        hipError_t e = hipStreamWaitEvent(st, f->ev_use[slot], 0);   // the new event then stands for the old reader too
        if (e != hipSuccess) err = e;
      }
      hipError_t e = hipEventRecord(f->ev_use[slot], st);
      if (e != hipSuccess) err = e;
      f->user[slot] = consumer; f->use_seq[slot] = ++f->seq;
    }
    f->mu.unlock();
  }
  if (err != hipSuccess) return ps_set_error(PS_ERR_HIP, "frame handle bookkeeping: %s", hipGetErrorString(err));
  return PS_OK;
}

extern "C" {

int ps_frame_create(int device, int capacity, ps_frame** out) {
  if (!out) return ps_set_error(PS_ERR_INVALID, "null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ps_set_error(PS_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return ps_set_error(PS_ERR_INVALID, "bad device ordinal");
  if (capacity < 1 || capacity > PS_FRAME_MAX_N) return ps_set_error(PS_ERR_INVALID, "ps_frame_create: capacity must be 1..%d", PS_FRAME_MAX_N);
  PS_HIP(hipSetDevice(device));
  ps_frame* f = new ps_frame();
  f->device = device; f->capacity = capacity;
  const size_t C = (size_t)capacity;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += al(bytes); return r; };
  const size_t o_hdr = take(sizeof(FrameHdr)), o_x = take(C * 4), o_y = take(C * 4), o_oct = take(C * 4), o_ang = take(C * 4), o_ur = take(C * 4);
  const size_t o_desc = take(C * 32), o_coff = take((size_t)(PS_FRAME_NCELL + 1) * 4), o_cidx = take(C * 4);
  f->stage_bytes = al16(C * sizeof(ps_keypoint)) + al16(C * 4) + C * 32;
  const size_t o_stage = take(f->stage_bytes);
  f->slab_bytes = off;
  hipError_t e = hipMalloc(&f->d_slab, f->slab_bytes);
  if (e == hipSuccess) e = hipHostMalloc(&f->h_stage, f->stage_bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);
  hipEvent_t* evs[4] = {&f->ev_ready, &f->ev_src, &f->ev_t0, &f->ev_t1};
  for (int i = 0; i < 4 && e == hipSuccess; i++) e = i < 2 ? hipEventCreateWithFlags(evs[i], hipEventDisableTiming) : hipEventCreate(evs[i]);
  for (int i = 0; i < ps_frame::USES && e == hipSuccess; i++) e = hipEventCreateWithFlags(&f->ev_use[i], hipEventDisableTiming);
  if (e == hipSuccess) {
    if (const char* fill = getenv("PS_DEBUG_FILL")) {   // diagnostic: poison the fresh slab; the fill runs on the null stream, which the
      e = hipMemset(f->d_slab, atoi(fill), f->slab_bytes);   // handle's non-blocking stream does not wait for (see match_host.hip: ensure)
      if (e == hipSuccess) e = hipDeviceSynchronize();
    }
  }
  if (e != hipSuccess) {
    int rc = ps_set_error(PS_ERR_HIP, "ps_frame_create: %s", hipGetErrorString(e));
    ps_frame_destroy(f);
    return rc;
  }
  uint8_t* D = f->d_slab;
  f->slab.hdr = (FrameHdr*)(D + o_hdr);
  f->slab.x = (float*)(D + o_x); f->slab.y = (float*)(D + o_y); f->slab.octave = (int32_t*)(D + o_oct);
  f->slab.angle = (float*)(D + o_ang); f->slab.u_right = (float*)(D + o_ur); f->slab.desc = D + o_desc;
  f->slab.cell_off = (int32_t*)(D + o_coff); f->slab.cell_idx = (int32_t*)(D + o_cidx);
  f->d_stage = D + o_stage;
  f->prev_n = capacity;   // the first publish clears whatever the fresh slab holds behind its n
  *out = f;
  return PS_OK;
}

void ps_frame_destroy(ps_frame* f) {
  if (!f) return;
  hipSetDevice(f->device);
  {
    std::lock_guard<std::mutex> lock(f->mu);
    if (f->published) hipEventSynchronize(f->ev_ready);
    for (int i = 0; i < ps_frame::USES; i++)
      if (f->user[i]) hipEventSynchronize(f->ev_use[i]);
    if (f->stream) hipStreamSynchronize(f->stream);
  }
  hipEvent_t evs[4] = {f->ev_ready, f->ev_src, f->ev_t0, f->ev_t1};
  for (hipEvent_t ev : evs) if (ev) hipEventDestroy(ev);
  for (int i = 0; i < ps_frame::USES; i++) if (f->ev_use[i]) hipEventDestroy(f->ev_use[i]);
  if (f->stream) hipStreamDestroy(f->stream);
  if (f->d_slab) hipFree(f->d_slab);
  if (f->h_stage) hipHostFree(f->h_stage);
  delete f;
}

int ps_frame_publish_host(ps_frame* f, const ps_keypoint* kps, const float* u_right, const uint8_t* desc, int n, float min_x, float min_y,
                          float grid_w_inv, float grid_h_inv) {
  if (!f || n < 0 || (n > 0 && (!kps || !desc))) return ps_set_error(PS_ERR_INVALID, "ps_frame_publish_host: bad argument");
  if (n > f->capacity) return ps_set_error(PS_ERR_CAPACITY, "ps_frame_publish_host: %d keypoints, the handle holds %d", n, f->capacity);
  std::lock_guard<std::mutex> lock(f->mu);
  PS_HIP(hipSetDevice(f->device));
  if (f->published) PS_HIP(hipEventSynchronize(f->ev_ready));   // the staging block is read by the upload of the publish before
  const size_t o_ur = al16((size_t)n * sizeof(ps_keypoint)), o_desc = o_ur + al16((size_t)n * 4), total = o_desc + (size_t)n * 32;
  if (n > 0) {
    memcpy(f->h_stage, kps, (size_t)n * sizeof(ps_keypoint));
    if (u_right) memcpy(f->h_stage + o_ur, u_right, (size_t)n * 4);
    memcpy(f->h_stage + o_desc, desc, (size_t)n * 32);
  }
  int rc = wait_for_slab(f, f->stream);
  if (rc != PS_OK) return rc;
  PS_HIP(hipEventRecord(f->ev_t0, f->stream));
  if (n > 0) PS_HIP(hipMemcpyAsync(f->d_stage, f->h_stage, total, hipMemcpyHostToDevice, f->stream));
  FramePubBatch B;
  memset(&B, 0, sizeof(B));
  fill_job(B.job[0], f, (const ps_keypoint*)f->d_stage, u_right ? (const float*)(f->d_stage + o_ur) : nullptr, f->d_stage + o_desc, nullptr, n,
           min_x, min_y, grid_w_inv, grid_h_inv);
  psk_frame_publish_launch(&B, 1, f->stream);
  PS_HIP(hipGetLastError());
  PS_HIP(hipEventRecord(f->ev_t1, f->stream));
  PS_HIP(hipEventRecord(f->ev_ready, f->stream));
  published(f, n, min_x, min_y, grid_w_inv, grid_h_inv);
  return PS_OK;
}

int ps_frame_publish_orb(ps_frame* const* frames, int nframes, ps_orb* h, const int32_t* image, const int32_t* pair, const int32_t* n,
                         float min_x, float min_y, float grid_w_inv, float grid_h_inv) {
  if (!frames || nframes < 1 || !h || !image || !pair || !n) return ps_set_error(PS_ERR_INVALID, "ps_frame_publish_orb: bad argument");
  PsOrbView V;
  int rc = psk_orb_view(h, &V);
  if (rc != PS_OK) return rc;
  if (!V.planned) return ps_set_error(PS_ERR_INVALID, "ps_frame_publish_orb: the extractor has not processed an image");
  for (int k = 0; k < nframes; k++) {
    if (!frames[k] || frames[k]->device != V.device) return ps_set_error(PS_ERR_INVALID, "ps_frame_publish_orb: frame %d is null or on another device", k);
    if (image[k] < 0 || image[k] >= V.max_batch || pair[k] < -1 || pair[k] >= V.max_batch || n[k] < 0 || n[k] > V.kp_cap)
      return ps_set_error(PS_ERR_INVALID, "ps_frame_publish_orb: frame %d: image %d / pair %d / n %d outside the extractor's batch", k, image[k], pair[k], n[k]);
    if (n[k] > frames[k]->capacity) return ps_set_error(PS_ERR_CAPACITY, "ps_frame_publish_orb: frame %d: %d keypoints, the handle holds %d", k, n[k], frames[k]->capacity);
  }
  std::vector<ps_frame*> order(frames, frames + nframes);
  std::sort(order.begin(), order.end());
  if (std::adjacent_find(order.begin(), order.end()) != order.end()) return ps_set_error(PS_ERR_INVALID, "ps_frame_publish_orb: a frame handle appears twice");
  PS_HIP(hipSetDevice(V.device));
  for (ps_frame* f : order) f->mu.lock();
  struct Unlock { std::vector<ps_frame*>& v; ~Unlock() { for (ps_frame* f : v) f->mu.unlock(); } } unlock{order};
  // one stream carries the launch: behind the extractor's stream (stereo matcher included) and behind every reader of the slabs
  hipStream_t st = frames[0]->stream;
  PS_HIP(hipEventRecord(frames[0]->ev_src, V.stream));
  PS_HIP(hipStreamWaitEvent(st, frames[0]->ev_src, 0));
  for (int k = 0; k < nframes; k++) {
    rc = wait_for_slab(frames[k], st);
    if (rc != PS_OK) return rc;
  }
  for (int k = 0; k < nframes; k++) PS_HIP(hipEventRecord(frames[k]->ev_t0, st));
  for (int k0 = 0; k0 < nframes; k0 += PS_FRAME_PUB_BATCH) {   // one launch for up to PS_FRAME_PUB_BATCH frames
    const int nb = std::min(PS_FRAME_PUB_BATCH, nframes - k0);
    FramePubBatch B;
    memset(&B, 0, sizeof(B));
    for (int j = 0; j < nb; j++) {
      const int k = k0 + j;
      const size_t row = (size_t)image[k] * V.kp_cap;
      fill_job(B.job[j], frames[k], V.d_kps + row, pair[k] >= 0 ? V.d_uright + (size_t)pair[k] * V.kp_cap : nullptr, V.d_desc + row * 32,
               V.d_counts + image[k], n[k], min_x, min_y, grid_w_inv, grid_h_inv);
    }
    psk_frame_publish_launch(&B, nb, st);
    PS_HIP(hipGetLastError());
  }
  for (int k = 0; k < nframes; k++) {
    PS_HIP(hipEventRecord(frames[k]->ev_t1, st));
    PS_HIP(hipEventRecord(frames[k]->ev_ready, st));
    published(frames[k], n[k], min_x, min_y, grid_w_inv, grid_h_inv);
  }
  // the extractor's next batch overwrites what the launch reads: its stream goes on behind the publish (a wait on the device)
  PS_HIP(hipStreamWaitEvent(V.stream, frames[nframes - 1]->ev_ready, 0));
  return PS_OK;
}

int ps_frame_count(ps_frame* f, int* n) {
  if (!f || !n) return ps_set_error(PS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(f->mu);
  *n = f->n;
  return PS_OK;
}

int ps_frame_last_publish_ms(ps_frame* f, float* ms) {
  if (!f || !ms) return ps_set_error(PS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(f->mu);
  if (!f->published) return ps_set_error(PS_ERR_INVALID, "the frame handle has never been published");
  PS_HIP(hipSetDevice(f->device));
  PS_HIP(hipEventSynchronize(f->ev_t1));
  PS_HIP(hipEventElapsedTime(ms, f->ev_t0, f->ev_t1));
  return PS_OK;
}

int ps_frame_debug_read(ps_frame* f, int what, void* out, size_t out_bytes, int* n) {
  if (!f || !n || what < 0 || what > 7) return ps_set_error(PS_ERR_INVALID, "ps_frame_debug_read: bad argument");
  std::lock_guard<std::mutex> lock(f->mu);
  if (!f->published) return ps_set_error(PS_ERR_INVALID, "the frame handle has never been published");
  PS_HIP(hipSetDevice(f->device));
  PS_HIP(hipEventSynchronize(f->ev_ready));
  FrameHdr hdr;
  PS_HIP(hipMemcpy(&hdr, f->slab.hdr, sizeof(hdr), hipMemcpyDeviceToHost));
  *n = hdr.n;
  if (hdr.mismatch || hdr.n != f->n)
    return ps_set_error(PS_ERR_INVALID, "the frame was published with n = %d, the extractor's count gave %d", f->n, hdr.n);
  const void* src[8] = {f->slab.x, f->slab.y, f->slab.octave, f->slab.angle, f->slab.u_right, f->slab.desc, f->slab.cell_off, f->slab.cell_idx};
  const size_t bytes = what == 5 ? (size_t)hdr.n * 32 : what == 6 ? (size_t)(PS_FRAME_NCELL + 1) * 4 : (size_t)hdr.n * 4;
  if (bytes > out_bytes) return ps_set_error(PS_ERR_CAPACITY, "ps_frame_debug_read: %zu bytes, caller buffer %zu", bytes, out_bytes);
  if (bytes > 0) {
    if (!out) return ps_set_error(PS_ERR_INVALID, "null output buffer");
    PS_HIP(hipMemcpy(out, src[what], bytes, hipMemcpyDeviceToHost));
  }
  return PS_OK;
}

}  // extern "C"
