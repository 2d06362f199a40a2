// Host side of the keyframe database C-ABI (include/pointslot_hip.h): the ps_kfdb handle, add / erase / clear, the batched query,
// ps_kfdb_score and the host-only covisibility stage ps_kfdb_select.  Replaces KeyFrameDatabase (src/KeyFrameDatabase.cc:41-310 of
// the reference).  The id -> slot map and the exclusion bitmask are host work; add, query and score run on the matcher handle's
// stream and arenas.
#include <hip/hip_runtime.h>
#include <cmath>
#include <mutex>
#include <set>
#include <string.h>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "kfdb_plan.h"
#include "matcher_host.h"
#include "ps_common.h"

extern "C" {
void psk_kfdb_put_launch(const KfdbAddArrays*, int, hipStream_t);
void psk_kfdb_query_launch(const KfdbQueryArrays*, int, hipStream_t);
void psk_kfdb_score_launch(const KfdbScoreArrays*, hipStream_t);
}

struct ps_kfdb {
  std::mutex mu;                                     // taken before the matcher's
  int device = 0, capacity = 0, max_words = 0;
  uint8_t* d_slab = nullptr;
  KfdbStore S = {};                                  // S.high follows the host's
  std::unordered_map<int64_t, int32_t> slot_of;      // live keyframes
  std::set<int32_t> free_slots;                      // the lowest free slot is taken first: the kernels walk [0, high)
  std::vector<int32_t> h_len;                        // host copies of len / serial, uploaded whole by erase and clear
  std::vector<uint32_t> h_serial;
  uint32_t next_serial = 1;
};

namespace {
bool ascending(const int32_t* id, int n) {
  for (int i = 0; i < n; i++)
    if (id[i] < 0 || (i > 0 && id[i] <= id[i - 1])) return false;
  return true;
}
void set_high(ps_kfdb* db) {
  int h = db->capacity;
  while (h > 0 && db->h_serial[(size_t)h - 1] == 0) h--;
  db->S.high = h;
}
int upload_state(ps_kfdb* db, int upto) {
  if (upto <= 0) return PS_OK;
  PS_HIP(hipSetDevice(db->device));
  PS_HIP(hipMemcpy(db->S.len, db->h_len.data(), (size_t)upto * 4, hipMemcpyHostToDevice));
  PS_HIP(hipMemcpy(db->S.serial, db->h_serial.data(), (size_t)upto * 4, hipMemcpyHostToDevice));
  return PS_OK;
}
}  // namespace

extern "C" {

int ps_kfdb_create(int device, int capacity, int max_words, ps_kfdb** out) {
  if (!out) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_create: null argument");
  *out = nullptr;
  if (capacity < 1 || capacity > PS_KFDB_MAX_CAPACITY) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_create: capacity %d outside 1 .. %d", capacity, PS_KFDB_MAX_CAPACITY);
  if (max_words < 1 || max_words > PS_KFDB_MAX_WORDS) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_create: max_words %d outside 1 .. %d", max_words, PS_KFDB_MAX_WORDS);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ps_set_error(PS_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return ps_set_error(PS_ERR_INVALID, "bad device ordinal");
  PS_HIP(hipSetDevice(device));
  const size_t C = (size_t)capacity, stride = ((size_t)max_words + 63) / 64 * 64;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t r = off; off += al(bytes); return r; };
  const size_t o_vals = take(C * stride * 8), o_ids = take(C * stride * 4), o_kfid = take(C * 8), o_len = take(C * 4), o_serial = take(C * 4), o_reloc = take(C * 4);
  ps_kfdb* db = new ps_kfdb();
  db->device = device; db->capacity = capacity; db->max_words = max_words;
  hipError_t e = hipMalloc(&db->d_slab, off);
  if (e == hipSuccess) e = hipMemset(db->d_slab + o_kfid, 0, off - o_kfid);
  if (const char* fill = getenv("PS_DEBUG_FILL")) {   // diagnostic, as in psm_ensure: poison the rows (vals, ids), which nothing zeroes, and wait for the fill
    if (e == hipSuccess) e = hipMemset(db->d_slab, atoi(fill), o_kfid);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e != hipSuccess) {
    if (db->d_slab) hipFree(db->d_slab);
    delete db;
    return ps_set_error(PS_ERR_HIP, "ps_kfdb_create: %s", hipGetErrorString(e));
  }
  uint8_t* D = db->d_slab;
  db->S.ids = (int32_t*)(D + o_ids); db->S.vals = (double*)(D + o_vals); db->S.len = (int32_t*)(D + o_len);
  db->S.serial = (uint32_t*)(D + o_serial); db->S.kfid = (int64_t*)(D + o_kfid); db->S.reloc = (float*)(D + o_reloc);
  db->S.stride = (int32_t)stride; db->S.high = 0;
  db->h_len.assign(C, 0); db->h_serial.assign(C, 0);
  for (int s = 0; s < capacity; s++) db->free_slots.insert(db->free_slots.end(), s);
  *out = db;
  return PS_OK;
}

void ps_kfdb_destroy(ps_kfdb* db) {
  if (!db) return;
  hipSetDevice(db->device);
  if (db->d_slab) hipFree(db->d_slab);
  delete db;
}

int ps_kfdb_size(const ps_kfdb* db, int32_t* size) {
  if (!db || !size) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_size: null argument");
  std::lock_guard<std::mutex> lock(const_cast<ps_kfdb*>(db)->mu);
  *size = (int32_t)db->slot_of.size();
  return PS_OK;
}

int ps_kfdb_add(ps_kfdb* db, ps_matcher* m, const int64_t* ids, const int32_t* const* bow_id, const double* const* bow_val,
                const int32_t* bow_n, int n, int32_t* stored) {
  if (!db || !m || n < 0 || (n > 0 && (!ids || !bow_id || !bow_val || !bow_n))) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_add: bad argument");
  if (db->device != m->device) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_add: the database lives on device %d, the matcher on device %d", db->device, m->device);
  std::lock_guard<std::mutex> dlock(db->mu);
  std::unordered_set<int64_t> seen;
  for (int e = 0; e < n; e++) {
    if (bow_n[e] < 0 || (bow_n[e] > 0 && (!bow_id[e] || !bow_val[e]))) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_add: entry %d: negative count or null arrays", e);
    if (db->slot_of.count(ids[e]) || !seen.insert(ids[e]).second) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_add: entry %d: id %lld is already stored", e, (long long)ids[e]);
    if (bow_n[e] <= db->max_words && !ascending(bow_id[e], bow_n[e])) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_add: entry %d: word ids not ascending", e);
  }
  // slots and serials in entry order; an entry beyond a limit fails alone
  std::vector<int32_t> slot, off, len, src;
  std::vector<uint32_t> serial;
  int nfail = 0, first_fail = -1;
  size_t NW = 0;
  for (int e = 0; e < n; e++) {
    const bool ok = bow_n[e] <= db->max_words && !db->free_slots.empty() && db->next_serial != 0;
    if (stored) stored[e] = ok ? 1 : 0;
    if (!ok) { if (nfail++ == 0) first_fail = e; continue; }
    const int32_t s = *db->free_slots.begin();
    db->free_slots.erase(db->free_slots.begin());
    slot.push_back(s); off.push_back((int32_t)NW); len.push_back(bow_n[e]); src.push_back(e); serial.push_back(db->next_serial++);
    NW += (size_t)bow_n[e];
  }
  const int ns = (int)slot.size();
  auto undo = [&]() { for (int i = 0; i < ns; i++) db->free_slots.insert(slot[i]); };
  if (ns > 0) {
    std::lock_guard<std::mutex> lock(m->mu);
    Arena a;
    const size_t o_slot = a.take((size_t)ns * 4), o_off = a.take((size_t)ns * 4), o_n = a.take((size_t)ns * 4), o_ser = a.take((size_t)ns * 4), o_kfid = a.take((size_t)ns * 8);
    const size_t o_id = a.take(NW * 4), o_val = a.take(NW * 8);
    hipError_t he = hipSetDevice(m->device);
    int rc = he == hipSuccess ? psm_ensure(m, a.off) : ps_set_error(PS_ERR_HIP, "ps_kfdb_add: %s", hipGetErrorString(he));
    if (rc != PS_OK) { undo(); return rc; }
    uint8_t* H = m->h_buf;
    memcpy(H + o_slot, slot.data(), (size_t)ns * 4); memcpy(H + o_off, off.data(), (size_t)ns * 4); memcpy(H + o_n, len.data(), (size_t)ns * 4);
    memcpy(H + o_ser, serial.data(), (size_t)ns * 4);
    for (int i = 0; i < ns; i++) ((int64_t*)(H + o_kfid))[i] = ids[src[i]];
    ps_parallel_for(ns, a.off, [&](int i) {
      if (len[i] == 0) return;
      memcpy(H + o_id + (size_t)off[i] * 4, bow_id[src[i]], (size_t)len[i] * 4);
      memcpy(H + o_val + (size_t)off[i] * 8, bow_val[src[i]], (size_t)len[i] * 8);
    });
    uint8_t* D = m->d_buf;
    KfdbAddArrays A;
    A.S = db->S;
    A.slot = (const int32_t*)(D + o_slot); A.off = (const int32_t*)(D + o_off); A.n = (const int32_t*)(D + o_n);
    A.serial = (const uint32_t*)(D + o_ser); A.kfid = (const int64_t*)(D + o_kfid);
    A.src_id = (const int32_t*)(D + o_id); A.src_val = (const double*)(D + o_val);
    he = hipMemcpyAsync(D, H, a.off, hipMemcpyHostToDevice, m->stream);
    if (he == hipSuccess) { psk_kfdb_put_launch(&A, ns, m->stream); he = hipGetLastError(); }
    if (he == hipSuccess) he = hipStreamSynchronize(m->stream);
    if (he != hipSuccess) { undo(); return ps_set_error(PS_ERR_HIP, "ps_kfdb_add: %s", hipGetErrorString(he)); }
    for (int i = 0; i < ns; i++) {
      db->slot_of[ids[src[i]]] = slot[i];
      db->h_len[(size_t)slot[i]] = len[i]; db->h_serial[(size_t)slot[i]] = serial[i];
    }
    set_high(db);
  }
  if (nfail > 0)
    return ps_set_error(PS_ERR_CAPACITY, "ps_kfdb_add: entry %d (and %d more): more than %d words, or the database is full (%d keyframes)", first_fail, nfail - 1, db->max_words, db->capacity);
  return PS_OK;
}

int ps_kfdb_erase(ps_kfdb* db, const int64_t* ids, int n) {
  if (!db || n < 0 || (n > 0 && !ids)) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_erase: bad argument");
  std::lock_guard<std::mutex> lock(db->mu);
  const int high = db->S.high;
  bool any = false;
  for (int i = 0; i < n; i++) {
    const auto it = db->slot_of.find(ids[i]);
    if (it == db->slot_of.end()) continue;
    const int32_t s = it->second;
    db->h_len[(size_t)s] = 0; db->h_serial[(size_t)s] = 0;
    db->free_slots.insert(s);
    db->slot_of.erase(it);
    any = true;
  }
  if (!any) return PS_OK;
  set_high(db);
  return upload_state(db, high);
}

int ps_kfdb_clear(ps_kfdb* db) {
  if (!db) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_clear: null argument");
  std::lock_guard<std::mutex> lock(db->mu);
  const int high = db->S.high;
  db->slot_of.clear();
  db->free_slots.clear();
  for (int s = 0; s < db->capacity; s++) db->free_slots.insert(db->free_slots.end(), s);
  std::fill(db->h_len.begin(), db->h_len.end(), 0);
  std::fill(db->h_serial.begin(), db->h_serial.end(), 0u);
  db->next_serial = 1;
  db->S.high = 0;
  return upload_state(db, high);
}

int ps_kfdb_query(ps_kfdb* db, ps_matcher* m, ps_kfdb_query_problem* probs, int nprob) {
  if (!db || !m || !probs || nprob < 1 || nprob > 65535) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_query: bad argument");
  if (db->device != m->device) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_query: the database lives on device %d, the matcher on device %d", db->device, m->device);
  std::lock_guard<std::mutex> dlock(db->mu);
  const int live = (int)db->slot_of.size(), high = db->S.high;
  std::vector<int> served, failed;
  for (int p = 0; p < nprob; p++) {
    const ps_kfdb_query_problem& P = probs[p];
    if (P.n < 0 || (P.mode != 0 && P.mode != 1) || P.nexcluded < 0) return ps_set_error(PS_ERR_INVALID, "keyframe database query %d: bad sizes or mode", p);
    if (P.n > PS_KFDB_MAX_WORDS) { failed.push_back(p); continue; }
    if ((P.n > 0 && (!P.bow_id || !P.bow_val)) || (P.mode == 1 && P.nexcluded > 0 && !P.excluded) || (live > 0 && (!P.share_id || !P.share_words || !P.share_score)))
      return ps_set_error(PS_ERR_INVALID, "keyframe database query %d: null arrays", p);
    if (!ascending(P.bow_id, P.n)) return ps_set_error(PS_ERR_INVALID, "keyframe database query %d: word ids not ascending", p);
    served.push_back(p);
  }
  for (int p : failed) probs[p].nshare = -1;
  const int ns = (int)served.size();
  auto capacity_error = [&]() {
    return ps_set_error(PS_ERR_CAPACITY, "keyframe database query %d (and %zu more): more than %d words", failed[0], failed.size() - 1, PS_KFDB_MAX_WORDS);
  };
  if (ns == 0) return capacity_error();
  if (high == 0) {                                   // an empty database: lKFsSharingWords.empty()
    for (int p : served) { probs[p].nshare = 0; probs[p].min_common_words = 0; }
    return failed.empty() ? PS_OK : capacity_error();
  }
  // the queries, their exclusion bitmasks over the slots, and the order kfdb_list serves them in
  const size_t mask_words = ((size_t)high + 31) / 32;
  std::vector<KfdbQuery> hq(ns);
  std::vector<uint32_t> excl;
  std::vector<int32_t> order;
  size_t NW = 0;
  int longest = 0, nloop = 0;
  for (int s = 0; s < ns; s++) {
    const ps_kfdb_query_problem& P = probs[served[s]];
    hq[s] = KfdbQuery{(int32_t)NW, P.n, P.mode, -1};
    NW += (size_t)P.n;
    longest = std::max(longest, (int)P.n);
    if (P.mode != 1) continue;
    order.push_back(s);
    nloop++;
    bool any = false;
    for (int i = 0; i < P.nexcluded; i++) {
      const auto it = db->slot_of.find(P.excluded[i]);
      if (it == db->slot_of.end()) continue;
      if (!any) { hq[s].excl = (int32_t)excl.size(); excl.resize(excl.size() + mask_words, 0u); any = true; }
      excl[(size_t)hq[s].excl + ((size_t)it->second >> 5)] |= 1u << (it->second & 31);
    }
  }
  for (int s = 0; s < ns; s++) if (hq[s].mode == 0) order.push_back(s);
  const size_t Q = (size_t)ns, QH = Q * (size_t)high, QL = Q * (size_t)live;
  Arena a;
  const size_t o_q = a.take(sizeof(KfdbQuery) * Q), o_order = a.take(Q * 4), o_excl = a.take(excl.size() * 4), o_qid = a.take(NW * 4), o_qval = a.take(NW * 8);
  const size_t in_bytes = a.off;
  const size_t o_maxw = a.take(Q * 4), o_words = a.take(QH * 4), o_lcw = a.take(QH * 4), o_score = a.take(QH * 4);
  const size_t o_sid = a.take(QL * 8), o_sw = a.take(QL * 4), o_ss = a.take(QL * 4), o_ns = a.take(Q * 4), o_mc = a.take(Q * 4);
  const size_t out_end = a.off;
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  PS_TRY(psm_ensure(m, a.off));
  uint8_t* H = m->h_buf;
  memcpy(H + o_q, hq.data(), sizeof(KfdbQuery) * Q);
  memcpy(H + o_order, order.data(), Q * 4);
  if (!excl.empty()) memcpy(H + o_excl, excl.data(), excl.size() * 4);
  for (int s = 0; s < ns; s++) {
    const ps_kfdb_query_problem& P = probs[served[s]];
    if (P.n == 0) continue;
    memcpy(H + o_qid + (size_t)hq[s].off * 4, P.bow_id, (size_t)P.n * 4);
    memcpy(H + o_qval + (size_t)hq[s].off * 8, P.bow_val, (size_t)P.n * 8);
  }
  uint8_t* D = m->d_buf;
  PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
  PS_HIP(hipMemsetAsync(D + o_maxw, 0, Q * 4, m->stream));
  PS_TRY(psm_kernels_begin(m));
  KfdbQueryArrays A;
  A.S = db->S;
  A.q = (const KfdbQuery*)(D + o_q); A.qid = (const int32_t*)(D + o_qid); A.qval = (const double*)(D + o_qval);
  A.excl = (const uint32_t*)(D + o_excl); A.order = (const int32_t*)(D + o_order);
  A.nq = ns; A.nloop = nloop; A.out_stride = live;
  A.spw = (int32_t)std::min<size_t>(4, std::max<size_t>(1, QH / 4096));   // about a thousand workgroups before a wave takes a second slot
  A.words = (int32_t*)(D + o_words); A.lcw = (int32_t*)(D + o_lcw); A.score = (float*)(D + o_score); A.maxw = (int32_t*)(D + o_maxw);
  A.share_id = (int64_t*)(D + o_sid); A.share_words = (int32_t*)(D + o_sw); A.share_score = (float*)(D + o_ss);
  A.nshare = (int32_t*)(D + o_ns); A.mincw = (int32_t*)(D + o_mc);
  psk_kfdb_query_launch(&A, longest, m->stream);
  PS_TRY(psm_kernels_end(m));
  PS_HIP(hipMemcpyAsync(H + o_sid, D + o_sid, out_end - o_sid, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  PS_TRY(psm_kernels_ms(m));
  for (int s = 0; s < ns; s++) {
    ps_kfdb_query_problem& P = probs[served[s]];
    const size_t k = (size_t)s * (size_t)live;
    P.nshare = ((const int32_t*)(H + o_ns))[s];
    P.min_common_words = ((const int32_t*)(H + o_mc))[s];
    if (P.nshare <= 0) continue;
    memcpy(P.share_id, H + o_sid + k * 8, (size_t)P.nshare * 8);
    memcpy(P.share_words, H + o_sw + k * 4, (size_t)P.nshare * 4);
    memcpy(P.share_score, H + o_ss + k * 4, (size_t)P.nshare * 4);
  }
  return failed.empty() ? PS_OK : capacity_error();
}

int ps_kfdb_score(ps_kfdb* db, ps_matcher* m, const int32_t* bow_id, const double* bow_val, int bow_n, const int64_t* ids, int n, double* out) {
  if (!db || !m || bow_n < 0 || n < 0 || (bow_n > 0 && (!bow_id || !bow_val)) || (n > 0 && (!ids || !out))) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_score: bad argument");
  if (db->device != m->device) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_score: the database lives on device %d, the matcher on device %d", db->device, m->device);
  if (bow_n > PS_KFDB_MAX_WORDS) return ps_set_error(PS_ERR_CAPACITY, "ps_kfdb_score: more than %d words", PS_KFDB_MAX_WORDS);
  if (!ascending(bow_id, bow_n)) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_score: word ids not ascending");
  if (n == 0) return PS_OK;
  std::lock_guard<std::mutex> dlock(db->mu);
  std::vector<int32_t> slot((size_t)n);
  int unknown = 0;
  for (int i = 0; i < n; i++) {
    const auto it = db->slot_of.find(ids[i]);
    slot[(size_t)i] = it == db->slot_of.end() ? -1 : it->second;
    unknown += it == db->slot_of.end();
  }
  Arena a;
  const size_t o_slot = a.take((size_t)n * 4), o_qid = a.take((size_t)bow_n * 4), o_qval = a.take((size_t)bow_n * 8);
  const size_t in_bytes = a.off;
  const size_t o_out = a.take((size_t)n * 8);
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  PS_TRY(psm_ensure(m, a.off));
  uint8_t* H = m->h_buf;
  memcpy(H + o_slot, slot.data(), (size_t)n * 4);
  if (bow_n > 0) { memcpy(H + o_qid, bow_id, (size_t)bow_n * 4); memcpy(H + o_qval, bow_val, (size_t)bow_n * 8); }
  uint8_t* D = m->d_buf;
  PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
  PS_TRY(psm_kernels_begin(m));
  KfdbScoreArrays A;
  A.S = db->S;
  A.qid = (const int32_t*)(D + o_qid); A.qval = (const double*)(D + o_qval); A.qn = bow_n;
  A.slot = (const int32_t*)(D + o_slot); A.n = n; A.out = (double*)(D + o_out);
  psk_kfdb_score_launch(&A, m->stream);
  PS_TRY(psm_kernels_end(m));
  PS_HIP(hipMemcpyAsync(H + o_out, D + o_out, (size_t)n * 8, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  PS_TRY(psm_kernels_ms(m));
  memcpy(out, H + o_out, (size_t)n * 8);
  if (unknown > 0) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_score: %d of the ids are not stored", unknown);
  return PS_OK;
}

int ps_kfdb_select(int mode, float min_score, const int64_t* share_id, const int32_t* share_words, const float* share_score, int nshare,
                   int min_common_words, const int64_t* neigh, const int32_t* neigh_n, int64_t* cand_out, int32_t* ncand) {
  if (!ncand || nshare < 0 || (mode != 0 && mode != 1)) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_select: bad argument");
  *ncand = 0;
  if (nshare == 0) return PS_OK;
  if (!share_id || !share_words || !share_score || !neigh || !neigh_n || !cand_out) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_select: null argument");
  std::unordered_map<int64_t, int> at;                // mnLoopQuery == pKF->mnId / mnRelocQuery == F->mnId: the keyframe is in the list
  for (int i = 0; i < nshare; i++) at[share_id[i]] = i;
  std::vector<float> acc;                             // lAccScoreAndMatch
  std::vector<int64_t> best;
  float bestAccScore = mode == 1 ? min_score : 0.f;
  for (int i = 0; i < nshare; i++) {
    if (!(share_words[i] > min_common_words)) continue;
    if (mode == 1 && !(share_score[i] >= min_score)) continue;
    if (neigh_n[i] < 0 || neigh_n[i] > 10) return ps_set_error(PS_ERR_INVALID, "ps_kfdb_select: entry %d has %d neighbours", i, neigh_n[i]);
    float bestScore = share_score[i], accScore = share_score[i];
    int64_t pBestKF = share_id[i];
    for (int k = 0; k < neigh_n[i]; k++) {
      const auto it = at.find(neigh[(size_t)i * 10 + k]);
      if (it == at.end()) continue;
      const int j = it->second;
      if (mode == 1 && !(share_words[j] > min_common_words)) continue;
      accScore += share_score[j];
      if (share_score[j] > bestScore) { pBestKF = share_id[j]; bestScore = share_score[j]; }
    }
    acc.push_back(accScore); best.push_back(pBestKF);
    if (accScore > bestAccScore) bestAccScore = accScore;
  }
  const float minScoreToRetain = 0.75f * bestAccScore;
  std::unordered_set<int64_t> added;
  for (size_t i = 0; i < acc.size(); i++)
    if (acc[i] > minScoreToRetain && added.insert(best[i]).second) cand_out[(*ncand)++] = best[i];
  return PS_OK;
}

}  // extern "C"
