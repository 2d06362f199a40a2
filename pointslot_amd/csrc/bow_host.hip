// Host side of the bag-of-words C-ABI (include/pointslot_hip.h): the vocabulary handle, ps_bow_transform and ps_search_by_bow.
// Replaces TemplatedVocabulary<FORB>::loadFromBinaryFile / transform (/root/reference/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h)
// and ORBmatcher::SearchByBoW (/root/reference/src/ORBmatcher.cc:280-410, :646-781).  The work of a call runs on the matcher
// handle's stream and arenas; the vocabulary is read-only device memory.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <iterator>
#include <mutex>
#include <string.h>
#include <string>
#include <vector>
#include "bow_plan.h"
#include "matcher_host.h"
#include "ps_common.h"
#include "vocab_file.h"

extern "C" {
void psk_bow_transform_launch(const BowTransformArrays*, int, hipStream_t);
void psk_bow_search_launch(const BowSearchArrays*, hipStream_t);
}

struct ps_vocabulary {
  int device = 0;
  int k = 0, L = 0, weighting = 0, nodes = 0, words = 0;
  uint8_t* d_slab = nullptr;
  BowTree tree = {};
};

extern "C" {

int ps_vocabulary_create(int device, int k, int L, int scoring, int weighting, int nnodes, const int32_t* parent, const uint8_t* desc,
                         const float* weight, const uint8_t* is_leaf, ps_vocabulary** out) {
  if (!out) return ps_set_error(PS_ERR_INVALID, "ps_vocabulary_create: null argument");
  *out = nullptr;
  if (nnodes > 0 && (!parent || !desc || !weight || !is_leaf)) return ps_set_error(PS_ERR_INVALID, "ps_vocabulary_create: null argument");
  const std::string bad = ps_vocab_check(k, L, scoring, weighting, nnodes, parent, is_leaf);
  if (!bad.empty()) return ps_set_error(PS_ERR_INVALID, "ps_vocabulary_create: %s", bad.c_str());
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ps_set_error(PS_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return ps_set_error(PS_ERR_INVALID, "bad device ordinal");
  // the tree in child-list order: the children of a node are one contiguous run of slots, in record order
  const size_t NN = (size_t)nnodes + 1;
  std::vector<int32_t> cnt(NN, 0), first(NN, 0), filled(NN, 0);
  for (int i = 0; i < nnodes; i++) cnt[parent[i]]++;
  int32_t run = 0, nwords = 0;
  for (size_t v = 0; v < NN; v++) {
    if (cnt[v] > 0xFFFFF) return ps_set_error(PS_ERR_INVALID, "ps_vocabulary_create: node %zu has %d children (at most 1048575)", v, cnt[v]);
    first[v] = run;
    run += cnt[v];
  }
  std::vector<BowSlot> slot((size_t)nnodes);
  std::vector<uint8_t> child_desc((size_t)nnodes * 32);
  std::vector<float> word_weight;
  for (int i = 0; i < nnodes; i++) {
    const size_t s = (size_t)first[parent[i]] + filled[parent[i]]++;
    slot[s].id = i + 1; slot[s].child_cnt = cnt[(size_t)i + 1]; slot[s].weight = weight[i];
    slot[s].off_or_word = first[(size_t)i + 1];
    memcpy(&child_desc[s * 32], desc + (size_t)i * 32, 32);
    if (is_leaf[i]) { slot[s].off_or_word = nwords++; word_weight.push_back(weight[i]); }
  }
  PS_HIP(hipSetDevice(device));
  Arena a;
  const size_t o_slot = a.take(sizeof(BowSlot) * (size_t)nnodes), o_cd = a.take((size_t)nnodes * 32), o_ww = a.take((size_t)nwords * 4);
  ps_vocabulary* v = new ps_vocabulary();
  v->device = device; v->k = k; v->L = L; v->weighting = weighting; v->nodes = (int)NN; v->words = nwords;
  hipError_t e = hipMalloc(&v->d_slab, a.off);
  if (e == hipSuccess) e = hipMemcpy(v->d_slab + o_slot, slot.data(), sizeof(BowSlot) * (size_t)nnodes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(v->d_slab + o_cd, child_desc.data(), (size_t)nnodes * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess && nwords > 0) e = hipMemcpy(v->d_slab + o_ww, word_weight.data(), (size_t)nwords * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (v->d_slab) hipFree(v->d_slab);
    delete v;
    return ps_set_error(PS_ERR_HIP, "ps_vocabulary_create: %s", hipGetErrorString(e));
  }
  v->tree.slot = (const BowSlot*)(v->d_slab + o_slot);
  v->tree.child_desc = v->d_slab + o_cd; v->tree.word_weight = (const float*)(v->d_slab + o_ww);
  v->tree.root_cnt = cnt[0]; v->tree.L = L; v->tree.weighting = weighting; v->tree.nodes = (int)NN; v->tree.words = nwords;
  *out = v;
  return PS_OK;
}

int ps_vocabulary_load_binary(int device, const char* path, ps_vocabulary** out) {
  if (!out || !path) return ps_set_error(PS_ERR_INVALID, "ps_vocabulary_load_binary: null argument");
  *out = nullptr;
  PsVocabFile F;
  const std::string bad = ps_vocab_file_read(path, F);
  if (!bad.empty()) return ps_set_error(PS_ERR_INVALID, "ps_vocabulary_load_binary: %s", bad.c_str());
  return ps_vocabulary_create(device, F.k, F.L, F.scoring, F.weighting, F.nnodes(), F.parent.data(), F.desc.data(), F.weight.data(), F.is_leaf.data(), out);
}

void ps_vocabulary_destroy(ps_vocabulary* v) {
  if (!v) return;
  hipSetDevice(v->device);
  if (v->d_slab) hipFree(v->d_slab);
  delete v;
}

int ps_vocabulary_info(const ps_vocabulary* v, int32_t* k, int32_t* L, int32_t* nodes, int32_t* words) {
  if (!v) return ps_set_error(PS_ERR_INVALID, "ps_vocabulary_info: null argument");
  if (k) *k = v->k;
  if (L) *L = v->L;
  if (nodes) *nodes = v->nodes;
  if (words) *words = v->words;
  return PS_OK;
}

int ps_bow_transform(ps_matcher* m, const ps_vocabulary* v, ps_bow_problem* probs, int nprob) {
  if (!m || !v || !probs || nprob < 1) return ps_set_error(PS_ERR_INVALID, "ps_bow_transform: bad argument");
  if (v->device != m->device) return ps_set_error(PS_ERR_INVALID, "ps_bow_transform: the vocabulary lives on device %d, the matcher on device %d", v->device, m->device);
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  std::vector<int> served, failed;
  for (int p = 0; p < nprob; p++) {
    const ps_bow_problem& P = probs[p];
    if (P.n < 0) return ps_set_error(PS_ERR_INVALID, "bag-of-words problem %d: negative count", p);
    if (P.n > PS_BOW_MAX_N) { failed.push_back(p); continue; }
    if (P.n > 0 && (!P.desc || !P.word || !P.node || !P.bow_id || !P.bow_val)) return ps_set_error(PS_ERR_INVALID, "bag-of-words problem %d: null arrays", p);
    served.push_back(p);
  }
  for (int p : failed) probs[p].bow_n = -1;
  const int ns = (int)served.size();
  if (ns == 0) return ps_set_error(PS_ERR_CAPACITY, "bag-of-words problem %d (and %zu more): more than %d features", failed[0], failed.size() - 1, PS_BOW_MAX_N);
  std::vector<BowFrame> hf(ns);
  size_t NF = 0;   // feature slots; every frame starts at a multiple of 16, the features of a workgroup of bow_walk
  for (int s = 0; s < ns; s++) {
    const ps_bow_problem& P = probs[served[s]];
    hf[s] = BowFrame{(int32_t)NF, P.n, P.levelsup, 0};
    NF += ((size_t)P.n + 15) / 16 * 16;
    if (NF > 0x7FFFFFF0ull) return ps_set_error(PS_ERR_CAPACITY, "ps_bow_transform: the batch holds more than 2^31 features");
  }
  const size_t NB = NF / 16;
  Arena a;
  const size_t o_frame = a.take(sizeof(BowFrame) * ns), o_ff = a.take(NB * 4), o_desc = a.take(NF * 32);
  const size_t in_bytes = a.off;
  const size_t o_word = a.take(NF * 4), o_node = a.take(NF * 4), o_id = a.take(NF * 4), o_n = a.take((size_t)ns * 4), o_val = a.take(NF * 8);
  const size_t out_end = a.off;
  PS_TRY(psm_ensure(m, a.off));
  uint8_t* H = m->h_buf;
  memcpy(H + o_frame, hf.data(), sizeof(BowFrame) * ns);
  ps_parallel_for(ns, in_bytes, [&](int s) {
    const ps_bow_problem& P = probs[served[s]];
    int32_t* ff = (int32_t*)(H + o_ff) + hf[s].f_off / 16;
    for (int b = 0; b < (P.n + 15) / 16; b++) ff[b] = s;
    if (P.n > 0) memcpy(H + o_desc + (size_t)hf[s].f_off * 32, P.desc, (size_t)P.n * 32);
  });
  uint8_t* D = m->d_buf;
  PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
  PS_TRY(psm_kernels_begin(m));
  BowTransformArrays A;
  A.tree = v->tree;
  A.frame = (const BowFrame*)(D + o_frame); A.desc = D + o_desc; A.feat_frame = (const int32_t*)(D + o_ff);
  A.word = (int32_t*)(D + o_word); A.node = (int32_t*)(D + o_node); A.bow_id = (int32_t*)(D + o_id); A.bow_val = (double*)(D + o_val);
  A.bow_n = (int32_t*)(D + o_n); A.nblocks16 = (int32_t)NB;
  psk_bow_transform_launch(&A, ns, m->stream);
  PS_TRY(psm_kernels_end(m));
  PS_HIP(hipMemcpyAsync(H + o_word, D + o_word, out_end - o_word, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  PS_TRY(psm_kernels_ms(m));
  ps_parallel_for(ns, out_end - o_word, [&](int s) {
    ps_bow_problem& P = probs[served[s]];
    const size_t f = (size_t)hf[s].f_off;
    P.bow_n = ((const int32_t*)(H + o_n))[s];
    if (P.n == 0) return;
    memcpy(P.word, H + o_word + f * 4, (size_t)P.n * 4);
    memcpy(P.node, H + o_node + f * 4, (size_t)P.n * 4);
    if (P.bow_n > 0) { memcpy(P.bow_id, H + o_id + f * 4, (size_t)P.bow_n * 4); memcpy(P.bow_val, H + o_val + f * 8, (size_t)P.bow_n * 8); }
  });
  if (!failed.empty())
    return ps_set_error(PS_ERR_CAPACITY, "bag-of-words problem %d (and %zu more): more than %d features", failed[0], failed.size() - 1, PS_BOW_MAX_N);
  return PS_OK;
}

}  // extern "C"

namespace {
bool bow_side_ok(const ps_bow_side& S, bool need_points) {
  if (S.n <= 0) return S.n == 0;
  return S.desc && S.angle && S.node && (!need_points || S.has_point);
}
// what one search problem contributes to the batch: the bucket lists of both sides and one item per common node
struct BowSearchPlan {
  std::vector<int32_t> lst;         // side a's buckets, then side b's
  std::vector<BowSItem> items;      // offsets relative to lst
};
// the features of a side bucketed by the common nodes: a counting sort, stable in the feature index
void bow_bucket(const ps_bow_side& S, const std::vector<int32_t>& common, std::vector<int32_t>& start, std::vector<int32_t>& out) {
  const int nu = (int)common.size();
  std::vector<int32_t> where((size_t)S.n, -1);
  start.assign((size_t)nu + 1, 0);
  for (int j = 0; j < S.n; j++) {
    const int32_t v = S.node[j];
    if (v < 0) continue;
    const auto it = std::lower_bound(common.begin(), common.end(), v);
    if (it == common.end() || *it != v) continue;
    where[j] = (int32_t)(it - common.begin());
    start[(size_t)where[j] + 1]++;
  }
  for (int c = 0; c < nu; c++) start[(size_t)c + 1] += start[c];
  out.assign((size_t)start[nu], 0);
  std::vector<int32_t> slot(start.begin(), start.end() - 1);
  for (int j = 0; j < S.n; j++)
    if (where[j] >= 0) out[(size_t)slot[where[j]]++] = j;
}
std::vector<int32_t> bow_nodes_of(const ps_bow_side& S) {
  std::vector<int32_t> un;
  for (int i = 0; i < S.n; i++) if (S.node[i] >= 0) un.push_back(S.node[i]);
  std::sort(un.begin(), un.end());
  un.erase(std::unique(un.begin(), un.end()), un.end());
  return un;
}
}  // namespace

extern "C" int ps_search_by_bow(ps_matcher* m, ps_bow_search_problem* probs, int nprob) {
  if (!m || !probs || nprob < 1) return ps_set_error(PS_ERR_INVALID, "ps_search_by_bow: bad argument");
  std::lock_guard<std::mutex> lock(m->mu);
  PS_HIP(hipSetDevice(m->device));
  std::vector<int> served, failed;
  for (int p = 0; p < nprob; p++) {
    const ps_bow_search_problem& P = probs[p];
    if (P.a.n < 0 || P.b.n < 0 || (P.mode != 0 && P.mode != 1)) return ps_set_error(PS_ERR_INVALID, "SearchByBoW problem %d: bad sizes or mode", p);
    if (P.a.n > PS_BOW_MAX_N || P.b.n > PS_BOW_MAX_N) { failed.push_back(p); continue; }
    if (!bow_side_ok(P.a, true) || !bow_side_ok(P.b, P.mode == 1)) return ps_set_error(PS_ERR_INVALID, "SearchByBoW problem %d: null arrays", p);
    if ((P.mode == 0 ? P.b.n : P.a.n) > 0 && !P.match) return ps_set_error(PS_ERR_INVALID, "SearchByBoW problem %d: null output array", p);
    served.push_back(p);
  }
  for (int p : failed) probs[p].nmatches = -1;
  const int ns = (int)served.size();
  if (ns == 0) return ps_set_error(PS_ERR_CAPACITY, "SearchByBoW problem %d (and %zu more): more than %d features on a side", failed[0], failed.size() - 1, PS_BOW_MAX_N);
  std::vector<BowSearchPlan> plan(ns);
  ps_parallel_for(ns, (size_t)ns << 16, [&](int s) {
    const ps_bow_search_problem& P = probs[served[s]];
    const std::vector<int32_t> na = bow_nodes_of(P.a), nb = bow_nodes_of(P.b);
    std::vector<int32_t> common;
    std::set_intersection(na.begin(), na.end(), nb.begin(), nb.end(), std::back_inserter(common));
    std::vector<int32_t> sa, sb, la, lb;
    bow_bucket(P.a, common, sa, la);
    bow_bucket(P.b, common, sb, lb);
    BowSearchPlan& pl = plan[s];
    pl.lst = la;
    pl.lst.insert(pl.lst.end(), lb.begin(), lb.end());
    const int32_t base_b = (int32_t)la.size();
    pl.items.resize(common.size());
    for (size_t c = 0; c < common.size(); c++) {
      BowSItem& I = pl.items[c];
      memset(&I, 0, sizeof(I));
      I.prob = s; I.a0 = sa[c]; I.a1 = sa[c + 1]; I.b0 = base_b + sb[c]; I.b1 = base_b + sb[c + 1];
    }
  });
  std::vector<BowSProb> hp(ns);
  std::vector<size_t> lst_off(ns), item_off(ns);
  size_t NF = 0, NO = 0, NL = 0, NI = 0;
  for (int s = 0; s < ns; s++) {
    const ps_bow_search_problem& P = probs[served[s]];
    BowSProb& d = hp[s];
    memset(&d, 0, sizeof(d));
    d.a_off = (int32_t)NF; d.a_n = P.a.n; NF += (size_t)P.a.n;
    d.b_off = (int32_t)NF; d.b_n = P.b.n; NF += (size_t)P.b.n;
    d.mode = P.mode; d.check_ori = P.check_orientation ? 1 : 0; d.nn_ratio = P.nn_ratio;
    d.out_off = (int32_t)NO; d.out_n = P.mode == 0 ? P.b.n : P.a.n; NO += (size_t)d.out_n;
    lst_off[s] = NL; NL += plan[s].lst.size();
    item_off[s] = NI; NI += plan[s].items.size();
    if (NF > 0x7FFFFFF0ull || NI > 0x7FFFFFF0ull) return ps_set_error(PS_ERR_CAPACITY, "ps_search_by_bow: the batch holds more than 2^31 features");
  }
  Arena a;
  const size_t o_prob = a.take(sizeof(BowSProb) * ns), o_item = a.take(sizeof(BowSItem) * NI), o_lst = a.take(NL * 4);
  const size_t o_desc = a.take(NF * 32), o_ang = a.take(NF * 4), o_hasp = a.take(NF);
  const size_t in_bytes = a.off;
  const size_t o_match = a.take(NO * 4), o_nm = a.take((size_t)ns * 4);
  const size_t out_end = a.off;
  PS_TRY(psm_ensure(m, a.off));
  uint8_t* H = m->h_buf;
  memcpy(H + o_prob, hp.data(), sizeof(BowSProb) * ns);
  ps_parallel_for(ns, in_bytes, [&](int s) {
    const ps_bow_search_problem& P = probs[served[s]];
    const BowSearchPlan& pl = plan[s];
    if (!pl.lst.empty()) memcpy(H + o_lst + lst_off[s] * 4, pl.lst.data(), pl.lst.size() * 4);
    BowSItem* it = (BowSItem*)(H + o_item) + item_off[s];
    for (size_t c = 0; c < pl.items.size(); c++) {
      it[c] = pl.items[c];
      it[c].a0 += (int32_t)lst_off[s]; it[c].a1 += (int32_t)lst_off[s]; it[c].b0 += (int32_t)lst_off[s]; it[c].b1 += (int32_t)lst_off[s];
    }
    for (int side = 0; side < 2; side++) {
      const ps_bow_side& S = side ? P.b : P.a;
      const size_t f = (size_t)(side ? hp[s].b_off : hp[s].a_off), n = (size_t)S.n;
      if (n == 0) continue;
      memcpy(H + o_desc + f * 32, S.desc, n * 32);
      memcpy(H + o_ang + f * 4, S.angle, n * 4);
      if (S.has_point) memcpy(H + o_hasp + f, S.has_point, n); else memset(H + o_hasp + f, 0, n);
    }
  });
  if (NL > 0x7FFFFFF0ull) return ps_set_error(PS_ERR_CAPACITY, "ps_search_by_bow: the batch holds more than 2^31 features");
  uint8_t* D = m->d_buf;
  PS_HIP(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, m->stream));
  if (NO > 0) PS_HIP(hipMemsetAsync(D + o_match, 0xFF, NO * 4, m->stream));   // -1 everywhere: vector<MapPoint*>(N, NULL)
  PS_TRY(psm_kernels_begin(m));
  BowSearchArrays A;
  A.prob = (const BowSProb*)(D + o_prob); A.item = (const BowSItem*)(D + o_item);
  A.desc = D + o_desc; A.ang = (const float*)(D + o_ang); A.hasp = D + o_hasp; A.lst = (const int32_t*)(D + o_lst);
  A.match = (int32_t*)(D + o_match); A.nmatch = (int32_t*)(D + o_nm); A.nitems = (int32_t)NI; A.nprob = ns;
  psk_bow_search_launch(&A, m->stream);
  PS_TRY(psm_kernels_end(m));
  PS_HIP(hipMemcpyAsync(H + o_match, D + o_match, out_end - o_match, hipMemcpyDeviceToHost, m->stream));
  PS_HIP(hipStreamSynchronize(m->stream));
  PS_TRY(psm_kernels_ms(m));
  for (int s = 0; s < ns; s++) {
    ps_bow_search_problem& P = probs[served[s]];
    P.nmatches = ((const int32_t*)(H + o_nm))[s];
    if (hp[s].out_n > 0) memcpy(P.match, H + o_match + (size_t)hp[s].out_off * 4, (size_t)hp[s].out_n * 4);
  }
  if (!failed.empty())
    return ps_set_error(PS_ERR_CAPACITY, "SearchByBoW problem %d (and %zu more): more than %d features on a side", failed[0], failed.size() - 1, PS_BOW_MAX_N);
  return PS_OK;
}
