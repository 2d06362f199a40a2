// Helper of tools/kfdb_quick.py: a single-threaded host inverted file structured as the reference structures KeyFrameDatabase
// (a std::list of keyframes per word, std::map BowVectors, per-keyframe query / words / score fields), serving a
// relocalisation query up to the scored sharing list - the part ps_kfdb_query serves.  It is the yardstick the device call is
// timed against, not part of the library.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <vector>

namespace {
typedef std::map<unsigned, double> BowVector;
struct KF {
  BowVector bow;
  long query = -1;
  int words = 0;
  float score = 0;
};
struct DB {
  std::vector<std::list<KF*>> inverted;
  std::vector<KF*> kfs;
  long next_query = 0;
};
double l1score(const BowVector& v1, const BowVector& v2) {
  auto a = v1.begin();
  auto b = v2.begin();
  double score = 0;
  while (a != v1.end() && b != v2.end()) {
    if (a->first == b->first) { score += std::fabs(a->second - b->second) - std::fabs(a->second) - std::fabs(b->second); ++a; ++b; }
    else if (a->first < b->first) a = v1.lower_bound(b->first);
    else b = v2.lower_bound(a->first);
  }
  return -score / 2.0;
}
}  // namespace

extern "C" {
void* ivf_create(int nwords) {
  DB* d = new DB();
  d->inverted.resize((size_t)nwords);
  return d;
}
void ivf_destroy(void* h) {
  DB* d = (DB*)h;
  for (KF* k : d->kfs) delete k;
  delete d;
}
void ivf_add(void* h, const int32_t* id, const double* val, int n) {
  DB* d = (DB*)h;
  KF* k = new KF();
  for (int i = 0; i < n; i++) k->bow.insert(k->bow.end(), std::make_pair((unsigned)id[i], val[i]));
  for (const auto& kv : k->bow) d->inverted[kv.first].push_back(k);
  d->kfs.push_back(k);
}
// one relocalisation query, `reps` times: writes each repetition's milliseconds to ms[] and returns the number of keyframes the
// last one scored
int ivf_query(void* h, const int32_t* id, const double* val, int n, int reps, double* ms, int* nshare) {
  DB* d = (DB*)h;
  BowVector q;
  for (int i = 0; i < n; i++) q.insert(q.end(), std::make_pair((unsigned)id[i], val[i]));
  int scored = 0;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    const long qid = d->next_query++;
    std::list<KF*> sharing;
    for (const auto& kv : q)
      for (KF* k : d->inverted[kv.first]) {
        if (k->query != qid) { k->words = 0; k->query = qid; sharing.push_back(k); }
        k->words++;
      }
    int maxCommonWords = 0;
    for (KF* k : sharing) if (k->words > maxCommonWords) maxCommonWords = k->words;
    const int minCommonWords = maxCommonWords * 0.8f;
    scored = 0;
    for (KF* k : sharing)
      if (k->words > minCommonWords) { k->score = (float)l1score(q, k->bow); scored++; }
    *nshare = (int)sharing.size();
    ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return scored;
}
}
