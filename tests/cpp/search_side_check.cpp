// Stand-alone check of pointslot_amd/csrc/search_side.h (host only; built with -fsanitize=address,undefined by
// tests/test_kfsearch_cpu.py): the arena stride, the three searched-side layouts and their skip ranges, and side_pack on a batch
// whose expected bytes are written out by hand - including a grid that claims more entries than the side has features.
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "search_side.h"

static int checks = 0, failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    checks++;                                                                \
    if (!(cond)) { failures++; printf("FAILED line %d: %s\n", __LINE__, #cond); } \
  } while (0)

static const int NC = 64 * 48;
static size_t stride(size_t bytes) { return (bytes + 64 + 255) / 256 * 256; }   // al(bytes + 64), spelled out again

// the slots frame_stage fills, as [lo, hi) intervals merged where they touch
static std::vector<std::pair<size_t, size_t>> staged_span(const SideOff& t, size_t NT, size_t nj) {
  std::vector<std::pair<size_t, size_t>> v = {{t.x, t.x + stride(NT * 4)}, {t.y, t.y + stride(NT * 4)}, {t.oct, t.oct + stride(NT * 4)},
                                              {t.desc, t.desc + stride(NT * 32)}};
  if (t.has & SIDE_ANG) v.push_back({t.ang, t.ang + stride(NT * 4)});
  if (t.has & SIDE_UR) v.push_back({t.ur, t.ur + stride(NT * 4)});
  if (t.has & SIDE_GRID) { v.push_back({t.coff, t.coff + stride(nj * (NC + 1) * 4)}); v.push_back({t.cidx, t.cidx + stride(NT * 4)}); }
  std::sort(v.begin(), v.end());
  std::vector<std::pair<size_t, size_t>> m;
  for (const auto& r : v) {
    if (!m.empty() && m.back().second == r.first) m.back().second = r.second; else m.push_back(r);
  }
  return m;
}
static bool skip_is(const SideSkip& s, const std::vector<std::pair<size_t, size_t>>& want) {
  if ((size_t)s.n != want.size()) return false;
  for (int i = 0; i < s.n; i++)
    if (s.r[i].lo != want[i].first || s.r[i].hi != want[i].second) return false;
  return true;
}

struct Dst { float* tx; float* ty; int32_t* toct; float* tang; float* tur; uint8_t* tdesc; int32_t* cell_off; int32_t* cell_idx; int32_t* status; };
struct Arrays { const float* tx; const float* ty; const int32_t* toct; const uint8_t* tdesc; const int32_t* cell_off; const int32_t* cell_idx; };

template <typename T> static void put(std::vector<uint8_t>& buf, size_t off, std::initializer_list<T> v) {
  size_t i = 0;
  for (T e : v) memcpy(&buf[off + (i++) * sizeof(T)], &e, sizeof(T));
}

int main() {
  // ---- the stride ----
  Arena a0;
  CHECK(a0.take(0) == 0 && a0.off == 256);
  CHECK(a0.take(192) == 256 && a0.off == 512);
  CHECK(a0.take(193) == 512 && a0.off == 1024);
  CHECK(al(0) == 0 && al(1) == 256 && al(256) == 256 && al(257) == 512);

  // ---- the three layouts: slot order, strides, and skip ranges = exactly the staged slots ----
  const size_t NT = 5, NJ = 3, first = stride(100);
  {
    Arena a; a.take(100);
    const PjSide s = pj_side_layout(a, NT, NJ);
    const size_t q = a.take(7);
    size_t o = first;
    CHECK(s.t.x == o); o += stride(NT * 4);
    CHECK(s.t.y == o); o += stride(NT * 4);
    CHECK(s.t.oct == o); o += stride(NT * 4);
    CHECK(s.t.ang == o); o += stride(NT * 4);
    CHECK(s.t.ur == o); o += stride(NT * 4);
    CHECK(s.t.desc == o); o += stride(NT * 32);
    CHECK(s.occ == o); o += stride(NT);
    CHECK(s.bbox == o); o += stride(NT);
    CHECK(s.t.coff == o); o += stride(NJ * (NC + 1) * 4);
    CHECK(s.t.cidx == o); o += stride(NT * 4);
    CHECK(q == o);
    const auto want = staged_span(s.t, NT, NJ);
    CHECK(want.size() == 2 && want[0].second == s.occ && want[1].first == s.bbox + stride(NT) && want[1].second == q);
    CHECK(skip_is(s.t.skip(), want));
  }
  {
    Arena a; a.take(100);
    const SideOff t = fu_side_layout(a, NT, NJ);
    const size_t q = a.take(7);
    CHECK(t.x == first && t.ur == first + 3 * stride(NT * 4) && t.desc == t.ur + stride(NT * 4) && t.coff == t.desc + stride(NT * 32));
    CHECK(!(t.has & SIDE_ANG) && (t.has & SIDE_UR) && (t.has & SIDE_GRID));
    const auto want = staged_span(t, NT, NJ);
    CHECK(want.size() == 1 && want[0].first == first && want[0].second == q);
    CHECK(skip_is(t.skip(), want));
    uint8_t base[1];
    const Dst d = side_stage_dst<Dst>(t, base, nullptr);
    CHECK(d.tang == nullptr && d.tur == (float*)(base + t.ur) && d.cell_idx == (int32_t*)(base + t.cidx) && d.tdesc == base + t.desc);
    Arrays A;
    side_arrays(A, t, base);
    CHECK(A.tx == (const float*)(base + t.x) && A.toct == (const int32_t*)(base + t.oct) && A.cell_off == (const int32_t*)(base + t.coff));
  }
  {
    Arena a; a.take(100);
    const KsSide s = ks_side_layout(a, NT, NJ);
    const size_t q = a.take(7);
    CHECK(s.t.ang == first + 3 * stride(NT * 4) && s.t.ur == s.t.ang + stride(NT * 4) && s.occ == s.t.cidx + stride(NT * 4) && q == s.occ + stride(NT));
    const auto want = staged_span(s.t, NT, NJ);
    CHECK(want.size() == 1 && want[0].first == first && want[0].second == s.occ);
    CHECK(skip_is(s.t.skip(), want));
  }
  {
    Arena a; a.take(100);
    SideOff t;                          // the triangulation's keys: no grid
    t.take_keys(a, NT, SIDE_ANG | SIDE_UR);
    CHECK(skip_is(t.skip(), staged_span(t, NT, NJ)) && t.skip().n == 1 && t.skip().r[0].hi == a.off);
    uint8_t base[1];
    const Dst d = side_stage_dst<Dst>(t, base, nullptr);
    CHECK(d.cell_off == nullptr && d.cell_idx == nullptr && d.tang == (float*)(base + t.ang));
  }

  // ---- side_pack: three sides (n = 3, 0, 2) in the projection layout, buffer not zeroed by the caller ----
  {
    Arena a; a.take(100);
    const PjSide s = pj_side_layout(a, NT, NJ);
    a.take(7);
    std::vector<uint8_t> buf(a.off, 0xA5), want(a.off, 0xA5);
    // side 0: three features, cell 5 holds features 2 and 0, cell 100 holds feature 1
    const float x0[3] = {1.5f, 2.5f, 3.5f}, y0[3] = {-1.f, -2.f, -3.f}, ang0[3] = {10.f, 20.f, 30.f}, ur0[3] = {-1.f, 0.25f, 7.f};
    const int32_t oct0[3] = {0, 3, 7}, idx0[3] = {2, 0, 1};
    uint8_t desc0[96];
    for (int i = 0; i < 96; i++) desc0[i] = (uint8_t)(i + 1);
    std::vector<int32_t> coff0(NC + 1);
    for (int c = 0; c <= NC; c++) coff0[c] = c <= 5 ? 0 : c <= 100 ? 2 : 3;
    ps_proj_train T0 = {};
    T0.n = 3; T0.x = x0; T0.y = y0; T0.octave = oct0; T0.angle = ang0; T0.u_right = ur0; T0.desc = desc0; T0.cell_off = coff0.data(); T0.cell_idx = idx0;
    // side 1: empty, every pointer null
    ps_proj_train T1 = {};
    // side 2: two features, and a grid that claims five entries; cell_idx holds exactly two, on the heap, so an over-read is caught
    const float x2[2] = {100.f, 200.f}, y2[2] = {300.f, 400.f}, ang2[2] = {1.f, 2.f}, ur2[2] = {3.f, 4.f};
    const int32_t oct2[2] = {1, 2};
    uint8_t desc2[64];
    for (int i = 0; i < 64; i++) desc2[i] = (uint8_t)(200 - i);
    std::vector<int32_t> coff2(NC + 1);
    for (int c = 0; c <= NC; c++) coff2[c] = c <= 7 ? 0 : 5;
    int32_t* idx2 = new int32_t[2];
    idx2[0] = 1; idx2[1] = 0;
    ps_proj_train T2 = {};
    T2.n = 2; T2.x = x2; T2.y = y2; T2.octave = oct2; T2.angle = ang2; T2.u_right = ur2; T2.desc = desc2; T2.cell_off = coff2.data(); T2.cell_idx = idx2;
    const unsigned all = SIDE_ANG | SIDE_UR | SIDE_GRID;
    side_pack(buf.data(), s.t, T0, 0, 0, all, false);
    side_pack(buf.data(), s.t, T1, 3, (size_t)(NC + 1), all, false);
    side_pack(buf.data(), s.t, T2, 3, (size_t)2 * (NC + 1), all, false);
    delete[] idx2;
    // the expected bytes, by hand: features 0..2 are side 0's, 3..4 side 2's
    put<float>(want, s.t.x, {1.5f, 2.5f, 3.5f, 100.f, 200.f});
    put<float>(want, s.t.y, {-1.f, -2.f, -3.f, 300.f, 400.f});
    put<int32_t>(want, s.t.oct, {0, 3, 7, 1, 2});
    put<float>(want, s.t.ang, {10.f, 20.f, 30.f, 1.f, 2.f});
    put<float>(want, s.t.ur, {-1.f, 0.25f, 7.f, 3.f, 4.f});
    for (int i = 0; i < 96; i++) want[s.t.desc + i] = (uint8_t)(i + 1);
    for (int i = 0; i < 64; i++) want[s.t.desc + 96 + i] = (uint8_t)(200 - i);
    put<int32_t>(want, s.t.cidx, {2, 0, 1, 1, 0});
    for (int c = 0; c <= NC; c++) {
      put<int32_t>(want, s.t.coff + (size_t)c * 4, {c <= 5 ? 0 : c <= 100 ? 2 : 3});
      put<int32_t>(want, s.t.coff + ((size_t)(NC + 1) + c) * 4, {0});
      put<int32_t>(want, s.t.coff + ((size_t)2 * (NC + 1) + c) * 4, {c <= 7 ? 0 : 5});
    }
    CHECK(buf == want);                 // every slice, and 0xA5 everywhere else (occupied, in_bbox and the slack included)
    CHECK(buf[s.occ] == 0xA5 && buf[s.bbox] == 0xA5 && buf[s.t.cidx + 20] == 0xA5 && buf[s.t.x + 20] == 0xA5);
  }

  // ---- side_pack: a grid with fewer entries than features, and a null angle (kf_search layout) ----
  for (int zeroed = 0; zeroed < 2; zeroed++) {
    Arena a;
    const KsSide s = ks_side_layout(a, 3, 1);
    std::vector<uint8_t> buf(a.off, 0xA5), want(a.off, 0xA5);
    const float x[3] = {1.f, 2.f, 3.f}, y[3] = {4.f, 5.f, 6.f};
    const int32_t oct[3] = {2, 1, 0};
    uint8_t desc[96];
    memset(desc, 0x3C, sizeof desc);
    std::vector<int32_t> coff(NC + 1);
    for (int c = 0; c <= NC; c++) coff[c] = c <= 9 ? 0 : 1;
    int32_t* idx = new int32_t[1];
    idx[0] = 2;
    ps_proj_train T = {};
    T.n = 3; T.x = x; T.y = y; T.octave = oct; T.desc = desc; T.cell_off = coff.data(); T.cell_idx = idx;
    side_pack(buf.data(), s.t, T, 0, 0, SIDE_ANG | SIDE_GRID, zeroed != 0);
    delete[] idx;
    put<float>(want, s.t.x, {1.f, 2.f, 3.f});
    put<float>(want, s.t.y, {4.f, 5.f, 6.f});
    put<int32_t>(want, s.t.oct, {2, 1, 0});
    memset(&want[s.t.desc], 0x3C, 96);
    for (int c = 0; c <= NC; c++) put<int32_t>(want, s.t.coff + (size_t)c * 4, {c <= 9 ? 0 : 1});
    put<int32_t>(want, s.t.cidx, {2});
    if (!zeroed) {                      // the tail behind the grid's entries and the absent angle are zeroed here ...
      put<int32_t>(want, s.t.cidx + 4, {0, 0});
      put<float>(want, s.t.ang, {0.f, 0.f, 0.f});
    }                                   // ... or left to the caller's memset; u_right is not this caller's to fill either way
    CHECK(buf == want);
  }

  if (failures) { printf("%d of %d checks FAILED\n", failures, checks); return 1; }
  printf("ok %d checks\n", checks);
  return 0;
}
