// How the calls on a matcher handle lay out their arenas, and the searched ("train") side of the windowed matchers described once:
// where x, y, octave, angle, u_right, the descriptors and the grids of a batch lie, how a caller's ps_proj_train is copied there, and
// which byte ranges a call whose frame handles stage all of that on the device leaves out of its upload.  Host only, no HIP include:
// tests/cpp/search_side_check.cpp builds this header alone under the host sanitizers.
#pragma once
#include <algorithm>
#include <string.h>
#include "../../include/pointslot_hip.h"

inline size_t al(size_t v) { return (v + 255) / 256 * 256; }
struct Arena {   // slots handed out in order, each rounded up to 256 bytes behind 64 bytes of slack
  size_t off = 0;
  size_t take(size_t bytes) { const size_t r = off; off += al(bytes + 64); return r; }
};
template <typename T> inline T* ptr(uint8_t* base, size_t off) { return reinterpret_cast<T*>(base + off); }

constexpr int PS_SIDE_NCELL = 64 * 48;   // PS_GRID_COLS * PS_GRID_ROWS of match_plan.h (search_host.hip asserts it)
enum : unsigned { SIDE_ANG = 1, SIDE_UR = 2, SIDE_GRID = 4 };   // the arrays of a side beyond x, y, octave and the descriptors
struct SideSkip { struct { size_t lo, hi; } r[2]; int n; };       // what a fully staged call does not upload

struct SideOff {
  size_t x = 0, y = 0, oct = 0, ang = 0, ur = 0, desc = 0, coff = 0, cidx = 0, keys_end = 0, grid_end = 0;
  unsigned has = 0;   // the SIDE_ slots taken (frame_stage fills every one of them)
  void take_keys(Arena& a, size_t NT, unsigned which) {   // x .. desc of NT features
    has |= which & (SIDE_ANG | SIDE_UR);
    x = a.take(NT * 4); y = a.take(NT * 4); oct = a.take(NT * 4);
    ang = (which & SIDE_ANG) ? a.take(NT * 4) : 0; ur = (which & SIDE_UR) ? a.take(NT * 4) : 0;
    desc = a.take(NT * 32); keys_end = a.off;
  }
  void take_grid(Arena& a, size_t NT, size_t nj) {         // the grids of nj problems over those features
    has |= SIDE_GRID;
    coff = a.take(nj * (PS_SIDE_NCELL + 1) * 4); cidx = a.take(NT * 4); grid_end = a.off;
  }
  SideSkip skip() const {   // exactly the slots above: one range where nothing lies between x .. desc and the grid
    if (!(has & SIDE_GRID) || keys_end == coff) return SideSkip{{{x, (has & SIDE_GRID) ? grid_end : keys_end}, {0, 0}}, 1};
    return SideSkip{{{x, keys_end}, {coff, grid_end}}, 2};
  }
};

// The three layouts, from the first slot of the searched side to the last (the library and the check call these same functions).
struct PjSide { SideOff t; size_t occ, bbox; };   // projection: occupied and in_bbox, host arrays in every call, lie before the grid
inline PjSide pj_side_layout(Arena& a, size_t NT, size_t nprob) {
  PjSide s; s.t.take_keys(a, NT, SIDE_ANG | SIDE_UR); s.occ = a.take(NT); s.bbox = a.take(NT); s.t.take_grid(a, NT, nprob); return s;
}
inline SideOff fu_side_layout(Arena& a, size_t NT, size_t nprob) {   // fuse: no angle
  SideOff t; t.take_keys(a, NT, SIDE_UR); t.take_grid(a, NT, nprob); return t;
}
struct KsSide { SideOff t; size_t occ; };          // kf_search / Sim3: occupied (host array) behind the grid
inline KsSide ks_side_layout(Arena& a, size_t NT, size_t nj) {
  KsSide s; s.t.take_keys(a, NT, SIDE_ANG | SIDE_UR); s.t.take_grid(a, NT, nj); s.occ = a.take(NT); return s;
}

// One ps_proj_train into its slices: x .. desc at feature t0, the grid at cell_off entry grid_off.  `which`: the optional arrays this
// caller has (a null angle counts as zeros).  The cell_idx copy stops at min(cell_off[NCELL], n) entries whatever the grid claims and
// the entries behind it are zero.  zeroed: the caller has zeroed the buffer, so nothing is zeroed here.
inline void side_pack(uint8_t* H, const SideOff& o, const ps_proj_train& T, size_t t0, size_t grid_off, unsigned which, bool zeroed) {
  const size_t n = T.n > 0 ? (size_t)T.n : 0, grid_bytes = (size_t)(PS_SIDE_NCELL + 1) * 4;
  if (n == 0 && (which & SIDE_GRID) && !zeroed) memset(H + o.coff + grid_off * 4, 0, grid_bytes);
  if (n == 0) return;
  memcpy(H + o.x + t0 * 4, T.x, n * 4); memcpy(H + o.y + t0 * 4, T.y, n * 4);
  memcpy(H + o.oct + t0 * 4, T.octave, n * 4); memcpy(H + o.desc + t0 * 32, T.desc, n * 32);
  if ((which & SIDE_ANG) && T.angle) memcpy(H + o.ang + t0 * 4, T.angle, n * 4);
  else if ((which & SIDE_ANG) && !zeroed) memset(H + o.ang + t0 * 4, 0, n * 4);
  if (which & SIDE_UR) memcpy(H + o.ur + t0 * 4, T.u_right, n * 4);
  if (!(which & SIDE_GRID)) return;
  const size_t filled = std::min((size_t)T.cell_off[PS_SIDE_NCELL], n);
  memcpy(H + o.coff + grid_off * 4, T.cell_off, grid_bytes);
  memcpy(H + o.cidx + t0 * 4, T.cell_idx, filled * 4);
  if (!zeroed && filled < n) memset(H + o.cidx + (t0 + filled) * 4, 0, (n - filled) * 4);
}

// the slots as frame_stage's destination (Dst: FrameStageDst) ...
template <typename Dst> inline Dst side_stage_dst(const SideOff& o, uint8_t* D, int32_t* status) {
  Dst d = {};
  d.tx = ptr<float>(D, o.x); d.ty = ptr<float>(D, o.y); d.toct = ptr<int32_t>(D, o.oct); d.tdesc = D + o.desc; d.status = status;
  d.tang = (o.has & SIDE_ANG) ? ptr<float>(D, o.ang) : nullptr; d.tur = (o.has & SIDE_UR) ? ptr<float>(D, o.ur) : nullptr;
  if (o.has & SIDE_GRID) { d.cell_off = ptr<int32_t>(D, o.coff); d.cell_idx = ptr<int32_t>(D, o.cidx); }
  return d;
}
// ... and as the kernels read them (A: PjArrays, FuArrays, KsArrays; tang and tur stay with the callers whose kernels read them)
template <typename A> inline void side_arrays(A& a, const SideOff& o, uint8_t* D) {
  a.tx = ptr<float>(D, o.x); a.ty = ptr<float>(D, o.y); a.toct = ptr<int32_t>(D, o.oct); a.tdesc = D + o.desc;
  a.cell_off = ptr<int32_t>(D, o.coff); a.cell_idx = ptr<int32_t>(D, o.cidx);
}
