// The ray caster of the generated drive sequences (pointslot_amd/sequence.py: _render / _sample) as plain host C++: the same IEEE double
// operations per pixel, in the same order, as the numpy statement it stands in for, so that both give the same bits (built with
// -ffp-contract=off; tests/test_sequence_render_cpu.py compares them).  Host code only - no part of libpointslot_hip.so; it exists because
// the numpy form costs 0.1 - 0.2 s per image and a benchmark run renders thousands of them before its first step.
//
// What is separable is hoisted: the ray direction's x / z depend on the column only and its y on the row only, hence the plane distances
// of ground and ceiling are per row, those of the walls, the end wall and the object faces per column.  Every pixel walks the planes in the
// order of the numpy form (a later plane wins only where it is strictly nearer), then samples the texture of the winner once.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace {

struct Mip { const double* p; int64_t h, w; };

inline int64_t wrap(int64_t i, int64_t n) {      // mirror tiling: ... 2 1 0 | 0 1 2 ... n-1 | n-1 n-2 ...
  int64_t m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

// bilinear lookup, mip level by the pixel footprint in texels; *uncertain counts footprints so close to a level boundary that another
// log2 could round the other way (the caller then renders that image with the numpy form)
inline double sample(const Mip* mips, int levels, double u, double v, double foot, int64_t* uncertain) {
  double l = std::log2(foot > 1.0 ? foot : 1.0) + 0.5;
  if (std::fabs(l - std::nearbyint(l)) < 1e-9) ++*uncertain;
  double lf = std::floor(l);
  if (lf < 0.0) lf = 0.0;
  if (lf > double(levels - 1)) lf = double(levels - 1);
  int lv = int(lf);
  const Mip& t = mips[lv];
  double div = double(int64_t(1) << lv);
  double uu = u / div - 0.5, vv = v / div - 0.5;
  double fu = std::floor(uu), fv = std::floor(vv);
  int64_t x0 = int64_t(fu), y0 = int64_t(fv);
  double fx = uu - double(x0), fy = vv - double(y0);
  int64_t xa = wrap(x0, t.w), xb = wrap(x0 + 1, t.w), ya = wrap(y0, t.h), yb = wrap(y0 + 1, t.h);
  return (t.p[ya * t.w + xa] * (1 - fx) + t.p[ya * t.w + xb] * fx) * (1 - fy) + (t.p[yb * t.w + xa] * (1 - fx) + t.p[yb * t.w + xb] * fx) * fy;
}

}  // namespace

// objs: n_objs x 5 doubles (centre x, bottom y, z of the face, width, height); obj_mips: n_objs x obj_levels textures.
// c, s_: cosine and sine of the yaw (from the caller, so that both forms use the same values).  img / depth: h x w doubles, oid: h x w int64.  Returns the number of uncertain mip decisions (0: the image is final).
extern "C" int64_t ps_seq_render(const double* cam_pos, double c, double s_, const double* K, int w, int h, const double* const* mip_ptr, const int64_t* mip_shape,
                                 int levels, const double* objs, int n_objs, const double* const* obj_mip_ptr, const int64_t* obj_mip_shape, int obj_levels,
                                 double texel_per_m, double* img, double* depth, int64_t* oid) {
  const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  const double half_w = 9.0, ground = 1.65, ceil_y = -7.0, z_end = 400.0;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<Mip> mips(levels), omips(size_t(n_objs) * obj_levels);
  for (int l = 0; l < levels; ++l) mips[l] = {mip_ptr[l], mip_shape[2 * l], mip_shape[2 * l + 1]};
  for (int i = 0; i < n_objs * obj_levels; ++i) omips[i] = {obj_mip_ptr[i], obj_mip_shape[2 * i], obj_mip_shape[2 * i + 1]};
  // per column: ray x / z in the world, distances of the planes x = +-half_w, z = z_end and of the object faces
  std::vector<double> dw0(w), dw2(w), t_wall_p(w), t_wall_n(w), t_end(w), t_obj(size_t(n_objs) * w);
  for (int x = 0; x < w; ++x) {
    double dc0 = (double(x) - cx) / fx;
    dw0[x] = c * dc0 + s_ * 1.0;
    dw2[x] = -s_ * dc0 + c * 1.0;
    t_wall_p[x] = (1.0 * half_w - cam_pos[0]) / dw0[x];
    t_wall_n[x] = (-1.0 * half_w - cam_pos[0]) / dw0[x];
    t_end[x] = (z_end - cam_pos[2]) / dw2[x];
    for (int k = 0; k < n_objs; ++k) t_obj[size_t(k) * w + x] = (objs[5 * k + 2] - cam_pos[2]) / dw2[x];
  }
  int64_t uncertain = 0;
  for (int y = 0; y < h; ++y) {
    const double dw1 = (double(y) - cy) / fy;
    const double t_ground = (ground - cam_pos[1]) / dw1, t_ceil = (ceil_y - cam_pos[1]) / dw1;
    for (int x = 0; x < w; ++x) {
      double best = inf;
      int win = -1;
      auto hit = [&](int id, double t, bool valid) {
        if (valid && t > 0.05 && t < best) { best = t; win = id; }
      };
      hit(0, t_ground, dw1 > 1e-9);
      hit(1, t_ceil, dw1 < -1e-9);
      hit(2, t_wall_p[x], 1.0 * dw0[x] > 1e-9);
      hit(3, t_wall_n[x], -1.0 * dw0[x] > 1e-9);
      hit(4, t_end[x], dw2[x] > 1e-9);
      for (int k = 0; k < n_objs; ++k) {
        const double* o = objs + 5 * k;
        double t = t_obj[size_t(k) * w + x];
        double px = cam_pos[0] + t * dw0[x], py = cam_pos[1] + t * dw1;
        bool inside = (dw2[x] > 1e-9) && (px >= o[0] - o[3] / 2) && (px < o[0] + o[3] / 2) && (py >= o[1] - o[4]) && (py < o[1]);
        hit(5 + k, t, inside);
      }
      double val = 0.0;
      int64_t ident = -1;
      const double t = best;
      switch (win) {
        case -1: break;
        case 0: val = sample(mips.data(), levels, (cam_pos[0] + t * dw0[x] + 1000.0) * texel_per_m, (cam_pos[2] + t * dw2[x]) * texel_per_m, (t / fx) * texel_per_m, &uncertain); break;
        case 1: { double sc = texel_per_m * 0.5;
                  val = sample(mips.data(), levels, (cam_pos[0] + t * dw0[x] + 1000.0) * sc, (cam_pos[2] + t * dw2[x] + 517.0) * sc, (t / fx) * sc, &uncertain); break; }
        case 2: val = sample(mips.data(), levels, (cam_pos[2] + t * dw2[x] + 211.0) * texel_per_m, (cam_pos[1] + t * dw1 + 50.0) * texel_per_m, (t / fx) * texel_per_m, &uncertain); break;
        case 3: val = sample(mips.data(), levels, (cam_pos[2] + t * dw2[x] + 733.0) * texel_per_m, (cam_pos[1] + t * dw1 + 50.0) * texel_per_m, (t / fx) * texel_per_m, &uncertain); break;
        case 4: { double sc = texel_per_m * 0.25;
                  val = sample(mips.data(), levels, (cam_pos[0] + t * dw0[x] + 300.0) * sc, (cam_pos[1] + t * dw1 + 80.0) * sc, (t / fx) * sc, &uncertain); break; }
        default: { int k = win - 5;
                   const double* o = objs + 5 * k;
                   double px = cam_pos[0] + t * dw0[x], py = cam_pos[1] + t * dw1;
                   val = sample(omips.data() + size_t(k) * obj_levels, obj_levels, (px - (o[0] - o[3] / 2)) * 60.0, (py - (o[1] - o[4])) * 60.0, (t / fx) * 60.0, &uncertain);
                   ident = k; }
      }
      size_t i = size_t(y) * w + x;
      img[i] = val; depth[i] = best * 1.0; oid[i] = ident;
    }
  }
  return uncertain;
}
