// Geometry and random numbers of the training augmentation (augment_ops.hip), host + device: the pixel map of a
// (rot, flipud, fliplr) element, the label map, the minimum-area rectangle of four integer points and Philox4x32-10.
//
// cv2.minAreaRect is OpenCV (third-party, not in the reference tree) and is restated from its definition: the convex hull
// of the points, then for every hull edge the bounding rectangle with a side along that edge, the smallest area wins.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define S2A_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define S2A_HD inline
#endif

namespace s2a {
namespace aug {

constexpr int kBorder = 114;   // borderValue=(114, 114, 114) of the reference's warpAffine

// ---------------------------------------------------------------------------------------------------------- Philox
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
S2A_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// one image's draw: (rot, flipud, fliplr) from the words of counter (image, 0, step_lo, step_hi), key (seed_lo, seed_hi)
S2A_HD void draw_params(uint32_t image, uint64_t step, uint64_t seed, int turn, float p_ud, float p_lr, int32_t out[4]) {
  const uint32_t ctr[4] = {image, 0u, (uint32_t)step, (uint32_t)(step >> 32)};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox4x32_10(ctr, key, w);
  const float u1 = (float)(w[1] >> 8) * (1.0f / 16777216.0f), u2 = (float)(w[2] >> 8) * (1.0f / 16777216.0f);
  out[0] = turn ? (int32_t)(w[0] & 3u) : 0;
  out[1] = u1 < p_ud;
  out[2] = u2 < p_lr;
  out[3] = 0;
}

// ------------------------------------------------------------------------------------------------------- pixel map
// destination pixel (X, Y) of an S x S chip takes source pixel (ax * U + bx, ay * V + by), (U, V) = (X, Y) or, transposed,
// (Y, X); a source coordinate equal to S is outside the chip (the turn is about S / 2, not (S - 1) / 2): border
struct PixelMap {
  int ax, bx, ay, by, transpose;
};

S2A_HD PixelMap pixel_map(int rot, int flipud, int fliplr, int S) {
  // after the turn: x' = px * X + qx, y' = py * Y + qy (np.flipud, np.fliplr: plain reversals)
  const int px = fliplr ? -1 : 1, qx = fliplr ? S - 1 : 0, py = flipud ? -1 : 1, qy = flipud ? S - 1 : 0;
  PixelMap m;
  switch (rot & 3) {
    case 1:   // 90 deg: x' = y, y' = S - x  ->  x = S - y', y = x'
      m.ax = -py; m.bx = S - qy; m.ay = px; m.by = qx; m.transpose = 1;
      break;
    case 2:   // -180 deg: x' = S - x, y' = S - y
      m.ax = -px; m.bx = S - qx; m.ay = -py; m.by = S - qy; m.transpose = 0;
      break;
    case 3:   // -90 deg: x' = S - y, y' = x  ->  x = y', y = S - x'
      m.ax = py; m.bx = qy; m.ay = -px; m.by = S - qx; m.transpose = 1;
      break;
    default:
      m.ax = px; m.bx = qx; m.ay = py; m.by = qy; m.transpose = 0;
  }
  return m;
}

// what one workgroup of the image kernel does: a kTile x kTile destination tile at (X0, Y0), its source tile staged in the
// LDS as kTile rows of kPitch dwords.  Shared with the host walk of tests/augment_tile_walk.cpp, which runs this
// arithmetic over every tile and element under the host's bounds checks
constexpr int kTile = 64;    // pixels per side
// LDS row: 64 pixels are 192 bytes, read from the dword below the first one: up to 49 dwords.  49 is odd, so the
// transposed read (lanes 4 LDS rows apart) walks the banks in steps of 4 and eight such lanes share no bank
constexpr int kPitch = 49;

struct TilePlan {
  PixelMap m;
  int tw, th;          // destination tile size (the chip's edge cuts the last tiles)
  int nu, nv;          // source tile: nu columns from sx_lo, nv rows from sy_lo
  int sx_lo, sy_lo;
  int d0, off, ndw;    // per source row: first dword, byte of pixel sx_lo in it, dwords to read (<= kPitch, d0 + ndw <= 3 S / 4)
};

S2A_HD TilePlan tile_plan(int rot, int flipud, int fliplr, int S, int X0, int Y0) {
  TilePlan p;
  p.m = pixel_map(rot, flipud, fliplr, S);
  p.tw = S - X0 < kTile ? S - X0 : kTile;
  p.th = S - Y0 < kTile ? S - Y0 : kTile;
  const int U0 = p.m.transpose ? Y0 : X0, V0 = p.m.transpose ? X0 : Y0;
  p.nu = p.m.transpose ? p.th : p.tw;
  p.nv = p.m.transpose ? p.tw : p.th;
  p.sx_lo = p.m.ax > 0 ? U0 + p.m.bx : p.m.bx - (U0 + p.nu - 1);
  p.sy_lo = p.m.ay > 0 ? V0 + p.m.by : p.m.by - (V0 + p.nv - 1);
  const int sx_end = p.sx_lo + p.nu < S ? p.sx_lo + p.nu : S;   // one past the last column inside the chip
  p.d0 = (3 * p.sx_lo) >> 2;
  p.off = (3 * p.sx_lo) & 3;
  p.ndw = ((3 * sx_end + 3) >> 2) - p.d0;
  return p;
}

// LDS byte of the source pixel of destination pixel (X, Y) of the tile, or -1: border
S2A_HD int tile_source_byte(const TilePlan& p, int S, int X, int Y) {
  const int sx = p.m.ax * (p.m.transpose ? Y : X) + p.m.bx, sy = p.m.ay * (p.m.transpose ? X : Y) + p.m.by;
  if (sx >= S || sy >= S) return -1;
  return (sy - p.sy_lo) * kPitch * 4 + p.off + 3 * (sx - p.sx_lo);
}

// four pixels (byte 0 = first channel) as the three dwords that hold them in memory
S2A_HD void pack_pixels(const uint32_t px[4], uint32_t out[3]) {
  out[0] = px[0] | (px[1] << 24);
  out[1] = (px[1] >> 8) | (px[2] << 16);
  out[2] = (px[2] >> 16) | (px[3] << 8);
}

// ------------------------------------------------------------------------------------------------------- label map
// M of random_perspective_rotation for the four turns, as exact integer maps
S2A_HD void turn_point(int rot, double S, double& x, double& y) {
  const double x0 = x, y0 = y;
  switch (rot & 3) {
    case 1: x = y0; y = S - x0; break;
    case 2: x = S - x0; y = S - y0; break;
    case 3: x = S - y0; y = x0; break;
    default: break;
  }
}

// astype(np.int64): towards zero; beyond +-2^29 the value saturates (and NaN becomes +2^29: both comparisons are false)
// so that the products below stay inside int64
S2A_HD long long trunc_coord(double v) {
  const double lim = 536870912.0;
  v = v < lim ? v : lim;
  v = v > -lim ? v : -lim;
  return (long long)v;
}

struct RBox {
  double cx, cy, w, h, theta;
};

S2A_HD long long cross3(long long ax, long long ay, long long bx, long long by, long long cx, long long cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// direction (dx, dy) or its opposite, whichever has its angle in [-pi/4, 3pi/4): exact on integers, so no mod pi of a
// rounded angle decides on which side of the seam a 45-degree box falls
S2A_HD double seam_angle(long long dx, long long dy) {
  if (dx + dy < 0 || (dx + dy == 0 && dx < 0)) {
    dx = -dx;
    dy = -dy;
  }
  return atan2((double)dy, (double)dx);
}

// minimum-area rectangle of four integer points (any order, concave or repeated points allowed) as (cx, cy, w, h, theta):
// w the long side, theta its direction in image coordinates in [-pi/4, 3pi/4).  false: the points span no area
S2A_HD bool min_area_rect4(const long long x[4], const long long y[4], RBox& out) {
  // sort by (x, y): five compare-exchanges
  long long sx[4] = {x[0], x[1], x[2], x[3]}, sy[4] = {y[0], y[1], y[2], y[3]};
#define S2A_AUG_CSWAP(i, j)                                              \
  if (sx[i] > sx[j] || (sx[i] == sx[j] && sy[i] > sy[j])) {              \
    const long long tx_ = sx[i], ty_ = sy[i];                            \
    sx[i] = sx[j]; sy[i] = sy[j]; sx[j] = tx_; sy[j] = ty_;              \
  }
  S2A_AUG_CSWAP(0, 1) S2A_AUG_CSWAP(2, 3) S2A_AUG_CSWAP(0, 2) S2A_AUG_CSWAP(1, 3) S2A_AUG_CSWAP(1, 2)
#undef S2A_AUG_CSWAP
  // monotone chain; collinear and repeated points drop out (cross <= 0)
  long long hx[8], hy[8];
  int k = 0;
  for (int i = 0; i < 4; i++) {
    while (k >= 2 && cross3(hx[k - 2], hy[k - 2], hx[k - 1], hy[k - 1], sx[i], sy[i]) <= 0) k--;
    hx[k] = sx[i]; hy[k] = sy[i]; k++;
  }
  for (int i = 2, t = k + 1; i >= 0; i--) {
    while (k >= t && cross3(hx[k - 2], hy[k - 2], hx[k - 1], hy[k - 1], sx[i], sy[i]) <= 0) k--;
    hx[k] = sx[i]; hy[k] = sy[i]; k++;
  }
  k--;   // the last point repeats the first
  if (k < 3) return false;
  double best = -1.0;
  for (int i = 0; i < k; i++) {
    const int j = i + 1 < k ? i + 1 : 0;
    const long long dx = hx[j] - hx[i], dy = hy[j] - hy[i];
    const double len = sqrt((double)(dx * dx + dy * dy));
    const double ex = (double)dx / len, ey = (double)dy / len;
    double umin = 0.0, umax = 0.0, vmin = 0.0, vmax = 0.0;   // hull point i itself sits at (0, 0)
    for (int q = 0; q < k; q++) {
      const double rx = (double)(hx[q] - hx[i]), ry = (double)(hy[q] - hy[i]);
      const double u = rx * ex + ry * ey, v = ry * ex - rx * ey;
      umin = u < umin ? u : umin; umax = u > umax ? u : umax;
      vmin = v < vmin ? v : vmin; vmax = v > vmax ? v : vmax;
    }
    const double lu = umax - umin, lv = vmax - vmin, area = lu * lv;
    if (best < 0.0 || area < best) {
      best = area;
      const double uc = 0.5 * (umax + umin), vc = 0.5 * (vmax + vmin);
      out.cx = (double)hx[i] + uc * ex - vc * ey;
      out.cy = (double)hy[i] + uc * ey + vc * ex;
      if (lu >= lv) {
        out.w = lu; out.h = lv; out.theta = seam_angle(dx, dy);
      } else {
        out.w = lv; out.h = lu; out.theta = seam_angle(-dy, dx);
      }
    }
  }
  return true;
}

enum LabelFate { kKept = 0, kPadding = 1, kOffCentre = 2, kDegenerate = 3 };

// one label row (image, class, x1, y1 .. x4, y4) through turn, centre filter, flips and the box conversion
S2A_HD int augment_label(const double pts[8], int rot, int flipud, int fliplr, double S, RBox& out) {
  double px[4], py[4];
  long long ix[4], iy[4];
  for (int i = 0; i < 4; i++) {
    px[i] = pts[2 * i]; py[i] = pts[2 * i + 1];
    turn_point(rot, S, px[i], py[i]);
    ix[i] = trunc_coord(px[i]); iy[i] = trunc_coord(py[i]);
  }
  if (!min_area_rect4(ix, iy, out)) return kDegenerate;
  // box_candidates_rotation_filter_center: 0 <= centre <= S on both axes
  if (!(out.cx >= 0.0 && out.cx <= S && out.cy >= 0.0 && out.cy <= S)) return kOffCentre;
  for (int i = 0; i < 4; i++) {
    if (flipud) py[i] = S - py[i];
    if (fliplr) px[i] = S - px[i];
    ix[i] = trunc_coord(px[i]); iy[i] = trunc_coord(py[i]);
  }
  if (!min_area_rect4(ix, iy, out)) return kDegenerate;
  return kKept;
}

}  // namespace aug
}  // namespace s2a
