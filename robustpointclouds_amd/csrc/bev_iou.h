// BEV IoU of two rotated boxes (x, y, dx, dy, yaw), shared by rpc_bev_iou_pairs and the rotated-NMS mask
// kernel (postprocess.hip). Restates what mmcv `box_iou_rotated` / `nms_rotated` compute (upstream
// mmcv/ops/csrc/common/box_iou_rotated_utils.hpp) as convex clipping instead of its intersection-point sort:
// box b is moved into the frame of box a (centre of a subtracted FIRST, then rotated by -yaw_a), so every
// coordinate the clipper sees is of the size of the boxes, not of their range: fp32 error does not grow with the
// distance from the origin. There a is the axis-aligned rectangle |x| <= dxa/2, |y| <= dya/2 and b's four corners
// are clipped against its four sides (Sutherland-Hodgman; a crossing lies exactly on the side). The area is the
// trapezoid form of the shoelace sum. Finite in [0, 1] for every finite input; a box with dx <= 0 or dy <= 0 has
// IoU 0; identical boxes give exactly 1.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace rpc {
namespace bev {

struct Poly {
  float x[8], y[8];
  int n;
};

// keep the part of p with sgn * (axis ? y : x) <= lim
template <int AXIS, int SGN>
__host__ __device__ __forceinline__ void clip_side(const Poly& p, float lim, Poly& q) {
  q.n = 0;
  if (p.n == 0) return;
  float px = p.x[p.n - 1], py = p.y[p.n - 1];
  float pd = SGN * (AXIS ? py : px) - lim;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k < p.n) {
      const float cx = p.x[k], cy = p.y[k];
      const float cd = SGN * (AXIS ? cy : cx) - lim;
      if ((pd <= 0.0f) != (cd <= 0.0f)) {  // the side is crossed between the previous vertex and this one
        const float t = pd / (pd - cd);
        if (q.n < 8) {
          q.x[q.n] = AXIS ? px + t * (cx - px) : SGN * lim;
          q.y[q.n] = AXIS ? SGN * lim : py + t * (cy - py);
          ++q.n;
        }
      }
      if (cd <= 0.0f && q.n < 8) {
        q.x[q.n] = cx;
        q.y[q.n] = cy;
        ++q.n;
      }
      px = cx, py = cy, pd = cd;
    }
  }
}

// ca, sa: cos / sin of a's yaw
__host__ __device__ __forceinline__ float iou_cs(float ax, float ay, float adx, float ady, float ayaw, float ca,
                                                 float sa, float bx, float by, float bdx, float bdy, float byaw) {
  if (!(adx > 0.0f) || !(ady > 0.0f) || !(bdx > 0.0f) || !(bdy > 0.0f)) return 0.0f;
  const float tx = bx - ax, ty = by - ay;
  const float cx = ca * tx + sa * ty, cy = ca * ty - sa * tx;   // b's centre in a's frame
  const float d = byaw - ayaw;
  float sd, cd;
  sincosf(d, &sd, &cd);
  const float hx = 0.5f * bdx, hy = 0.5f * bdy;
  const float ux = cd * hx, uy = sd * hx;    // half-length vector
  const float vx = -sd * hy, vy = cd * hy;   // half-width vector
  Poly p, q;
  p.n = 4;
  p.x[0] = cx + ux + vx, p.y[0] = cy + uy + vy;
  p.x[1] = cx - ux + vx, p.y[1] = cy - uy + vy;
  p.x[2] = cx - ux - vx, p.y[2] = cy - uy - vy;
  p.x[3] = cx + ux - vx, p.y[3] = cy + uy - vy;
  const float hax = 0.5f * adx, hay = 0.5f * ady;
  clip_side<0, 1>(p, hax, q);
  clip_side<0, -1>(q, hax, p);
  clip_side<1, 1>(p, hay, q);
  clip_side<1, -1>(q, hay, p);
  float s = 0.0f;
  if (p.n >= 3) {
    float px = p.x[p.n - 1], py = p.y[p.n - 1];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < p.n) {
        s += (px - p.x[k]) * (py + p.y[k]);
        px = p.x[k], py = p.y[k];
      }
    }
  }
  const float area_a = adx * ady, area_b = bdx * bdy;
  float inter = 0.5f * fabsf(s);
  inter = fminf(inter, fminf(area_a, area_b));
  const float iou = inter / (area_a + area_b - inter);
  return iou >= 0.0f ? fminf(iou, 1.0f) : 0.0f;   // NaN (overflowed areas, 0 / 0) -> 0
}

}  // namespace bev
}  // namespace rpc
