// Overlap of two LiDAR boxes (x, y, z, dx, dy, dz, yaw) for the KITTI evaluator (kitti_eval.hip), beside
// rpc::bev::iou_cs of bev_iou.h and with its construction: box b is moved into the frame of box a first
// (a's centre subtracted, then rotated by -yaw_a; z relative to a's bottom face), so every number the clipper
// and the z-interval see is of the size of the boxes and fp32 error does not grow with range.
// z is the BOTTOM face, as in mmdet3d LiDARInstance3DBoxes and as `predict` returns it (Anchor3DHead decodes
// z_centre - dz / 2, CenterHead subtracts dz / 2 in predict_by_feat): the box spans [z, z + dz].
//   inter_cs     area of the intersection of the two footprints, <= min(area_a, area_b)
//   overlap_3d   inter_cs * |z-interval overlap| / (vol_a + vol_b - inter)
// Both are finite in [0, 1] (overlap) for every finite input, exactly 0 when any extent is <= 0, and overlap_3d
// of identical boxes is exactly 1: the footprint intersection of identical boxes is exactly dx * dy (every
// corner lies on a side of the clip rectangle; bev_iou.h) and the z-overlap, taken relative to a's bottom face,
// is exactly dz.
#pragma once
#include "bev_iou.h"

namespace rpc {
namespace bev {

// ca, sa: cos / sin of a's yaw. Both boxes must have positive dx, dy (the callers check).
__host__ __device__ __forceinline__ float inter_cs(float ax, float ay, float adx, float ady, float ayaw, float ca,
                                                   float sa, float bx, float by, float bdx, float bdy, float byaw) {
  const float tx = bx - ax, ty = by - ay;
  const float cx = ca * tx + sa * ty, cy = ca * ty - sa * tx;
  const float d = byaw - ayaw;
  float sd, cd;
  sincosf(d, &sd, &cd);
  const float hx = 0.5f * bdx, hy = 0.5f * bdy;
  const float ux = cd * hx, uy = sd * hx;
  const float vx = -sd * hy, vy = cd * hy;
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
  const float inter = 0.5f * fabsf(s);
  return fminf(inter, fminf(adx * ady, bdx * bdy));   // fminf drops a NaN operand
}

// a, b: (x, y, z, dx, dy, dz, yaw); ca, sa: cos / sin of a[6]
__host__ __device__ __forceinline__ float overlap_3d(const float* a, float ca, float sa, const float* b) {
  if (!(a[3] > 0.0f) || !(a[4] > 0.0f) || !(a[5] > 0.0f) || !(b[3] > 0.0f) || !(b[4] > 0.0f) || !(b[5] > 0.0f))
    return 0.0f;
  const float tz = b[2] - a[2];                                // b's bottom face above a's
  const float lo = fmaxf(tz, 0.0f), hi = fminf(tz + b[5], a[5]);
  const float h = hi - lo;
  if (!(h > 0.0f)) return 0.0f;                                // apart or touching in z (or NaN)
  const float area = inter_cs(a[0], a[1], a[3], a[4], a[6], ca, sa, b[0], b[1], b[3], b[4], b[6]);
  const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
  const float inter = fminf(area * h, fminf(va, vb));
  const float iou = inter / (va + vb - inter);
  return iou >= 0.0f ? fminf(iou, 1.0f) : 0.0f;                // NaN (overflowed volumes, 0 / 0) -> 0
}

// rotated BEV IoU of the footprints of two 7-number boxes; z is not looked at, but a box with dz <= 0 is no box
// here either (every non-positive extent gives 0 in both modes)
__host__ __device__ __forceinline__ float overlap_bev(const float* a, float ca, float sa, const float* b) {
  if (!(a[5] > 0.0f) || !(b[5] > 0.0f)) return 0.0f;
  return iou_cs(a[0], a[1], a[3], a[4], a[6], ca, sa, b[0], b[1], b[3], b[4], b[6]);
}

}  // namespace bev
}  // namespace rpc
