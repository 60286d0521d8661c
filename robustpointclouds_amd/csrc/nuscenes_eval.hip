// nuScenes detection score for gfx950: the device part (include/rpc_hip.h, "nuScenes"; the specification is in
// DESIGN.md "nuScenes detection score", restated from nuscenes-devkit eval/detection, detection_cvpr_2019).
//   rpc_nus_match      the greedy centre-distance matcher for all frames x classes x thresholds in one launch
//   rpc_nus_tp_errors  the five true-positive errors of every matched detection
// No MFMA here. Frames are ragged (offset arrays on the device).
//   match: one wave per (frame, class, threshold), the decomposition of k_match_scores (kitti_eval.hip) turned
//          round: the DETECTIONS are sequential (the greedy order is theirs) and lane l owns ground truths l,
//          l + 64, ... of the frame — their xy and a `free` bit each in registers (8 words at the cap), the bit
//          set only for kept ground truths of the wave's class. The detections are read 64 at a time (lane =
//          detection, one ballot for "kept and of this class"), and the wave walks only those in index order, the
//          detection's xy broadcast from the owning lane. Each lane takes its own minimum over its free ground
//          truths (strict <: the lowest row stays), the wave reduces on (distance, lowest row), the owning lane
//          clears the bit and one lane stores the row. Matches interact only inside one (frame, class,
//          threshold), so no atomics and no dependence on the launch geometry. The squared distance is
//          fl(fl(dx dx) + fl(dy dy)) with every operation rounded (no contraction), so that a host can restate it.
//   errors: one thread per detection; everything it needs arrives as numbers (period of the yaw difference and
//          attribute ids per detection / ground truth).
#include <hip/hip_runtime.h>

#include "common.h"

namespace rpc {
namespace nus {

constexpr int kWords = RPC_NUS_MAX_GT / 64;   // 64-ground-truth words of a frame
constexpr float kPi = 3.14159265358979323846f;

__device__ __forceinline__ float dist2(float ax, float ay, float bx, float by) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by);
  return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

// first row and clamped count of frame f: in [0, n] whatever the offsets hold
__device__ __forceinline__ void span_of(const int* off, int f, int cap, long long n, int& first, int& count) {
  const long long a = min(max((long long)off[f], 0ll), n);
  const long long c = min(max((long long)off[f + 1] - a, 0ll), min((long long)cap, n - a));
  first = (int)a, count = (int)c;
}

__global__ __launch_bounds__(64) void k_match(const float* __restrict__ det_xy, const int* __restrict__ det_label,
                                              const signed char* __restrict__ det_keep,
                                              const int* __restrict__ det_off, const float* __restrict__ gt_xy,
                                              const int* __restrict__ gt_label,
                                              const signed char* __restrict__ gt_keep,
                                              const int* __restrict__ gt_off, int max_det, int max_gt,
                                              long long n_det, long long n_gt, const float* __restrict__ thr,
                                              int* __restrict__ match) {
  const int f = blockIdx.x, c = blockIdx.y, t = blockIdx.z, lane = threadIdx.x;
  int d0, nd, g0, ng;
  span_of(det_off, f, max_det, n_det, d0, nd);
  span_of(gt_off, f, max_gt, n_gt, g0, ng);
  if (nd == 0 || ng == 0) return;   // wave-uniform
  float gx[kWords], gy[kWords];
  unsigned free_ = 0;   // bit w: ground truth 64 w + lane is kept, of class c and not taken yet
#pragma unroll
  for (int w = 0; w < kWords; ++w) {
    const int i = w * 64 + lane;
    const bool in = i < ng;
    gx[w] = in ? gt_xy[2ll * (g0 + i)] : 0.0f;
    gy[w] = in ? gt_xy[2ll * (g0 + i) + 1] : 0.0f;
    if (in && gt_keep[g0 + i] != 0 && gt_label[g0 + i] == c) free_ |= 1u << w;
  }
  if (__ballot(free_ != 0) == 0ull) return;   // no ground truth of this class: every detection stays -1
  const float th = thr[t];
  const float t2 = __fmul_rn(th, th);
  int* out = match + (long long)t * n_det + d0;
  for (int j0 = 0; j0 < nd; j0 += 64) {   // wave-uniform
    const int j = j0 + lane;
    const bool in = j < nd;
    const float px = in ? det_xy[2ll * (d0 + j)] : 0.0f;
    const float py = in ? det_xy[2ll * (d0 + j) + 1] : 0.0f;
    unsigned long long todo = __ballot(in && det_keep[d0 + j] != 0 && det_label[d0 + j] == c);
    while (todo) {   // wave-uniform: the detections of this class, in evaluation order
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const float x = __shfl(px, b, 64), y = __shfl(py, b, 64);
      float best = INFINITY;
      int bi = -1;
#pragma unroll
      for (int w = 0; w < kWords; ++w) {
        if ((free_ >> w) & 1u) {
          const float d = dist2(gx[w], gy[w], x, y);
          if (d < best) best = d, bi = w * 64 + lane;   // strict: the lowest row of equal distances stays
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (oi >= 0 && (bi < 0 || ob < best || (ob == best && oi < bi))) best = ob, bi = oi;
      }
      if (bi >= 0 && best < t2) {   // wave-uniform after the reduction
        if ((bi & 63) == lane) free_ &= ~(1u << (bi >> 6));
        if (lane == 0) out[j0 + b] = g0 + bi;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_tp_errors(const float* __restrict__ det, const float* __restrict__ gt,
                                                   const int* __restrict__ match, const float* __restrict__ period,
                                                   const int* __restrict__ det_attr, const int* __restrict__ gt_attr,
                                                   long long n_det, long long n_gt, float* __restrict__ err) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_det) return;
  float* e = err + 5 * j;
  const int m = match[j];
  if (m < 0 || m >= n_gt) {
#pragma unroll
    for (int k = 0; k < 5; ++k) e[k] = NAN;
    return;
  }
  float d[9], g[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) d[k] = det[9 * j + k], g[k] = gt[9ll * m + k];
  e[0] = sqrtf(dist2(g[0], g[1], d[0], d[1]));
  float scale = 1.0f;
  if (d[3] > 0 && d[4] > 0 && d[5] > 0 && g[3] > 0 && g[4] > 0 && g[5] > 0) {
    const float inter = fminf(d[3], g[3]) * fminf(d[4], g[4]) * fminf(d[5], g[5]);
    const float vg = g[3] * g[4] * g[5], vd = d[3] * d[4] * d[5];
    scale = 1.0f - inter / (vg + vd - inter);
  }
  e[1] = scale;
  const float p = period[j];
  float v = fmodf(g[6] - d[6] + 0.5f * p, p);   // floor-mod: fmod, then the sign of p
  if (v < 0) v += p;
  v -= 0.5f * p;
  if (v > kPi) v -= 2.0f * kPi;
  e[2] = fabsf(v);
  const float dvx = g[7] - d[7], dvy = g[8] - d[8];
  e[3] = sqrtf(dvx * dvx + dvy * dvy);
  const int ga = gt_attr[m];
  e[4] = ga < 0 ? NAN : (det_attr[j] == ga ? 0.0f : 1.0f);
}

}  // namespace nus
}  // namespace rpc

using namespace rpc::nus;

extern "C" {

int rpc_nus_match(const float* det_xy, const int* det_label, const signed char* det_keep, const int* det_off,
                  const float* gt_xy, const int* gt_label, const signed char* gt_keep, const int* gt_off, int frames,
                  int max_det, int max_gt, long long n_det, long long n_gt, int n_classes, const float* thr,
                  int n_thr, int* match, void* stream) {
  if (frames < 0 || max_det < 0 || max_gt < 0 || n_det < 0 || n_gt < 0 || n_classes < 0 || n_thr < 0 ||
      n_classes > 65535)
    return RPC_ERR_ARG;
  if (max_det > RPC_NUS_MAX_DET || max_gt > RPC_NUS_MAX_GT || n_thr > RPC_NUS_MAX_THR) return RPC_ERR_UNSUPPORTED;
  if (frames == 0 || n_det == 0 || n_thr == 0) return RPC_OK;
  if (!det_xy || !det_label || !det_keep || !det_off || !gt_off || !thr || !match) return RPC_ERR_ARG;
  if (n_gt && (!gt_xy || !gt_label || !gt_keep)) return RPC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  RPC_CHECK(hipMemsetAsync(match, 0xff, (size_t)n_thr * (size_t)n_det * sizeof(int), st));   // -1: no match
  if (n_gt == 0 || n_classes == 0 || max_det == 0 || max_gt == 0) return RPC_OK;
  hipLaunchKernelGGL(k_match, dim3(frames, n_classes, n_thr), dim3(64), 0, st, det_xy, det_label, det_keep, det_off,
                     gt_xy, gt_label, gt_keep, gt_off, max_det, max_gt, n_det, n_gt, thr, match);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

int rpc_nus_tp_errors(const float* det, const float* gt, const int* match, const float* period, const int* det_attr,
                      const int* gt_attr, long long n_det, long long n_gt, float* err, void* stream) {
  if (n_det < 0 || n_gt < 0) return RPC_ERR_ARG;
  if (n_det == 0) return RPC_OK;
  if (!det || !match || !period || !det_attr || !err) return RPC_ERR_ARG;
  if (n_gt && (!gt || !gt_attr)) return RPC_ERR_ARG;
  const long long blocks = (n_det + 255) / 256;
  if (blocks > 0x7fffffffll) return RPC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_tp_errors, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, det, gt, match, period,
                     det_attr, gt_attr, n_det, n_gt, err);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

}  // extern "C"
