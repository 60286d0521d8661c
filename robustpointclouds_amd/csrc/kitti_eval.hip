// KITTI BEV / 3D average precision for gfx950: the device part (include/rpc_hip.h, "KITTI"; the specification is
// in DESIGN.md "KITTI average precision", restated from mmdet3d v1.x kitti_utils/eval.py).
//   rpc_kitti_overlaps      ov[frame][det][gt] for all frames in one launch                (box_overlap.h)
//   rpc_kitti_match_scores  matcher pass 1: the score of every matched valid ground truth
//   rpc_kitti_match_counts  matcher pass 2: tp / fp / fn at every threshold of every group
// No MFMA here. Frames are ragged (offset arrays on the device); a group is one (class, difficulty, table).
//   overlaps: one thread per (det, gt) pair, 256 pairs a block, the frame's ground truths staged in LDS with
//          the cos / sin of their yaw (pitch 9 floats: conflict-free). The ground truth is box a of the clipper.
//   pass 1: one wave per (frame, group). Without a threshold the greedy choice for a ground truth is the
//          unassigned detection of the highest score among those above the minimum overlap, the first of equal
//          scores: lane l owns detections l, l + 64, ... (scores and an `eligible` bit each in registers), takes
//          its own best and the wave reduces (score, lowest index). Ground truths stay sequential.
//   pass 2: one wave per (frame, group), ONE LANE PER THRESHOLD (41 <= 64). Each lane runs the sequential loop
//          for its own threshold; its `assigned` set is a 512-bit mask in registers. What does not depend on the
//          threshold is done once for the wave: per ground truth the detections above the minimum overlap are
//          found 64 at a time (lane = detection, one ballot), and the lanes then walk only those candidates in
//          index order (wave-uniform loop, score / overlap broadcast from the owning lane), every update a
//          select. A wave walks frames blockIdx.x, + gridDim.x, ... with its counts in registers and adds them
//          once with integer atomics: deterministic.
#include <hip/hip_runtime.h>

#include "box_overlap.h"
#include "common.h"

namespace rpc {
namespace kitti {

constexpr int kWords = RPC_KITTI_MAX_DET / 64;   // 64-detection words of a frame
constexpr float kNo = RPC_KITTI_NO_SCORE;

struct Frame {
  int d0, nd, g0, ng;
  long long o0;
};

__device__ __forceinline__ Frame frame_of(const int* det_off, const int* gt_off, const long long* ov_off, int f,
                                          int max_det, int max_gt) {
  Frame r;
  r.d0 = det_off[f];
  r.nd = min(max(det_off[f + 1] - r.d0, 0), max_det);
  r.g0 = gt_off[f];
  r.ng = min(max(gt_off[f + 1] - r.g0, 0), max_gt);
  r.o0 = ov_off[f];
  return r;
}

__global__ __launch_bounds__(256) void k_overlaps(const float* __restrict__ det, const int* __restrict__ det_off,
                                                  const float* __restrict__ gt, const int* __restrict__ gt_off,
                                                  const long long* __restrict__ ov_off, int frames, int max_det,
                                                  int max_gt, int mode, float* __restrict__ ov) {
  __shared__ float sg[RPC_KITTI_MAX_GT][9];   // box(7), cos, sin
  for (int f = blockIdx.y; f < frames; f += gridDim.y) {
    const Frame fr = frame_of(det_off, gt_off, ov_off, f, max_det, max_gt);
    const int npair = fr.nd * fr.ng;
    if ((int)blockIdx.x * 256 >= npair) continue;   // block-uniform
    for (int i = threadIdx.x; i < fr.ng; i += 256) {
      const float* p = gt + 7ll * (fr.g0 + i);
#pragma unroll
      for (int k = 0; k < 7; ++k) sg[i][k] = p[k];
      float s, c;
      sincosf(p[6], &s, &c);
      sg[i][7] = c, sg[i][8] = s;
    }
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < npair) {
      const int j = p / fr.ng, i = p - j * fr.ng;
      float b[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) b[k] = det[7ll * (fr.d0 + j) + k];
      const float* a = sg[i];
      ov[fr.o0 + p] = mode ? bev::overlap_3d(a, a[7], a[8], b) : bev::overlap_bev(a, a[7], a[8], b);
    }
    __syncthreads();   // the next frame restages sg
  }
}

__global__ __launch_bounds__(64) void k_match_scores(const float* __restrict__ ov, const long long* __restrict__ ov_off,
                                                     const int* __restrict__ det_off, const int* __restrict__ gt_off,
                                                     int max_det, int max_gt, const float* __restrict__ score,
                                                     const signed char* __restrict__ flag_det,
                                                     const signed char* __restrict__ flag_gt, long long n_det,
                                                     long long n_gt, const float* __restrict__ min_ov, int ntab,
                                                     float* __restrict__ tp_score) {
  const int f = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
  const Frame fr = frame_of(det_off, gt_off, ov_off, f, max_det, max_gt);
  if (fr.ng == 0) return;
  const int row = g / ntab;
  const signed char* fd = flag_det + row * n_det + fr.d0;
  const signed char* fg = flag_gt + row * n_gt + fr.g0;
  float* out = tp_score + g * n_gt + fr.g0;
  const float mo = min_ov[g];
  float s[kWords];
  unsigned elig = 0;   // bit w: detection 64 w + lane exists, is not of flag -1 and is not assigned yet
#pragma unroll
  for (int w = 0; w < kWords; ++w) {
    const int j = w * 64 + lane;
    const bool in = j < fr.nd;
    s[w] = in ? score[fr.d0 + j] : kNo;
    if (in && fd[j] != -1) elig |= 1u << w;
  }
  for (int i = 0; i < fr.ng; ++i) {
    const int fgi = fg[i];
    float res = kNo;
    if (fgi != -1) {   // wave-uniform
      float best = kNo;
      int bj = -1;
#pragma unroll
      for (int w = 0; w < kWords; ++w) {
        if ((elig >> w) & 1u) {
          const int j = w * 64 + lane;
          const float o = ov[fr.o0 + (long long)j * fr.ng + i];
          if (o > mo && s[w] > best) best = s[w], bj = j;   // strict: the first of equal scores stays
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oj = __shfl_xor(bj, off, 64);
        if (oj >= 0 && (bj < 0 || ob > best || (ob == best && oj < bj))) best = ob, bj = oj;
      }
      if (bj >= 0) {   // wave-uniform after the reduction
        if ((bj & 63) == lane) elig &= ~(1u << (bj >> 6));
        if (fgi == 0 && fd[bj] == 0) res = best;   // a true positive; otherwise the detection is only used up
      }
    }
    if (lane == 0) out[i] = res;
  }
}

__global__ __launch_bounds__(64) void k_match_counts(const float* __restrict__ ov, const long long* __restrict__ ov_off,
                                                     const int* __restrict__ det_off, const int* __restrict__ gt_off,
                                                     int frames, int max_det, int max_gt,
                                                     const float* __restrict__ score,
                                                     const signed char* __restrict__ flag_det,
                                                     const signed char* __restrict__ flag_gt, long long n_det,
                                                     long long n_gt, const float* __restrict__ min_ov, int ntab,
                                                     const float* __restrict__ thr, const int* __restrict__ nthr,
                                                     int* __restrict__ counts) {
  const int g = blockIdx.y, lane = threadIdx.x;
  const int nt = min(nthr[g], RPC_KITTI_MAX_THR);
  if (nt <= 0) return;   // a group without thresholds counts nothing
  const bool active = lane < nt;
  const float th = active ? thr[g * RPC_KITTI_MAX_THR + lane] : INFINITY;   // idle lanes match nothing
  const int row = g / ntab;
  const float mo = min_ov[g];
  int tp = 0, fp = 0, fn = 0;
  for (int f = blockIdx.x; f < frames; f += gridDim.x) {
    const Frame fr = frame_of(det_off, gt_off, ov_off, f, max_det, max_gt);
    const signed char* fd = flag_det + row * n_det + fr.d0;
    const signed char* fg = flag_gt + row * n_gt + fr.g0;
    float s[kWords];                      // lane = detection: its score
    unsigned long long mc[kWords];        // wave-uniform: detections of flag != -1
    unsigned long long m0[kWords];        // wave-uniform: detections of flag 0
    unsigned long long asg[kWords];       // lane = threshold: the detections it has assigned
#pragma unroll
    for (int w = 0; w < kWords; ++w) {
      const int j = w * 64 + lane;
      const bool in = j < fr.nd;
      s[w] = in ? score[fr.d0 + j] : kNo;
      const int c = in ? (int)fd[j] : -1;
      mc[w] = __ballot(c != -1);
      m0[w] = __ballot(c == 0);
      asg[w] = 0ull;
    }
    for (int i = 0; i < fr.ng; ++i) {
      const int fgi = fg[i];
      if (fgi == -1) continue;   // wave-uniform
      bool valid = false, took = false;
      float max_ov = 0.0f;
      int det = -1, detf = 0;
#pragma unroll
      for (int w = 0; w < kWords; ++w) {
        if (w * 64 < fr.nd) {   // wave-uniform
          const int j = w * 64 + lane;
          const bool mine = (mc[w] >> lane) & 1ull;
          const float o = mine ? ov[fr.o0 + (long long)j * fr.ng + i] : 0.0f;
          unsigned long long cand = __ballot(mine && o > mo);
          while (cand) {   // wave-uniform: the detections above the minimum overlap, in index order
            const int b = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            const float oo = __shfl(o, b, 64), ss = __shfl(s[w], b, 64);
            const bool f0 = (m0[w] >> b) & 1ull;   // flag 0, else flag 1
            const bool skip = ((asg[w] >> b) & 1ull) || ss < th;
            const bool c1 = !skip && f0 && (oo > max_ov || took);
            const bool c2 = !skip && !f0 && !valid;
            if (c1) max_ov = oo, det = w * 64 + b, detf = 0, valid = true, took = false;
            if (c2) det = w * 64 + b, detf = 1, valid = true, took = true;
          }
        }
      }
      if (!valid) {
        fn += fgi == 0;
      } else {
        tp += fgi == 0 && detf == 0;
#pragma unroll
        for (int w = 0; w < kWords; ++w)
          if ((det >> 6) == w) asg[w] |= 1ull << (det & 63);
      }
    }
    // false positives: valid detections at or above the threshold that no ground truth took
#pragma unroll
    for (int w = 0; w < kWords; ++w) {
      unsigned long long m = m0[w];
      while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float ss = __shfl(s[w], b, 64);
        fp += !((asg[w] >> b) & 1ull) && !(ss < th);
      }
    }
  }
  if (active) {
    int* c = counts + ((long long)g * RPC_KITTI_MAX_THR + lane) * 3;
    if (tp) atomicAdd(c, tp);
    if (fp) atomicAdd(c + 1, fp);
    if (fn) atomicAdd(c + 2, fn);
  }
}

static int check_frames(const void* ov_off, const void* det_off, const void* gt_off, int frames, int max_det,
                        int max_gt) {
  if (frames < 0 || max_det < 0 || max_gt < 0) return RPC_ERR_ARG;
  if (max_det > RPC_KITTI_MAX_DET || max_gt > RPC_KITTI_MAX_GT) return RPC_ERR_UNSUPPORTED;
  if (frames && (!ov_off || !det_off || !gt_off)) return RPC_ERR_ARG;
  return RPC_OK;
}

static int check_match(const float* ov, const long long* ov_off, const int* det_off, const int* gt_off, int frames,
                       int max_det, int max_gt, const float* score, const signed char* flag_det,
                       const signed char* flag_gt, long long n_det, long long n_gt, const float* min_ov, int groups,
                       int ntab) {
  const int rc = check_frames(ov_off, det_off, gt_off, frames, max_det, max_gt);
  if (rc != RPC_OK) return rc;
  if (groups < 0 || groups > 65535 || ntab <= 0 || groups % ntab || n_det < 0 || n_gt < 0) return RPC_ERR_ARG;
  if (frames == 0 || groups == 0) return RPC_OK;
  if (!min_ov || (n_det && (!score || !flag_det)) || (n_gt && !flag_gt) || (n_det && n_gt && !ov)) return RPC_ERR_ARG;
  return RPC_OK;
}

}  // namespace kitti
}  // namespace rpc

using namespace rpc::kitti;

extern "C" {

int rpc_kitti_overlaps(const float* det, const int* det_off, const float* gt, const int* gt_off,
                       const long long* ov_off, int frames, int max_det, int max_gt, int mode, float* ov,
                       void* stream) {
  const int rc = check_frames(ov_off, det_off, gt_off, frames, max_det, max_gt);
  if (rc != RPC_OK) return rc;
  if (mode != 0 && mode != 1) return RPC_ERR_ARG;
  if (frames == 0 || max_det == 0 || max_gt == 0) return RPC_OK;
  if (!det || !gt || !ov) return RPC_ERR_ARG;
  const dim3 grid((max_det * max_gt + 255) / 256, frames < 65535 ? frames : 65535);
  hipLaunchKernelGGL(k_overlaps, grid, dim3(256), 0, (hipStream_t)stream, det, det_off, gt, gt_off, ov_off, frames,
                     max_det, max_gt, mode, ov);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

int rpc_kitti_match_scores(const float* ov, const long long* ov_off, const int* det_off, const int* gt_off,
                           int frames, int max_det, int max_gt, const float* score, const signed char* flag_det,
                           const signed char* flag_gt, long long n_det, long long n_gt, const float* min_ov,
                           int groups, int ntab, float* tp_score, void* stream) {
  const int rc = check_match(ov, ov_off, det_off, gt_off, frames, max_det, max_gt, score, flag_det, flag_gt, n_det,
                             n_gt, min_ov, groups, ntab);
  if (rc != RPC_OK) return rc;
  if (frames == 0 || groups == 0 || n_gt == 0) return RPC_OK;
  if (!tp_score) return RPC_ERR_ARG;
  hipLaunchKernelGGL(k_match_scores, dim3(frames, groups), dim3(64), 0, (hipStream_t)stream, ov, ov_off, det_off,
                     gt_off, max_det, max_gt, score, flag_det, flag_gt, n_det, n_gt, min_ov, ntab, tp_score);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

int rpc_kitti_match_counts(const float* ov, const long long* ov_off, const int* det_off, const int* gt_off,
                           int frames, int max_det, int max_gt, const float* score, const signed char* flag_det,
                           const signed char* flag_gt, long long n_det, long long n_gt, const float* min_ov,
                           int groups, int ntab, const float* thr, const int* nthr, int* counts, void* stream) {
  const int rc = check_match(ov, ov_off, det_off, gt_off, frames, max_det, max_gt, score, flag_det, flag_gt, n_det,
                             n_gt, min_ov, groups, ntab);
  if (rc != RPC_OK) return rc;
  if (groups == 0) return RPC_OK;
  if (!thr || !nthr || !counts) return RPC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  RPC_CHECK(hipMemsetAsync(counts, 0, (size_t)groups * RPC_KITTI_MAX_THR * 3 * sizeof(int), st));
  if (frames == 0) return RPC_OK;
  hipLaunchKernelGGL(k_match_counts, dim3(frames < 256 ? frames : 256, groups), dim3(64), 0, st, ov, ov_off, det_off,
                     gt_off, frames, max_det, max_gt, score, flag_det, flag_gt, n_det, n_gt, min_ov, ntab, thr, nthr,
                     counts);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

}  // extern "C"
