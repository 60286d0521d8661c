// KITTI BEV / 3D average precision for gfx950: the device part (include/rpc_hip.h, "KITTI"; the specification is
// in DESIGN.md "KITTI average precision", restated from mmdet3d v1.x kitti_utils/eval.py).
//   rpc_kitti_overlaps      ov[frame][det][gt] for all frames in one launch                (box_overlap.h)
//   rpc_kitti_match_scores  matcher pass 1: the score of every matched valid ground truth
//   rpc_kitti_match_counts  matcher pass 2: tp / fp / fn at every threshold of every group
//   rpc_kitti_project       LiDAR boxes through a frame's lidar2img: raw / clipped 2D box, validity, alpha, height
//   rpc_kitti_overlaps_2d   mode 0: 2D IoU [det][gt]; mode 1: the DontCare `stuff` bits [class][det]
//   rpc_kitti_match_counts_aos  pass 2 with the stuff bits and the AOS similarity sums (the same kernel template)
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

// EXT = false is pass 2 as rpc_kitti_match_counts runs it: every `if constexpr (EXT)` below is compiled out.
// EXT = true adds the two optional inputs of the 2D / AOS metrics (either may be null): `stuff` [groups / gps][n_det]
// (a detection inside a DontCare region is no false positive; it still takes part in the matching) and the
// observation angles, whose similarity (1 + cos(alpha_gt - alpha_det)) / 2 every true positive adds to sim[g][k] in
// fixed point (RPC_KITTI_SIM_ONE = 2^40 = 1.0; the angles and the cosine are float64, so a term is off by the
// rounding to 2^-40, at most 2^-41, and a few 1e-16): integer sums in registers, one 64-bit integer vector atomic
// a lane — bit-reproducible.
template <bool EXT>
__global__ __launch_bounds__(64) void k_match_counts(const float* __restrict__ ov, const long long* __restrict__ ov_off,
                                                     const int* __restrict__ det_off, const int* __restrict__ gt_off,
                                                     int frames, int max_det, int max_gt,
                                                     const float* __restrict__ score,
                                                     const signed char* __restrict__ flag_det,
                                                     const signed char* __restrict__ flag_gt, long long n_det,
                                                     long long n_gt, const float* __restrict__ min_ov, int ntab,
                                                     const float* __restrict__ thr, const int* __restrict__ nthr,
                                                     int* __restrict__ counts, const unsigned char* __restrict__ stuff,
                                                     int gps, const double* __restrict__ alpha_det,
                                                     const double* __restrict__ alpha_gt,
                                                     unsigned long long* __restrict__ sim) {
  const int g = blockIdx.y, lane = threadIdx.x;
  const int nt = min(nthr[g], RPC_KITTI_MAX_THR);
  if (nt <= 0) return;   // a group without thresholds counts nothing
  const bool active = lane < nt;
  const float th = active ? thr[g * RPC_KITTI_MAX_THR + lane] : INFINITY;   // idle lanes match nothing
  const int row = g / ntab;
  const float mo = min_ov[g];
  int tp = 0, fp = 0, fn = 0;
  unsigned long long simq = 0ull;
  for (int f = blockIdx.x; f < frames; f += gridDim.x) {
    const Frame fr = frame_of(det_off, gt_off, ov_off, f, max_det, max_gt);
    const signed char* fd = flag_det + row * n_det + fr.d0;
    const signed char* fg = flag_gt + row * n_gt + fr.g0;
    unsigned long long ms[kWords];        // wave-uniform: detections inside a DontCare region (EXT only)
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
      ms[w] = 0ull;
      if constexpr (EXT)
        if (stuff) ms[w] = __ballot(in && stuff[(long long)(g / gps) * n_det + fr.d0 + j] != 0);
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
        if constexpr (EXT) {
          if (alpha_det && fgi == 0 && detf == 0) {   // per lane: its own true positive `det`
            const double v = (1.0 + cos(alpha_gt[fr.g0 + i] - alpha_det[fr.d0 + det])) * 0.5;
            simq += (unsigned long long)__double2ll_rn(fmin(fmax(v, 0.0), 1.0) * RPC_KITTI_SIM_ONE);   // NaN: 0
          }
        }
#pragma unroll
        for (int w = 0; w < kWords; ++w)
          if ((det >> 6) == w) asg[w] |= 1ull << (det & 63);
      }
    }
    // false positives: valid detections at or above the threshold that no ground truth took
#pragma unroll
    for (int w = 0; w < kWords; ++w) {
      unsigned long long m = m0[w] & ~ms[w];
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
    if constexpr (EXT)
      if (simq) atomicAdd(sim + (long long)g * RPC_KITTI_MAX_THR + lane, simq);
  }
}

// ---------------------------------------------------------------------------------- camera calibration
struct Range {
  float v[6];
};

// One thread per box. blockIdx.y walks the frames and, as index `frames`, the rows past the last offset (no frame:
// all outputs 0); blockIdx.x walks a frame's boxes 256 at a time, so a block never straddles a frame and stages
// its 12 matrix floats and (h, w) in LDS once. Every operation is a rounded fp32 one in the written order
// (__fmul_rn / __fadd_rn: no contraction), the order of tests/_kitti_calib_ref.py's float32 restatement.
__global__ __launch_bounds__(256) void k_project(const float* __restrict__ box, long long n, const int* __restrict__ off,
                                                 int frames, int max_box, const float* __restrict__ mat,
                                                 const float* __restrict__ hw, Range rg, float* __restrict__ raw,
                                                 float* __restrict__ clip, unsigned char* __restrict__ valid,
                                                 double* __restrict__ alpha, float* __restrict__ height) {
  __shared__ float sm[14];
  for (int f = blockIdx.y; f <= frames; f += gridDim.y) {
    const bool tail = f == frames;
    long long p0 = frames ? (long long)off[f] : 0ll, p1;
    if (tail) {
      p1 = n;
    } else {
      p1 = p0 + min(max(off[f + 1] - off[f], 0), max_box);
      if (threadIdx.x < 12) sm[threadIdx.x] = mat[12ll * f + threadIdx.x];
      if (threadIdx.x >= 12 && threadIdx.x < 14) sm[threadIdx.x] = hw[2ll * f + threadIdx.x - 12];
    }
    p0 = max(p0, 0ll);
    p1 = min(p1, n);
    __syncthreads();
    for (long long p = p0 + (long long)blockIdx.x * 256 + threadIdx.x; p < p1; p += (long long)gridDim.x * 256) {
      float o[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      double al = 0.0;
      bool ok = false;
      if (!tail) {
        const float* q = box + 7 * p;
        const float x = q[0], y = q[1], z = q[2], yaw = q[6];
        const float hx = __fmul_rn(q[3], 0.5f), hy = __fmul_rn(q[4], 0.5f), zt = __fadd_rn(z, q[5]);
        float s, c;
        sincosf(yaw, &s, &c);
        const float h = sm[12], w = sm[13];
        float x1 = INFINITY, y1 = INFINITY, x2 = -INFINITY, y2 = -INFINITY;
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float lx = (k & 1) ? -hx : hx, ly = (k & 2) ? -hy : hy, cz = (k & 4) ? zt : z;
          const float cx = __fsub_rn(__fadd_rn(x, __fmul_rn(lx, c)), __fmul_rn(ly, s));
          const float cy = __fadd_rn(__fadd_rn(y, __fmul_rn(lx, s)), __fmul_rn(ly, c));
          float r[3];
#pragma unroll
          for (int a = 0; a < 3; ++a)
            r[a] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(sm[4 * a], cx), __fmul_rn(sm[4 * a + 1], cy)),
                                       __fmul_rn(sm[4 * a + 2], cz)),
                             sm[4 * a + 3]);
          const float u = __fdiv_rn(r[0], r[2]), v = __fdiv_rn(r[1], r[2]);   // no depth test
          fin = fin && isfinite(u) && isfinite(v);
          x1 = fminf(x1, u), y1 = fminf(y1, v), x2 = fmaxf(x2, u), y2 = fmaxf(y2, v);
        }
        if (fin) {
          o[0] = x1, o[1] = y1, o[2] = x2, o[3] = y2;
          o[4] = fminf(fmaxf(x1, 0.0f), w), o[5] = fminf(fmaxf(y1, 0.0f), h);
          o[6] = fminf(fmaxf(x2, 0.0f), w), o[7] = fminf(fmaxf(y2, 0.0f), h);
          ok = x1 < w && y1 < h && x2 > 0.0f && y2 > 0.0f && x > rg.v[0] && y > rg.v[1] && z > rg.v[2] &&
               x < rg.v[3] && y < rg.v[4] && z < rg.v[5];   // a NaN centre fails every comparison
        } else {
          o[0] = o[1] = o[2] = o[3] = NAN;   // the clipped box stays (0, 0, 0, 0)
        }
        al = atan2((double)y, (double)x) - (double)yaw - 1.57079632679489661923;   // float64: AOS is held to 1e-9
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) raw[4 * p + k] = o[k], clip[4 * p + k] = o[4 + k];
      valid[p] = ok ? 1 : 0;
      alpha[p] = al;
      height[p] = __fsub_rn(o[7], o[5]);
    }
    __syncthreads();   // the next frame restages sm
  }
}

__device__ __forceinline__ float inter_2d(const float* a, const float* b) {
  const float iw = __fsub_rn(fminf(a[2], b[2]), fmaxf(a[0], b[0]));
  const float ih = __fsub_rn(fminf(a[3], b[3]), fmaxf(a[1], b[1]));
  return (iw > 0.0f && ih > 0.0f) ? __fmul_rn(iw, ih) : 0.0f;
}

// mode 0: IoU of detection j and ground truth i, one thread per pair as k_overlaps (the ground truths in LDS)
__global__ __launch_bounds__(256) void k_overlaps_2d(const float* __restrict__ det, const int* __restrict__ det_off,
                                                     const float* __restrict__ gt, const int* __restrict__ gt_off,
                                                     const long long* __restrict__ ov_off, int frames, int max_det,
                                                     int max_gt, float* __restrict__ ov) {
  __shared__ float sg[RPC_KITTI_MAX_GT][5];
  for (int f = blockIdx.y; f < frames; f += gridDim.y) {
    const Frame fr = frame_of(det_off, gt_off, ov_off, f, max_det, max_gt);
    const int npair = fr.nd * fr.ng;
    if ((int)blockIdx.x * 256 >= npair) continue;   // block-uniform
    for (int i = threadIdx.x; i < fr.ng; i += 256) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sg[i][k] = gt[4ll * (fr.g0 + i) + k];
    }
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < npair) {
      const int j = p / fr.ng, i = p - j * fr.ng;
      float b[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) b[k] = det[4ll * (fr.d0 + j) + k];
      const float* a = sg[i];
      float v = 0.0f;
      if (a[2] - a[0] > 0.0f && a[3] - a[1] > 0.0f && b[2] - b[0] > 0.0f && b[3] - b[1] > 0.0f) {
        const float in = inter_2d(a, b);
        const float aa = __fmul_rn(__fsub_rn(a[2], a[0]), __fsub_rn(a[3], a[1]));
        const float ab = __fmul_rn(__fsub_rn(b[2], b[0]), __fsub_rn(b[3], b[1]));
        if (in > 0.0f) v = __fdiv_rn(in, __fsub_rn(__fadd_rn(aa, ab), in));
      }
      ov[fr.o0 + p] = v;
    }
    __syncthreads();   // the next frame restages sg
  }
}

// mode 1: stuff[c][j] = some DontCare box i of j's frame has inter(j, i) / area(j) > min_ov[c], which is
// max_i ratio > min_ov[c]. One thread per detection, the frame's DontCare boxes in LDS. stuff was zeroed.
__global__ __launch_bounds__(256) void k_stuff(const float* __restrict__ det, const int* __restrict__ det_off,
                                               const float* __restrict__ dc, const int* __restrict__ dc_off,
                                               int frames, int max_det, int max_dc, const float* __restrict__ min_ov,
                                               int classes, long long n_det, unsigned char* __restrict__ stuff) {
  __shared__ float sd[RPC_KITTI_MAX_DC][4];
  for (int f = blockIdx.x; f < frames; f += gridDim.x) {
    const int d0 = det_off[f], nd = min(max(det_off[f + 1] - d0, 0), max_det);
    const int c0 = dc_off[f], nc = min(max(dc_off[f + 1] - c0, 0), max_dc);
    if (nd == 0 || nc == 0) continue;   // block-uniform
    for (int i = threadIdx.x; i < nc * 4; i += 256) sd[i >> 2][i & 3] = dc[4ll * c0 + i];
    __syncthreads();
    for (int j = threadIdx.x; j < nd; j += 256) {
      const long long row = (long long)d0 + j;
      if (row < 0 || row >= n_det) continue;
      float b[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) b[k] = det[4 * row + k];
      const float bw = __fsub_rn(b[2], b[0]), bh = __fsub_rn(b[3], b[1]);
      float best = 0.0f;
      if (bw > 0.0f && bh > 0.0f) {
        const float area = __fmul_rn(bw, bh);
        for (int i = 0; i < nc; ++i) best = fmaxf(best, __fdiv_rn(inter_2d(sd[i], b), area));
      }
      for (int c = 0; c < classes; ++c) stuff[c * n_det + row] = best > min_ov[c] ? 1 : 0;
    }
    __syncthreads();   // the next frame restages sd
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
  hipLaunchKernelGGL(k_match_counts<false>, dim3(frames < 256 ? frames : 256, groups), dim3(64), 0, st, ov, ov_off,
                     det_off, gt_off, frames, max_det, max_gt, score, flag_det, flag_gt, n_det, n_gt, min_ov, ntab, thr,
                     nthr, counts, (const unsigned char*)nullptr, 1, (const double*)nullptr, (const double*)nullptr,
                     (unsigned long long*)nullptr);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

int rpc_kitti_project(const float* boxes, long long n, const int* off, int frames, int max_box, const float* lidar2img,
                      const float* img_hw, const float* range, float* raw, float* clip, unsigned char* valid,
                      double* alpha, float* height, void* stream) {
  if (n < 0 || frames < 0 || max_box < 0) return RPC_ERR_ARG;
  if (!range || (frames && (!off || !lidar2img || !img_hw))) return RPC_ERR_ARG;
  if (n == 0) return RPC_OK;
  if (!boxes || !raw || !clip || !valid || !alpha || !height) return RPC_ERR_ARG;
  Range rg;
  for (int k = 0; k < 6; ++k) rg.v[k] = range[k];
  // x: a frame's boxes 256 at a time (a stride loop beyond 16 blocks, which also walks the rows of no frame)
  const dim3 grid(max_box > 256 ? (max_box < 4096 ? (max_box + 255) / 256 : 16) : 1,
                  frames + 1 < 65535 ? frames + 1 : 65535);
  hipLaunchKernelGGL(k_project, grid, dim3(256), 0, (hipStream_t)stream, boxes, n, off, frames, max_box, lidar2img,
                     img_hw, rg, raw, clip, valid, alpha, height);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

int rpc_kitti_overlaps_2d(const float* det, const int* det_off, const float* other, const int* other_off,
                          const long long* ov_off, int frames, int max_det, int max_other, int mode, float* ov,
                          const float* min_ov, int classes, long long n_det, unsigned char* stuff, void* stream) {
  if (mode != 0 && mode != 1) return RPC_ERR_ARG;
  if (frames < 0 || max_det < 0 || max_other < 0) return RPC_ERR_ARG;
  if (max_det > RPC_KITTI_MAX_DET || max_other > (mode ? RPC_KITTI_MAX_DC : RPC_KITTI_MAX_GT))
    return RPC_ERR_UNSUPPORTED;
  if (frames && (!det_off || !other_off || (mode == 0 && !ov_off))) return RPC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0) {
    if (frames == 0 || max_det == 0 || max_other == 0) return RPC_OK;
    if (!det || !other || !ov) return RPC_ERR_ARG;
    const dim3 grid((max_det * max_other + 255) / 256, frames < 65535 ? frames : 65535);
    hipLaunchKernelGGL(k_overlaps_2d, grid, dim3(256), 0, st, det, det_off, other, other_off, ov_off, frames, max_det,
                       max_other, ov);
  } else {
    if (classes < 0 || n_det < 0) return RPC_ERR_ARG;
    if (classes == 0 || n_det == 0) return RPC_OK;
    if (!stuff || !min_ov) return RPC_ERR_ARG;
    const bool work = frames && max_det && max_other;
    if (work && (!det || !other)) return RPC_ERR_ARG;
    RPC_CHECK(hipMemsetAsync(stuff, 0, (size_t)classes * (size_t)n_det, st));
    if (!work) return RPC_OK;
    hipLaunchKernelGGL(k_stuff, dim3(frames < 4096 ? frames : 4096), dim3(256), 0, st, det, det_off, other, other_off,
                       frames, max_det, max_other, min_ov, classes, n_det, stuff);
  }
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

int rpc_kitti_match_counts_aos(const float* ov, const long long* ov_off, const int* det_off, const int* gt_off,
                               int frames, int max_det, int max_gt, const float* score, const signed char* flag_det,
                               const signed char* flag_gt, long long n_det, long long n_gt, const float* min_ov,
                               int groups, int ntab, const float* thr, const int* nthr, const unsigned char* stuff,
                               int groups_per_stuff_row, const double* alpha_det, const double* alpha_gt, int* counts,
                               long long* sim, void* stream) {
  const int rc = check_match(ov, ov_off, det_off, gt_off, frames, max_det, max_gt, score, flag_det, flag_gt, n_det,
                             n_gt, min_ov, groups, ntab);
  if (rc != RPC_OK) return rc;
  if (stuff && (groups_per_stuff_row <= 0 || groups % groups_per_stuff_row)) return RPC_ERR_ARG;
  if (!alpha_det || !alpha_gt) alpha_det = alpha_gt = nullptr;   // the angles count only as a pair
  if (groups == 0) return RPC_OK;
  if (!thr || !nthr || !counts || !sim) return RPC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  RPC_CHECK(hipMemsetAsync(counts, 0, (size_t)groups * RPC_KITTI_MAX_THR * 3 * sizeof(int), st));
  RPC_CHECK(hipMemsetAsync(sim, 0, (size_t)groups * RPC_KITTI_MAX_THR * sizeof(long long), st));
  if (frames == 0) return RPC_OK;
  hipLaunchKernelGGL(k_match_counts<true>, dim3(frames < 256 ? frames : 256, groups), dim3(64), 0, st, ov, ov_off,
                     det_off, gt_off, frames, max_det, max_gt, score, flag_det, flag_gt, n_det, n_gt, min_ov, ntab, thr,
                     nthr, counts, stuff, stuff ? groups_per_stuff_row : 1, alpha_det, alpha_gt,
                     (unsigned long long*)sim);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

}  // extern "C"
