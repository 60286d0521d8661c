// §8(f2b): the GT-database augmentations of the training pipeline on the GPU (gfx950): points in rotated
// boxes, ObjectSample (GT paste) and ObjectNoise of configs/_base_/kitti-3d-car.py:42-68 (upstream mmdet3d
// v1.x transforms and mmcv's points_in_boxes, not vendored here; the rules are stated in DESIGN.md
// "GT-database augmentation").
//
// Conventions: box = (x, y, z, dx, dy, dz, yaw), z the bottom face; a box exists iff its label is >= 0 and
// its three extents are positive. Points are B frames back to back, [P][F] fp32, with device offsets [B+1];
// rows past offsets[B] belong to no frame. All random numbers come from the host; the device does the
// arithmetic and the decisions, and nothing here is read back by the host.
//
//   inside(p, box)   lx =  (px-x) cos + (py-y) sin, ly = -(px-x) sin + (py-y) cos;
//                    |lx| < dx/2 and |ly| < dy/2 and |pz - (z + dz/2)| <= dz/2   (mmcv check_pt_in_box3d)
//   collide(a, b)    separating axes on the four edge normals of the two footprints:
//                    sep = max_axes(|centre distance along axis| - sum of projected half extents) < 0
//
// Point kernels run one thread per point in blocks that never straddle a frame: frame b is covered by
// ceil(n_b / 256) blocks (block_span walks the B offsets), so a block stages its frame's boxes in LDS once
// (centre, half extents, cos, sin: 32 B a box, read as a broadcast by every lane).
//   k_pib           first containing box, optional bitmask of all, per-box counts (LDS atomics, then one
//                   global atomic per block and box)
//   k_sample_select one block per frame: candidate x (existing + candidate) collision bits in parallel into
//                   LDS bitmasks, then one lane walks the candidates (rules (a)-(c)) and fills free slots
//   k_sample_*      stable compaction of the scene points outside every accepted box behind the pasted
//                   objects: per-block keep counts, one small scan over blocks and frames, block scans
//   k_noise_select  one block per frame, boxes serial; tries x other boxes in parallel, first free try by
//                   an LDS minimum
//   k_noise_points  each point moves with the first box, in its original pose, that contains it
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <math.h>

#include "common.h"

namespace rpc {
namespace gta {

constexpr int BLK = 256;
constexpr int MAXB = RPC_GT_MAX_BOXES;   // boxes per frame, candidates per frame
constexpr int MAXT = RPC_GT_MAX_TRY;
static_assert(RPC_GT_MAX_CAND == RPC_GT_MAX_BOXES && RPC_GT_MAX_BOXES <= 128, "the bitmasks are four words");

struct ShBox {   // a box as the inside test reads it; hx < 0: the box does not exist
  float cx, cy, cz, hx, hy, hz, c, s;
};

struct Fp {      // a footprint as the collision test reads it; hx < 0: does not exist
  float cx, cy, hx, hy, c, s;
};

// blocks are laid frame after frame, then over the rows past offsets[B] (frame index B: no boxes)
__device__ __forceinline__ int span_blocks(const int* off, int B, int P, int f, int& s, int& e) {
  s = off[f < B ? f : B];
  e = f < B ? off[f + 1] : P;
  s = min(max(s, 0), P);
  e = min(max(e, s), P);
  return (e - s + BLK - 1) / BLK;
}

__device__ __forceinline__ bool block_span(const int* off, int B, int P, int blk, int& b, int& p0, int& p1) {
  int acc = 0;
  for (int f = 0; f <= B; ++f) {
    int s, e;
    const int nb = span_blocks(off, B, P, f, s, e);
    if (blk < acc + nb) {
      b = f;
      p0 = s + (blk - acc) * BLK;
      p1 = min(p0 + BLK, e);
      return true;
    }
    acc += nb;
  }
  return false;
}

__device__ __forceinline__ bool box_exists(const float* q, long long label) {
  return label >= 0 && q[3] > 0.0f && q[4] > 0.0f && q[5] > 0.0f;
}

__device__ __forceinline__ void stage_boxes(ShBox* sh, const float* boxes, const long long* labels, int M) {
  for (int m = threadIdx.x; m < M; m += BLK) {
    const float* q = boxes + (size_t)m * 7;
    const bool ex = box_exists(q, labels[m]);
    ShBox s;
    s.cx = q[0];
    s.cy = q[1];
    s.hz = q[5] * 0.5f;
    s.cz = q[2] + s.hz;
    s.hx = ex ? q[3] * 0.5f : -1.0f;
    s.hy = q[4] * 0.5f;
    s.c = cosf(q[6]);
    s.s = sinf(q[6]);
    sh[m] = s;
  }
}

__device__ __forceinline__ bool inside(const ShBox& q, float x, float y, float z) {
  const float dx = x - q.cx, dy = y - q.cy;
  const float lx = dx * q.c + dy * q.s;
  const float ly = dy * q.c - dx * q.s;
  return fabsf(lx) < q.hx && fabsf(ly) < q.hy && fabsf(z - q.cz) <= q.hz;   // NaN: every compare is false
}

__device__ __forceinline__ Fp footprint(const float* q, bool ex) {
  Fp f;
  f.cx = q[0];
  f.cy = q[1];
  f.hx = ex ? q[3] * 0.5f : -1.0f;
  f.hy = q[4] * 0.5f;
  f.c = cosf(q[6]);
  f.s = sinf(q[6]);
  return f;
}

// separating-axis margin of two footprints (negative: they overlap with positive area)
__device__ __forceinline__ float sat_sep(const Fp& a, const Fp& b) {
  const float dx = b.cx - a.cx, dy = b.cy - a.cy;
  const float cc = fabsf(a.c * b.c + a.s * b.s);
  const float ss = fabsf(a.s * b.c - a.c * b.s);
  const float s0 = fabsf(dx * a.c + dy * a.s) - (a.hx + b.hx * cc + b.hy * ss);
  const float s1 = fabsf(dy * a.c - dx * a.s) - (a.hy + b.hx * ss + b.hy * cc);
  const float s2 = fabsf(dx * b.c + dy * b.s) - (b.hx + a.hx * cc + a.hy * ss);
  const float s3 = fabsf(dy * b.c - dx * b.s) - (b.hy + a.hx * ss + a.hy * cc);
  return fmaxf(fmaxf(s0, s1), fmaxf(s2, s3));
}

// ---------------------------------------------------------------------------------- points in boxes
__global__ __launch_bounds__(BLK) void k_pib(const float* __restrict__ pts, int F, int P, const int* __restrict__ off,
                                             int B, const float* __restrict__ boxes,
                                             const long long* __restrict__ labels, int M, int* __restrict__ first,
                                             unsigned* __restrict__ mask, int* __restrict__ counts) {
  __shared__ ShBox sh[MAXB];
  __shared__ int cnt[MAXB];
  int b, p0, p1;
  if (!block_span(off, B, P, blockIdx.x, b, p0, p1)) return;
  const int Mf = b < B ? M : 0;
  if (Mf > 0) stage_boxes(sh, boxes + (size_t)b * M * 7, labels + (size_t)b * M, Mf);
  for (int m = threadIdx.x; m < Mf; m += BLK) cnt[m] = 0;
  __syncthreads();
  const int p = p0 + threadIdx.x;
  if (p < p1) {
    const float* q = pts + (size_t)p * F;
    const float x = q[0], y = q[1], z = q[2];
    const int W = (M + 31) >> 5;
    int fst = -1;
    unsigned word = 0;
    for (int m = 0; m < Mf; ++m) {
      if (inside(sh[m], x, y, z)) {
        if (fst < 0) fst = m;
        word |= 1u << (m & 31);
        if (counts) atomicAdd(&cnt[m], 1);
      }
      if ((m & 31) == 31 || m == Mf - 1) {
        if (mask) mask[(size_t)p * W + (m >> 5)] = word;
        word = 0;
      }
    }
    if (mask)
      for (int w = (Mf + 31) >> 5; w < W; ++w) mask[(size_t)p * W + w] = 0u;
    first[p] = fst;
  }
  __syncthreads();
  if (counts)
    for (int m = threadIdx.x; m < Mf; m += BLK)
      if (cnt[m]) atomicAdd(&counts[(size_t)b * M + m], cnt[m]);
}

// ---------------------------------------------------------------------------------- ObjectSample: selection
__global__ __launch_bounds__(BLK) void k_sample_select(const float* __restrict__ db_boxes,
                                                       const long long* __restrict__ db_labels, int N,
                                                       const int* __restrict__ cand, const int* __restrict__ draw,
                                                       int S, float* __restrict__ gt_boxes,
                                                       long long* __restrict__ gt_labels, int M,
                                                       int* __restrict__ accept) {
  __shared__ Fp ex[MAXB];
  __shared__ Fp ca[MAXB];
  __shared__ unsigned colE[MAXB][4];
  __shared__ unsigned colC[MAXB][4];
  const int b = blockIdx.x;
  float* gb = gt_boxes + (size_t)b * M * 7;
  long long* gl = gt_labels + (size_t)b * M;
  const int* cd = cand + (size_t)b * S;
  for (int m = threadIdx.x; m < M; m += BLK) ex[m] = footprint(gb + (size_t)m * 7, box_exists(gb + (size_t)m * 7, gl[m]));
  for (int i = threadIdx.x; i < S; i += BLK) {
    const int c = cd[i];
    if (c >= 0 && c < N) {
      ca[i] = footprint(db_boxes + (size_t)c * 7, box_exists(db_boxes + (size_t)c * 7, db_labels[c]));
    } else {
      Fp f = {0.0f, 0.0f, -1.0f, 0.0f, 1.0f, 0.0f};
      ca[i] = f;
    }
    for (int w = 0; w < 4; ++w) colE[i][w] = colC[i][w] = 0u;
  }
  __syncthreads();
  const int K = M + S;
  for (int q = threadIdx.x; q < S * K; q += BLK) {
    const int i = q / K, k = q - i * K;
    if (k - M == i) continue;
    const Fp a = ca[i];
    const Fp o = k < M ? ex[k] : ca[k - M];
    if (a.hx < 0.0f || o.hx < 0.0f) continue;
    if (sat_sep(a, o) < 0.0f) {
      if (k < M) atomicOr(&colE[i][k >> 5], 1u << (k & 31));
      else atomicOr(&colC[i][(k - M) >> 5], 1u << ((k - M) & 31));
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // the serial walk: candidate i of a draw is accepted iff it collides with no existing box, no candidate
  // accepted before it, and no later candidate of its own draw (whatever becomes of that one)
  unsigned acc[4] = {0u, 0u, 0u, 0u};
  int slot = 0, dend = 0;
  for (int i = 0; i < S; ++i) {
    int got = -1;
    if (ca[i].hx >= 0.0f) {
      if (i >= dend) {
        const int d = draw[(size_t)b * S + i];
        dend = i + 1;
        while (dend < S && draw[(size_t)b * S + dend] == d) ++dend;
      }
      bool hit = false;
      for (int w = 0; w < 4; ++w) {
        // bits of the candidates in (i, dend)
        const int lo = max(i + 1 - 32 * w, 0), hi = min(dend - 32 * w, 32);
        unsigned later = 0u;
        if (hi > lo) later = (hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
        hit = hit || colE[i][w] != 0u || (colC[i][w] & (acc[w] | later)) != 0u;
      }
      if (!hit) {
        while (slot < M && gl[slot] >= 0) ++slot;
        if (slot < M) {
          const int c = cd[i];
          for (int k = 0; k < 7; ++k) gb[(size_t)slot * 7 + k] = db_boxes[(size_t)c * 7 + k];
          gl[slot] = db_labels[c];
          acc[i >> 5] |= 1u << (i & 31);
          got = slot++;
        }
      }
    }
    accept[(size_t)b * S + i] = got;
  }
}

// ---------------------------------------------------------------------------------- ObjectSample: points
// per frame: the accepted objects' boxes as a box table for k_pib, each object's first output row (relative
// to the frame's start) and the frame's pasted total
__global__ __launch_bounds__(MAXB) void k_sample_prepare(const int* __restrict__ cand, const int* __restrict__ accept,
                                                         int S, const int* __restrict__ db_off,
                                                         const float* __restrict__ db_boxes, int N,
                                                         float* __restrict__ sel_boxes,
                                                         long long* __restrict__ sel_labels,
                                                         int* __restrict__ paste_start, int* __restrict__ paste_total) {
  typedef hipcub::BlockScan<int, MAXB> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const int b = blockIdx.x, i = threadIdx.x;
  int n = 0;
  if (i < S) {
    const int c = cand[(size_t)b * S + i];
    const bool ok = accept[(size_t)b * S + i] >= 0 && c >= 0 && c < N;
    if (ok) n = max(db_off[c + 1] - db_off[c], 0);
    for (int k = 0; k < 7; ++k) sel_boxes[((size_t)b * S + i) * 7 + k] = ok ? db_boxes[(size_t)c * 7 + k] : 0.0f;
    sel_labels[(size_t)b * S + i] = ok ? 0 : -1;
  }
  int start, total;
  Scan(tmp).ExclusiveSum(n, start, total);
  if (i < S) paste_start[(size_t)b * S + i] = start;
  if (i == 0) paste_total[b] = total;
}

__global__ __launch_bounds__(BLK) void k_sample_count(const int* __restrict__ first, int P, const int* __restrict__ off,
                                                      int B, int* __restrict__ blockcnt) {
  int b, p0, p1;
  int keep = 0;
  if (block_span(off, B, P, blockIdx.x, b, p0, p1)) {
    const int p = p0 + threadIdx.x;
    keep = (b < B && p < p1 && first[p] < 0) ? 1 : 0;
  }
  const int n = __syncthreads_count(keep);
  if (threadIdx.x == 0) blockcnt[blockIdx.x] = n;
}

// one block: exclusive scan of the per-block keep counts, then each frame's first block and output offset
__global__ __launch_bounds__(BLK) void k_sample_scan(const int* __restrict__ blockcnt, int nblk,
                                                     const int* __restrict__ off, int B, int P,
                                                     const int* __restrict__ paste_total, int* __restrict__ blockoff,
                                                     int* __restrict__ frame_blk, int* __restrict__ out_off) {
  typedef hipcub::BlockScan<int, BLK> Scan;
  __shared__ typename Scan::TempStorage tmp;
  __shared__ int run;
  if (threadIdx.x == 0) run = 0;
  __syncthreads();
  for (int base = 0; base < nblk; base += BLK) {
    const int k = base + threadIdx.x;
    const int v = k < nblk ? blockcnt[k] : 0;
    int e, total;
    Scan(tmp).ExclusiveSum(v, e, total);
    if (k < nblk) blockoff[k] = run + e;
    __syncthreads();
    if (threadIdx.x == 0) run += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    blockoff[nblk] = run;
    int acc = 0, pasted = 0;
    for (int f = 0; f <= B; ++f) {
      int s, e;
      const int nb = span_blocks(off, B, P, f, s, e);
      frame_blk[f] = acc;
      out_off[f] = blockoff[min(acc, nblk)] + pasted;   // kept scene points of earlier frames + their pastes
      if (f < B) pasted += paste_total[f];
      acc += nb;
    }
  }
}

__global__ __launch_bounds__(BLK) void k_sample_compact(const float* __restrict__ pts, int F, int P,
                                                        const int* __restrict__ off, int B,
                                                        const int* __restrict__ first,
                                                        const int* __restrict__ blockoff,
                                                        const int* __restrict__ frame_blk,
                                                        const int* __restrict__ paste_total,
                                                        const int* __restrict__ out_off, float* __restrict__ out,
                                                        int cap) {
  typedef hipcub::BlockScan<int, BLK> Scan;
  __shared__ typename Scan::TempStorage tmp;
  int b, p0, p1;
  if (!block_span(off, B, P, blockIdx.x, b, p0, p1) || b >= B) return;
  const int p = p0 + threadIdx.x;
  const int keep = (p < p1 && first[p] < 0) ? 1 : 0;
  int rank;
  Scan(tmp).ExclusiveSum(keep, rank);
  if (!keep) return;
  const int row = out_off[b] + paste_total[b] + (blockoff[blockIdx.x] - blockoff[frame_blk[b]]) + rank;
  if (row < 0 || row >= cap) return;
  const float* s = pts + (size_t)p * F;
  float* d = out + (size_t)row * F;
  for (int f = 0; f < F; ++f) d[f] = s[f];
}

// block (i, b): the points of accepted candidate i of frame b, translated by the object's box origin
__global__ __launch_bounds__(BLK) void k_sample_paste(const int* __restrict__ cand, const int* __restrict__ accept,
                                                      int S, const float* __restrict__ db_pts, int F,
                                                      const int* __restrict__ db_off,
                                                      const float* __restrict__ db_boxes, int N,
                                                      const int* __restrict__ paste_start,
                                                      const int* __restrict__ out_off, float* __restrict__ out,
                                                      int cap) {
  const int i = blockIdx.x, b = blockIdx.y;
  const int c = cand[(size_t)b * S + i];
  if (accept[(size_t)b * S + i] < 0 || c < 0 || c >= N) return;
  const int q0 = db_off[c], n = db_off[c + 1] - q0;
  const float ox = db_boxes[(size_t)c * 7], oy = db_boxes[(size_t)c * 7 + 1], oz = db_boxes[(size_t)c * 7 + 2];
  const int row0 = out_off[b] + paste_start[(size_t)b * S + i];
  for (int k = threadIdx.x; k < n; k += BLK) {
    const int row = row0 + k;
    if (row < 0 || row >= cap) continue;
    const float* s = db_pts + (size_t)(q0 + k) * F;
    float* d = out + (size_t)row * F;
    d[0] = s[0] + ox;
    d[1] = s[1] + oy;
    d[2] = s[2] + oz;
    for (int f = 3; f < F; ++f) d[f] = s[f];
  }
}

__global__ __launch_bounds__(BLK) void k_nan_tail(float* __restrict__ out, int F, int cap,
                                                  const int* __restrict__ out_off, int B) {
  const int r = blockIdx.x * BLK + threadIdx.x;
  if (r >= cap || r < out_off[B]) return;
  float* d = out + (size_t)r * F;
  for (int f = 0; f < F; ++f) d[f] = __builtin_nanf("");
}

// ---------------------------------------------------------------------------------- ObjectNoise
__global__ __launch_bounds__(BLK) void k_noise_select(const float* __restrict__ gt_boxes,
                                                      const long long* __restrict__ gt_labels, int M,
                                                      const float* __restrict__ loc, const float* __restrict__ rot,
                                                      int T, int* __restrict__ chosen) {
  __shared__ Fp cur[MAXB];
  __shared__ float tcx[MAXT], tcy[MAXT], tc[MAXT], ts[MAXT];
  __shared__ int fail[MAXT];
  __shared__ int best;
  const int b = blockIdx.x;
  const float* gb = gt_boxes + (size_t)b * M * 7;
  const long long* gl = gt_labels + (size_t)b * M;
  for (int m = threadIdx.x; m < M; m += BLK) cur[m] = footprint(gb + (size_t)m * 7, box_exists(gb + (size_t)m * 7, gl[m]));
  __syncthreads();
  for (int i = 0; i < M; ++i) {
    if (cur[i].hx < 0.0f) {   // block-uniform
      if (threadIdx.x == 0) chosen[(size_t)b * M + i] = -1;
      continue;
    }
    const float yaw = gb[(size_t)i * 7 + 6];
    const float* li = loc + ((size_t)b * M + i) * T * 3;
    const float* ri = rot + ((size_t)b * M + i) * T;
    for (int j = threadIdx.x; j < T; j += BLK) {
      const float a = yaw + ri[j];
      tcx[j] = cur[i].cx + li[(size_t)j * 3];
      tcy[j] = cur[i].cy + li[(size_t)j * 3 + 1];
      tc[j] = cosf(a);
      ts[j] = sinf(a);
      fail[j] = 0;
    }
    if (threadIdx.x == 0) best = INT_MAX;
    __syncthreads();
    for (int q = threadIdx.x; q < T * M; q += BLK) {
      const int j = q / M, k = q - j * M;
      if (k == i || cur[k].hx < 0.0f) continue;
      Fp t;
      t.cx = tcx[j];
      t.cy = tcy[j];
      t.hx = cur[i].hx;
      t.hy = cur[i].hy;
      t.c = tc[j];
      t.s = ts[j];
      if (sat_sep(t, cur[k]) < 0.0f) fail[j] = 1;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < T; j += BLK)
      if (!fail[j]) atomicMin(&best, j);
    __syncthreads();
    if (threadIdx.x == 0) {
      const int j = best;
      if (j != INT_MAX) {
        cur[i].cx = tcx[j];
        cur[i].cy = tcy[j];
        cur[i].c = tc[j];
        cur[i].s = ts[j];
      }
      chosen[(size_t)b * M + i] = j == INT_MAX ? -1 : j;
    }
    __syncthreads();
  }
}

// in place: p' = R(rot) (p - c_xy) + c_xy + loc, z' = z + loc_z for the first original box around p
__global__ __launch_bounds__(BLK) void k_noise_points(float* __restrict__ pts, int F, int P, const int* __restrict__ off,
                                                      int B, const float* __restrict__ boxes,
                                                      const long long* __restrict__ labels, int M,
                                                      const float* __restrict__ loc, const float* __restrict__ rot,
                                                      int T, const int* __restrict__ chosen) {
  __shared__ ShBox sh[MAXB];
  int b, p0, p1;
  if (!block_span(off, B, P, blockIdx.x, b, p0, p1) || b >= B) return;
  stage_boxes(sh, boxes + (size_t)b * M * 7, labels + (size_t)b * M, M);
  __syncthreads();
  const int p = p0 + threadIdx.x;
  if (p >= p1) return;
  float* q = pts + (size_t)p * F;
  const float x = q[0], y = q[1], z = q[2];
  int m = 0;
  while (m < M && !inside(sh[m], x, y, z)) ++m;
  if (m == M) return;
  const int j = chosen[(size_t)b * M + m];
  if (j < 0 || j >= T) return;
  const float* l = loc + (((size_t)b * M + m) * T + j) * 3;
  const float r = rot[((size_t)b * M + m) * T + j];
  const float c = cosf(r), s = sinf(r);
  const float dx = x - sh[m].cx, dy = y - sh[m].cy;
  q[0] = (dx * c - dy * s) + sh[m].cx + l[0];
  q[1] = (dx * s + dy * c) + sh[m].cy + l[1];
  q[2] = z + l[2];
}

__global__ __launch_bounds__(BLK) void k_noise_boxes(float* __restrict__ boxes, int BM, const float* __restrict__ loc,
                                                     const float* __restrict__ rot, int T,
                                                     const int* __restrict__ chosen) {
  const int t = blockIdx.x * BLK + threadIdx.x;
  if (t >= BM) return;
  const int j = chosen[t];
  if (j < 0 || j >= T) return;
  const float* l = loc + ((size_t)t * T + j) * 3;
  float* q = boxes + (size_t)t * 7;
  q[0] += l[0];
  q[1] += l[1];
  q[2] += l[2];
  q[6] += rot[(size_t)t * T + j];
}

}  // namespace gta
}  // namespace rpc

using namespace rpc;
using namespace rpc::gta;

static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

static unsigned span_grid(int P, int B) { return (unsigned)((P + BLK - 1) / BLK + B + 1); }

extern "C" int rpc_points_in_boxes(const float* points, int F, int P, const int* frame_offsets, int B,
                                   const float* boxes, const long long* labels, int M, int* first, unsigned* mask,
                                   int* counts, void* stream) {
  if (F < 3 || P < 0 || B < 0 || M < 0 || !frame_offsets) return RPC_ERR_ARG;
  if (P > 0 && (!points || !first)) return RPC_ERR_ARG;
  if ((long long)B * M > 0 && (!boxes || !labels || !counts)) return RPC_ERR_ARG;
  if (M > RPC_GT_MAX_BOXES) return RPC_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if ((long long)B * M > 0) RPC_CHECK(hipMemsetAsync(counts, 0, sizeof(int) * (size_t)B * M, st));
  if (P == 0) return RPC_OK;
  hipLaunchKernelGGL(k_pib, dim3(span_grid(P, B)), dim3(BLK), 0, st, points, F, P, frame_offsets, B, boxes, labels, M,
                     first, mask, (long long)B * M > 0 ? counts : (int*)nullptr);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

extern "C" int rpc_object_sample_select(const float* db_boxes, const long long* db_labels, int N, const int* cand,
                                        const int* draw, int B, int S, float* gt_boxes, long long* gt_labels, int M,
                                        int* accept, void* stream) {
  if (N < 0 || B < 0 || S < 0 || M < 0) return RPC_ERR_ARG;
  if (N > 0 && (!db_boxes || !db_labels)) return RPC_ERR_ARG;
  if ((long long)B * S > 0 && (!cand || !draw || !accept)) return RPC_ERR_ARG;
  if ((long long)B * M > 0 && (!gt_boxes || !gt_labels)) return RPC_ERR_ARG;
  if (M > RPC_GT_MAX_BOXES || S > RPC_GT_MAX_CAND) return RPC_ERR_UNSUPPORTED;
  if (B == 0 || S == 0) return RPC_OK;
  hipLaunchKernelGGL(k_sample_select, dim3((unsigned)B), dim3(BLK), 0, (hipStream_t)stream, db_boxes, db_labels, N,
                     cand, draw, S, gt_boxes, gt_labels, M, accept);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

struct SampleWs {
  size_t sel_boxes, sel_labels, paste_start, paste_total, first, blockcnt, blockoff, frame_blk, total;
  int nblk;
};

static SampleWs sample_ws(int P, int B, int S) {
  SampleWs w;
  w.nblk = (int)span_grid(P, B);
  const size_t bs = (size_t)(B > 0 ? B : 1) * (size_t)(S > 0 ? S : 1);
  size_t o = 0;
  w.sel_boxes = o; o += al256(sizeof(float) * 7 * bs);
  w.sel_labels = o; o += al256(sizeof(long long) * bs);
  w.paste_start = o; o += al256(sizeof(int) * bs);
  w.paste_total = o; o += al256(sizeof(int) * (size_t)(B + 1));
  w.first = o; o += al256(sizeof(int) * (size_t)(P > 0 ? P : 1));
  w.blockcnt = o; o += al256(sizeof(int) * (size_t)w.nblk);
  w.blockoff = o; o += al256(sizeof(int) * (size_t)(w.nblk + 1));
  w.frame_blk = o; o += al256(sizeof(int) * (size_t)(B + 1));
  w.total = o;
  return w;
}

extern "C" size_t rpc_object_sample_points_workspace_size(int total_points, int batch, int max_cand) {
  if (total_points < 0 || batch < 0 || max_cand < 0) return 0;
  return sample_ws(total_points, batch, max_cand).total;
}

extern "C" int rpc_object_sample_points(const float* points, int F, int P, const int* frame_offsets, int B,
                                        const float* db_points, const int* db_offsets, const float* db_boxes, int N,
                                        const int* cand, const int* accept, int S, float* out_points, int cap,
                                        int* out_offsets, void* workspace, size_t ws_bytes, void* stream) {
  if (F < 3 || P < 0 || B < 0 || N < 0 || S < 0 || cap < 0 || !frame_offsets || !out_offsets || !workspace)
    return RPC_ERR_ARG;
  if (P > 0 && !points) return RPC_ERR_ARG;
  if (N > 0 && (!db_offsets || !db_boxes)) return RPC_ERR_ARG;
  if ((long long)B * S > 0 && (!cand || !accept)) return RPC_ERR_ARG;
  if (cap > 0 && !out_points) return RPC_ERR_ARG;
  if (S > RPC_GT_MAX_CAND || B > 65535) return RPC_ERR_UNSUPPORTED;
  const SampleWs w = sample_ws(P, B, S);
  if (ws_bytes < w.total) return RPC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace;
  float* sel_boxes = (float*)(base + w.sel_boxes);
  long long* sel_labels = (long long*)(base + w.sel_labels);
  int* paste_start = (int*)(base + w.paste_start);
  int* paste_total = (int*)(base + w.paste_total);
  int* first = (int*)(base + w.first);
  int* blockcnt = (int*)(base + w.blockcnt);
  int* blockoff = (int*)(base + w.blockoff);
  int* frame_blk = (int*)(base + w.frame_blk);
  const bool cands = B > 0 && S > 0;
  if (cands) {
    hipLaunchKernelGGL(k_sample_prepare, dim3((unsigned)B), dim3(MAXB), 0, st, cand, accept, S, db_offsets, db_boxes, N,
                       sel_boxes, sel_labels, paste_start, paste_total);
    RPC_LAUNCH_CHECK();
  } else {
    RPC_CHECK(hipMemsetAsync(paste_total, 0, sizeof(int) * (size_t)(B + 1), st));
  }
  const unsigned nblk = (unsigned)w.nblk;
  if (P > 0) {
    hipLaunchKernelGGL(k_pib, dim3(nblk), dim3(BLK), 0, st, points, F, P, frame_offsets, B, (const float*)sel_boxes,
                       (const long long*)sel_labels, cands ? S : 0, first, (unsigned*)nullptr, (int*)nullptr);
    RPC_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_sample_count, dim3(nblk), dim3(BLK), 0, st, (const int*)first, P, frame_offsets, B, blockcnt);
  RPC_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(BLK), 0, st, (const int*)blockcnt, (int)nblk, frame_offsets, B, P,
                     (const int*)paste_total, blockoff, frame_blk, out_offsets);
  RPC_LAUNCH_CHECK();
  if (P > 0 && B > 0) {
    hipLaunchKernelGGL(k_sample_compact, dim3(nblk), dim3(BLK), 0, st, points, F, P, frame_offsets, B,
                       (const int*)first, (const int*)blockoff, (const int*)frame_blk, (const int*)paste_total,
                       (const int*)out_offsets, out_points, cap);
    RPC_LAUNCH_CHECK();
  }
  if (cands) {
    hipLaunchKernelGGL(k_sample_paste, dim3((unsigned)S, (unsigned)B), dim3(BLK), 0, st, cand, accept, S, db_points, F,
                       db_offsets, db_boxes, N, (const int*)paste_start, (const int*)out_offsets, out_points, cap);
    RPC_LAUNCH_CHECK();
  }
  if (cap > 0) {
    hipLaunchKernelGGL(k_nan_tail, dim3((unsigned)((cap + BLK - 1) / BLK)), dim3(BLK), 0, st, out_points, F, cap,
                       (const int*)out_offsets, B);
    RPC_LAUNCH_CHECK();
  }
  return RPC_OK;
}

extern "C" int rpc_object_noise_select(const float* gt_boxes, const long long* gt_labels, int B, int M,
                                       const float* loc, const float* rot, int T, int* chosen, void* stream) {
  if (B < 0 || M < 0 || T < 0) return RPC_ERR_ARG;
  if ((long long)B * M > 0 && (!gt_boxes || !gt_labels || !chosen)) return RPC_ERR_ARG;
  if ((long long)B * M * T > 0 && (!loc || !rot)) return RPC_ERR_ARG;
  if (M > RPC_GT_MAX_BOXES || T > RPC_GT_MAX_TRY) return RPC_ERR_UNSUPPORTED;
  if (B == 0 || M == 0) return RPC_OK;
  hipLaunchKernelGGL(k_noise_select, dim3((unsigned)B), dim3(BLK), 0, (hipStream_t)stream, gt_boxes, gt_labels, M, loc,
                     rot, T, chosen);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

extern "C" int rpc_object_noise_apply(float* points, int F, int P, const int* frame_offsets, int B, float* gt_boxes,
                                      const long long* gt_labels, int M, const float* loc, const float* rot, int T,
                                      const int* chosen, void* stream) {
  if (F < 3 || P < 0 || B < 0 || M < 0 || T < 0 || !frame_offsets) return RPC_ERR_ARG;
  if (P > 0 && !points) return RPC_ERR_ARG;
  if ((long long)B * M > 0 && (!gt_boxes || !gt_labels || !chosen)) return RPC_ERR_ARG;
  if ((long long)B * M * T > 0 && (!loc || !rot)) return RPC_ERR_ARG;
  if (M > RPC_GT_MAX_BOXES || T > RPC_GT_MAX_TRY) return RPC_ERR_UNSUPPORTED;
  if (B == 0 || M == 0 || T == 0) return RPC_OK;
  hipStream_t st = (hipStream_t)stream;
  if (P > 0) {   // the point pass reads the boxes' original poses: it goes first
    hipLaunchKernelGGL(k_noise_points, dim3(span_grid(P, B)), dim3(BLK), 0, st, points, F, P, frame_offsets, B,
                       (const float*)gt_boxes, gt_labels, M, loc, rot, T, chosen);
    RPC_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_noise_boxes, dim3((unsigned)((B * M + BLK - 1) / BLK)), dim3(BLK), 0, st, gt_boxes, B * M, loc,
                     rot, T, chosen);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}
