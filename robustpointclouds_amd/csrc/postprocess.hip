// Detection post-processing for gfx950: what `predict` needs after the heads (include/rpc_hip.h, "predict").
//   rpc_bev_iou_pairs   BEV IoU of n pairs of rotated boxes                          (bev_iou.h)
//   rpc_nms_bev         greedy rotated NMS, all groups (frames x classes) in one call (mmcv nms_rotated)
//   rpc_nms_circle      greedy centre-distance NMS, all groups (frames x tasks)      (mmdet3d circle_nms)
//   rpc_anchor_decode   sigmoid scores + DeltaXYZWLHRBBoxCoder.decode + dir label of the candidate anchors
//   rpc_center_decode   CenterPointBBoxCoder.decode of the top-K heatmap cells from the packed head buffers
// No MFMA here. NMS is two launches for all groups, with no host read between them:
//   mask:  one wave per 64 x 64 tile of the upper triangle of a group's pair matrix. The column tile's boxes are
//          staged in LDS (every lane then reads the same address: a broadcast, no bank conflict); lane r owns
//          row 64 * rt + r and builds the 64-bit word of the columns it suppresses.
//   scan:  one wave per group; lane w holds word w of `removed` in a register (hence the cap of 64 words = 4096
//          boxes). Per 64-row tile the diagonal words resolve the tile's rows in order (a register-only loop over
//          i: row i is kept when its bit in `removed` is clear, and then ORs its word in); the rows kept then OR
//          their later words into `removed`, four independent loads in flight. It stops at max_keep.
#include <hip/hip_runtime.h>

#include "bev_iou.h"
#include "common.h"

namespace rpc {
namespace post {

constexpr int kTile = 64;

__global__ __launch_bounds__(256) void k_iou_pairs(const float* __restrict__ a, const float* __restrict__ b, int n,
                                                   float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* pa = a + 5ll * i;
  const float* pb = b + 5ll * i;
  float sa, ca;
  sincosf(pa[4], &sa, &ca);
  out[i] = bev::iou_cs(pa[0], pa[1], pa[2], pa[3], pa[4], ca, sa, pb[0], pb[1], pb[2], pb[3], pb[4]);
}

// tile pair (rt <= ct) of the linear upper-triangle index t, T tiles a side
__device__ __forceinline__ void tri_decode(int t, int T, int& rt, int& ct) {
  int r = 0;
  while (t >= T - r) {
    t -= T - r;
    ++r;
  }
  rt = r;
  ct = r + t;
}

__device__ __forceinline__ int group_count(const int* counts, int g, int max_n) {
  return min(max(counts[g], 0), max_n);
}

// mask[g][i][w]: bit c of word w set when row i suppresses column 64 w + c (> i, < count)
template <bool CIRCLE>
__global__ __launch_bounds__(64) void k_nms_mask(const float* __restrict__ boxes, const int* __restrict__ counts,
                                                 const float* __restrict__ radius, int max_n, int T, float thr,
                                                 unsigned long long* __restrict__ mask) {
  constexpr int D = CIRCLE ? 2 : 5;
  __shared__ float col[kTile][D];
  const int g = blockIdx.y;
  const int n = group_count(counts, g, max_n);
  int rt, ct;
  tri_decode(blockIdx.x, T, rt, ct);
  if (rt * kTile >= n || ct * kTile >= n) return;   // block-uniform
  const int lane = threadIdx.x;
  const float* gb = boxes + (long long)g * max_n * D;
  const int j0 = ct * kTile;
  {
    const int j = j0 + lane;
#pragma unroll
    for (int k = 0; k < D; ++k) col[lane][k] = j < n ? gb[(long long)j * D + k] : 0.0f;
  }
  __syncthreads();
  const int i = rt * kTile + lane;
  if (i >= n) return;
  float a[D];
#pragma unroll
  for (int k = 0; k < D; ++k) a[k] = gb[(long long)i * D + k];
  const int jend = min(kTile, n - j0);
  unsigned long long word = 0;
  if constexpr (CIRCLE) {
    // mmdet3d circle_nms parity: the SQUARED centre distance is compared with the UNSQUARED min_radius, and the
    // comparison is non-strict (`dist <= thresh`)
    const float r = radius[g];
    for (int c = 0; c < jend; ++c) {
      const float dx = a[0] - col[c][0], dy = a[1] - col[c][1];
      const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
      if (j0 + c > i && d2 <= r) word |= 1ull << c;
    }
  } else {
    float sa, ca;
    sincosf(a[4], &sa, &ca);
    for (int c = 0; c < jend; ++c) {
      if (j0 + c > i) {   // strict, as mmcv nms_rotated: suppressed when IoU > thr
        const float v = bev::iou_cs(a[0], a[1], a[2], a[3], a[4], ca, sa, col[c][0], col[c][1], col[c][2],
                                    col[c][3], col[c][4]);
        if (v > thr) word |= 1ull << c;
      }
    }
  }
  mask[((long long)g * max_n + i) * T + ct] = word;
}

__global__ __launch_bounds__(64) void k_nms_scan(const unsigned long long* __restrict__ mask,
                                                 const int* __restrict__ counts, int max_n, int T, int max_keep,
                                                 int* __restrict__ keep, int* __restrict__ nkeep) {
  const int g = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = group_count(counts, g, max_n);
  const unsigned long long* gm = mask + (long long)g * max_n * T;
  int* gk = keep + (long long)g * max_keep;
  unsigned long long rem = 0;   // lane w: word w of `removed`
  int nk = 0;
  const int tiles = (n + kTile - 1) / kTile;
  for (int rt = 0; rt < tiles && nk < max_keep; ++rt) {
    const int i0 = rt * kTile;
    const int rows = min(kTile, n - i0);
    const unsigned long long diag = lane < rows ? gm[(long long)(i0 + lane) * T + rt] : 0ull;
    unsigned long long dead = __shfl(rem, rt, 64);   // the tile's word of `removed`, wave-uniform
    unsigned long long alive = 0;
    for (int b = 0; b < rows && nk < max_keep; ++b) {
      const unsigned long long row = __shfl(diag, b, 64);
      if (!((dead >> b) & 1ull)) {
        dead |= row;
        alive |= 1ull << b;
        if (lane == 0) gk[nk] = i0 + b;
        ++nk;
      }
    }
    // rows kept in this tile suppress columns of the later tiles
    const bool mine = lane > rt && lane < tiles;
    unsigned long long acc = 0;
    int last = 0;
    while (alive) {
      int b[4];   // the next four kept rows; when fewer are left the last repeats (OR is idempotent)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (alive) {
          last = __ffsll((long long)alive) - 1;
          alive &= alive - 1;
        }
        b[k] = last;
      }
      if (mine) {
        unsigned long long v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = gm[(long long)(i0 + b[k]) * T + lane];
        acc |= (v[0] | v[1]) | (v[2] | v[3]);
      }
    }
    rem |= acc;
  }
  for (int k = nk + lane; k < max_keep; k += kTile) gk[k] = -1;
  if (lane == 0) nkeep[g] = nk;
}

struct DecodeStrides {
  long long s[3][4];   // cls / reg / dir maps: element strides of (frame, channel, row, column)
};

__global__ __launch_bounds__(256) void k_anchor_decode(const int* __restrict__ cand, int B, int K, int H, int W,
                                                       int S, int R, int C, const float* __restrict__ tab,
                                                       const float* __restrict__ cls, const float* __restrict__ reg,
                                                       const float* __restrict__ dir, DecodeStrides st,
                                                       float* __restrict__ scores, float* __restrict__ boxes,
                                                       int* __restrict__ dir_label) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * K) return;
  const int b = t / K;
  int idx = cand[t];
  const int N = H * W * S * R;
  idx = min(max(idx, 0), N - 1);
  const int r = idx % R, s = (idx / R) % S, w = (idx / (R * S)) % W, h = idx / (R * S * W);
  const int a = s * R + r;
  // anchor_table layout: xc[S][W], yc[S][H], zc[S], sizes[S][3], rotations[R]
  const float* xc = tab;
  const float* yc = xc + S * W;
  const float* zc = yc + S * H;
  const float* sz = zc + S;
  const float* rot = sz + 3 * S;
  const float xa = xc[s * W + w], ya = yc[s * H + h], wa = sz[3 * s], la = sz[3 * s + 1], ha = sz[3 * s + 2];
  const float za = zc[s] + ha / 2, ra = rot[r];
  const long long oc = b * st.s[0][0] + h * st.s[0][2] + w * st.s[0][3];
  for (int c = 0; c < C; ++c) {
    const float z = cls[oc + (long long)(a * C + c) * st.s[0][1]];
    scores[(long long)t * C + c] = 1.0f / (1.0f + expf(-z));
  }
  const long long orr = b * st.s[1][0] + h * st.s[1][2] + w * st.s[1][3];
  float d[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) d[k] = reg[orr + (long long)(a * 7 + k) * st.s[1][1]];
  const float diag = sqrtf(la * la + wa * wa);
  const float xg = d[0] * diag + xa, yg = d[1] * diag + ya, zg = d[2] * ha + za;
  const float wg = expf(d[3]) * wa, lg = expf(d[4]) * la, hg = expf(d[5]) * ha;
  float* o = boxes + 7ll * t;
  o[0] = xg, o[1] = yg, o[2] = zg - hg / 2, o[3] = wg, o[4] = lg, o[5] = hg, o[6] = d[6] + ra;
  int dl = 0;
  if (dir) {
    const long long od = b * st.s[2][0] + h * st.s[2][2] + w * st.s[2][3];
    const float d0 = dir[od + (long long)(a * 2) * st.s[2][1]], d1 = dir[od + (long long)(a * 2 + 1) * st.s[2][1]];
    dl = d1 > d0 ? 1 : 0;   // torch.max: the first of equal logits
  }
  dir_label[t] = dl;
}

__global__ __launch_bounds__(256) void k_center_decode(RpcCenterDecodeCfg c, const float* __restrict__ hm,
                                                       const float* __restrict__ box, const int* __restrict__ topk,
                                                       float* __restrict__ boxes, float* __restrict__ scores,
                                                       int* __restrict__ labels, int* __restrict__ valid) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= c.B * c.ntasks * c.K) return;
  const int k = t % c.K, task = (t / c.K) % c.ntasks, b = t / (c.K * c.ntasks);
  float* o = boxes + 9ll * t;
  int c0 = 0;
  for (int q = 0; q < task; ++q) c0 += c.task_ncls[q];
  const int HW = c.H * c.W;
  const int ncls = c.task_ncls[task];
  if (k >= c.task_k[task]) {
#pragma unroll
    for (int q = 0; q < 9; ++q) o[q] = 0.0f;
    scores[t] = 0.0f, labels[t] = 0, valid[t] = 0;
    return;
  }
  const int idx = min(max(topk[t], 0), ncls * HW - 1);
  const int cls = idx / HW, cell = idx % HW, row = cell / c.W, col = cell % c.W;
  const long long p = (long long)b * HW + cell;
  const float score = 1.0f / (1.0f + expf(-hm[p * c.hm_pitch + c0 + cls]));
  const float* v = box + p * c.box_pitch + 10 * task;   // reg(2) | height(1) | dim(3) | rot(2) | vel(2)
  const float x = ((float)col + v[0]) * (float)c.out_size_factor * c.voxel_x + c.pc_x;
  const float y = ((float)row + v[1]) * (float)c.out_size_factor * c.voxel_y + c.pc_y;
  const float z = v[2];
  o[0] = x, o[1] = y, o[2] = z;
#pragma unroll
  for (int q = 0; q < 3; ++q) o[3 + q] = c.norm_bbox ? expf(v[3 + q]) : v[3 + q];
  o[6] = atan2f(v[6], v[7]);   // rot = (sine, cosine)
  o[7] = v[8], o[8] = v[9];
  bool ok = !c.use_score_threshold || score > c.score_threshold;
  ok = ok && x >= c.limit[0] && y >= c.limit[1] && z >= c.limit[2] && x <= c.limit[3] && y <= c.limit[4] &&
       z <= c.limit[5];
  scores[t] = score, labels[t] = cls, valid[t] = ok ? 1 : 0;
}

static size_t nms_ws(int groups, int max_n) {
  const int T = (max_n + kTile - 1) / kTile;
  return (size_t)groups * (size_t)max_n * (size_t)T * sizeof(unsigned long long);
}

template <bool CIRCLE>
static int nms(const float* boxes, const int* counts, const float* radius, int groups, int max_n, float thr,
               int max_keep, int* keep, int* nkeep, void* workspace, size_t ws_bytes, void* stream) {
  if (groups < 0 || max_n < 0 || max_keep < 0) return RPC_ERR_ARG;
  if (max_n > RPC_NMS_MAX_N) return RPC_ERR_UNSUPPORTED;
  if (groups == 0) return RPC_OK;
  if (!counts || !nkeep || (max_n && !boxes) || (max_keep && !keep) || (CIRCLE && !radius)) return RPC_ERR_ARG;
  if (groups > 65535) return RPC_ERR_ARG;
  if (ws_bytes < nms_ws(groups, max_n) || (nms_ws(groups, max_n) && !workspace)) return RPC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int T = (max_n + kTile - 1) / kTile;
  auto* mask = (unsigned long long*)workspace;
  if (T > 0) {
    hipLaunchKernelGGL(k_nms_mask<CIRCLE>, dim3(T * (T + 1) / 2, groups), dim3(64), 0, st, boxes, counts, radius,
                       max_n, T, thr, mask);
    RPC_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_nms_scan, dim3(groups), dim3(64), 0, st, mask, counts, max_n, T, max_keep, keep, nkeep);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

}  // namespace post
}  // namespace rpc

using namespace rpc::post;

extern "C" {

int rpc_bev_iou_pairs(const float* a, const float* b, int n, float* iou, void* stream) {
  if (n < 0) return RPC_ERR_ARG;
  if (n == 0) return RPC_OK;
  if (!a || !b || !iou) return RPC_ERR_ARG;
  hipLaunchKernelGGL(k_iou_pairs, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, b, n, iou);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

size_t rpc_nms_workspace_size(int groups, int max_n) {
  if (groups <= 0 || max_n <= 0 || max_n > RPC_NMS_MAX_N) return 0;
  return nms_ws(groups, max_n);
}

int rpc_nms_bev(const float* boxes, const int* counts, int groups, int max_n, float thr, int max_keep, int* keep,
                int* nkeep, void* workspace, size_t ws_bytes, void* stream) {
  return nms<false>(boxes, counts, nullptr, groups, max_n, thr, max_keep, keep, nkeep, workspace, ws_bytes, stream);
}

int rpc_nms_circle(const float* xy, const int* counts, const float* radius, int groups, int max_n, int max_keep,
                   int* keep, int* nkeep, void* workspace, size_t ws_bytes, void* stream) {
  return nms<true>(xy, counts, radius, groups, max_n, 0.0f, max_keep, keep, nkeep, workspace, ws_bytes, stream);
}

int rpc_anchor_decode(const int* cand, int batch, int ncand, int H, int W, int S, int R, int C,
                      const float* anchor_tab, const float* cls, const float* reg, const float* dir,
                      const long long* strides, float* scores, float* boxes, int* dir_label, void* stream) {
  if (batch < 0 || ncand < 0 || H <= 0 || W <= 0 || S <= 0 || R <= 0 || C <= 0) return RPC_ERR_ARG;
  if ((long long)H * W * S * R > 0x7fffffffll || (long long)batch * ncand > 0x7fffffffll) return RPC_ERR_ARG;
  if (batch == 0 || ncand == 0) return RPC_OK;
  if (!cand || !anchor_tab || !cls || !reg || !strides || !scores || !boxes || !dir_label) return RPC_ERR_ARG;
  DecodeStrides ds;
  for (int m = 0; m < 3; ++m)
    for (int k = 0; k < 4; ++k) ds.s[m][k] = strides[4 * m + k];
  const int n = batch * ncand;
  hipLaunchKernelGGL(k_anchor_decode, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, cand, batch, ncand, H,
                     W, S, R, C, anchor_tab, cls, reg, dir, ds, scores, boxes, dir_label);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

int rpc_center_decode(const RpcCenterDecodeCfg* cfg, const float* hm, const float* box, const int* topk, float* boxes,
                      float* scores, int* labels, int* valid, void* stream) {
  if (!cfg) return RPC_ERR_ARG;
  const RpcCenterDecodeCfg& c = *cfg;
  if (c.B < 0 || c.H <= 0 || c.W <= 0 || c.K < 0 || c.ntasks <= 0 || c.ntasks > RPC_CENTER_MAX_TASKS)
    return RPC_ERR_ARG;
  int ncls = 0;
  for (int t = 0; t < c.ntasks; ++t) {
    if (c.task_ncls[t] <= 0 || c.task_k[t] < 0 || c.task_k[t] > c.K) return RPC_ERR_ARG;
    if ((long long)c.task_ncls[t] * c.H * c.W > 0x7fffffffll) return RPC_ERR_ARG;
    ncls += c.task_ncls[t];
  }
  if (c.hm_pitch < ncls || c.box_pitch < 10 * c.ntasks) return RPC_ERR_ARG;
  const long long n = (long long)c.B * c.ntasks * c.K;
  if (n > 0x7fffffffll) return RPC_ERR_ARG;
  if (n == 0) return RPC_OK;
  if (!hm || !box || !topk || !boxes || !scores || !labels || !valid) return RPC_ERR_ARG;
  hipLaunchKernelGGL(k_center_decode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c, hm, box,
                     topk, boxes, scores, labels, valid);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}

}  // extern "C"
