// a2/a3/a4: VoxelPerturber forward + backward on gfx950, fused with the valid-point
// compaction / masked scatter of AdversarialVoxelNet.extract_feat and the HardSimpleVFE
// that follows it.
//
// Reference semantics (models/adversarial/voxel_perturber.py):
//   s     = std(x, dim=0, unbiased) + 1e-6 ; NaN/Inf -> 1                 (:158-163)
//   xn    = clamp(x / s, -10, 10)                                         (:165-168)
//   raw   = Tanh(L5(ReLU(BN4(L4(... ReLU(BN0(L0(xn))) ...)))))            (:82-103, :176)
//   raw  *= sigmoid(La1(ReLU(La0(xn))))                                   (:107-112, :203-205)
//   pert  = clamp(raw * bound, -cbound, cbound), nan_to_num               (:209-256, :323-365)
//   out   = x + pert ; l2 = mean ||pert||_2 ; intensity = mean |pert_3| ;
//   bias  = mean_f |mean_n pert| ; imbalance = std_f(std_n pert)          (:268-299)
// BatchNorm1d in train mode uses batch statistics (biased var) and updates the running
// stats with momentum 0.1 and the unbiased var; eval mode uses the running stats.
//
// Structure: this file holds the workspace layout, the C entry points (each reads as its launch
// sequence) and the valid-slot scan; the kernels live in one file per family, each with its
// launchers (declared in perturber_common.h):
//   perturber_point.hip  the boundary layers (F -> C0 forward, output layer + losses, C4 -> F and
//                        layer-0 BatchNorm backward) as per-point passes with no reductions in the
//                        loop, and k_colstats, the column pass that forms their BatchNorm sums;
//   perturber_mfma.hip   the hidden layers on fp32 MFMA tiles (BatchNorm sums in the same launch),
//                        and the hidden layers' weight gradients: k_wgrad_mf (fp32 MFMA), or
//                        k_wgrad_bx3 (split bf16) under cfg->wgrad_split_bf16;
//   perturber_valu.hip   the VALU fallback of the hidden layers for widths 8 and 256, the weight
//                        gradients of every other job (layers 0 and 5, the attention layers, hidden
//                        layers that do not tile) in one launch of k_wgrad_pp, or k_wgrad where a
//                        wide layer's elements exceed it, and k_wgrad_reduce over all jobs.
// Per-channel batch statistics are reduced per wave with shuffles, per block in LDS and across
// blocks by the last-arriving block (agent-scope release/acquire ticket), in a fixed order, so
// results are run-to-run deterministic. Activations z_l are kept in HBM for the backward pass. The
// weight gradients dW = dZ^T H are split-K reductions over KS_MAX point ranges, summed in double in
// a fixed order and passed through the reference's grad hook clamp(nan_to_num(g), -0.1, 0.1).
// Only this file includes hipcub: its scan kernels are instantiated once.
#include <hipcub/hipcub.hpp>
#include <string.h>

#include "perturber_common.h"

namespace rpc {
namespace pert {

// ------------------------------------------------------------------ host side
static inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
// channel stride of the SoA activation buffers: whole 64-point MFMA groups, 16-byte aligned rows
static inline size_t chan_stride(int rows, int slots) {
  size_t n = (size_t)rows * slots;
  return n < 64 ? 64 : (n + 63) & ~(size_t)63;
}

struct Layout {
  size_t off, list, meta, xs, z[5], bn[5], bnsum[5], part, gpart, pstat, ticket, dz[6], dh[2], dsig, da,
      aact, wpart, scan_tmp, scan_bytes, cnt, total;
};

static int widths(const rpc_perturber_cfg* cfg, int C[7]) {
  C[0] = cfg->F;
  C[1] = cfg->hidden[0];
  C[2] = cfg->hidden[1];
  C[3] = cfg->hidden[2];
  C[4] = cfg->hidden[1];
  C[5] = cfg->hidden[0];
  C[6] = cfg->F;
  if (cfg->F < 4 || cfg->F > 5) return RPC_ERR_UNSUPPORTED;
  for (int k = 1; k < 6; ++k)
    if (!hidden_width(C[k])) return RPC_ERR_UNSUPPORTED;
  return RPC_OK;
}

static int make_layout(const rpc_perturber_cfg* cfg, int rows, int slots, Layout* L) {
  int C[7];
  int rc = widths(cfg, C);
  if (rc) return rc;
  size_t Nmax = chan_stride(rows, slots);
  size_t scan_b = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, (const int*)nullptr, (int*)nullptr, rows + 1,
                                       (hipStream_t)0) != hipSuccess)
    return RPC_ERR_HIP;
  int A = cfg->F / 2 > 1 ? cfg->F / 2 : 1;
  size_t welems = 0;
  for (int l = 0; l < 6; ++l) welems += (size_t)C[l + 1] * (C[l] + 1);
  welems += (size_t)A * (cfg->F + 1) + (size_t)(A + 1);
  size_t o = 0;
  L->off = o; o += al(sizeof(int) * (rows + 2));
  L->cnt = o; o += al(sizeof(int) * (rows + 1));
  L->list = o; o += al(sizeof(int) * Nmax);
  L->meta = o; o += al(sizeof(int) * 8);
  L->xs = o; o += al(sizeof(float) * MAXF);
  for (int l = 0; l < 5; ++l) { L->z[l] = o; o += al(sizeof(float) * Nmax * C[l + 1]); }
  for (int l = 0; l < 5; ++l) { L->bn[l] = o; o += al(sizeof(float) * 4 * C[l + 1]); }
  for (int l = 0; l < 5; ++l) { L->bnsum[l] = o; o += al(sizeof(double) * 2 * C[l + 1]); }
  L->part = o; o += al(sizeof(double) * GRID * PSTR);
  L->pstat = o; o += al(sizeof(float) * 4 * MAXF);
  L->ticket = o; o += al(sizeof(unsigned) * NTICKET * TSTRIDE);
  L->gpart = o; o += al(sizeof(double) * NGRP * PSTR);
  for (int l = 0; l < 5; ++l) { L->dz[l] = o; o += al(sizeof(float) * Nmax * C[l + 1]); }
  L->dz[5] = o; o += al(sizeof(float) * Nmax * cfg->F);
  int cmax = 0;
  for (int k = 1; k < 6; ++k) cmax = C[k] > cmax ? C[k] : cmax;
  for (int k = 0; k < 2; ++k) { L->dh[k] = o; o += al(sizeof(float) * Nmax * cmax); }
  L->dsig = o; o += al(sizeof(float) * Nmax);
  L->da = o; o += al(sizeof(float) * Nmax * A);
  L->aact = o; o += al(sizeof(float) * Nmax * A);
  L->wpart = o; o += al(sizeof(float) * KS_MAX * welems);
  L->scan_tmp = o; o += al(scan_b);
  L->scan_bytes = scan_b;
  L->total = o;
  return RPC_OK;
}

static void float_bounds(const rpc_perturber_cfg* cfg, Dev& d) {
  // exact float32 op order of voxel_perturber.py:209-256 and :333-359
  const int F = cfg->F;
  const float e = cfg->sensor_error_bound;
  for (int f = 0; f < MAXF; ++f) d.bscale[f] = d.bclamp[f] = 0.0f;
  if (F == 4) {
    if (!cfg->training) {
      float eb = e;
      volatile float mult = (float)(2.5 * ((2.0 + 1.5 + 1.2) / 3.0));
      eb = eb * mult;
      for (int f = 0; f < 3; ++f) d.bscale[f] = eb * 2.0f;
      d.bscale[3] = 1.5f;
      volatile float fb = e * 5.0f;
      for (int f = 0; f < 3; ++f) d.bclamp[f] = fb * 5.0f;
      d.bclamp[3] = 2.0f;
    } else {
      volatile float eb = e * 0.8f;
      for (int f = 0; f < 3; ++f) d.bscale[f] = eb * 1.3f;
      d.bscale[3] = 0.2f;
      volatile float fb = e * 0.9f;
      for (int f = 0; f < 3; ++f) d.bclamp[f] = fb * 1.2f;
      d.bclamp[3] = 0.1f;
    }
  } else {
    for (int f = 0; f < 4; ++f) d.bscale[f] = d.bclamp[f] = e;
  }
}

static int fill_dev(const rpc_perturber_cfg* cfg, const float* const* P, const float* x, int rows,
                    int slots, const int* npts, void* ws, size_t wsb, Dev& d, Layout& L) {
  int rc = make_layout(cfg, rows, slots, &L);
  if (rc) return rc;
  if (wsb < L.total) return RPC_ERR_WORKSPACE;
  memset(&d, 0, sizeof(d));
  d.F = cfg->F;
  d.A = cfg->F / 2 > 1 ? cfg->F / 2 : 1;
  widths(cfg, d.C);
  // 16-bit rows only where every hidden layer has them, and only with the split-bf16 weight gradient: the
  // fp32-MFMA k_wgrad_mf reads both its z_{l-1} and its dz_l rows as fp32
  d.a16 = cfg->act16 & 3;
  for (int l = 1; l < 5; ++l)
    if (!a16_shape(d.C[l], d.C[l + 1])) d.a16 = 0;
  if (!cfg->wgrad_split_bf16) d.a16 = 0;
  d.dsums = cfg->double_sums != 0;
  d.rows = rows;
  d.slots = slots;
  d.S = (int)chan_stride(rows, slots);
  d.fused = npts != nullptr;
  d.training = cfg->training;
  d.use_att = cfg->use_attention;
  d.vfe_f = cfg->vfe_features;
  d.eps = cfg->bn_eps;
  d.mom = cfg->bn_momentum;
  float_bounds(cfg, d);
  d.x = x;
  d.npts = npts;
  for (int l = 0; l < 5; ++l) {
    d.W[l] = P[6 * l + 0];
    d.b[l] = P[6 * l + 1];
    d.g[l] = P[6 * l + 2];
    d.be[l] = P[6 * l + 3];
    d.rm[l] = (float*)P[6 * l + 4];
    d.rv[l] = (float*)P[6 * l + 5];
  }
  d.W[5] = P[30];
  d.b[5] = P[31];
  d.Wa0 = P[32];
  d.ba0 = P[33];
  d.Wa1 = P[34];
  d.ba1 = P[35];
  char* w = (char*)ws;
  d.off = (int*)(w + L.off);
  d.list = (int*)(w + L.list);
  d.meta = (int*)(w + L.meta);
  d.xs = (float*)(w + L.xs);
  for (int l = 0; l < 5; ++l) {
    d.z[l] = (float*)(w + L.z[l]);
    d.bn[l] = (float*)(w + L.bn[l]);
    d.bnsum[l] = (double*)(w + L.bnsum[l]);
  }
  d.part = (double*)(w + L.part);
  d.gpart = (double*)(w + L.gpart);
  d.pstat = (float*)(w + L.pstat);
  d.ticket = (unsigned*)(w + L.ticket);
  for (int l = 0; l < 6; ++l) d.dz[l] = (float*)(w + L.dz[l]);
  d.dh[0] = (float*)(w + L.dh[0]);
  d.dh[1] = (float*)(w + L.dh[1]);
  d.dsig = (float*)(w + L.dsig);
  d.da = (float*)(w + L.da);
  d.aact = (float*)(w + L.aact);
  d.wpart = (float*)(w + L.wpart);
  return RPC_OK;
}

// hidden layer l on the family that owns its shape
static int launch_mid(int CI, int CO, Dev& d, int l, hipStream_t st, bool bwd, int src = 0) {
  return mid_on_mfma(CI, CO, bwd) ? launch_mid_mfma(CI, CO, d, l, st, bwd, src)
                                  : launch_mid_valu(CI, CO, d, l, st, bwd, src);
}

// ---- weight-gradient job tables of one backward call
struct WgradJobs {
  Jobs J;        // every job in wpart element order: layers 0..5, then the two attention layers
  Jobs JV;       // the jobs of the VALU kernels, with their element-chunk bases
  GradOut G;     // where each job's gradient goes (indexed like J), and each BatchNorm layer's
  MfJobs M[4];   // the MFMA jobs: one table per distinct (shape, z_{l-1} row type)
  int mjobs[4];  // jobs in M[g]
  int mlayer[4]; // first hidden layer of M[g] (its shape and row type are the table's)
  int nm;        // tables in M
};
// the z_{l-1} rows of hidden layer l's weight gradient are fp16 (act16 bit 0: z_1..z_3)
static bool wgrad_z16(const Dev& d, int l) { return (d.a16 & 1) && l - 1 >= 1 && l - 1 <= 3; }

static void make_wgrad_jobs(const Dev& d, float* const* grads, WgradJobs& T) {
  memset(&T, 0, sizeof(T));
  Jobs& J = T.J;
  int nj = 0, eoff = 0;
  auto add = [&](const float* dz, int CO, int CI, int hsrc, const float* h, const float* bn,
                 float* gW, float* gb) {
    Job& j = J.j[nj];
    j.dz = dz; j.CO = CO; j.CI = CI; j.hsrc = hsrc; j.h = h; j.bn = bn;
    j.eoff = eoff; j.nelem = CO * (CI + 1);
    T.G.W[nj] = gW; T.G.b[nj] = gb;
    eoff += j.nelem;
    ++nj;
  };
  for (int l = 0; l < 6; ++l) {
    int CO = d.C[l + 1], CI = d.C[l];
    if (l == 0) add(d.dz[0], CO, CI, H_XN, nullptr, nullptr, grads[0], grads[1]);
    else add(d.dz[l], CO, CI, H_BNRELU, d.z[l - 1], d.bn[l - 1],
             grads[l < 5 ? 6 * l : 30], grads[l < 5 ? 6 * l + 1 : 31]);
  }
  if (d.use_att) {
    add(d.da, d.A, d.F, H_XN, nullptr, nullptr, grads[32], grads[33]);
    add(d.dsig, 1, d.A, H_RAW, d.aact, nullptr, grads[34], grads[35]);
  }
  J.njob = nj;
  J.total = eoff;
  J.KS = KS_MAX;
  for (int l = 0; l < 5; ++l) {
    T.G.gg[l] = grads[6 * l + 2];
    T.G.gb[l] = grads[6 * l + 3];
  }
  // VALU / MFMA partition: hidden layers 1..4 whose (CO, CI) tile go to MFMA, every other job to JV
  bool is_mf[MAXJOB] = {false};
  for (int l = 1; l < 5; ++l) is_mf[l] = wgrad_on_mfma(d.C[l + 1], d.C[l]);
  Jobs& JV = T.JV;
  int nv = 0, chunks = 0;
  for (int k = 0; k < nj; ++k)
    if (!is_mf[k]) JV.j[nv++] = J.j[k];
  JV.njob = nv;
  JV.total = J.total;
  JV.KS = KS_MAX;
  for (int k = 0; k < nv; ++k) {
    JV.cbase[k] = chunks;
    JV.echunks[k] = (JV.j[k].nelem + BLK * EPT - 1) / (BLK * EPT);
    chunks += JV.echunks[k];
  }
  // MFMA jobs grouped by (shape, z_{l-1} row type): one table, and one launch, per distinct kind
  for (int l = 1; l < 5; ++l) {
    if (!is_mf[l]) continue;
    auto same = [&](int k) {
      return is_mf[k] && d.C[k + 1] == d.C[l + 1] && d.C[k] == d.C[l] && wgrad_z16(d, k) == wgrad_z16(d, l);
    };
    bool first = true;
    for (int k = 1; k < l; ++k)
      if (same(k)) first = false;
    if (!first) continue;
    MfJobs& M = T.M[T.nm];
    int n = 0;
    for (int k = l; k < 5; ++k)
      if (same(k)) M.j[n++] = MfJob{d.dz[k], d.z[k - 1], d.bn[k - 1], J.j[k].eoff};
    M.total = J.total;
    M.KS = KS_MAX;
    T.mjobs[T.nm] = n;
    T.mlayer[T.nm] = l;
    ++T.nm;
  }
}

}  // namespace pert
}  // namespace rpc

using namespace rpc;
using namespace rpc::pert;

extern "C" size_t rpc_perturber_workspace_size(const rpc_perturber_cfg* cfg, int rows, int slots) {
  Layout L;
  if (!cfg || make_layout(cfg, rows, slots, &L) != RPC_OK) return 0;
  return L.total;
}

extern "C" int rpc_perturber_forward(const rpc_perturber_cfg* cfg, const float* const* params,
                                     const float* x, int rows, int slots, const int* num_points,
                                     float* out, float* vfe_out, float* losses, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (!cfg || !params || !x || !out || !losses || rows < 1 || slots < 1) return RPC_ERR_ARG;
  if (num_points && (!vfe_out || cfg->vfe_features < 1 || cfg->vfe_features > cfg->F)) return RPC_ERR_ARG;
  if (!num_points && slots != 1) return RPC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Dev d;
  Layout L;
  int rc = fill_dev(cfg, params, x, rows, slots, num_points, workspace, workspace_bytes, d, L);
  if (rc) return rc;
  d.out = out;
  d.vfe = vfe_out;
  d.losses = losses;
  RPC_CHECK(hipMemsetAsync(d.ticket, 0, sizeof(unsigned) * NTICKET * TSTRIDE, st));
  if (d.fused) {
    int* cnt = (int*)((char*)workspace + L.cnt);
    RPC_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * ((size_t)rows + 1), st));
    launch_valid_count(x, rows, slots, cfg->F, cnt, st);
    RPC_LAUNCH_CHECK();
    size_t sb = L.scan_bytes;
    RPC_CHECK(hipcub::DeviceScan::ExclusiveSum((char*)workspace + L.scan_tmp, sb, cnt, d.off, rows + 1, st));
  }
  launch_xstats(d, st);
  RPC_LAUNCH_CHECK();
  if (!cfg->training) {
    launch_bn_eval(d, st);
    RPC_LAUNCH_CHECK();
  }
  rc = launch_first(d, st);
  if (rc) return rc;
  RPC_LAUNCH_CHECK();
  if (cfg->training) {
    rc = launch_colstats(d.C[1], 0, d, 0, nullptr, 1, st);
    if (rc) return rc;
    RPC_LAUNCH_CHECK();
  }
  for (int l = 1; l < 5; ++l) {
    rc = launch_mid(d.C[l], d.C[l + 1], d, l, st, false);
    if (rc) return rc;
    RPC_LAUNCH_CHECK();
  }
  rc = launch_last(d, st, false);
  if (rc) return rc;
  RPC_LAUNCH_CHECK();
  launch_restore(d, st);
  RPC_LAUNCH_CHECK();
  if (d.fused) {
    launch_vfe(d, st);
    RPC_LAUNCH_CHECK();
  }
  return RPC_OK;
}

extern "C" int rpc_perturber_backward(const rpc_perturber_cfg* cfg, const float* const* params,
                                      const float* x, int rows, int slots, const int* num_points,
                                      const float* dout, const float* dlosses, float* const* grads,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!cfg || !params || !x || !dout || !dlosses || !grads || rows < 1 || slots < 1) return RPC_ERR_ARG;
  if (!cfg->training) return RPC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Dev d;
  Layout L;
  int rc = fill_dev(cfg, params, x, rows, slots, num_points, workspace, workspace_bytes, d, L);
  if (rc) return rc;
  d.dout = dout;
  d.dl = dlosses;
  RPC_CHECK(hipMemsetAsync(d.ticket, 0, sizeof(unsigned) * NTICKET * TSTRIDE, st));
  rc = launch_last(d, st, true);
  if (rc) return rc;
  RPC_LAUNCH_CHECK();
  rc = launch_colstats(d.C[5], 1, d, 4, d.dh[0], 7, st);
  if (rc) return rc;
  RPC_LAUNCH_CHECK();
  int src = 0;
  for (int l = 4; l >= 1; --l) {
    rc = launch_mid(d.C[l], d.C[l + 1], d, l, st, true, src);
    if (rc) return rc;
    RPC_LAUNCH_CHECK();
    src ^= 1;
  }
  launch_bwd_first(d, st, src);
  RPC_LAUNCH_CHECK();
  // weight gradients: the VALU jobs in one launch, the MFMA jobs one launch per kind, then the reduce
  WgradJobs T;
  make_wgrad_jobs(d, grads, T);
  launch_wgrad_valu(d, T.JV, st);
  RPC_LAUNCH_CHECK();
  for (int g = 0; g < T.nm; ++g) {
    const int l = T.mlayer[g];
    rc = launch_wgrad_mfma(d.C[l + 1], d.C[l], d, T.M[g], T.mjobs[g], cfg->wgrad_split_bf16 != 0, wgrad_z16(d, l), st);
    if (rc) return rc;
    RPC_LAUNCH_CHECK();
  }
  launch_wgrad_reduce(d, T.J, T.G, st);
  RPC_LAUNCH_CHECK();
  return RPC_OK;
}
