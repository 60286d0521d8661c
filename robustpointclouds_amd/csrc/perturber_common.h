// Shared by the perturber translation units (perturber.hip and perturber_{point,valu,mfma}.hip): the
// launch constants, the kernel argument structs, the device helpers that more than one kernel family
// uses, the host-side routing predicates and the declarations of the per-family launchers.
#pragma once
#include <type_traits>
#include <math.h>

#include "common.h"

namespace rpc {
namespace pert {

// The supported hidden-layer widths, ascending: widths() validates against this list, MAXW is its last
// entry, and for_width is the one place where it becomes a switch over template arguments.
#define RPC_HID(X) X(8) X(16) X(32) X(64) X(128) X(256)
#define RPC_HID_ITEM(w) w,
#define RPC_HID_CASE(w) case w: return f(std::integral_constant<int, w>{});
constexpr int HID[] = {RPC_HID(RPC_HID_ITEM)};
constexpr bool hidden_width(int c) {
  for (int w : HID)
    if (w == c) return true;
  return false;
}
// f(std::integral_constant<int, c>{}) for a supported width c (f returns an rpc status)
template <class Fn>
int for_width(int c, Fn&& f) {
  switch (c) {
    RPC_HID(RPC_HID_CASE)
    default: return RPC_ERR_UNSUPPORTED;
  }
}
#undef RPC_HID_ITEM
#undef RPC_HID_CASE
#undef RPC_HID

constexpr int BLK = 256;
constexpr int NWAVE = BLK / 64;
constexpr int GRID = 256;        // blocks of every per-point VALU pass (= partial rows)
constexpr int MFW = 8;           // waves per block of the MFMA hidden-layer passes: 256 blocks x 8
constexpr int MFBLK = MFW * 64;  // waves = 2 waves per SIMD on 256 CUs (256 VGPRs), GRID partial rows
constexpr int MAXF = 8;
constexpr int MAXC = 128;         // widest layer of the MFMA hidden-layer kernels (their LDS sums)
constexpr int MAXW = HID[sizeof(HID) / sizeof(int) - 1];  // widest hidden layer: above MAXC on the per-point VALU kernels
constexpr int PSTR = 2 * MAXW;    // row stride of the partial-sum rows part / gpart
constexpr int NTICKET = 16;       // hand-off points per pass (each TSTRIDE counters, see grid_col_totals)
constexpr int GS = 16;            // blocks per first-level reduction group
constexpr int NGRP = GRID / GS;   // groups
constexpr int TSTRIDE = 1 + NGRP;
constexpr int KS_MAX = 256;       // point ranges of the weight-gradient passes (= wpart rows)

struct Dev {
  int F, A, C[7];
  int a16;         // effective rpc_perturber_cfg.act16 (0 unless every hidden shape has a 16-bit instantiation)
  int dsums;       // rpc_perturber_cfg.double_sums: batch sums of z and of the perturbation accumulated in double
  int S;           // channel stride of the SoA activation buffers (>= N)
  int rows, slots, fused, training, use_att, vfe_f;
  float eps, mom;
  float bscale[MAXF], bclamp[MAXF];
  const float* x;
  const int* npts;
  const float* W[6];
  const float* b[6];
  const float* g[5];
  const float* be[5];
  float* rm[5];
  float* rv[5];
  const float* Wa0;
  const float* ba0;
  const float* Wa1;
  const float* ba1;
  float* out;
  float* vfe;
  float* losses;
  // workspace
  int* off;        // fused: [rows+1] exclusive scan of valid-slot counts
  int* list;       // fused: [rows*slots] slot index of each valid point
  int* meta;       // [8]: 0 N, 1 fallback flag (NaN / empty)
  float* xs;       // [MAXF] s_f
  float* z[5];     // [C_{l+1}][S] channel-major
  float* bn[5];    // [4*C]: scale (gamma*invstd), beta, mean, invstd
  double* bnsum[5];  // backward: [2*C] sum dy, sum dy*xhat
  double* part;    // [GRID][PSTR]
  double* gpart;   // [NGRP][PSTR] group sums of part
  float* pstat;    // [4*MAXF]: mean_f, s_f, cimb_f, S
  unsigned* ticket;
  float* dz[6];    // dz_0..dz_4 [C_{l+1}][S], dz_5 [F][S]
  float* dh[2];    // [MAXW][S] post-ReLU grads, ping-pong
  float* dsig;     // [S]
  float* da;       // [A][S]
  float* aact;     // [A][S]
  float* wpart;    // [KS][total elements] split-K partial weight grads
  const float* dout;
  const float* dl;  // [4]
};

// ------------------------------------------------------------------ weight-gradient job tables
// job: dW[o][i] = sum_n dz[n][o] * h[n][i] ; i == CI is the bias column (h = 1)
enum HSrc { H_XN = 0, H_BNRELU = 1, H_RAW = 2 };
struct Job {
  const float* dz;  // [CO][S]
  int CO, CI;
  int hsrc;         // HSrc
  const float* h;   // H_BNRELU: z_{l-1} ; H_RAW: activations, both [CI][S]
  const float* bn;  // H_BNRELU: scale, beta, mean of layer l-1
  int eoff;         // element offset in wpart rows
  int nelem;        // CO * (CI + 1)
};
constexpr int MAXJOB = 8;
struct Jobs {
  Job j[MAXJOB];
  int njob;
  int echunks[MAXJOB];  // element chunks per job (k_wgrad: BLK * EPT elements each)
  int cbase[MAXJOB];    // first chunk id of each job
  int KS;               // row splits
  int total;            // total elements over jobs
};
constexpr int EPT = 8;
// a hidden layer's job on the MFMA weight-gradient kernels (k_wgrad_mf / k_wgrad_bx3)
struct MfJob {
  const float* dz;  // [CO][S]
  const float* z;   // z_{l-1} [CI][S]
  const float* bn;  // scale, beta, mean of layer l-1
  int eoff;
};
struct MfJobs {
  MfJob j[4];
  int total, KS;
};
struct GradOut {
  float* W[MAXJOB];
  float* b[MAXJOB];
  float* gg[5];
  float* gb[5];
};

// ------------------------------------------------------------------ routing predicates
// Each decision is stated once: the run-time dispatch in perturber.hip and the `if constexpr` guards of
// the family that owns the kernels evaluate the same function, so a family instantiates exactly the
// shapes that are routed to it.
// Hidden layer l runs on the fp32-MFMA kernels where the tile shape fits (forward: CO % 16, backward:
// CI % 16), on the per-point VALU kernels otherwise (8-channel layers, and layers wider than MAXC).
constexpr bool mid_on_mfma(int CI, int CO, bool bwd) {
  return CI <= MAXC && CO <= MAXC && (bwd ? CI % 16 == 0 : CO % 16 == 0);
}
// 16-bit activation rows (act16) are instantiated for the encoder-decoder shapes of the configs in scope (each
// hidden width twice or half the previous: [64, 128, 64] 3-class, [16, 32, 64] nuScenes); any other hidden shape
// keeps fp32 rows for the whole perturber (fill_dev). Every such shape is mid_on_mfma in both directions.
constexpr bool a16_shape(int CI, int CO) {
  return CI >= 16 && CO >= 16 && CI % 16 == 0 && CO % 16 == 0 && CI * CO <= 8192 && (CI == 2 * CO || CO == 2 * CI);
}
// A hidden layer's weight gradient runs on k_wgrad_mf / k_wgrad_bx3 (at most 32 accumulator tiles), else
// as a job of the VALU kernels.
constexpr bool wgrad_on_mfma(int CO, int CI) {
  return CO % 16 == 0 && CI % 16 == 0 && CO <= MAXC && CI <= MAXC && CO * CI <= 8192;
}

// ------------------------------------------------------------------ device helpers
__device__ __forceinline__ int point_slot(const Dev& d, int i) { return d.fused ? d.list[i] : i; }

// Column totals of the GRID partial rows part[r][0..ncol) (ncol <= PSTR), handed off in two
// levels: the last-arriving block of each group of GS consecutive blocks sums its group's rows in row
// order into gpart[q]; the last group finisher sums gpart[0..NGRP) in group order into lds[0..ncol)
// and returns true (every other block returns false). Each level issues all of its GS resp. NGRP
// loads per column at once: a single block sweeping 256 rows 4 at a time spent ~64 back-to-back
// memory latencies (~40-50 us) at the end of every BatchNorm pass. Fixed groups and fixed order:
// run-to-run deterministic. ticket k owns counters d.ticket[k * TSTRIDE + 0 .. TSTRIDE).
__device__ inline bool grid_col_totals(Dev& d, int k, int ncol, double* lds, int* flag) {
  unsigned* tk = d.ticket + k * TSTRIDE;
  const int q = blockIdx.x / GS;
  if (!last_block_arrive_2d(tk + 1 + q, flag, GS)) return false;
  for (int j = threadIdx.x; j < ncol; j += blockDim.x) {
    double v[GS];
#pragma unroll
    for (int i = 0; i < GS; ++i) v[i] = d.part[(size_t)(q * GS + i) * PSTR + j];
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < GS; ++i) t += v[i];
    d.gpart[(size_t)q * PSTR + j] = t;
  }
  if (!last_block_arrive_2d(tk, flag, NGRP)) return false;
  for (int j = threadIdx.x; j < ncol; j += blockDim.x) {
    double v[NGRP];
#pragma unroll
    for (int i = 0; i < NGRP; ++i) v[i] = d.gpart[(size_t)i * PSTR + j];
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < NGRP; ++i) t += v[i];
    lds[j] = t;
  }
  __syncthreads();
  return true;
}

// finalize a BatchNorm layer from its batch sums (train) — run by the last block
template <int C>
__device__ void bn_finalize(Dev& d, int l, double* lds) {
  const int N = d.meta[0];
  for (int c = threadIdx.x; c < C; c += BLK) {
    double mean = lds[c] / N;
    double var = lds[C + c] / N - mean * mean;
    if (var < 0) var = 0;
    float invstd = 1.0f / sqrtf((float)var + d.eps);
    // applied as (z - mean) * scale + beta (no cancellation)
    float* bn = d.bn[l];
    bn[c] = d.g[l][c] * invstd;
    bn[C + c] = d.be[l][c];
    bn[2 * C + c] = (float)mean;
    bn[3 * C + c] = invstd;
    // N < 2 is the fallback (k_xstats): the reference raises before BatchNorm touches its running stats
    if (N < 2) continue;
    double uvar = var * N / (N - 1);
    d.rm[l][c] = (1.0f - d.mom) * d.rm[l][c] + d.mom * (float)mean;
    d.rv[l][c] = (1.0f - d.mom) * d.rv[l][c] + d.mom * (float)uvar;
  }
}

// hand the backward sums of BatchNorm layer l (sum dy, sum dy*xhat) to the next pass — run by the last block
template <int C>
__device__ void bnb_finalize(Dev& d, int l, double* lds) {
  for (int j = threadIdx.x; j < 2 * C; j += blockDim.x) d.bnsum[l][j] = lds[j];
}

// ------------------------------------------------------------------ per-family launchers
// Plain host functions, each defined next to the kernels it launches; the caller checks the launch.
// Those that return a status give RPC_ERR_UNSUPPORTED for a shape their file does not instantiate.
// perturber_point.hip
void launch_valid_count(const float* x, int rows, int slots, int F, int* cnt, hipStream_t st);
void launch_xstats(Dev& d, hipStream_t st);
void launch_bn_eval(Dev& d, hipStream_t st);
int launch_first(Dev& d, hipStream_t st);
int launch_colstats(int C, int mode, Dev& d, int l, const float* g, int tk, hipStream_t st);
int launch_last(Dev& d, hipStream_t st, bool bwd);
void launch_bwd_first(Dev& d, hipStream_t st, int src);
void launch_restore(Dev& d, hipStream_t st);
void launch_vfe(Dev& d, hipStream_t st);
// perturber_valu.hip / perturber_mfma.hip: hidden layer l on the family mid_on_mfma(CI, CO, bwd) names
int launch_mid_valu(int CI, int CO, Dev& d, int l, hipStream_t st, bool bwd, int src);
int launch_mid_mfma(int CI, int CO, Dev& d, int l, hipStream_t st, bool bwd, int src);
// perturber_valu.hip: the VALU weight-gradient jobs JV (none: no launch), and the reduction of all jobs J
void launch_wgrad_valu(Dev& d, const Jobs& JV, hipStream_t st);
void launch_wgrad_reduce(Dev& d, const Jobs& J, const GradOut& G, hipStream_t st);
// perturber_mfma.hip: njob wgrad_on_mfma(CO, CI) jobs of one shape and row type
int launch_wgrad_mfma(int CO, int CI, Dev& d, const MfJobs& M, int njob, bool split, bool zh16, hipStream_t st);

}  // namespace pert
}  // namespace rpc
