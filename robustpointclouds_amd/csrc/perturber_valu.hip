// VoxelPerturber, VALU kernels (see perturber.hip for the structure): the hidden layers that do not
// fit the MFMA tiles (mid_on_mfma false: 8-channel layers and layers wider than MAXC), fully unrolled
// per point, and the weight gradients of every job that is not on MFMA, with the reduction of all jobs.
// k_fwd_mid and k_bwd_mid stay in one translation unit: compiled apart, three of their instantiations
// come out with reordered address arithmetic, and k_bwd_mid alone compiles no faster than this file.
#include "perturber_common.h"

namespace rpc {
namespace pert {

// per-lane double accumulators for per-channel sums; channel c lives in lane c&63, slot c>>6
template <int C>
struct ChanAcc {
  static constexpr int K = (C + 63) / 64;
  double s[2][K];
  __device__ void zero() {
#pragma unroll
    for (int k = 0; k < K; ++k) s[0][k] = s[1][k] = 0.0;
  }
  // wave-reduce this thread's (v, w) for channel c; lane c&63 keeps the running sums.
  // c must be a compile-time constant after unrolling (static register index).
  __device__ __forceinline__ void add1(int c, float v, float w) {
    const int lane = threadIdx.x & 63;
    float a = wave_sum(v);
    float q = wave_sum(w);
    if (lane == (c & 63)) {
      s[0][c >> 6] += (double)a;
      s[1][c >> 6] += (double)q;
    }
  }
  // block-combine into part[blockIdx.x][0..2C)
  __device__ void flush(double* part, double* lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      int c = k * 64 + lane;
      if (c < C) {
        lds[(w * 2 + 0) * MAXW + c] = s[0][k];
        lds[(w * 2 + 1) * MAXW + c] = s[1][k];
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < 2 * C; j += BLK) {
      int which = j / C, c = j - which * C;
      double t = 0.0;
      for (int ww = 0; ww < NWAVE; ++ww) t += lds[(ww * 2 + which) * MAXW + c];
      part[(size_t)blockIdx.x * PSTR + j] = t;
    }
  }
};
// VALU hidden layers whose weights exceed 64 KB read them from global memory (wave-uniform loads)
__host__ __device__ constexpr bool wide_w(int CI, int CO) { return CI * CO > 16384; }

// layer l (1..4): relu(bn_{l-1}(z_{l-1})) -> z_l
template <int CI, int CO>
__global__ __launch_bounds__(BLK) void k_fwd_mid(Dev d, int l) {
  constexpr int WN = wide_w(CI, CO) ? 0 : CO * CI;  // weights staged in LDS (else read from global)
  __shared__ float sW[WN + CO + 3 * CI];
  __shared__ double lds[NWAVE * 2 * MAXW];
  __shared__ int lastf;
  for (int j = threadIdx.x; j < WN; j += BLK) sW[j] = d.W[l][j];
  for (int j = threadIdx.x; j < CO; j += BLK) sW[WN + j] = d.b[l][j];
  for (int j = threadIdx.x; j < 3 * CI; j += BLK) sW[WN + CO + j] = d.bn[l - 1][j];
  __syncthreads();
  const float* Wl = WN ? sW : d.W[l];
  const float* sc = sW + WN + CO;
  const float* sh = sc + CI;
  const float* mu = sh + CI;
  const int N = d.meta[0];
  ChanAcc<CO> acc;
  acc.zero();
  for (int t = blockIdx.x; t * BLK < N; t += GRID) {
    int i = t * BLK + threadIdx.x;
    bool act = i < N;
    float h[CI];
    const float* zi = d.z[l - 1] + (act ? i : 0);
#pragma unroll
    for (int c = 0; c < CI; ++c)
      h[c] = act ? fmaxf(fmaf(zi[(size_t)c * d.S] - mu[c], sc[c], sh[c]), 0.0f) : 0.0f;
#pragma unroll
    for (int o = 0; o < CO; ++o) {
      float a = sW[WN + o];
#pragma unroll
      for (int c = 0; c < CI; ++c) a = fmaf(Wl[o * CI + c], h[c], a);
      float z = act ? a : 0.0f;
      if (act) d.z[l][(size_t)o * d.S + i] = z;
      if (d.training) acc.add1(o, z, z * z);
    }
  }
  if (!d.training) return;
  acc.flush(d.part, lds);
  if (!grid_col_totals(d, 1 + l, 2 * CO, lds, &lastf)) return;
  bn_finalize<CO>(d, l, lds);
}

// BN layer l backward (l = 4..1): dz_l from dh_l'; dh_{l-1}' = relu'(.) * W_l^T dz_l
template <int CI, int CO>
__global__ __launch_bounds__(BLK) void k_bwd_mid(Dev d, int l, int src) {
  constexpr int WN = wide_w(CI, CO) ? 0 : CO * CI;  // weights staged in LDS (else read from global)
  __shared__ float sW[WN + 7 * CO + 4 * CI];
  __shared__ double lds[NWAVE * 2 * MAXW];
  __shared__ int lastf;
  const int N = d.meta[0];
  const double invN = 1.0 / N;
  for (int j = threadIdx.x; j < WN; j += BLK) sW[j] = d.W[l][j];
  for (int j = threadIdx.x; j < 4 * CO; j += BLK) sW[WN + j] = d.bn[l][j];
  for (int j = threadIdx.x; j < 4 * CI; j += BLK) sW[WN + 4 * CO + j] = d.bn[l - 1][j];
  for (int j = threadIdx.x; j < CO; j += BLK) {
    float* m = sW + WN + 4 * CO + 4 * CI;
    m[j] = (float)(d.bnsum[l][j] * invN);
    m[CO + j] = (float)(d.bnsum[l][CO + j] * invN);
    m[2 * CO + j] = d.g[l][j] * d.bn[l][3 * CO + j];
  }
  __syncthreads();
  const float* Wl = WN ? sW : d.W[l];
  const float* bo = sW + WN;           // scale, beta, mean, invstd of layer l
  const float* bi = bo + 4 * CO;       // of layer l-1
  const float* m1 = bi + 4 * CI;
  const float* m2 = m1 + CO;
  const float* gi = m2 + CO;
  ChanAcc<CI> acc;
  acc.zero();
  for (int t = blockIdx.x; t * BLK < N; t += GRID) {
    int i = t * BLK + threadIdx.x;
    bool act = i < N;
    int ii = act ? i : 0;
    const float* dhi = d.dh[src] + ii;
    const float* zl = d.z[l] + ii;
    float dz[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) {
      float xh = (zl[(size_t)o * d.S] - bo[2 * CO + o]) * bo[3 * CO + o];
      dz[o] = act ? gi[o] * (dhi[(size_t)o * d.S] - m1[o] - xh * m2[o]) : 0.0f;
      if (act) d.dz[l][(size_t)o * d.S + i] = dz[o];
    }
    const float* zp = d.z[l - 1] + ii;
#pragma unroll
    for (int c = 0; c < CI; ++c) {
      float s = 0.0f;
#pragma unroll
      for (int o = 0; o < CO; ++o) s = fmaf(Wl[o * CI + c], dz[o], s);
      float zc = zp[(size_t)c * d.S];
      float hv = fmaxf(fmaf(zc - bi[2 * CI + c], bi[c], bi[CI + c]), 0.0f);
      s = (act && hv > 0.0f) ? s : 0.0f;
      if (act) d.dh[src ^ 1][(size_t)c * d.S + i] = s;
      acc.add1(c, s, s * ((zc - bi[2 * CI + c]) * bi[3 * CI + c]));
    }
  }
  acc.flush(d.part, lds);
  if (!grid_col_totals(d, 7 + (5 - l), 2 * CI, lds, &lastf)) return;
  bnb_finalize<CI>(d, l - 1, lds);
}

// ------------------------------------------------------------------ weight gradients
// (Job / Jobs: perturber_common.h)
constexpr int TR = 64;

// LDS rows are [r][CO + 1] dz and [r][CI + 2] h values; the row tile tr shrinks so that layers up to MAXW
// channels wide fit the same 66 KB as the 64-row tile of MAXC-wide ones.
constexpr int WG_LDS = 2 * TR * (MAXC + 1);
template <int F>
__global__ __launch_bounds__(BLK) void k_wgrad(Dev d, Jobs J) {
  __shared__ float sbuf[WG_LDS];
  int chunk = blockIdx.x / J.KS, ks = blockIdx.x - chunk * J.KS;
  int jb = 0;
  while (jb + 1 < J.njob && chunk >= J.cbase[jb + 1]) ++jb;
  const Job& job = J.j[jb];
  const int e0 = (chunk - J.cbase[jb]) * BLK * EPT;
  const int CO = job.CO, CI = job.CI, CI1 = CI + 1;
  const int SZ = CO + 1, SH = CI1 + 1;
  const int tr = min(TR, WG_LDS / (SZ + SH));
  float* sdz = sbuf;
  float* shh = sbuf + tr * SZ;
  const int N = d.meta[0];
  const int rows_per = (N + J.KS - 1) / J.KS;
  const int r0 = ks * rows_per, r1 = min(N, r0 + rows_per);
  float acc[EPT];
  int eo[EPT], ei[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    acc[k] = 0.0f;
    int e = e0 + k * BLK + threadIdx.x;
    eo[k] = e < job.nelem ? e / CI1 : -1;
    ei[k] = e < job.nelem ? e - (e / CI1) * CI1 : 0;
  }
  for (int rb = r0; rb < r1; rb += tr) {
    int nr = min(tr, r1 - rb);
    __syncthreads();
    for (int q = threadIdx.x; q < tr * CO; q += BLK) {
      int o = q / tr, r = q - o * tr;
      sdz[r * SZ + o] = r < nr ? job.dz[(size_t)o * d.S + rb + r] : 0.0f;
    }
    for (int q = threadIdx.x; q < tr * CI1; q += BLK) {
      int c = q / tr, r = q - c * tr;
      float v = 0.0f;
      if (r < nr) {
        int n = rb + r;
        if (c == CI) v = 1.0f;
        else if (job.hsrc == H_XN) {
          int slot = point_slot(d, n);
          float t = d.x[(size_t)slot * F + c] / d.xs[c];
          v = fminf(fmaxf(t, -10.0f), 10.0f);
        } else if (job.hsrc == H_BNRELU) {
          v = fmaxf(fmaf(job.h[(size_t)c * d.S + n] - job.bn[2 * CI + c], job.bn[c], job.bn[CI + c]), 0.0f);
        } else {
          v = job.h[(size_t)c * d.S + n];
        }
      }
      shh[r * SH + c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if (eo[k] < 0) continue;
      float a = acc[k];
      const float* pz = sdz + eo[k];
      const float* ph = shh + ei[k];
      for (int r = 0; r < tr; ++r) a = fmaf(pz[r * SZ], ph[r * SH], a);
      acc[k] = a;
    }
  }
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    int e = e0 + k * BLK + threadIdx.x;
    if (e < job.nelem) d.wpart[(size_t)ks * J.total + job.eoff + e] = acc[k];
  }
}

// All VALU weight-gradient jobs of one point range per block (grid = KS ranges): per 64-point tile
// every job's dz rows and h rows are staged channel-major in LDS (dynamic: the host sizes it), then
// each thread accumulates up to EPT (job, o, i) elements in fixed row order. The staging is one flat
// sweep over a per-block table of source rows (raw / BatchNorm+ReLU / normalised-x gather), double
// buffered: the next tile's loads are in flight while the current one is summed.
// (One block grid per job — 4 jobs x 256 ranges of 7 serial tiles — took 97 us.)
// 1024 threads (16 waves per CU keep the staging loads in flight); WPRE float4 per thread: nrow * TR / 4 <= 12288.
// TR = points per tile, the largest of 256 / 128 / 64 whose two tile buffers fit the LDS (host): a block's range is
// a chain of tiles (fetch one ahead, two barriers per tile), so fewer, larger tiles shorten it (r06: 64-point tiles
// made nuScenes' 10-sweep batch ~60 tiles per block)
constexpr int WPB = 1024, WPRE = 12, WEPT = 2;
struct RowSrc {
  const float* p;   // channel row base ([S] floats); XN: nullptr
  float mu, sc, be; // BNRELU: relu((v - mu) * sc + be)
  int kind;         // HSrc, or 3 = dz row (raw)
  int c;            // XN: feature index
};
template <int F, int TRP>
__global__ __launch_bounds__(WPB) void k_wgrad_pp(Dev d, Jobs J, int nrow) {
  constexpr int TPP = TRP + 1;
  extern __shared__ float sbuf[];
  RowSrc* rows = (RowSrc*)(sbuf + 2 * ((nrow * TPP + 3) & ~3));
  const int N = d.meta[0];
  const int rows_per = ((N + J.KS - 1) / J.KS + TRP - 1) / TRP * TRP;
  const int r0 = blockIdx.x * rows_per, r1 = min(N, r0 + rows_per);
  int joff[MAXJOB + 1];
  joff[0] = 0;
  for (int k = 0; k < J.njob; ++k) joff[k + 1] = joff[k] + J.j[k].CO + J.j[k].CI;
  // source table: job k's dz rows at joff[k] .., then its h rows
  for (int k = 0; k < J.njob; ++k) {
    const Job& job = J.j[k];
    for (int q = threadIdx.x; q < job.CO + job.CI; q += WPB) {
      RowSrc rs{};
      if (q < job.CO) {
        rs.p = job.dz + (size_t)q * d.S;
        rs.kind = 3;
      } else {
        const int c = q - job.CO;
        rs.kind = job.hsrc;
        rs.c = c;
        if (job.hsrc != H_XN) rs.p = job.h + (size_t)c * d.S;
        if (job.hsrc == H_BNRELU) {
          rs.mu = job.bn[2 * job.CI + c];
          rs.sc = job.bn[c];
          rs.be = job.bn[job.CI + c];
        }
      }
      rows[joff[k] + q] = rs;
    }
  }
  // this thread's elements
  int ej[WEPT];
  int pz[WEPT], ph[WEPT];
  float acc[WEPT];
  int nE = 0;
  for (int k = 0; k < J.njob; ++k) nE += J.j[k].nelem;
#pragma unroll
  for (int k = 0; k < WEPT; ++k) {
    acc[k] = 0.0f;
    ej[k] = -1;
    pz[k] = ph[k] = -1;
    int e = threadIdx.x + k * WPB;
    if (e < nE) {
      int jb = 0;
      while (e >= J.j[jb].nelem) { e -= J.j[jb].nelem; ++jb; }
      const int CI1 = J.j[jb].CI + 1, o = e / CI1, ii = e - o * CI1;
      ej[k] = J.j[jb].eoff + e;
      pz[k] = (joff[jb] + o) * TPP;
      ph[k] = ii < J.j[jb].CI ? (joff[jb] + J.j[jb].CO + ii) * TPP : -1;
    }
  }
  __syncthreads();
  // staging sweep: float4 of 4 consecutive points per lane (rows_per is a multiple of 64, so every
  // tile starts 16-byte aligned); tile t + 1 is fetched into registers while tile t is summed
  const int nq = nrow * (TRP / 4);
  float4 pre[WPRE];
  auto fetch = [&](int rb) {
#pragma unroll
    for (int u = 0; u < WPRE; ++u) {
      const int q = threadIdx.x + u * WPB;
      float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (q < nq) {
        const int row = q / (TRP / 4), n0 = rb + (q - row * (TRP / 4)) * 4;
        const RowSrc rs = rows[row];
        if (rs.kind == H_XN) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (n0 + j < r1) {
              const float t = d.x[(size_t)point_slot(d, n0 + j) * F + rs.c] / d.xs[rs.c];
              v[j] = fminf(fmaxf(t, -10.0f), 10.0f);
            }
        } else if (n0 < r1) {
          const float4 x = *(const float4*)(rs.p + n0);
          v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (rs.kind == H_BNRELU) v[j] = fmaxf(fmaf(v[j] - rs.mu, rs.sc, rs.be), 0.0f);
            if (n0 + j >= r1) v[j] = 0.0f;
          }
        }
      }
      pre[u] = make_float4(v[0], v[1], v[2], v[3]);
    }
  };
  const int tsz = (nrow * TPP + 3) & ~3;
  int cur = 0;
  if (r0 < r1) fetch(r0);
  for (int rb = r0; rb < r1; rb += TRP) {
    float* buf = sbuf + cur * tsz;
#pragma unroll
    for (int u = 0; u < WPRE; ++u) {
      const int q = threadIdx.x + u * WPB;
      if (q < nq) {
        const int row = q / (TRP / 4), r4 = (q - row * (TRP / 4)) * 4;
        float* dst = buf + row * TPP + r4;
        dst[0] = pre[u].x;
        dst[1] = pre[u].y;
        dst[2] = pre[u].z;
        dst[3] = pre[u].w;
      }
    }
    __syncthreads();
    if (rb + TRP < r1) fetch(rb + TRP);
#pragma unroll
    for (int k = 0; k < WEPT; ++k) {
      if (ej[k] < 0) continue;
      float a = acc[k];
      const float* z = buf + pz[k];
      if (ph[k] >= 0) {
        const float* hh = buf + ph[k];
        for (int r = 0; r < TRP; ++r) a = fmaf(z[r], hh[r], a);
      } else {
        for (int r = 0; r < TRP; ++r) a += z[r];
      }
      acc[k] = a;
    }
    cur ^= 1;
  }
#pragma unroll
  for (int k = 0; k < WEPT; ++k)
    if (ej[k] >= 0) d.wpart[(size_t)blockIdx.x * J.total + ej[k]] = acc[k];
}

__device__ __forceinline__ float grad_hook(float g) {
  // clamp(nan_to_num(g, nan=0, posinf=0, neginf=0), -0.1, 0.1)  (voxel_perturber.py:465-470)
  if (isnan(g) || isinf(g)) g = 0.0f;
  return fminf(fmaxf(g, -0.1f), 0.1f);
}

// Fixed-order reduction of the KS partial rows + the reference's grad hook. Block = 64 elements x 4
// row quarters (each quarter 8 interleaved sums, 8 loads in flight), quarters combined in order through
// LDS; elements past J.total are the BatchNorm affine gradients (no rows).
__global__ __launch_bounds__(BLK) void k_wgrad_reduce(Dev d, Jobs J, GradOut G) {
  __shared__ double sq[4][64];
  const int el = threadIdx.x & 63, qt = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;
  const int flag = d.meta[1];
  if (e < J.total) {
    const int k0 = qt * J.KS / 4, k1 = (qt + 1) * J.KS / 4;
    double q[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int k = k0;
    for (; k + 8 <= k1; k += 8)
#pragma unroll
      for (int u = 0; u < 8; ++u) q[u] += d.wpart[(size_t)(k + u) * J.total + e];
    for (; k < k1; ++k) q[0] += d.wpart[(size_t)k * J.total + e];
    sq[qt][el] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
  }
  __syncthreads();
  if (qt != 0) return;
  if (e < J.total) {
    int jb = 0;
    while (jb + 1 < J.njob && e >= J.j[jb + 1].eoff) ++jb;
    const Job& job = J.j[jb];
    const int le = e - job.eoff;
    const double s = (sq[0][el] + sq[1][el]) + (sq[2][el] + sq[3][el]);
    const float g = flag ? 0.0f : grad_hook((float)s);
    const int CI1 = job.CI + 1, o = le / CI1, i = le - o * CI1;
    if (i < job.CI) { if (G.W[jb]) G.W[jb][o * job.CI + i] = g; }
    else if (G.b[jb]) G.b[jb][o] = g;
  }
  // BatchNorm gamma / beta: sum dy*xhat, sum dy
  const int t = e - J.total;
  if (t >= 0) {
    int l = 0, base = 0;
    while (l < 5 && t >= base + d.C[l + 1]) { base += d.C[l + 1]; ++l; }
    if (l < 5) {
      const int c = t - base, C = d.C[l + 1];
      const float gg = flag ? 0.0f : grad_hook((float)d.bnsum[l][C + c]);
      const float gb = flag ? 0.0f : grad_hook((float)d.bnsum[l][c]);
      if (G.gg[l]) G.gg[l][c] = gg;
      if (G.gb[l]) G.gb[l][c] = gb;
    }
  }
}

// ------------------------------------------------------------------ launchers
template <int CI, int CO>
static int launch_mid_t(Dev& d, int l, hipStream_t st, bool bwd, int src) {
  if (bwd) {
    if constexpr (!mid_on_mfma(CI, CO, true)) {
      hipLaunchKernelGGL((k_bwd_mid<CI, CO>), dim3(GRID), dim3(BLK), 0, st, d, l, src);
      return RPC_OK;
    }
  } else {
    if constexpr (!mid_on_mfma(CI, CO, false)) {
      hipLaunchKernelGGL((k_fwd_mid<CI, CO>), dim3(GRID), dim3(BLK), 0, st, d, l);
      return RPC_OK;
    }
  }
  return RPC_ERR_UNSUPPORTED;  // an MFMA shape: not instantiated here
}
int launch_mid_valu(int CI, int CO, Dev& d, int l, hipStream_t st, bool bwd, int src) {
  return for_width(CI, [&](auto ci) {
    return for_width(CO, [&](auto co) { return launch_mid_t<ci.value, co.value>(d, l, st, bwd, src); });
  });
}

void launch_wgrad_valu(Dev& d, const Jobs& JV, hipStream_t st) {
  if (!JV.njob) return;
  const int F = d.F, ks = JV.KS;
  // one launch over KS point ranges covering every VALU job (LDS sized to the jobs' tile rows)
  int nrow = 0, nel = 0;
  for (int k = 0; k < JV.njob; ++k) { nrow += JV.j[k].CO + JV.j[k].CI; nel += JV.j[k].nelem; }
  auto lds_of = [&](int tr) {
    return (size_t)2 * ((nrow * (tr + 1) + 3) & ~3) * sizeof(float) + (size_t)nrow * sizeof(RowSrc);
  };
  int tr = 0;
  for (int t = 256; t >= 64 && !tr; t >>= 1)
    if (lds_of(t) <= 160 * 1024 && nrow * (t / 4) <= WPB * WPRE) tr = t;
  if (nel > WPB * WEPT || !tr) {
    // wide VALU hidden layers (CO * CI > 8192): the per-job chunked kernel
    const int chunks = JV.cbase[JV.njob - 1] + JV.echunks[JV.njob - 1];
    if (F == 4) hipLaunchKernelGGL((k_wgrad<4>), dim3(chunks * ks), dim3(BLK), 0, st, d, JV);
    else hipLaunchKernelGGL((k_wgrad<5>), dim3(chunks * ks), dim3(BLK), 0, st, d, JV);
  } else {
    const size_t lds = lds_of(tr);
#define WPP_CASE(FF, TT)                                                                                      \
  if (F == FF && tr == TT) {                                                                                  \
    if (lds > 64 * 1024)                                                                                      \
      (void)hipFuncSetAttribute((const void*)k_wgrad_pp<FF, TT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL((k_wgrad_pp<FF, TT>), dim3(ks), dim3(WPB), lds, st, d, JV, nrow);                     \
  }
    WPP_CASE(4, 256) WPP_CASE(4, 128) WPP_CASE(4, 64) WPP_CASE(5, 256) WPP_CASE(5, 128) WPP_CASE(5, 64)
#undef WPP_CASE
  }
}

void launch_wgrad_reduce(Dev& d, const Jobs& J, const GradOut& G, hipStream_t st) {
  int nbn = d.C[1] + d.C[2] + d.C[3] + d.C[4] + d.C[5];
  int nr = (J.total + nbn + 63) / 64;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3(nr), dim3(BLK), 0, st, d, J, G);
}

}  // namespace pert
}  // namespace rpc
