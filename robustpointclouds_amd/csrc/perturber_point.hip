// VoxelPerturber, per-point and boundary passes (see perturber.hip for the structure): valid-slot
// counts, input statistics, the F -> C0 / C4 -> F boundary layers with the losses and the attention
// gate, the BatchNorm column sums of those layers, the fallback restore and the fused VFE mean.
#include "perturber_common.h"

namespace rpc {
namespace pert {

// ------------------------------------------------------------------ forward kernels
// stats of x over the valid points + compaction list + copy of the voxel slots to out
template <int F>
__global__ __launch_bounds__(BLK) void k_xstats(Dev d) {
  __shared__ double lds[NWAVE * 2 * MAXC];
  __shared__ int lastf;
  double s1[F], s2[F];
#pragma unroll
  for (int f = 0; f < F; ++f) s1[f] = s2[f] = 0.0;
  int nan = 0;
  const int stride = GRID * BLK;
  for (int r = blockIdx.x * BLK + threadIdx.x; r < d.rows; r += stride) {
    if (d.fused) {
      int base = d.off[r], j = 0;
      // eight slots' loads in flight before their copies are stored (d.out may alias d.x as far as the
      // compiler knows: interleaved, every slot's loads waited behind the previous slot's stores)
      for (int s0 = 0; s0 < d.slots; s0 += 8) {
        float vv[8][F];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const size_t slot = (size_t)r * d.slots + s0 + u;
#pragma unroll
          for (int f = 0; f < F; ++f) vv[u][f] = s0 + u < d.slots ? d.x[slot * F + f] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (s0 + u >= d.slots) break;
          const size_t slot = (size_t)r * d.slots + s0 + u;
          float sum = 0.0f;
#pragma unroll
          for (int f = 0; f < F; ++f) {
            sum = f == 0 ? vv[u][0] : sum + vv[u][f];
            d.out[slot * F + f] = vv[u][f];
          }
          if (sum != 0.0f) {
            d.list[base + j++] = (int)slot;
#pragma unroll
            for (int f = 0; f < F; ++f) {
              s1[f] += vv[u][f];
              s2[f] += (double)vv[u][f] * vv[u][f];
              nan |= isnan(vv[u][f]);
            }
          }
        }
      }
    } else {
      const float* p = d.x + (size_t)r * F;
#pragma unroll
      for (int f = 0; f < F; ++f) {
        float v = p[f];
        s1[f] += v;
        s2[f] += (double)v * v;
        nan |= isnan(v);
      }
    }
  }
  // block reduce 2F doubles + nan flag
#pragma unroll
  for (int f = 0; f < F; ++f) {
    s1[f] = wave_sum(s1[f]);
    s2[f] = wave_sum(s2[f]);
  }
  nan = __any(nan);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < F; ++f) {
      lds[w * 2 * MAXC + f] = s1[f];
      lds[w * 2 * MAXC + F + f] = s2[f];
    }
    lds[w * 2 * MAXC + 2 * F] = nan;
  }
  __syncthreads();
  if (threadIdx.x < 2 * F + 1) {
    double t = 0.0;
    for (int ww = 0; ww < NWAVE; ++ww) t += lds[ww * 2 * MAXC + threadIdx.x];
    d.part[(size_t)blockIdx.x * PSTR + threadIdx.x] = t;
  }
  if (!grid_col_totals(d, 0, 2 * F + 1, lds, &lastf)) return;
  if (threadIdx.x == 0) {
    int N = d.fused ? d.off[d.rows] : d.rows;
    d.meta[0] = N;
    // fewer than two points in train mode: the reference's BatchNorm1d raises on one sample and the detector
    // falls back to the unperturbed voxels with zero losses (adversarial_voxelnet.py:123-132)
    int flag = (lds[2 * F] != 0.0) || N == 0 || (d.training && N < 2);
    d.meta[1] = flag;
    // s = std(x, unbiased) + 1e-6; any NaN/Inf entry resets the whole vector (:158-163)
    int bad = 0;
    for (int f = 0; f < F; ++f) {
      double mean = lds[f] / N;
      double var = N > 1 ? (lds[F + f] - N * mean * mean) / (N - 1) : NAN;
      if (var < 0) var = 0;
      float s = sqrtf((float)var) + 1e-6f;
      bad |= (isnan(s) || isinf(s));
      d.xs[f] = s;
    }
    if (bad)
      for (int f = 0; f < F; ++f) d.xs[f] = 1.0f;
  }
}

template <int F>
__device__ __forceinline__ void load_xn(const Dev& d, int slot, float (&xv)[F], float (&xn)[F]) {
  const float* p = d.x + (size_t)slot * F;
#pragma unroll
  for (int f = 0; f < F; ++f) {
    xv[f] = p[f];
    float t = xv[f] / d.xs[f];
    xn[f] = fminf(fmaxf(t, -10.0f), 10.0f);
  }
}

// recompute the attention gate for one point
template <int F>
__device__ __forceinline__ float attention(const Dev& d, const float (&xn)[F], float (&a)[MAXF]) {
  const int A = d.A;
  float t = d.ba1[0];
  for (int j = 0; j < A; ++j) {
    float s = d.ba0[j];
#pragma unroll
    for (int f = 0; f < F; ++f) s = fmaf(d.Wa0[j * F + f], xn[f], s);
    a[j] = fmaxf(s, 0.0f);
    t = fmaf(d.Wa1[j], a[j], t);
  }
  return 1.0f / (1.0f + expf(-t));
}

// output layer: relu(bn4(z4)) -> tanh -> *att -> bounds -> clamp -> out, loss sums
template <int CI, int F, bool EX>
__global__ __launch_bounds__(BLK) void k_fwd_last(Dev d) {
  __shared__ float sW[F * CI + F + 3 * CI];
  __shared__ double lds[NWAVE * 2 * MAXC];
  __shared__ int lastf;
  for (int j = threadIdx.x; j < F * CI; j += BLK) sW[j] = d.W[5][j];
  for (int j = threadIdx.x; j < F; j += BLK) sW[F * CI + j] = d.b[5][j];
  for (int j = threadIdx.x; j < 3 * CI; j += BLK) sW[F * CI + F + j] = d.bn[4][j];
  __syncthreads();
  const float* sc = sW + F * CI + F;
  const float* sh = sc + CI;
  const float* mu = sh + CI;
  const int N = d.meta[0];
  // sums: [0] sum ||pert||, [1] sum |pert_3|, [2..2+F) sum pert_f, [2+F..2+2F) sum pert_f^2, [2+2F] nan
  constexpr int NS = 3 + 2 * F;
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  for (int t = blockIdx.x; t * BLK < N; t += GRID) {
    int i = t * BLK + threadIdx.x;
    bool act = i < N;
    float v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = 0.0f;
    // EX (rpc_perturber_cfg.double_sums): sum pert_f and sum pert_f^2 in double (the square of a float is
    // exact there, the running sums round at 2^-53). Their difference is the variance, and a feature whose points all sit on the clamp has variance
    // 0: float sums leave a std of ~3e-4 |pert| there, and the imbalance loss and its gradient with it
    double pd[EX ? 2 * F : 1];
#pragma unroll
    for (int k = 0; k < (EX ? 2 * F : 1); ++k) pd[k] = 0.0;
    if (act) {
      int slot = point_slot(d, i);
      float xv[F], xn[F], h[CI];
      load_xn<F>(d, slot, xv, xn);
      const float* zi = d.z[4] + i;
#pragma unroll
      for (int c = 0; c < CI; ++c) h[c] = fmaxf(fmaf(zi[(size_t)c * d.S] - mu[c], sc[c], sh[c]), 0.0f);
      float am[MAXF];
      float att = d.use_att ? attention<F>(d, xn, am) : 1.0f;
      float nrm2 = 0.0f;
      int bad = 0;
#pragma unroll
      for (int f = 0; f < F; ++f) {
        float u = sW[F * CI + f];
#pragma unroll
        for (int c = 0; c < CI; ++c) u = fmaf(sW[f * CI + c], h[c], u);
        float raw = tanhf(u);
        float pp = (raw * att) * d.bscale[f];
        bad |= isnan(pp);
        float p = fminf(fmaxf(pp, -d.bclamp[f]), d.bclamp[f]);
        d.out[(size_t)slot * F + f] = xv[f] + p;
        nrm2 = fmaf(p, p, nrm2);
        if constexpr (EX) {
          pd[f] = (double)p;
          pd[F + f] = (double)p * (double)p;
        } else {
          v[2 + f] = p;
          v[2 + F + f] = p * p;
        }
        if (f == 3) v[1] = fabsf(p);
      }
      v[0] = sqrtf(nrm2);
      v[2 + 2 * F] = (float)bad;
    }
#pragma unroll
    for (int k = 0; k < NS; ++k)
      if (!EX || k < 2 || k >= 2 + 2 * F) acc[k] += (double)wave_sum(v[k]);
    if constexpr (EX)
#pragma unroll
      for (int k = 0; k < 2 * F; ++k) acc[2 + k] += wave_sum(pd[k]);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NS; ++k) lds[w * 2 * MAXC + k] = acc[k];
  __syncthreads();
  if (threadIdx.x < NS) {
    double t = 0.0;
    for (int ww = 0; ww < NWAVE; ++ww) t += lds[ww * 2 * MAXC + threadIdx.x];
    d.part[(size_t)blockIdx.x * PSTR + threadIdx.x] = t;
  }
  if (!grid_col_totals(d, 6, NS, lds, &lastf)) return;
  if (threadIdx.x == 0) {
    const int n = N;
    int flag = d.meta[1] || lds[2 + 2 * F] != 0.0;
    d.meta[1] = flag;
    float l2 = (float)(lds[0] / n);
    float inten = F >= 4 ? (float)(lds[1] / n) : 0.0f;
    float bias = 0.0f, S = 0.0f;
    float sf[F], mf[F];
    for (int f = 0; f < F; ++f) {
      double m = lds[2 + f] / n;
      double var = n > 1 ? (lds[2 + F + f] - n * m * m) / (n - 1) : NAN;
      if (var < 0) var = 0;
      mf[f] = (float)m;
      sf[f] = sqrtf((float)var);
      bias += fabsf(mf[f]);
      S += sf[f];
    }
    bias /= F;
    S /= F;
    float q = 0.0f;
    for (int f = 0; f < F; ++f) q += (sf[f] - S) * (sf[f] - S);
    float imb = sqrtf(q / (F - 1));
    for (int f = 0; f < F; ++f) {
      d.pstat[f] = mf[f];
      d.pstat[MAXF + f] = sf[f];
      // d imb / d pert[n,f] = cimb_f * (pert[n,f] - mean_f)
      float ci = (imb > 0.0f && sf[f] > 0.0f && n > 1)
                     ? (sf[f] - S) / ((F - 1) * imb) / ((n - 1) * sf[f])
                     : 0.0f;
      d.pstat[2 * MAXF + f] = ci;
    }
    if (flag) l2 = inten = bias = imb = 0.0f;
    d.losses[0] = l2;
    d.losses[1] = inten;
    d.losses[2] = bias;
    d.losses[3] = imb;
    d.losses[4] = (float)n;
    d.losses[5] = (float)flag;
    d.losses[6] = 0.0f;
    d.losses[7] = 0.0f;
  }
}

// fused VFE: mean over the slots of the (perturbed) voxel; the unperturbed voxels when the
// NaN / empty fallback fired (adversarial_voxelnet.py:123-132).
__global__ __launch_bounds__(BLK) void k_vfe(Dev d, int F) {
  int t = blockIdx.x * BLK + threadIdx.x;
  if (t >= d.rows * d.vfe_f) return;
  int v = t / d.vfe_f, f = t - v * d.vfe_f;
  const float* src = d.meta[1] ? d.x : d.out;
  const float* p = src + (size_t)v * d.slots * F + f;
  float s = p[0];
  for (int j = 1; j < d.slots; ++j) s += p[(size_t)j * F];
  d.vfe[t] = s / (float)d.npts[v];
}

// fallback: out = x (unperturbed) when the flag is set
__global__ __launch_bounds__(BLK) void k_restore(Dev d, int F) {
  if (!d.meta[1]) return;
  long long n = (long long)d.rows * d.slots * F;
  for (long long t = (long long)blockIdx.x * BLK + threadIdx.x; t < n; t += (long long)gridDim.x * BLK)
    d.out[t] = d.x[t];
}

// eval mode: BN scale/shift from the running stats
__global__ void k_bn_eval(Dev d) {
  for (int l = 0; l < 5; ++l) {
    int C = d.C[l + 1];
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float invstd = 1.0f / sqrtf(d.rv[l][c] + d.eps);
      d.bn[l][c] = d.g[l][c] * invstd;
      d.bn[l][C + c] = d.be[l][c];
      d.bn[l][2 * C + c] = d.rm[l][c];
      d.bn[l][3 * C + c] = invstd;
    }
  }
}

// ------------------------------------------------------------------ per-point boundary layers
// The VALU boundary layers (F -> C0 forward, C4 -> F backward, and the layer-0 BatchNorm backward) as
// per-point passes over ceil(S / BLK) blocks (the point count N lives on the device: blocks past it
// exit) with no reductions in the loop; their BatchNorm sums run as a separate column pass
// (k_colstats). The grid-stride kernels they replaced (k_fwd_first, k_bwd_last, k_bwd_first, since
// removed) reduced every channel of every point with two wave shuffle chains on one wave per SIMD
// (k_bwd_last 96 us, k_fwd_first 55 us for 112k points).
template <int F, int CO>
__global__ __launch_bounds__(BLK) void k_fwd_first_pp(Dev d) {
  __shared__ float sW[CO * F + CO];
  for (int j = threadIdx.x; j < CO * F; j += BLK) sW[j] = d.W[0][j];
  for (int j = threadIdx.x; j < CO; j += BLK) sW[CO * F + j] = d.b[0][j];
  __syncthreads();
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i >= d.meta[0]) return;
  float xv[F], xn[F];
  load_xn<F>(d, point_slot(d, i), xv, xn);
#pragma unroll
  for (int o = 0; o < CO; ++o) {
    float a = sW[CO * F + o];
#pragma unroll
    for (int f = 0; f < F; ++f) a = fmaf(sW[o * F + f], xn[f], a);
    d.z[0][(size_t)o * d.S + i] = a;
  }
}

// per-channel sums over the N points of channel-major [C][S] rows: MODE 0 (forward BatchNorm of
// layer l): sum z, sum z^2 of z_l, then bn_finalize; MODE 1 (backward of layer l): sum g, sum g*xhat_l
// with g = the masked post-ReLU gradient, then bnb_finalize. GRID blocks of contiguous point ranges,
// 1024 threads = 64 channels x 16 lanes of float4 (the whole range in flight at once: 256-thread blocks
// ran these at 1.4 TB/s), double accumulation, fixed-order combine (deterministic).
constexpr int CSB = 1024;
template <int C, int MODE>
__global__ __launch_bounds__(CSB) void k_colstats(Dev d, int l, const float* __restrict__ gsrc, int tk) {
  __shared__ double lds[PSTR];
  __shared__ int lastf;
  const int N = d.meta[0];
  const int rows_per = ((N + GRID - 1) / GRID + 15) & ~15;
  const int p0 = blockIdx.x * rows_per, p1 = min(N, p0 + rows_per);
  const int q = threadIdx.x & 15;
  for (int c0 = 0; c0 < C; c0 += CSB / 16) {
    const int c = c0 + (threadIdx.x >> 4);
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
      const float* zr = d.z[l] + (size_t)c * d.S;
      const float* ar = MODE == 0 ? zr : gsrc + (size_t)c * d.S;
      const float mu = MODE == 1 ? d.bn[l][2 * C + c] : 0.0f;
      const float is = MODE == 1 ? d.bn[l][3 * C + c] : 0.0f;
      for (int pb = p0 + 4 * q; pb < p1; pb += 64 * 8) {
        float4 a[8], z[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int p = pb + 64 * u;
          a[u] = p < p1 ? *(const float4*)(ar + p) : make_float4(0.f, 0.f, 0.f, 0.f);
          z[u] = a[u];
          if (MODE == 1 && p < p1) z[u] = *(const float4*)(zr + p);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int p = pb + 64 * u;
          const float av[4] = {a[u].x, a[u].y, a[u].z, a[u].w}, zv[4] = {z[u].x, z[u].y, z[u].z, z[u].w};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (p + j < p1) {
              s1 += (double)av[j];
              s2 += MODE == 0 ? (double)av[j] * av[j] : (double)(av[j] * ((zv[j] - mu) * is));
            }
        }
      }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    if (q == 0 && c < C) {
      d.part[(size_t)blockIdx.x * PSTR + c] = s1;
      d.part[(size_t)blockIdx.x * PSTR + C + c] = s2;
    }
  }
  if (!grid_col_totals(d, tk, 2 * C, lds, &lastf)) return;
  if (MODE == 0) bn_finalize<C>(d, l, lds);
  else bnb_finalize<C>(d, l, lds);
}

// output layer + attention backward, per point: dz5 = d u, dsig, da, a, and dh4' (BN4 sums: k_colstats).
// Block = 64 points x 4 waves; wave w owns a quarter of the CI channels (their z4 rows are loaded once
// per wave, coalesced over the 64 points), the partial products u = W5 h4 are combined through LDS in
// wave order, and every wave then finishes the per-point output-layer math for its own channels.
template <int CI, int F>
__global__ __launch_bounds__(BLK) void k_bwd_last_pp(Dev d) {
  __shared__ float sW[F * CI + F + 4 * CI];
  __shared__ float su[NWAVE][F][64];
  const int N = d.meta[0];
  if (blockIdx.x * 64 >= N) return;
  for (int j = threadIdx.x; j < F * CI; j += BLK) sW[j] = d.W[5][j];
  for (int j = threadIdx.x; j < F; j += BLK) sW[F * CI + j] = d.b[5][j];
  for (int j = threadIdx.x; j < 4 * CI; j += BLK) sW[F * CI + F + j] = d.bn[4][j];
  __syncthreads();
  const float* sc = sW + F * CI + F;
  const float* sh = sc + CI;
  const float* mean4 = sh + CI;
  const int pl = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + pl;
  const bool act = i < N;
  constexpr int CQ = (CI + NWAVE - 1) / NWAVE;
  const int cb = w * CQ, ce = min(CI, cb + CQ);
  const float* zi = d.z[4] + (act ? i : 0);
  float up[F];
#pragma unroll
  for (int f = 0; f < F; ++f) up[f] = 0.0f;
  if (act) {
#pragma unroll 8
    for (int c = cb; c < ce; ++c) {
      const float hc = fmaxf(fmaf(zi[(size_t)c * d.S] - mean4[c], sc[c], sh[c]), 0.0f);
#pragma unroll
      for (int f = 0; f < F; ++f) up[f] = fmaf(sW[f * CI + c], hc, up[f]);
    }
  }
#pragma unroll
  for (int f = 0; f < F; ++f) su[w][f][pl] = up[f];
  __syncthreads();
  if (!act) return;
  const float gl2 = d.dl[0], gint = d.dl[1], gbias = d.dl[2], gimb = d.dl[3];
  const float invN = 1.0f / (float)N;
  const int slot = point_slot(d, i);
  float xv[F], xn[F], du[F];
  load_xn<F>(d, slot, xv, xn);
  float am[MAXF];
  const float att = d.use_att ? attention<F>(d, xn, am) : 1.0f;
  float raw[F], pp[F], p[F], dout[F];
  float nrm2 = 0.0f;
#pragma unroll
  for (int f = 0; f < F; ++f) {
    float u = sW[F * CI + f];
#pragma unroll
    for (int ww = 0; ww < NWAVE; ++ww) u += su[ww][f][pl];
    raw[f] = tanhf(u);
    pp[f] = (raw[f] * att) * d.bscale[f];
    p[f] = fminf(fmaxf(pp[f], -d.bclamp[f]), d.bclamp[f]);
    nrm2 = fmaf(p[f], p[f], nrm2);
  }
  if (d.fused) {
    const int v = slot / d.slots;
    const float rn = 1.0f / (float)d.npts[v];
#pragma unroll
    for (int f = 0; f < F; ++f) dout[f] = f < d.vfe_f ? d.dout[(size_t)v * d.vfe_f + f] * rn : 0.0f;
  } else {
#pragma unroll
    for (int f = 0; f < F; ++f) dout[f] = d.dout[(size_t)i * F + f];
  }
  const float nrm = sqrtf(nrm2);
  float datt = 0.0f;
#pragma unroll
  for (int f = 0; f < F; ++f) {
    float g = dout[f];
    if (nrm > 0.0f) g += gl2 * invN * (p[f] / nrm);
    if (f == 3) g += gint * invN * (float)((p[3] > 0.0f) - (p[3] < 0.0f));
    const float m = d.pstat[f];
    g += gbias * invN / (float)F * (float)((m > 0.0f) - (m < 0.0f));
    g += gimb * d.pstat[2 * MAXF + f] * (p[f] - m);
    const float dpp = (pp[f] >= -d.bclamp[f] && pp[f] <= d.bclamp[f]) ? g : 0.0f;
    const float draw = dpp * att * d.bscale[f];
    datt = fmaf(dpp * raw[f], d.bscale[f], datt);
    du[f] = draw * (1.0f - raw[f] * raw[f]);
    if (w == 0) d.dz[5][(size_t)f * d.S + i] = du[f];
  }
  if (d.use_att && w == 0) {
    const float dt = datt * att * (1.0f - att);
    d.dsig[i] = dt;
    for (int j = 0; j < d.A; ++j) {
      d.aact[(size_t)j * d.S + i] = am[j];
      d.da[(size_t)j * d.S + i] = am[j] > 0.0f ? d.Wa1[j] * dt : 0.0f;
    }
  }
#pragma unroll 8
  for (int c = cb; c < ce; ++c) {
    float s = 0.0f;
#pragma unroll
    for (int f = 0; f < F; ++f) s = fmaf(sW[f * CI + c], du[f], s);
    const float hc = fmaxf(fmaf(zi[(size_t)c * d.S] - mean4[c], sc[c], sh[c]), 0.0f);
    d.dh[0][(size_t)c * d.S + i] = hc > 0.0f ? s : 0.0f;
  }
}

// layer 0 BatchNorm backward, 4 points of one channel per thread (grid: point quads x CO)
__global__ __launch_bounds__(BLK) void k_bwd_first_pp(Dev d, int src, int CO) {
  const int o = blockIdx.y;
  const int i = (blockIdx.x * BLK + threadIdx.x) * 4;
  const int N = d.meta[0];
  if (i >= N) return;
  const double invN = 1.0 / N;
  const float* bo = d.bn[0];
  const float m1 = (float)(d.bnsum[0][o] * invN), m2 = (float)(d.bnsum[0][CO + o] * invN);
  const float mu = bo[2 * CO + o], is = bo[3 * CO + o], gi = d.g[0][o] * is;
  const size_t base = (size_t)o * d.S + i;
  const float4 z = *(const float4*)(d.z[0] + base);
  const float4 g = *(const float4*)(d.dh[src] + base);
  float4 r;
  r.x = gi * (g.x - m1 - ((z.x - mu) * is) * m2);
  r.y = gi * (g.y - m1 - ((z.y - mu) * is) * m2);
  r.z = gi * (g.z - m1 - ((z.z - mu) * is) * m2);
  r.w = gi * (g.w - m1 - ((z.w - mu) * is) * m2);
  *(float4*)(d.dz[0] + base) = r;
}

// ------------------------------------------------------------------ valid-slot counts (fused mode)
struct ValidCount {
  const float* x;
  int slots, F, rows;
};
// per-row valid-slot counts as a plain pass (the scan then runs over ints: with the counting done inside
// the scan's transform iterator the strided slot reads ran at the scan's low parallelism, 38 us)
// with one thread per point slot (adjacent lanes read adjacent slots: the per-row form read
// each row's slots x F floats serially, 202 us on CenterPoint's 10-sweep voxels): a wave's lanes of one row
// add their valid bits by one popcount of the wave's ballot and one integer atomic (cnt zeroed first; integer
// sums, so the counts do not depend on the order). A slot is valid when its F features, summed in order, are
// not 0 (the same test as k_xstats)
__global__ __launch_bounds__(BLK) void k_valid_count_pts(ValidCount vc, int* __restrict__ cnt) {
  const long long n = (long long)vc.rows * vc.slots;
  const long long p = (long long)blockIdx.x * BLK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool valid = false;
  if (p < n) {
    const float* q = vc.x + p * vc.F;
    float sum = q[0];
    for (int f = 1; f < vc.F; ++f) sum += q[f];
    valid = sum != 0.0f;
  }
  const unsigned long long vb = __ballot(valid);
  if (p < n) {
    const int s = (int)(p % vc.slots);
    if (s == 0 || lane == 0) {   // first lane of this row's segment in the wave
      const int len = min(vc.slots - s, 64 - lane);
      const unsigned long long seg = (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
      const int c = __popcll(vb & seg);
      if (c) atomicAdd(&cnt[p / vc.slots], c);
    }
  }
}

// ------------------------------------------------------------------ launchers
void launch_valid_count(const float* x, int rows, int slots, int F, int* cnt, hipStream_t st) {
  ValidCount vc{x, slots, F, rows};
  const long long npts = (long long)rows * slots;
  if (npts > 0)
    hipLaunchKernelGGL(k_valid_count_pts, dim3((unsigned)((npts + BLK - 1) / BLK)), dim3(BLK), 0, st, vc, cnt);
}

void launch_xstats(Dev& d, hipStream_t st) {
  if (d.F == 4) hipLaunchKernelGGL((k_xstats<4>), dim3(GRID), dim3(BLK), 0, st, d);
  else hipLaunchKernelGGL((k_xstats<5>), dim3(GRID), dim3(BLK), 0, st, d);
}

void launch_bn_eval(Dev& d, hipStream_t st) { hipLaunchKernelGGL(k_bn_eval, dim3(1), dim3(BLK), 0, st, d); }

void launch_restore(Dev& d, hipStream_t st) {
  int ng = grid_for((long long)d.rows * d.slots * d.F, BLK, 1024);
  hipLaunchKernelGGL(k_restore, dim3(ng), dim3(BLK), 0, st, d, d.F);
}

void launch_vfe(Dev& d, hipStream_t st) {
  int nv = (d.rows * d.vfe_f + BLK - 1) / BLK;
  hipLaunchKernelGGL(k_vfe, dim3(nv), dim3(BLK), 0, st, d, d.F);
}

// per-point passes cover every slot the batch can have (S >= N); blocks past N exit at once
static inline dim3 pp_grid(const Dev& d) { return dim3((unsigned)((d.S + BLK - 1) / BLK)); }

int launch_colstats(int C, int mode, Dev& d, int l, const float* g, int tk, hipStream_t st) {
  return for_width(C, [&](auto c) {
    if (mode == 0) hipLaunchKernelGGL((k_colstats<c.value, 0>), dim3(GRID), dim3(CSB), 0, st, d, l, g, tk);
    else hipLaunchKernelGGL((k_colstats<c.value, 1>), dim3(GRID), dim3(CSB), 0, st, d, l, g, tk);
    return (int)RPC_OK;
  });
}

int launch_first(Dev& d, hipStream_t st) {
  return for_width(d.C[1], [&](auto c) {
    if (d.F == 4) hipLaunchKernelGGL((k_fwd_first_pp<4, c.value>), pp_grid(d), dim3(BLK), 0, st, d);
    else hipLaunchKernelGGL((k_fwd_first_pp<5, c.value>), pp_grid(d), dim3(BLK), 0, st, d);
    return (int)RPC_OK;
  });
}

template <int CI, int F>
static int launch_last_t(Dev& d, hipStream_t st, bool bwd) {
  if (bwd) hipLaunchKernelGGL((k_bwd_last_pp<CI, F>), dim3((d.S + 63) / 64), dim3(BLK), 0, st, d);
  else if (d.dsums) hipLaunchKernelGGL((k_fwd_last<CI, F, true>), dim3(GRID), dim3(BLK), 0, st, d);
  else hipLaunchKernelGGL((k_fwd_last<CI, F, false>), dim3(GRID), dim3(BLK), 0, st, d);
  return RPC_OK;
}
int launch_last(Dev& d, hipStream_t st, bool bwd) {
  return for_width(d.C[5], [&](auto c) {
    return d.F == 4 ? launch_last_t<c.value, 4>(d, st, bwd) : launch_last_t<c.value, 5>(d, st, bwd);
  });
}

void launch_bwd_first(Dev& d, hipStream_t st, int src) {
  const int CO = d.C[1];
  const unsigned nq = (unsigned)((d.S / 4 + BLK - 1) / BLK);
  hipLaunchKernelGGL(k_bwd_first_pp, dim3(nq, CO), dim3(BLK), 0, st, d, src, CO);
}

}  // namespace pert
}  // namespace rpc
