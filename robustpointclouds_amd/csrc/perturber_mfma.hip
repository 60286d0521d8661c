// VoxelPerturber, MFMA kernels (see perturber.hip for the structure): the hidden layers whose shape
// fits the 16x16 tiles (mid_on_mfma), forward and backward, with fp32 or 16-bit activation rows, and
// the hidden layers' weight gradients (wgrad_on_mfma) on fp32 or split-bf16 MFMA.
#include "perturber_common.h"

namespace rpc {
namespace pert {

// ------------------------------------------------------------------ fp32 MFMA hidden layers
// The hidden Linear layers as 16-point x 16-channel v_mfma_f32_16x16x4_f32 tiles (fp32 operands,
// fp32 accumulation — the reference arithmetic, only the summation order differs). One wave owns a
// 64-point group = 4 interleaved tiles: A = activations (lane: 4 consecutive points 4(l&15).., channel
// 4s + l>>4, one 16-byte load from the channel-major [C][S] buffers feeds the 4 tiles), B = weights
// from LDS (pitch chosen so the 64 lanes hit 64 distinct banks), D = 4 consecutive points x 1
// channel per lane across the 4 tiles, stored as one 16-byte vector per channel row. BatchNorm batch
// sums are reduced across the 4 lane groups with two shuffles per group and kept in double, then
// combined in fixed order like the VALU kernels.
typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int pitch_mod(int ci, int m) { return ci + ((m - ci % 64) + 64) % 64; }

__device__ __forceinline__ float grp_sum(float v) {  // sum over the 4 lanes sharing l&15
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// BatchNorm batch sums of the MFMA passes: each wave accumulates its channel sums in its own LDS rows
// lds[w][2][MAXC] (double, lanes l < 16 own channel 16j + l of tile column j), then the block
// combines the waves in fixed order into its partial row (keeps 2 * C / 16 doubles out of VGPRs).
__device__ __forceinline__ void wave_sums_zero(double* lds) {
  for (int j = threadIdx.x; j < MFW * 2 * MAXC; j += MFBLK) lds[j] = 0.0;
}
__device__ __forceinline__ double grp_sum(double v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
template <class T>
__device__ __forceinline__ void wave_sums_add(double* lds, int j, T t1, T t2) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  t1 = grp_sum(t1);
  t2 = grp_sum(t2);
  if (lane < 16) {
    lds[(w * 2 + 0) * MAXC + 16 * j + lane] += (double)t1;
    lds[(w * 2 + 1) * MAXC + 16 * j + lane] += (double)t2;
  }
}
template <int C>
__device__ __forceinline__ void tile_flush(double* part, const double* lds) {
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * C; j += MFBLK) {
    int which = j / C, c = j - which * C;
    double t = 0.0;
    for (int ww = 0; ww < MFW; ++ww) t += lds[(ww * 2 + which) * MAXC + c];
    part[(size_t)blockIdx.x * PSTR + j] = t;
  }
}

// 4 consecutive points n..n+3 of one channel row (n % 4 == 0). Rows are S >= 64-rounded N floats
// long and n lies in a 64-point group (16-point block) that starts below N, so the 16-byte access never leaves the row:
// branch-free (a tail branch per access made the compiler wait for every outstanding load at each
// join); points >= N read as 0 and are written with whatever the caller put there (0: masked).
__device__ __forceinline__ f32x4 ld4(const float* p, int n, int N) {
  f32x4 v = *(const f32x4*)(p + n);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = n + i < N ? v[i] : 0.0f;
  return v;
}
// Q = 2 or 4 consecutive points of one channel row (same contract as ld4, n % Q == 0)
template <int Q>
using fvec = float __attribute__((ext_vector_type(Q)));
template <int Q>
__device__ __forceinline__ fvec<Q> ldq(const float* p, int n, int N) {
  fvec<Q> v = *(const fvec<Q>*)(p + n);
#pragma unroll
  for (int i = 0; i < Q; ++i) v[i] = n + i < N ? v[i] : 0.0f;
  return v;
}
template <int Q>
__device__ __forceinline__ void stq(float* p, int n, fvec<Q> v) { *(fvec<Q>*)(p + n) = v; }

// 16-bit activation rows (perf mode, rpc_perturber_cfg.act16): the same channel-major [C][S] rows with 2-byte
// elements — fp16 for the hidden pre-activations z_1..z_3 (the reference AMP's Linear outputs, train.py:91-103;
// finite values saturate at +-65504 like the fp16 sparse rows), bf16 for the gradient rows dh / dz_1..dz_4
// (unscaled gradients ~1e-7 need bf16's range; the AMP's loss scaling has no counterpart here). Values that
// are stored are also what the producer's BatchNorm sums see (rnd), so the statistics describe the rows.
typedef _Float16 f16;
typedef __bf16 b16;
__device__ __forceinline__ float rnd(float v, float*) { return v; }
__device__ __forceinline__ float rnd(float v, f16*) { return (float)(f16)fminf(fmaxf(v, -65504.0f), 65504.0f); }
__device__ __forceinline__ float rnd(float v, b16*) { return (float)(b16)v; }
template <typename T>
__device__ __forceinline__ float rnd_as(float v) { return rnd(v, (T*)nullptr); }
template <int Q, typename T>
__device__ __forceinline__ fvec<Q> ldq(const T* p, int n, int N) {
  if constexpr (sizeof(T) == 4) {
    return ldq<Q>((const float*)p, n, N);
  } else {
    typedef T tv __attribute__((ext_vector_type(Q)));
    const tv h = *(const tv*)(p + n);
    fvec<Q> v;
#pragma unroll
    for (int i = 0; i < Q; ++i) v[i] = n + i < N ? (float)h[i] : 0.0f;
    return v;
  }
}
// the values must already be representable (rnd_as<T>): the conversion is then exact
template <int Q, typename T>
__device__ __forceinline__ void stq(T* p, int n, fvec<Q> v) {
  if constexpr (sizeof(T) == 4) {
    stq<Q>((float*)p, n, v);
  } else {
    typedef T tv __attribute__((ext_vector_type(Q)));
    tv h;
#pragma unroll
    for (int i = 0; i < Q; ++i) h[i] = (T)v[i];
    *(tv*)(p + n) = h;
  }
}
// element types of one hidden-layer launch (host-chosen per layer, see row_types)
template <class ZI, class ZO>
struct FwdT {
  using zi = ZI;   // z_{l-1} rows read
  using zo = ZO;   // z_l rows written
};
template <class ZL, class ZP, class GI, class GO, class DZ>
struct BwdT {
  using zl = ZL;   // z_l rows read
  using zp = ZP;   // z_{l-1} rows read (ReLU mask of h_{l-1})
  using gi = GI;   // dh_l rows read
  using go = GO;   // dh_{l-1} rows written
  using dz = DZ;   // dz_l rows written (read by the weight gradient)
};
using FwdF32 = FwdT<float, float>;
using BwdF32 = BwdT<float, float, float, float, float>;
// W_l [R][CI] row-major -> LDS rows of pitch P: all of a thread's loads in flight before its first LDS
// store (a load -> store loop waited out one L2 round trip per pass: 16 at the start of every block)
template <int NTOT, int CI, int P>
__device__ __forceinline__ void stage_w(float* sW, const float* __restrict__ W) {
  constexpr int NQ = (NTOT + MFBLK - 1) / MFBLK;
  float v[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) v[i] = W[min((int)threadIdx.x + i * MFBLK, NTOT - 1)];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int j = threadIdx.x + i * MFBLK;
    if (j < NTOT) sW[(j / CI) * P + j % CI] = v[i];
  }
}
// interleaved tiles per wave group: 4 (64 points, 16-byte accesses) while the group's activation
// operand fits 64 VGPRs, else 2 (32 points, 8-byte accesses) — 2 waves per SIMD, no spills
__host__ __device__ constexpr int tiles_per_group(int ks) { return ks * 4 <= 64 ? 4 : 2; }

// layer l (1..4) forward: z_l = W_l relu(bn_{l-1}(z_{l-1})) + b_l, BN_l batch statistics.
// A wave owns a 64-point group as 4 interleaved MFMA tiles: tile q holds points n0 + 4m + q (m = row),
// so the A operand of all 4 tiles for channel 4s + g is ONE 16-byte load of points n0 + 4a .. +3, and
// the 4 tiles' D values for output row 4g + i are 4 consecutive points (one 16-byte store). Every
// weight read from LDS feeds 4 MFMAs. Groups go to waves block-fastest (t = wave * GRID + block) so
// each CU gets an equal share when N / 64 is not much larger than the wave count.
template <int CI, int CO, class RT>
__global__ __launch_bounds__(MFBLK) void k_fwd_mid_mf(Dev d, int l) {
  using ZI = typename RT::zi;
  using ZO = typename RT::zo;
  constexpr int P = pitch_mod(CI, 4), NT = CO / 16, KS = CI / 4, TQ = tiles_per_group(KS), GP = 16 * TQ;
  __shared__ float sW[CO * P];
  __shared__ float sp[3 * CI + CO];
  __shared__ double lds[MFW * 2 * MAXC];
  __shared__ int lastf;
  stage_w<CO * CI, CI, P>(sW, d.W[l]);
  for (int j = threadIdx.x; j < 3 * CI; j += MFBLK) sp[j] = d.bn[l - 1][j];
  for (int j = threadIdx.x; j < CO; j += MFBLK) sp[3 * CI + j] = d.b[l][j];
  wave_sums_zero(lds);
  __syncthreads();
  const float* sc = sp;
  const float* sh = sp + CI;
  const float* mu = sp + 2 * CI;
  const float* bias = sp + 3 * CI;
  const int N = d.meta[0];
  const int lane = threadIdx.x & 63, a = lane & 15, g = lane >> 4, wv = threadIdx.x >> 6;
  const ZI* zin = (const ZI*)d.z[l - 1];
  ZO* zout = (ZO*)d.z[l];
  for (int t = wv * GRID + blockIdx.x; t * GP < N; t += GRID * MFW) {
    const int n0 = t * GP, na = n0 + TQ * a;
    fvec<TQ> hv[KS];
    // all KS activation loads in flight before the first BN / ReLU (load + transform per s waited out
    // one round trip per s)
#pragma unroll
    for (int s = 0; s < KS; ++s) hv[s] = ldq<TQ>(zin + (size_t)(4 * s + g) * d.S, na, N);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int c = 4 * s + g;
#pragma unroll
      for (int q = 0; q < TQ; ++q) hv[s][q] = na + q < N ? fmaxf(fmaf(hv[s][q] - mu[c], sc[c], sh[c]), 0.0f) : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float b = bias[16 * j + a];
      f32x4 v[TQ];
#pragma unroll
      for (int q = 0; q < TQ; ++q) v[q] = (f32x4){b, b, b, b};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float w = sW[(16 * j + a) * P + 4 * s + g];
#pragma unroll
        for (int q = 0; q < TQ; ++q) v[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[s][q], w, v[q], 0, 0, 0);
      }
      ZO* row = zout + (size_t)(16 * j + a) * d.S;
      fvec<TQ> o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int nb = n0 + TQ * (4 * g + i);
#pragma unroll
        for (int q = 0; q < TQ; ++q) o[i][q] = nb + q < N ? rnd_as<ZO>(v[q][i]) : 0.0f;
        stq<TQ>(row, nb, o[i]);
      }
      if (d.training) {
        if (d.dsums) {
          // parity mode: sum z and sum z^2 in double (the square of a float is exact there). The batch variance
          // is their difference, and float sums lose it where |mean| >> std (6e-8 mean^2 against var + eps:
          // 0.3 % of the dominant channel's gradient with two points)
          double t1 = 0.0, t2 = 0.0;
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < TQ; ++q) {
              const double od = (double)o[i][q];
              t1 += od;
              t2 = fma(od, od, t2);
            }
          wave_sums_add(lds, j, t1, t2);
        } else {
          float t1 = 0.0f, t2 = 0.0f;
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < TQ; ++q) {
              t1 += o[i][q];
              t2 = fmaf(o[i][q], o[i][q], t2);
            }
          wave_sums_add(lds, j, t1, t2);
        }
      }
      asm volatile("" ::: "memory");  // keep the next tile's B reads here (register pressure)
    }
  }
  if (!d.training) return;
  tile_flush<CO>(d.part, lds);
  if (!grid_col_totals(d, 1 + l, 2 * CO, lds, &lastf)) return;
  bn_finalize<CO>(d, l, lds);
}

// layer l (4..1) backward: dz_l = BN_l backward of dh_l (stored), dh_{l-1} = relu'(h_{l-1}) W_l^T dz_l,
// BN_{l-1} backward sums (sum dh, sum dh * xhat). Same interleaved point groups as the forward.
template <int CI, int CO, class RT>
__global__ __launch_bounds__(MFBLK) void k_bwd_mid_mf(Dev d, int l, int src) {
  using ZL = typename RT::zl;
  using ZP = typename RT::zp;
  using GI = typename RT::gi;
  using GO = typename RT::go;
  using DZ = typename RT::dz;
  constexpr int P = pitch_mod(CI, 16), NT = CI / 16, KS = CO / 4, TQ = tiles_per_group(KS), GP = 16 * TQ;
  __shared__ float sW[CO * P];
  __shared__ float sp[7 * CO + 4 * CI];
  __shared__ double lds[MFW * 2 * MAXC];
  __shared__ int lastf;
  const int N = d.meta[0];
  const double invN = 1.0 / N;
  stage_w<CO * CI, CI, P>(sW, d.W[l]);
  for (int j = threadIdx.x; j < 4 * CO; j += MFBLK) sp[j] = d.bn[l][j];
  for (int j = threadIdx.x; j < 4 * CI; j += MFBLK) sp[4 * CO + j] = d.bn[l - 1][j];
  for (int j = threadIdx.x; j < CO; j += MFBLK) {
    float* m = sp + 4 * CO + 4 * CI;
    m[j] = (float)(d.bnsum[l][j] * invN);
    m[CO + j] = (float)(d.bnsum[l][CO + j] * invN);
    m[2 * CO + j] = d.g[l][j] * d.bn[l][3 * CO + j];
  }
  wave_sums_zero(lds);
  __syncthreads();
  const float* bo = sp;            // scale, beta, mean, invstd of layer l
  const float* bi = sp + 4 * CO;   // of layer l-1
  const float* m1 = bi + 4 * CI;
  const float* m2 = m1 + CO;
  const float* gi = m2 + CO;
  const int lane = threadIdx.x & 63, a = lane & 15, g = lane >> 4, wv = threadIdx.x >> 6;
  const GI* dhin = (const GI*)d.dh[src];
  GO* dhout = (GO*)d.dh[src ^ 1];
  const ZL* zl = (const ZL*)d.z[l];
  const ZP* zp = (const ZP*)d.z[l - 1];
  DZ* dzl = (DZ*)d.dz[l];
  for (int t = wv * GRID + blockIdx.x; t * GP < N; t += GRID * MFW) {
    const int n0 = t * GP, na = n0 + TQ * a;
    fvec<TQ> dzv[KS];
    // 8 channel rows per batch: their z / dh loads all in flight before the batch's dz stores (the
    // stores may alias the next rows' loads, so a load -> store per row waited one round trip per row)
    constexpr int SB = KS < 8 ? KS : 8;
#pragma unroll
    for (int s0 = 0; s0 < KS; s0 += SB) {
      fvec<TQ> zv[SB], dv[SB];
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const int o = 4 * (s0 + u) + g;
        zv[u] = ldq<TQ>(zl + (size_t)o * d.S, na, N);
        dv[u] = ldq<TQ>(dhin + (size_t)o * d.S, na, N);
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const int s = s0 + u, o = 4 * s + g;
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
          const float xh = (zv[u][q] - bo[2 * CO + o]) * bo[3 * CO + o];
          dzv[s][q] = na + q < N ? gi[o] * (dv[u][q] - m1[o] - xh * m2[o]) : 0.0f;
        }
        if constexpr (sizeof(DZ) == 4) {
          stq<TQ>(dzl + (size_t)o * d.S, na, dzv[s]);
        } else {   // the weight gradient's rows (bf16); this kernel's data gradient keeps the fp32 values
          fvec<TQ> r;
#pragma unroll
          for (int q = 0; q < TQ; ++q) r[q] = rnd_as<DZ>(dzv[s][q]);
          stq<TQ>(dzl + (size_t)o * d.S, na, r);
        }
      }
      asm volatile("" ::: "memory");  // bound the loads in flight (register pressure)
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int c = 16 * j + a;
      fvec<TQ> zc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) zc[i] = ldq<TQ>(zp + (size_t)c * d.S, n0 + TQ * (4 * g + i), N);
      f32x4 v[TQ];
#pragma unroll
      for (int q = 0; q < TQ; ++q) v[q] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float w = sW[(4 * s + g) * P + c];
#pragma unroll
        for (int q = 0; q < TQ; ++q) v[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(dzv[s][q], w, v[q], 0, 0, 0);
      }
      float t1 = 0.0f, t2 = 0.0f;
      GO* row = dhout + (size_t)c * d.S;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int nb = n0 + TQ * (4 * g + i);
        fvec<TQ> o;
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
          const float hv = fmaxf(fmaf(zc[i][q] - bi[2 * CI + c], bi[c], bi[CI + c]), 0.0f);
          o[q] = (nb + q < N && hv > 0.0f) ? rnd_as<GO>(v[q][i]) : 0.0f;
          t1 += o[q];
          t2 += o[q] * ((zc[i][q] - bi[2 * CI + c]) * bi[3 * CI + c]);
        }
        stq<TQ>(row, nb, o);
      }
      wave_sums_add(lds, j, t1, t2);
      asm volatile("" ::: "memory");  // keep the next tile's B reads here (register pressure)
    }
  }
  tile_flush<CI>(d.part, lds);
  if (!grid_col_totals(d, 7 + (5 - l), 2 * CI, lds, &lastf)) return;
  bnb_finalize<CI>(d, l - 1, lds);
}

// weight gradient of a hidden layer: dW[o][c] = sum_n dz_l[o][n] h_{l-1}[c][n], db[o] = sum_n dz_l[o][n],
// h = relu(bn_{l-1}(z_{l-1})). K = points: lane k-slot j of a 16-point block holds point 4(l>>4) + j,
// one 16-byte load per channel row for A and B alike. grid (KS row chunks, jobs): the 4 waves take
// interleaved 16-point blocks of the chunk and are combined in LDS in wave order; one slab row of
// the job's CO*(CI+1) elements per block (reduced with the VALU jobs by k_wgrad_reduce). MfJob / MfJobs:
// perturber_common.h.
template <int CO, int CI>
__global__ __launch_bounds__(BLK, 2) void k_wgrad_mf(Dev d, MfJobs J) {
  // every block covers ALL output tiles of its point chunk (h_{l-1} and dz_l are read once per chunk;
  // splitting the outputs over blocks re-read h CO/16 times): wave wv accumulates the 16-point
  // blocks r0 + 16 wv, + 64, ... into CO/16 x CI/16 tiles (<= 32: 128 accumulator VGPRs), the 4 waves
  // are summed in wave order through one LDS image
  constexpr int TO = CO / 16, TC = CI / 16;
  static_assert(TO * TC <= 32, "accumulator tiles");
  __shared__ float red[CO * CI];
  __shared__ float bred[NWAVE][CO];
  const MfJob& job = J.j[blockIdx.y];
  const int N = d.meta[0];
  const int rows_per = ((N + J.KS - 1) / J.KS + 15) & ~15;
  const int r0 = blockIdx.x * rows_per, r1 = min(N, r0 + rows_per);
  const int lane = threadIdx.x & 63, a = lane & 15, g = lane >> 4, wv = threadIdx.x >> 6;
  float sc[TC], sh[TC], mu[TC];
#pragma unroll
  for (int jc = 0; jc < TC; ++jc) {
    const int c = 16 * jc + a;
    sc[jc] = job.bn[c];
    sh[jc] = job.bn[CI + c];
    mu[jc] = job.bn[2 * CI + c];
  }
  f32x4 acc[TO][TC];
  float bsum[TO];
#pragma unroll
  for (int i = 0; i < TO; ++i) {
    bsum[i] = 0.0f;
#pragma unroll
    for (int jc = 0; jc < TC; ++jc) acc[i][jc] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  }
  for (int n0 = r0 + 16 * wv; n0 < r1; n0 += 16 * NWAVE) {
    const int nb = n0 + 4 * g;
    f32x4 av[TO], bv[TC];
#pragma unroll
    for (int i = 0; i < TO; ++i) av[i] = ld4(job.dz + (size_t)(16 * i + a) * d.S, nb, r1);
#pragma unroll
    for (int jc = 0; jc < TC; ++jc) {
      const f32x4 zc = ld4(job.z + (size_t)(16 * jc + a) * d.S, nb, r1);
#pragma unroll
      for (int k = 0; k < 4; ++k) bv[jc][k] = nb + k < r1 ? fmaxf(fmaf(zc[k] - mu[jc], sc[jc], sh[jc]), 0.0f) : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < TO; ++i) bsum[i] += (av[i][0] + av[i][1]) + (av[i][2] + av[i][3]);
    // k outermost: consecutive MFMAs update different accumulators (the 4 k-steps of one tile back to
    // back waited out the 16x16x4 f32 dependent latency, 40 of every 32-cycle issue slot); each tile
    // still sums k = 0..3 in order
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int i = 0; i < TO; ++i)
#pragma unroll
        for (int jc = 0; jc < TC; ++jc)
          acc[i][jc] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][k], bv[jc][k], acc[i][jc], 0, 0, 0);
  }
  // lane (a, g) of tile (i, jc) holds dW[16i + 4g + r][16jc + a]; waves summed in order 0, 1, 2, 3
  for (int ww = 0; ww < NWAVE; ++ww) {
    if (wv == ww) {
#pragma unroll
      for (int i = 0; i < TO; ++i)
#pragma unroll
        for (int jc = 0; jc < TC; ++jc)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* e = &red[(16 * i + 4 * g + r) * CI + 16 * jc + a];
            *e = ww == 0 ? acc[i][jc][r] : *e + acc[i][jc][r];
          }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < TO; ++i) {
    const float bt = grp_sum(bsum[i]);
    if (g == 0) bred[wv][16 * i + a] = bt;
  }
  __syncthreads();
  float* out = d.wpart + (size_t)blockIdx.x * J.total + job.eoff;
  for (int e = threadIdx.x; e < CO * (CI + 1); e += BLK) {
    const int o = e / (CI + 1), c = e - o * (CI + 1);
    out[e] = c < CI ? red[o * CI + c] : ((bred[0][o] + bred[1][o]) + bred[2][o]) + bred[3][o];
  }
}

// Perf mode (cfg->wgrad_split_bf16): the same weight gradient on bf16 MFMA with each fp32 operand split
// into hi = bf16(v) and lo = bf16(v - hi) and dW += lo_a hi_b + hi_a lo_b + hi_a hi_b (fp32 accumulate):
// ~16 significant bits per product (relative error ~2^-16, the lo*lo term dropped) at 3 x 16-cycle
// v_mfma_f32_16x16x32_bf16 per 32 points where the fp32 path issues 8 x 32-cycle 16x16x4 MFMAs (5.3x
// fewer MFMA cycles). Lane (a, g) holds 8 consecutive points n0 + 8g .. of channel row 16i + a (A = dz_l
// rows, B = h_{l-1} rows), so one k-step covers 32 points; the tile / wave / bias bookkeeping is
// k_wgrad_mf's (same slab row, reduced by k_wgrad_reduce).
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split_bf16x8(const float* v, bf16x8_t& hi, bf16x8_t& lo) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const __bf16 h = (__bf16)v[k];
    hi[k] = h;
    lo[k] = (__bf16)(v[k] - (float)h);
  }
}

template <int CO, int CI, class DZ, class ZP>
__global__ __launch_bounds__(BLK, 2) void k_wgrad_bx3(Dev d, MfJobs J) {
  // DZ / ZP: element types of the dz_l / z_{l-1} rows (float, or the 16-bit rows of act16); bf16 dz rows are
  // their own hi part (lo = 0 exactly), so their lo * hi product is skipped
  // above 8 accumulator tiles the output tiles are split in two halves (along the wider of CO / CI): waves
  // (2p + h) take half h of the tiles over the point stream p (32-point blocks, the 2 streams interleaved),
  // so a wave holds at most 16 tiles plus its hi / lo operand splits without spilling; the operand rows of
  // the other dimension are loaded by both halves (the second read hits L2)
  constexpr int TO = CO / 16, TC = CI / 16;
  static_assert(TO * TC <= 32, "accumulator tiles");
  constexpr bool SPLIT = TO * TC > 8, SPLIT_C = SPLIT && TC >= TO, SPLIT_O = SPLIT && !SPLIT_C;
  constexpr int TOW = SPLIT_O ? TO / 2 : TO, TCW = SPLIT_C ? TC / 2 : TC;
  constexpr int NSTREAM = SPLIT ? NWAVE / 2 : NWAVE;
  __shared__ float red[CO * CI];
  __shared__ float bred[NWAVE][CO];
  const MfJob& job = J.j[blockIdx.y];
  const int N = d.meta[0];
  const int rows_per = ((N + J.KS - 1) / J.KS + 31) & ~31;
  const int r0 = blockIdx.x * rows_per, r1 = min(N, r0 + rows_per);
  const int lane = threadIdx.x & 63, a = lane & 15, g = lane >> 4, wv = threadIdx.x >> 6;
  const int half = SPLIT ? (wv & 1) : 0, stream = SPLIT ? (wv >> 1) : wv;
  const int o0 = SPLIT_O ? half * TOW : 0, c0 = SPLIT_C ? half * TCW : 0;   // first tile row / column
  float sc[TCW], sh[TCW], mu[TCW];
#pragma unroll
  for (int jc = 0; jc < TCW; ++jc) {
    const int c = 16 * (c0 + jc) + a;
    sc[jc] = job.bn[c];
    sh[jc] = job.bn[CI + c];
    mu[jc] = job.bn[2 * CI + c];
  }
  f32x4 acc[TOW][TCW];
  float bsum[TOW];
#pragma unroll
  for (int i = 0; i < TOW; ++i) {
    bsum[i] = 0.0f;
#pragma unroll
    for (int jc = 0; jc < TCW; ++jc) acc[i][jc] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  }
  for (int n0 = r0 + 32 * stream; n0 < r1; n0 += 32 * NSTREAM) {
    const int nb = n0 + 8 * g;
    f32x4 dv[TOW][2], zv[TCW][2];
#pragma unroll
    for (int i = 0; i < TOW; ++i) {
      const DZ* row = (const DZ*)job.dz + (size_t)(16 * (o0 + i) + a) * d.S;
      dv[i][0] = ldq<4>(row, nb, r1);
      dv[i][1] = ldq<4>(row, nb + 4, r1);
    }
#pragma unroll
    for (int jc = 0; jc < TCW; ++jc) {
      const ZP* row = (const ZP*)job.z + (size_t)(16 * (c0 + jc) + a) * d.S;
      zv[jc][0] = ldq<4>(row, nb, r1);
      zv[jc][1] = ldq<4>(row, nb + 4, r1);
    }
    bf16x8_t ah[TOW], al[TOW];
#pragma unroll
    for (int i = 0; i < TOW; ++i) {
      float t[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        t[k] = dv[i][0][k];
        t[4 + k] = dv[i][1][k];
      }
      bsum[i] += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
      split_bf16x8(t, ah[i], al[i]);
    }
#pragma unroll
    for (int jc = 0; jc < TCW; ++jc) {
      float t[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float z = k < 4 ? zv[jc][0][k] : zv[jc][1][k - 4];
        t[k] = nb + k < r1 ? fmaxf(fmaf(z - mu[jc], sc[jc], sh[jc]), 0.0f) : 0.0f;
      }
      bf16x8_t bh, bl;
      split_bf16x8(t, bh, bl);
#pragma unroll
      for (int i = 0; i < TOW; ++i) {
        if constexpr (!std::is_same<DZ, b16>::value)
          acc[i][jc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, acc[i][jc], 0, 0, 0);
        acc[i][jc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, acc[i][jc], 0, 0, 0);
        acc[i][jc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, acc[i][jc], 0, 0, 0);
      }
    }
  }
  // streams summed in order per tile (the two halves own disjoint tiles)
  for (int s = 0; s < NSTREAM; ++s) {
    if (stream == s) {
#pragma unroll
      for (int i = 0; i < TOW; ++i)
#pragma unroll
        for (int jc = 0; jc < TCW; ++jc)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* e = &red[(16 * (o0 + i) + 4 * g + r) * CI + 16 * (c0 + jc) + a];
            *e = s == 0 ? acc[i][jc][r] : *e + acc[i][jc][r];
          }
    }
    __syncthreads();
  }
  // bias sums: every stream's own rows (with the CI split both halves summed the same rows: half 0 only)
#pragma unroll
  for (int i = 0; i < TOW; ++i) {
    const float bt = grp_sum(bsum[i]);
    if (g == 0 && !(SPLIT_C && half == 1)) bred[stream][16 * (o0 + i) + a] = bt;
  }
  __syncthreads();
  float* out = d.wpart + (size_t)blockIdx.x * J.total + job.eoff;
  for (int e = threadIdx.x; e < CO * (CI + 1); e += BLK) {
    const int o = e / (CI + 1), c = e - o * (CI + 1);
    float b = 0.0f;
    if (c == CI)
      for (int s2 = 0; s2 < NSTREAM; ++s2) b += bred[s2][o];
    out[e] = c < CI ? red[o * CI + c] : b;
  }
}

// ------------------------------------------------------------------ launchers
template <bool H>
using Z16 = typename std::conditional<H, f16, float>::type;
template <bool H>
using G16 = typename std::conditional<H, b16, float>::type;
// row types of layer l: z_1..z_3 16-bit (z_0 / z_4 stay fp32: the per-point boundary passes read them), dh_l
// 16-bit between hidden layers (dh_4 comes from the fp32 output-layer pass, dh_0 feeds the fp32 layer-0 pass)
template <int CI, int CO, bool ZH, bool GH>
static void launch_mid16(Dev& d, int l, hipStream_t st, bool bwd, int src) {
  if (bwd) {
    if (l == 4)
      hipLaunchKernelGGL((k_bwd_mid_mf<CI, CO, BwdT<float, Z16<ZH>, float, G16<GH>, G16<GH>>>), dim3(GRID), dim3(MFBLK),
                         0, st, d, l, src);
    else if (l == 1)
      hipLaunchKernelGGL((k_bwd_mid_mf<CI, CO, BwdT<Z16<ZH>, float, G16<GH>, float, G16<GH>>>), dim3(GRID), dim3(MFBLK),
                         0, st, d, l, src);
    else
      hipLaunchKernelGGL((k_bwd_mid_mf<CI, CO, BwdT<Z16<ZH>, Z16<ZH>, G16<GH>, G16<GH>, G16<GH>>>), dim3(GRID),
                         dim3(MFBLK), 0, st, d, l, src);
  } else {
    if (l == 1)
      hipLaunchKernelGGL((k_fwd_mid_mf<CI, CO, FwdT<float, Z16<ZH>>>), dim3(GRID), dim3(MFBLK), 0, st, d, l);
    else if (l == 4)
      hipLaunchKernelGGL((k_fwd_mid_mf<CI, CO, FwdT<Z16<ZH>, float>>), dim3(GRID), dim3(MFBLK), 0, st, d, l);
    else
      hipLaunchKernelGGL((k_fwd_mid_mf<CI, CO, FwdT<Z16<ZH>, Z16<ZH>>>), dim3(GRID), dim3(MFBLK), 0, st, d, l);
  }
}
// hidden layer l of an MFMA shape: 16-bit rows where act16 asks for them and the shape has them, else fp32 rows
template <int CI, int CO>
static int launch_mid_t(Dev& d, int l, hipStream_t st, bool bwd, int src) {
  if constexpr (a16_shape(CI, CO)) {
    switch (d.a16) {
      case 1: launch_mid16<CI, CO, true, false>(d, l, st, bwd, src); return RPC_OK;
      case 2: launch_mid16<CI, CO, false, true>(d, l, st, bwd, src); return RPC_OK;
      case 3: launch_mid16<CI, CO, true, true>(d, l, st, bwd, src); return RPC_OK;
      default: break;
    }
  }
  if (bwd) {
    if constexpr (mid_on_mfma(CI, CO, true)) {
      hipLaunchKernelGGL((k_bwd_mid_mf<CI, CO, BwdF32>), dim3(GRID), dim3(MFBLK), 0, st, d, l, src);
      return RPC_OK;
    }
  } else {
    if constexpr (mid_on_mfma(CI, CO, false)) {
      hipLaunchKernelGGL((k_fwd_mid_mf<CI, CO, FwdF32>), dim3(GRID), dim3(MFBLK), 0, st, d, l);
      return RPC_OK;
    }
  }
  return RPC_ERR_UNSUPPORTED;  // a VALU shape: not instantiated here
}
int launch_mid_mfma(int CI, int CO, Dev& d, int l, hipStream_t st, bool bwd, int src) {
  return for_width(CI, [&](auto ci) {
    return for_width(CO, [&](auto co) { return launch_mid_t<ci.value, co.value>(d, l, st, bwd, src); });
  });
}
// zh16: the jobs' z_{l-1} rows are fp16 (act16 bit 0, layers 2..4); dz rows are bf16 under act16 bit 1. Both only
// reach the split-bf16 kernel: fill_dev clears d.a16 without it, so k_wgrad_mf always sees fp32 rows
template <int CO, int CI>
static int launch_wgrad_mf_t(Dev& d, const MfJobs& M, int njob, bool split, bool zh16, hipStream_t st) {
  if constexpr (wgrad_on_mfma(CO, CI)) {
    if (split) {
      const bool gh = d.a16 & 2;
      if constexpr (a16_shape(CI, CO)) {
        if (zh16 && gh) { hipLaunchKernelGGL((k_wgrad_bx3<CO, CI, b16, f16>), dim3(M.KS, njob), dim3(BLK), 0, st, d, M); return RPC_OK; }
        if (zh16) { hipLaunchKernelGGL((k_wgrad_bx3<CO, CI, float, f16>), dim3(M.KS, njob), dim3(BLK), 0, st, d, M); return RPC_OK; }
        if (gh) { hipLaunchKernelGGL((k_wgrad_bx3<CO, CI, b16, float>), dim3(M.KS, njob), dim3(BLK), 0, st, d, M); return RPC_OK; }
      }
      hipLaunchKernelGGL((k_wgrad_bx3<CO, CI, float, float>), dim3(M.KS, njob), dim3(BLK), 0, st, d, M);
    } else {
      hipLaunchKernelGGL((k_wgrad_mf<CO, CI>), dim3(M.KS, njob), dim3(BLK), 0, st, d, M);
    }
    return RPC_OK;
  }
  return RPC_ERR_UNSUPPORTED;  // a job of the VALU kernels: not instantiated here
}
int launch_wgrad_mfma(int CO, int CI, Dev& d, const MfJobs& M, int njob, bool split, bool zh16, hipStream_t st) {
  return for_width(CO, [&](auto co) {
    return for_width(CI, [&](auto ci) { return launch_wgrad_mf_t<co.value, ci.value>(d, M, njob, split, zh16, st); });
  });
}

}  // namespace pert
}  // namespace rpc
