// The SimSiam visual self-supervision head (include/ctclip_hip.h, ctclip_ssl_linear_bn / ctclip_ssl_bn_bwd /
// ctclip_simsiam_loss; Chen & He 2021, "Exploring Simple Siamese Representation Learning").
//
// (a) lb_kernel: Linear + BatchNorm1d (+ ReLU) in one launch.  BatchNorm reduces over ROWS per feature, so a
//     workgroup that owns a strip of 16 output features for ALL rows (G groups of R rows, G R <= 128) has the
//     statistics locally: no second pass, no atomics.  y = X W^T on the f32 matrix pipe as sgemm_tn.hip does
//     it (v_mfma_f32_16x16x4_f32, exact f32, one fma chain per output in ascending k; W is the first MFMA
//     operand, so a lane ends with one row and 4 consecutive features).  The strip is ONE 16 x 16 block per
//     16 rows: wave w owns the row blocks w and w + 4.  N = 4096 gives 256 workgroups, one per CU, each
//     streaming its 16 rows of W from HBM once; X is re-read through L2 by every workgroup.
//     K step 32: operands register-staged with 16-B loads into double-buffered LDS images [rows][32 k] with a
//     36-float row stride (16-B aligned writes, the 64 lanes' fragment reads on 64 banks), one barrier per
//     step.  One workgroup per CU means one step of loads in flight would leave the launch waiting on HBM
//     latency, so the loads run a ring of RING steps ahead in registers.
//     Epilogue through LDS: the y tile [rows][16], then one thread per (group, feature): mean and biased
//     variance over the group's rows ascending, xhat, out, rstd; then one thread per feature folds the
//     groups' statistics into the running ones, g ascending.
// (b) bnb_kernel: the BatchNorm (+ ReLU) backward, one thread per feature column, lanes along N.
// (c) ss_row_kernel / ss_sum_kernel: the SimSiam loss and its gradient, a wave per row; the row terms are
//     folded by one workgroup in a fixed order.
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int MAXROWS = 128;      // G R
constexpr int NS = 16;            // features of a workgroup
constexpr int KT = 32;            // K step
constexpr int LDR = 36;           // LDS image row stride (floats)
constexpr int NTH = 256;
constexpr int RING = 4;           // K steps of loads in flight
constexpr int STAGE = (MAXROWS + NS) * LDR;     // one buffer: X image, then W image
constexpr int LDY = NS + 1;       // y tile row stride

struct LP {
  const float* X; int64_t ldx;
  const float* W;
  const float* bias; const float* gamma; const float* beta;
  float* rm; float* rv;
  int G, R, M;
  int64_t K, N;
  int relu, use_running;
  float eps, mom;
  float* out; float* xhat; float* rstd;
};

// XPT: 16-B chunks of the X image per thread and step (rows (t + 256 i) / 8, k quad t % 8)
template <int XPT>
struct Regs {
  f32x4 x[XPT];
  f32x4 w;
};

template <int XPT>
__device__ __forceinline__ void lb_load(Regs<XPT>& r, const LP& p, int64_t n0, int64_t k0) {
  const int t = threadIdx.x;
  const int64_t gk = k0 + (t & 7) * 4;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int row = (t + NTH * i) >> 3;
    r.x[i] = (row < p.M && gk < p.K) ? *(const f32x4*)(p.X + (int64_t)row * p.ldx + gk) : zero;
  }
  const int64_t gn = n0 + (t >> 3);
  r.w = (t < NS * 8 && gn < p.N && gk < p.K) ? *(const f32x4*)(p.W + gn * p.K + gk) : zero;
}

template <int XPT>
__device__ __forceinline__ void lb_write(float* Xb, float* Wb, const Regs<XPT>& r) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < XPT; ++i) *(f32x4*)(Xb + ((t + NTH * i) >> 3) * LDR + (t & 7) * 4) = r.x[i];
  if (t < NS * 8) *(f32x4*)(Wb + (t >> 3) * LDR + (t & 7) * 4) = r.w;
}

template <int XPT>
__global__ __launch_bounds__(NTH) void lb_kernel(LP p) {
  constexpr int NI = XPT == 4 ? 2 : 1;          // row blocks per wave (XPT 1, 2: at most 4 blocks)
  static_assert(XPT * NTH / 8 <= MAXROWS, "the X image has 128 rows");
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, r16 = lane & 15, g = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * NS;
  const int MB = (p.M + 15) >> 4;
  f32x4 acc[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (int)((p.K + KT - 1) / KT);
  Regs<XPT> ring[RING];
#pragma unroll
  for (int d = 0; d < RING; ++d) lb_load(ring[d], p, n0, (int64_t)d * KT);     // past K: zeros, no access
  for (int kt0 = 0; kt0 < nk; kt0 += RING) {
#pragma unroll
    for (int d = 0; d < RING; ++d) {
      const int kt = kt0 + d;
      if (kt < nk) {
        // buffer kt & 1 was last read in step kt - 2, which every wave left before the barrier of kt - 1
        float* Xb = smem + (d & 1) * STAGE;
        float* Wb = Xb + MAXROWS * LDR;
        lb_write(Xb, Wb, ring[d]);
        lb_load(ring[d], p, n0, (int64_t)(kt + RING) * KT);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KT / 4; ++s) {       // k = 4 s + g: ascending
          const float b = Wb[r16 * LDR + 4 * s + g];
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            const int mb = w + 4 * i;
            if (mb < MB) {
              const float a = Xb[(mb * 16 + r16) * LDR + 4 * s + g];
              acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(b, a, acc[i], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  __syncthreads();                               // the last step's reads, before the images are reused
  // lane: row mb*16 + r16, features n0 + 4 g + [0, 4)
  float* Y = smem;                               // [MAXROWS][LDY]
  float* st_m = smem + MAXROWS * LDY;            // [G][NS] group mean
  float* st_v = st_m + MAXROWS * NS;             // [G][NS] group unbiased variance
  static_assert(MAXROWS * LDY + 2 * MAXROWS * NS <= 2 * STAGE, "the epilogue fits the operand images");
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int mb = w + 4 * i;
    if (mb < MB) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 4 * g + r;
        const float bv = (p.bias && n0 + f < p.N) ? p.bias[n0 + f] : 0.f;
        Y[(mb * 16 + r16) * LDY + f] = acc[i][r] + bv;
      }
    }
  }
  __syncthreads();
  const int R = p.R;
  for (int pair = t; pair < p.G * NS; pair += NTH) {
    const int f = pair & (NS - 1), grp = pair >> 4;
    const int64_t n = n0 + f;
    if (n >= p.N) continue;
    const float* y = Y + (grp * R) * LDY + f;
    float mean, var;
    if (p.use_running) {
      mean = p.rm[n];
      var = p.rv[n];
    } else {
      float s = 0.f;
      for (int r = 0; r < R; ++r) s += y[r * LDY];
      mean = s / (float)R;
      float q = 0.f;
      for (int r = 0; r < R; ++r) {
        const float dv = y[r * LDY] - mean;
        q += dv * dv;
      }
      var = q / (float)R;
      st_m[pair] = mean;
      st_v[pair] = q / (float)(R - 1);
    }
    const float rs = 1.f / sqrtf(var + p.eps);
    p.rstd[(int64_t)grp * p.N + n] = rs;
    const float ga = p.gamma ? p.gamma[n] : 1.f, be = p.gamma ? p.beta[n] : 0.f;
    for (int r = 0; r < R; ++r) {
      const int64_t o = (int64_t)(grp * R + r) * p.N + n;
      const float xh = (y[r * LDY] - mean) * rs;
      float v = ga * xh + be;
      if (p.relu) v = fmaxf(v, 0.f);
      p.xhat[o] = xh;
      p.out[o] = v;
    }
  }
  __syncthreads();
  if (!p.use_running && t < NS && n0 + t < p.N) {
    float m = p.rm[n0 + t], v = p.rv[n0 + t];
    for (int grp = 0; grp < p.G; ++grp) {        // what G successive BatchNorm1d calls leave
      m = (1.f - p.mom) * m + p.mom * st_m[grp * NS + t];
      v = (1.f - p.mom) * v + p.mom * st_v[grp * NS + t];
    }
    p.rm[n0 + t] = m;
    p.rv[n0 + t] = v;
  }
}

// ------------------------------------------------------------------ (b) BatchNorm (+ ReLU) backward
struct BP {
  const float* dout; const float* out; const float* xhat; const float* rstd; const float* gamma;
  int G, R;
  int64_t N;
  int relu, use_running;
  float* dy; float* dgamma; float* dbeta; float* dbias;
};

constexpr int BNTH = 64;

__global__ __launch_bounds__(BNTH) void bnb_kernel(BP p) {
  const int64_t n = (int64_t)blockIdx.x * BNTH + threadIdx.x;
  if (n >= p.N) return;
  const float ga = p.gamma ? p.gamma[n] : 1.f;
  const int R = p.R;
  const float fR = (float)R;
  float dg = 0.f, db = 0.f, dbi = 0.f;
  for (int grp = 0; grp < p.G; ++grp) {
    const float rs = p.rstd[(int64_t)grp * p.N + n];
    const int64_t base = (int64_t)grp * R * p.N + n;
    float s1 = 0.f, s2 = 0.f, sg = 0.f, sb = 0.f;
    for (int r = 0; r < R; ++r) {
      const int64_t o = base + (int64_t)r * p.N;
      float d = p.dout[o];
      if (p.relu && !(p.out[o] > 0.f)) d = 0.f;
      const float xh = p.xhat[o], dxh = d * ga;
      sb += d;
      sg += d * xh;
      s1 += dxh;
      s2 += dxh * xh;
    }
    const float c = rs / fR;
    float sdy = 0.f;
    for (int r = 0; r < R; ++r) {
      const int64_t o = base + (int64_t)r * p.N;
      float d = p.dout[o];
      if (p.relu && !(p.out[o] > 0.f)) d = 0.f;
      const float xh = p.xhat[o], dxh = d * ga;
      const float v = p.use_running ? dxh * rs : c * (fR * dxh - s1 - xh * s2);
      p.dy[o] = v;
      sdy += v;
    }
    dg += sg;
    db += sb;
    dbi += sdy;
  }
  if (p.dgamma) p.dgamma[n] = dg;
  if (p.dbeta) p.dbeta[n] = db;
  if (p.dbias) p.dbias[n] = dbi;
}

// ------------------------------------------------------------------ (c) SimSiam loss
constexpr int SS_MAX = 8192;

__global__ __launch_bounds__(NTH) void ss_row_kernel(const float* p1, const float* p2, const float* z1,
                                                     const float* z2, int B, int P, float* dp1, float* dp2,
                                                     float* ws) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;
  const float sc = -2.f / (float)B;
  float term = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {                  // (p1, z2), then (p2, z1)
    const float* pv = (q ? p2 : p1) + (int64_t)b * P;
    const float* zv = (q ? z1 : z2) + (int64_t)b * P;
    float* dp = (q ? dp2 : dp1) + (int64_t)b * P;
    float pp = 0.f, zz = 0.f, pz = 0.f;
    for (int k = lane; k < P; k += 64) {
      const float a = pv[k], c = zv[k];
      pp += a * a;
      zz += c * c;
      pz += a * c;
    }
    pp = warp_sum(pp);
    zz = warp_sum(zz);
    pz = warp_sum(pz);
    const float np = sqrtf(pp), nz = sqrtf(zz);
    const float ip = 1.f / fmaxf(np, 1e-12f), iz = 1.f / fmaxf(nz, 1e-12f);
    const float c = pz * ip * iz;
    term += 2.f - 2.f * c;
    // d cos / d p = ip (z iz - p ip cos); a clamped norm is a constant: the second term drops
    const float back = np > 1e-12f ? ip * c : 0.f;
    for (int k = lane; k < P; k += 64) dp[k] = sc * ip * (zv[k] * iz - pv[k] * back);
  }
  if (lane == 0) ws[b] = term;
}

__global__ __launch_bounds__(NTH) void ss_sum_kernel(const float* ws, int B, float* loss) {
  __shared__ float red[NTH / 64];
  float v = 0.f;
  for (int i = threadIdx.x; i < B; i += NTH) v += ws[i];
  v = block_sum(v, red);
  if (threadIdx.x == 0) loss[0] = v / (float)B;
}

}  // namespace

extern "C" int ctclip_ssl_linear_bn(const ctclip_ssl_linear_bn_args* a, void* stream) {
  CT_REQUIRE(a != nullptr, CT_EINVAL);
  CT_REQUIRE(a->G >= 1 && a->R >= 1 && a->K >= 1 && a->N >= 1, CT_ESHAPE);
  CT_REQUIRE((int64_t)a->G * a->R <= MAXROWS && a->K % 4 == 0, CT_ESHAPE);
  CT_REQUIRE(a->use_running || a->R >= 2, CT_ESHAPE);
  CT_REQUIRE(a->X && a->W && a->running_mean && a->running_var && a->out && a->xhat && a->rstd, CT_EINVAL);
  CT_REQUIRE((a->gamma == nullptr) == (a->beta == nullptr), CT_EINVAL);
  CT_REQUIRE(a->ldx >= a->K && a->ldx % 4 == 0 && aligned16(a->X) && aligned16(a->W), CT_EALIGN);
  LP p{a->X, a->ldx, a->W, a->bias, a->gamma, a->beta, a->running_mean, a->running_var,
       a->G, a->R, a->G * a->R, a->K, a->N, a->relu, a->use_running, a->eps, a->momentum,
       a->out, a->xhat, a->rstd};
  const dim3 grid((unsigned)cdiv(a->N, NS));
  const hipStream_t st = (hipStream_t)stream;
  if (p.M <= 32)
    hipLaunchKernelGGL(lb_kernel<1>, grid, dim3(NTH), 0, st, p);
  else if (p.M <= 64)
    hipLaunchKernelGGL(lb_kernel<2>, grid, dim3(NTH), 0, st, p);
  else
    hipLaunchKernelGGL(lb_kernel<4>, grid, dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_ssl_bn_bwd(const ctclip_ssl_bn_bwd_args* a, void* stream) {
  CT_REQUIRE(a != nullptr, CT_EINVAL);
  CT_REQUIRE(a->G >= 1 && a->R >= 1 && a->N >= 1 && (int64_t)a->G * a->R <= MAXROWS, CT_ESHAPE);
  CT_REQUIRE(a->use_running || a->R >= 2, CT_ESHAPE);
  CT_REQUIRE(a->dout && a->xhat && a->rstd && a->dy && (a->out || !a->relu), CT_EINVAL);
  BP p{a->dout, a->out, a->xhat, a->rstd, a->gamma, a->G, a->R, a->N, a->relu, a->use_running,
       a->dy, a->dgamma, a->dbeta, a->dbias};
  hipLaunchKernelGGL(bnb_kernel, dim3((unsigned)cdiv(a->N, BNTH)), dim3(BNTH), 0, (hipStream_t)stream, p);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_simsiam_loss(const float* p1, const float* p2, const float* z1, const float* z2, int32_t B,
                                   int32_t P, float* loss, float* dp1, float* dp2, float* ws, void* stream) {
  CT_REQUIRE(B >= 1 && B <= SS_MAX && P >= 1 && P <= SS_MAX, CT_ESHAPE);
  CT_REQUIRE(p1 && p2 && z1 && z2 && loss && dp1 && dp2 && ws, CT_EINVAL);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ss_row_kernel, dim3((unsigned)cdiv(B, 4)), dim3(NTH), 0, st, p1, p2, z1, z2, B, P, dp1, dp2, ws);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(ss_sum_kernel, dim3(1), dim3(NTH), 0, st, ws, B, loss);
  CT_CHECK_LAUNCH();
  return 0;
}
