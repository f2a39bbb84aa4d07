// Linear-probe head (include/ctclip_hip.h, ctclip_probe_step): multi-label logistic regression over frozen
// f32 latents -- BCE-with-logits (torch's stable pos_weight formula) forward and gradient in ONE pass over X.
//   z = x . w^T + b,  L = 1 + (pw - 1) y,  l = (1 - y) z + L (max(-z, 0) + log1p(exp(-|z|)))
//   r = (1 - y) - L (1 - sigmoid(z)),  loss = sum l / count,  dW = r^T X / count,  db = sum_rows r / count
// over the counted entries (y != 255 of a row the step runs over).
//
// Two plain launches, no float atomics, nothing waits on another workgroup:
//   (a) probe_tile_kernel  a workgroup (4 waves) walks the 32-row tiles  blockIdx.x, + gridDim.x, ...  in that
//       order.  A tile is loaded ONCE into LDS (rows through idx when given, 16-B loads, rows padded by 4
//       floats).  Phase 1: Z = X W^T on v_mfma_f32_16x16x4_f32 with W held in REGISTERS for the whole kernel --
//       wave w owns the 16-column chunks w, w + 4, ... of D, so the four waves read every LDS element of the
//       tile once (ds_read_b128) and leave four K-partials, folded in wave order.  Epilogue: 4 logits per
//       thread -> loss term, residual r into LDS, Z to memory only when asked for.  Phase 2: dW += r^T X from
//       the SAME resident tile, wave w owning the same column chunks, so dW stays in accumulators across all
//       tiles of the workgroup.  At the end the workgroup writes one slab [dW | db | loss | count].
//   (b) probe_reduce_kernel  slabs summed in a fixed order (four ascending runs, then their sum), divided by the
//       integer count.  r is scaled HERE, once per output, not per entry: the count needs no pass of its own.
// The grid is a function of M alone (min(256, ceil(tiles / 2))), so two runs give the same bits.
// P is padded to 16 / 32 in registers (zero W rows), never in memory.
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int RT = 32;            // rows of a tile
constexpr int PP = 32;            // padded label count of the LDS images
constexpr int ZLD = 36;           // row stride of the logit partials / residual images
constexpr int NTH = 256;
constexpr int MAXGRID = 256;      // one workgroup per CU at most: the slab traffic stays small beside X
constexpr int RED_COLS = 64, RED_RUNS = 4;

struct PP_ {
  const float* X; int64_t ldx, N;
  const int32_t* idx;
  int M, D, P;
  const float* W; const float* b; const uint8_t* Y; const float* pw;
  float* loss; float* dW; float* db; float* Z; int32_t* count;
  float* ws;
  int64_t SL;                     // floats of a slab
  int ntiles, grid, grad, stats;
};

__host__ __device__ inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }
inline int64_t slab_floats(int D, int P) { return up4((int64_t)P * D + P + 2); }
inline int grid_for(int M) {
  const int nt = cdiv(M, RT);
  return std::max(1, std::min(MAXGRID, (nt + 1) / 2));
}
inline size_t lds_bytes(int D) { return sizeof(float) * ((size_t)RT * (D + 4) + 5 * RT * ZLD + RT + 8); }

template <int PT, int JMAX>
__global__ __launch_bounds__(NTH) void probe_tile_kernel(PP_ p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = p.D, P = p.P, ld = D + 4, nc = D >> 4;
  float* Xs = smem;                           // [32][ld]
  float* Zp = Xs + RT * ld;                   // [4 waves][32][ZLD]
  float* Rs = Zp + 4 * RT * ZLD;              // [32][ZLD]
  int* srow = (int*)(Rs + RT * ZLD);          // [32] source row of each tile row, -1: none
  float* red = (float*)(srow + RT);           // [8]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, r16 = lane & 15, g = lane >> 4;

  // W in registers: chunk c = w + 4 jj, label 16 pt + r16, columns 16 c + 4 g + [0, 4)
  f32x4 wreg[PT][JMAX];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int jj = 0; jj < JMAX; ++jj) {
      const int c = w + 4 * jj, prow = 16 * pt + r16;
      wreg[pt][jj] = (c < nc && prow < P) ? *(const f32x4*)(p.W + (int64_t)prow * D + 16 * c + 4 * g)
                                          : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  f32x4 dacc[PT][JMAX];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int jj = 0; jj < JMAX; ++jj) dacc[pt][jj] = f32x4{0.f, 0.f, 0.f, 0.f};

  // epilogue ownership: tile row t / 8, labels 4 (t % 8) + [0, 4)
  const int erow = t >> 3, ep0 = (t & 7) * 4;
  float eb[4], epw[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = ep0 + e;
    eb[e] = q < P ? p.b[q] : 0.f;
    epw[e] = (q < P && p.pw) ? p.pw[q] : 1.f;
  }
  float lossacc = 0.f, dbacc = 0.f;
  int cntacc = 0;

  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int m0 = tile * RT;
    if (t < RT) {
      const int m = m0 + t;
      int64_t src = -1;
      if (m < p.M) src = p.idx ? (int64_t)p.idx[m] : (int64_t)m;
      srow[t] = (src >= 0 && src < p.N) ? (int)src : -1;
    }
    __syncthreads();
    // the tile, once: wave w loads rows 8 w + [0, 8), LB rows' 16-B loads in flight per lane before the
    // first LDS store (one load latency per batch, not per row)
    constexpr int LB = JMAX == 16 ? 4 : 8;
    for (int c4 = lane; c4 < (D >> 2); c4 += 64)
#pragma unroll
      for (int r0 = 0; r0 < 8; r0 += LB) {
        f32x4 v[LB];
#pragma unroll
        for (int rr = 0; rr < LB; ++rr) {
          const int src = srow[w * 8 + r0 + rr];
          v[rr] = src >= 0 ? *(const f32x4*)(p.X + (int64_t)src * p.ldx + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int rr = 0; rr < LB; ++rr) *(f32x4*)(Xs + (w * 8 + r0 + rr) * ld + 4 * c4) = v[rr];
      }
    __syncthreads();

    // ---- phase 1: this wave's K-partial of Z [32][16 PT]
    f32x4 acc[2][PT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) acc[rt][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < JMAX; ++jj) {
      const int c = w + 4 * jj;
      if (c < nc) {
        f32x4 xa[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) xa[rt] = *(const f32x4*)(Xs + (rt * 16 + r16) * ld + 16 * c + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int pt = 0; pt < PT; ++pt)
              acc[rt][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[pt][jj][e], xa[rt][e], acc[rt][pt], 0, 0, 0);
      }
    }
    // lane: tile row 16 rt + r16, labels 16 pt + 4 g + [0, 4)
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) *(f32x4*)(Zp + (w * RT + rt * 16 + r16) * ZLD + 16 * pt + 4 * g) = acc[rt][pt];
    __syncthreads();

    // ---- epilogue: logits, loss terms, residuals
    {
      const int m = m0 + erow, src = srow[erow];
      f32x4 zo = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ep0 < 16 * PT) {
        const f32x4 z0 = *(const f32x4*)(Zp + (0 * RT + erow) * ZLD + ep0);
        const f32x4 z1 = *(const f32x4*)(Zp + (1 * RT + erow) * ZLD + ep0);
        const f32x4 z2 = *(const f32x4*)(Zp + (2 * RT + erow) * ZLD + ep0);
        const f32x4 z3 = *(const f32x4*)(Zp + (3 * RT + erow) * ZLD + ep0);
        zo = ((z0 + z1) + z2) + z3;
      }
      f32x4 rv = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = ep0 + e;
        const float z = zo[e] + eb[e];
        if (q < P && m < p.M) {
          if (p.Z) p.Z[(int64_t)m * P + q] = z;
          if (p.stats && src >= 0) {
            const unsigned yy = p.Y[(int64_t)src * P + q];
            if (yy != 255u) {
              const float y = yy ? 1.f : 0.f;
              const float L = 1.f + (epw[e] - 1.f) * y;
              const float ex = expf(-fabsf(z));
              const float sp = fmaxf(-z, 0.f) + log1pf(ex);          // softplus(-z)
              const float s = 1.f / (1.f + ex);
              const float sneg = z >= 0.f ? ex * s : s;              // 1 - sigmoid(z)
              lossacc += (1.f - y) * z + L * sp;
              rv[e] = (1.f - y) - L * sneg;
              ++cntacc;
            }
          }
        }
      }
      *(f32x4*)(Rs + erow * ZLD + ep0) = rv;
    }
    __syncthreads();

    if (p.stats) {
      if (t < PP) {
        float s = 0.f;
        for (int row = 0; row < RT; ++row) s += Rs[row * ZLD + t];
        dbacc += s;
      }
      if (p.grad) {
        // ---- phase 2: dW [16 PT][this wave's chunks] += r^T X, K = the tile's 32 rows ascending
        float ra[PT][8];
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
          for (int s = 0; s < 8; ++s) ra[pt][s] = Rs[(4 * s + g) * ZLD + 16 * pt + r16];
#pragma unroll
        for (int jj = 0; jj < JMAX; ++jj) {
          const int c = w + 4 * jj;
          if (c < nc) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
              const float xb = Xs[(4 * s + g) * ld + 16 * c + r16];
#pragma unroll
              for (int pt = 0; pt < PT; ++pt)
                dacc[pt][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[pt][s], xb, dacc[pt][jj], 0, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();
  }

  if (!p.stats) return;
  float* slab = p.ws + (int64_t)blockIdx.x * p.SL;
  const int64_t PD = (int64_t)P * D;
  if (p.grad) {
    // lane: label 16 pt + 4 g + r, column 16 c + r16
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
      for (int jj = 0; jj < JMAX; ++jj) {
        const int c = w + 4 * jj;
        if (c < nc) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int q = 16 * pt + 4 * g + r;
            if (q < P) slab[(int64_t)q * D + 16 * c + r16] = dacc[pt][jj][r];
          }
        }
      }
  }
  if (t < P) slab[PD + t] = dbacc;
  const float ltot = block_sum(lossacc, red);
  // the count: integers, so any order gives the same sum
  int cw = cntacc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cw += __shfl_xor(cw, o, 64);
  int* redi = (int*)red + 4;
  __syncthreads();
  if (lane == 0) redi[w] = cw;
  __syncthreads();
  if (t == 0) {
    slab[PD + P] = ltot;
    ((int*)slab)[PD + P + 1] = redi[0] + redi[1] + redi[2] + redi[3];
  }
}

// out[i] = (sum over the slabs of element i) / count.  Block = 64 elements x 4 runs of slabs: run q sums slabs
// [q S, (q + 1) S), S = ceil(nslab / 4), ascending; the four runs are then added in order.
__global__ __launch_bounds__(RED_COLS* RED_RUNS) void probe_reduce_kernel(PP_ p) {
  __shared__ float part[RED_RUNS][RED_COLS];
  __shared__ int cnt_s;
  const int x = threadIdx.x & (RED_COLS - 1), q = threadIdx.x / RED_COLS;
  const int64_t PD = (int64_t)p.P * p.D, E = PD + p.P + 1, i = (int64_t)blockIdx.x * RED_COLS + x;
  const int G = p.grid;
  if (threadIdx.x == 0) {
    int c = 0;
    for (int s = 0; s < G; ++s) c += ((const int*)(p.ws + (int64_t)s * p.SL))[PD + p.P + 1];
    cnt_s = c;
  }
  float* dst = nullptr;
  if (i < PD) dst = p.dW ? p.dW + i : nullptr;
  else if (i < PD + p.P) dst = p.db ? p.db + (i - PD) : nullptr;
  else if (i < E) dst = p.loss;
  const int S = (G + RED_RUNS - 1) / RED_RUNS, s0 = q * S, s1 = min(G, s0 + S);
  float a = 0.f;
  if (dst)
    for (int s = s0; s < s1; ++s) a += p.ws[(int64_t)s * p.SL + i];
  part[q][x] = a;
  __syncthreads();
  if (q == 0 && dst) {
    const float tot = ((part[0][x] + part[1][x]) + part[2][x]) + part[3][x];
    dst[0] = cnt_s > 0 ? tot / (float)cnt_s : 0.f;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && p.count) p.count[0] = cnt_s;
}

bool shape_ok(const ctclip_probe_args* a) {
  return a->P >= 1 && a->P <= 32 && a->D >= 16 && a->D <= 1024 && a->D % 16 == 0 && a->M >= 1 && a->N >= 1 &&
         a->ldx >= a->D;
}

template <int PT, int JMAX>
int launch_tile(const PP_& p, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)probe_tile_kernel<PT, JMAX>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL((probe_tile_kernel<PT, JMAX>), dim3(p.grid), dim3(NTH), lds_bytes(p.D), st, p);
  CT_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int64_t ctclip_probe_step_ws_bytes(const ctclip_probe_args* a) {
  if (!a || !shape_ok(a)) return 0;
  return 4 * slab_floats(a->D, a->P) * grid_for(a->M);
}

extern "C" int ctclip_probe_step(const ctclip_probe_args* a, void* stream) {
  CT_REQUIRE(a != nullptr, CT_EINVAL);
  CT_REQUIRE(shape_ok(a), CT_ESHAPE);
  CT_REQUIRE(a->X && a->W && a->b, CT_EINVAL);
  CT_REQUIRE(a->idx || (int64_t)a->M == a->N, CT_EINVAL);
  const bool stats = a->loss || a->dW || a->db || a->count;
  CT_REQUIRE(stats || a->Z, CT_EINVAL);
  CT_REQUIRE(!stats || a->Y, CT_EINVAL);
  CT_REQUIRE(aligned16(a->X) && a->ldx % 4 == 0 && aligned16(a->W), CT_EALIGN);
  PP_ p;
  p.X = a->X; p.ldx = a->ldx; p.N = a->N; p.idx = a->idx; p.M = a->M; p.D = a->D; p.P = a->P;
  p.W = a->W; p.b = a->b; p.Y = a->Y; p.pw = a->pos_weight;
  p.loss = a->loss; p.dW = a->dW; p.db = a->db; p.Z = a->Z; p.count = a->count;
  p.ws = (float*)a->ws;
  p.SL = slab_floats(a->D, a->P);
  p.ntiles = cdiv(a->M, RT);
  p.grid = grid_for(a->M);
  p.grad = a->dW != nullptr;
  p.stats = stats;
  if (stats) {
    CT_REQUIRE(a->ws && a->ws_bytes >= 4 * p.SL * p.grid, CT_EINVAL);
    CT_REQUIRE(aligned16(a->ws), CT_EALIGN);
  }
  const hipStream_t st = (hipStream_t)stream;
  const int pt = a->P <= 16 ? 1 : 2, jm = a->D <= 256 ? 4 : a->D <= 512 ? 8 : 16;
  int rc;
  if (pt == 1) rc = jm == 4 ? launch_tile<1, 4>(p, st) : jm == 8 ? launch_tile<1, 8>(p, st) : launch_tile<1, 16>(p, st);
  else rc = jm == 4 ? launch_tile<2, 4>(p, st) : jm == 8 ? launch_tile<2, 8>(p, st) : launch_tile<2, 16>(p, st);
  if (rc) return rc;
  if (stats) {
    const int64_t E = (int64_t)a->P * a->D + a->P + 1;
    hipLaunchKernelGGL(probe_reduce_kernel, dim3((unsigned)cdiv(E, RED_COLS)), dim3(RED_COLS * RED_RUNS), 0, st, p);
    CT_CHECK_LAUNCH();
  }
  return 0;
}
