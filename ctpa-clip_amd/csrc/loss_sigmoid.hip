// Pairwise sigmoid (SigLIP) contrastive loss (include/ctclip_hip.h, ctclip_sigmoid_loss; Zhai et al. 2023,
// "Sigmoid Loss for Language Image Pre-Training"): every (report i, volume j) pair of the global batch is
// an independent binary problem,
//   x_ij = exp(log_temp) <t^_i, i^_j> + bias,  z_ij = +1 (i = j) / -1,  L = 1/Bg sum_ij softplus(-z_ij x_ij),
// so nothing is normalised over the batch: no row or column sums, no waiting between workgroups.  Built as
// loss_tiled.hip is (its tile sizes, LDS images and MFMA operand maps), on the f32 matrix pipe
// (v_mfma_f32_16x16x4_f32, exact f32: each output is one fma chain in ascending k).  Four launches:
//   (a) sg_norm_kernel    both latent sets l2-normalised ONCE into the workspace (eps 1e-12), norms kept
//   (b) sg_logits_kernel  grid (column tile, row tile): s = t^ . i^T on MFMA; per element the loss term
//                         softplus(u), u = -z x, as max(u, 0) + log1p(exp(-|u|)), and g = dL/dx = -z sigmoid(u) / Bg
//                         from the same exp; G STORED; the tile's partial sums of loss, g and g s
//   (c) sg_grad_kernel    grid (Dl chunk, row tile, side): side 0 G . I^ for the requested text rows (G read
//                         along its rows), side 1 G^T . T^ for the requested image rows (along its columns);
//                         one MFMA chain per output over all Bg rows of the other side, ascending; times temp
//   (d) sg_finish_kernel  one wave per output row: the l2norm backward; the last workgroup folds the tile
//                         partials -- a tile row in ascending column-tile order, then the tile rows ascending --
//                         into loss, dbias = sum g and dlogtemp = temp sum g s
// G is stored, not recomputed: the gradient products then read one f32 per (i, j) instead of repeating the
// Bg x Bg x Dl logits product twice (5 products instead of 3 for all rows); the price is Bg x Bg floats of
// workspace (256 MiB at Bg = 8192, what the tiled InfoNCE loss keeps for exp(S) of one pair).
// Every sum has a fixed order that depends on neither the launch geometry of another row nor the requested
// row range: the logits pass always covers the whole matrix, a tile's partials are folded lane -> wave
// butterfly -> the four waves ascending, and a gradient row's chain runs over k = 0 .. Bg-1.  So two runs
// -- and a row asked for alone or inside 0..Bg -- give the same bits; the scalars are always global.
//
// Workspace (floats, every segment a multiple of 4; ldD = Dl rounded up to 4, ldG = Bg rounded up to 4,
// nT = ceil(Bg / 64)):
//   nv [2][Bg][ldD] normalised latents, text then image (pad columns zero) | nrm [2][Bg] |
//   G [Bg][ldG] (pad columns zero) | part [3][nT][nT] (loss, g, g s; [row tile][column tile])
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int MAXBG = 8192, MAXDL = 8192;
constexpr int TB = 64;            // rows / columns of a logits tile, rows of a gradient tile
constexpr int DC = 128;           // Dl chunk of a gradient tile
constexpr int KT = 16;            // K step
constexpr int LDR = 20;           // K-contiguous LDS image [row][16 k]: 16-B aligned rows, 64 lanes on 64 banks
constexpr int LDA = 80;           // row-contiguous LDS image [16 k][64 rows]: k groups 16 banks apart
constexpr int LDB = 144;          // row-contiguous LDS image [16 k][128 columns]
constexpr int NTH = 256;

struct Layout {
  int64_t ldD, ldG, nT;
  int64_t nv, nrm, G, part, total;
};

__host__ __device__ inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }

inline Layout make_layout(int Bg, int Dl) {
  Layout L;
  L.ldD = up4(Dl);
  L.ldG = up4(Bg);
  L.nT = (Bg + TB - 1) / TB;
  int64_t o = 0;
  L.nv = o;   o += 2 * (int64_t)Bg * L.ldD;
  L.nrm = o;  o += up4(2 * (int64_t)Bg);
  L.G = o;    o += (int64_t)Bg * L.ldG;
  L.part = o; o += up4(3 * L.nT * L.nT);
  L.total = o;
  return L;
}

struct SP {
  const float* t_raw; const float* i_raw; const float* log_temp; const float* bias;
  int Bg, Dl, row0, rows;
  float* loss; float* dt; float* di; float* dlogtemp; float* dbias;
  float* ws;
  Layout L;
};

// ------------------------------------------------------------------ (a) normalise: one wave per row
__global__ __launch_bounds__(NTH) void sg_norm_kernel(SP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;            // rows 0..Bg-1 text, Bg..2Bg-1 image
  if (r >= 2 * (int64_t)p.Bg) return;
  const float* src = (r < p.Bg ? p.t_raw + r * p.Dl : p.i_raw + (r - p.Bg) * p.Dl);
  float q = 0.f;
  for (int k = lane; k < p.Dl; k += 64) q += src[k] * src[k];
  q = warp_sum(q);
  const float nn = sqrtf(q);
  const float inv = 1.f / fmaxf(nn, 1e-12f);
  float* dst = p.ws + p.L.nv + r * p.L.ldD;
  for (int k = lane; k < (int)p.L.ldD; k += 64) dst[k] = k < p.Dl ? src[k] * inv : 0.f;
  if (lane == 0) p.ws[p.L.nrm + r] = nn;
}

// ------------------------------------------------------------------ (b) logits tile
// one 16-B chunk of a 64-row x 16-k K-contiguous tile: row t / 4, k quad t % 4 (rows of ldD floats,
// pad columns zero, so only the row and the padded width bound the load)
__device__ __forceinline__ f32x4 kload(const float* __restrict__ base, int64_t ld, int rows, int row0, int k0) {
  const int t = threadIdx.x, gr = row0 + (t >> 2), gk = k0 + (t & 3) * 4;
  return (gr < rows && gk < ld) ? *(const f32x4*)(base + (int64_t)gr * ld + gk) : f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void kwrite(float* img, const f32x4& r) {
  const int t = threadIdx.x;
  *(f32x4*)(img + (t >> 2) * LDR + (t & 3) * 4) = r;
}

__global__ __launch_bounds__(NTH) void sg_logits_kernel(SP p) {
  __shared__ __attribute__((aligned(16))) float smem[4 * TB * LDR];   // [buf][A | B]
  __shared__ float Gs[TB][TB + 1];
  __shared__ float red[3][NTH / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  const int i0 = blockIdx.y * TB, j0 = blockIdx.x * TB, Bg = p.Bg;
  const int64_t ldD = p.L.ldD, ldG = p.L.ldG;
  const float* A = p.ws + p.L.nv;                          // text
  const float* B = A + (int64_t)Bg * ldD;                  // image
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (int)((ldD + KT - 1) / KT);
  f32x4 ra = kload(A, ldD, Bg, i0, 0), rb = kload(B, ldD, Bg, j0, 0);
  kwrite(smem, ra);
  kwrite(smem + TB * LDR, rb);
  __syncthreads();
  const int r16 = lane & 15, g = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const float* As = smem + (kt & 1) * 2 * TB * LDR;
    const float* Bs = As + TB * LDR;
    if (kt + 1 < nk) {
      ra = kload(A, ldD, Bg, i0, (kt + 1) * KT);
      rb = kload(B, ldD, Bg, j0, (kt + 1) * KT);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {          // k = 4 s + g, ascending
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = As[(wm * 32 + i * 16 + r16) * LDR + 4 * s + g];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = Bs[(wn * 32 + j * 16 + r16) * LDR + 4 * s + g];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j], a[i], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      float* nb = smem + ((kt + 1) & 1) * 2 * TB * LDR;
      kwrite(nb, ra);
      kwrite(nb + TB * LDR, rb);
    }
    __syncthreads();
  }
  // lane: tile row wm*32 + 16 i + r16, tile columns wn*32 + 16 j + 4 g + [0, 4)
  const float temp = expf(p.log_temp[0]), bias = p.bias[0], invB = 1.f / (float)Bg;
  float sl = 0.f, sg = 0.f, sgs = 0.f;     // this lane's 16 elements, ascending (i, j, r)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tr = wm * 32 + i * 16 + r16, tc = wn * 32 + j * 16 + 4 * g + r;
        const bool ok = i0 + tr < Bg && j0 + tc < Bg;
        const float s = acc[i][j][r];
        const float x = fmaf(temp, s, bias);
        const bool pos = i0 + tr == j0 + tc;
        const float u = pos ? -x : x;                       // -z x
        const float e = expf(-fabsf(u));                    // in (0, 1]: no overflow on either sign
        const float l = fmaxf(u, 0.f) + log1pf(e);
        const float sig = (u >= 0.f ? 1.f : e) / (1.f + e); // sigmoid(u)
        const float gv = ok ? (pos ? -sig : sig) * invB : 0.f;
        Gs[tr][tc] = gv;
        sl += ok ? l : 0.f;
        sg += gv;
        sgs += gv * s;
      }
  sl = warp_sum(sl);
  sg = warp_sum(sg);
  sgs = warp_sum(sgs);
  if (lane == 0) { red[0][w] = sl; red[1][w] = sg; red[2][w] = sgs; }
  __syncthreads();
  float* G = p.ws + p.L.G;
  for (int e = threadIdx.x; e < TB * TB; e += NTH) {
    const int tr = e >> 6, tc = e & 63;
    if (i0 + tr < Bg && j0 + tc < ldG) G[(int64_t)(i0 + tr) * ldG + j0 + tc] = Gs[tr][tc];
  }
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    float v = 0.f;
    for (int k = 0; k < NTH / 64; ++k) v += red[q][k];
    p.ws[p.L.part + ((int64_t)q * p.L.nT + blockIdx.y) * p.L.nT + blockIdx.x] = q == 0 ? v * invB : v;
  }
}

// ------------------------------------------------------------------ (c) gradient tile
// out[row][d] = temp sum_k g(row, k) other[k][d] over all Bg rows k of the other side.  TEXT: the output rows
// are text rows i, G is read along its rows (K-contiguous); otherwise they are image rows j and G is read
// along its columns (row-contiguous).
template <bool TEXT>
__device__ __forceinline__ void grad_tile(const SP& p, float* smem) {
  constexpr int A_FLOATS = TEXT ? TB * LDR : KT * LDA, B_FLOATS = KT * LDB;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int Bg = p.Bg;
  const int r0 = p.row0 + blockIdx.y * TB, d0 = blockIdx.x * DC;
  const int rend = p.row0 + p.rows;
  const int64_t ldD = p.L.ldD, ldG = p.L.ldG;
  const float* G = p.ws + p.L.G;
  const float* O = p.ws + p.L.nv + (TEXT ? (int64_t)Bg * ldD : 0);    // the other side's normalised latents
  const int steps = (Bg + KT - 1) / KT;
  // this thread's 4 G elements of a step: TEXT row t / 4, k = 4 (t % 4) + e; else row t % 64, k = t / 64 + 4 e
  const int am = TEXT ? t >> 2 : t & 63;
  const int grow = r0 + am;                            // the output row (text row i / image row j)
  const bool rowok = grow < Bg;
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  float ga[4];
  f32x4 rb[2];
  auto gload = [&](int step) {
    const int k0 = step * KT;
    if (TEXT) {
      const int gk = k0 + (t & 3) * 4;
      // the pad columns of G are zero and ldG bounds the 16-B load
      const f32x4 g4 = (rowok && gk < ldG) ? *(const f32x4*)(G + (int64_t)grow * ldG + gk) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) ga[e] = g4[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int gk = k0 + (t >> 6) + 4 * e;
        ga[e] = (rowok && gk < Bg) ? G[(int64_t)gk * ldG + grow] : 0.f;
      }
    }
    // rows k0 + t / 32 + 8 i, columns d0 + 4 (t % 32)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int gk = k0 + (t >> 5) + 8 * i, gd = d0 + (t & 31) * 4;
      rb[i] = (gk < Bg && gd < ldD) ? *(const f32x4*)(O + (int64_t)gk * ldD + gd) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto swrite = [&](float* As, float* Bs) {
    if (TEXT) {
      *(f32x4*)(As + (t >> 2) * LDR + (t & 3) * 4) = f32x4{ga[0], ga[1], ga[2], ga[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) As[((t >> 6) + 4 * e) * LDA + (t & 63)] = ga[e];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) *(f32x4*)(Bs + ((t >> 5) + 8 * i) * LDB + (t & 31) * 4) = rb[i];
  };

  gload(0);
  swrite(smem, smem + A_FLOATS);
  __syncthreads();
  const int r16 = lane & 15, g = lane >> 4;
  for (int st = 0; st < steps; ++st) {
    const float* As = smem + (st & 1) * (A_FLOATS + B_FLOATS);
    const float* Bs = As + A_FLOATS;
    if (st + 1 < steps) gload(st + 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float a[2], b[4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        a[i] = TEXT ? As[(wm * 32 + i * 16 + r16) * LDR + 4 * s + g] : As[(4 * s + g) * LDA + wm * 32 + i * 16 + r16];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Bs[(4 * s + g) * LDB + wn * 64 + j * 16 + r16];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j], a[i], acc[i][j], 0, 0, 0);
    }
    if (st + 1 < steps) {
      float* nb = smem + ((st + 1) & 1) * (A_FLOATS + B_FLOATS);
      swrite(nb, nb + A_FLOATS);
    }
    __syncthreads();
  }
  // lane: tile row wm*32 + 16 i + r16, columns d0 + wn*64 + 16 j + 4 g + [0, 4); the gradient w.r.t. the
  // normalised latent, finished by sg_finish_kernel
  const float temp = expf(p.log_temp[0]);
  float* out = TEXT ? p.dt : p.di;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int gr = r0 + wm * 32 + i * 16 + r16;
    if (gr >= rend) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gd = d0 + wn * 64 + j * 16 + 4 * g + r;
        if (gd < p.Dl) out[(int64_t)(gr - p.row0) * p.Dl + gd] = temp * acc[i][j][r];
      }
  }
}

__global__ __launch_bounds__(NTH) void sg_grad_kernel(SP p) {
  // both sides' images have the same size: [64][LDR] / [16][LDA] floats of G plus [16][LDB] of latents, twice
  static_assert(TB * LDR == KT * LDA, "one LDS buffer serves both sides");
  __shared__ __attribute__((aligned(16))) float smem[2 * (TB * LDR + KT * LDB)];
  if (blockIdx.z == 0) grad_tile<true>(p, smem);
  else grad_tile<false>(p, smem);
}

// ------------------------------------------------------------------ (d) l2norm backward, final scalars
__global__ __launch_bounds__(NTH) void sg_finish_kernel(SP p) {
  __shared__ float rowsum[3][(MAXBG + TB - 1) / TB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (blockIdx.x + 1 < gridDim.x) {
    const int64_t r = (int64_t)blockIdx.x * 4 + w;          // rows 0..rows-1 text, rows..2 rows-1 image
    if (r >= 2 * (int64_t)p.rows) return;
    const int side = r >= p.rows, lr = (int)(r - (int64_t)side * p.rows);
    const int64_t grow = (int64_t)side * p.Bg + p.row0 + lr;
    const float* self = p.ws + p.L.nv + grow * p.L.ldD;
    const float nn = p.ws[p.L.nrm + grow];
    float* out = (side ? p.di : p.dt) + (int64_t)lr * p.Dl;
    float dotp = 0.f;
    for (int k = lane; k < p.Dl; k += 64) dotp += out[k] * self[k];
    dotp = warp_sum(dotp);
    const float inv = 1.f / fmaxf(nn, 1e-12f);
    for (int k = lane; k < p.Dl; k += 64) {
      const float gq = out[k];
      out[k] = nn > 1e-12f ? (gq - self[k] * dotp) * inv : gq * inv;
    }
    return;
  }
  // the last workgroup: thread (q, row tile) folds its tile row in ascending column-tile order, then one
  // thread per scalar folds the tile rows in ascending order
  const int nT = (int)p.L.nT;
  for (int e = threadIdx.x; e < 3 * nT; e += NTH) {
    const int q = e / nT, ti = e - q * nT;
    const float* src = p.ws + p.L.part + ((int64_t)q * nT + ti) * nT;
    float v = 0.f;
    for (int tj = 0; tj < nT; ++tj) v += src[tj];
    rowsum[q][ti] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    float v = 0.f;
    for (int ti = 0; ti < nT; ++ti) v += rowsum[q][ti];
    if (q == 0) p.loss[0] = v;
    else if (q == 1) p.dbias[0] = v;
    else p.dlogtemp[0] = expf(p.log_temp[0]) * v;
  }
}

bool shape_ok(const ctclip_sigmoid_loss_args* a) {
  return a->Bg >= 1 && a->Bg <= MAXBG && a->Dl >= 1 && a->Dl <= MAXDL;
}

}  // namespace

extern "C" int64_t ctclip_sigmoid_loss_ws_bytes(const ctclip_sigmoid_loss_args* a) {
  if (!a || !shape_ok(a)) return 0;
  return 4 * make_layout(a->Bg, a->Dl).total;
}

extern "C" int ctclip_sigmoid_loss(const ctclip_sigmoid_loss_args* a, void* stream) {
  CT_REQUIRE(a != nullptr, CT_EINVAL);
  CT_REQUIRE(shape_ok(a), CT_ESHAPE);
  CT_REQUIRE(a->t_raw && a->i_raw && a->log_temp && a->bias && a->loss && a->dt_raw && a->di_raw && a->dlogtemp &&
                 a->dbias && a->ws,
             CT_EINVAL);
  CT_REQUIRE(a->grad_row0 >= 0 && a->grad_rows >= 1 && (int64_t)a->grad_row0 + a->grad_rows <= a->Bg, CT_EINVAL);
  CT_REQUIRE(aligned16(a->ws), CT_EALIGN);
  SP p;
  p.t_raw = a->t_raw; p.i_raw = a->i_raw; p.log_temp = a->log_temp; p.bias = a->bias;
  p.Bg = a->Bg; p.Dl = a->Dl; p.row0 = a->grad_row0; p.rows = a->grad_rows;
  p.loss = a->loss; p.dt = a->dt_raw; p.di = a->di_raw; p.dlogtemp = a->dlogtemp; p.dbias = a->dbias;
  p.ws = a->ws;
  p.L = make_layout(a->Bg, a->Dl);
  CT_REQUIRE(a->ws_bytes >= 4 * p.L.total, CT_EINVAL);
  const hipStream_t st = (hipStream_t)stream;
  const int nT = (int)p.L.nT;
  hipLaunchKernelGGL(sg_norm_kernel, dim3((unsigned)cdiv(2 * (int64_t)p.Bg, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(sg_logits_kernel, dim3(nT, nT), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(sg_grad_kernel, dim3(cdiv(p.Dl, DC), cdiv(p.rows, TB), 2), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(sg_finish_kernel, dim3((unsigned)cdiv(2 * (int64_t)p.rows, 4) + 1), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  return 0;
}
