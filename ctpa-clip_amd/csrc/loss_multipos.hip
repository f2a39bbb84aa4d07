// Multi-positive (duplicate-report-aware) InfoNCE loss (include/ctclip_hip.h, ctclip_multipos_loss; DESIGN.md
// section 34): the positives of global row i are all rows of its group, P_i = { j : ids_j == ids_i }, n_i = |P_i|,
//   x_ij = exp(log_temp) <t^_i, i^_j>,
//   L = 1/2Bg [ sum_i (lse_j x_ij - 1/n_i sum_{j in P_i} x_ij) + sum_j (lse_i x_ij - 1/n_j sum_{i in P_j} x_ij) ],
//   dL/dx_ij = 1/2Bg [ exp(x_ij - lse_row_i) + exp(x_ij - lse_col_j) - [ids_i == ids_j] (1/n_i + 1/n_j) ],
// InfoNCE when all ids differ.  Every logsumexp is carried as (max, sum exp(x - max)), so the loss and its
// gradients are finite for any temperature.  Built as loss_tiled.hip and loss_sigmoid.hip are (their tile sizes,
// LDS images and MFMA operand maps), on the f32 matrix pipe (v_mfma_f32_16x16x4_f32, exact f32: each output is
// one fma chain in ascending k).  Six launches, none waiting on another workgroup:
//   (a) mp_norm_kernel    both latent sets l2-normalised ONCE into the workspace (eps 1e-12), norms kept
//   (b) mp_logits_kernel  grid (column tile, row tile): x = temp t^ . i^T on MFMA, STORED; from the tile in LDS
//                         (with the tile's 64 row ids and 64 column ids) the partials of its 64 rows and of its
//                         64 columns: (max, sum exp(x - max)), sum_{P} x and the count of equal ids
//   (c) mp_merge_kernel   one thread per row and per column: the partials merged in ascending tile order into
//                         lse, n, and the row's / column's loss term lse - (sum_P x) / n
//   (d) mp_g_kernel       grid (column tile, row tile): x overwritten IN PLACE by g = dL/dx; the tile's sum g x
//   (e) mp_grad_kernel    grid (Dl chunk, row tile, side): side 0 G . I^ for the requested text rows, side 1
//                         G^T . T^ for the requested image rows; one MFMA chain per output over all Bg rows of
//                         the other side, ascending; times temp
//   (f) mp_finish_kernel  one wave per output row: the l2norm backward; the last workgroup folds the loss terms,
//                         the counts and the tile sums into loss, npos and dlogtemp = sum g x
// G is stored (as loss_sigmoid.hip does), over the logits it was made from: the gradient products then read
// one f32 per (i, j) and are the sigmoid loss's pass verbatim; forming g while the gradient pass loads x would
// save one Bg x Bg read and write but cost two exponentials per element and Dl chunk, inside the MFMA loop.
// Every sum has a fixed order that depends on neither the launch geometry of another row nor the requested
// row range: passes (a)-(d) always cover the whole matrix; a tile row's / column's partial is two ascending
// 32-element halves merged low then high; tiles merge ascending; a tile's sum g x is folded lane -> wave
// butterfly -> the four waves ascending; a gradient row's chain runs over k = 0 .. Bg-1.  So two runs -- and
// a row asked for alone or inside 0..Bg -- give the same bits; the scalars are always global.
//
// Workspace (floats, every segment a multiple of 4; ldD = Dl rounded up to 4, ldG = Bg rounded up to 4,
// nT = ceil(Bg / 64), Bp = 64 nT):
//   nv [2][Bg][ldD] normalised latents, text then image (pad columns zero) | nrm [2][Bg] |
//   X [Bg][ldG] logits, then G (pad columns zero) | rp [4][nT][Bp] row partials (max, sum, sum_P x, count;
//   [column tile][row]) | cp [4][nT][Bp] column partials ([row tile][column]) |
//   st [6][Bp] (lse_row, lse_col, term_row, term_col, 1 / n, n) | part [nT][nT] (sum g x; [row tile][column tile])
//
// ctclip_report_ids (same header) hashes each report's kept tokens into the id, one wave per report.
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
enum { ST_LSER = 0, ST_LSEC, ST_TERMR, ST_TERMC, ST_INVN, ST_N, ST_COUNT };

struct Layout {
  int64_t ldD, ldG, nT, Bp;
  int64_t nv, nrm, X, rp, cp, st, part, total;
};

__host__ __device__ inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }

inline Layout make_layout(int Bg, int Dl) {
  Layout L;
  L.ldD = up4(Dl);
  L.ldG = up4(Bg);
  L.nT = (Bg + TB - 1) / TB;
  L.Bp = L.nT * TB;
  int64_t o = 0;
  L.nv = o;   o += 2 * (int64_t)Bg * L.ldD;
  L.nrm = o;  o += up4(2 * (int64_t)Bg);
  L.X = o;    o += (int64_t)Bg * L.ldG;
  L.rp = o;   o += 4 * L.nT * L.Bp;
  L.cp = o;   o += 4 * L.nT * L.Bp;
  L.st = o;   o += ST_COUNT * L.Bp;
  L.part = o; o += up4(L.nT * L.nT);
  L.total = o;
  return L;
}

struct MP {
  const float* t_raw; const float* i_raw; const long long* ids; const float* log_temp;
  int Bg, Dl, row0, rows;
  float* loss; float* dt; float* di; float* dlogtemp; int* npos;
  float* ws;
  Layout L;
};

// ------------------------------------------------------------------ (a) normalise: one wave per row
__global__ __launch_bounds__(NTH) void mp_norm_kernel(MP p) {
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

__global__ __launch_bounds__(NTH) void mp_logits_kernel(MP p) {
  __shared__ __attribute__((aligned(16))) float smem[4 * TB * LDR];   // [buf][A | B]
  __shared__ float Xs[TB][TB + 1];
  __shared__ long long ids_s[2][TB];                                  // the tile's row ids, column ids
  __shared__ float hp[2][2][TB][4];                                   // [side][half][row / column][quantity]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  const int i0 = blockIdx.y * TB, j0 = blockIdx.x * TB, Bg = p.Bg;
  const int64_t ldD = p.L.ldD, ldG = p.L.ldG;
  const float* A = p.ws + p.L.nv;                          // text
  const float* B = A + (int64_t)Bg * ldD;                  // image
  if (threadIdx.x < 2 * TB) {
    const int side = threadIdx.x >> 6, g = (side ? j0 : i0) + lane;
    ids_s[side][lane] = g < Bg ? p.ids[g] : 0;
  }
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
  const float temp = expf(p.log_temp[0]);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Xs[wm * 32 + i * 16 + r16][wn * 32 + j * 16 + 4 * g + r] = temp * acc[i][j][r];
  __syncthreads();
  float* X = p.ws + p.L.X;
  for (int e = threadIdx.x; e < TB * TB; e += NTH) {
    const int tr = e >> 6, tc = e & 63;
    if (i0 + tr < Bg && j0 + tc < ldG) X[(int64_t)(i0 + tr) * ldG + j0 + tc] = j0 + tc < Bg ? Xs[tr][tc] : 0.f;
  }
  // waves 0, 1: the tile's 64 rows, columns [0, 32) / [32, 64); waves 2, 3: its 64 columns, rows likewise.
  // Ascending within the half; elements outside the batch are left out.
  {
    const int side = w >> 1, half = w & 1;
    const long long myid = ids_s[side][lane];
    const int obase = (side ? i0 : j0) + half * 32;
    float v[32];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      v[c] = side ? Xs[half * 32 + c][lane] : Xs[lane][half * 32 + c];
      if (obase + c < Bg) m = fmaxf(m, v[c]);
    }
    float s = 0.f, ps = 0.f, cnt = 0.f;
#pragma unroll
    for (int c = 0; c < 32; ++c)
      if (obase + c < Bg) {
        s += expf(v[c] - m);
        if (ids_s[side ^ 1][half * 32 + c] == myid) { ps += v[c]; cnt += 1.f; }
      }
    hp[side][half][lane][0] = m; hp[side][half][lane][1] = s;
    hp[side][half][lane][2] = ps; hp[side][half][lane][3] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 2 * TB) {
    // the low half always holds an element of the batch (the tile starts inside it); an empty high half is
    // (-inf, 0) and drops out: 0 * exp(-inf) = 0
    const int side = w;
    const float m0 = hp[side][0][lane][0], m1 = hp[side][1][lane][0];
    const float M = fmaxf(m0, m1);
    const float S = hp[side][0][lane][1] * expf(m0 - M) + hp[side][1][lane][1] * expf(m1 - M);
    const float PS = hp[side][0][lane][2] + hp[side][1][lane][2];
    const float C = hp[side][0][lane][3] + hp[side][1][lane][3];
    const int64_t nT = p.L.nT, Bp = p.L.Bp;
    float* dst = p.ws + (side ? p.L.cp + (int64_t)blockIdx.y * Bp + j0 + lane
                              : p.L.rp + (int64_t)blockIdx.x * Bp + i0 + lane);
    dst[0] = M; dst[nT * Bp] = S; dst[2 * nT * Bp] = PS; dst[3 * nT * Bp] = C;
  }
}

// ------------------------------------------------------------------ (c) merge the partials: a thread per row / column
__global__ __launch_bounds__(NTH) void mp_merge_kernel(MP p) {
  const int64_t e = (int64_t)blockIdx.x * NTH + threadIdx.x;
  if (e >= 2 * (int64_t)p.Bg) return;
  const int side = e >= p.Bg, idx = (int)(e - (int64_t)side * p.Bg);
  const int64_t nT = p.L.nT, Bp = p.L.Bp;
  const float* src = p.ws + (side ? p.L.cp : p.L.rp) + idx;
  float M = src[0], S = src[nT * Bp], PS = src[2 * nT * Bp], C = src[3 * nT * Bp];
  for (int64_t tk = 1; tk < nT; ++tk) {                    // ascending tile order
    const float m = src[tk * Bp], s = src[(nT + tk) * Bp];
    const float Mn = fmaxf(M, m);
    S = S * expf(M - Mn) + s * expf(m - Mn);
    M = Mn;
    PS += src[(2 * nT + tk) * Bp];
    C += src[(3 * nT + tk) * Bp];
  }
  const float lse = M + logf(S), invn = 1.f / C;           // C >= 1: a row is in its own group
  float* st = p.ws + p.L.st;
  st[(side ? ST_LSEC : ST_LSER) * Bp + idx] = lse;
  st[(side ? ST_TERMC : ST_TERMR) * Bp + idx] = lse - PS * invn;
  if (!side) { st[ST_INVN * Bp + idx] = invn; st[ST_N * Bp + idx] = C; }
}

// ------------------------------------------------------------------ (d) x -> g = dL/dx in place, the tile's sum g x
__global__ __launch_bounds__(NTH) void mp_g_kernel(MP p) {
  __shared__ float lser[TB], lsec[TB], invn[TB];
  __shared__ long long ids_s[2][TB];
  __shared__ float red[NTH / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i0 = blockIdx.y * TB, j0 = blockIdx.x * TB, Bg = p.Bg;
  const int64_t ldG = p.L.ldG, Bp = p.L.Bp;
  const float* st = p.ws + p.L.st;
  if (w == 0) {
    lser[lane] = st[ST_LSER * Bp + i0 + lane];             // i0 + lane < Bp: rows past Bg are never used
    invn[lane] = st[ST_INVN * Bp + i0 + lane];
    ids_s[0][lane] = i0 + lane < Bg ? p.ids[i0 + lane] : 0;
  } else if (w == 1) {
    lsec[lane] = st[ST_LSEC * Bp + j0 + lane];
    ids_s[1][lane] = j0 + lane < Bg ? p.ids[j0 + lane] : 0;
  }
  __syncthreads();
  float* X = p.ws + p.L.X;
  const float h = 0.5f / (float)Bg;
  float sgx = 0.f;                                          // this thread's 16 elements, ascending
  for (int e = threadIdx.x; e < TB * TB; e += NTH) {
    const int tr = e >> 6, tc = e & 63;
    if (i0 + tr < Bg && j0 + tc < Bg) {
      float* px = X + (int64_t)(i0 + tr) * ldG + j0 + tc;
      const float x = *px;
      const float pos = ids_s[0][tr] == ids_s[1][tc] ? 2.f * invn[tr] : 0.f;   // n_i = n_j inside a group
      const float gv = h * ((expf(x - lser[tr]) + expf(x - lsec[tc])) - pos);
      *px = gv;
      sgx += gv * x;
    }
  }
  sgx = warp_sum(sgx);
  if (lane == 0) red[w] = sgx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = 0.f;
    for (int k = 0; k < NTH / 64; ++k) v += red[k];
    p.ws[p.L.part + (int64_t)blockIdx.y * p.L.nT + blockIdx.x] = v;
  }
}

// ------------------------------------------------------------------ (e) gradient tile
// out[row][d] = temp sum_k g(row, k) other[k][d] over all Bg rows k of the other side.  TEXT: the output rows
// are text rows i, G is read along its rows (K-contiguous); otherwise they are image rows j and G is read
// along its columns (row-contiguous).
template <bool TEXT>
__device__ __forceinline__ void grad_tile(const MP& p, float* smem) {
  constexpr int A_FLOATS = TEXT ? TB * LDR : KT * LDA, B_FLOATS = KT * LDB;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int Bg = p.Bg;
  const int r0 = p.row0 + blockIdx.y * TB, d0 = blockIdx.x * DC;
  const int rend = p.row0 + p.rows;
  const int64_t ldD = p.L.ldD, ldG = p.L.ldG;
  const float* G = p.ws + p.L.X;
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
  // normalised latent, finished by mp_finish_kernel
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

__global__ __launch_bounds__(NTH) void mp_grad_kernel(MP p) {
  // both sides' images have the same size: [64][LDR] / [16][LDA] floats of G plus [16][LDB] of latents, twice
  static_assert(TB * LDR == KT * LDA, "one LDS buffer serves both sides");
  __shared__ __attribute__((aligned(16))) float smem[2 * (TB * LDR + KT * LDB)];
  if (blockIdx.z == 0) grad_tile<true>(p, smem);
  else grad_tile<false>(p, smem);
}

// ------------------------------------------------------------------ (f) l2norm backward, final scalars
__global__ __launch_bounds__(NTH) void mp_finish_kernel(MP p) {
  __shared__ float fsum[NTH];
  __shared__ int isum[NTH];
  __shared__ float rowsum[(MAXBG + TB - 1) / TB];
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
  // the last workgroup.  Loss: the 2 Bg terms (rows, then columns) in 256 consecutive blocks, each summed
  // ascending by one thread, the 256 block sums ascending.  npos: integers.  dlogtemp: thread ti folds its
  // tile row in ascending column-tile order, then the tile rows ascending.
  const int Bg = p.Bg, nT = (int)p.L.nT, t = threadIdx.x;
  const int64_t Bp = p.L.Bp;
  const float* st = p.ws + p.L.st;
  const int per = (2 * Bg + NTH - 1) / NTH;
  float fs = 0.f;
  int is = 0;
  for (int e = t * per; e < (t + 1) * per && e < 2 * Bg; ++e) {
    fs += e < Bg ? st[ST_TERMR * Bp + e] : st[ST_TERMC * Bp + e - Bg];
    if (e < Bg) is += (int)st[ST_N * Bp + e] - 1;
  }
  fsum[t] = fs;
  isum[t] = is;
  for (int ti = t; ti < nT; ti += NTH) {
    const float* src = p.ws + p.L.part + (int64_t)ti * nT;
    float v = 0.f;
    for (int tj = 0; tj < nT; ++tj) v += src[tj];
    rowsum[ti] = v;
  }
  __syncthreads();
  if (t == 0) {
    float v = 0.f;
    for (int k = 0; k < NTH; ++k) v += fsum[k];
    p.loss[0] = v * (0.5f / (float)Bg);
  } else if (t == 64) {
    int v = 0;
    for (int k = 0; k < NTH; ++k) v += isum[k];
    p.npos[0] = v;
  } else if (t == 128) {
    float v = 0.f;
    for (int ti = 0; ti < nT; ++ti) v += rowsum[ti];
    p.dlogtemp[0] = v;                                      // x carries temp: dL/dlog_temp = sum g x
  }
}

bool shape_ok(const ctclip_multipos_loss_args* a) {
  return a->Bg >= 1 && a->Bg <= MAXBG && a->Dl >= 1 && a->Dl <= MAXDL;
}

// ------------------------------------------------------------------ report ids: one wave per report
__device__ __forceinline__ uint64_t fmix64(uint64_t x) {   // the splitmix64 finaliser of common.h hid_keep
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

__global__ __launch_bounds__(NTH) void report_ids_kernel(const long long* __restrict__ ids,
                                                         const long long* __restrict__ mask, int B, int L,
                                                         long long* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= B) return;
  unsigned long long sum = 0, kept = 0;                     // wrapping adds commute: any order, same bits
  for (int c0 = 0; c0 < L; c0 += 64) {                     // wave-uniform trip count
    const int c = c0 + lane;
    const bool keep = c < L && mask[r * L + c] != 0;
    const unsigned long long b = __ballot(keep);
    if (keep) {
      const unsigned long long k = kept + __popcll(b & ((1ull << lane) - 1ull));   // index among the kept tokens
      sum += fmix64(fmix64((uint64_t)ids[r * L + c]) + (k + 1ull) * 0x9E3779B97F4A7C15ull);
    }
    kept += __popcll(b);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) out[r] = (long long)fmix64(sum + kept * 0xD1B54A32D192ED03ull);
}

}  // namespace

extern "C" int64_t ctclip_multipos_loss_ws_bytes(const ctclip_multipos_loss_args* a) {
  if (!a || !shape_ok(a)) return 0;
  return 4 * make_layout(a->Bg, a->Dl).total;
}

extern "C" int ctclip_multipos_loss(const ctclip_multipos_loss_args* a, void* stream) {
  CT_REQUIRE(a != nullptr, CT_EINVAL);
  CT_REQUIRE(shape_ok(a), CT_ESHAPE);
  CT_REQUIRE(a->t_raw && a->i_raw && a->ids && a->log_temp && a->loss && a->dt_raw && a->di_raw && a->dlogtemp &&
                 a->npos && a->ws,
             CT_EINVAL);
  CT_REQUIRE(a->grad_row0 >= 0 && a->grad_rows >= 1 && (int64_t)a->grad_row0 + a->grad_rows <= a->Bg, CT_EINVAL);
  CT_REQUIRE(aligned16(a->ws), CT_EALIGN);
  MP p;
  p.t_raw = a->t_raw; p.i_raw = a->i_raw; p.ids = (const long long*)a->ids; p.log_temp = a->log_temp;
  p.Bg = a->Bg; p.Dl = a->Dl; p.row0 = a->grad_row0; p.rows = a->grad_rows;
  p.loss = a->loss; p.dt = a->dt_raw; p.di = a->di_raw; p.dlogtemp = a->dlogtemp; p.npos = a->npos;
  p.ws = a->ws;
  p.L = make_layout(a->Bg, a->Dl);
  CT_REQUIRE(a->ws_bytes >= 4 * p.L.total, CT_EINVAL);
  const hipStream_t st = (hipStream_t)stream;
  const int nT = (int)p.L.nT;
  hipLaunchKernelGGL(mp_norm_kernel, dim3((unsigned)cdiv(2 * (int64_t)p.Bg, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(mp_logits_kernel, dim3(nT, nT), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(mp_merge_kernel, dim3((unsigned)cdiv(2 * (int64_t)p.Bg, NTH)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(mp_g_kernel, dim3(nT, nT), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(mp_grad_kernel, dim3(cdiv(p.Dl, DC), cdiv(p.rows, TB), 2), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(mp_finish_kernel, dim3((unsigned)cdiv(2 * (int64_t)p.rows, 4) + 1), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_report_ids(const int64_t* input_ids, const int64_t* attention_mask, int32_t B, int32_t L,
                                 int64_t* out, void* stream) {
  CT_REQUIRE(B >= 1 && L >= 1 && L <= (1 << 20), CT_ESHAPE);
  CT_REQUIRE(input_ids && attention_mask && out, CT_EINVAL);
  hipLaunchKernelGGL(report_ids_kernel, dim3((unsigned)cdiv(B, 4)), dim3(NTH), 0, (hipStream_t)stream,
                     (const long long*)input_ids, (const long long*)attention_mask, (int)B, (int)L, (long long*)out);
  CT_CHECK_LAUNCH();
  return 0;
}
