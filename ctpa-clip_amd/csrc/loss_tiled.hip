// Tiled contrastive loss (include/ctclip_hip.h, ctclip_clip_loss_tiled): the general loss of loss.hip
// (ct_clip/ct_clip.py:845-899: multiview pairs, the CLOOB extra pair, decoupled contrastive learning)
// for global batches the one-workgroup kernel cannot hold -- Bg up to 8192 -- with the Bg x Bg logits
// and both gradient products on the f32 matrix pipe (v_mfma_f32_16x16x4_f32, exact f32: each output
// is one fma chain in ascending k).  Five passes (six launches), no waiting between workgroups, no
// float atomics:
//   (a) lt_norm_kernel    every latent set l2-normalised ONCE into the workspace (eps 1e-12), norms kept
//   (b) lt_logits_kernel  grid (column tile, row tile, pair x matrix): S = temp t . i^T on MFMA, E = exp(S)
//                         STORED, per-tile partial row / column sums of E and of E S, the diagonal
//   (c) lt_sums_kernel    one workgroup per pair: partials folded in ascending tile order into the
//                         reciprocal denominators, the pair loss and the pair's d loss / d log-temp
//   (d) lt_grad_kernel    one launch for the text views, one for the image views; grid (Dl chunk, row tile,
//                         latent pair x view): G = sum over the pairs of the row (ascending) and their
//                         column tiles (ascending) of w_p temp dS . other, dS formed from E and the
//                         denominators while the tile is staged; one MFMA chain per output
//   (e) lt_finish_kernel  one wave per output row: the l2norm backward (linear, so it follows the weighted
//                         pair sum); thread 0 folds the pair losses and temperature gradients in pair order
// Every sum has a fixed order that depends on neither the launch geometry of another row nor the
// requested row range, so two runs -- and a row asked for alone or inside 0..Bg -- give the same bits.
// d loss / d log-temp needs no sweep of its own: sum_ij dS_ij S_ij splits into the row sums of
// E S over the row denominators, the column sums over the column denominators and the diagonal.
//
// Workspace (floats, every segment a multiple of 4; ldD = Dl rounded up to 4, ldE = Bg rounded up to 4,
// NV = (extra ? 2 : 1) (Vt + Vi) latent views, NM = extra ? 2 : 1 matrices per pair, nT = ceil(Bg / 64)):
//   nv [NV][Bg][ldD] normalised latents (pad columns zero) | nrm [NV][Bg] | E [P][NM][Bg][ldE] |
//   part [4][P][nT][Bg] (row E, row ES, column E, column ES) | diag [P][2][2][Bg] (E, S of matrix 0 and
//   NM-1) | den [P][2][Bg] (1 / (row sum + 1e-20), 1 / (column sum + 1e-20)) | sc [P][2] (loss, dlogtemp)
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int MAXBG = 8192, MAXDL = 8192, MAXP = 64;
constexpr int TB = 64;            // rows / columns of a logits tile, rows of a gradient tile
constexpr int DC = 128;           // Dl chunk of a gradient tile
constexpr int KT = 16;            // K step
constexpr int LDR = 20;           // K-contiguous LDS image [row][16 k]: 16-B aligned rows, 64 lanes on 64 banks
constexpr int LDA = 80;           // row-contiguous LDS image [16 k][64 rows]: k groups 16 banks apart
constexpr int LDB = 144;          // row-contiguous LDS image [16 k][128 columns]
constexpr int NTH = 256;

struct Layout {
  int64_t ldD, ldE, nT, NV, NM, P;
  int64_t nv, nrm, E, part, diag, den, sc, total;
};

__host__ __device__ inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }

inline Layout make_layout(int Vt, int Vi, int Bg, int Dl, bool extra) {
  Layout L;
  L.ldD = up4(Dl);
  L.ldE = up4(Bg);
  L.nT = (Bg + TB - 1) / TB;
  L.NM = extra ? 2 : 1;
  L.NV = L.NM * (Vt + Vi);
  L.P = (int64_t)Vt * Vi;
  int64_t o = 0;
  L.nv = o;   o += L.NV * Bg * L.ldD;
  L.nrm = o;  o += up4(L.NV * Bg);
  L.E = o;    o += L.P * L.NM * Bg * L.ldE;
  L.part = o; o += up4(4 * L.P * L.nT * Bg);
  L.diag = o; o += up4(L.P * 4 * Bg);
  L.den = o;  o += up4(L.P * 2 * Bg);
  L.sc = o;   o += up4(L.P * 2);
  L.total = o;
  return L;
}

struct TP {
  const float* t_raw; const float* i_raw; const float* t_extra; const float* i_extra;
  const float* log_temp;
  int Vt, Vi, Bg, Dl, dcl;
  float w_main, w_mv;
  int row0, rows;
  float* loss; float* pair_loss; float* dt; float* di; float* dtx; float* dix; float* dlogtemp;
  float* ws;
  Layout L;
};

// latent view v in [0, NV): x = v / (Vt + Vi) (0 main, 1 extra pair), u = v % (Vt + Vi) (text views first)
__device__ __forceinline__ const float* raw_view(const TP& p, int v) {
  const int nvw = p.Vt + p.Vi, x = v / nvw, u = v - x * nvw;
  const int64_t set = (int64_t)p.Bg * p.Dl;
  if (u < p.Vt) return (x ? p.t_extra : p.t_raw) + u * set;
  return (x ? p.i_extra : p.i_raw) + (u - p.Vt) * set;
}

// ------------------------------------------------------------------ (a) normalise: one wave per row
__global__ __launch_bounds__(NTH) void lt_norm_kernel(TP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= p.L.NV * p.Bg) return;
  const int v = (int)(r / p.Bg), a = (int)(r - (int64_t)v * p.Bg);
  const float* src = raw_view(p, v) + (int64_t)a * p.Dl;
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

__global__ __launch_bounds__(NTH) void lt_logits_kernel(TP p) {
  __shared__ __attribute__((aligned(16))) float smem[4 * TB * LDR];   // [buf][A | B]
  __shared__ float Es[TB][TB + 1], Ss[TB][TB + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  const int NM = (int)p.L.NM, nvw = p.Vt + p.Vi;
  const int pq = blockIdx.z, pr = pq / NM, q = pq - pr * NM, m = pr / p.Vi, n = pr - m * p.Vi;
  const int i0 = blockIdx.y * TB, j0 = blockIdx.x * TB, Bg = p.Bg;
  const int64_t ldD = p.L.ldD, ldE = p.L.ldE, vs = (int64_t)Bg * ldD;
  const float* A = p.ws + p.L.nv + (int64_t)(q * nvw + m) * vs;            // text view m of latent pair q
  const float* B = p.ws + p.L.nv + (int64_t)(q * nvw + p.Vt + n) * vs;     // image view n
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
      for (int r = 0; r < 4; ++r) {
        const int tr = wm * 32 + i * 16 + r16, tc = wn * 32 + j * 16 + 4 * g + r;
        const bool ok = i0 + tr < Bg && j0 + tc < Bg;
        const float s = acc[i][j][r] * temp;
        Ss[tr][tc] = ok ? s : 0.f;
        Es[tr][tc] = ok ? expf(s) : 0.f;
      }
  __syncthreads();
  float* E = p.ws + p.L.E + (int64_t)pq * Bg * ldE;
  for (int e = threadIdx.x; e < TB * TB; e += NTH) {
    const int tr = e >> 6, tc = e & 63;
    if (i0 + tr < Bg && j0 + tc < ldE) E[(int64_t)(i0 + tr) * ldE + j0 + tc] = Es[tr][tc];
  }
  // partial sums in ascending order inside the tile; the decoupled loss leaves the diagonal out
  const int t = threadIdx.x;
  const int64_t pstride = p.L.P * p.L.nT * Bg;
  if (t < TB) {
    if (q == 0 && i0 + t < Bg) {             // row sums feed the text -> image direction: matrix 0
      float se = 0.f, ses = 0.f;
      for (int c = 0; c < TB; ++c) {
        if (p.dcl && i0 + t == j0 + c) continue;
        se += Es[t][c];
        ses += Es[t][c] * Ss[t][c];
      }
      float* dst = p.ws + p.L.part + ((int64_t)pr * p.L.nT + blockIdx.x) * Bg + i0 + t;
      dst[0] = se;
      dst[pstride] = ses;
    }
  } else if (t < 2 * TB) {
    const int c = t - TB;
    if (q == NM - 1 && j0 + c < Bg) {        // column sums feed image -> text: the extra pair's matrix if any
      float se = 0.f, ses = 0.f;
      for (int r = 0; r < TB; ++r) {
        if (p.dcl && i0 + r == j0 + c) continue;
        se += Es[r][c];
        ses += Es[r][c] * Ss[r][c];
      }
      float* dst = p.ws + p.L.part + 2 * pstride + ((int64_t)pr * p.L.nT + blockIdx.y) * Bg + j0 + c;
      dst[0] = se;
      dst[pstride] = ses;
    }
  } else if (t < 3 * TB) {
    const int d = t - 2 * TB;
    if (i0 == j0 && i0 + d < Bg) {
      float* dg = p.ws + p.L.diag + (int64_t)pr * 4 * Bg + i0 + d;
      if (q == 0) { dg[0] = Es[d][d]; dg[Bg] = Ss[d][d]; }
      if (q == NM - 1) { dg[2 * (int64_t)Bg] = Es[d][d]; dg[3 * (int64_t)Bg] = Ss[d][d]; }
    }
  }
}

// ------------------------------------------------------------------ (c) sums: one workgroup per pair
__global__ __launch_bounds__(NTH) void lt_sums_kernel(TP p) {
  __shared__ float red[NTH / 64];
  const int pr = blockIdx.x, Bg = p.Bg, nT = (int)p.L.nT;
  const int64_t pstride = p.L.P * p.L.nT * Bg;
  const float* part = p.ws + p.L.part + (int64_t)pr * nT * Bg;
  const float* dg = p.ws + p.L.diag + (int64_t)pr * 4 * Bg;
  float* den = p.ws + p.L.den + (int64_t)pr * 2 * Bg;
  float lpart = 0.f, dpart = 0.f;
  for (int i = threadIdx.x; i < Bg; i += NTH) {
    float rs = 0.f, rses = 0.f, cs = 0.f, cses = 0.f;
    for (int tl = 0; tl < nT; ++tl) {
      const int64_t o = (int64_t)tl * Bg + i;
      rs += part[o];
      rses += part[pstride + o];
      cs += part[2 * pstride + o];
      cses += part[3 * pstride + o];
    }
    const float e0 = dg[i], s0 = dg[Bg + i], e1 = dg[2 * (int64_t)Bg + i], s1 = dg[3 * (int64_t)Bg + i];
    const float rr = 1.f / (rs + 1e-20f), cc = 1.f / (cs + 1e-20f);
    den[i] = rr;
    den[Bg + i] = cc;
    lpart += (-logf(e0 + 1e-20f) + logf(rs + 1e-20f)) + (-logf(e1 + 1e-20f) + logf(cs + 1e-20f));
    dpart += (rses * rr + cses * cc) - (s0 * (e0 / (e0 + 1e-20f)) + s1 * (e1 / (e1 + 1e-20f)));
  }
  const float tot = block_sum(lpart, red);
  const float dtot = block_sum(dpart, red);
  if (threadIdx.x == 0) {
    p.ws[p.L.sc + 2 * pr] = 0.5f * tot / Bg;
    p.ws[p.L.sc + 2 * pr + 1] = (0.5f / Bg) * dtot;
  }
}

// ------------------------------------------------------------------ (d) gradient tile
// G[v][row][d] = sum_c scale_p sum_k dS_p(row, k) other_c[k][d] over the partner views c of view v
// (pair p ascending with c) and all Bg rows k of the other side.  TEXT: the output rows are text rows i,
// dS is read along its rows (E is K-contiguous); otherwise they are image rows j and dS is read along its
// columns (row-contiguous).  dS of one element, E = exp(S), rr / cc the reciprocal denominators:
//   no extra pair: E rr_i + E cc_j, on the diagonal (0 when decoupled) - 2 E / (E + 1e-20)
//   extra pair:    matrix 0 carries E rr_i, matrix 1 E cc_j, on the diagonal (0 when decoupled) - E / (E + 1e-20)
template <bool TEXT>
__global__ __launch_bounds__(NTH) void lt_grad_kernel(TP p) {
  constexpr int A_FLOATS = TEXT ? TB * LDR : KT * LDA, B_FLOATS = KT * LDB;
  __shared__ __attribute__((aligned(16))) float smem[2 * (A_FLOATS + B_FLOATS)];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int nvw = p.Vt + p.Vi, NM = (int)p.L.NM, Bg = p.Bg;
  // blockIdx.z walks the text (TEXT) or image views of every latent pair x
  const int cntv = TEXT ? p.Vt : p.Vi, x = blockIdx.z / cntv, uu = blockIdx.z - x * cntv;
  const int r0 = p.row0 + blockIdx.y * TB, d0 = blockIdx.x * DC;
  const int rend = p.row0 + p.rows;
  const int64_t ldD = p.L.ldD, ldE = p.L.ldE, vs = (int64_t)Bg * ldD;
  const int cnt = TEXT ? p.Vi : p.Vt;
  const int dmode = NM == 1 ? 0 : (x == 0 ? 1 : 2);   // 0: both directions, 1: rows only, 2: columns only
  const float dcoef = NM == 1 ? 2.f : 1.f;
  const float temp = expf(p.log_temp[0]);
  const float w_rest = p.L.P > 1 ? p.w_mv / (float)(p.L.P - 1) : 0.f;
  const int nkb = (Bg + KT - 1) / KT, steps = cnt * nkb;
  // this thread's 4 dS elements of a step: TEXT row t / 4, k = 4 (t % 4) + e; else row t % 64, k = t / 64 + 4 e
  const int am = TEXT ? t >> 2 : t & 63;
  const int grow = r0 + am;                            // the output row (text row i / image row j)
  const bool rowok = grow < Bg;
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  float ea[4], va[4];       // staged E values and the varying denominators
  float fixden = 0.f, scale = 0.f;
  f32x4 rb[2];
  auto gload = [&](int step) {
    const int c = step / nkb, k0 = (step - c * nkb) * KT;
    const int pr = TEXT ? uu * p.Vi + c : c * p.Vi + uu;
    const float* E = p.ws + p.L.E + ((int64_t)pr * NM + x) * Bg * ldE;
    const float* den = p.ws + p.L.den + (int64_t)pr * 2 * Bg;
    scale = (pr == 0 ? p.w_main : w_rest) * temp * (0.5f / Bg);
    // fixed denominator of the output row, varying one of the k index
    fixden = rowok ? (TEXT ? den[grow] : den[Bg + grow]) : 0.f;
    if (TEXT) {
      const int gk = k0 + (t & 3) * 4;
      f32x4 e4 = (rowok && gk < ldE) ? *(const f32x4*)(E + (int64_t)grow * ldE + gk) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = rowok && gk + e < Bg;
        ea[e] = ok ? e4[e] : 0.f;
        va[e] = ok ? den[Bg + gk + e] : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int gk = k0 + (t >> 6) + 4 * e;
        const bool ok = rowok && gk < Bg;
        ea[e] = ok ? E[(int64_t)gk * ldE + grow] : 0.f;
        va[e] = ok ? den[gk] : 0.f;
      }
    }
    // the other side's normalised latents: rows k0 + t / 32 + 8 i, columns d0 + 4 (t % 32)
    const float* O = p.ws + p.L.nv + (int64_t)(x * nvw + (TEXT ? p.Vt + c : c)) * vs;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int gk = k0 + (t >> 5) + 8 * i, gd = d0 + (t & 31) * 4;
      rb[i] = (gk < Bg && gd < ldD) ? *(const f32x4*)(O + (int64_t)gk * ldD + gd) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto swrite = [&](int step, float* As, float* Bs) {
    const int c = step / nkb, k0 = (step - c * nkb) * KT;
    float d[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int gk = TEXT ? k0 + (t & 3) * 4 + e : k0 + (t >> 6) + 4 * e;
      const float E = ea[e];
      const float rr = TEXT ? fixden : va[e], cc = TEXT ? va[e] : fixden;
      float v = dmode == 0 ? E * rr + E * cc : dmode == 1 ? E * rr : E * cc;
      if (gk == grow) {
        if (p.dcl) v = 0.f;
        v -= dcoef * (E / (E + 1e-20f));
      }
      d[e] = (rowok && gk < Bg) ? v * scale : 0.f;
    }
    if (TEXT) {
      *(f32x4*)(As + (t >> 2) * LDR + (t & 3) * 4) = f32x4{d[0], d[1], d[2], d[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) As[((t >> 6) + 4 * e) * LDA + (t & 63)] = d[e];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) *(f32x4*)(Bs + ((t >> 5) + 8 * i) * LDB + (t & 31) * 4) = rb[i];
  };

  gload(0);
  swrite(0, smem, smem + A_FLOATS);
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
      swrite(st + 1, nb, nb + A_FLOATS);
    }
    __syncthreads();
  }
  // lane: tile row wm*32 + 16 i + r16, columns d0 + wn*64 + 16 j + 4 g + [0, 4); raw gradient w.r.t. the
  // normalised latent, finished by lt_finish_kernel
  float* outb = x == 0 ? (TEXT ? p.dt : p.di) : (TEXT ? p.dtx : p.dix);
  float* out = outb + (int64_t)uu * p.rows * p.Dl;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int gr = r0 + wm * 32 + i * 16 + r16;
    if (gr >= rend) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gd = d0 + wn * 64 + j * 16 + 4 * g + r;
        if (gd < p.Dl) out[(int64_t)(gr - p.row0) * p.Dl + gd] = acc[i][j][r];
      }
  }
}

// ------------------------------------------------------------------ (e) l2norm backward, final scalars
__global__ __launch_bounds__(NTH) void lt_finish_kernel(TP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r < p.L.NV * p.rows) {
    const int nvw = p.Vt + p.Vi;
    const int v = (int)(r / p.rows), lr = (int)(r - (int64_t)v * p.rows), x = v / nvw, u = v - x * nvw;
    const int64_t grow = (int64_t)v * p.Bg + p.row0 + lr;
    const float* self = p.ws + p.L.nv + grow * p.L.ldD;
    const float nn = p.ws[p.L.nrm + grow];
    float* outb = x == 0 ? (u < p.Vt ? p.dt : p.di) : (u < p.Vt ? p.dtx : p.dix);
    float* out = outb + ((int64_t)(u < p.Vt ? u : u - p.Vt) * p.rows + lr) * p.Dl;
    float dotp = 0.f;
    for (int k = lane; k < p.Dl; k += 64) dotp += out[k] * self[k];
    dotp = warp_sum(dotp);
    const float inv = 1.f / fmaxf(nn, 1e-12f);
    for (int k = lane; k < p.Dl; k += 64) {
      const float gq = out[k];
      out[k] = nn > 1e-12f ? (gq - self[k] * dotp) * inv : gq * inv;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int P = (int)p.L.P;
    const float* sc = p.ws + p.L.sc;
    const float w_rest = P > 1 ? p.w_mv / (float)(P - 1) : 0.f;
    float rest = 0.f, dl = p.w_main * sc[1];
    for (int q = 0; q < P; ++q) p.pair_loss[q] = sc[2 * q];
    for (int q = 1; q < P; ++q) {
      rest += sc[2 * q];
      dl += w_rest * sc[2 * q + 1];
    }
    p.loss[0] = P > 1 ? p.w_main * sc[0] + p.w_mv * (rest / (float)(P - 1)) : p.w_main * sc[0];
    p.dlogtemp[0] = dl;
  }
}

bool shape_ok(const ctclip_clip_loss_tiled_args* a) {
  return a->Vt >= 1 && a->Vi >= 1 && (int64_t)a->Vt * a->Vi <= MAXP && a->Bg >= 1 && a->Bg <= MAXBG && a->Dl >= 1 &&
         a->Dl <= MAXDL;
}

}  // namespace

extern "C" int64_t ctclip_clip_loss_tiled_ws_bytes(const ctclip_clip_loss_tiled_args* a) {
  if (!a || !shape_ok(a)) return 0;
  return 4 * make_layout(a->Vt, a->Vi, a->Bg, a->Dl, a->t_extra != nullptr).total;
}

extern "C" int ctclip_clip_loss_tiled(const ctclip_clip_loss_tiled_args* a, void* stream) {
  CT_REQUIRE(a != nullptr, CT_EINVAL);
  CT_REQUIRE(shape_ok(a), CT_ESHAPE);
  const bool extra = a->t_extra != nullptr;
  CT_REQUIRE(extra == (a->i_extra != nullptr), CT_EINVAL);
  CT_REQUIRE(a->t_raw && a->i_raw && a->log_temp && a->loss && a->pair_loss && a->dt_raw && a->di_raw && a->dlogtemp &&
                 a->ws,
             CT_EINVAL);
  CT_REQUIRE(!extra || (a->dt_extra && a->di_extra), CT_EINVAL);
  CT_REQUIRE(a->grad_row0 >= 0 && a->grad_rows >= 1 && (int64_t)a->grad_row0 + a->grad_rows <= a->Bg, CT_EINVAL);
  CT_REQUIRE(aligned16(a->ws), CT_EALIGN);
  TP p;
  p.t_raw = a->t_raw; p.i_raw = a->i_raw; p.t_extra = a->t_extra; p.i_extra = a->i_extra;
  p.log_temp = a->log_temp;
  p.Vt = a->Vt; p.Vi = a->Vi; p.Bg = a->Bg; p.Dl = a->Dl; p.dcl = a->decoupled != 0;
  p.w_main = a->w_main; p.w_mv = a->w_multiview;
  p.row0 = a->grad_row0; p.rows = a->grad_rows;
  p.loss = a->loss; p.pair_loss = a->pair_loss; p.dt = a->dt_raw; p.di = a->di_raw; p.dtx = a->dt_extra;
  p.dix = a->di_extra; p.dlogtemp = a->dlogtemp;
  p.ws = a->ws;
  p.L = make_layout(a->Vt, a->Vi, a->Bg, a->Dl, extra);
  CT_REQUIRE(a->ws_bytes >= 4 * p.L.total, CT_EINVAL);
  const hipStream_t st = (hipStream_t)stream;
  const int NM = (int)p.L.NM, P = (int)p.L.P, nT = (int)p.L.nT;
  hipLaunchKernelGGL(lt_norm_kernel, dim3((unsigned)cdiv(p.L.NV * p.Bg, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(lt_logits_kernel, dim3(nT, nT, P * NM), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(lt_sums_kernel, dim3(P), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  const dim3 gt(cdiv(p.Dl, DC), cdiv(p.rows, TB), NM * p.Vt), gi(cdiv(p.Dl, DC), cdiv(p.rows, TB), NM * p.Vi);
  hipLaunchKernelGGL(lt_grad_kernel<true>, gt, dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(lt_grad_kernel<false>, gi, dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(lt_finish_kernel, dim3((unsigned)cdiv(p.L.NV * p.rows, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  return 0;
}
