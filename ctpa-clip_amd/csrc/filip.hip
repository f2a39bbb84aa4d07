// Fine-grained (FILIP) token-wise contrastive loss (include/ctclip_hip.h, ctclip_filip_loss;
// ct_clip/ct_clip.py:751-755, 829-878 with use_all_token_embeds): every text token of report x is scored
// against every image token of volume y, S[x,y,t,i] = temp <tn[x,t], in[y,i]> on unit latents,
//   A[x,y] = sum_t mask[x,t] max_i S / max(sum_t mask[x,t], 1e-6)      (text -> image)
//   C[x,y] = (1 / I) sum_i max_{t : mask[x,t]} S                        (image -> text)
// and InfoNCE is taken over A and over C.  The Bg x Bg x T x I scores are never written: the products run
// tile-wise on the f32 matrix pipe (v_mfma_f32_16x16x4_f32, exact f32, one fma chain in ascending k per
// score) and only the argmax of every row / column leaves the kernel.
// TIE RULE: a max that several indices attain belongs to the LOWEST of them, and the whole gradient of
// that max goes there (torch.amax would split it).  Equal tokens give equal bits on the matrix pipe (same
// operands, same order), so duplicates tie exactly and the backward is a pure function of the indices.
// Launch plan (seven launches, no waiting between workgroups, no float atomics):
//   (a) fl_norm_kernel      every token l2-normalised ONCE into the workspace (eps 1e-12), norms kept
//   (b) fl_argmax_kernel    <true>:  grid (t tile, y, x): 64 text rows x all I image tokens -> idx_t2i; a tile
//                                    of masked text tokens is left without a product
//                           <false>: grid (i tile, y, x): 64 image rows x the text tokens -> idx_i2t; masked
//                                    text tokens never enter the max, a 64-token tile of them is skipped
//   (c) fl_pair_kernel      one workgroup per (x, y): the chosen scores again as plain f32 dot products
//                           (O(Bg^2 (T + I) Dl)), summed in a fixed order into A[x,y] and C[x,y]
//   (d) fl_sums_kernel      one workgroup: the two Bg x Bg softmaxes, the loss, d loss / d log-temp =
//                           sum_xy (dA A + dC C) (S is linear in temp), reciprocal denominators kept
//   (e) fl_grad_kernel      <true> one wave per text token, <false> one wave per image token.  dS has ONE
//                           nonzero per (x, y, t) row and ONE per (x, y, i) column, so the gradient of a token
//                           is a weighted sum of gathered rows of the other side: its own winner per pair,
//                           plus every row whose winner it is, found by scanning that pair's index row 64
//                           entries at a time (ballot) in ascending order.  The wave owns its output row (in
//                           registers), walks the pairs in ascending order and finishes with the l2norm
//                           backward: no scatter, no LDS accumulation, no second MFMA product.
// Every sum has a fixed order, so two runs give the same bits.
//
// Workspace (4-byte words, every segment a multiple of 4): tn [Bg][T][Dl] | in [Bg][I][Dl] normalised |
// nrm [Bg (T + I)] | den [4][Bg] (1 / (row sum of e^A + 1e-20), the same for C, the mask counts, unused) |
// A, C [Bg][Bg] each (only when the caller passes none) | idx_t2i [Bg][Bg][T], idx_i2t [Bg][Bg][I] int32
// (each only when the caller passes none).
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int MAXBG = 128, MAXT = 512, MAXI = 1024, MAXDL = 512;
constexpr int TB = 64;            // rows / columns of a score tile
constexpr int KT = 16;            // K step
constexpr int LDR = 20;           // K-contiguous LDS image [row][16 k]: 16-B aligned rows, 64 lanes on 64 banks
constexpr int NTH = 256;
constexpr int MR = MAXDL / 64;    // floats of a latent row per lane

struct Layout {
  int64_t tn, in, nrm, den, A, C, idxT, idxI, total;
};

inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }

inline Layout make_layout(const ctclip_filip_args* a) {
  const int64_t Bg = a->Bg, T = a->T, I = a->I, Dl = a->Dl;
  Layout L;
  int64_t o = 0;
  L.tn = o;   o += Bg * T * Dl;
  L.in = o;   o += Bg * I * Dl;
  L.nrm = o;  o += up4(Bg * (T + I));
  L.den = o;  o += up4(4 * Bg);
  L.A = o;    o += a->A ? 0 : up4(Bg * Bg);
  L.C = o;    o += a->C ? 0 : up4(Bg * Bg);
  L.idxT = o; o += a->idx_t2i ? 0 : up4(Bg * Bg * T);
  L.idxI = o; o += a->idx_i2t ? 0 : up4(Bg * Bg * I);
  L.total = o;
  return L;
}

struct FP {
  const float* t_raw; const float* i_raw; const uint8_t* mask; const float* log_temp;
  int Bg, T, I, Dl, dcl, over_text;
  float* loss; float* dt; float* di; float* dlogtemp;
  float* A; float* C; int* idxT; int* idxI;       // the caller's or the workspace's
  float* tn; float* in; float* nrm; float* den;   // workspace
};

// ------------------------------------------------------------------ (a) normalise: one wave per token
__global__ __launch_bounds__(NTH) void fl_norm_kernel(FP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t nt = (int64_t)p.Bg * p.T, r = (int64_t)blockIdx.x * 4 + w;
  if (r >= nt + (int64_t)p.Bg * p.I) return;
  const float* src = r < nt ? p.t_raw + r * p.Dl : p.i_raw + (r - nt) * p.Dl;
  float* dst = r < nt ? p.tn + r * p.Dl : p.in + (r - nt) * p.Dl;
  float q = 0.f;
  for (int k = lane; k < p.Dl; k += 64) q += src[k] * src[k];
  q = warp_sum(q);
  const float nn = sqrtf(q);
  const float inv = 1.f / fmaxf(nn, 1e-12f);
  for (int k = lane; k < p.Dl; k += 64) dst[k] = src[k] * inv;
  if (lane == 0) p.nrm[r] = nn;
}

// ------------------------------------------------------------------ (b) row argmax of P . Q^T
// one 16-B chunk of a 64-row x 16-k K-contiguous tile: row t / 4, k quad t % 4.  Rows past the token count
// are zeros in LDS (never a read past the array); Dl % 16 == 0, so there is no K tail.
__device__ __forceinline__ f32x4 kload(const float* __restrict__ base, int ld, int rows, int row0, int k0) {
  const int t = threadIdx.x, gr = row0 + (t >> 2), gk = k0 + (t & 3) * 4;
  return gr < rows ? *(const f32x4*)(base + (int64_t)gr * ld + gk) : f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void kwrite(float* img, const f32x4& r) {
  const int t = threadIdx.x;
  *(f32x4*)(img + (t >> 2) * LDR + (t & 3) * 4) = r;
}
// the better of two (score, index) candidates: the higher score, on equal scores the lower index
__device__ __forceinline__ void take_better(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// TEXT: rows are the text tokens of x (masked rows get index -1), columns the image tokens of y;
// otherwise rows are the image tokens of y, columns the text tokens of x that the mask keeps.
template <bool TEXT>
__global__ __launch_bounds__(NTH) void fl_argmax_kernel(FP p) {
  __shared__ __attribute__((aligned(16))) float smem[4 * TB * LDR];   // [buf][P | Q]
  __shared__ int qv[TB];
  __shared__ float rv[2][TB];
  __shared__ int ri[2][TB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
  const int x = blockIdx.z, y = blockIdx.y, p0 = blockIdx.x * TB, Dl = p.Dl;
  const uint8_t* mrow = p.mask + (int64_t)x * p.T;
  const float* P = TEXT ? p.tn + (int64_t)x * p.T * Dl : p.in + (int64_t)y * p.I * Dl;
  const float* Q = TEXT ? p.in + (int64_t)y * p.I * Dl : p.tn + (int64_t)x * p.T * Dl;
  const int nP = TEXT ? p.T : p.I, nQ = TEXT ? p.I : p.T;
  int* out = TEXT ? p.idxT + ((int64_t)x * p.Bg + y) * p.T : p.idxI + ((int64_t)x * p.Bg + y) * p.I;
  if (TEXT) {
    const int live = __syncthreads_or(tid < TB && p0 + tid < nP && mrow[p0 + tid]);
    if (!live) {                                   // a tile of masked text tokens: no product
      if (tid < TB && p0 + tid < nP) out[p0 + tid] = -1;
      return;
    }
  }
  const int r16 = lane & 15, g = lane >> 4, nk = Dl / KT;
  float best[2] = {-INFINITY, -INFINITY};
  int bidx[2] = {0, 0};
  for (int q0 = 0; q0 < nQ; q0 += TB) {
    if (!TEXT) {
      const int keep = tid < TB && q0 + tid < nQ && mrow[q0 + tid];
      if (tid < TB) qv[tid] = keep;
      if (!__syncthreads_or(keep)) continue;       // a tile of masked text tokens is skipped
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ra = kload(P, Dl, nP, p0, 0), rb = kload(Q, Dl, nQ, q0, 0);
    kwrite(smem, ra);
    kwrite(smem + TB * LDR, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const float* As = smem + (kt & 1) * 2 * TB * LDR;
      const float* Bs = As + TB * LDR;
      if (kt + 1 < nk) {
        ra = kload(P, Dl, nP, p0, (kt + 1) * KT);
        rb = kload(Q, Dl, nQ, q0, (kt + 1) * KT);
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
    // lane: tile row wm*32 + 16 i + r16, tile columns wn*32 + 16 j + 4 g + [0, 4), taken in ascending order
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int tc = wn * 32 + j * 16 + 4 * g + r, gq = q0 + tc;
          const bool ok = gq < nQ && (TEXT || qv[tc]);
          const float v = acc[i][j][r];
          if (ok && v > best[i]) {
            best[i] = v;
            bidx[i] = gq;
          }
        }
    if (!TEXT) __syncthreads();                    // qv is rewritten for the next tile
  }
  // the four column groups of a wave, then the two column halves of the tile
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const float ov = __shfl_xor(best[i], o, 64);
      const int oi = __shfl_xor(bidx[i], o, 64);
      take_better(best[i], bidx[i], ov, oi);
    }
    if (g == 0) {
      rv[wn][wm * 32 + i * 16 + r16] = best[i];
      ri[wn][wm * 32 + i * 16 + r16] = bidx[i];
    }
  }
  __syncthreads();
  if (tid < TB && p0 + tid < nP) {
    float v = rv[0][tid];
    int ix = ri[0][tid];
    take_better(v, ix, rv[1][tid], ri[1][tid]);
    out[p0 + tid] = (TEXT && !mrow[p0 + tid]) ? -1 : ix;
  }
}

// ------------------------------------------------------------------ (c) A[x,y], C[x,y]: one workgroup per pair
__device__ __forceinline__ float row_dot(const float* __restrict__ a, const float* __restrict__ b, int Dl, int lane) {
  float d = 0.f;
  for (int k = lane; k < Dl; k += 64) d = fmaf(a[k], b[k], d);
  return warp_sum(d);
}
__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

__global__ __launch_bounds__(NTH) void fl_pair_kernel(FP p) {
  __shared__ float part[2][4];
  __shared__ float red[NTH / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int y = blockIdx.x, x = blockIdx.y, T = p.T, I = p.I, Dl = p.Dl;
  const int64_t pr = (int64_t)x * p.Bg + y;
  const uint8_t* mrow = p.mask + (int64_t)x * T;
  const float* tx = p.tn + (int64_t)x * T * Dl;
  const float* iy = p.in + (int64_t)y * I * Dl;
  float sa = 0.f, sc = 0.f, cn = 0.f;
  for (int t = w; t < T; t += 4)
    if (mrow[t]) sa += row_dot(tx + (int64_t)t * Dl, iy + (int64_t)clampi(p.idxT[pr * T + t], I) * Dl, Dl, lane);
  for (int i = w; i < I; i += 4)
    sc += row_dot(iy + (int64_t)i * Dl, tx + (int64_t)clampi(p.idxI[pr * I + i], T) * Dl, Dl, lane);
  for (int t = tid; t < T; t += NTH) cn += mrow[t] ? 1.f : 0.f;
  const float cnt = block_sum(cn, red);
  if (lane == 0) {
    part[0][w] = sa;
    part[1][w] = sc;
  }
  __syncthreads();
  if (tid == 0) {
    const float temp = expf(p.log_temp[0]);
    p.A[pr] = temp * (((part[0][0] + part[0][1]) + part[0][2]) + part[0][3]) / fmaxf(cnt, 1e-6f);
    p.C[pr] = temp * (((part[1][0] + part[1][1]) + part[1][2]) + part[1][3]) / (float)I;
  }
}

// ------------------------------------------------------------------ (d) the two Bg x Bg softmaxes
// d loss / d M[x,y] of one direction: e = exp(M[x,y]), rden = 1 / (denominator + 1e-20) of its row (or
// column); the decoupled loss leaves the diagonal out of the denominator
__device__ __forceinline__ float dcoef(int x, int y, float m, float rden, int dcl, float scale) {
  const float e = expf(m);
  float g = (dcl && x == y) ? 0.f : e * rden;
  if (x == y) g -= e / (e + 1e-20f);
  return g * scale;
}

__global__ __launch_bounds__(NTH) void fl_sums_kernel(FP p) {
  __shared__ float red[NTH / 64];
  const int k = threadIdx.x, Bg = p.Bg;
  float* rdA = p.den;
  float* rdC = p.den + Bg;
  float* cnt = p.den + 2 * Bg;
  float lpart = 0.f;
  if (k < Bg) {
    float c = 0.f;
    for (int t = 0; t < p.T; ++t) c += p.mask[(int64_t)k * p.T + t] ? 1.f : 0.f;
    cnt[k] = c;
    float da = 0.f, dc = 0.f;
    for (int j = 0; j < Bg; ++j) {
      if (p.dcl && j == k) continue;
      da += expf(p.A[k * Bg + j]);
      dc += expf(p.over_text ? p.C[j * Bg + k] : p.C[k * Bg + j]);   // over texts x for image k, or over images
    }
    rdA[k] = 1.f / (da + 1e-20f);
    rdC[k] = 1.f / (dc + 1e-20f);
    lpart = (-logf(expf(p.A[k * Bg + k]) + 1e-20f) + logf(da + 1e-20f)) +
            (-logf(expf(p.C[k * Bg + k]) + 1e-20f) + logf(dc + 1e-20f));
  }
  __syncthreads();
  float dpart = 0.f;
  const float scale = 0.5f / Bg;
  if (k < Bg)
    for (int j = 0; j < Bg; ++j) {
      const float a = p.A[k * Bg + j], c = p.C[k * Bg + j];
      dpart += dcoef(k, j, a, rdA[k], p.dcl, scale) * a + dcoef(k, j, c, rdC[p.over_text ? j : k], p.dcl, scale) * c;
    }
  const float tot = block_sum(lpart, red);
  const float dtot = block_sum(dpart, red);
  if (k == 0) {
    p.loss[0] = scale * tot;
    p.dlogtemp[0] = dtot;
  }
}

// ------------------------------------------------------------------ (e) gradients: one wave per token
template <bool TEXT>
__global__ __launch_bounds__(NTH) void fl_grad_kernel(FP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int Bg = p.Bg, T = p.T, I = p.I, Dl = p.Dl, n = TEXT ? T : I;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= (int64_t)Bg * n) return;
  const int b = (int)(r / n), tok = (int)(r - (int64_t)b * n);     // TEXT: (x, t); else (y, i)
  float* out = (TEXT ? p.dt : p.di) + r * Dl;
  if (TEXT && !p.mask[r]) {                                        // a masked text token takes no part
    for (int k = lane; k < Dl; k += 64) out[k] = 0.f;
    return;
  }
  const float* rdA = p.den;
  const float* rdC = p.den + Bg;
  const float* cnt = p.den + 2 * Bg;
  const float temp = expf(p.log_temp[0]), scale = 0.5f / Bg;
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.f;
  auto add_row = [&](const float* __restrict__ row, float wgt) {
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int k = lane + 64 * m;
      if (k < Dl) acc[m] = fmaf(wgt, row[k], acc[m]);
    }
  };
  for (int o = 0; o < Bg; ++o) {                                   // the other side's sample, ascending
    const int x = TEXT ? b : o, y = TEXT ? o : b;
    const int64_t pr = (int64_t)x * Bg + y;
    const float wa = dcoef(x, y, p.A[pr], rdA[x], p.dcl, scale) * temp / fmaxf(cnt[x], 1e-6f);
    const float wc = dcoef(x, y, p.C[pr], rdC[p.over_text ? y : x], p.dcl, scale) * temp / (float)I;
    const int* it = p.idxT + pr * T;
    const int* ii = p.idxI + pr * I;
    const uint8_t* mrow = p.mask + (int64_t)x * T;
    if (TEXT) {
      // A: this token's own winner; C: every image token whose winner this token is
      add_row(p.in + ((int64_t)y * I + clampi(it[tok], I)) * Dl, wa);
      for (int i0 = 0; i0 < I; i0 += 64) {
        const int i = i0 + lane;
        unsigned long long hit = __ballot(i < I && ii[i] == tok);
        while (hit) {
          const int l = __ffsll((long long)hit) - 1;
          hit &= hit - 1;
          add_row(p.in + ((int64_t)y * I + i0 + l) * Dl, wc);
        }
      }
    } else {
      // C: this token's own winner; A: every kept text token whose winner this token is
      add_row(p.tn + ((int64_t)x * T + clampi(ii[tok], T)) * Dl, wc);
      for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        unsigned long long hit = __ballot(t < T && mrow[t] && it[t] == tok);
        while (hit) {
          const int l = __ffsll((long long)hit) - 1;
          hit &= hit - 1;
          add_row(p.tn + ((int64_t)x * T + t0 + l) * Dl, wa);
        }
      }
    }
  }
  // l2norm backward (eps 1e-12: a zero row keeps g / 1e-12 finite)
  const float* self = (TEXT ? p.tn : p.in) + r * Dl;
  const float nn = p.nrm[TEXT ? r : (int64_t)Bg * T + r];
  float dotp = 0.f;
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    const int k = lane + 64 * m;
    if (k < Dl) dotp = fmaf(acc[m], self[k], dotp);
  }
  dotp = warp_sum(dotp);
  const float inv = 1.f / fmaxf(nn, 1e-12f);
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    const int k = lane + 64 * m;
    if (k < Dl) out[k] = nn > 1e-12f ? (acc[m] - self[k] * dotp) * inv : acc[m] * inv;
  }
}

bool shape_ok(const ctclip_filip_args* a) {
  return a->Bg >= 1 && a->Bg <= MAXBG && a->T >= 1 && a->T <= MAXT && a->I >= 1 && a->I <= MAXI && a->Dl >= 16 &&
         a->Dl <= MAXDL && a->Dl % 16 == 0;
}

}  // namespace

extern "C" int64_t ctclip_filip_ws_bytes(const ctclip_filip_args* a) {
  if (!a || !shape_ok(a)) return 0;
  return 4 * make_layout(a).total;
}

extern "C" int ctclip_filip_loss(const ctclip_filip_args* a, void* stream) {
  CT_REQUIRE(a != nullptr, CT_EINVAL);
  CT_REQUIRE(shape_ok(a), CT_ESHAPE);
  CT_REQUIRE(a->t_raw && a->i_raw && a->mask && a->log_temp && a->loss && a->dt_raw && a->di_raw && a->dlogtemp && a->ws,
             CT_EINVAL);
  CT_REQUIRE(aligned16(a->ws), CT_EALIGN);
  const Layout L = make_layout(a);
  CT_REQUIRE(a->ws_bytes >= 4 * L.total, CT_EINVAL);
  float* ws = (float*)a->ws;
  FP p;
  p.t_raw = a->t_raw; p.i_raw = a->i_raw; p.mask = a->mask; p.log_temp = a->log_temp;
  p.Bg = a->Bg; p.T = a->T; p.I = a->I; p.Dl = a->Dl; p.dcl = a->decoupled != 0; p.over_text = a->i2t_over_text != 0;
  p.loss = a->loss; p.dt = a->dt_raw; p.di = a->di_raw; p.dlogtemp = a->dlogtemp;
  p.A = a->A ? a->A : ws + L.A;
  p.C = a->C ? a->C : ws + L.C;
  p.idxT = a->idx_t2i ? a->idx_t2i : (int*)(ws + L.idxT);
  p.idxI = a->idx_i2t ? a->idx_i2t : (int*)(ws + L.idxI);
  p.tn = ws + L.tn; p.in = ws + L.in; p.nrm = ws + L.nrm; p.den = ws + L.den;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nt = (int64_t)p.Bg * p.T, ni = (int64_t)p.Bg * p.I;
  hipLaunchKernelGGL(fl_norm_kernel, dim3((unsigned)cdiv(nt + ni, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(fl_argmax_kernel<true>, dim3(cdiv(p.T, TB), p.Bg, p.Bg), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(fl_argmax_kernel<false>, dim3(cdiv(p.I, TB), p.Bg, p.Bg), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(fl_pair_kernel, dim3(p.Bg, p.Bg), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(fl_sums_kernel, dim3(1), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(fl_grad_kernel<true>, dim3((unsigned)cdiv(nt, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(fl_grad_kernel<false>, dim3((unsigned)cdiv(ni, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  return 0;
}
