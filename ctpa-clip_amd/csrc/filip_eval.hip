// Evaluation of a use_all_token_embeds model (include/ctclip_hip.h, ctclip_filip_scores, ctclip_score_ranks):
// the token-wise scores of filip.hip, forward only, for an UNPAIRED rectangle of R reports x V volumes,
//   S[x,y,t,i] = temp <tn[x,t], in[y,i]>                                   (unit latents, eps 1e-12)
//   A[x,y] = sum_t mask[x,t] max_i S / max(sum_t mask[x,t], 1e-6)          (text -> image)
//   C[x,y] = (1 / I) sum_i max_{t : mask[x,t]} S                            (image -> text)
// and optionally every kept text token's winning image token (lowest index on ties) with its score.
// ONE product feeds both directions: a workgroup owns a whole (x, y) pair, so it sees every row and every
// column of the pair's score tile.  S is never written.
// Launch plan (two launches, no waiting between workgroups, no float atomics):
//   (a) fs_norm_kernel   one wave per token: the image tokens l2-normalised into the workspace; a KEPT text
//                        token normalised into slot (number of kept tokens before it) of its report, so the
//                        kept tokens of a report are contiguous rows; per report the count and the ascending
//                        list of kept positions (a ballot prefix over the mask row, no host read)
//   (b) fs_score_kernel  grid (V, R), one workgroup per pair: the kept text tokens in 64-row strips against
//                        the I image tokens in 64-column tiles on v_mfma_f32_16x16x4_f32 (exact f32, one fma
//                        chain in ascending k per score; the K-contiguous double-buffered LDS pipeline of
//                        filip.hip).  Row maxima (value, lowest index) run in registers across a strip's
//                        column tiles and are folded in ascending t into the A sum; column maxima live in an
//                        I-float LDS array across the strips and are summed at the end: 16-element blocks in
//                        ascending i, then the block sums in ascending order.
// Every sum has an order fixed by the pair alone: the bits of A[x,y], C[x,y], idx and val depend only on
// report x and volume y -- not on R, V or the pair's place in the call -- and two runs give the same bits.
//
// Workspace (4-byte words): tn [R][T][Dl] (the first count rows of each report) | in [V][I][Dl] |
// cnt [R] int32 | kept [R][T] int32 (cnt and kept rounded up to a multiple of 4).
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int MAXRV = 65535, MAXT = 512, MAXI = 1024, MAXDL = 512;
constexpr int TB = 64;            // rows / columns of a score tile
constexpr int KT = 16;            // K step
constexpr int LDR = 20;           // K-contiguous LDS image [row][16 k]: 16-B aligned rows, 64 lanes on 64 banks
constexpr int NTH = 256;
constexpr int CB = 16;            // block of the column-max sum

struct Layout {
  int64_t tn, in, cnt, kept, total;
};

inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }

inline Layout make_layout(const ctclip_filip_scores_args* a) {
  const int64_t R = a->R, V = a->V, T = a->T, I = a->I, Dl = a->Dl;
  Layout L;
  int64_t o = 0;
  L.tn = o;   o += R * T * Dl;
  L.in = o;   o += V * I * Dl;
  L.cnt = o;  o += up4(R);
  L.kept = o; o += up4(R * T);
  L.total = o;
  return L;
}

struct SP {
  const float* t_raw; const float* i_raw; const uint8_t* mask; const float* log_temp;
  int R, V, T, I, Dl;
  float* A; float* C; int* idx; float* val;       // idx, val: null when not wanted
  float* tn; float* in; int* cnt; int* kept;      // workspace
};

// ------------------------------------------------------------------ (a) normalise: one wave per token
__global__ __launch_bounds__(NTH) void fs_norm_kernel(SP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t nt = (int64_t)p.R * p.T, r = (int64_t)blockIdx.x * 4 + w;
  if (r >= nt + (int64_t)p.V * p.I) return;
  const float* src;
  float* dst;
  if (r < nt) {
    const int x = (int)(r / p.T), t = (int)(r - (int64_t)x * p.T);
    const uint8_t* mrow = p.mask + (int64_t)x * p.T;
    int pos = 0;                                     // kept tokens before t
    for (int c0 = 0; c0 < t; c0 += 64) pos += __popcll(__ballot(c0 + lane < t && mrow[c0 + lane]));
    const bool keep = mrow[t] != 0;
    if (t == p.T - 1 && lane == 0) p.cnt[x] = pos + (keep ? 1 : 0);
    if (!keep) return;
    if (lane == 0) p.kept[(int64_t)x * p.T + pos] = t;
    src = p.t_raw + r * p.Dl;
    dst = p.tn + ((int64_t)x * p.T + pos) * p.Dl;
  } else {
    src = p.i_raw + (r - nt) * p.Dl;
    dst = p.in + (r - nt) * p.Dl;
  }
  float q = 0.f;
  for (int k = lane; k < p.Dl; k += 64) q += src[k] * src[k];
  q = warp_sum(q);
  const float inv = 1.f / fmaxf(sqrtf(q), 1e-12f);
  for (int k = lane; k < p.Dl; k += 64) dst[k] = src[k] * inv;
}

// ------------------------------------------------------------------ (b) one pair per workgroup
// one 16-B chunk of a 64-row x 16-k K-contiguous tile: row t / 4, k quad t % 4.  Rows past the row count
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

__global__ __launch_bounds__(NTH) void fs_score_kernel(SP p) {
  __shared__ __attribute__((aligned(16))) float smem[4 * TB * LDR];   // [buf][text | image]
  __shared__ float colmax[MAXI];
  __shared__ float cm[2][TB];
  __shared__ float rv[2][TB];
  __shared__ int ri[2][TB];
  __shared__ float part[MAXI / CB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
  const int y = blockIdx.x, x = blockIdx.y, T = p.T, I = p.I, Dl = p.Dl;
  const int64_t pr = (int64_t)x * p.V + y;
  const int n = min(max(p.cnt[x], 0), T);            // kept tokens of the report
  const float* P = p.tn + (int64_t)x * T * Dl;
  const float* Q = p.in + (int64_t)y * I * Dl;
  const int* kp = p.kept + (int64_t)x * T;
  const float temp = expf(p.log_temp[0]);
  for (int i = tid; i < I; i += NTH) colmax[i] = -INFINITY;
  if (p.idx || p.val) {
    const uint8_t* mrow = p.mask + (int64_t)x * T;
    for (int t = tid; t < T; t += NTH)
      if (!mrow[t]) {
        if (p.idx) p.idx[pr * T + t] = -1;
        if (p.val) p.val[pr * T + t] = 0.f;
      }
  }
  __syncthreads();
  const int r16 = lane & 15, g = lane >> 4, nk = Dl / KT;
  float asum = 0.f;                                  // thread 0: the row maxima in ascending t
  for (int s0 = 0; s0 < n; s0 += TB) {
    float best[2] = {-INFINITY, -INFINITY};
    int bidx[2] = {0, 0};
    for (int q0 = 0; q0 < I; q0 += TB) {
      f32x4 acc[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 ra = kload(P, Dl, n, s0, 0), rb = kload(Q, Dl, I, q0, 0);
      kwrite(smem, ra);
      kwrite(smem + TB * LDR, rb);
      __syncthreads();
      for (int kt = 0; kt < nk; ++kt) {
        const float* As = smem + (kt & 1) * 2 * TB * LDR;
        const float* Bs = As + TB * LDR;
        if (kt + 1 < nk) {
          ra = kload(P, Dl, n, s0, (kt + 1) * KT);
          rb = kload(Q, Dl, I, q0, (kt + 1) * KT);
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
      // lane: strip row wm*32 + 16 i + r16, tile columns wn*32 + 16 j + 4 g + [0, 4), taken in ascending order
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int gq = q0 + wn * 32 + j * 16 + 4 * g + r;
            const float v = acc[i][j][r];
            if (gq < I && v > best[i]) {
              best[i] = v;
              bidx[i] = gq;
            }
          }
      // column maxima over the strip's live rows: the wave's 32 rows, then its two row halves through LDS
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float m = -INFINITY;
#pragma unroll
          for (int i = 0; i < 2; ++i)
            if (s0 + wm * 32 + i * 16 + r16 < n) m = fmaxf(m, acc[i][j][r]);
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
          if (r16 == 0) cm[wm][wn * 32 + j * 16 + 4 * g + r] = m;
        }
      __syncthreads();
      if (tid < TB && q0 + tid < I) colmax[q0 + tid] = fmaxf(colmax[q0 + tid], fmaxf(cm[0][tid], cm[1][tid]));
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
    if (tid < TB && s0 + tid < n) {
      float v = rv[0][tid];
      int ix = ri[0][tid];
      take_better(v, ix, rv[1][tid], ri[1][tid]);
      rv[0][tid] = v;
      const int t = min(max(kp[s0 + tid], 0), T - 1);
      if (p.idx) p.idx[pr * T + t] = ix;
      if (p.val) p.val[pr * T + t] = temp * v;
    }
    __syncthreads();
    if (tid == 0) {
      const int live = min(TB, n - s0);
      for (int r = 0; r < live; ++r) asum += rv[0][r];
    }
    __syncthreads();
  }
  // C: blocks of CB column maxima in ascending i, then the block sums in ascending order
  if (tid < ((I + CB - 1) / CB)) {
    float s = 0.f;
    const int e = min(I, (tid + 1) * CB);
    for (int i = tid * CB; i < e; ++i) s += colmax[i];
    part[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    float c = 0.f;
    const int nb = ((I + CB - 1) / CB);
    for (int b = 0; b < nb; ++b) c += part[b];
    p.A[pr] = temp * asum / fmaxf((float)n, 1e-6f);
    p.C[pr] = temp * c / (float)I;
  }
}

// ------------------------------------------------------------------ ranks from a ready score matrix
// one wave per query: integer counts of the gallery entries that come before the positive
__global__ __launch_bounds__(NTH) void score_ranks_kernel(const float* __restrict__ S, const int* __restrict__ pair,
                                                          int N, int M, int* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= N) return;
  int pp = pair[q];
  if (pp < 0 || pp >= M) pp = 0;                     // the caller's duty; never a read out of bounds
  const float* row = S + q * M;
  const float sp = row[pp];
  int c = 0;
  for (int j = lane; j < M; j += 64) {
    const float s = row[j];
    c += (j != pp && (s > sp || (s == sp && j < pp))) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) rank[q] = c;
}

bool shape_ok(const ctclip_filip_scores_args* a) {
  return a->R >= 1 && a->R <= MAXRV && a->V >= 1 && a->V <= MAXRV && a->T >= 1 && a->T <= MAXT && a->I >= 1 &&
         a->I <= MAXI && a->Dl >= 16 && a->Dl <= MAXDL && a->Dl % 16 == 0;
}

}  // namespace

extern "C" int64_t ctclip_filip_scores_ws_bytes(const ctclip_filip_scores_args* a) {
  if (!a || !shape_ok(a)) return 0;
  return 4 * make_layout(a).total;
}

extern "C" int ctclip_filip_scores(const ctclip_filip_scores_args* a, void* stream) {
  CT_REQUIRE(a != nullptr, CT_EINVAL);
  CT_REQUIRE(shape_ok(a), CT_ESHAPE);
  CT_REQUIRE(a->t_raw && a->i_raw && a->mask && a->log_temp && a->A && a->C && a->ws, CT_EINVAL);
  CT_REQUIRE(aligned16(a->ws), CT_EALIGN);
  const Layout L = make_layout(a);
  CT_REQUIRE(a->ws_bytes >= 4 * L.total, CT_EINVAL);
  float* ws = (float*)a->ws;
  SP p;
  p.t_raw = a->t_raw; p.i_raw = a->i_raw; p.mask = a->mask; p.log_temp = a->log_temp;
  p.R = a->R; p.V = a->V; p.T = a->T; p.I = a->I; p.Dl = a->Dl;
  p.A = a->A; p.C = a->C; p.idx = a->idx_t2i; p.val = a->val_t2i;
  p.tn = ws + L.tn; p.in = ws + L.in; p.cnt = (int*)(ws + L.cnt); p.kept = (int*)(ws + L.kept);
  const hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)p.R * p.T + (int64_t)p.V * p.I;
  hipLaunchKernelGGL(fs_norm_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(fs_score_kernel, dim3(p.V, p.R), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_score_ranks(const float* S, const int32_t* pair, int32_t N, int32_t M, int32_t* rank,
                                  void* stream) {
  CT_REQUIRE(N >= 1 && M >= 1, CT_ESHAPE);
  CT_REQUIRE(S && pair && rank, CT_EINVAL);
  hipLaunchKernelGGL(score_ranks_kernel, dim3((unsigned)cdiv(N, 4)), dim3(NTH), 0, (hipStream_t)stream, S, pair, N, M,
                     rank);
  CT_CHECK_LAUNCH();
  return 0;
}
