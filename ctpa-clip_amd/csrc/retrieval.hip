// Retrieval evaluation (include/ctclip_hip.h, ctclip_retrieval_ranks / ctclip_retrieval_topk): how high
// does each query's own gallery row rank among all M gallery rows, and which are its k best rows -- the
// report-to-volume Recall@K of CT-CLIP's evaluation, without ever writing the N x M score matrix.
//
// Scores: S_ij = q^_i . g^_j of the l2-normalised latents (as lt_norm_kernel of loss_tiled.hip: sqrtf, a
// true division by max(norm, 1e-12)), on the f32 matrix pipe (v_mfma_f32_16x16x4_f32) in 64 x 64 tiles
// staged through LDS like pass (b) of loss_tiled.hip.  Each S_ij is ONE fma chain in ascending k, so its
// bits depend on neither the tile it falls in nor its place there; the pad columns (ldD = Dl rounded up
// to 4, the K step to 16) add fma(0, 0, acc) = acc.  The tie rule (equal scores: the lower gallery index
// first) rests on that: bit-equal gallery rows give bit-equal scores.
//
// ranks, three launches:
//   (a) rt_norm_kernel   q and g normalised once into the workspace; rank[] zeroed
//   (b) rt_own_kernel    own_i = S_i,pair_i: one wave per 16 queries runs the SAME MFMA chain on (its 16
//                        queries) x (their 16 positives) and keeps the diagonal -- the bits the tile pass
//                        produces for that element, whichever tile holds it
//   (c) rt_count_kernel  grid (column chunk, row tile): the workgroup walks its column tiles, every lane
//                        counts the j != pair_i of its elements with S_ij > own_i or (S_ij == own_i and
//                        j < pair_i); the counts are folded across the lanes of a row and added to rank[i]
//                        with one integer atomic per (row, wave): integer sums, any order, the same bits
// topk, two or three launches:
//   (a) rt_norm_kernel
//   (b) rt_topk_kernel   grid (column chunk, row tile): per tile the scores go to LDS and each wave takes 16
//                        rows: one ballot finds the scores that beat the row's k-th best, and those are
//                        inserted into the row's sorted list, which lives in LDS for the whole walk and in
//                        the wave's registers (one place per lane) while it is changed.  The gallery is
//                        walked in ascending j and an equal score never overtakes, so ties keep the
//                        ascending index.  One chunk: the lists are the result.  C > 1 chunks (more
//                        workgroups than row tiles alone give): partial lists [N][C][k] in the workspace,
//                        unfilled places marked
//   (c) rt_merge_kernel  one thread per row: C-way merge of the sorted partial lists, the lower chunk first
//                        among equal scores (chunks are ascending ranges of j)
//
// Workspace (bytes, every segment 16-B aligned; ldD = Dl rounded up to 4):
//   ranks: qn [N][ldD] f32 | gn [M][ldD] f32 | own [N] f32
//   topk:  qn [N][ldD] f32 | gn [M][ldD] f32 | ps [N][C][k] f32 | pi [N][C][k] i32   (ps / pi only if C > 1)
#include "common.h"
#include "retrieval_tile.h"
#include "../../include/ctclip_hip.h"

namespace {

using namespace rtile;

constexpr int MAXROWS = 65536, MAXDL = 8192, MAXK = 128, MAXC = 16;
constexpr int NO_IDX = 0x7fffffff;   // an unfilled place of a partial list

struct RP {
  const float* q; const float* g; const int32_t* pair;
  int N, M, Dl, k;
  int C, span;                    // column chunks and the column tiles of one chunk
  int64_t ldD;
  float* qn; float* gn; float* own;
  float* ps; int32_t* pi;
  int32_t* rank; float* score; int32_t* idx;
};

// ------------------------------------------------------------------ (a) normalise: one wave per row
__global__ __launch_bounds__(NTH) void rt_norm_kernel(RP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= (int64_t)p.N + p.M) return;
  const bool isq = r < p.N;
  const int64_t a = isq ? r : r - p.N;
  norm_row((isq ? p.q : p.g) + a * p.Dl, (isq ? p.qn : p.gn) + a * p.ldD, p.Dl, (int)p.ldD);
  if (isq && lane == 0 && p.rank) p.rank[a] = 0;
}

// (a pair entry outside [0, M) is the caller's error: it is read as row 0, never out of bounds)
__device__ __forceinline__ int pair_of(const RP& p, int i) {
  const int v = p.pair[i];
  return (unsigned)v < (unsigned)p.M ? v : 0;
}

// ------------------------------------------------------------------ (b) own scores: one wave per 16 queries
__global__ __launch_bounds__(NTH) void rt_own_kernel(RP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const int i = (blockIdx.x * 4 + w) * 16 + r16;
  const bool ok = i < p.N;
  const float* a_row = p.qn + (int64_t)(ok ? i : 0) * p.ldD;
  const float* b_row = p.gn + (int64_t)(ok ? pair_of(p, i) : 0) * p.ldD;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // the tile pass's operand order and k order: slot l & 15 of the first operand is the gallery row, of
  // the second the query; D[4 g + r][l & 15] -> the diagonal sits in lane (m, g = m / 4), register m % 4
  for (int k4 = 0; k4 < (int)p.ldD; k4 += 4) {
    const float a = ok ? a_row[k4 + g] : 0.f, b = ok ? b_row[k4 + g] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b, a, acc, 0, 0, 0);
  }
  if (ok && g == (r16 >> 2)) {
    const int r = r16 & 3;
    p.own[i] = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
  }
}

// ------------------------------------------------------------------ (c) count the rows ranked above
__global__ __launch_bounds__(NTH) void rt_count_kernel(RP p) {
  __shared__ __attribute__((aligned(16))) float smem[TILE_SMEM];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  const int r16 = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.y * TB;
  const int nTc = (p.M + TB - 1) / TB;
  const int t0 = blockIdx.x * p.span, t1 = min(t0 + p.span, nTc);
  float own[2];
  int pr[2], cnt[2] = {0, 0};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int gi = i0 + wm * 32 + i * 16 + r16;
    own[i] = gi < p.N ? p.own[gi] : 0.f;
    pr[i] = gi < p.N ? pair_of(p, gi) : 0;
  }
  for (int tl = t0; tl < t1; ++tl) {
    const int j0 = tl * TB;
    f32x4 acc[2][2];
    score_tile(p, i0, j0, smem, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gj = j0 + wn * 32 + j * 16 + 4 * g + r;
          const float s = acc[i][j][r];
          cnt[i] += (gj < p.M && gj != pr[i] && (s > own[i] || (s == own[i] && gj < pr[i]))) ? 1 : 0;
        }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int c = cnt[i];
    c += __shfl_xor(c, 16, 64);
    c += __shfl_xor(c, 32, 64);
    const int gi = i0 + wm * 32 + i * 16 + r16;
    if (g == 0 && gi < p.N && c) atomicAdd(&p.rank[gi], c);
  }
}

// ------------------------------------------------------------------ (b) top-k lists
// A row's list is k places sorted by (score descending, index ascending), unfilled places (-inf, NO_IDX)
// at the end, so it is always "full" and its last place is the threshold a new score must beat.  Wave w
// owns tile rows 16 w .. 16 w + 15; per tile and row, lane c holds the score of column c, one ballot
// finds the columns above the threshold, and each of those (ascending c) is inserted with the list in
// registers -- place l in lane l (and 64 + l with KCAP = 128): the insert position is the count of
// places >= the score (an equal earlier score stays ahead), everything behind moves up one lane.
template <int KCAP>
__global__ __launch_bounds__(NTH) void rt_topk_kernel(RP p) {
  constexpr int LDL = KCAP + 1;
  constexpr bool TWO = KCAP > 64;
  __shared__ __attribute__((aligned(16))) float smem[TILE_SMEM];
  __shared__ float Ss[TB][TB + 1];
  __shared__ float ls[TB * LDL];
  __shared__ int li[TB * LDL];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int r16 = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.y * TB, k = p.k;
  const int nTc = (p.M + TB - 1) / TB;
  const int t0 = blockIdx.x * p.span, t1 = min(t0 + p.span, nTc);
  const float NEG = -__builtin_huge_valf();
  for (int e = t; e < TB * LDL; e += NTH) {
    ls[e] = NEG;
    li[e] = NO_IDX;
  }
  // (the first barrier inside score_tile orders this before any list is read)
  for (int tl = t0; tl < t1; ++tl) {
    const int j0 = tl * TB;
    f32x4 acc[2][2];
    score_tile(p, i0, j0, smem, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ss[wm * 32 + i * 16 + r16][wn * 32 + j * 16 + 4 * g + r] = acc[i][j][r];
    __syncthreads();
    for (int rr = 0; rr < 16; ++rr) {      // every branch below is wave-uniform
      const int row = w * 16 + rr;
      if (i0 + row >= p.N) break;
      float* ms = ls + row * LDL;
      int* mi = li + row * LDL;
      const float s = Ss[row][lane];
      float thr = ms[k - 1];
      unsigned long long mask = __ballot(j0 + lane < p.M && s > thr);
      if (!mask) continue;
      float e0 = ms[lane], e1 = TWO ? ms[64 + lane] : NEG;
      int x0 = mi[lane], x1 = TWO ? mi[64 + lane] : NO_IDX;
      while (mask) {                       // ascending j: an equal score stays behind the earlier one
        const int c = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const float sc = __shfl(s, c, 64);
        if (!(sc > thr)) continue;
        int pos = __popcll(__ballot(lane < k && e0 >= sc));
        if (TWO) pos += __popcll(__ballot(64 + lane < k && e1 >= sc));
        const float u0 = __shfl_up(e0, 1, 64);
        const int v0 = __shfl_up(x0, 1, 64);
        if (TWO) {
          const float u1 = __shfl_up(e1, 1, 64), c0 = __shfl(e0, 63, 64);
          const int v1 = __shfl_up(x1, 1, 64), d0 = __shfl(x0, 63, 64);
          const int t1p = 64 + lane;
          const float m1 = lane == 0 ? c0 : u1;
          const int n1 = lane == 0 ? d0 : v1;
          e1 = t1p < pos ? e1 : t1p == pos ? sc : m1;
          x1 = t1p < pos ? x1 : t1p == pos ? j0 + c : n1;
        }
        e0 = lane < pos ? e0 : lane == pos ? sc : u0;
        x0 = lane < pos ? x0 : lane == pos ? j0 + c : v0;
        thr = (!TWO || k <= 64) ? __shfl(e0, k - 1, 64) : __shfl(e1, k - 65, 64);
      }
      ms[lane] = e0;
      mi[lane] = x0;
      if (TWO) {
        ms[64 + lane] = e1;
        mi[64 + lane] = x1;
      }
    }
    __syncthreads();
  }
  const bool direct = p.C == 1;
  for (int e = t; e < TB * k; e += NTH) {
    const int row = e / k, q = e - row * k, gi = i0 + row;
    if (gi >= p.N) break;
    const float s = ls[row * LDL + q];
    const int ix = li[row * LDL + q];
    if (direct) {
      p.score[(int64_t)gi * k + q] = s;
      p.idx[(int64_t)gi * k + q] = ix;
    } else {
      const int64_t o = ((int64_t)gi * p.C + blockIdx.x) * k + q;
      p.ps[o] = s;
      p.pi[o] = ix;
    }
  }
}

// ------------------------------------------------------------------ (c) merge the chunks' lists
__global__ __launch_bounds__(64) void rt_merge_kernel(RP p) {
  __shared__ float hs[MAXC][64];
  __shared__ int hi[MAXC][64];
  __shared__ int hp[MAXC][64];
  const int t = threadIdx.x, i = blockIdx.x * 64 + t, k = p.k, C = p.C;
  if (i >= p.N) return;
  const float* ps = p.ps + (int64_t)i * C * k;
  const int32_t* pi = p.pi + (int64_t)i * C * k;
  for (int c = 0; c < C; ++c) {
    hp[c][t] = 0;
    hs[c][t] = ps[(int64_t)c * k];
    hi[c][t] = pi[(int64_t)c * k];
  }
  for (int q = 0; q < k; ++q) {
    int best = -1;
    float bs = 0.f;
    for (int c = 0; c < C; ++c)            // ascending chunks: the lower j wins among equal scores
      if (hi[c][t] != NO_IDX && (best < 0 || hs[c][t] > bs)) {
        best = c;
        bs = hs[c][t];
      }
    p.score[(int64_t)i * k + q] = best < 0 ? -__builtin_huge_valf() : bs;
    p.idx[(int64_t)i * k + q] = best < 0 ? NO_IDX : hi[best][t];
    if (best < 0) continue;
    const int np = ++hp[best][t];
    hs[best][t] = np < k ? ps[(int64_t)best * k + np] : 0.f;
    hi[best][t] = np < k ? pi[(int64_t)best * k + np] : NO_IDX;
  }
}

bool shape_ok(int64_t N, int64_t M, int64_t Dl) {
  return N >= 1 && N <= MAXROWS && M >= 1 && M <= MAXROWS && Dl >= 1 && Dl <= MAXDL;
}

struct Layout {
  int64_t qn, gn, own, ps, pi, total;   // byte offsets
};
inline int64_t up16(int64_t x) { return (x + 15) & ~(int64_t)15; }
inline Layout make_layout(int64_t N, int64_t M, int64_t Dl, int64_t C, int64_t k) {
  Layout L;
  const int64_t ldD = up4(Dl);
  int64_t o = 0;
  L.qn = o;  o += up16(4 * N * ldD);
  L.gn = o;  o += up16(4 * M * ldD);
  L.own = o; o += k ? 0 : up16(4 * N);
  L.ps = o;  o += (k && C > 1) ? up16(4 * N * C * k) : 0;
  L.pi = o;  o += (k && C > 1) ? up16(4 * N * C * k) : 0;
  L.total = o;
  return L;
}

void fill(RP& p, const float* q, const float* g, int N, int M, int Dl, int k, void* ws, const Layout& L) {
  p.q = q; p.g = g; p.pair = nullptr;
  p.N = N; p.M = M; p.Dl = Dl; p.k = k;
  p.ldD = up4(Dl);
  char* b = (char*)ws;
  p.qn = (float*)(b + L.qn); p.gn = (float*)(b + L.gn); p.own = (float*)(b + L.own);
  p.ps = (float*)(b + L.ps); p.pi = (int32_t*)(b + L.pi);
  p.rank = nullptr; p.score = nullptr; p.idx = nullptr;
}

}  // namespace

extern "C" int64_t ctclip_retrieval_ranks_ws_bytes(int32_t N, int32_t M, int32_t Dl) {
  if (!shape_ok(N, M, Dl)) return 0;
  return make_layout(N, M, Dl, 1, 0).total;
}

extern "C" int ctclip_retrieval_ranks(const float* q, const float* g, const int32_t* pair, int32_t N, int32_t M,
                                      int32_t Dl, int32_t* rank, void* ws, int64_t ws_bytes, void* stream) {
  CT_REQUIRE(shape_ok(N, M, Dl), CT_ESHAPE);
  CT_REQUIRE(q && g && pair && rank && ws, CT_EINVAL);
  CT_REQUIRE(aligned16(ws), CT_EALIGN);
  const Layout L = make_layout(N, M, Dl, 1, 0);
  CT_REQUIRE(ws_bytes >= L.total, CT_EINVAL);
  RP p;
  fill(p, q, g, N, M, Dl, 0, ws, L);
  p.pair = pair;
  p.rank = rank;
  chunks(N, M, 1024, MAXROWS, &p.C, &p.span);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rt_norm_kernel, dim3((unsigned)cdiv((int64_t)N + M, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(rt_own_kernel, dim3((unsigned)cdiv(N, 64)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(rt_count_kernel, dim3(p.C, cdiv(N, TB)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t ctclip_retrieval_topk_ws_bytes(int32_t N, int32_t M, int32_t Dl, int32_t k) {
  if (!shape_ok(N, M, Dl) || k < 1 || k > MAXK || k > M) return 0;
  int C, span;
  chunks(N, M, 512, MAXC, &C, &span);
  return make_layout(N, M, Dl, C, k).total;
}

extern "C" int ctclip_retrieval_topk(const float* q, const float* g, int32_t N, int32_t M, int32_t Dl, int32_t k,
                                     float* score, int32_t* idx, void* ws, int64_t ws_bytes, void* stream) {
  CT_REQUIRE(shape_ok(N, M, Dl) && k >= 1 && k <= MAXK && k <= M, CT_ESHAPE);
  CT_REQUIRE(q && g && score && idx && ws, CT_EINVAL);
  CT_REQUIRE(aligned16(ws), CT_EALIGN);
  int C, span;
  chunks(N, M, 512, MAXC, &C, &span);
  const Layout L = make_layout(N, M, Dl, C, k);
  CT_REQUIRE(ws_bytes >= L.total, CT_EINVAL);
  RP p;
  fill(p, q, g, N, M, Dl, k, ws, L);
  p.C = C; p.span = span;
  p.score = score;
  p.idx = idx;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rt_norm_kernel, dim3((unsigned)cdiv((int64_t)N + M, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  const dim3 grid(C, cdiv(N, TB));
  if (k <= 64)
    hipLaunchKernelGGL(rt_topk_kernel<64>, grid, dim3(NTH), 0, st, p);
  else
    hipLaunchKernelGGL(rt_topk_kernel<MAXK>, grid, dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  if (C > 1) {
    hipLaunchKernelGGL(rt_merge_kernel, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, st, p);
    CT_CHECK_LAUNCH();
  }
  return 0;
}
