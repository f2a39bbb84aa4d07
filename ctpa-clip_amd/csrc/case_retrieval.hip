// Volume-to-volume ("case") retrieval scored by pathology labels (include/ctclip_hip.h,
// ctclip_case_retrieval): each query's K_max best VISIBLE gallery rows, and from the labels of those rows
// hits@K, AP@K and the graded (Jaccard) gain@K, in one pass that never writes the N x M score matrix.
//
// Inputs: q [N][Dl], g [M][Dl] raw f32 latents (may be one buffer); qlab [N], glab [M] int64 label
// bitmasks (bit c = label c present); qgrp [N], ggrp [M] int32 group ids or both null; ks [nK] strictly
// ascending, 1 <= nK <= 8, K_max = ks[nK - 1] <= 128; rel_mode 0 = any, 1 = exact.
//
// Scores: S_ij = q^_i . g^_j exactly as retrieval.hip makes them -- the normalise step and the score tile
// are the code of retrieval_tile.h, so an entry's bits depend only on its two rows.
// Exclusion: gallery row j is invisible to query i iff qgrp != null && qgrp[i] >= 0 && ggrp[j] == qgrp[i]
// (self-exclusion: qgrp = ggrp = arange).
// List of query i: the first n_i = min(K_max, visible_i) visible rows by descending score, ties by
// ascending gallery index; unfilled places hold idx = -1, score = 0.
// Relevance of row j to query i, a = qlab[i], b = glab[j]:
//   any:   (a & b) != 0 || (a == 0 && b == 0)        exact: a == b
//   graded, always Jaccard: J = popcount(a & b) / popcount(a | b), an f64 division; 1.0 when a | b == 0
// Outputs per query: idx / score [N][K_max]; filled [N] = n_i; nrel [N] = R_i, the relevant rows among ALL
// visible gallery rows; and per K_a, with m = min(K_a, n_i) and h_r = the relevant among the first r:
//   hits [N][nK] = h_m
//   ap   [N][nK] = (sum_{r = 1..m, rel_r} (double)h_r / (double)r) / (double)min(K_a, R_i), summed in
//                  ascending r; -1.0 when R_i == 0 or n_i == 0
//   gain [N][nK] = sum_{r = 1..m} J_r in ascending r, NOT divided
// Every float operation has a fixed order: an f64 restatement on idx reproduces ap and gain bit for bit.
//
// Three launches:
//   (a) cr_norm_kernel    q and g normalised into the workspace (once when q == g); nrel[] zeroed
//   (b) cr_walk_kernel    grid (column chunk, row tile), rt_topk_kernel's walk.  Per tile the 64 columns'
//                         label and group words are staged in LDS beside the tile; in the epilogue every
//                         lane tests visibility and relevance of its 2 x 8 elements and counts the relevant
//                         visible ones, folded over the four lanes of a row and added to nrel[i] with one
//                         integer atomic per (row, wave).  The list update is rt_topk's ballot-and-insert
//                         with the visibility test in the ballot: an excluded column never reaches a list.
//                         Every chunk writes its partial lists [N][C][K_max] (also with C == 1)
//   (c) cr_finish_kernel  one thread per row: C-way merge of the partial lists, the lower chunk first among
//                         equal scores; glab[idx] gathered; hits, ap and gain of every K_a written in the
//                         same ascending walk of the list
// No float atomics, integer sums only: the same bits on every run.
//
// Workspace (bytes, every segment 16-B aligned; ldD = Dl rounded up to 4):
//   qn [N][ldD] f32 | gn [M][ldD] f32 | ps [N][C][K_max] f32 | pi [N][C][K_max] i32
// (qn is unused when q == g; the size does not depend on it)
#include "common.h"
#include "retrieval_tile.h"
#include "../../include/ctclip_hip.h"

namespace {

using namespace rtile;

constexpr int MAXROWS = 65536, MAXDL = 8192, MAXK = 128, MAXC = 16, MAXNK = 8;
constexpr int NO_IDX = 0x7fffffff;   // an unfilled place of a partial list

struct CP {
  const float* q; const float* g;
  const int64_t* qlab; const int64_t* glab;
  const int32_t* qgrp; const int32_t* ggrp;
  int N, M, Dl, k;                  // k = K_max
  int nq;                           // query rows to normalise: N, or 0 when q == g (qn == gn then)
  int C, span;
  int nK, rel_mode;
  int ks[MAXNK];
  int64_t ldD;
  float* qn; float* gn;
  float* ps; int32_t* pi;
  int32_t* idx; float* score; int32_t* filled; int32_t* nrel; int32_t* hits;
  double* ap; double* gain;
};

__device__ __forceinline__ bool relevant(int64_t a, int64_t b, int mode) {
  return mode ? a == b : ((a & b) != 0 || (a | b) == 0);
}

// ------------------------------------------------------------------ (a) normalise: one wave per row
__global__ __launch_bounds__(NTH) void cr_norm_kernel(CP p) {
  const int w = threadIdx.x >> 6;
  const int64_t tid = (int64_t)blockIdx.x * NTH + threadIdx.x;   // the grid has at least N threads
  if (tid < p.N) p.nrel[tid] = 0;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= (int64_t)p.nq + p.M) return;
  const bool isq = r < p.nq;
  const int64_t a = isq ? r : r - p.nq;
  norm_row((isq ? p.q : p.g) + a * p.Dl, (isq ? p.qn : p.gn) + a * p.ldD, p.Dl, (int)p.ldD);
}

// ------------------------------------------------------------------ (b) tile walk: counts and partial lists
// The lists are rt_topk_kernel's (retrieval.hip): k places sorted by (score descending, index ascending),
// unfilled places (-inf, NO_IDX) at the end; wave w owns tile rows 16 w .. 16 w + 15, lane c holds the
// score of column c, one ballot finds the visible columns above the row's threshold and each of those
// (ascending c) is inserted with the list in registers, place l in lane l (and 64 + l with KCAP = 128).
template <int KCAP>
__global__ __launch_bounds__(NTH) void cr_walk_kernel(CP p) {
  constexpr int LDL = KCAP + 1;
  constexpr bool TWO = KCAP > 64;
  __shared__ __attribute__((aligned(16))) float smem[TILE_SMEM];
  __shared__ float Ss[TB][TB + 1];
  __shared__ float ls[TB * LDL];
  __shared__ int li[TB * LDL];
  __shared__ long long cl[TB];     // label words of the tile's columns
  __shared__ int cg[TB];           // their group ids
  __shared__ int rg[TB];           // group ids of the rows; -1: nothing is excluded
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
  if (t < TB) rg[t] = (p.qgrp && i0 + t < p.N) ? p.qgrp[i0 + t] : -1;
  int64_t qa[2];
  int qg[2], cnt[2] = {0, 0};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int gi = i0 + wm * 32 + i * 16 + r16;
    qa[i] = gi < p.N ? p.qlab[gi] : 0;
    qg[i] = (p.qgrp && gi < p.N) ? p.qgrp[gi] : -1;
  }
  // (the first barrier inside score_tile orders the LDS writes above and below before any read)
  for (int tl = t0; tl < t1; ++tl) {
    const int j0 = tl * TB;
    if (t < TB) {
      const int gj = j0 + t;
      cl[t] = gj < p.M ? p.glab[gj] : 0;
      cg[t] = (p.ggrp && gj < p.M) ? p.ggrp[gj] : 0;
    }
    f32x4 acc[2][2];
    score_tile(p, i0, j0, smem, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = wn * 32 + j * 16 + 4 * g + r;
          const bool vis = j0 + c < p.M && !(qg[i] >= 0 && cg[c] == qg[i]);
          cnt[i] += (vis && relevant(qa[i], cl[c], p.rel_mode)) ? 1 : 0;
          Ss[wm * 32 + i * 16 + r16][c] = acc[i][j][r];
        }
    __syncthreads();
    for (int rr = 0; rr < 16; ++rr) {      // every branch below is wave-uniform
      const int row = w * 16 + rr;
      if (i0 + row >= p.N) break;
      float* ms = ls + row * LDL;
      int* mi = li + row * LDL;
      const float s = Ss[row][lane];
      const int qgr = rg[row];
      float thr = ms[k - 1];
      unsigned long long mask = __ballot(j0 + lane < p.M && !(qgr >= 0 && cg[lane] == qgr) && s > thr);
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
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int c = cnt[i];
    c += __shfl_xor(c, 16, 64);
    c += __shfl_xor(c, 32, 64);
    const int gi = i0 + wm * 32 + i * 16 + r16;
    if (g == 0 && gi < p.N && c) atomicAdd(&p.nrel[gi], c);
  }
  for (int e = t; e < TB * k; e += NTH) {
    const int row = e / k, q = e - row * k, gi = i0 + row;
    if (gi >= p.N) break;
    const int64_t o = ((int64_t)gi * p.C + blockIdx.x) * k + q;
    p.ps[o] = ls[row * LDL + q];
    p.pi[o] = li[row * LDL + q];
  }
}

// ------------------------------------------------------------------ (c) merge the chunks' lists, score them
__global__ __launch_bounds__(64) void cr_finish_kernel(CP p) {
  __shared__ float hs[MAXC][64];
  __shared__ int hi[MAXC][64];
  __shared__ int hp[MAXC][64];
  const int t = threadIdx.x, i = blockIdx.x * 64 + t, k = p.k, C = p.C, nK = p.nK;
  if (i >= p.N) return;
  const float* ps = p.ps + (int64_t)i * C * k;
  const int32_t* pi = p.pi + (int64_t)i * C * k;
  for (int c = 0; c < C; ++c) {
    hp[c][t] = 0;
    hs[c][t] = ps[(int64_t)c * k];
    hi[c][t] = pi[(int64_t)c * k];
  }
  const int64_t a = p.qlab[i];
  const int R = p.nrel[i];
  int n = 0, h = 0;
  double aps = 0.0, gs = 0.0;
  for (int q = 0; q < k; ++q) {
    int best = -1;
    float bs = 0.f;
    for (int c = 0; c < C; ++c)            // ascending chunks: the lower j wins among equal scores
      if (hi[c][t] != NO_IDX && (best < 0 || hs[c][t] > bs)) {
        best = c;
        bs = hs[c][t];
      }
    p.score[(int64_t)i * k + q] = best < 0 ? 0.f : bs;
    p.idx[(int64_t)i * k + q] = best < 0 ? -1 : hi[best][t];
    if (best >= 0) {
      const int64_t b = p.glab[hi[best][t]];
      ++n;
      if (relevant(a, b, p.rel_mode)) {
        ++h;
        aps += (double)h / (double)(q + 1);
      }
      const int un = __popcll((unsigned long long)(a | b));
      gs += un ? (double)__popcll((unsigned long long)(a & b)) / (double)un : 1.0;
      const int np = ++hp[best][t];
      hs[best][t] = np < k ? ps[(int64_t)best * k + np] : 0.f;
      hi[best][t] = np < k ? pi[(int64_t)best * k + np] : NO_IDX;
    }
    // the places behind n_i change nothing, so the state at place K_a is the one of m = min(K_a, n_i)
#pragma unroll
    for (int ka = 0; ka < MAXNK; ++ka)
      if (ka < nK && p.ks[ka] == q + 1) {
        const int64_t o = (int64_t)i * nK + ka;
        p.hits[o] = h;
        p.ap[o] = (R == 0 || n == 0) ? -1.0 : aps / (double)min(q + 1, R);
        p.gain[o] = gs;
      }
  }
  p.filled[i] = n;
}

bool shape_ok(int64_t N, int64_t M, int64_t Dl) {
  return N >= 1 && N <= MAXROWS && M >= 1 && M <= MAXROWS && Dl >= 1 && Dl <= MAXDL;
}

struct Layout {
  int64_t qn, gn, ps, pi, total;   // byte offsets
};
inline int64_t up16(int64_t x) { return (x + 15) & ~(int64_t)15; }
inline Layout make_layout(int64_t N, int64_t M, int64_t Dl, int64_t C, int64_t k) {
  Layout L;
  const int64_t ldD = up4(Dl);
  int64_t o = 0;
  L.qn = o; o += up16(4 * N * ldD);
  L.gn = o; o += up16(4 * M * ldD);
  L.ps = o; o += up16(4 * N * C * k);
  L.pi = o; o += up16(4 * N * C * k);
  L.total = o;
  return L;
}

}  // namespace

extern "C" int64_t ctclip_case_retrieval_ws_bytes(int32_t N, int32_t M, int32_t Dl, int32_t Kmax) {
  if (!shape_ok(N, M, Dl) || Kmax < 1 || Kmax > MAXK) return 0;
  int C, span;
  chunks(N, M, 512, MAXC, &C, &span);
  return make_layout(N, M, Dl, C, Kmax).total;
}

extern "C" int ctclip_case_retrieval(const float* q, const float* g, const int64_t* qlab, const int64_t* glab,
                                     const int32_t* qgrp, const int32_t* ggrp, int32_t N, int32_t M, int32_t Dl,
                                     const int32_t* ks, int32_t nK, int32_t rel_mode, int32_t* idx, float* score,
                                     int32_t* filled, int32_t* nrel, int32_t* hits, double* ap, double* gain,
                                     void* ws, int64_t ws_bytes, void* stream) {
  CT_REQUIRE(shape_ok(N, M, Dl), CT_ESHAPE);
  CT_REQUIRE(q && g && qlab && glab && ks && idx && score && filled && nrel && hits && ap && gain && ws, CT_EINVAL);
  CT_REQUIRE((qgrp == nullptr) == (ggrp == nullptr), CT_EINVAL);
  CT_REQUIRE(nK >= 1 && nK <= MAXNK && (rel_mode == 0 || rel_mode == 1), CT_EINVAL);
  CT_REQUIRE(ks[0] >= 1, CT_EINVAL);
  for (int a = 1; a < nK; ++a) CT_REQUIRE(ks[a] > ks[a - 1], CT_EINVAL);
  const int k = ks[nK - 1];
  CT_REQUIRE(k <= MAXK, CT_ESHAPE);
  CT_REQUIRE(aligned16(ws), CT_EALIGN);
  CP p;
  p.q = q; p.g = g; p.qlab = qlab; p.glab = glab; p.qgrp = qgrp; p.ggrp = ggrp;
  p.N = N; p.M = M; p.Dl = Dl; p.k = k;
  p.ldD = up4(Dl);
  chunks(N, M, 512, MAXC, &p.C, &p.span);
  const Layout L = make_layout(N, M, Dl, p.C, k);
  CT_REQUIRE(ws_bytes >= L.total, CT_EINVAL);
  p.nK = nK; p.rel_mode = rel_mode;
  for (int a = 0; a < MAXNK; ++a) p.ks[a] = a < nK ? ks[a] : 0;
  char* b = (char*)ws;
  const bool same = q == g && N == M;
  p.nq = same ? 0 : N;
  p.gn = (float*)(b + L.gn);
  p.qn = same ? p.gn : (float*)(b + L.qn);
  p.ps = (float*)(b + L.ps); p.pi = (int32_t*)(b + L.pi);
  p.idx = idx; p.score = score; p.filled = filled; p.nrel = nrel; p.hits = hits; p.ap = ap; p.gain = gain;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cr_norm_kernel, dim3((unsigned)cdiv((int64_t)p.nq + M, 4)), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  const dim3 grid(p.C, cdiv(N, TB));
  if (k <= 64)
    hipLaunchKernelGGL(cr_walk_kernel<64>, grid, dim3(NTH), 0, st, p);
  else
    hipLaunchKernelGGL(cr_walk_kernel<MAXK>, grid, dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(cr_finish_kernel, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, st, p);
  CT_CHECK_LAUNCH();
  return 0;
}
