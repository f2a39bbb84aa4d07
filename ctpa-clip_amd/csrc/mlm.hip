// Masked language modelling on the text tower (include/ctclip_hip.h, ctclip_mlm_*): the masking rule of
// ct_clip/mlm.py (get_mask_subset_with_prob) on a hash stream, and a cross-entropy head that only ever sees
// the SELECTED rows -- M = B * ceil(mask_prob * L) of the B * L hidden rows.
//
//   mlm_mask_kernel     one workgroup per sequence, thread l owns position l: the eligible positions' keys
//                       (32 hash bits | l, so no two are equal) go to LDS, a position's rank is the number of
//                       smaller keys, the c_b = ceil(mask_prob * n_b) lowest ranks are selected and slot
//                       `rank` of the row's selection list takes the flat index; the other slots get -1, so
//                       the host knows every later shape (M rows) without reading anything back
//   mlm_gather_kernel   the selected hidden rows as the A operand of the logits GEMM (a zero row for -1): a
//                       bf16 image and the bf16 image of what it drops (hi + lo, ~16 mantissa bits)
//   (ctclip_gemm)       logits [M][ld] f32 = A . W^T + bias on the padded bf16 weight shadows (ld = V rounded
//                       up to 8: the GEMM's 16-B row chunks; pad rows of W and pad bias entries are zero),
//                       as A_hi (W_hi + W_lo)^T + A_lo W_hi^T: single bf16 operands put the loss ~2e-3 off
//   mlm_prep_kernel     one workgroup: target[m] (the label, or -1 for an invalid row) and the valid-row count
//   mlm_ce_kernel       one workgroup per row: ONE pass over V with a running maximum per thread -> (max, sum)
//                       pairs folded in a fixed order (xor butterfly, then the four waves in turn) -> lse;
//                       row loss = lse - logit[label]; the row is then overwritten with (softmax - onehot) /
//                       count, in f32 in place and in bf16 for the backward GEMMs
//   mlm_finish_kernel   one workgroup: loss = (row losses summed in a fixed order) / count; 0 / 0 = NaN when no
//                       row is valid, as F.cross_entropy gives for targets that are all ignored
//   mlm_scatter_kernel  dH [B L][D] = 0 (a memset node), then the selected rows' gradients by plain stores
//
// No float atomics anywhere and every reduction order is fixed: the same inputs give the same bits.
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int MAXL = 512, MAXIGN = 32, NTH = 256;
constexpr int MAXM = 1 << 20;

__device__ __forceinline__ uint64_t mlm_hash(uint64_t seed, uint64_t s, uint64_t i) {
  uint64_t x = (seed ^ (s * 0xBF58476D1CE4E5B9ull)) ^ (i * 0x9E3779B97F4A7C15ull);
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

struct MP {
  ctclip_mlm_mask_args a;
  uint64_t t_replace, t_random;   // floor(p * 2^32)
};

__device__ __forceinline__ bool mlm_ignored(const MP& p, int64_t id) {
  bool ig = id == p.a.pad_token_id;
  for (int k = 0; k < p.a.n_ignore; ++k) ig |= id == p.a.ignore[k];
  return ig;
}

// blockDim = L rounded up to 64 (<= 512)
__global__ __launch_bounds__(MAXL) void mlm_mask_kernel(MP p) {
  __shared__ uint64_t keys[MAXL];
  const int t = threadIdx.x, b = blockIdx.x, L = p.a.L, m_max = p.a.m_max;
  const bool in = t < L;
  const int64_t gi = (int64_t)b * L + t;
  const int64_t id = in ? p.a.ids[gi] : p.a.pad_token_id;
  const bool elig = in && !mlm_ignored(p, id);
  const uint64_t key = elig ? (((mlm_hash(p.a.seed, 0, (uint64_t)gi) >> 32) << 32) | (uint64_t)t) : ~0ull;
  keys[t] = key;
  const int n_b = __syncthreads_count(elig);          // (also orders the key stores before the reads)
  const int c_b = min((int)ceil((double)n_b * p.a.mask_prob), m_max);
  int rank = 0;
  if (elig)
    for (int j = 0; j < L; ++j) rank += keys[j] < key ? 1 : 0;
  const bool selected = elig && rank < c_b;
  if (in) {
    int64_t out = id;
    bool rnd = false;
    if (p.t_random) {     // ct_clip/mlm.py:83-90: every position, eligible or not
      const uint64_t tok = ((mlm_hash(p.a.seed, 3, (uint64_t)gi) >> 32) * (uint64_t)p.a.num_tokens) >> 32;
      rnd = (mlm_hash(p.a.seed, 2, (uint64_t)gi) >> 32) < p.t_random && !mlm_ignored(p, (int64_t)tok);
      if (rnd) out = (int64_t)tok;
    }
    if (selected && !rnd && (mlm_hash(p.a.seed, 1, (uint64_t)gi) >> 32) < p.t_replace) out = p.a.mask_token_id;
    p.a.masked_ids[gi] = out;
    p.a.labels[gi] = selected ? id : p.a.pad_token_id;
  }
  if (selected) p.a.sel[(int64_t)b * m_max + rank] = (int32_t)gi;
  if (t < m_max && t >= c_b) p.a.sel[(int64_t)b * m_max + t] = -1;     // (m_max <= L <= blockDim)
}

__global__ __launch_bounds__(NTH) void mlm_gather_kernel(const float* __restrict__ hidden, int64_t ldh, int64_t R,
                                                         const int32_t* __restrict__ sel, int D,
                                                         u16* __restrict__ out, u16* __restrict__ out_lo,
                                                         int64_t ldo) {
  const int m = blockIdx.x;
  const int64_t s = sel[m];
  const bool ok = s >= 0 && s < R;
  const float* src = hidden + (ok ? s : 0) * ldh;
  for (int c = threadIdx.x * 4; c < D; c += NTH * 4) {      // D % 8 == 0, rows 16-B aligned
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (ok) *(f32x4*)v = *(const f32x4*)(src + c);
    *(uint2*)(out + (int64_t)m * ldo + c) = pack4(v);
    if (out_lo) {      // the part of the row the bf16 image drops: x = hi + lo to ~16 mantissa bits
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] -= bf2f(f2bf(v[e]));
      *(uint2*)(out_lo + (int64_t)m * ldo + c) = pack4(v);
    }
  }
}

struct CP {
  float* logits; u16* dlb; int64_t ld;
  const int32_t* sel; const int64_t* labels; int64_t R;
  int M, V;
  float* loss; float* count;
  int32_t* target; float* rowloss; float* cnt;      // workspace
};

__global__ __launch_bounds__(NTH) void mlm_prep_kernel(CP p) {
  __shared__ int red[NTH / 64];
  const int t = threadIdx.x;
  int n = 0;
  for (int m = t; m < p.M; m += NTH) {
    const int64_t s = p.sel[m];
    int32_t tgt = -1;
    if (s >= 0 && s < p.R) {
      const int64_t lab = p.labels[s];
      if (lab >= 0 && lab < p.V) tgt = (int32_t)lab;
    }
    p.target[m] = tgt;
    n += tgt >= 0 ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((t & 63) == 0) red[t >> 6] = n;
  __syncthreads();
  if (t == 0) {
    int tot = 0;
    for (int w = 0; w < NTH / 64; ++w) tot += red[w];
    p.cnt[0] = (float)tot;
    p.count[0] = (float)tot;
  }
}

// (max, sum of exp(. - max)) of two disjoint sets; symmetric in its arguments bit for bit
__device__ __forceinline__ void lse_fold(float& m, float& s, float m2, float s2) {
  const float NEG = -__builtin_huge_valf();
  const float mm = fmaxf(m, m2);
  const float a = m == NEG ? 0.f : s * expf(m - mm);
  const float b = m2 == NEG ? 0.f : s2 * expf(m2 - mm);
  m = mm;
  s = a + b;
}

__global__ __launch_bounds__(NTH) void mlm_ce_kernel(CP p) {
  __shared__ float rm[NTH / 64], rs[NTH / 64];
  __shared__ float zt;
  const int t = threadIdx.x, m = blockIdx.x, V = p.V;
  const int tgt = p.target[m];
  float* z = p.logits + (int64_t)m * p.ld;
  u16* zb = p.dlb + (int64_t)m * p.ld;
  if (tgt < 0) {     // (uniform over the workgroup)
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = t * 4; c < (int)p.ld; c += NTH * 4) {
      *(f32x4*)(z + c) = f32x4{0.f, 0.f, 0.f, 0.f};
      *(uint2*)(zb + c) = pack4(zero);
    }
    if (t == 0) p.rowloss[m] = 0.f;
    return;
  }
  const float NEG = -__builtin_huge_valf();
  float mx = NEG, s = 0.f;
  for (int c = t * 4; c < V; c += NTH * 4) {
    float v[4];
    *(f32x4*)v = *(const f32x4*)(z + c);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < V) {
        if (v[e] > mx) {
          s = s * expf(mx - v[e]) + 1.f;      // (mx = -inf: s = 0 * 0 + 1)
          mx = v[e];
        } else {
          s += expf(v[e] - mx);
        }
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(mx, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_fold(mx, s, m2, s2);
  }
  if ((t & 63) == 0) {
    rm[t >> 6] = mx;
    rs[t >> 6] = s;
  }
  if (t == 0) zt = z[tgt];
  __syncthreads();
  mx = rm[0];
  s = rs[0];
  for (int w = 1; w < NTH / 64; ++w) lse_fold(mx, s, rm[w], rs[w]);
  const float lse = mx + logf(s);
  if (t == 0) p.rowloss[m] = lse - zt;
  const float inv = 1.f / p.cnt[0];
  for (int c = t * 4; c < (int)p.ld; c += NTH * 4) {
    float v[4];
    *(f32x4*)v = *(const f32x4*)(z + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = c + e < V ? (expf(v[e] - lse) - (c + e == tgt ? 1.f : 0.f)) * inv : 0.f;
    *(f32x4*)(z + c) = *(const f32x4*)v;
    *(uint2*)(zb + c) = pack4(v);
  }
}

__global__ __launch_bounds__(NTH) void mlm_finish_kernel(CP p) {
  __shared__ float red[NTH / 64];
  float s = 0.f;
  for (int m = threadIdx.x; m < p.M; m += NTH) s += p.rowloss[m];
  s = block_sum(s, red);
  if (threadIdx.x == 0) p.loss[0] = s / p.cnt[0];
}

__global__ __launch_bounds__(NTH) void mlm_scatter_kernel(const float* __restrict__ dsel, int64_t lds,
                                                          const int32_t* __restrict__ sel, int D,
                                                          float* __restrict__ dh, int64_t ldh, int64_t R) {
  const int m = blockIdx.x;
  const int64_t s = sel[m];
  if (s < 0 || s >= R) return;
  for (int c = threadIdx.x * 4; c < D; c += NTH * 4)
    *(f32x4*)(dh + s * ldh + c) = *(const f32x4*)(dsel + (int64_t)m * lds + c);
}

inline int64_t up16(int64_t x) { return (x + 15) & ~(int64_t)15; }
inline bool prob_ok(double p) { return p >= 0.0 && p <= 1.0; }

}  // namespace

extern "C" int ctclip_mlm_mask(const ctclip_mlm_mask_args* a, void* stream) {
  CT_REQUIRE(a, CT_EINVAL);
  CT_REQUIRE(a->L >= 1 && a->L <= MAXL && a->B >= 1 && a->m_max >= 1 && a->m_max <= a->L && a->n_ignore >= 0 &&
                 a->n_ignore <= MAXIGN && (int64_t)a->B * a->L <= 0x7fffffff,
             CT_ESHAPE);
  CT_REQUIRE(a->ids && a->masked_ids && a->labels && a->sel && prob_ok(a->mask_prob) && prob_ok(a->replace_prob) &&
                 prob_ok(a->random_token_prob) && a->num_tokens >= 1 && a->num_tokens <= 0x7fffffff,
             CT_EINVAL);
  MP p;
  p.a = *a;
  p.t_replace = (uint64_t)(a->replace_prob * 4294967296.0);
  p.t_random = (uint64_t)(a->random_token_prob * 4294967296.0);
  hipLaunchKernelGGL(mlm_mask_kernel, dim3(a->B), dim3((a->L + 63) / 64 * 64), 0, (hipStream_t)stream, p);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_mlm_gather(const float* hidden, int64_t ldh, int64_t R, const int32_t* sel, int32_t M, int32_t D,
                                 void* out, void* out_lo, int64_t ldo, void* stream) {
  CT_REQUIRE(M >= 1 && M <= MAXM && D >= 8 && R >= 1, CT_ESHAPE);
  CT_REQUIRE(hidden && sel && out && ldh >= D && ldo >= D, CT_EINVAL);
  CT_REQUIRE(D % 8 == 0 && ldh % 4 == 0 && ldo % 8 == 0 && aligned16(hidden) && aligned16(out) && aligned16(out_lo),
             CT_EALIGN);
  hipLaunchKernelGGL(mlm_gather_kernel, dim3(M), dim3(NTH), 0, (hipStream_t)stream, hidden, ldh, R, sel, D, (u16*)out,
                     (u16*)out_lo, ldo);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t ctclip_mlm_ce_ws_bytes(int32_t M) {
  if (M < 1 || M > MAXM) return 0;
  return 2 * up16(4 * (int64_t)M) + 16;     // target [M] i32 | row loss [M] f32 | count f32
}

extern "C" int ctclip_mlm_ce(float* logits, void* dlogits_bf16, int64_t ld, const int32_t* sel, const int64_t* labels,
                             int64_t R, int32_t M, int32_t V, float* loss, float* count, void* ws, int64_t ws_bytes,
                             void* stream) {
  CT_REQUIRE(M >= 1 && M <= MAXM && V >= 1 && R >= 1 && ld >= V && ld <= 0x7fffffff, CT_ESHAPE);
  CT_REQUIRE(logits && dlogits_bf16 && sel && labels && loss && count && ws && ws_bytes >= ctclip_mlm_ce_ws_bytes(M),
             CT_EINVAL);
  CT_REQUIRE(ld % 8 == 0 && aligned16(logits) && aligned16(dlogits_bf16) && aligned16(ws), CT_EALIGN);
  CP p;
  p.logits = logits; p.dlb = (u16*)dlogits_bf16; p.ld = ld;
  p.sel = sel; p.labels = labels; p.R = R;
  p.M = M; p.V = V;
  p.loss = loss; p.count = count;
  char* b = (char*)ws;
  p.target = (int32_t*)b;
  p.rowloss = (float*)(b + up16(4 * (int64_t)M));
  p.cnt = (float*)(b + 2 * up16(4 * (int64_t)M));
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mlm_prep_kernel, dim3(1), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(mlm_ce_kernel, dim3(M), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  hipLaunchKernelGGL(mlm_finish_kernel, dim3(1), dim3(NTH), 0, st, p);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_mlm_scatter(const float* dsel, int64_t lds, const int32_t* sel, int32_t M, int32_t D, float* dh,
                                  int64_t ldh, int64_t R, void* stream) {
  CT_REQUIRE(M >= 1 && M <= MAXM && D >= 4 && R >= 1, CT_ESHAPE);
  CT_REQUIRE(dsel && sel && dh && lds >= D && ldh == D, CT_EINVAL);
  CT_REQUIRE(D % 4 == 0 && lds % 4 == 0 && aligned16(dsel) && aligned16(dh), CT_EALIGN);
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(dh, 0, (size_t)R * D * sizeof(float), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(mlm_scatter_kernel, dim3(M), dim3(NTH), 0, st, dsel, lds, sel, D, dh, ldh, R);
  CT_CHECK_LAUNCH();
  return 0;
}
