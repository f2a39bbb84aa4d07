// Image x text similarity + symmetric InfoNCE (ct_clip/ct_clip.py:771,796,845-901), fused
// forward + backward in one workgroup.  Exactly the reference's formula: no max subtraction,
// log(x + 1e-20), mean over rows, both directions averaged.  Inputs are the RAW projected
// latents of the (all-gathered) global batch; the kernel l2-normalises them (F.normalize,
// eps 1e-12, ct_clip.py:771) and returns d(loss)/d(raw latents) for every row.
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int MAXB = 128;

// 1,024 threads: the per-row passes (2 Bg rows) and the Bg^2 dot products spread over 16 waves
// (with 4 waves each walked 4 rows / 16 dots in sequence: ~110 us in the step, on its critical path)
constexpr int CL_NT = 1024, CL_NW = CL_NT / 64;
__global__ __launch_bounds__(CL_NT) void clip_loss_kernel(const float* __restrict__ t_raw, const float* __restrict__ i_raw,
                                                        int Bg, int Dl, const float* __restrict__ log_temp,
                                                        float* __restrict__ tn, float* __restrict__ in_,
                                                        float* __restrict__ loss_out, float* __restrict__ dt_raw,
                                                        float* __restrict__ di_raw, float* __restrict__ dlogtemp,
                                                        float* __restrict__ sim_out) {
  __shared__ float S[MAXB][MAXB + 1];
  __shared__ float tnorm[MAXB], inorm[MAXB], rs[MAXB], cs[MAXB], red[CL_NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float temp = __expf(log_temp[0]);
  // 1. norms (one wave per row)
  for (int r = w; r < 2 * Bg; r += CL_NW) {
    const float* src = r < Bg ? t_raw + (int64_t)r * Dl : i_raw + (int64_t)(r - Bg) * Dl;
    float s = 0.f;
    for (int k = lane; k < Dl; k += 64) s += src[k] * src[k];
    s = warp_sum(s);
    const float n = sqrtf(s);
    const float inv = 1.f / fmaxf(n, 1e-12f);
    float* dst = r < Bg ? tn + (int64_t)r * Dl : in_ + (int64_t)(r - Bg) * Dl;
    for (int k = lane; k < Dl; k += 64) dst[k] = src[k] * inv;
    if (lane == 0) { if (r < Bg) tnorm[r] = n; else inorm[r - Bg] = n; }
  }
  __syncthreads();
  // 2. S = temp * tn . in^T
  for (int e = w; e < Bg * Bg; e += CL_NW) {
    const int i = e / Bg, j = e - i * Bg;
    float s = 0.f;
    for (int k = lane; k < Dl; k += 64) s += tn[(int64_t)i * Dl + k] * in_[(int64_t)j * Dl + k];
    s = warp_sum(s);
    if (lane == 0) S[i][j] = s * temp;
  }
  __syncthreads();
  // 3. exp, row / column sums
  for (int e = tid; e < Bg * Bg; e += CL_NT) {
    const int i = e / Bg, j = e - i * Bg;
    if (sim_out) sim_out[e] = S[i][j];
  }
  __syncthreads();
  for (int e = tid; e < Bg * Bg; e += CL_NT) {
    const int i = e / Bg, j = e - i * Bg;
    S[i][j] = __expf(S[i][j]);
  }
  __syncthreads();
  if (tid < Bg) {
    float r = 0.f, c = 0.f;
    for (int j = 0; j < Bg; ++j) { r += S[tid][j]; c += S[j][tid]; }
    rs[tid] = r;
    cs[tid] = c;
  }
  __syncthreads();
  float part = 0.f;
  if (tid < Bg) {
    const float e = S[tid][tid];
    part = (-__logf(e + 1e-20f) + __logf(rs[tid] + 1e-20f)) + (-__logf(e + 1e-20f) + __logf(cs[tid] + 1e-20f));
  }
  const float tot = block_sum(part, red);
  if (tid == 0) loss_out[0] = 0.5f * tot / Bg;
  __syncthreads();
  // 4. dS (stored in place over exp(S)); dlogtemp = sum dS * S  (S = log(E))
  const float c0 = 0.5f / Bg;
  float dlt = 0.f;
  for (int e = tid; e < Bg * Bg; e += CL_NT) {
    const int i = e / Bg, j = e - i * Bg;
    const float E = S[i][j];
    float d = E / (rs[i] + 1e-20f) + E / (cs[j] + 1e-20f);
    if (i == j) d -= 2.f * E / (E + 1e-20f);
    d *= c0;
    dlt += d * __logf(E);
    S[i][j] = d;  // safe: every thread reads only its own elements after the sums
  }
  const float dltot = block_sum(dlt, red);
  if (tid == 0 && dlogtemp) dlogtemp[0] = dltot;
  __syncthreads();
  // 5. d tn_i = temp * sum_j dS_ij in_j ; d in_j = temp * sum_i dS_ij tn_i ; then through l2norm
  for (int r = w; r < 2 * Bg; r += CL_NW) {
    const bool is_t = r < Bg;
    const int a = is_t ? r : r - Bg;
    const float* self = is_t ? tn + (int64_t)a * Dl : in_ + (int64_t)a * Dl;
    const float* other = is_t ? in_ : tn;
    float* out = is_t ? dt_raw + (int64_t)a * Dl : di_raw + (int64_t)a * Dl;
    const float n = is_t ? tnorm[a] : inorm[a];
    // pass 1: dot(self, dn)
    float dotp = 0.f;
    for (int k = lane; k < Dl; k += 64) {
      float g = 0.f;
      for (int b = 0; b < Bg; ++b) g += (is_t ? S[a][b] : S[b][a]) * other[(int64_t)b * Dl + k];
      g *= temp;
      out[k] = g;
      dotp += g * self[k];
    }
    dotp = warp_sum(dotp);
    const float inv = 1.f / fmaxf(n, 1e-12f);
    for (int k = lane; k < Dl; k += 64) {
      const float g = out[k];
      out[k] = n > 1e-12f ? (g - self[k] * dotp) * inv : g * inv;
    }
  }
}

__global__ void clip_scores_kernel(const float* __restrict__ t_raw, const float* __restrict__ i_raw, int B, int Dl,
                                   const float* __restrict__ log_temp, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = w; b < B; b += 4) {
    float tt = 0.f, ii = 0.f, ti = 0.f;
    for (int k = lane; k < Dl; k += 64) {
      const float x = t_raw[(int64_t)b * Dl + k], y = i_raw[(int64_t)b * Dl + k];
      tt += x * x; ii += y * y; ti += x * y;
    }
    tt = warp_sum(tt); ii = warp_sum(ii); ti = warp_sum(ti);
    if (lane == 0) out[b] = ti / (fmaxf(sqrtf(tt), 1e-12f) * fmaxf(sqrtf(ii), 1e-12f)) * __expf(log_temp[0]);
  }
}

// Zero-shot scoring (ct_clip/ctclip_inference.py:305-315 over the eval branch ct_clip.py:805-807):
// one workgroup per image row n; the image latent is l2-normalised once, then every wave takes
// prompt pairs j: s = temp * <t_norm, i_norm> for "present" (row 2j) and "not present" (2j+1),
// prob = softmax over the pair, entry 0.  The image latent stays in LDS; F.normalize eps 1e-12.
__global__ __launch_bounds__(256) void zero_shot_kernel(const float* __restrict__ t_raw, const float* __restrict__ i_raw,
                                                        int P, int Dl, const float* __restrict__ log_temp,
                                                        float* __restrict__ scores, float* __restrict__ probs) {
  extern __shared__ float img[];
  __shared__ float red[4];
  const int n = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float ii = 0.f;
  for (int k = threadIdx.x; k < Dl; k += 256) {
    const float y = i_raw[(int64_t)n * Dl + k];
    img[k] = y;
    ii += y * y;
  }
  ii = warp_sum(ii);
  if (lane == 0) red[w] = ii;
  __syncthreads();
  const float inorm = fmaxf(sqrtf(red[0] + red[1] + red[2] + red[3]), 1e-12f);
  const float temp = expf(log_temp[0]);
  for (int j = w; j < P; j += 4) {
    float s[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float* t = t_raw + (int64_t)(2 * j + e) * Dl;
      float tt = 0.f, ti = 0.f;
      for (int k = lane; k < Dl; k += 64) {
        const float x = t[k];
        tt += x * x;
        ti += x * img[k];
      }
      tt = warp_sum(tt);
      ti = warp_sum(ti);
      s[e] = ti / (fmaxf(sqrtf(tt), 1e-12f) * inorm) * temp;
    }
    if (lane == 0) {
      const float m = fmaxf(s[0], s[1]), e0 = expf(s[0] - m), e1 = expf(s[1] - m);
      scores[((int64_t)n * P + j) * 2] = s[0];
      scores[((int64_t)n * P + j) * 2 + 1] = s[1];
      probs[(int64_t)n * P + j] = e0 / (e0 + e1);
    }
  }
}

// The general loss of ct_clip/ct_clip.py:845-899 (include/ctclip_hip.h, ctclip_clip_loss_ex): one
// workgroup per view pair p = m * Vi + n, the passes of clip_loss_kernel above in the same order (so
// the plain instance <false, false> reproduces it bit for bit).  EXTRA: the image -> text direction has
// its own latent pair and its own matrix S[1] (2 x 128 x 129 f32 = 132 KiB of the CU's 160 KiB LDS);
// DCL: the diagonal leaves both denominators.  Latent sets s: 0 text, 1 image, 2 / 3 the extra pair.
// The pair's workspace slice: [NS][Bg][Dl] normalised latents, [NS][Bg][Dl] gradients w.r.t. the raw
// latents (unweighted), then its loss and d loss / d log-temp.
template <bool EXTRA, bool DCL>
__global__ __launch_bounds__(CL_NT) void clip_loss_ex_kernel(const float* __restrict__ t_raw, const float* __restrict__ i_raw,
                                                           const float* __restrict__ t_ex, const float* __restrict__ i_ex,
                                                           int Vi, int Bg, int Dl, const float* __restrict__ log_temp,
                                                           float* __restrict__ ws, int64_t per_pair) {
  constexpr int NM = EXTRA ? 2 : 1, NS = 2 * NM;
  __shared__ float S[NM][MAXB][MAXB + 1];
  __shared__ float nrm[NS][MAXB], rs[MAXB], cs[MAXB], red[CL_NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int p = blockIdx.x, m = p / Vi, n = p - m * Vi;
  const int64_t set = (int64_t)Bg * Dl;
  float* nv = ws + (int64_t)p * per_pair;
  float* gv = nv + NS * set;
  float* sc = gv + NS * set;
  const float temp = __expf(log_temp[0]);
  // 1. norms (one wave per row)
  for (int r = w; r < NS * Bg; r += CL_NW) {
    const int s = r / Bg, a = r - s * Bg;
    const float* base = s == 0 ? t_raw + m * set : s == 1 ? i_raw + n * set : s == 2 ? t_ex + m * set : i_ex + n * set;
    const float* src = base + (int64_t)a * Dl;
    float q = 0.f;
    for (int k = lane; k < Dl; k += 64) q += src[k] * src[k];
    q = warp_sum(q);
    const float nn = sqrtf(q);
    const float inv = 1.f / fmaxf(nn, 1e-12f);
    float* dst = nv + s * set + (int64_t)a * Dl;
    for (int k = lane; k < Dl; k += 64) dst[k] = src[k] * inv;
    if (lane == 0) nrm[s][a] = nn;
  }
  __syncthreads();
  // 2. S[q] = temp * tn . in^T of latent pair q (text rows, image columns for both directions)
  for (int q = 0; q < NM; ++q) {
    const float* tn = nv + 2 * q * set;
    const float* in_ = tn + set;
    for (int e = w; e < Bg * Bg; e += CL_NW) {
      const int i = e / Bg, j = e - i * Bg;
      float s = 0.f;
      for (int k = lane; k < Dl; k += 64) s += tn[(int64_t)i * Dl + k] * in_[(int64_t)j * Dl + k];
      s = warp_sum(s);
      if (lane == 0) S[q][i][j] = s * temp;
    }
  }
  __syncthreads();
  // 3. exp, row sums of the text -> image matrix, column sums of the image -> text one
  for (int q = 0; q < NM; ++q)
    for (int e = tid; e < Bg * Bg; e += CL_NT) {
      const int i = e / Bg, j = e - i * Bg;
      S[q][i][j] = __expf(S[q][i][j]);
    }
  __syncthreads();
  if (tid < Bg) {
    float r = 0.f, c = 0.f;
    for (int j = 0; j < Bg; ++j) {
      if (DCL && j == tid) continue;
      r += S[0][tid][j];
      c += S[NM - 1][j][tid];
    }
    rs[tid] = r;
    cs[tid] = c;
  }
  __syncthreads();
  float part = 0.f;
  if (tid < Bg) {
    const float e = S[0][tid][tid], e2 = S[NM - 1][tid][tid];
    part = (-__logf(e + 1e-20f) + __logf(rs[tid] + 1e-20f)) + (-__logf(e2 + 1e-20f) + __logf(cs[tid] + 1e-20f));
  }
  const float tot = block_sum(part, red);
  if (tid == 0) sc[0] = 0.5f * tot / Bg;
  __syncthreads();
  // 4. dS in place over exp(S); dlogtemp = sum dS * S  (S = log(E))
  const float c0 = 0.5f / Bg;
  float dlt = 0.f;
  for (int e = tid; e < Bg * Bg; e += CL_NT) {
    const int i = e / Bg, j = e - i * Bg;
    if (!EXTRA) {
      const float E = S[0][i][j];
      float d = E / (rs[i] + 1e-20f) + E / (cs[j] + 1e-20f);
      if (DCL && i == j) d = 0.f;
      if (i == j) d -= 2.f * E / (E + 1e-20f);
      d *= c0;
      dlt += d * __logf(E);
      S[0][i][j] = d;  // safe: every thread reads only its own elements after the sums
    } else {
      const float E1 = S[0][i][j], E2 = S[NM - 1][i][j];
      float d1 = E1 / (rs[i] + 1e-20f), d2 = E2 / (cs[j] + 1e-20f);
      if (DCL && i == j) d1 = d2 = 0.f;
      if (i == j) {
        d1 -= E1 / (E1 + 1e-20f);
        d2 -= E2 / (E2 + 1e-20f);
      }
      d1 *= c0;
      d2 *= c0;
      dlt += d1 * __logf(E1);
      dlt += d2 * __logf(E2);
      S[0][i][j] = d1;
      S[NM - 1][i][j] = d2;
    }
  }
  const float dltot = block_sum(dlt, red);
  if (tid == 0) sc[1] = dltot;
  __syncthreads();
  // 5. d tn_i = temp * sum_j dS_ij in_j ; d in_j = temp * sum_i dS_ij tn_i ; then through l2norm
  for (int r = w; r < NS * Bg; r += CL_NW) {
    const int s = r / Bg, a = r - s * Bg, q = s >> 1;
    const bool is_t = (s & 1) == 0;
    const float* self = nv + s * set + (int64_t)a * Dl;
    const float* other = nv + (s ^ 1) * set;
    float* out = gv + s * set + (int64_t)a * Dl;
    const float nn = nrm[s][a];
    float dotp = 0.f;
    for (int k = lane; k < Dl; k += 64) {
      float g = 0.f;
      for (int b = 0; b < Bg; ++b) g += (is_t ? S[q][a][b] : S[q][b][a]) * other[(int64_t)b * Dl + k];
      g *= temp;
      out[k] = g;
      dotp += g * self[k];
    }
    dotp = warp_sum(dotp);
    const float inv = 1.f / fmaxf(nn, 1e-12f);
    for (int k = lane; k < Dl; k += 64) {
      const float g = out[k];
      out[k] = nn > 1e-12f ? (g - self[k] * dotp) * inv : g * inv;
    }
  }
}

// Second pass of ctclip_clip_loss_ex: every output element is the weighted sum of its pairs' partials
// in ascending pair order (pair 0: w_main, the others w_multiview / (P - 1) each) -- one thread per
// element, no atomics.  Thread 0 also folds the pair losses and the log-temperature gradients.
__global__ __launch_bounds__(256) void clip_loss_ex_reduce_kernel(const float* __restrict__ ws, int64_t per_pair, int Vt,
                                                                int Vi, int64_t set, int NS, float w_main, float w_mv,
                                                                float* __restrict__ loss, float* __restrict__ pair_loss,
                                                                float* __restrict__ dt, float* __restrict__ di,
                                                                float* __restrict__ dtx, float* __restrict__ dix,
                                                                float* __restrict__ dlogtemp) {
  const int P = Vt * Vi;
  const float w_rest = P > 1 ? w_mv / (float)(P - 1) : 0.f;
  const int64_t per_set = (int64_t)(Vt + Vi) * set, total = per_set * (NS / 2);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(e / per_set);            // 0: main pair, 1: extra pair
    const int64_t f = e - x * per_set;
    const int v = (int)(f / set);                // view: text views first, then image views
    const int64_t idx = f - v * set;
    const bool is_t = v < Vt;
    const int s = 2 * x + (is_t ? 0 : 1);
    const int cnt = is_t ? Vi : Vt;
    float acc = 0.f;
    for (int c = 0; c < cnt; ++c) {
      const int p = is_t ? v * Vi + c : c * Vi + (v - Vt);
      const float g = (p == 0 ? w_main : w_rest) * ws[(int64_t)p * per_pair + NS * set + s * set + idx];
      acc = c == 0 ? g : acc + g;
    }
    float* out = x == 0 ? (is_t ? dt : di) : (is_t ? dtx : dix);
    out[(is_t ? (int64_t)v : (int64_t)(v - Vt)) * set + idx] = acc;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float* sc = ws + 2 * NS * set;
    float rest = 0.f, dl = w_main * sc[1];
    for (int p = 0; p < P; ++p) pair_loss[p] = sc[(int64_t)p * per_pair];
    for (int p = 1; p < P; ++p) {
      rest += sc[(int64_t)p * per_pair];
      dl += w_rest * sc[(int64_t)p * per_pair + 1];
    }
    loss[0] = P > 1 ? w_main * sc[0] + w_mv * (rest / (float)(P - 1)) : w_main * sc[0];
    dlogtemp[0] = dl;
  }
}

// floats of one pair's workspace slice, 0 for an unsupported shape
int64_t clip_loss_ex_per_pair(const ctclip_clip_loss_ex_args* a) {
  if (!a || a->Vt < 1 || a->Vi < 1 || (int64_t)a->Vt * a->Vi > 64 || a->Bg < 1 || a->Bg > MAXB || a->Dl < 1 ||
      a->Dl > 8192)
    return 0;
  const int64_t ns = a->t_extra ? 4 : 2;
  return 2 * ns * (int64_t)a->Bg * a->Dl + 4;
}

}  // namespace

extern "C" int ctclip_clip_loss_ex_ws_floats(const ctclip_clip_loss_ex_args* a) {
  const int64_t per_pair = clip_loss_ex_per_pair(a);
  return per_pair ? (int)(per_pair * a->Vt * a->Vi) : 0;   // < 2^31: 64 pairs x (8 x 128 x 8192 + 4)
}

extern "C" int ctclip_clip_loss_ex(const ctclip_clip_loss_ex_args* a, void* stream) {
  CT_REQUIRE(a != nullptr, CT_EINVAL);
  const int64_t per_pair = clip_loss_ex_per_pair(a);
  CT_REQUIRE(per_pair > 0, CT_ESHAPE);
  const bool extra = a->t_extra != nullptr;
  CT_REQUIRE(extra == (a->i_extra != nullptr), CT_EINVAL);
  CT_REQUIRE(a->t_raw && a->i_raw && a->log_temp && a->loss && a->pair_loss && a->dt_raw && a->di_raw && a->dlogtemp &&
                 a->ws,
             CT_EINVAL);
  CT_REQUIRE(!extra || (a->dt_extra && a->di_extra), CT_EINVAL);
  const int P = a->Vt * a->Vi;
  CT_REQUIRE(a->ws_floats >= per_pair * P, CT_EINVAL);
  const hipStream_t st = (hipStream_t)stream;
#define CT_LOSS_EX(EX, DC)                                                                                          \
  hipLaunchKernelGGL((clip_loss_ex_kernel<EX, DC>), dim3(P), dim3(CL_NT), 0, st, a->t_raw, a->i_raw, a->t_extra,    \
                     a->i_extra, a->Vi, a->Bg, a->Dl, a->log_temp, a->ws, per_pair)
  if (extra) {
    if (a->decoupled) CT_LOSS_EX(true, true); else CT_LOSS_EX(true, false);
  } else {
    if (a->decoupled) CT_LOSS_EX(false, true); else CT_LOSS_EX(false, false);
  }
#undef CT_LOSS_EX
  CT_CHECK_LAUNCH();
  const int64_t set = (int64_t)a->Bg * a->Dl, total = (int64_t)(a->Vt + a->Vi) * set * (extra ? 2 : 1);
  const int grid = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(clip_loss_ex_reduce_kernel, dim3(grid), dim3(256), 0, st, a->ws, per_pair, a->Vt, a->Vi, set,
                     extra ? 4 : 2, a->w_main, a->w_multiview, a->loss, a->pair_loss, a->dt_raw, a->di_raw, a->dt_extra,
                     a->di_extra, a->dlogtemp);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_zero_shot(const float* t_raw, const float* i_raw, int32_t P, int32_t N, int32_t Dl,
                                const float* log_temp, float* scores, float* probs, void* stream) {
  CT_REQUIRE(P >= 0 && N >= 0 && Dl > 0 && Dl <= 8192, CT_ESHAPE);
  if (P == 0 || N == 0) return 0;
  hipLaunchKernelGGL(zero_shot_kernel, dim3(N), dim3(256), (size_t)Dl * 4, (hipStream_t)stream, t_raw, i_raw, P, Dl,
                     log_temp, scores, probs);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_clip_loss(const float* t_raw, const float* i_raw, int32_t Bg, int32_t Dl, const float* log_temp,
                                float* t_norm, float* i_norm, float* loss, float* dt_raw, float* di_raw,
                                float* dlogtemp, float* sim, void* stream) {
  CT_REQUIRE(Bg > 0 && Bg <= MAXB, CT_ESHAPE);
  hipLaunchKernelGGL(clip_loss_kernel, dim3(1), dim3(CL_NT), 0, (hipStream_t)stream, t_raw, i_raw, Bg, Dl, log_temp,
                     t_norm, i_norm, loss, dt_raw, di_raw, dlogtemp, sim);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_clip_scores(const float* t_raw, const float* i_raw, int32_t B, int32_t Dl, const float* log_temp,
                                  float* out, void* stream) {
  hipLaunchKernelGGL(clip_scores_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, t_raw, i_raw, B, Dl, log_temp,
                     out);
  CT_CHECK_LAUNCH();
  return 0;
}
