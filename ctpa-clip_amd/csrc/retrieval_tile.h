// The normalise step and the 64 x 64 score tile that retrieval.hip and case_retrieval.hip share: both
// files must give one S_ij the same bits (case_retrieval's lists equal retrieval_topk's), so the code
// that makes them exists once.
//
// P is the file's parameter struct; used here: q, g (raw latents), N, M, Dl, ldD (Dl rounded up to 4),
// qn [N][ldD], gn [M][ldD] (the normalised rows, pad columns zero).
#pragma once
#include "common.h"

namespace rtile {

constexpr int TB = 64;            // rows / columns of a score tile
constexpr int KT = 16;            // K step
constexpr int LDR = 20;           // K-contiguous LDS image [row][16 k]: 16-B aligned rows, 64 lanes on 64 banks
constexpr int NTH = 256;
constexpr int TILE_SMEM = 4 * TB * LDR;   // floats: [buf][A | B]

__host__ __device__ inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }

// column chunks: enough workgroups to fill the device when the row tiles alone do not
inline void chunks(int N, int M, int target, int cap, int* C, int* span) {
  const int nTr = (N + TB - 1) / TB, nTc = (M + TB - 1) / TB;
  int c = std::min(std::min((target + nTr - 1) / nTr, nTc), cap);
  *span = (nTc + c - 1) / c;
  *C = (nTc + *span - 1) / *span;
}

// one row: x / max(|x|, 1e-12) (sqrtf, a true division; a zero row stays zero), pad columns zeroed.
// Called by a whole wave.
__device__ __forceinline__ void norm_row(const float* __restrict__ src, float* __restrict__ dst, int Dl, int ldD) {
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  for (int k = lane; k < Dl; k += 64) s += src[k] * src[k];
  s = warp_sum(s);
  const float inv = 1.f / fmaxf(sqrtf(s), 1e-12f);
  for (int k = lane; k < ldD; k += 64) dst[k] = k < Dl ? src[k] * inv : 0.f;
}

// ------------------------------------------------------------------ score tile (loss_tiled.hip pass b)
// one 16-B chunk of a 64-row x 16-k K-contiguous tile: row t / 4, k quad t % 4 (rows of ldD floats, pad
// columns zero, so only the row and the padded width bound the load)
__device__ __forceinline__ f32x4 kload(const float* __restrict__ base, int64_t ld, int rows, int row0, int k0) {
  const int t = threadIdx.x, gr = row0 + (t >> 2), gk = k0 + (t & 3) * 4;
  return (gr < rows && gk < ld) ? *(const f32x4*)(base + (int64_t)gr * ld + gk) : f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void kwrite(float* img, const f32x4& r) {
  const int t = threadIdx.x;
  *(f32x4*)(img + (t >> 2) * LDR + (t & 3) * 4) = r;
}

// acc[i][j][r] = S of query i0 + wm*32 + 16 i + (lane & 15), gallery row j0 + wn*32 + 16 j + 4 (lane >> 4) + r.
// smem: TILE_SMEM floats.  Ends with a barrier: smem may be staged again at once.
template <class P>
__device__ __forceinline__ void score_tile(const P& p, int i0, int j0, float* smem, f32x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  const int64_t ldD = p.ldD;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (int)((ldD + KT - 1) / KT);
  f32x4 ra = kload(p.qn, ldD, p.N, i0, 0), rb = kload(p.gn, ldD, p.M, j0, 0);
  kwrite(smem, ra);
  kwrite(smem + TB * LDR, rb);
  __syncthreads();
  const int r16 = lane & 15, g = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const float* As = smem + (kt & 1) * 2 * TB * LDR;
    const float* Bs = As + TB * LDR;
    if (kt + 1 < nk) {
      ra = kload(p.qn, ldD, p.N, i0, (kt + 1) * KT);
      rb = kload(p.gn, ldD, p.M, j0, (kt + 1) * KT);
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
}

}  // namespace rtile
