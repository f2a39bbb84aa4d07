// Zero-shot attribution maps (include/ctclip_hip.h, ctclip_attr_weights / ctclip_attr_map): the exact
// split of a pathology's log-odds over the (t, h, w) token grid.  After the VQ and the mean over t
// (ct_clip/ct_clip.py:724,740) the image latent is LINEAR in the quantised tokens -- to_visual_latent
// has no bias (:767) -- so with d a direction in latent space (a normalised prompt latent, or the
// difference of a prompt pair, :771,805-807, ctclip_inference.py:305-315)
//   d . v_n = sum_{t,hw} (1/T) (W[:, hw*D:(hw+1)*D]^T d) . C[idx[n][t][hw]]
// without remainder.  Two kernels, both on the f32 matrix pipe (v_mfma_f32_16x16x4_f32: every output
// is ONE f32 fma chain in a fixed k order -- exact products of the f32 / bf16 operands, no cross-lane
// reduction, no atomics, the same bits on every run; its rate equals the packed f32 VALU's, but an
// operand costs one VGPR per lane and the sum over k needs no shuffles):
//
// attr_weights  V[R][K] = Dm[R][Dl] . Wb[Dl][K], once per prompt set: one pass over the 302 MB bf16
//   weight, HBM-bound.  A wave owns 128 columns for all Dl rows (no split of the sum, no slabs); lane
//   (c = l & 15, q = l >> 4) reads 16 bytes = columns 8c .. 8c+7 of row 16g + 4q + s (s = 0..3, g the
//   16-row group): 256 contiguous bytes per row and instruction.  MFMA j of the eight of a step takes
//   element j of every lane, i.e. columns {8c + j}: a column permutation that only decides where the
//   accumulator is stored.  The rows of Dm are the A operand (lane: row 16rg + c, 16 bytes = the four s
//   of its q), rows >= R read as zero.  Sum order of an output: g ascending, s ascending, q ascending.
//
// attr_map  out[n][r][t][hw] = s_n sum_d V[r][hw][d] C[idx[n][t*HW+hw]][d], once per batch.  A
//   workgroup owns four consecutive hw and 64 consecutive tokens m = n*T + t (wave w: 16 of them).  Per
//   hw it stages V[:, hw, :] (R x D f32, 72 KB at R = 36, D = 512; rows padded by 16 bytes) in LDS once,
//   then every wave gathers its 16 codebook rows with 16-byte loads (lane: token c, d = 32g + 8q .. +7,
//   128 contiguous bytes per row and step; the next step's loads are issued before this step's MFMAs)
//   and multiplies them with the R directions (B operand from LDS, ds_read_b128; direction rows >= R
//   re-read row R-1 and are never stored).  The four hw results of a (token, r) pair stay in the lane's
//   accumulators and leave as ONE 16-byte store (HW % 4 == 0; scalar stores otherwise): every output
//   element is written exactly once.  s_n = exp(*log_temp) / (T max(||i_raw[n]||, 1e-12)) is computed
//   by the workgroup for the volumes its tokens belong to (a fixed-order wave sum); raw mode skips it.
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int ATTR_MAX_ROWS = CTCLIP_ATTR_MAX_ROWS;   // 48 = three 16-row MFMA groups
constexpr int MAP_TOK = 64;                            // tokens per workgroup (16 per wave)
constexpr int MAP_HWB = 4;                             // hw per workgroup (one 16-byte store)
constexpr int MAP_PAD = 4;                             // floats of padding per staged V row

// ------------------------------------------------------------------------------------ attr_weights
template <int RG>
struct WStep {
  u32x4 w[4];
  f32x4 a[RG];
};

template <int RG>
__device__ __forceinline__ void w_load(WStep<RG>& s, const u16* __restrict__ wp, int64_t K, bool colok,
                                       const float* const (&ap)[RG], const bool (&rowok)[RG], int lb) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    s.w[i] = colok ? *(const u32x4*)(wp + (int64_t)(lb + i) * K) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int g = 0; g < RG; ++g) s.a[g] = rowok[g] ? *(const f32x4*)(ap[g] + lb) : f32x4{0.f, 0.f, 0.f, 0.f};
}

template <int RG>
__device__ __forceinline__ void w_mma(f32x4 (&acc)[RG][8], const WStep<RG>& s) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float f[8];
    unpack8(s.w[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int g = 0; g < RG; ++g)
        acc[g][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(s.a[g][i], f[j], acc[g][j], 0, 0, 0);
  }
}

template <int RG>
__global__ __launch_bounds__(256) void attr_weights_kernel(const float* __restrict__ Dm, const u16* __restrict__ Wb,
                                                           int R, int Dl, int64_t K, float* __restrict__ V) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int64_t col0 = ((int64_t)blockIdx.x * 4 + w) * 128;   // this wave's 128 columns
  if (col0 >= K) return;                                      // wave-uniform
  const int64_t col = col0 + 8 * c;
  const bool colok = col < K;                                 // K % 8 == 0: a lane's 8 columns are in or out
  const u16* wp = Wb + (int64_t)(4 * q) * K + (colok ? col : 0);
  const float* ap[RG];
  bool rowok[RG];
#pragma unroll
  for (int g = 0; g < RG; ++g) {
    rowok[g] = 16 * g + c < R;
    ap[g] = Dm + (int64_t)(rowok[g] ? 16 * g + c : 0) * Dl + 4 * q;
  }
  f32x4 acc[RG][8];
#pragma unroll
  for (int g = 0; g < RG; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[g][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nsteps = Dl / 16;
  WStep<RG> s0, s1;
  w_load<RG>(s0, wp, K, colok, ap, rowok, 0);
  int t = 0;
  for (; t + 2 <= nsteps; t += 2) {
    w_load<RG>(s1, wp, K, colok, ap, rowok, (t + 1) * 16);
    w_mma<RG>(acc, s0);
    // the step after next, clamped to the last one (re-read, unused) so no branch merges s0
    w_load<RG>(s0, wp, K, colok, ap, rowok, min(t + 2, nsteps - 1) * 16);
    w_mma<RG>(acc, s1);
  }
  if (t < nsteps) w_mma<RG>(acc, s0);
  // acc[g][j][v] = V[r = 16g + 4q + v][col + j]
  if (!colok) return;
#pragma unroll
  for (int g = 0; g < RG; ++g)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = 16 * g + 4 * q + v;
      if (r < R) {
        float* o = V + (int64_t)r * K + col;
        *(f32x4*)o = f32x4{acc[g][0][v], acc[g][1][v], acc[g][2][v], acc[g][3][v]};
        *(f32x4*)(o + 4) = f32x4{acc[g][4][v], acc[g][5][v], acc[g][6][v], acc[g][7][v]};
      }
    }
}

template <int RG>
void weights_launch(const float* Dm, const u16* Wb, int R, int Dl, int64_t K, float* V, hipStream_t st) {
  const int64_t waves = (K + 127) / 128;
  hipLaunchKernelGGL(attr_weights_kernel<RG>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, Dm, Wb, R, Dl, K, V);
}

// ---------------------------------------------------------------------------------------- attr_map
template <int RG>
__global__ __launch_bounds__(256) void attr_map_kernel(const float* __restrict__ V, const int32_t* __restrict__ idx,
                                                       const float* __restrict__ cb, int codes, int N, int R, int T,
                                                       int HW, int D, const float* __restrict__ i_raw, int Dl,
                                                       const float* __restrict__ log_temp, float* __restrict__ out,
                                                       int nchunks) {
  extern __shared__ __attribute__((aligned(16))) float vs[];   // [R][D + MAP_PAD]
  __shared__ float sn[MAP_TOK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int hwg = blockIdx.x / nchunks, chunk = blockIdx.x - hwg * nchunks;
  const int hw0 = hwg * MAP_HWB;
  const int64_t M = (int64_t)N * T;
  const int64_t m0 = (int64_t)chunk * MAP_TOK;
  const int ldv = D + MAP_PAD;
  // s_n of the volumes this chunk's tokens belong to (at most MAP_TOK of them)
  const int nlo = (int)(m0 / T);
  if (i_raw != nullptr) {
    const int nhi = (int)(((m0 + MAP_TOK < M ? m0 + MAP_TOK : M) - 1) / T);
    const float temp = expf(log_temp[0]);
    for (int n = nlo + w; n <= nhi; n += 4) {
      float ii = 0.f;
      for (int k = lane; k < Dl; k += 64) {
        const float y = i_raw[(int64_t)n * Dl + k];
        ii += y * y;
      }
      ii = warp_sum(ii);
      if (lane == 0) sn[n - nlo] = temp / ((float)T * fmaxf(sqrtf(ii), 1e-12f));
    }
  }
  // the A operand's token: row c of this wave's 16; tokens past the end read token 0, stored nowhere
  const int64_t ma = m0 + 16 * w + c;
  const int64_t ma_rd = ma < M ? ma : 0;
  int brow[RG];
#pragma unroll
  for (int g = 0; g < RG; ++g) brow[g] = min(16 * g + c, R - 1) * ldv + 8 * q;
  f32x4 acc[MAP_HWB][RG];
#pragma unroll
  for (int h = 0; h < MAP_HWB; ++h)
#pragma unroll
    for (int g = 0; g < RG; ++g) acc[h][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nch = D / 4, nsteps = D / 32;
#pragma unroll
  for (int h = 0; h < MAP_HWB; ++h) {
    const int hw = hw0 + h;
    if (hw >= HW) break;                      // workgroup-uniform
    __syncthreads();                          // the previous hw's reads of vs are done
    for (int i = threadIdx.x; i < R * nch; i += 256) {
      const int r = i / nch, k = i - r * nch;
      *(f32x4*)(vs + r * ldv + 4 * k) = *(const f32x4*)(V + ((int64_t)r * HW + hw) * D + 4 * k);
    }
    int code = idx[ma_rd * HW + hw];
    code = (unsigned)code < (unsigned)codes ? code : 0;
    const float* ap = cb + (int64_t)code * D + 8 * q;
    __syncthreads();
    f32x4 a0 = *(const f32x4*)ap, a1 = *(const f32x4*)(ap + 4);
    for (int s = 0; s < nsteps; ++s) {
      const int sn_ = min(s + 1, nsteps - 1) * 32;      // the next step's rows (the last one re-read, unused)
      const f32x4 n0 = *(const f32x4*)(ap + sn_), n1 = *(const f32x4*)(ap + sn_ + 4);
      f32x4 b0[RG], b1[RG];
#pragma unroll
      for (int g = 0; g < RG; ++g) {
        b0[g] = *(const f32x4*)(vs + brow[g] + 32 * s);
        b1[g] = *(const f32x4*)(vs + brow[g] + 32 * s + 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < RG; ++g)
          acc[h][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], b0[g][j], acc[h][g], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < RG; ++g)
          acc[h][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], b1[g][j], acc[h][g], 0, 0, 0);
      a0 = n0;
      a1 = n1;
    }
  }
  // acc[h][g][v] = token m0 + 16w + 4q + v, direction 16g + c, hw0 + h
  const bool vec = (HW % MAP_HWB) == 0;       // then hw0 + 3 < HW and the four floats are 16-byte aligned
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int64_t m = m0 + 16 * w + 4 * q + v;
    if (m >= M) continue;
    const int n = (int)(m / T), t = (int)(m - (int64_t)n * T);
    const float sc = i_raw != nullptr ? sn[n - nlo] : 1.f;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
      const int r = 16 * g + c;
      if (r >= R) continue;
      float* o = out + (((int64_t)n * R + r) * T + t) * HW + hw0;
      // (copied out of the accumulators, which stay as the MFMAs left them)
      float x[MAP_HWB];
#pragma unroll
      for (int h = 0; h < MAP_HWB; ++h) x[h] = i_raw != nullptr ? acc[h][g][v] * sc : acc[h][g][v];
      if (vec) {
        *(f32x4*)o = f32x4{x[0], x[1], x[2], x[3]};
      } else {
#pragma unroll
        for (int h = 0; h < MAP_HWB; ++h)
          if (hw0 + h < HW) o[h] = x[h];
      }
    }
  }
}

template <int RG>
int map_launch(const float* V, const int32_t* idx, const float* cb, int codes, int N, int R, int T, int HW, int D,
               const float* i_raw, int Dl, const float* log_temp, float* out, hipStream_t st) {
  const size_t smem = (size_t)R * (D + MAP_PAD) * sizeof(float);
  hipError_t e = hipFuncSetAttribute((const void*)attr_map_kernel<RG>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)smem);
  if (e != hipSuccess) return (int)e;
  const int nchunks = (int)(((int64_t)N * T + MAP_TOK - 1) / MAP_TOK);
  const int hwgs = (HW + MAP_HWB - 1) / MAP_HWB;
  hipLaunchKernelGGL(attr_map_kernel<RG>, dim3((unsigned)(hwgs * nchunks)), dim3(256), smem, st, V, idx, cb, codes, N,
                     R, T, HW, D, i_raw, Dl, log_temp, out, nchunks);
  return 0;
}

}  // namespace

extern "C" int ctclip_attr_weights(const float* dirs, const void* w_bf16, int32_t R, int32_t Dl, int64_t K, float* V,
                                   void* stream) {
  CT_REQUIRE(R >= 1 && R <= ATTR_MAX_ROWS && Dl >= 16 && Dl % 16 == 0 && K >= 8 && K % 8 == 0, CT_ESHAPE);
  CT_REQUIRE(dirs && w_bf16 && V, CT_EINVAL);
  CT_REQUIRE(aligned16(dirs) && aligned16(w_bf16) && aligned16(V), CT_EALIGN);
  const hipStream_t st = (hipStream_t)stream;
  const u16* Wb = (const u16*)w_bf16;
  if (R <= 16) weights_launch<1>(dirs, Wb, R, Dl, K, V, st);
  else if (R <= 32) weights_launch<2>(dirs, Wb, R, Dl, K, V, st);
  else weights_launch<3>(dirs, Wb, R, Dl, K, V, st);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_attr_map(const float* V, const int32_t* idx, const float* codebook, int32_t codes, int32_t N,
                               int32_t R, int32_t T, int32_t HW, int32_t D, const float* i_raw, int32_t Dl,
                               const float* log_temp, float* out, void* stream) {
  CT_REQUIRE(N >= 1 && R >= 1 && R <= ATTR_MAX_ROWS && T >= 1 && HW >= 1 && codes >= 1, CT_ESHAPE);
  CT_REQUIRE(D >= 32 && D <= 512 && D % 32 == 0, CT_ESHAPE);
  // 32-bit block index and LDS offsets; the token count N * T * HW stays below 2^31 as in ctclip_vq_pool
  CT_REQUIRE((int64_t)N * T * HW < (1ll << 31) &&
                 (int64_t)((HW + MAP_HWB - 1) / MAP_HWB) * (((int64_t)N * T + MAP_TOK - 1) / MAP_TOK) < (1ll << 31),
             CT_ESHAPE);
  CT_REQUIRE(V && idx && codebook && out, CT_EINVAL);
  CT_REQUIRE(i_raw == nullptr || (log_temp != nullptr && Dl >= 1), CT_EINVAL);
  CT_REQUIRE(aligned16(V) && aligned16(codebook) && aligned16(out), CT_EALIGN);
  const hipStream_t st = (hipStream_t)stream;
  int rc;
  if (R <= 16) rc = map_launch<1>(V, idx, codebook, codes, N, R, T, HW, D, i_raw, Dl, log_temp, out, st);
  else if (R <= 32) rc = map_launch<2>(V, idx, codebook, codes, N, R, T, HW, D, i_raw, Dl, log_temp, out, st);
  else rc = map_launch<3>(V, idx, codebook, codes, N, R, T, HW, D, i_raw, Dl, log_temp, out, st);
  if (rc != 0) return rc;
  CT_CHECK_LAUNCH();
  return 0;
}
