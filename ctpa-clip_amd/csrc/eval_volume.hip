// The evaluation / inference loader arithmetic on the GPU: ct_clip/data_inference.py:78-122
// (CTReportDatasetinfer.nii_img_to_tensor), one launch per volume.
//
//   v = x * 1000 -> clip(-1000, 200) -> (v + 400) / 600 -> centre crop / pad (value -1) to
//   480 x 480 x 240 -> (1, D, H, W) f32.
//
// The arithmetic type is numpy's: an f32 scan computes in f32, an f64 scan in f64 with the result
// rounded to f32 once; every operation is rounded on its own (no FMA contraction), so the output
// is the reference's bit for bit.  There is no resampling: an output voxel is either one source
// voxel or the pad value, so the kernel is a pure stream (up to 221 MB read + 221 MB written).
//
// Layout: the stored (a0, a1, a2) scan is read through strides as (h, w, d) = (a1, a2, a0), so both
// the source and the (D, H, W) output are contiguous along w.  A thread owns four consecutive w of
// one output row: one 16-byte store when the row base allows it, and one 16-byte load (two for
// f64) when its four voxels lie inside the scan, the scan is w-contiguous and that address happens
// to be 16-byte aligned (the crop / pad offset decides); scalar accesses otherwise.
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

struct EP {
  const void* src;
  int64_t D, H, W;              // source extents, (d, h, w) view
  int64_t sd, sh, sw;           // source strides (elements)
  int64_t Do, Ho, Wo;           // output extents
  int64_t od, oh, ow;           // output index - source index
  int64_t Wq;                   // quads per output row, ceil(Wo / 4)
  float fill;
};

template <typename T>
__device__ __forceinline__ float norm1(T x) {
#pragma clang fp contract(off)
  T v = x * (T)1000;
  v = v < (T)-1000 ? (T)-1000 : (v > (T)200 ? (T)200 : v);     // np.clip: a NaN stays a NaN
  v = v + (T)400;
  return (float)(v / (T)600);
}

// VEC: Wo % 4 == 0 and a 16-byte aligned output, so every quad is one aligned 16-byte store.
// grid (ceil(Ho * Wq / 256), Do), 256 threads.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void eval_volume_kernel(EP p, float* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= p.Ho * p.Wq) return;
  const int64_t d = blockIdx.y, h = q / p.Wq, w0 = (q - h * p.Wq) * 4;
  const int64_t ds = d - p.od, hs = h - p.oh, ws0 = w0 - p.ow;
  const bool row_in = ds >= 0 && ds < p.D && hs >= 0 && hs < p.H;
  float r[4] = {p.fill, p.fill, p.fill, p.fill};
  if (row_in && ws0 + 3 >= 0 && ws0 < p.W) {
    const T* s = (const T*)p.src + ds * p.sd + hs * p.sh;
    if (p.sw == 1 && ws0 >= 0 && ws0 + 3 < p.W && ((uintptr_t)(s + ws0) & 15) == 0) {
      if constexpr (sizeof(T) == 4) {
        const f32x4 x = *(const f32x4*)(s + ws0);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = norm1<float>(x[k]);
      } else {
        const double2 x0 = *(const double2*)(s + ws0), x1 = *(const double2*)(s + ws0 + 2);
        r[0] = norm1<double>(x0.x);
        r[1] = norm1<double>(x0.y);
        r[2] = norm1<double>(x1.x);
        r[3] = norm1<double>(x1.y);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t ws = ws0 + k;
        if (ws >= 0 && ws < p.W) r[k] = norm1<T>(s[ws * p.sw]);
      }
    }
  }
  float* o = out + (d * p.Ho + h) * p.Wo + w0;
  if constexpr (VEC) {
    f32x4 v = {r[0], r[1], r[2], r[3]};
    *(f32x4*)o = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (w0 + k < p.Wo) o[k] = r[k];
  }
}

template <typename T>
void launch(const EP& p, float* out, hipStream_t st) {
  dim3 grid((unsigned)((p.Ho * p.Wq + 255) / 256), (unsigned)p.Do);
  if (p.Wo % 4 == 0 && aligned16(out)) hipLaunchKernelGGL((eval_volume_kernel<T, true>), grid, dim3(256), 0, st, p, out);
  else hipLaunchKernelGGL((eval_volume_kernel<T, false>), grid, dim3(256), 0, st, p, out);
}

}  // namespace

extern "C" int ctclip_eval_volume(const ctclip_eval_volume_args* a, float* out, void* stream) {
  CT_REQUIRE(a && a->src && out, CT_EINVAL);
  CT_REQUIRE(a->src_dtype == CTCLIP_F32 || a->src_dtype == CTCLIP_F64, CT_EINVAL);
  CT_REQUIRE(a->D > 0 && a->H > 0 && a->W > 0 && a->sd >= 0 && a->sh >= 0 && a->sw >= 0, CT_ESHAPE);
  CT_REQUIRE(a->Do > 0 && a->Ho > 0 && a->Wo > 0 && a->Do < 65536, CT_ESHAPE);
  CT_REQUIRE((uintptr_t)a->src % (a->src_dtype == CTCLIP_F64 ? 8 : 4) == 0 && (uintptr_t)out % 4 == 0, CT_EALIGN);
  EP p;
  p.src = a->src;
  p.D = a->D; p.H = a->H; p.W = a->W;
  p.sd = a->sd; p.sh = a->sh; p.sw = a->sw;
  p.Do = a->Do; p.Ho = a->Ho; p.Wo = a->Wo;
  p.od = a->od; p.oh = a->oh; p.ow = a->ow;
  p.Wq = (a->Wo + 3) / 4;
  p.fill = a->fill;
  CT_REQUIRE((p.Ho * p.Wq + 255) / 256 < 2147483647LL, CT_ESHAPE);
  hipStream_t st = (hipStream_t)stream;
  if (a->src_dtype == CTCLIP_F64) launch<double>(p, out, st);
  else launch<float>(p, out, st);
  CT_CHECK_LAUNCH();
  return 0;
}
