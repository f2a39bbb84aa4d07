// CT volume augmentation on the GPU: the views CTCLIP.forward(aug_image=...) takes, every view of
// every sample in one launch.
//
//   video (B, 1, D, H, W), int16 HU or f32 in [-1, 1]  ->  out [V, B, 1, D, H, W], same dtype.
//
// Per (view v, sample b) one 128-byte record (ctclip_augment_rec): a 3 x 4 matrix [M | t], gain,
// shift, sigma (float64) and a 64-bit noise seed.  For the output voxel o = (d, h, w), with
// c = ((D-1)/2, (H-1)/2, (W-1)/2):
//
//   s      = M (o - c) + (c + t)               inverse map, each row summed left to right
//   i0     = floor(s), i1 = i0 + 1, l1 = s - i0, l0 = 1 - l1        per axis
//   x(i)   = clip(HU, -1000, 1000) / 1000 (int16) or the voxel (f32); -1 where a tap's index lies
//            outside [0, n - 1] (the loader's pad value)
//   xi     = trilinear: w, then h, then d, (a * l0) + (b * l1) each (resample.hip's order)
//   n      = (u0 + u1 + u2 + u3 - 2 * 65535) / sqrt(4 (65536^2 - 1) / 12), u_k the four 16-bit
//            fields of the splitmix64 finaliser of seed ^ flat * phi (common.h hid_keep's hash),
//            flat = (d H + h) W + w: a zero-mean unit-variance Irwin-Hall(4) variate
//   y      = clip((gain * xi + shift) + sigma * n, -1, 1)           (the noise term only if sigma != 0)
//   out    = (float)y, or (int16)rint(1000 y) (half to even)
//
// All of it in float64, every operation rounded on its own (no FMA contraction), the result rounded
// once: a numpy float64 restatement reproduces the bits (tests/augment_common.py).  Identity
// parameters therefore return the input, diag(1, 1, -1) is a flip along w, an integer t an exact
// shift with fill, and a quarter-turn matrix torch.rot90.
//
// Schedule: lanes along w, the contiguous axis of source and output.  A thread owns NV consecutive
// voxels of one output row (8 int16 / 4 f32 = 16 bytes), stored as one vector when the row has room
// and the address is 16-byte aligned, voxel by voxel otherwise (W not a multiple of NV, unaligned
// bases).  A workgroup owns 256 such groups of one output plane; grid (groups / 256, D, V * B).  The
// row part of s (M[.][0] (d - cd) + M[.][1] (h - ch)) is computed once per thread -- the same
// left-to-right sum.  The eight taps are read from clamped addresses and replaced by the fill value
// afterwards, so there is no divergent branch; they are served by L2 (a wave's footprint under an
// in-plane rotation of a few degrees is a slightly slanted row).  No LDS.
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

struct AP {
  const void* src;
  void* out;
  const ctclip_augment_rec* recs;   // [V * B]
  int64_t B, D, H, W;
  int64_t Wg;                       // groups per output row, ceil(W / NV)
};

constexpr double NOISE_DIV = 37837.22723720648;   // sqrt(4 * (65536^2 - 1) / 12)
constexpr double FILL = -1.0;

__device__ __forceinline__ double noise(uint64_t seed, int64_t flat) {
#pragma clang fp contract(off)
  uint64_t x = seed ^ ((uint64_t)flat * 0x9E3779B97F4A7C15ull);
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  const int sum = (int)(x & 0xffff) + (int)((x >> 16) & 0xffff) + (int)((x >> 32) & 0xffff) + (int)(x >> 48);
  return (double)(sum - 2 * 65535) / NOISE_DIV;
}

template <typename T>
__device__ __forceinline__ double load1(const T* s, int64_t i) {
#pragma clang fp contract(off)
  if constexpr (sizeof(T) == 2) {
    double v = (double)s[i];
    v = v < -1000.0 ? -1000.0 : (v > 1000.0 ? 1000.0 : v);
    return v / 1000.0;
  } else {
    return (double)s[i];
  }
}

// one axis of the inverse map: the two tap indices clamped into [0, n-1] (a safe address), whether
// each lies inside, and the weights.  floor(s) is clamped as a double before the conversion, so a
// far-away (finite) s never reaches an out-of-range double -> int conversion; l1 is s - floor(s)
// whatever the clamp does.
struct Axis {
  int64_t a0, a1;
  bool in0, in1;
  double l0, l1;
};
__device__ __forceinline__ Axis axis(double s, int64_t n) {
#pragma clang fp contract(off)
  Axis t;
  const double fl = floor(s);
  t.l1 = s - fl;
  t.l0 = 1.0 - t.l1;
  const double nd = (double)(int)n;                                  // n < 2^31 (entry point)
  const double flc = fl < -2.0 ? -2.0 : (fl > nd ? nd : fl);         // NaN never arrives (host check)
  const int64_t i0 = (int)flc, i1 = i0 + 1;
  t.in0 = i0 >= 0 && i0 < n;
  t.in1 = i1 >= 0 && i1 < n;
  t.a0 = i0 < 0 ? 0 : (i0 > n - 1 ? n - 1 : i0);
  t.a1 = i1 < 0 ? 0 : (i1 > n - 1 ? n - 1 : i1);
  return t;
}

template <typename T>
__device__ __forceinline__ T voxel(const AP& p, const ctclip_augment_rec& r, const T* __restrict__ src,
                                   const double* row, double cw, int64_t flat, int64_t w) {
#pragma clang fp contract(off)
  const double ow = (double)(int)w - cw;
  const Axis td = axis((row[0] + r.m[2] * ow) + row[3], p.D);
  const Axis th = axis((row[1] + r.m[6] * ow) + row[4], p.H);
  const Axis tw = axis((row[2] + r.m[10] * ow) + row[5], p.W);
  double fd[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int64_t di = a ? td.a1 : td.a0;
    const bool din = a ? td.in1 : td.in0;
    double fh[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int64_t base = (di * p.H + (b ? th.a1 : th.a0)) * p.W;
      const bool rin = din && (b ? th.in1 : th.in0);
      const double x0 = load1<T>(src, base + tw.a0), x1 = load1<T>(src, base + tw.a1);
      double o = (rin && tw.in0 ? x0 : FILL) * tw.l0;
      o += (rin && tw.in1 ? x1 : FILL) * tw.l1;
      fh[b] = o;
    }
    double o = fh[0] * th.l0;
    o += fh[1] * th.l1;
    fd[a] = o;
  }
  double xi = fd[0] * td.l0;
  xi += fd[1] * td.l1;
  double y = r.gain * xi + r.shift;
  if (r.sigma != 0.0) y = y + r.sigma * noise(r.seed, flat);
  y = y < -1.0 ? -1.0 : (y > 1.0 ? 1.0 : y);
  if constexpr (sizeof(T) == 2) return (T)(int)rint(1000.0 * y);
  else return (float)y;
}

// grid (ceil(H * Wg / 256), D, V * B), 256 threads; NV = 16 / sizeof(T) voxels per thread
template <typename T>
__global__ __launch_bounds__(256) void augment_kernel(AP p) {
#pragma clang fp contract(off)
  constexpr int NV = 16 / sizeof(T);
  typedef T VT __attribute__((ext_vector_type(NV)));
  const unsigned q = blockIdx.x * 256u + threadIdx.x, Wg = (unsigned)p.Wg;   // H * W < 2^31 (entry point)
  if (q >= (unsigned)p.H * Wg) return;
  const int64_t d = blockIdx.y, vb = blockIdx.z, b = (unsigned)vb % (unsigned)p.B;
  const int64_t h = q / Wg, w0 = (int64_t)(q - (unsigned)h * Wg) * NV;
  const ctclip_augment_rec& r = p.recs[vb];
  const double cd = (double)(int)(p.D - 1) / 2.0, ch = (double)(int)(p.H - 1) / 2.0, cw = (double)(int)(p.W - 1) / 2.0;
  const double od = (double)(int)d - cd, oh = (double)(int)h - ch;
  // per axis: M[a][0] od + M[a][1] oh, and c + t
  const double row[6] = {r.m[0] * od + r.m[1] * oh, r.m[4] * od + r.m[5] * oh, r.m[8] * od + r.m[9] * oh,
                         cd + r.m[3],               ch + r.m[7],               cw + r.m[11]};
  const int64_t vol = p.D * p.H * p.W;
  const T* src = (const T*)p.src + b * vol;
  const int64_t flat0 = (d * p.H + h) * p.W + w0;
  T* o = (T*)p.out + vb * vol + flat0;
  if (w0 + NV <= p.W && ((uintptr_t)o & 15) == 0) {
    VT v;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = voxel<T>(p, r, src, row, cw, flat0 + k, w0 + k);
    *(VT*)o = v;
  } else {
    for (int k = 0; k < NV && w0 + k < p.W; ++k) o[k] = voxel<T>(p, r, src, row, cw, flat0 + k, w0 + k);
  }
}

template <typename T>
void launch(const AP& p0, int64_t VB, hipStream_t st) {
  AP p = p0;
  constexpr int NV = 16 / sizeof(T);
  p.Wg = (p.W + NV - 1) / NV;
  dim3 grid((unsigned)((p.H * p.Wg + 255) / 256), (unsigned)p.D, (unsigned)VB);
  hipLaunchKernelGGL((augment_kernel<T>), grid, dim3(256), 0, st, p);
}

}  // namespace

extern "C" int ctclip_augment_volume(const ctclip_augment_args* a, void* out, void* stream) {
  CT_REQUIRE(a && a->src && a->recs && out, CT_EINVAL);
  CT_REQUIRE(a->dtype == CTCLIP_F32 || a->dtype == CTCLIP_I16, CT_EINVAL);
  CT_REQUIRE(a->B > 0 && a->D > 0 && a->H > 0 && a->W > 0 && a->V >= 1, CT_ESHAPE);
  CT_REQUIRE(a->V * a->B <= 65535 && a->D <= 65535, CT_ESHAPE);
  CT_REQUIRE(a->H < (1LL << 31) && a->W < (1LL << 31) && a->H * a->W < (1LL << 31), CT_ESHAPE);
  const int esz = a->dtype == CTCLIP_I16 ? 2 : 4;
  CT_REQUIRE((uintptr_t)a->src % esz == 0 && (uintptr_t)out % esz == 0 && (uintptr_t)a->recs % 8 == 0, CT_EALIGN);
  AP p;
  p.src = a->src; p.out = out; p.recs = a->recs;
  p.B = a->B; p.D = a->D; p.H = a->H; p.W = a->W; p.Wg = 0;
  hipStream_t st = (hipStream_t)stream;
  if (a->dtype == CTCLIP_I16) launch<int16_t>(p, a->V * a->B, st);
  else launch<float>(p, a->V * a->B, st);
  CT_CHECK_LAUNCH();
  return 0;
}
