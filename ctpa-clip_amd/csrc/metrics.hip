// Bootstrap AUROC on the GPU: ct_clip/evaluate.py:160-207 (roc_curve + auc per label) inside the
// resampling loop of evaluate.py:305-337, 1,000 resamples x 18 labels on the host in the reference.
//
// The area under the ROC curve of a sample with ties is the Mann-Whitney statistic with ties
// counted half:  AUROC = sum_g pos_g (2 neg_below_g + neg_g) / (2 Pos Neg), g running over the
// groups of equal scores.  A bootstrap resample only changes how often each row counts (its
// multiplicity), not the order of the scores, so each label is sorted ONCE (by the caller) and a
// resample is a walk along that order with multiplicities as weights:
//
//   * one workgroup per resample builds mult[N] from the resample's N indices with integer LDS
//     atomics, once for all P labels;
//   * per label, thread t owns positions [t L, (t + 1) L) of the sorted order: a local running sum
//     of (pos, neg) weights, packed (pos << 16 | neg, both <= N <= 8192), then one block scan,
//     leaves the exclusive prefix pre[i] in LDS; bit 31 of pre[i] marks a position whose score
//     differs in bits from its predecessor's (a group start);
//   * a second walk over pre[] adds, at every group end e with start s, the integer
//     (Cpos[e] - Cpos[s]) (Cneg[s] + Cneg[e]) to a 64-bit accumulator; the start of a group that
//     began in an earlier thread's range is the last start recorded by the threads before;
//   * the 64-bit partial sums are added across the block and divided once, in f64, by 2 Pos Neg
//     (NaN when the resample holds one class only).
//
// Everything before the one division is an exact integer, so the result does not depend on the
// launch geometry or on the order of the atomics.  LDS: 4 N (mult) + 4 (N + 1) (pre) bytes + 3 KB
// of scratch: 67 KB at the N = 8192 cap, two workgroups per CU of the 160 KiB; up to N = 2048 the
// small instantiation takes 19 KB.
#include "common.h"
#include "../../include/ctclip_hip.h"

namespace {

constexpr int NT = 256;

template <int CAP>
__global__ __launch_bounds__(NT) void auroc_boot_kernel(const float* __restrict__ scores,
                                                        const uint8_t* __restrict__ labels,
                                                        const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ resample, int N, int P,
                                                        double* __restrict__ out) {
  __shared__ int mult[CAP];
  __shared__ unsigned pre[CAP + 1];
  __shared__ unsigned wave_tot[NT / 64];
  __shared__ int last_start[NT];
  __shared__ long long red[NT];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t s = blockIdx.x;

  for (int i = t; i < N; i += NT) mult[i] = 0;
  __syncthreads();
  for (int i = t; i < N; i += NT) {
    const int r = resample[s * N + i];
    if ((unsigned)r < (unsigned)N) atomicAdd(&mult[r], 1);
  }
  __syncthreads();

  // (an order entry outside [0, N) is the caller's error: it is read as row 0, never out of bounds)
  auto row = [N](int r) { return (unsigned)r < (unsigned)N ? r : 0; };
  const int L = (N + NT - 1) / NT;
  const int a = min(t * L, N), b = min(a + L, N);
  for (int p = 0; p < P; ++p) {
    const int32_t* ord = order + (int64_t)p * N;
    // walk 1: local exclusive prefix of the packed (pos, neg) weights, group starts, last start
    unsigned run = 0, prev_key = 0;
    int last = -1;
    if (a < b && a > 0) prev_key = __float_as_uint(scores[(int64_t)row(ord[a - 1]) * P + p]);
    for (int i = a; i < b; ++i) {
      const int r = row(ord[i]);
      const unsigned key = __float_as_uint(scores[(int64_t)r * P + p]);
      const unsigned m = (unsigned)mult[r];
      const bool start = i == 0 || key != prev_key;
      prev_key = key;
      if (start) last = i;
      pre[i] = run | (start ? 0x80000000u : 0u);
      run += labels[(int64_t)r * P + p] ? (m << 16) : m;
    }
    last_start[t] = last;
    // exclusive block scan of the per-thread totals
    unsigned inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    unsigned base = inc - run, total = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
      if (k < wv) base += wave_tot[k];
      total += wave_tot[k];
    }
    for (int i = a; i < b; ++i) pre[i] += base;      // base < 2^30: bit 31 is kept
    if (t == 0) pre[N] = total;
    // the start of the group that is open where this thread's range begins
    int open = -1;
    for (int k = t - 1; k >= 0 && open < 0; --k) open = last_start[k];
    __syncthreads();
    // walk 2: every group end adds (Cpos[e] - Cpos[s]) (Cneg[s] + Cneg[e])
    long long acc = 0;
    auto close = [&](int gs, int ge) {
      const unsigned ws = pre[gs] & 0x7fffffffu, we = pre[ge] & 0x7fffffffu;
      acc += (long long)((we >> 16) - (ws >> 16)) * (long long)((ws & 0xffffu) + (we & 0xffffu));
    };
    for (int i = a; i < b; ++i) {
      if (pre[i] >> 31) {
        if (i > 0) close(open, i);
        open = i;
      }
    }
    if (t == NT - 1) close(open, N);                 // the last group ends at N (position 0 is a start)
    red[t] = acc;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
      if (t < o) red[t] += red[t + o];
      __syncthreads();
    }
    if (t == 0) {
      const long long pos = total >> 16, neg = total & 0xffffu, den = 2 * pos * neg;
      out[s * P + p] = den ? (double)red[0] / (double)den : __builtin_nan("");
    }
    __syncthreads();                                  // pre / red / last_start are reused by label p + 1
  }
}

// Operating point and precision-recall sums of the same resamples: ct_clip/evaluate.py:104-113
// (choose_operating_point over roc_curve) and :116-118 (auc(recall, precision) over
// precision_recall_curve), plus sklearn's average_precision_score.  The launch shape, mult[] and the
// packed prefix pre[] are auroc_boot_kernel's; the second walk differs.
//
// A POINT is a group of bit-equal scores whose weight in the resample is > 0: pre[e] != pre[s] for
// the group [s, e).  A group of rows the resample did not draw is no point (sklearn never sees its
// score).  Points are met in ascending order, but every quantity is a function of the two prefixes
// at the group's ends, so the walk direction does not matter: down to and including the point,
//   tp = Pos - Cpos[s], fp = Neg - Cneg[s];   above it, tp' = Pos - Cpos[e], fp' = Neg - Cneg[e]
// (groups of weight 0 in between change neither).
//   * Operating point: J = tp Neg - fp Pos (int64, = Pos Neg (tpr - fpr)); the point of maximal J,
//     among equal J the larger ascending start (= the first in descending score order, as the
//     reference's strict `>` keeps it), chosen by per-thread maxima and a fixed LDS tree on
//     (J, start); reported only if J > 0 (else sensitivity = specificity = 0, threshold NaN, the
//     reference's initial values).  roc_curve's drop_intermediate=True removes only points that are
//     collinear with their neighbours at equal steps; such a point has J = (J_prev + J_next) / 2, so
//     it is maximal only if its predecessor is too: the first maximiser is never removed.
//   * pr_auc = sum (pos_g / Pos) (prec + prec') / 2 and average_precision = sum (pos_g / Pos) prec,
//     prec = tp / (tp + fp), prec' = tp' / (tp' + fp') or 1 above the first point (the curve is
//     closed at recall 0, precision 1).  Points without positives have zero width and are skipped.
//     f64 terms, no contraction; summed per thread in position order, then over the block in the
//     fixed tree: the same bits on every run, no float atomics.
// One class only: five NaN.  LDS: mult + pre + 9 KB of scratch: 25 KB (CAP 2048) / 73 KB (CAP 8192,
// still two workgroups per CU).
template <int CAP>
__global__ __launch_bounds__(NT) void curve_boot_kernel(const float* __restrict__ scores,
                                                        const uint8_t* __restrict__ labels,
                                                        const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ resample, int N, int P,
                                                        double* __restrict__ out) {
  __shared__ int mult[CAP];
  __shared__ unsigned pre[CAP + 1];
  __shared__ unsigned wave_tot[NT / 64];
  __shared__ int last_start[NT];
  __shared__ double red_auc[NT], red_ap[NT];
  __shared__ long long red_j[NT];
  __shared__ int red_i[NT];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t s = blockIdx.x;

  for (int i = t; i < N; i += NT) mult[i] = 0;
  __syncthreads();
  for (int i = t; i < N; i += NT) {
    const int r = resample[s * N + i];
    if ((unsigned)r < (unsigned)N) atomicAdd(&mult[r], 1);
  }
  __syncthreads();

  auto row = [N](int r) { return (unsigned)r < (unsigned)N ? r : 0; };
  const int L = (N + NT - 1) / NT;
  const int a = min(t * L, N), b = min(a + L, N);
  for (int p = 0; p < P; ++p) {
    const int32_t* ord = order + (int64_t)p * N;
    // walk 1 and the block scan: as in auroc_boot_kernel
    unsigned run = 0, prev_key = 0;
    int last = -1;
    if (a < b && a > 0) prev_key = __float_as_uint(scores[(int64_t)row(ord[a - 1]) * P + p]);
    for (int i = a; i < b; ++i) {
      const int r = row(ord[i]);
      const unsigned key = __float_as_uint(scores[(int64_t)r * P + p]);
      const unsigned m = (unsigned)mult[r];
      const bool start = i == 0 || key != prev_key;
      prev_key = key;
      if (start) last = i;
      pre[i] = run | (start ? 0x80000000u : 0u);
      run += labels[(int64_t)r * P + p] ? (m << 16) : m;
    }
    last_start[t] = last;
    unsigned inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    unsigned base = inc - run, total = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
      if (k < wv) base += wave_tot[k];
      total += wave_tot[k];
    }
    for (int i = a; i < b; ++i) pre[i] += base;      // base < 2^30: bit 31 is kept
    if (t == 0) pre[N] = total;
    int open = -1;
    for (int k = t - 1; k >= 0 && open < 0; --k) open = last_start[k];
    __syncthreads();
    // walk 2: every group end that closes a point
    const long long Pos = total >> 16, Neg = total & 0xffffu;
    const double dPos = (double)Pos;
    double auc = 0.0, ap = 0.0;
    long long best_j = -(1ll << 62);                  // |J| <= 2^26
    int best_i = -1;
    auto close = [&](int gs, int ge) {
      const unsigned ws = pre[gs] & 0x7fffffffu, we = pre[ge] & 0x7fffffffu;
      if (we == ws) return;                           // nothing drawn from this group: not a point
      const long long tp = Pos - (ws >> 16), fp = Neg - (ws & 0xffffu);
      const long long j = tp * Neg - fp * Pos;
      if (j >= best_j) best_j = j, best_i = gs;       // gs ascends: >= keeps the larger start
      const long long pos_g = (long long)(we >> 16) - (long long)(ws >> 16);
      if (pos_g == 0 || Neg == 0) return;             // zero width (one class: the output is NaN anyway)
      const long long tpn = Pos - (we >> 16), fpn = Neg - (we & 0xffffu);
      const double dr = (double)pos_g / dPos;
      const double prec = (double)tp / (double)(tp + fp);
      const double precn = tpn + fpn ? (double)tpn / (double)(tpn + fpn) : 1.0;
      ap = __dadd_rn(ap, __dmul_rn(dr, prec));
      auc = __dadd_rn(auc, __dmul_rn(dr, __dmul_rn(__dadd_rn(prec, precn), 0.5)));
    };
    for (int i = a; i < b; ++i) {
      if (pre[i] >> 31) {
        if (i > 0) close(open, i);
        open = i;
      }
    }
    if (t == NT - 1) close(open, N);                 // the last group ends at N (position 0 is a start)
    red_auc[t] = auc;
    red_ap[t] = ap;
    red_j[t] = best_j;
    red_i[t] = best_i;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
      if (t < o) {
        red_auc[t] = __dadd_rn(red_auc[t], red_auc[t + o]);
        red_ap[t] = __dadd_rn(red_ap[t], red_ap[t + o]);
        const long long j = red_j[t + o];
        const int i = red_i[t + o];
        if (j > red_j[t] || (j == red_j[t] && i > red_i[t])) red_j[t] = j, red_i[t] = i;
      }
      __syncthreads();
    }
    if (t == 0) {
      double* o5 = out + (s * P + p) * 5;
      const double nan = __builtin_nan("");
      if (Pos == 0 || Neg == 0) {
        o5[0] = o5[1] = o5[2] = o5[3] = o5[4] = nan;
      } else {
        const int gs = red_i[0];
        if (red_j[0] > 0 && gs >= 0) {
          const unsigned ws = pre[gs] & 0x7fffffffu;
          o5[0] = (double)(Pos - (ws >> 16)) / dPos;
          o5[1] = 1.0 - (double)(Neg - (ws & 0xffffu)) / (double)Neg;
          o5[2] = (double)scores[(int64_t)row(ord[gs]) * P + p];
        } else {
          o5[0] = 0.0, o5[1] = 0.0, o5[2] = nan;
        }
        o5[3] = red_auc[0];
        o5[4] = red_ap[0];
      }
    }
    __syncthreads();                                  // pre / red_* / last_start are reused by label p + 1
  }
}

}  // namespace

extern "C" int ctclip_curve_boot(const float* scores, const uint8_t* labels, const int32_t* order,
                                 const int32_t* resample, int32_t N, int32_t P, int32_t S, double* out, void* stream) {
  CT_REQUIRE(scores && labels && order && resample && out, CT_EINVAL);
  CT_REQUIRE(N >= 1 && N <= 8192 && P >= 1 && S >= 1, CT_ESHAPE);
  hipStream_t st = (hipStream_t)stream;
  if (N <= 2048)
    hipLaunchKernelGGL((curve_boot_kernel<2048>), dim3((unsigned)S), dim3(NT), 0, st, scores, labels, order, resample,
                       (int)N, (int)P, out);
  else
    hipLaunchKernelGGL((curve_boot_kernel<8192>), dim3((unsigned)S), dim3(NT), 0, st, scores, labels, order, resample,
                       (int)N, (int)P, out);
  CT_CHECK_LAUNCH();
  return 0;
}

extern "C" int ctclip_auroc_boot(const float* scores, const uint8_t* labels, const int32_t* order,
                                 const int32_t* resample, int32_t N, int32_t P, int32_t S, double* out, void* stream) {
  CT_REQUIRE(scores && labels && order && resample && out, CT_EINVAL);
  CT_REQUIRE(N >= 1 && N <= 8192 && P >= 1 && S >= 1, CT_ESHAPE);
  hipStream_t st = (hipStream_t)stream;
  if (N <= 2048)
    hipLaunchKernelGGL((auroc_boot_kernel<2048>), dim3((unsigned)S), dim3(NT), 0, st, scores, labels, order, resample,
                       (int)N, (int)P, out);
  else
    hipLaunchKernelGGL((auroc_boot_kernel<8192>), dim3((unsigned)S), dim3(NT), 0, st, scores, labels, order, resample,
                       (int)N, (int)P, out);
  CT_CHECK_LAUNCH();
  return 0;
}
