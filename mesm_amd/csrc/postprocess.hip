// Submission rows on the device: the ranked, rounded `pred_relevant_windows` of eval.py:63-92 /
// utils/post_processing.py:22-47, bit-identical to mesm_amd.postprocess.predict_windows (the host referee).
#include "common.hpp"

namespace {

constexpr int ROWS_WAVES = 4;  // queries per workgroup: one wave64 each, one lane per row

// float(f"{x:.4f}") of a float32 x: the product is exact (24 + 14 significand bits fit in 53), rint rounds the exact
// decimal value half-to-even like Python's formatting, and the correctly rounded division gives the double nearest to
// q / 10^4, which is what float() parses.  Signs of zero survive both steps (-0.00001 -> -0.0, like Python).
__device__ __forceinline__ double round4(float x) {
  return __ddiv_rn(rint(__dmul_rn((double)x, 1e4)), 1e4);
}

__global__ __launch_bounds__(64 * ROWS_WAVES) void windows_rows_kernel(
    const float* __restrict__ logits, const float* __restrict__ spans, const float* __restrict__ duration,
    double* __restrict__ out, int N, int Q, float clip_len, int snap, float lo, float hi, int sort) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * ROWS_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;  // (whole waves: every lane of a live wave reaches the shuffles below)
  const bool live = lane < Q;
  const int i = n * Q + (live ? lane : 0);
  // windows_kernel's arithmetic, operation for operation (eltwise.hip): the raw rows equal raw_windows() bit for bit
  const float l0 = logits[2 * i], l1 = logits[2 * i + 1];
  const float m = fmaxf(l0, l1);
  const float e0 = expf(l0 - m), e1 = expf(l1 - m);
  const float cx = spans[2 * i], w = spans[2 * i + 1];
  const float d = duration[n];
  const float hw = __fmul_rn(0.5f, w);
  const float st = __fmul_rn(__fsub_rn(cx, hw), d);
  const float ed = __fmul_rn(__fadd_rn(cx, hw), d);
  const float sc = __fdiv_rn(e0, __fadd_rn(e0, e1));
  // stable descending rank: the rows with a higher score, plus the tied rows in front of this one (Python's
  // sorted(..., reverse=True) keeps ties in their order).  A NaN score ranks like -inf: the ranks stay a permutation
  int rank = lane;
  if (sort) {
    const float key = isnan(sc) ? -INFINITY : sc;
    rank = 0;
    for (int k = 0; k < Q; ++k) {
      const float kk = __shfl(key, k, 64);
      rank += (kk > key || (kk == key && k < lane)) ? 1 : 0;
    }
  }
  if (!live) return;
  // predict_windows: round to 4 decimals, float32, clamp, snap to the clip grid; the score rounded, cast to float32 and
  // rounded again
  float ws = (float)round4(st), we = (float)round4(ed);
  // np.clip / torch.clamp: x is replaced only when it lies strictly outside, so -0.0 against a bound of 0 stays -0.0
  ws = ws < lo ? lo : ws;
  ws = ws > hi ? hi : ws;
  we = we < lo ? lo : we;
  we = we > hi ? hi : we;
  if (snap) {
    ws = __fmul_rn(rintf(__fdiv_rn(ws, clip_len)), clip_len);
    we = __fmul_rn(rintf(__fdiv_rn(we, clip_len)), clip_len);
  }
  const double s4 = round4((float)round4(sc));
  double* o = out + 3 * ((int64_t)n * Q + rank);
  o[0] = (double)ws;
  o[1] = (double)we;
  o[2] = s4;
}

}  // namespace

extern "C" int mesm_windows_rows(const float* logits, const float* spans, const float* duration, double* out,
                                 int32_t N, int32_t Q, float clip_len, float min_ts_val, float max_ts_val,
                                 int32_t sort, void* stream) {
  if (!logits || !spans || !duration || !out || N <= 0 || Q <= 0 || Q > 64) return MESM_EINVAL;
  const int snap = clip_len != -1.0f;
  if (snap && !(clip_len != 0.0f)) return MESM_EINVAL;
  hipLaunchKernelGGL(windows_rows_kernel, dim3((unsigned)((N + ROWS_WAVES - 1) / ROWS_WAVES)), dim3(64 * ROWS_WAVES),
                     0, (hipStream_t)stream, logits, spans, duration, out, N, Q, clip_len, snap, min_ts_val, max_ts_val,
                     sort ? 1 : 0);
  return mesm_launch_status();
}
