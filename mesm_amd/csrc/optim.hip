// Optimizer tail of the reference train loop (train.py:68-72, runner.py:348-352) on the FLAT
// parameter / gradient buffers: global-norm gradient clipping (nn.utils.clip_grad_norm_) and the
// AdamW update (torch.optim.AdamW, amsgrad off) in two launches for all 273 tensors --
// SURVEY.md §8f row 1.  HBM-bound: the update reads p, g, m, v and writes p, m, v once
// (28 B per element, 13.7 M elements = 383 MB per step).
#include "common.hpp"

namespace {

constexpr int OPT_THREADS = 256;

// GATED instantiations (the *_gated entries: the optimizer tail captured in a micro-stepped graph, graphed.py) take one
// more device word, the cycle's `due` flag, which mesm_micro_begin alone writes: when it is 0 every workgroup leaves after
// one scalar load, before it has written anything -- partials, the step counter, norm_out, p, m, v.  The ungated
// instantiations never look at the argument.

// partial sums of squares of the flat gradient buffer, one per workgroup (plain stores);
// workgroup 0 also advances the device-side step counter
template <bool GATED>
__global__ __launch_bounds__(OPT_THREADS) void sumsq_kernel(const float* __restrict__ g, int64_t n4,
                                                           float* __restrict__ partials,
                                                           int32_t* __restrict__ step,
                                                           const int32_t* __restrict__ due) {
  if constexpr (GATED) {
    if (due[0] == 0) return;
  }
  __shared__ float sh[OPT_THREADS / 64];
  float a = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * OPT_THREADS) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    a += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
    if (blockIdx.x == 0 && step) step[0] += 1;
  }
}

// total gradient norm from the partials (every workgroup sums them itself: <= 1024 floats)
__device__ __forceinline__ float total_norm(const float* __restrict__ partials, int np, float* sh) {
  float a = 0.0f;
  for (int i = threadIdx.x; i < np; i += OPT_THREADS) a += partials[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  const float t = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return sqrtf(t);
}

__global__ __launch_bounds__(OPT_THREADS) void clip_scale_kernel(float* __restrict__ g, int64_t n4,
                                                                const float* __restrict__ partials, int np,
                                                                float max_norm, float* __restrict__ norm_out) {
  __shared__ float sh[OPT_THREADS / 64];
  const float norm = total_norm(partials, np, sh);
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[0] = norm;
  const float coef = fminf(max_norm / (norm + 1e-6f), 1.0f);
  if (coef >= 1.0f) return;
  for (int64_t i = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * OPT_THREADS) {
    float4 v = reinterpret_cast<float4*>(g)[i];
    v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
    reinterpret_cast<float4*>(g)[i] = v;
  }
}

// decay of the EMA update that goes with step count `t` (the count AFTER this update's increment): n = t - 1 - step0
// averages have been taken before it; with warm-up the decay rises as (1 + n) / (10 + n) up to es->decay.  Uniform, plain
// IEEE float arithmetic; optim.py's ema_decay_at is the host mirror.
__device__ __forceinline__ float ema_decay(const MesmEmaState* __restrict__ es, int32_t t) {
  const int32_t n = t - 1 - es->step0;
  const float d = es->decay;
  const float nf = (float)(n < 0 ? 0 : n);
  return es->warmup ? fminf(d, (1.0f + nf) / (10.0f + nf)) : d;
}

// e = d * e + (1 - d) * p as one subtract and one FMA: e == p is an exact fixed point
__device__ __forceinline__ float4 ema_update(float d, const float4 e, const float (&pe)[4]) {
  return make_float4(fmaf(d, e.x - pe[0], pe[0]), fmaf(d, e.y - pe[1], pe[1]), fmaf(d, e.z - pe[2], pe[2]),
                     fmaf(d, e.w - pe[3], pe[3]));
}

// AdamW on groups of 4 elements; active4[i] == 0 skips group i (parameters that have no gradient this
// step are left untouched, exactly like torch.optim skips p.grad is None: no decay, no state update)
//
// EMA instantiations (the *_ema entries) also keep an exponential moving average of the parameters in `ema`, a buffer with
// p's layout: every group of 4 whose p is written, and no other, gets e = d * e + (1 - d) * p_new from the registers that
// hold p_new.  The other instantiations never look at the three arguments.
template <bool GATED, bool EMA>
__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    const uint8_t* __restrict__ active4, int64_t n4, const float* __restrict__ partials, int np,
    float max_norm, const float* __restrict__ lr_p, float beta1, float beta2, float eps, float wd,
    const int32_t* __restrict__ step, float* __restrict__ norm_out, const int32_t* __restrict__ due,
    float* __restrict__ ema, const MesmEmaState* __restrict__ es, float* __restrict__ decay_out) {
  if constexpr (GATED) {
    if (due[0] == 0) return;
  }
  __shared__ float sh[OPT_THREADS / 64];
  float coef = 1.0f;
  if (max_norm > 0.0f) {
    const float norm = total_norm(partials, np, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[0] = norm;
    coef = fminf(max_norm / (norm + 1e-6f), 1.0f);
  }
  const float lr = lr_p[0];
  const float t = (float)step[0];
  const float bc1 = 1.0f - powf(beta1, t);
  const float bc2 = 1.0f - powf(beta2, t);
  const float step_size = lr / bc1;
  const float inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
  const float decay = 1.0f - lr * wd;
  float ed = 0.0f;
  if constexpr (EMA) {
    ed = ema_decay(es, step[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0 && decay_out) decay_out[0] = ed;
  }
  for (int64_t i = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * OPT_THREADS) {
    if (active4 && !active4[i]) continue;
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ev;
    if constexpr (EMA) ev = reinterpret_cast<float4*>(ema)[i];
    float pe[4] = {pv.x, pv.y, pv.z, pv.w}, ge[4] = {gv.x, gv.y, gv.z, gv.w};
    float me[4] = {mv.x, mv.y, mv.z, mv.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = ge[e] * coef;
      pe[e] *= decay;
      me[e] = beta1 * me[e] + (1.0f - beta1) * gg;
      ve[e] = beta2 * ve[e] + (1.0f - beta2) * gg * gg;
      const float denom = sqrtf(ve[e]) * inv_sqrt_bc2 + eps;
      pe[e] -= step_size * (me[e] / denom);
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pe[0], pe[1], pe[2], pe[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(me[0], me[1], me[2], me[3]);
    reinterpret_cast<float4*>(v)[i] = make_float4(ve[0], ve[1], ve[2], ve[3]);
    if constexpr (EMA) reinterpret_cast<float4*>(ema)[i] = ema_update(ed, ev, pe);
  }
}

// what adamw_kernel derives from its scalar arguments, per parameter group (32 bytes: two 16-byte LDS reads)
struct alignas(16) GroupConsts {
  float step_size, inv_sqrt_bc2, decay, eps, beta1, beta2, one_m_beta1, one_m_beta2;
};

// AdamW with per-group hyperparameters: tag4[i] == 0 skips group-of-4 i (a tensor no parameter group covers, or one
// without a gradient this step), tag4[i] == k + 1 updates it with groups[k].  The constants of every group are derived
// once per workgroup from the device table, with adamw_kernel's float expressions (one group over the whole buffer gives
// adamw_kernel's bits), and kept in LDS; the per-element work is adamw_kernel's plus that indexed read, which is
// wave-uniform except where two tensors of different groups meet inside a wave.
// EMA: as in adamw_kernel; a group that is not live leaves its average alone like its p, m and v.
template <bool GATED, bool EMA>
__global__ __launch_bounds__(OPT_THREADS) void adamw_groups_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    const uint8_t* __restrict__ tag4, int64_t n4, const float* __restrict__ partials, int np, float max_norm,
    const MesmAdamGroup* __restrict__ groups, int n_groups, const int32_t* __restrict__ step,
    float* __restrict__ norm_out, const int32_t* __restrict__ due, float* __restrict__ ema,
    const MesmEmaState* __restrict__ es, float* __restrict__ decay_out) {
  if constexpr (GATED) {
    if (due[0] == 0) return;
  }
  __shared__ float sh[OPT_THREADS / 64];
  __shared__ GroupConsts gc[MESM_ADAM_MAX_GROUPS];
  __shared__ uint32_t live[MESM_ADAM_MAX_GROUPS];  // 0: a group that has not seen a step yet (t < 1) is skipped
  float coef = 1.0f;
  if (max_norm > 0.0f) {
    const float norm = total_norm(partials, np, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[0] = norm;
    coef = fminf(max_norm / (norm + 1e-6f), 1.0f);
  }
  if ((int)threadIdx.x < n_groups) {
    const MesmAdamGroup h = groups[threadIdx.x];
    const int32_t ti = step[0] - h.step0;
    const float lr = h.lr, beta1 = h.beta1, beta2 = h.beta2, wd = h.weight_decay;
    const float t = (float)(ti < 1 ? 1 : ti);  // (a skipped group divides nothing by zero)
    const float bc1 = 1.0f - powf(beta1, t);
    const float bc2 = 1.0f - powf(beta2, t);
    GroupConsts c;
    c.step_size = lr / bc1;
    c.inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    c.decay = 1.0f - lr * wd;
    c.eps = h.eps;
    c.beta1 = beta1;
    c.beta2 = beta2;
    c.one_m_beta1 = 1.0f - beta1;
    c.one_m_beta2 = 1.0f - beta2;
    gc[threadIdx.x] = c;
    live[threadIdx.x] = ti >= 1;
  }
  float ed = 0.0f;
  if constexpr (EMA) {
    ed = ema_decay(es, step[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0 && decay_out) decay_out[0] = ed;
  }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * OPT_THREADS) {
    const uint32_t k = (uint32_t)tag4[i] - 1u;  // tag 0 wraps past every group
    if (k >= (uint32_t)n_groups) continue;
    const GroupConsts c = gc[k];
    const uint32_t alive = live[k];  // (looked at after the loads: no LDS round trip in front of them)
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ev;
    if constexpr (EMA) ev = reinterpret_cast<float4*>(ema)[i];
    float pe[4] = {pv.x, pv.y, pv.z, pv.w}, ge[4] = {gv.x, gv.y, gv.z, gv.w};
    float me[4] = {mv.x, mv.y, mv.z, mv.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = ge[e] * coef;
      pe[e] *= c.decay;
      me[e] = c.beta1 * me[e] + c.one_m_beta1 * gg;
      ve[e] = c.beta2 * ve[e] + c.one_m_beta2 * gg * gg;
      const float denom = sqrtf(ve[e]) * c.inv_sqrt_bc2 + c.eps;
      pe[e] -= c.step_size * (me[e] / denom);
    }
    if (!alive) continue;
    reinterpret_cast<float4*>(p)[i] = make_float4(pe[0], pe[1], pe[2], pe[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(me[0], me[1], me[2], me[3]);
    reinterpret_cast<float4*>(v)[i] = make_float4(ve[0], ve[1], ve[2], ve[3]);
    if constexpr (EMA) reinterpret_cast<float4*>(ema)[i] = ema_update(ed, ev, pe);
  }
}

// a <-> b in place, 16 bytes per lane and pass: every float4 is read from both buffers and written to both by the one
// lane that owns it, so there is no temporary and no ordering between lanes to respect
__global__ __launch_bounds__(OPT_THREADS) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * OPT_THREADS) {
    const float4 x = reinterpret_cast<float4*>(a)[i];
    const float4 y = reinterpret_cast<float4*>(b)[i];
    reinterpret_cast<float4*>(a)[i] = y;
    reinterpret_cast<float4*>(b)[i] = x;
  }
}

// The non-finite guard between the sum of squares and a gated update (mesm_grad_guard).  Every workgroup sums the partials
// with total_norm -- the expression of the update kernels on the same operands, so `finite` is the verdict their norm would
// give -- and workgroup 0, lane 0 alone writes go, gs, step and norm_out; no workgroup reads a word another one writes in
// this launch, and none waits for another.  Only a due launch over a non-finite norm goes on to walk g: a lane counts the
// non-finite elements of its float4s in a register for as long as they fall into one segment (found by binary search in
// the table of float4 starts, which sits in LDS together with one counter per segment when LDS_TABLE), adds the run to the
// workgroup's counter when the segment changes, and each workgroup adds its non-zero counters to seg_elems once at the
// end: integer sums, whatever the arrival order.  Without LDS_TABLE (more than GUARD_LDS_SEGS segments) the table is
// searched in global memory and the workgroup's counters are a hash table in LDS: slot s % GUARD_LDS_SEGS belongs to the
// first segment that claims it (one compare-and-swap on its tag), and only a run whose slot another segment of the same
// workgroup holds goes to seg_elems directly.  A lane's run and a workgroup's counter hold at most
// 4 * n4 / gridDim.x <= 2^25 (grad_guard_blocks, n4 < 2^31): 32 bits.
constexpr int GUARD_LDS_SEGS = 2048;
constexpr int GUARD_BLOCKS = 256;  // one workgroup per CU: the finite path reads np floats per workgroup and ends

__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

template <bool LDS_TABLE>
__global__ __launch_bounds__(OPT_THREADS) void grad_guard_kernel(
    const float* __restrict__ g, int64_t n4, const int32_t* __restrict__ seg_start4, int n_seg,
    const float* __restrict__ partials, int np, const int32_t* __restrict__ due, int32_t* __restrict__ step,
    MesmGuardState* __restrict__ gs, int32_t* __restrict__ go, float* __restrict__ norm_out,
    unsigned long long* __restrict__ seg_elems) {
  const bool lane0 = blockIdx.x == 0 && threadIdx.x == 0;
  if (due && due[0] == 0) {
    if (lane0) go[0] = 0;  // (written on every launch: a 1 left by the last cycle would let this replay update)
    return;
  }
  __shared__ float sh[OPT_THREADS / 64];
  __shared__ int32_t tab_s[LDS_TABLE ? GUARD_LDS_SEGS + 1 : 1];
  __shared__ int32_t tag_s[LDS_TABLE ? 1 : GUARD_LDS_SEGS];  // the segment that owns a hashed counter, -1: none yet
  __shared__ uint32_t cnt_s[GUARD_LDS_SEGS];
  const float norm = total_norm(partials, np, sh);
  const bool bad = nonfinite(norm);
  if (lane0) {
    const int32_t attempt = gs->attempts + 1;
    gs->attempts = attempt;
    if (bad) {
      step[0] -= 1;  // the sum of squares counted an update that will not happen
      gs->skipped += 1;
      gs->consecutive += 1;
      gs->last_skipped_attempt = attempt;
    } else {
      gs->consecutive = 0;
    }
    go[0] = bad ? 0 : 1;
    if (norm_out) norm_out[0] = norm;
  }
  if (!bad) return;
  const int32_t* tab = seg_start4;
  if constexpr (LDS_TABLE) {
    for (int s = threadIdx.x; s <= n_seg; s += OPT_THREADS) tab_s[s] = seg_start4[s];
    for (int s = threadIdx.x; s < n_seg; s += OPT_THREADS) cnt_s[s] = 0u;
    __syncthreads();
    tab = tab_s;
  } else {
    for (int s = threadIdx.x; s < GUARD_LDS_SEGS; s += OPT_THREADS) {
      tag_s[s] = -1;
      cnt_s[s] = 0u;
    }
    __syncthreads();
  }
  int cur = -1;            // the segment of the run, -1: none
  int32_t b0 = 0, b1 = 0;  // its float4 range [b0, b1)
  uint32_t run = 0;
  auto flush = [&]() {
    if (cur >= 0 && run) {
      if constexpr (LDS_TABLE) {
        atomicAdd(&cnt_s[cur], run);
      } else {
        const int h = cur & (GUARD_LDS_SEGS - 1);
        const int32_t owner = atomicCAS(&tag_s[h], -1, cur);
        if (owner == -1 || owner == cur) atomicAdd(&cnt_s[h], run);
        else atomicAdd(&seg_elems[cur], (unsigned long long)run);
      }
    }
    run = 0;
  };
  for (int64_t i = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * OPT_THREADS) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    const uint32_t k = (uint32_t)nonfinite(v.x) + (uint32_t)nonfinite(v.y) + (uint32_t)nonfinite(v.z) + (uint32_t)nonfinite(v.w);
    if (k == 0) continue;
    const int32_t i4 = (int32_t)i;
    if (i4 < b0 || i4 >= b1) {
      flush();
      int lo = 0, hi = n_seg;  // the last s in [0, n_seg) with tab[s] <= i4 (0 when there is none): always inside the table
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= i4) lo = mid; else hi = mid;
      }
      cur = lo;
      b0 = tab[lo];
      b1 = tab[lo + 1];
      if (i4 < b0 || i4 >= b1) {  // an element no segment holds is not counted
        cur = -1;
        b0 = b1 = 0;
        continue;
      }
    }
    run += k;
  }
  flush();
  __syncthreads();
  if constexpr (LDS_TABLE) {
    for (int s = threadIdx.x; s < n_seg; s += OPT_THREADS) {
      const uint32_t c = cnt_s[s];
      if (c) atomicAdd(&seg_elems[s], (unsigned long long)c);
    }
  } else {
    for (int h = threadIdx.x; h < GUARD_LDS_SEGS; h += OPT_THREADS) {
      const uint32_t c = cnt_s[h];
      if (c) atomicAdd(&seg_elems[tag_s[h]], (unsigned long long)c);  // (a counter that is not 0 has an owner)
    }
  }
}

// Per-tensor statistics of the flat gradient and parameter buffers (mesm_tensor_stats): for every segment of the table and
// for g and p each, the sum of squares in fp64 -- an element is widened to double before it is squared, so a square is exact
// and neither overflows nor underflows -- and the largest magnitude as bits (the unsigned maximum of bits & 0x7fffffff: exact,
// independent of the order, a NaN above inf).  Workgroup b owns the CONTIGUOUS float4s [b * chunk4, (b + 1) * chunk4): the
// segments that meet that range are consecutive, so it accumulates them in LDS (per lane a run in registers for as long as
// its float4s fall into one segment, then ds atomics; the wave's last run through one reduction when the whole wave sits in
// one segment) and leaves each with PLAIN stores in slot s + b of a table of n_seg + gridDim.x slots: going from one
// (workgroup, segment) pair that meet to the next raises b, s or both, so no two pairs share a slot, and the host, which knows
// which workgroups meet a segment from the table and chunk4, adds their slots in ascending order.  Nothing is zeroed in
// global memory, no workgroup reads or writes a word another one writes in this launch, and none waits; the only words
// with a single writer are st->samples and st->last_attempt (workgroup 0, lane 0).  A workgroup whose range meets more than
// STATS_LDS_SEGS segments takes them in windows of that many, one after the other; the table is searched in global memory
// once, for the first segment of the range, and in LDS after that.  An element in front of the first or behind the last
// segment falls into no window's segment and is not counted.  Every index is clamped to the buffers whatever the table
// holds.
constexpr int STATS_LDS_SEGS = 512;     // 512 * (2 * 8 + 2 * 4) + 513 * 4 bytes of LDS: 14 KiB
constexpr int STATS_MAX_BLOCKS = 1024;  // four workgroups per CU
constexpr int STATS_MIN_CHUNK4 = 1024;  // float4s per workgroup before there is a second one

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  for (int o = 32; o; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o);
    v = w > v ? w : v;
  }
  return v;
}

__device__ __forceinline__ void stats_take(const float4 v, double& a, uint32_t& m) {
  const double x = (double)v.x, y = (double)v.y, z = (double)v.z, w = (double)v.w;
  a += x * x;  // (exact products: fp64 holds the square of any float)
  a += y * y;
  a += z * z;
  a += w * w;
  const uint32_t bx = __float_as_uint(v.x) & 0x7fffffffu, by = __float_as_uint(v.y) & 0x7fffffffu;
  const uint32_t bz = __float_as_uint(v.z) & 0x7fffffffu, bw = __float_as_uint(v.w) & 0x7fffffffu;
  const uint32_t mxy = bx > by ? bx : by, mzw = bz > bw ? bz : bw;
  const uint32_t q = mxy > mzw ? mxy : mzw;
  m = q > m ? q : m;
}

__global__ __launch_bounds__(OPT_THREADS) void tensor_stats_kernel(
    const float* __restrict__ g, const float* __restrict__ p, int32_t n4, int32_t chunk4,
    const int32_t* __restrict__ seg_start4, int n_seg, const int32_t* __restrict__ due, const int32_t* __restrict__ index,
    MesmStatsState* st, double* __restrict__ sumsq, uint32_t* __restrict__ absmax) {
  if (due && due[0] == 0) return;
  const int32_t every = st->every, idx = index[0];
  if (every <= 0 || idx % every != 0) return;  // (the same verdict in every workgroup: nobody writes these words here)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->samples += 1;
    st->last_attempt = idx;
  }
  __shared__ int32_t tab_s[STATS_LDS_SEGS + 1];
  __shared__ double ss_s[2][STATS_LDS_SEGS];
  __shared__ uint32_t mx_s[2][STATS_LDS_SEGS];
  const int64_t first = (int64_t)blockIdx.x * chunk4;
  if (first >= n4) return;
  int32_t lo = (int32_t)first;
  const int32_t hi = (int32_t)(first + chunk4 < (int64_t)n4 ? first + chunk4 : (int64_t)n4);
  // the last segment that starts at or before lo (the one that holds it; 0 when there is none), found by the whole workgroup
  // in two counting passes over the ascending table, every `stride`-th entry and then the entries of one stride: two global
  // loads in a row, where a binary search is a chain of up to 16 with every workgroup of the launch waiting on its own
  const int stride = (n_seg + OPT_THREADS - 1) / OPT_THREADS;
  const int j1 = (int)threadIdx.x * stride;
  int s = __syncthreads_count(j1 < n_seg && seg_start4[j1] <= lo);
  s = s > 0 ? (s - 1) * stride : 0;
  if (stride > 1) {
    const int j2 = s + (int)threadIdx.x;
    const int c = __syncthreads_count((int)threadIdx.x < stride && j2 < n_seg && seg_start4[j2] <= lo);
    s += c > 0 ? c - 1 : 0;
  }
  const int64_t n_slots = (int64_t)n_seg + gridDim.x;
  while (lo < hi && s < n_seg) {
    const int cnt = n_seg - s < STATS_LDS_SEGS ? n_seg - s : STATS_LDS_SEGS;
    for (int j = threadIdx.x; j <= cnt; j += OPT_THREADS) tab_s[j] = seg_start4[s + j];
    for (int j = threadIdx.x; j < cnt; j += OPT_THREADS) {
      ss_s[0][j] = ss_s[1][j] = 0.0;
      mx_s[0][j] = mx_s[1][j] = 0u;
    }
    __syncthreads();
    int32_t whi = tab_s[cnt] < hi ? tab_s[cnt] : hi;  // this window ends with its last segment or with the range
    if (whi < lo) whi = lo;
    int cur = -1;            // the segment of the run (window-relative), -1: none
    int32_t b0 = 0, b1 = 0;  // its float4 range [b0, b1)
    double ag = 0.0, ap = 0.0;
    uint32_t mg = 0u, mp = 0u;
    auto flush = [&]() {
      if (cur >= 0) {
        atomicAdd(&ss_s[0][cur], ag);
        atomicAdd(&ss_s[1][cur], ap);
        atomicMax(&mx_s[0][cur], mg);
        atomicMax(&mx_s[1][cur], mp);
      }
      ag = ap = 0.0;
      mg = mp = 0u;
    };
    for (int64_t i = (int64_t)lo + threadIdx.x; i < whi; i += OPT_THREADS) {
      const float4 gv = reinterpret_cast<const float4*>(g)[i];
      const float4 pv = reinterpret_cast<const float4*>(p)[i];
      const int32_t i4 = (int32_t)i;
      if (i4 < b0 || i4 >= b1) {
        flush();
        int a = 0;  // the last j in [0, cnt) with tab_s[j] <= i4 (0 when there is none): always inside the window
        for (int b = cnt; b - a > 1;) {
          const int mid = (a + b) >> 1;
          if (tab_s[mid] <= i4) a = mid; else b = mid;
        }
        cur = a;
        b0 = tab_s[a];
        b1 = tab_s[a + 1];
        if (i4 < b0 || i4 >= b1) {  // an element no segment holds is not counted
          cur = -1;
          b0 = b1 = 0;
          continue;
        }
      }
      stats_take(gv, ag, mg);
      stats_take(pv, ap, mp);
    }
    // the last run: one reduction and one lane's atomics when the whole wave ends in one segment (the usual case: a
    // tensor is much longer than a workgroup's range), every lane's own otherwise
    const int cur0 = __builtin_amdgcn_readfirstlane(cur);
    if (__all(cur == cur0)) {
      ag = wave_sum_f64(ag);
      ap = wave_sum_f64(ap);
      mg = wave_max_u32(mg);
      mp = wave_max_u32(mp);
      if ((threadIdx.x & 63) == 0) flush();
    } else {
      flush();
    }
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += OPT_THREADS) {
      const int32_t t0 = tab_s[j], t1 = tab_s[j + 1];
      if (t0 < t1 && t1 > lo && t0 < whi) {  // the segment meets [lo, whi): slot s + b is this pair's alone
        const int64_t slot = (int64_t)s + j + blockIdx.x;
        sumsq[slot] = ss_s[0][j];
        sumsq[n_slots + slot] = ss_s[1][j];
        absmax[slot] = mx_s[0][j];
        absmax[n_slots + slot] = mx_s[1][j];
      }
    }
    __syncthreads();
    lo = whi;
    s += cnt;
  }
}

inline int tensor_stats_blocks(int64_t n4) {
  int64_t b = (n4 + STATS_MIN_CHUNK4 - 1) / STATS_MIN_CHUNK4;
  if (b > STATS_MAX_BLOCKS) b = STATS_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

inline int opt_blocks(int64_t n4) {
  int64_t b = (n4 + OPT_THREADS - 1) / OPT_THREADS;
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  return (int)b;
}

inline int grad_guard_blocks(int64_t n4) {
  const int64_t b = (n4 + OPT_THREADS - 1) / OPT_THREADS;
  return (int)(b < GUARD_BLOCKS ? b : GUARD_BLOCKS);
}

template <bool GATED>
int grad_sumsq(const float* g, int64_t n, float* partials, int32_t* np_out, int32_t* step, const int32_t* due,
               void* stream) {
  if (!g || !partials || !np_out || n <= 0 || (n & 3) || ((uintptr_t)g & 15)) return MESM_EINVAL;
  if (GATED && (!due || ((uintptr_t)due & 3))) return MESM_EINVAL;
  const int nb = opt_blocks(n / 4);
  *np_out = nb;
  hipLaunchKernelGGL(sumsq_kernel<GATED>, dim3(nb), dim3(OPT_THREADS), 0, (hipStream_t)stream, g, n / 4, partials, step,
                     due);
  return mesm_launch_status();
}

// the checks the *_ema entries add to their twins' (after the twin's own MESM_EINVAL checks, before its alignment ones)
inline int ema_check(const float* ema, const MesmEmaState* es) {
  if (!ema || !es || ((uintptr_t)es & 3)) return MESM_EINVAL;
  if ((uintptr_t)ema & 15) return MESM_EALIGN;
  return 0;
}

template <bool GATED, bool EMA>
int adamw_step(float* p, const float* g, float* m, float* v, const uint8_t* active4, int64_t n, const float* partials,
               int32_t np, float max_norm, const float* lr, float beta1, float beta2, float eps, float weight_decay,
               const int32_t* step, float* norm_out, const int32_t* due, float* ema, const MesmEmaState* es,
               float* decay_out, void* stream) {
  if (!p || !g || !m || !v || !lr || !step || n <= 0 || (n & 3)) return MESM_EINVAL;
  if (GATED && (!due || ((uintptr_t)due & 3))) return MESM_EINVAL;
  if (max_norm > 0.f && (!partials || np <= 0 || np > 1024)) return MESM_EINVAL;
  if (EMA) {
    if (const int rc = ema_check(ema, es)) return rc;
  }
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) != 0) return MESM_EALIGN;
  hipLaunchKernelGGL((adamw_kernel<GATED, EMA>), dim3(opt_blocks(n / 4)), dim3(OPT_THREADS), 0, (hipStream_t)stream, p,
                     g, m, v, active4, n / 4, partials, np, max_norm, lr, beta1, beta2, eps, weight_decay, step, norm_out,
                     due, ema, es, decay_out);
  return mesm_launch_status();
}

template <bool GATED, bool EMA>
int adamw_step_groups(float* p, const float* g, float* m, float* v, const uint8_t* tag4, int64_t n,
                      const float* partials, int32_t np, float max_norm, const MesmAdamGroup* groups, int32_t n_groups,
                      const int32_t* step, float* norm_out, const int32_t* due, float* ema, const MesmEmaState* es,
                      float* decay_out, void* stream) {
  if (!p || !g || !m || !v || !tag4 || !groups || !step || n <= 0 || (n & 3)) return MESM_EINVAL;
  if (GATED && (!due || ((uintptr_t)due & 3))) return MESM_EINVAL;
  if (n_groups < 1 || n_groups > MESM_ADAM_MAX_GROUPS) return MESM_EINVAL;
  if (max_norm > 0.f && (!partials || np <= 0 || np > 1024)) return MESM_EINVAL;
  if (EMA) {
    if (const int rc = ema_check(ema, es)) return rc;
  }
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) != 0) return MESM_EALIGN;
  if (((uintptr_t)groups & 3) != 0) return MESM_EALIGN;
  hipLaunchKernelGGL((adamw_groups_kernel<GATED, EMA>), dim3(opt_blocks(n / 4)), dim3(OPT_THREADS), 0,
                     (hipStream_t)stream, p, g, m, v, tag4, n / 4, partials, np, max_norm, groups, n_groups, step, norm_out,
                     due, ema, es, decay_out);
  return mesm_launch_status();
}

}  // namespace

extern "C" int mesm_grad_sumsq(const float* g, int64_t n, float* partials, int32_t* np_out, int32_t* step,
                               void* stream) {
  return grad_sumsq<false>(g, n, partials, np_out, step, nullptr, stream);
}

extern "C" int mesm_grad_sumsq_gated(const float* g, int64_t n, float* partials, int32_t* np_out, int32_t* step,
                                     const int32_t* due, void* stream) {
  return grad_sumsq<true>(g, n, partials, np_out, step, due, stream);
}

extern "C" int mesm_clip_grad(float* g, int64_t n, const float* partials, int32_t np, float max_norm,
                              float* norm_out, void* stream) {
  if (!g || !partials || n <= 0 || (n & 3) || np <= 0 || np > 1024 || max_norm <= 0.f) return MESM_EINVAL;
  hipLaunchKernelGGL(clip_scale_kernel, dim3(opt_blocks(n / 4)), dim3(OPT_THREADS), 0, (hipStream_t)stream, g,
                     n / 4, partials, np, max_norm, norm_out);
  return mesm_launch_status();
}

extern "C" int mesm_adamw_step(float* p, const float* g, float* m, float* v, const uint8_t* active4, int64_t n,
                               const float* partials, int32_t np, float max_norm, const float* lr,
                               float beta1, float beta2, float eps, float weight_decay, const int32_t* step,
                               float* norm_out, void* stream) {
  return adamw_step<false, false>(p, g, m, v, active4, n, partials, np, max_norm, lr, beta1, beta2, eps, weight_decay,
                                  step, norm_out, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int mesm_adamw_step_gated(float* p, const float* g, float* m, float* v, const uint8_t* active4, int64_t n,
                                     const float* partials, int32_t np, float max_norm, const float* lr,
                                     float beta1, float beta2, float eps, float weight_decay, const int32_t* step,
                                     float* norm_out, const int32_t* due, void* stream) {
  return adamw_step<true, false>(p, g, m, v, active4, n, partials, np, max_norm, lr, beta1, beta2, eps, weight_decay,
                                 step, norm_out, due, nullptr, nullptr, nullptr, stream);
}

extern "C" int mesm_adamw_step_groups(float* p, const float* g, float* m, float* v, const uint8_t* tag4, int64_t n,
                                      const float* partials, int32_t np, float max_norm,
                                      const MesmAdamGroup* groups, int32_t n_groups, const int32_t* step,
                                      float* norm_out, void* stream) {
  return adamw_step_groups<false, false>(p, g, m, v, tag4, n, partials, np, max_norm, groups, n_groups, step, norm_out,
                                         nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int mesm_adamw_step_groups_gated(float* p, const float* g, float* m, float* v, const uint8_t* tag4,
                                            int64_t n, const float* partials, int32_t np, float max_norm,
                                            const MesmAdamGroup* groups, int32_t n_groups, const int32_t* step,
                                            float* norm_out, const int32_t* due, void* stream) {
  return adamw_step_groups<true, false>(p, g, m, v, tag4, n, partials, np, max_norm, groups, n_groups, step, norm_out,
                                        due, nullptr, nullptr, nullptr, stream);
}

// ---- the four updates with the weight EMA fused in (their twins' argument lists with ema, es, decay_out before stream)
extern "C" int mesm_adamw_step_ema(float* p, const float* g, float* m, float* v, const uint8_t* active4, int64_t n,
                                   const float* partials, int32_t np, float max_norm, const float* lr, float beta1,
                                   float beta2, float eps, float weight_decay, const int32_t* step, float* norm_out,
                                   float* ema, const MesmEmaState* es, float* decay_out, void* stream) {
  return adamw_step<false, true>(p, g, m, v, active4, n, partials, np, max_norm, lr, beta1, beta2, eps, weight_decay,
                                 step, norm_out, nullptr, ema, es, decay_out, stream);
}

extern "C" int mesm_adamw_step_ema_gated(float* p, const float* g, float* m, float* v, const uint8_t* active4,
                                         int64_t n, const float* partials, int32_t np, float max_norm, const float* lr,
                                         float beta1, float beta2, float eps, float weight_decay, const int32_t* step,
                                         float* norm_out, const int32_t* due, float* ema, const MesmEmaState* es,
                                         float* decay_out, void* stream) {
  return adamw_step<true, true>(p, g, m, v, active4, n, partials, np, max_norm, lr, beta1, beta2, eps, weight_decay,
                                step, norm_out, due, ema, es, decay_out, stream);
}

extern "C" int mesm_adamw_step_groups_ema(float* p, const float* g, float* m, float* v, const uint8_t* tag4, int64_t n,
                                          const float* partials, int32_t np, float max_norm,
                                          const MesmAdamGroup* groups, int32_t n_groups, const int32_t* step,
                                          float* norm_out, float* ema, const MesmEmaState* es, float* decay_out,
                                          void* stream) {
  return adamw_step_groups<false, true>(p, g, m, v, tag4, n, partials, np, max_norm, groups, n_groups, step, norm_out,
                                        nullptr, ema, es, decay_out, stream);
}

extern "C" int mesm_adamw_step_groups_ema_gated(float* p, const float* g, float* m, float* v, const uint8_t* tag4,
                                                int64_t n, const float* partials, int32_t np, float max_norm,
                                                const MesmAdamGroup* groups, int32_t n_groups, const int32_t* step,
                                                float* norm_out, const int32_t* due, float* ema,
                                                const MesmEmaState* es, float* decay_out, void* stream) {
  return adamw_step_groups<true, true>(p, g, m, v, tag4, n, partials, np, max_norm, groups, n_groups, step, norm_out,
                                       due, ema, es, decay_out, stream);
}

extern "C" int mesm_swap_f32(float* a, float* b, int64_t n, void* stream) {
  if (!a || !b || n <= 0 || (n & 3)) return MESM_EINVAL;
  if ((((uintptr_t)a | (uintptr_t)b) & 15) != 0) return MESM_EALIGN;
  if (a == b) return 0;
  hipLaunchKernelGGL(swap_kernel, dim3(opt_blocks(n / 4)), dim3(OPT_THREADS), 0, (hipStream_t)stream, a, b, n / 4);
  return mesm_launch_status();
}

extern "C" int mesm_grad_guard(const float* g, int64_t n, const int32_t* seg_start4, int32_t n_seg, const float* partials,
                               int32_t np, const int32_t* due, int32_t* step, MesmGuardState* gs, int32_t* go,
                               float* norm_out, unsigned long long* seg_elems, void* stream) {
  if (!g || !seg_start4 || !partials || !step || !gs || !go || !seg_elems || n <= 0 || (n & 3)) return MESM_EINVAL;
  if (n / 4 > INT32_MAX || n_seg < 1 || n_seg > MESM_GUARD_MAX_SEGMENTS || np <= 0 || np > 1024) return MESM_EINVAL;
  if ((uintptr_t)g & 15) return MESM_EALIGN;
  if ((((uintptr_t)seg_start4 | (uintptr_t)due | (uintptr_t)step | (uintptr_t)gs | (uintptr_t)go | (uintptr_t)norm_out) & 3) ||
      ((uintptr_t)seg_elems & 7))
    return MESM_EALIGN;
  const int64_t n4 = n / 4;
  const int nb = grad_guard_blocks(n4);
  if (n_seg <= GUARD_LDS_SEGS)
    hipLaunchKernelGGL(grad_guard_kernel<true>, dim3(nb), dim3(OPT_THREADS), 0, (hipStream_t)stream, g, n4, seg_start4, n_seg,
                       partials, np, due, step, gs, go, norm_out, seg_elems);
  else
    hipLaunchKernelGGL(grad_guard_kernel<false>, dim3(nb), dim3(OPT_THREADS), 0, (hipStream_t)stream, g, n4, seg_start4,
                       n_seg, partials, np, due, step, gs, go, norm_out, seg_elems);
  return mesm_launch_status();
}

extern "C" int32_t mesm_tensor_stats_workgroups(int64_t n) {
  if (n <= 0 || (n & 3) || n / 4 > INT32_MAX) return MESM_EINVAL;
  return tensor_stats_blocks(n / 4);
}

extern "C" int mesm_tensor_stats(const float* g, const float* p, int64_t n, const int32_t* seg_start4, int32_t n_seg,
                                 const int32_t* due, const int32_t* index, MesmStatsState* st, double* sumsq,
                                 uint32_t* absmax, void* stream) {
  if (!g || !p || !seg_start4 || !index || !st || !sumsq || !absmax || n <= 0 || (n & 3)) return MESM_EINVAL;
  if (n / 4 > INT32_MAX || n_seg < 1 || n_seg > MESM_GUARD_MAX_SEGMENTS) return MESM_EINVAL;
  if ((((uintptr_t)g | (uintptr_t)p) & 15) != 0) return MESM_EALIGN;
  if ((((uintptr_t)seg_start4 | (uintptr_t)due | (uintptr_t)index | (uintptr_t)st | (uintptr_t)absmax) & 3) ||
      ((uintptr_t)sumsq & 7))
    return MESM_EALIGN;
  const int64_t n4 = n / 4;
  const int nb = tensor_stats_blocks(n4);
  const int32_t chunk4 = (int32_t)((n4 + nb - 1) / nb);
  hipLaunchKernelGGL(tensor_stats_kernel, dim3(nb), dim3(OPT_THREADS), 0, (hipStream_t)stream, g, p, (int32_t)n4, chunk4,
                     seg_start4, n_seg, due, index, st, sumsq, absmax);
  return mesm_launch_status();
}
