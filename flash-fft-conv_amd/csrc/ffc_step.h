// Direct step of the partial convolution (ffc_k_step.hip): a piece of L <= 64 new samples per row behind a carried state of S samples,
// y[t] = postgate[t] * sum_{j < taps} k[j] * w[S + t - j] + residual[t] on w = cat(state, x * pregate), and new_state = w[L : L + S].
// No transform and no plan.  A workgroup of 256 lanes owns one head and walks a slice of the batch: lane l owns the C taps
// [l C, (l + 1) C) of k[h] (C = 8, 16, 32 or 64, the smallest with 256 C >= taps), the row w sits in LDS in the module dtype, and every
// lane slides a window of C + 8 samples over its taps for a tile of STEP_TT = 8 outputs at a time.  DESIGN.md section 2.12.
#pragma once

namespace ffc {

constexpr int STEP_MAX = 64;          // longest piece of a step
constexpr int STEP_TT = 8;            // outputs per tile: 8 accumulators per lane, whatever L is
constexpr int STEP_LANES = 256;
constexpr int STEP_MIN_ROWS = 4;      // a workgroup of a split batch keeps at least this many rows behind one read of k[h]
constexpr int STEP_ROW_PAD = 72;      // samples behind the state in the LDS row: L <= 64 and the overshoot of the last tile

// Skewed LDS arrays of 16-byte units: one unit of padding behind every 8.  Lane l reads units at a stride of u = C / 8 (row) or
// C / 4 (k in the backward); with the skew any 8 neighbouring lanes fall on 8 different 16-byte bank groups for u = 1, 2, 4, 8 and on
// at least 4 for u = 16 (DESIGN.md section 2.12 has the arithmetic).
__host__ __device__ __forceinline__ int step_unit(int v) { return v + (v >> 3); }
static inline int step_row_units(int S) { return step_unit((S + STEP_ROW_PAD) / 8 - 1) + 1; }
static inline int step_k_units(int C) { return step_unit((STEP_LANES * C + STEP_ROW_PAD) / 4 - 1) + 1; }
static inline int step_chunk(int taps) { return taps <= 2048 ? 8 : taps <= 4096 ? 16 : taps <= 8192 ? 32 : 64; }

// The batch split, the one rule of both launches: workgroup (h, s) of the grid H x nsplit walks the rows b of [s bper, (s + 1) bper).
// nsplit grows until the grid holds two workgroups per CU, but never so far that a workgroup has fewer than STEP_MIN_ROWS rows.
static inline void step_split(int64_t B, int64_t H, int num_cu, int* nsplit, int* bper) {
  int64_t want = (2 * (int64_t)num_cu + H - 1) / H, cap = B / STEP_MIN_ROWS;
  int64_t n = want < cap ? want : cap;
  if (n < 1) n = 1;
  *bper = (int)((B + n - 1) / n);
  *nsplit = (int)((B + *bper - 1) / *bper);
}

struct StepDims {
  int B, H, L, S, Lk, taps, bper;
  int row_bytes, k_bytes;      // LDS: the row, then (backward) k[h], then the cross-wave sums / g
  int kvec;                    // k rows are 16-byte aligned: 4 taps per load
};
struct StepFwdArgs {
  StepDims d;
  const uint16_t *x, *pregate, *postgate, *residual, *state;
  const float* k;
  uint16_t *y, *new_state;
  float* raw;
};
struct StepBwdArgs {
  StepDims d;
  const uint16_t *dy, *x, *pregate, *postgate, *state, *dstate_new;
  const float *k, *raw;
  uint16_t *dx, *dpregate, *dpostgate, *dstate;
  float* dk_part;
};

#ifdef __HIPCC__
template <int DT> FFC_FN float step_f(uint16_t s) { return DevB::unpack_lo<DT>((uint32_t)s); }
template <int DT> FFC_FN uint16_t step_r(float v) { return (uint16_t)(DevB::pack<DT>(v, 0.f) & 0xffffu); }

// w = cat(state, x * pregate) of one row into the skewed LDS row: the state 16 bytes per lane, the piece sample by sample (its row in
// global memory starts at any multiple of 2 bytes), zeros up to STEP_ROW_PAD.
template <int DT>
FFC_FN void step_stage_row(u32x4v* row, const uint16_t* state, const uint16_t* x, const uint16_t* pre, int S, int L, int tid) {
  const u32x4v z = {0u, 0u, 0u, 0u};
  for (int v = tid; v < S / 8; v += STEP_LANES) row[step_unit(v)] = state ? ((const u32x4v*)state)[v] : z;
  if (tid < STEP_ROW_PAD) {
    uint16_t s = 0;
    if (tid < L) s = pre ? step_r<DT>(step_f<DT>(x[tid]) * step_f<DT>(pre[tid])) : x[tid];
    const int i = S + tid;
    ((uint16_t*)row)[step_unit(i >> 3) * 8 + (i & 7)] = s;
  }
}

// The window of lane `tid` for the tile at t0: wf[m] = w[S + t0 - (tid + 1) C + m], m < C + 8, so tap l C + jj meets output t0 + tt at
// m = C + tt - jj.  (tid + 1) C <= 256 C <= S: the window never starts below the row.
template <int DT, int C>
FFC_FN void step_window(const u32x4v* row, int S, int t0, int tid, float* wf) {
  const int v0 = (S + t0 - (tid + 1) * C) >> 3;
#pragma unroll
  for (int q = 0; q < C / 8 + 1; q++) {
    const u32x4v u = row[step_unit(v0 + q)];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      wf[8 * q + 2 * e] = DevB::unpack_lo<DT>(u[e]);
      wf[8 * q + 2 * e + 1] = DevB::unpack_hi<DT>(u[e]);
    }
  }
}

// Sum of v[0..7] over the 64 lanes of the wave in 10 exchanges: three halving steps (a lane keeps half of its values and hands the other
// half to its partner), then three plain ones.  Afterwards v[0] of lane l holds output 4 (l & 1) + 2 (l >> 1 & 1) + (l >> 2 & 1).
FFC_FN float step_wave_sum8(float* v, int lane) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const bool hi = lane & 1;
    const float keep = hi ? v[i + 4] : v[i], send = hi ? v[i] : v[i + 4];
    v[i] = keep + __shfl_xor(send, 1);
  }
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const bool hi = lane & 2;
    const float keep = hi ? v[i + 2] : v[i], send = hi ? v[i] : v[i + 2];
    v[i] = keep + __shfl_xor(send, 2);
  }
  {
    const bool hi = lane & 4;
    const float keep = hi ? v[1] : v[0], send = hi ? v[0] : v[1];
    v[0] = keep + __shfl_xor(send, 4);
  }
  float s = v[0];
  s += __shfl_xor(s, 8);
  s += __shfl_xor(s, 16);
  s += __shfl_xor(s, 32);
  return s;
}
FFC_FN int step_sum8_index(int lane) { return 4 * (lane & 1) + 2 * ((lane >> 1) & 1) + ((lane >> 2) & 1); }

template <int DT, int C, bool GATED>
FFC_FN void step_fwd_body(const StepFwdArgs& a) {
  const StepDims& d = a.d;
  u32x4v* row = (u32x4v*)ffc_smem;
  float* red = (float*)(ffc_smem + d.row_bytes);      // [wave][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x % d.H, sp = blockIdx.x / d.H;
  const int S = d.S, L = d.L, taps = d.taps;
  const int nact = (taps + C - 1) / C, nwave = (nact + 63) >> 6;      // lanes and waves that hold taps
  const bool active = tid < nact;

  float kr[C];
  {
    const float* kh = a.k + (int64_t)h * d.Lk;
    const int j0 = tid * C;
#pragma unroll
    for (int q = 0; q < C / 4; q++) {
      if (d.kvec && j0 + 4 * q + 3 < taps) {
        const f32x4 t = *(const f32x4*)(kh + j0 + 4 * q);
        kr[4 * q] = t[0]; kr[4 * q + 1] = t[1]; kr[4 * q + 2] = t[2]; kr[4 * q + 3] = t[3];
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++) kr[4 * q + e] = j0 + 4 * q + e < taps ? kh[j0 + 4 * q + e] : 0.f;
      }
    }
  }

  const int b1 = min(d.B, (sp + 1) * d.bper);
  for (int b = sp * d.bper; b < b1; b++) {
    const int64_t r = (int64_t)b * d.H + h;
    step_stage_row<DT>(row, a.state ? a.state + r * S : nullptr, a.x + r * L, GATED && a.pregate ? a.pregate + r * L : nullptr, S, L, tid);
    __syncthreads();
    if (wave < nwave) {
      for (int t0 = 0; t0 < L; t0 += STEP_TT) {
        float acc[STEP_TT];
#pragma unroll
        for (int tt = 0; tt < STEP_TT; tt++) acc[tt] = 0.f;
        if (active) {
          float wf[C + 8];
          step_window<DT, C>(row, S, t0, tid, wf);
#pragma unroll
          for (int jj = 0; jj < C; jj++)
#pragma unroll
            for (int tt = 0; tt < STEP_TT; tt++) acc[tt] = __builtin_fmaf(kr[jj], wf[C + tt - jj], acc[tt]);
        }
        const float s = step_wave_sum8(acc, lane);
        if (lane < 8) red[wave * 64 + t0 + step_sum8_index(lane)] = s;
      }
    }
    if (a.new_state) {
      // new_state[m] = w[L + m]: 16-byte stores aligned on the destination, the source read from LDS word by word at any offset
      const uint32_t* r32 = (const uint32_t*)row;
      u32x4v* ns = (u32x4v*)(a.new_state + r * S);
      for (int v = tid; v < S / 8; v += STEP_LANES) {
        const int i0 = (L + 8 * v) & ~1;      // even sample at or below the unit's first
        uint32_t w[5];
#pragma unroll
        for (int o = 0; o < 5; o++) { const int i = i0 + 2 * o; w[o] = r32[step_unit(i >> 3) * 4 + ((i & 7) >> 1)]; }
        u32x4v out;
#pragma unroll
        for (int o = 0; o < 4; o++) out[o] = (L & 1) ? (w[o] >> 16) | (w[o + 1] << 16) : w[o];
        ns[v] = out;
      }
    }
    __syncthreads();
    if (tid < L) {
      float s = 0.f;
      for (int w = 0; w < nwave; w++) s += red[w * 64 + tid];
      const int64_t o = r * L + tid;
      if (GATED) {
        if (a.raw) a.raw[o] = s;
        if (a.postgate) s *= step_f<DT>(a.postgate[o]);
        if (a.residual) s += step_f<DT>(a.residual[o]);
      }
      a.y[o] = step_r<DT>(s);
    }
  }
}

// Backward of the same shape.  k[h] sits in LDS as fp32 (skewed like the row) next to w and g = dy * postgate; dk lives in the lane's
// registers over the batch loop (the forward's window walk with the roles of k and the accumulators exchanged); dw[i] =
// sum_t g[t] k[S + t - i] runs on sub-chunks of SC outputs per lane below S and on one lane per sample of the piece; the gradient that
// arrives on new_state is staged into the row's LDS at an offset of L samples once dk is done with w, which lines it up with dw.
template <int DT, int C, bool GATED>
FFC_FN void step_bwd_body(const StepBwdArgs& a) {
  constexpr int SC = C < 16 ? C : 16;
  const StepDims& d = a.d;
  u32x4v* row = (u32x4v*)ffc_smem;
  f32x4* kl = (f32x4*)(ffc_smem + d.row_bytes);
  float* g = (float*)(ffc_smem + d.row_bytes + d.k_bytes);      // [64], zeros from L on
  const int tid = threadIdx.x;
  const int h = blockIdx.x % d.H, sp = blockIdx.x / d.H;
  const int S = d.S, L = d.L, taps = d.taps;
  const bool active = tid * C < taps;
  const bool want_dw = a.dstate || a.dx || a.dpregate;

  if (want_dw) {
    const float* kh = a.k + (int64_t)h * d.Lk;
    for (int v = tid; v < (STEP_LANES * C + STEP_ROW_PAD) / 4; v += STEP_LANES) {
      f32x4 t;
#pragma unroll
      for (int e = 0; e < 4; e++) t[e] = 4 * v + e < taps ? kh[4 * v + e] : 0.f;
      kl[step_unit(v)] = t;
    }
  }
  float dk[C];
#pragma unroll
  for (int jj = 0; jj < C; jj++) dk[jj] = 0.f;

  const int b1 = min(d.B, (sp + 1) * d.bper);
  for (int b = sp * d.bper; b < b1; b++) {
    const int64_t r = (int64_t)b * d.H + h;
    const int64_t o = r * L + tid;
    const float dyv = tid < L ? step_f<DT>(a.dy[o]) : 0.f;
    if (a.dk_part) step_stage_row<DT>(row, a.state ? a.state + r * S : nullptr, a.x + r * L, GATED && a.pregate ? a.pregate + r * L : nullptr, S, L, tid);
    if (tid < 64) g[tid] = tid < L ? (GATED && a.postgate ? dyv * step_f<DT>(a.postgate[o]) : dyv) : 0.f;
    if (GATED && a.dpostgate && tid < L) a.dpostgate[o] = step_r<DT>(dyv * a.raw[o]);
    __syncthreads();
    if (a.dk_part && active) {
      for (int t0 = 0; t0 < L; t0 += STEP_TT) {
        float wf[C + 8], gt[STEP_TT];
        step_window<DT, C>(row, S, t0, tid, wf);
#pragma unroll
        for (int tt = 0; tt < STEP_TT; tt++) gt[tt] = g[t0 + tt];
#pragma unroll
        for (int jj = 0; jj < C; jj++)
#pragma unroll
          for (int tt = 0; tt < STEP_TT; tt++) dk[jj] = __builtin_fmaf(gt[tt], wf[C + tt - jj], dk[jj]);
      }
    }
    if (!want_dw) { __syncthreads(); continue; }
    const bool has_in = a.dstate_new != nullptr;
    if (has_in) {
      // the row's LDS again: sample i <- dstate_new[i - L], zeros below L (16-byte loads, 2-byte LDS writes at the shifted place)
      if (a.dk_part) __syncthreads();
      uint16_t* r16 = (uint16_t*)row;
      const u32x4v* dn = (const u32x4v*)(a.dstate_new + r * S);
      if (tid < L) r16[step_unit(tid >> 3) * 8 + (tid & 7)] = 0;
      for (int v = tid; v < S / 8; v += STEP_LANES) {
        const u32x4v u = dn[v];
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int i = L + 8 * v + e;
          r16[step_unit(i >> 3) * 8 + (i & 7)] = (uint16_t)(e & 1 ? u[e >> 1] >> 16 : u[e >> 1] & 0xffffu);
        }
      }
      __syncthreads();
    }
    // outputs i = S - j0 below S: lane l has j0 in [l C + 1, (l + 1) C], SC at a time, the unit of i = ibase .. ibase + SC - 1
#pragma unroll
    for (int sub = 0; sub < C / SC; sub++) {
      float acc[SC];
#pragma unroll
      for (int ii = 0; ii < SC; ii++) acc[ii] = 0.f;
      if (tid * C + sub * SC + 1 < taps) {
        for (int t0 = 0; t0 < L; t0 += STEP_TT) {
          float kw[SC + 8], gt[STEP_TT];
          const int v0 = (tid * C + sub * SC + t0) >> 2;      // kw[m] = k[l C + sub SC + t0 + m]; output ii meets t0 + tt at m = SC - ii + tt
#pragma unroll
          for (int q = 0; q < SC / 4 + 2; q++) {
            const f32x4 t = kl[step_unit(v0 + q)];
            kw[4 * q] = t[0]; kw[4 * q + 1] = t[1]; kw[4 * q + 2] = t[2]; kw[4 * q + 3] = t[3];
          }
#pragma unroll
          for (int tt = 0; tt < STEP_TT; tt++) gt[tt] = g[t0 + tt];
#pragma unroll
          for (int ii = 0; ii < SC; ii++)
#pragma unroll
            for (int tt = 0; tt < STEP_TT; tt++) acc[ii] = __builtin_fmaf(gt[tt], kw[SC - ii + tt], acc[ii]);
        }
      }
      if (a.dstate) {
        const int ibase = S - tid * C - (sub + 1) * SC;
#pragma unroll
        for (int q = 0; q < SC / 8; q++) {
          u32x4v out, in = {0u, 0u, 0u, 0u};
          if (has_in) in = row[step_unit((ibase >> 3) + q)];
#pragma unroll
          for (int e = 0; e < 4; e++)
            out[e] = DevB::pack<DT>(acc[8 * q + 2 * e] + DevB::unpack_lo<DT>(in[e]), acc[8 * q + 2 * e + 1] + DevB::unpack_hi<DT>(in[e]));
          ((u32x4v*)(a.dstate + r * S))[(ibase >> 3) + q] = out;
        }
      }
    }
    if (a.dstate) {      // below S - 256 C no tap reaches: the shifted copy alone
      const u32x4v z = {0u, 0u, 0u, 0u};
      for (int v = tid; v < (S - STEP_LANES * C) / 8; v += STEP_LANES) ((u32x4v*)(a.dstate + r * S))[v] = has_in ? row[step_unit(v)] : z;
    }
    if (tid < L && (a.dx || a.dpregate)) {      // the piece itself: dxg[t'] = sum_{t >= t'} g[t] k[t - t']
      const float* kf = (const float*)kl;
      float s = 0.f;
      for (int t = tid; t < L; t++) { const int j = t - tid; s = __builtin_fmaf(g[t], kf[step_unit(j >> 2) * 4 + (j & 3)], s); }
      if (has_in) { const int i = S + tid; s += step_f<DT>(((const uint16_t*)row)[step_unit(i >> 3) * 8 + (i & 7)]); }
      const bool pre = GATED && a.pregate;
      if (a.dx) a.dx[o] = step_r<DT>(pre ? s * step_f<DT>(a.pregate[o]) : s);
      if (GATED && a.dpregate) a.dpregate[o] = step_r<DT>(s * step_f<DT>(a.x[o]));
    }
    __syncthreads();
  }
  if (a.dk_part && active) {
    float* out = a.dk_part + ((int64_t)sp * d.H + h) * taps + tid * C;
#pragma unroll
    for (int jj = 0; jj < C; jj++)
      if (tid * C + jj < taps) out[jj] = dk[jj];
  }
}
#endif

}  // namespace ffc
