// Direct step kernels of the partial convolution (ffc_step.h) + ffc_partial_step_fwd / ffc_partial_step_bwd / ffc_partial_step_nsplit.
// One instantiation per dtype x chunk class C (8, 16, 32, 64 taps per lane) x gated or plain; no plan, no tables.
#include "ffc_dev.h"
#include "ffc_step.h"
using namespace ffc;

template <int DT, int C, bool GATED>
__global__ __launch_bounds__(STEP_LANES) void step_fwd_kernel(StepFwdArgs a) { step_fwd_body<DT, C, GATED>(a); }
template <int DT, int C, bool GATED>
__global__ __launch_bounds__(STEP_LANES) void step_bwd_kernel(StepBwdArgs a) { step_bwd_body<DT, C, GATED>(a); }

namespace {

template <int DT, int C>
int step_launch_c(const StepFwdArgs& a, bool gated, dim3 grid, int lds, hipStream_t st) {
  return gated ? ffc_launch(step_fwd_kernel<DT, C, true>, "step_fwd_kernel", grid, STEP_LANES, lds, lds, st, a)
               : ffc_launch(step_fwd_kernel<DT, C, false>, "step_fwd_kernel", grid, STEP_LANES, lds, lds, st, a);
}
template <int DT, int C>
int step_launch_c(const StepBwdArgs& a, bool gated, dim3 grid, int lds, hipStream_t st) {
  return gated ? ffc_launch(step_bwd_kernel<DT, C, true>, "step_bwd_kernel", grid, STEP_LANES, lds, lds, st, a)
               : ffc_launch(step_bwd_kernel<DT, C, false>, "step_bwd_kernel", grid, STEP_LANES, lds, lds, st, a);
}
template <int DT, class A>
int step_launch_dt(const A& a, int C, bool gated, dim3 grid, int lds, hipStream_t st) {
  switch (C) {
    case 8: return step_launch_c<DT, 8>(a, gated, grid, lds, st);
    case 16: return step_launch_c<DT, 16>(a, gated, grid, lds, st);
    case 32: return step_launch_c<DT, 32>(a, gated, grid, lds, st);
    default: return step_launch_c<DT, 64>(a, gated, grid, lds, st);
  }
}
template <class A>
int step_launch(int dtype, const A& a, int C, bool gated, int nsplit, int lds, hipStream_t st) {
  const dim3 grid((unsigned)(a.d.H * nsplit));
  return dtype == DT_BF16 ? step_launch_dt<DT_BF16>(a, C, gated, grid, lds, st) : step_launch_dt<DT_F16>(a, C, gated, grid, lds, st);
}

// the checks of both entry points that need no device; the ranges come first
const char* step_limits(int dtype, int64_t B, int64_t H, int64_t L, int64_t S, int64_t Lk, int64_t taps) {
  if (L < 1 || L > STEP_MAX) return "partial step: L must be 1 .. 64";
  if (taps < 1 || taps > 16384) return "partial step: taps must be 1 .. 16384";
  if (S < 2048 || S > 16384 || (S & (S - 1))) return "partial step: S must be a power of two, 2048 .. 16384";
  if (taps > S || taps > Lk) return "partial step: taps must not exceed S or k's row length";
  if (dtype != DT_BF16 && dtype != DT_F16) return "partial step: dtype must be bf16 (0) or fp16 (1)";
  if (B < 1 || H < 1 || B * H * S >= ((int64_t)1 << 31)) return "partial step: B, H >= 1 and B * H * S below 2^31";
  return nullptr;
}
bool step_hits(const void* p, int64_t pbytes, const void* q, int64_t qbytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}
int step_num_cu() {
  static int cu[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cu[dev]) {
    hipDeviceProp_t prop;
    cu[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
  }
  return cu[dev];
}
StepDims step_dims(int64_t B, int64_t H, int64_t L, int64_t S, int64_t Lk, int64_t taps, int bper, const float* k, bool k_in_lds) {
  StepDims d{};
  d.B = (int)B; d.H = (int)H; d.L = (int)L; d.S = (int)S; d.Lk = (int)Lk; d.taps = (int)taps; d.bper = bper;
  d.row_bytes = step_row_units((int)S) * 16;
  d.k_bytes = k_in_lds ? step_k_units(step_chunk((int)taps)) * 16 : 0;
  d.kvec = !((uintptr_t)k & 15) && !(Lk & 3);
  return d;
}

}  // namespace

extern "C" {

int64_t ffc_partial_step_split(int64_t B, int64_t H, int num_cu) {
  if (B < 1 || H < 1 || num_cu < 1) return 0;
  int nsplit, bper;
  step_split(B, H, num_cu, &nsplit, &bper);
  return nsplit;
}
int64_t ffc_partial_step_nsplit(int64_t B, int64_t H) { return ffc_partial_step_split(B, H, step_num_cu()); }

int ffc_partial_step_fwd(int dtype, const void* x, const float* k, const void* pregate, const void* postgate, const void* residual,
                         const void* state, void* y, void* new_state, float* raw, int64_t B, int64_t H, int64_t L, int64_t S, int64_t Lk,
                         int64_t taps, void* stream) {
  if (const char* e = step_limits(dtype, B, H, L, S, Lk, taps)) return ffc_fail(e);
  if (!x || !k || !y) return ffc_fail("null arg");
  if (((uintptr_t)state | (uintptr_t)new_state) & 15) return ffc_fail("partial step: state and new_state must be 16-byte aligned");
  if (((uintptr_t)x | (uintptr_t)pregate | (uintptr_t)postgate | (uintptr_t)residual | (uintptr_t)y) & 1 || ((uintptr_t)k | (uintptr_t)raw) & 3)
    return ffc_fail("partial step: misaligned tensor");
  const int64_t sb = B * H * S * 2, lb = B * H * L * 2;
  if (step_hits(state, sb, new_state, sb)) return ffc_fail("partial step: new_state overlaps state");
  if (step_hits(y, lb, new_state, sb) || step_hits(x, lb, new_state, sb) || step_hits(pregate, lb, new_state, sb))
    return ffc_fail("partial step: new_state overlaps another tensor of the launch");
  int nsplit, bper;
  step_split(B, H, step_num_cu(), &nsplit, &bper);
  StepFwdArgs a{};
  a.d = step_dims(B, H, L, S, Lk, taps, bper, k, false);
  a.x = (const uint16_t*)x; a.pregate = (const uint16_t*)pregate; a.postgate = (const uint16_t*)postgate;
  a.residual = (const uint16_t*)residual; a.state = (const uint16_t*)state; a.k = k;
  a.y = (uint16_t*)y; a.new_state = (uint16_t*)new_state; a.raw = raw;
  const bool gated = pregate || postgate || residual || raw;
  return step_launch(dtype, a, step_chunk((int)taps), gated, nsplit, a.d.row_bytes + 4 * 64 * 4, (hipStream_t)stream);
}

int ffc_partial_step_bwd(int dtype, const void* dy, const void* x, const float* k, const void* pregate, const void* postgate,
                         const void* state, const float* raw, const void* dstate_new, void* dx, void* dpregate, void* dpostgate,
                         void* dstate, float* dk_part, int64_t nsplit, int64_t B, int64_t H, int64_t L, int64_t S, int64_t Lk, int64_t taps,
                         void* stream) {
  if (const char* e = step_limits(dtype, B, H, L, S, Lk, taps)) return ffc_fail(e);
  if (!dy || !x || !k) return ffc_fail("null arg");
  if (dpostgate && !raw) return ffc_fail("partial step: dpostgate needs the sums that the forward kept (raw)");
  if (dpregate && !pregate) return ffc_fail("partial step: dpregate without a pregate");
  if (((uintptr_t)state | (uintptr_t)dstate_new | (uintptr_t)dstate) & 15) return ffc_fail("partial step: state, dstate_new and dstate must be 16-byte aligned");
  if (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)pregate | (uintptr_t)postgate | (uintptr_t)dx | (uintptr_t)dpregate | (uintptr_t)dpostgate) & 1 ||
      ((uintptr_t)k | (uintptr_t)raw | (uintptr_t)dk_part) & 3)
    return ffc_fail("partial step: misaligned tensor");
  const int64_t sb = B * H * S * 2;
  if (step_hits(dstate, sb, dstate_new, sb) || step_hits(dstate, sb, state, sb)) return ffc_fail("partial step: dstate overlaps an input state");
  int ns, bper;
  step_split(B, H, step_num_cu(), &ns, &bper);
  if (dk_part && nsplit != ns) return ffc_fail("partial step: dk_part must hold ffc_partial_step_nsplit(B, H) partial sums");
  StepBwdArgs a{};
  a.d = step_dims(B, H, L, S, Lk, taps, bper, k, dstate || dx || dpregate);
  a.dy = (const uint16_t*)dy; a.x = (const uint16_t*)x; a.pregate = (const uint16_t*)pregate; a.postgate = (const uint16_t*)postgate;
  a.state = (const uint16_t*)state; a.dstate_new = (const uint16_t*)dstate_new; a.k = k; a.raw = raw;
  a.dx = (uint16_t*)dx; a.dpregate = (uint16_t*)dpregate; a.dpostgate = (uint16_t*)dpostgate; a.dstate = (uint16_t*)dstate; a.dk_part = dk_part;
  const bool gated = pregate || postgate;
  return step_launch(dtype, a, step_chunk((int)taps), gated, ns, a.d.row_bytes + a.d.k_bytes + 64 * 4, (hipStream_t)stream);
}

}  // extern "C"
