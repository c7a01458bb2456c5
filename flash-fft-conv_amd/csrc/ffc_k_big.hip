// HBM-level outer DFT passes for FFT sizes >= 65536 (ffc_big.h) + C-ABI.  The level rules (dtype flags, long side, pipelined / wide form,
// workgroup counts) are in ffc_route.h.
#include "ffc_dev.h"
using namespace ffc;

// ST: batch-strided long side (BigBody's ST; BigArgs::strided picks it at launch)
template <int N0, int DT, bool FWD, bool ST = false>
__global__ __launch_bounds__(GeoBig<N0>::WGW * 64, 2) void big_kernel(BigArgs a) {
  BigBody<DevB, N0, DT, ST>::template run<FWD>(a, blockIdx.x);
}
// persistent, double-buffered form (BigBody::run_pipe): one workgroup per CU walks the blocks, the next block's rows arrive by
// LDS-DMA while the current one is transformed and stored
template <int N0, int DT, bool FWD>
__global__ __launch_bounds__((GeoBig<N0>::WGW + 1) * 64, 1) void big_pipe_kernel(BigArgs a) {      // + the loader wave
  BigBody<DevB, N0, DT>::template run_pipe<FWD>(a, blockIdx.x, gridDim.x);
}
// ---- all R passes of a factor R * 32 in one launch (BigBody::run_all): the forward reads the long side once instead of R times,
// the inverse sums the passes in its fp32 accumulators and writes the long side once (no read-modify-write between launches)
template <int DT, bool FWD, bool ST = false>
__global__ __launch_bounds__(GeoBig<32>::WGW * 64, 2) void big_all_kernel(BigArgs a) {
  BigBody<DevB, 32, DT, ST>::template run_all<FWD>(a, blockIdx.x);
}
// the WIDE form (BigBody::run_wide, round 6): the long side holds up to R * 32 rows -- fft 4194304 = 128 x 32768 and 2097152 = 64 x 32768 in ONE level at
// any length (the reference's 128- / 64-point butterflies take any length too: csrc/flashfftconv/butterfly/butterfly_padded_cuda_bf16.cu:302-487)
template <int DT, bool FWD>
__global__ __launch_bounds__(GeoBig<32>::WGW * 64, 2) void big_wide_kernel(BigArgs a) {
  BigBody<DevB, 32, DT>::template run_wide<FWD>(a, blockIdx.x);
}

// a level launch: `blocks` column blocks, `grid` workgroups on them (the pipelined form walks its blocks, every other form has one each)
template <class K>
static int launch_blocks(K kernel, const char* what, int64_t blocks, int64_t grid, int threads, int lds, const BigArgs& a, hipStream_t st) {
  if (blocks <= 0 || blocks > 2147483647LL) return ffc_fail("outer pass: bad grid");
  return ffc_launch(kernel, what, (unsigned)grid, threads, lds, lds, st, a);
}
// The pipelined form is OPT-IN (tuning flag 16, FFC_FLAGS=16) for passes that qualify (16-byte accesses, no input gate on the forward
// side): measured on MI355X it LOSES to run<> -- module level fwd / bwd ms at B16 H768, profiles/r04_ab_bigpipe.txt: fft 262144
// 12.0 / 13.7 against 11.0 / 12.8, fft 1M 49.5 / 55.5 against 47.8 / 53.6 (a first version without the loader wave: 12.6 / 14.5).  Two
// independent one-block workgroups per CU keep more of the HBM pipe busy than one workgroup that double-buffers.  Kept because the
// GPU parity suite ran green on it and the next attempt (two pipelined workgroups of 32 KB blocks) starts from here.
// A batch-strided long side (BigArgs::strided) never takes it: big_pipe_kernel has no ST = true build, such a call runs big_kernel<.., ST = true>.
template <int N0, int DT, bool FWD>
static int launch_level(const BigArgs& a, bool pipe_opt_in, int num_cu, hipStream_t st) {
  const int64_t nblk = level_blocks(a, GeoBig<N0>::Mi);
  constexpr int T = GeoBig<N0>::WGW * 64;
  if (level_pipe(a, FWD, pipe_opt_in))
    return launch_blocks(big_pipe_kernel<N0, DT, FWD>, "big_pipe_kernel", nblk, nblk < num_cu ? nblk : num_cu, T + 64, BigBody<DevB, N0, DT>::PIPE_LDS, a, st);
  return pick([&](auto strided) -> int {
    return launch_blocks(big_kernel<N0, DT, FWD, decltype(strided)::value>, "big_kernel", nblk, nblk, T, GeoBig<N0>::LDS_BYTES, a, st);
  }, a.strided != 0);
}
template <int DT, bool FWD>
static int launch_big_all(const BigArgs& a, hipStream_t st) {
  constexpr int T = GeoBig<32>::WGW * 64;
  if (a.wide) {
    const int64_t nblk = level_blocks(a, level_wide_cols(a.R));
    return launch_blocks(big_wide_kernel<DT, FWD>, "big_wide_kernel", nblk, nblk, T, GeoBig<32>::EBYTES, a, st);
  }
  const int64_t nblk = level_blocks(a, GeoBig<32>::Mi);
  return pick([&](auto strided) -> int {
    return launch_blocks(big_all_kernel<DT, FWD, decltype(strided)::value>, "big_all_kernel", nblk, nblk, T, GeoBig<32>::EBYTES, a, st);
  }, a.strided != 0);
}

// What the level entry points check and fill alike: pointers, `dtype` flags (ffc::decode_dtype), shape and long side (ffc::set_level).
// *bf: the level runs on the plan's bf16 tables.  Returns the error text, or null.
static const char* level_args(BigArgs* a, const ffc_plan* p, int dtype, int dir, const void* in, void* out, const void* gate, int64_t Bv,
                              int64_t npair, int64_t Hin, int64_t Mi, int64_t Llong, float scale, int64_t pitch_in, int64_t pitch_out,
                              int64_t pitch_gate, bool* bf) {
  a->in = in; a->out = out; a->gate = gate;
  dtype = decode_dtype(dtype, dir, a);
  if (dtype != DT_BF16 && dtype != DT_F16) return "outer pass: bad dtype";
  if (!half_rows_ok(*a, Bv, npair)) return "outer pass (half rows): one real row per head only (Bv == 1)";
  *bf = dtype == DT_BF16;
  if (!*bf && p->hp.dtype != DT_F16) return "outer pass: fp16 tables need an fp16 plan";
  return set_level(a, dir, Bv, npair, Hin, Mi, Llong, scale, pitch_in, pitch_out, pitch_gate);
}
// the plan's outer-digit operand table: pass c of a multi-pass plan in direction dir, or (c < 0) the plain one
static const uint8_t* level_mat(const ffc_plan* p, bool bf, int c, int dir) {
  const PlanTabs& t = bf ? p->hp_bf.tabs : p->hp.tabs;
  return (bf ? p->d_blob_bf : p->d_blob) + (c < 0 ? t.mat[0] : t.matk[c][dir ? 0 : 1]);
}

// One outer level.  dir = 1 forward (long side `in` (Bv,Hin,Llong) -> `out` (2*npair, Hin*N0, Mi)),
// dir = 0 inverse (`in` (2*npair, Hin*N0, Mi) -> long side `out` (Bv,Hin,Llong)).
// `plan` supplies the N0-point DFT operand table in `dtype` (any plan of a size whose outer digit is N0).
// pitch_*: batch pitches of the long-side operands in elements, 0 = contiguous (ffc::set_long_side).
extern "C" int ffc_outer_pass_strided(const ffc_plan* plan16, const ffc_plan* plan32, int n0, int dtype, int dir, const void* in, void* out,
                                      const void* gate, int64_t Bv, int64_t npair, int64_t Hin, int64_t Mi, int64_t Llong, float scale,
                                      int64_t pitch_in, int64_t pitch_out, int64_t pitch_gate, void* stream) {
  const ffc_plan* p = n0 == 16 ? plan16 : plan32;
  if (!p || !in || !out) return ffc_fail("null arg");
  if (n0 != p->hp.N1) return ffc_fail("outer pass: plan's outer digit does not match n0");
  if (Mi % (n0 == 16 ? GeoBig<16>::Mi : GeoBig<32>::Mi)) return ffc_fail("outer pass: Mi must be a multiple of the column block");
  if (Llong <= 0 || Llong > n0 * Mi) return ffc_fail("outer pass: bad length");
  BigArgs a{};
  bool bf;
  if (const char* e = level_args(&a, p, dtype, dir, in, out, gate, Bv, npair, Hin, Mi, Llong, scale, pitch_in, pitch_out, pitch_gate, &bf)) return ffc_fail(e);
  a.fmat = level_mat(p, bf, -1, dir);
  a.R = 1; a.c = 0;
  return level_dispatch(n0, !bf, dir != 0, [&](auto N0, auto DT, auto FWD) -> int {
    return launch_level<decltype(N0)::value, decltype(DT)::value, decltype(FWD)::value>(a, (p->env_flags & 16) != 0, p->num_cu, (hipStream_t)stream);
  });
}
extern "C" int ffc_outer_pass(const ffc_plan* plan16, const ffc_plan* plan32, int n0, int dtype, int dir, const void* in, void* out,
                              const void* gate, int64_t Bv, int64_t npair, int64_t Hin, int64_t Mi, int64_t Llong, float scale,
                              void* stream) {
  return ffc_outer_pass_strided(plan16, plan32, n0, dtype, dir, in, out, gate, Bv, npair, Hin, Mi, Llong, scale, 0, 0, 0, stream);
}

// One level of factor R * 32 as R passes of the 32-point kernel (BigArgs::R): fft 4194304 = 128 x 32768 in ONE HBM level when
// the long side is at most a quarter of it (Llong <= 32 * Mi, the HyenaDNA shape L = N / 4), instead of two levels of 16
// (the reference runs 4M in one level with its 128-point butterfly: csrc/flashfftconv/butterfly/butterfly_padded_cuda_bf16.cu
// :302-487, conv.py:511-551).  `plan_r`: a multi-pass plan with the same R and a 32-point outer digit (fft 131072 for R = 4):
// its per-pass outer-digit tables are the matrices needed here.  dir = 1: every pass reads the long side and writes its
// 32 rows of the R * 32 per head; dir = 0: pass c reads its rows, passes c > 0 add to the long side (call them in order).
// An output gate (dir = 0) multiplies every pass's contribution before it is added: the same product, distributed over the sum.
extern "C" int ffc_outer_pass_r_strided(const ffc_plan* plan_r, int c, int dtype, int dir, const void* in, void* out, const void* gate,
                                        int64_t Bv, int64_t npair, int64_t Hin, int64_t Mi, int64_t Llong, float scale,
                                        int64_t pitch_in, int64_t pitch_out, int64_t pitch_gate, void* stream) {
  const ffc_plan* p = plan_r;
  if (!p || !in || !out) return ffc_fail("null arg");
  if (p->hp.N1 != 32 || p->hp.R < 2) return ffc_fail("outer pass (R passes): needs a multi-pass plan with a 32-point outer digit");
  if (c < 0 || c >= p->hp.R) return ffc_fail("outer pass (R passes): bad pass index");
  if (Mi % GeoBig<32>::Mi) return ffc_fail("outer pass: Mi must be a multiple of the column block");
  if (Llong <= 0 || Llong > 32 * Mi) return ffc_fail("outer pass (R passes): the long side must fit the first 32 rows (L <= N / R)");
  BigArgs a{};
  bool bf;
  if (const char* e = level_args(&a, p, dtype, dir, in, out, gate, Bv, npair, Hin, Mi, Llong, scale, pitch_in, pitch_out, pitch_gate, &bf)) return ffc_fail(e);
  a.fmat = level_mat(p, bf, c, dir);
  a.R = p->hp.R; a.c = c;
  return level_dispatch(32, !bf, dir != 0, [&](auto N0, auto DT, auto FWD) -> int {
    if constexpr (decltype(N0)::value != 32) return ffc_fail("internal: R passes run on the 32-point kernel");
    else return launch_level<32, decltype(DT)::value, decltype(FWD)::value>(a, false, 0, (hipStream_t)stream);      // (R > 1: never pipelined)
  });
}
extern "C" int ffc_outer_pass_r(const ffc_plan* plan_r, int c, int dtype, int dir, const void* in, void* out, const void* gate,
                                int64_t Bv, int64_t npair, int64_t Hin, int64_t Mi, int64_t Llong, float scale, void* stream) {
  return ffc_outer_pass_r_strided(plan_r, c, dtype, dir, in, out, gate, Bv, npair, Hin, Mi, Llong, scale, 0, 0, 0, stream);
}

// Same level as the R calls ffc_outer_pass_r(plan_r, c = 0 .. R-1, ...), in one launch.
extern "C" int ffc_outer_pass_all_strided(const ffc_plan* plan_r, int dtype, int dir, const void* in, void* out, const void* gate,
                                          int64_t Bv, int64_t npair, int64_t Hin, int64_t Mi, int64_t Llong, float scale,
                                          int64_t pitch_in, int64_t pitch_out, int64_t pitch_gate, void* stream) {
  const ffc_plan* p = plan_r;
  if (!p || !in || !out) return ffc_fail("null arg");
  if (p->hp.N1 != 32 || p->hp.R < 2 || p->hp.R > 4) return ffc_fail("outer pass (R passes): needs a multi-pass plan with a 32-point outer digit");
  if (Mi % GeoBig<32>::Mi) return ffc_fail("outer pass: Mi must be a multiple of the column block");
  if (Llong <= 0 || Llong > (int64_t)p->hp.R * 32 * Mi) return ffc_fail("outer pass (R passes): the long side is longer than the level (L > N)");
  BigArgs a{};
  bool bf;
  if (const char* e = level_args(&a, p, dtype, dir, in, out, gate, Bv, npair, Hin, Mi, Llong, scale, pitch_in, pitch_out, pitch_gate, &bf)) return ffc_fail(e);
  for (int c = 0; c < p->hp.R; c++) a.fmats[c] = level_mat(p, bf, c, dir);
  a.fmat = a.fmats[0];
  a.R = p->hp.R; a.c = 0;
  if (level_wide(a)) {      // more than the first 32 long-side rows: the wide form
    if (const char* e = level_wide_check(a)) return ffc_fail(e);
    a.wide = 1;
  }
  return level_dispatch(32, !bf, dir != 0, [&](auto N0, auto DT, auto FWD) -> int {
    if constexpr (decltype(N0)::value != 32) return ffc_fail("internal: R passes run on the 32-point kernel");
    else return launch_big_all<decltype(DT)::value, decltype(FWD)::value>(a, (hipStream_t)stream);
  });
}
extern "C" int ffc_outer_pass_all(const ffc_plan* plan_r, int dtype, int dir, const void* in, void* out, const void* gate,
                                  int64_t Bv, int64_t npair, int64_t Hin, int64_t Mi, int64_t Llong, float scale, void* stream) {
  return ffc_outer_pass_all_strided(plan_r, dtype, dir, in, out, gate, Bv, npair, Hin, Mi, Llong, scale, 0, 0, 0, stream);
}
