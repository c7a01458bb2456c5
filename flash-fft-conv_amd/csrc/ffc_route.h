// Host launch rules: which kernel instantiation a call runs, with which grid and how much LDS.  Plain C++17, no device code: the HIP
// launchers (through ffc_dev.h) and the CPU wave simulator (ffc_sim.cpp) both ask these functions, so that the simulator runs the
// instantiation the library launches.  tests/test_launch_rules.py pins the values.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "ffc_body.h"
#include "ffc_modes.h"
#include "ffc_big.h"

namespace ffc {

// Run-time booleans -> template arguments: pick(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...), so a
// launcher names each instantiation once, guarded by `if constexpr` where a combination has no kernel.
template <class F>
inline int pick(F&& f) { return f(); }
template <class F, class... Bs>
inline int pick(F&& f, bool b, Bs... bs) {
  return b ? pick([&](auto... r) { return f(std::true_type{}, r...); }, bs...)
           : pick([&](auto... r) { return f(std::false_type{}, r...); }, bs...);
}
// the level passes: f(N0, DT, FWD) with the run-time outer digit (16 / 32), table dtype and direction as compile-time constants
template <class F>
inline int level_dispatch(int n0, bool f16, bool fwd, F&& f) {
  return pick([&](auto n32, auto h, auto fw) -> int {
    return f(std::integral_constant<int, decltype(n32)::value ? 32 : 16>{}, std::integral_constant<int, decltype(h)::value ? DT_F16 : DT_BF16>{}, fw);
  }, n0 == 32, f16, fwd);
}

// fft size -> Geo<N1, N2, N3>: f(Geo<..>{}) for a supported size, false otherwise
template <class F>
inline bool with_geo(int N, F&& f) {
  switch (N) {
    case 256: f(Geo<1, 16, 16>{}); return true;
    case 512: f(Geo<1, 16, 32>{}); return true;
    case 1024: case 2048: f(Geo<1, 32, 32>{}); return true;      // 2048: 2 passes of the 1024 kernel (inner-only multi-pass form, Body::InnerPass)
    case 4096: f(Geo<16, 16, 16>{}); return true;
    case 8192: f(Geo<32, 16, 16>{}); return true;
    case 16384: f(Geo<16, 32, 32>{}); return true;
    case 32768: case 65536: case 131072: f(Geo<32, 32, 32>{}); return true;      // multi-pass sizes: R passes of the 32768 kernel (HostPlan::R, struct Pass)
  }
  return false;
}

static constexpr int IPASS_BYTES = 2 * 6144 + 2 * 8192;      // == Body<..>::IPASS_BYTES (the launchers assert it): per-pass tables of fft 2048
static constexpr const char* NO_MULTI_PASS = "multi-pass plan on a geometry without multi-pass kernels";

// grid cap of the persistent single-tile kernels: two workgroups per CU (FFC_PERSIST=0: uncapped)
inline int cap_two_per_cu(int grid, int persist) {
  const int cap = (persist > 0 && persist < (1 << 29)) ? 2 * persist : (1 << 30);
  return grid > cap ? cap : grid;
}

// ---- forward / input-gradient kernels (conv_kernel, conv_rp_kernel and their addend forms conv_res_*)
struct FwdRoute {
  bool multi_pass;      // conv_rp_kernel: the R passes of a job in one workgroup (fft 2048, 65536, 131072)
  bool half;            // HALF: L <= N/2 of a 32-point outer digit (N/4 .. of the multi-pass sizes): only E rows < 16 carry data
  bool sz;              // SZ: also stores the spectra and / or the output before the postgate
  bool sp;              // SP: frequency-sparse k_f
  int grid, lds_max, lds;      // workgroups, dynamic-LDS limit of the kernel, dynamic LDS of this launch
  const char* err;      // non-null: no kernel for this call
  bool gs;              // GS: phase C stores the output rows itself (Body::outer_inv_half<true>), see direct_store_ok
  bool pl;              // PL: a GS kernel whose input rows are plain at compile time as well, see plain_rows_ok
};
// Where phase C may store its rows straight to global memory: single-pass fft 32768 at L <= N/2, plain output rows -- 16-byte-aligned
// tensors with L % 8 == 0 (`fast`), and nothing that multiplies, adds to or copies the rows on their way out (`plain`).  Tuning flag 256
// keeps the earlier stages and rows_out everywhere.
template <class GEO>
inline bool direct_store_ok(bool half, bool multi_pass, int fast, bool plain, int flags) {
  return GEO::N == 32768 && half && !multi_pass && fast && plain && !(flags & 256);
}
// Where the rows also come IN plain: a direct-store call (so 16-byte rows: `fast`) with nothing that multiplies the input rows or takes a
// side product from them (`plain_in`).  Those calls run the PL form of the GS kernels, which has no gate, side-product or element-wise arm
// in its pair loop (Body::rows_load_pl; the backward on saved spectra takes its rows by LDS-DMA unconditionally, so tuning flag 8 is part
// of its `plain_in`).  Tuning flag 512 keeps the GS kernels with the run-time arms.
inline bool plain_rows_ok(bool gs, bool plain_in, int flags) { return gs && plain_in && !(flags & 512); }
template <class GEO>
inline FwdRoute fwd_route(const ConvArgs& a) {
  FwdRoute r{};
  r.grid = ((a.H + 7) & ~7) * a.nchunk;
  r.lds_max = r.lds = GEO::LDS_BYTES;
  if (a.R > 1) {
    r.multi_pass = true;
    if (GEO::N == 32768) {
      r.half = 16 * GEO::Mi >= a.L;
      r.sz = a.zsave != nullptr;
    } else if (GEO::N == 1024) {
      r.sz = a.zsave || a.yraw;
      r.grid = cap_two_per_cu(r.grid, a.persist);
      r.lds_max = GEO::LDS_BYTES + 2 * IPASS_BYTES;
      r.lds = GEO::LDS_BYTES + a.R * IPASS_BYTES;
    } else {
      r.err = NO_MULTI_PASS;
    }
    return r;
  }
  if (GEO::OUTER && GEO::NW == 1 && r.grid > a.persist) r.grid = a.persist;      // persistent: one workgroup per CU (fft 4096)
  if (!GEO::OUTER && a.persist > 0 && a.persist < (1 << 29) && r.grid > 2 * a.persist) r.grid = 2 * a.persist;      // two per CU
  r.half = GEO::OUTER && (GEO::N1 / 2) * GEO::Mi >= a.L;
  if (a.sparse) {
    if (GEO::HAS_SP) r.sp = true;
    else r.err = "frequency-sparse kernel: fft 16384 / 32768 only";
    return r;
  }
  // y_raw without the spectra: the single-tile sizes only
  r.sz = a.zsave || (!GEO::OUTER && a.yraw);
  r.gs = direct_store_ok<GEO>(r.half, false, a.fast, !a.postgate && !a.addend && !a.yraw, a.flags);
  r.pl = plain_rows_ok(r.gs, !a.pregate && !a.aux_in, a.flags);
  return r;
}
// the forward instantiations that exist (add: the family with an addend in the output epilogue has no frequency-sparse form)
template <class GEO>
constexpr bool fwd_kernel_exists(bool add, bool multi_pass, bool half, bool sz, bool sp) {
  if (multi_pass) return !sp && (GEO::N == 32768 || (GEO::N == 1024 && !half));
  if (sp) return GEO::HAS_SP && !add && !sz;
  return GEO::OUTER || !half;
}

// ---- backward kernels: bwd_kernel / bwd_rp_kernel / bwd_kernel_small (dkf = false) and dkf_kernel / dkf_rp_kernel / dkf_kernel_small
struct BwdRoute {
  bool multi_pass;      // *_rp_kernel (fft 65536 / 131072; fft 2048 runs its passes inside the single-tile kernel)
  bool half;
  bool fastk;           // bwd_rp_kernel only: the 16-byte-only instantiation (aligned tensors, L % 8 == 0; build switch FFC_RP_FASTK)
  bool small;           // single-tile kernel
  int grid, lds_max, lds;
  const char* err;
  bool gs;              // bwd_kernel only: the du rows from phase C itself (no input gate, no dpregate), see direct_store_ok
  bool pl;              // bwd_kernel only: a GS kernel whose dout (and u) rows come in plain as well, see plain_rows_ok
};
template <class GEO>
inline BwdRoute bwd_route(const DkfArgs& d, bool dkf) {
  const ConvArgs& c = d.c;
  BwdRoute r{};
  r.grid = ((c.H + 7) & ~7) * c.nchunk;
  r.lds_max = r.lds = GEO::LDS_BYTES;
  if (c.R > 1 && GEO::OUTER) {
    if (GEO::N != 32768) { r.err = NO_MULTI_PASS; return r; }
    r.multi_pass = true;
    r.half = 16 * GEO::Mi >= c.L;
    r.fastk = !dkf && c.fast && (FFC_RP_FASTK != 0);
    return r;
  }
  if (GEO::OUTER) {
    if (GEO::NW == 1 && c.persist > 0 && r.grid > c.persist) r.grid = c.persist;      // persistent: one workgroup per CU (fft 4096)
    r.half = (GEO::N1 / 2) * GEO::Mi >= c.L;
    r.gs = !dkf && direct_store_ok<GEO>(r.half, false, c.fast, !c.pregate && !d.dpre, c.flags);
    r.pl = plain_rows_ok(r.gs, !c.postgate && !d.dpost && !d.yraw && !(c.flags & 8), c.flags);
    return r;
  }
  r.small = true;
  if (c.R > 1 && GEO::N != 1024) { r.err = NO_MULTI_PASS; return r; }
  r.lds_max = GEO::LDS_BYTES + 2 * IPASS_BYTES;      // inner-only multi-pass form (fft 2048): per-pass tables behind the plan tables
  r.lds = GEO::LDS_BYTES + (c.R > 1 ? c.R * IPASS_BYTES : 0);
  if (!dkf) r.grid = cap_two_per_cu(r.grid, c.persist);      // bwd_kernel_small is persistent, dkf_kernel_small is not
  return r;
}

// ---- steps a convolution launch may take over from a launch of their own (flags: the plan's tuning flags, FFC_FLAGS)
// k -> k_f inside the forward launch (Modes::kfft_head): a workgroup owns its head, fft 8192 / 16384 / 32768 (the sizes whose waves
// meet at workgroup barriers anyway); tuning flag 64 keeps the separate launch
inline bool fwd_takes_kfft(const HostPlan& hp, int nchunk, int sparse, int flags) {
  return nchunk == 1 && hp.N >= 8192 && hp.N <= 32768 && hp.R == 1 && !sparse && !(flags & 64);
}
// dk out of the backward launch: the workgroup owns all pairs of its head.  Tuning flag 32 keeps the slab + ffc_kernel_ifft_grad pair.
enum { DK_SEPARATE = 0, DK_TAIL = 1, DK_TAIL_MULTI = 2 };
// Modes::dk_tail, real dk or complex rows: fft 16384 / 32768 (fft 8192: the tail runs on 2 of the workgroup's 8 waves and measured
// +-0 / +2 % on the backward call, profiles/r04_ab_launch_fusion.txt: kept on the separate kernel unless tuning flag 128 asks for it)
inline bool bwd_takes_dk(const HostPlan& hp, int nchunk, int flags) {
  return nchunk == 1 && hp.N >= ((flags & 128) ? 8192 : 16384) && hp.N <= 32768 && hp.R == 1 && !(flags & 32);
}
// Modes::dk_tail_rp: every pass of fft 65536 / 131072 ends with its share of dk (bf16 plans, real dk only)
inline bool bwd_takes_dk_multi(const HostPlan& hp, int nchunk, int flags) {
  return nchunk == 1 && hp.R > 1 && hp.N1 > 1 && hp.dtype == DT_BF16 && !(flags & 32);
}
inline int bwd_dk_form(const HostPlan& hp, int nchunk, int flags, bool complex_rows) {
  if (bwd_takes_dk(hp, nchunk, flags)) return DK_TAIL;
  return (!complex_rows && bwd_takes_dk_multi(hp, nchunk, flags)) ? DK_TAIL_MULTI : DK_SEPARATE;
}
// the tail's fields: dk (H, Lk) fp32, or complex rows `pair` (pair-plane tensor (2, H, N) bf16) with the caller's scale; the tail runs on
// the plan's bf16 tables
inline void set_dk_tail(DkfArgs* d, float* dk, void* pair, int Lk, float scale, int fast, const uint8_t* tab_bf, const PlanTabs& t_bf) {
  d->dk_out = dk; d->dk_pair = pair; d->Lk = Lk; d->dk_scale = scale; d->dk_fast = fast;
  d->tab_bf = tab_bf; d->t_bf = t_bf;
}

// ---- HBM-level passes (ffc_big.h)
// `dtype` of the level entry points: bits 0..3 the 16-bit type; | FFC_LONG_F32 (16): the long side is fp32 (dir = 1: `in` is read as
// float, multiplied by 2^e, e = bits 8..15, and rounded to the 16-bit type; dir = 0: `out` is written as float).  Gates stay 16-bit.
// | FFC_HALF_ROWS (32): the long side is one REAL row per head (Bv == 1) and the short side holds the rows k0 <= K / 2 only (BigArgs::half).
inline int decode_dtype(int dtype, int dir, BigArgs* a) {
  a->lf32 = (dtype & 16) ? 1 : 0;
  a->half = (dtype & 32) ? 1 : 0;
  const int e = (dtype >> 8) & 0xff;
  if (e > 30 || (e && !(a->lf32 && dir))) return -1;
  a->lpre = (float)(1u << e);
  return dtype & 15;
}
// The long side of a level: batch pitches in elements (0 = contiguous, Hin * Llong) of `in` (dir = 1) / `out` (dir = 0) and of the gate, and
// whether it takes 16-byte accesses: rows of a multiple of 8 elements, every base pointer 16-byte aligned, every pitch a multiple of 8.
// Otherwise the element-wise path runs, as it does for odd Llong.  The short side is always contiguous: its pitch must be given as 0.
inline const char* set_long_side(BigArgs* a, int dir, int64_t Hin, int64_t Llong, int64_t pitch_in, int64_t pitch_out, int64_t pitch_gate) {
  const int64_t hl = Hin * Llong;
  if ((dir ? pitch_out : pitch_in) != 0) return "outer pass: the short side (pair-plane tensor) is contiguous, its pitch must be 0";
  int64_t pl = dir ? pitch_in : pitch_out, pg = a->gate ? pitch_gate : 0;
  if (!pl) pl = hl;
  if (!pg) pg = hl;
  if (pl < hl || pg < hl) return "outer pass: a batch pitch is smaller than Hin * Llong";
  if (a->lf32 && pl != hl) return "outer pass: the fp32 long side is contiguous";
  a->pin = dir ? pl : 0; a->pout = dir ? 0 : pl; a->pgate = pg;
  a->strided = (pl != hl || pg != hl) ? 1 : 0;
  a->fast = (Llong % 8 == 0) && !(((uintptr_t)a->in | (uintptr_t)a->out | (uintptr_t)a->gate) & 15) && !((pl | pg) & 7);
  return nullptr;
}
// the half-row form (BigArgs::half) takes one real row per head
inline bool half_rows_ok(const BigArgs& a, int64_t Bv, int64_t npair) { return !a.half || (Bv == 1 && npair == 1); }
// the shape and the long side, which every level entry point fills the same way
inline const char* set_level(BigArgs* a, int dir, int64_t Bv, int64_t npair, int64_t Hin, int64_t Mi, int64_t Llong, float scale,
                             int64_t pitch_in, int64_t pitch_out, int64_t pitch_gate) {
  a->Bp_valid = (int)Bv; a->npair = (int)npair; a->Hin = (int)Hin; a->Mi = (int)Mi; a->Llong = (int)Llong; a->scale = scale;
  return set_long_side(a, dir, Hin, Llong, pitch_in, pitch_out, pitch_gate);
}
// big_pipe_kernel (persistent, double-buffered) is opt-in (the library: tuning flag 16) for plain levels with 16-byte accesses and no input
// gate on the forward side; a batch-strided long side never takes it
inline bool level_pipe(const BigArgs& a, bool fwd, bool opt_in) {
  return opt_in && a.R == 1 && a.fast && !a.lf32 && !a.half && !a.strided && !(fwd && a.gate);
}
// all R passes in one launch: the wide form when the long side reaches beyond the first 32 rows
inline bool level_wide(const BigArgs& a) { return a.Llong > 32 * a.Mi; }
inline const char* level_wide_check(const BigArgs& a) {
  if (a.strided) return "outer pass (R passes), wide form: contiguous long side only";
  if (a.lf32 || a.half) return "outer pass (R passes), long side beyond the first 32 rows: 16-bit rows and all short-side rows only";
  if (GeoBig<32>::WGW % a.R) return "outer pass (R passes), wide form: R must divide the workgroup's waves";
  return nullptr;
}
// workgroups of a level: one per block of `cols` columns; the wide form's block is WGW / R groups of 128, R waves (passes / row blocks) on each
inline int level_wide_cols(int R) { return 128 * (GeoBig<32>::WGW / R); }
inline int64_t level_blocks(const BigArgs& a, int cols) { return (int64_t)a.npair * a.Hin * (a.Mi / cols); }

}  // namespace ffc
