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

// ---- overlap-save form on blocked rows (struct OsRows; conv_os_kernel and dkf_os_kernel): a row of L samples as nblk = ceil(L / S)
// blocks of S = N / 2, the kernels' batch B * nblk.  Single-pass sizes with an outer digit: their window has a history half.
struct OsRoute {
  int grid, lds_max, lds;
  const char* err;
};
static constexpr const char* NO_OS = "overlap-save form: fft 4096 / 8192 / 16384 / 32768, no gates";
inline int64_t os_blocks(int64_t N, int64_t L) { return (L + N / 2 - 1) / (N / 2); }
// The row copies index a tensor row in 32 bits up to one window past its end (j S + n < nblk S + S), and the batch of blocks is an int
inline const char* os_limits(int64_t N, int64_t B, int64_t H, int64_t L) {
  if (B * H * L >= ((int64_t)1 << 31) || L + N >= ((int64_t)1 << 31) || B * os_blocks(N, L) >= ((int64_t)1 << 30))
    return "overlap-save form: B * H * L and L + fft size must be below 2^31, B * blocks below 2^30";
  return nullptr;
}
static constexpr int OS_CHUNK_SEARCH = 4096;      // pairs up to which the forward launcher runs the chunk-length search of the plain forward
// a.B = B * nblk, a.L = N; grid as the plain kernels of the size take it (fft 4096: persistent, one workgroup per CU)
template <class GEO>
inline OsRoute os_route(const ConvArgs& a, const OsRows& o) {
  OsRoute r{};
  if (!GEO::OUTER || a.R > 1 || GEO::N > 32768 || a.pregate || a.postgate || o.S != GEO::N / 2 || o.nblk < 1 || o.L > (int64_t)o.nblk * o.S) {
    r.err = NO_OS;
    return r;
  }
  r.grid = ((a.H + 7) & ~7) * a.nchunk;
  if (GEO::NW == 1 && a.persist > 0 && r.grid > a.persist) r.grid = a.persist;
  r.lds_max = r.lds = GEO::LDS_BYTES;
  return r;
}
// what the two entry points fill alike: the kernels' batch and window, the tensor's strides and rows
inline void set_os_rows(ConvArgs* a, OsRows* o, int64_t N, int64_t B, int64_t H, int64_t L, int wrap) {
  o->S = (int)(N / 2); o->nblk = (int)os_blocks(N, L); o->L = (int)L; o->wrap = wrap;
  a->B = (int)(B * o->nblk); a->H = (int)H; a->L = (int)N; a->npair = (a->B + 1) / 2;
  a->sbu = a->sbg = a->sbp = a->sby = H * L;
}

// ---- gated form of the blocked rows (struct OsGate; conv_os_g_kernel and dkf_os_g_kernel): the grid and LDS of os_route, gates allowed.
// Every operand is optional (a call with none computes what the ungated kernels compute); a second output needs its gate.
static constexpr const char* NO_OS_GATED = "gated overlap-save form: fft 4096 / 8192 / 16384 / 32768, a second output only with its gate";
template <class GEO>
inline OsRoute os_gated_route(const ConvArgs& a, const OsRows& o, const OsGate& g) {
  ConvArgs plain = a;
  plain.pregate = plain.postgate = nullptr;
  OsRoute r = os_route<GEO>(plain, o);
  if (r.err || (g.out2 && !g.gate2)) r.err = NO_OS_GATED;
  return r;
}
// A block is its successor's history and a gate is read by the block's own workgroup only, so no output may share memory with any input
// of the launch, nor with the other output: tensors of `elems` 16-bit elements; null pointers take no part.
inline const char* os_alias(const void* const* outs, int nout, const void* const* ins, int nin, int64_t elems) {
  const uintptr_t bytes = (uintptr_t)elems * 2;
  for (int i = 0; i < nout; i++) {
    if (!outs[i]) continue;
    const uintptr_t w = (uintptr_t)outs[i];
    for (int j = 0; j < nin + nout; j++) {
      const void* q = j < nin ? ins[j] : outs[j - nin];
      if (!q || (j >= nin && j - nin == i)) continue;
      const uintptr_t r = (uintptr_t)q;
      if (w < r + bytes && r < w + bytes) return "gated overlap-save form: an output overlaps an input or the other output of the launch";
    }
  }
  return nullptr;
}
// the operands' batch strides for contiguous tensors (set_os_rows fills sbu / sbg / sbp / sby)
inline void set_os_gate(ConvArgs* a, OsGate* g, const void* addend, const void* gate2, void* out2, int64_t H, int64_t L) {
  a->addend = addend; a->sba = H * L;
  g->gate2 = gate2; g->out2 = out2; g->sbg2 = g->sbo2 = H * L;
}
// 16-byte accesses: L % 8 == 0 and every tensor of the launch 16-byte aligned
inline int os_fast(int64_t L, const void* const* ptrs, int n) {
  uintptr_t all = 0;
  for (int i = 0; i < n; i++) all |= (uintptr_t)ptrs[i];
  return (L % 8 == 0) && !(all & 15);
}

// ---- history form of the gated blocked rows (struct OsHist; conv_os_h_kernel and dkf_os_h_kernel): os_gated_route's grid and LDS.  The
// history feeds the wrapped window only, the state gradient comes from the natural-order window only (block -1 has no history half), and
// both tensors are always accessed 16 bytes at a time, whatever L is.
static constexpr const char* NO_OS_HIST =
    "overlap-save history form: fft 4096 / 8192 / 16384 / 32768, a history with wrap = 1 only, a state gradient with wrap = 0 only, both 16-byte aligned";
template <class GEO>
inline OsRoute os_hist_route(const ConvArgs& a, const OsRows& o, const OsGate& g, const OsHist& oh) {
  OsRoute r = os_gated_route<GEO>(a, o, g);
  if (r.err) return r;
  if ((oh.hist && !o.wrap) || (oh.dhist && o.wrap) || (((uintptr_t)oh.hist | (uintptr_t)oh.dhist) & 15) || oh.sbh % 8) r.err = NO_OS_HIST;
  return r;
}
// os_limits with the block -1 of every row counted and the (B, H, S) history tensors indexed in 32 bits
inline const char* os_hist_limits(int64_t N, int64_t B, int64_t H, int64_t L) {
  if (const char* e = os_limits(N, B, H, L)) return e;
  if (B * (os_blocks(N, L) + 1) >= ((int64_t)1 << 30) || B * H * (N / 2) >= ((int64_t)1 << 31))
    return "overlap-save history form: B * (blocks + 1) must be below 2^30, B * H * S below 2^31";
  return nullptr;
}
// os_alias with the history tensors (`helems` elements each): hist is one more input, dhist one more output
inline const char* os_hist_alias(const void* const* outs, int nout, const void* const* ins, int nin, int64_t elems, const void* hist,
                                 const void* dhist, int64_t helems) {
  if (const char* e = os_alias(outs, nout, ins, nin, elems)) return e;
  const auto hits = [](const void* p, int64_t pe, const void* q, int64_t qe) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + (uintptr_t)qe * 2 && b < a + (uintptr_t)pe * 2;
  };
  bool bad = hits(hist, helems, dhist, helems);
  for (int i = 0; i < nout; i++) bad = bad || hits(outs[i], elems, hist, helems) || hits(outs[i], elems, dhist, helems);
  for (int i = 0; i < nin; i++) bad = bad || hits(ins[i], elems, dhist, helems);
  return bad ? "overlap-save history form: an output overlaps an input or another output of the launch" : nullptr;
}
// after set_os_rows: contiguous (B, H, S) history tensors; with a state gradient every row gets its block -1
inline void set_os_hist(ConvArgs* a, OsRows* o, OsHist* oh, const void* hist, void* dhist, int64_t B, int64_t H) {
  oh->hist = hist; oh->dhist = dhist; oh->sbh = H * o->S;
  if (dhist) {
    o->nblk += 1;
    a->B = (int)(B * o->nblk); a->npair = (a->B + 1) / 2;
  }
}

// ---- frequency-sparse fused backward (bwd_sp_kernel, Modes::bwd_sp) and its dk_f -> dk kernel (dkifft_sp_kernel): refused where the
// forward's sparse form is (fwd_route: GEO::HAS_SP, single pass, 1 <= rows <= 4, no spectrum buffer); one workgroup per (head, chunk)
struct BwdSpRoute {
  bool half;
  int grid, lds_max, lds;
  const char* err;
};
static constexpr const char* NO_SPARSE_BWD = "frequency-sparse backward: fft 16384 / 32768, 1 <= rows <= 4, no spectrum buffer";
template <class GEO>
inline BwdSpRoute bwd_sp_route(const DkfArgs& d, int rows) {
  const ConvArgs& c = d.c;
  BwdSpRoute r{};
  if (!GEO::HAS_SP || c.R > 1 || rows < 1 || rows > 4 || d.zin || d.yraw) { r.err = NO_SPARSE_BWD; return r; }
  r.grid = ((c.H + 7) & ~7) * c.nchunk;
  r.lds_max = r.lds = GEO::LDS_BYTES;
  r.half = (GEO::N1 / 2) * GEO::Mi >= c.L;
  return r;
}
// workgroups of the live-row dk inverse: UPW heads each
template <class GEO>
inline int dk_sp_grid(int H) { return (H + GEO::UPW - 1) / GEO::UPW; }

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
