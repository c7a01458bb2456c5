// Fused backward kernels (Modes::bwd) and their launcher, shared by the two translation units that instantiate them:
//   ffc_k_bwd.hip   ZM = 0: recomputing form (+ the single-tile kernels, which decide at run time)
//   ffc_k_bwdz.hip  ZM = 1: on the spectra saved by the forward pass (ffc_conv_bwd_z / ffc_conv_bwd_zy)
// Two units so that the library's longest compile runs as two parallel halves, and so that a profile names the two forms apart
// (one kernel name averaged saved-spectra and recompute launches).
#pragma once
// gated rows: gate loads one chunk (both planes: 2 x 16 bytes per lane in flight) at a time: these kernels run on a 128-VGPR budget next
// to the 128 accumulation registers; with batches of 2 chunks the allocator reached into a0..a127 (build.py check_agpr), the forward
// kernels take 4 (ffc_body.h rows_store_g)
#ifndef FFC_GATE_BATCH
#define FFC_GATE_BATCH 1
#define FFC_GATE_BATCH_OUT 2
#endif
#include "ffc_dev.h"
using namespace ffc;

// GS: the du rows are stored by phase C itself (Modes::bwd; fft 32768 at L <= N/2, plain rows: ffc::direct_store_ok)
// PL: a GS kernel without the input-side arms (no input gate, no dpost: ffc::plain_rows_ok)
template <class GEO, int DT, bool HALF, int ZM, bool GS = false, bool PL = false>
__global__ __launch_bounds__(GEO::WGW * 64, 2) __attribute__((amdgpu_num_vgpr(128))) void bwd_kernel(DkfArgs d) {
  if constexpr (GEO::NW == 1) {
    // one wave per unit (fft 4096): persistent workgroups walk the (head, chunk) jobs (see conv_kernel); the waves
    // only meet at the table copy and at the end-of-chunk reduction of the dk_f sums
    const int total = ((d.c.H + 7) & ~7) * d.c.nchunk;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int h, chunk;
      if (map_id(id, d.c.H, d.c.nchunk, &h, &chunk)) Modes<DevBO, GEO, DT>::template bwd<HALF, false, true, ZM>(d, h, chunk, blockIdx.x);
    }
  } else {
    int h, chunk;
    if (!map_block(d.c.H, d.c.nchunk, &h, &chunk)) return;
    stagger_start(d.c.flags);
    Modes<DevBO, GEO, DT>::template bwd<HALF, false, true, ZM, GS, PL>(d, h, chunk, blockIdx.x);
  }
}
// single-tile sizes (fft <= 2048): persistent workgroups (two per CU) walk the (head, chunk) jobs, the plan tables are copied
// to LDS once per workgroup instead of once per job (a job is one pair per wave at B = 16: the copy was as large as the work)
template <class GEO, int DT>
__global__ __launch_bounds__(GEO::WGW * 64, 2) void bwd_kernel_small(DkfArgs d) {
  using M = Modes<DevB, GEO, DT>;
  M::BD::setup_tables(d.c.tab, d.c.t);
  if constexpr (GEO::N == 1024) { if (d.c.R > 1) M::BD::setup_tables_ipass(d.c.tab, d.c.t, d.c.R); }
  const int total = ((d.c.H + 7) & ~7) * d.c.nchunk;
  for (int id = blockIdx.x; id < total; id += gridDim.x) {
    int h, chunk;
    if (map_id(id, d.c.H, d.c.nchunk, &h, &chunk)) M::template bwd<false, false, false>(d, h, chunk, id);
  }
}
// FASTK: launched only when every tensor is 16-byte aligned and L % 8 == 0 (DkfArgs::c.fast): the row code exists once, as 16-byte
// accesses (DevBOF); FASTK = false keeps the run-time switch for ragged / misaligned calls
template <class GEO, int DT, bool HALF, int ZM, bool FASTK>
__global__ __launch_bounds__(GEO::WGW * 64, 2) __attribute__((amdgpu_num_vgpr(128))) void bwd_rp_kernel(DkfArgs d) {
  using BK = typename std::conditional<FASTK, DevBOF, DevBO>::type;
  int h, chunk;
  if (!map_block(d.c.H, d.c.nchunk, &h, &chunk)) return;
  Modes<BK, GEO, DT>::BD::setup_tables(d.c.tab, d.c.t);
  const int wv = DevBO::wave(), wg = blockIdx.x;
#pragma unroll 1
  for (int k0 = 0; k0 < d.c.R; k0++) Modes<BK, GEO, DT>::template bwd<HALF, true, true, ZM>(d, h, chunk, wg, k0, wv);
}

// the variant, grid and LDS rules are ffc::bwd_route (ffc_route.h)
template <int ZM>
struct BwdLaunchZ {
template <class GEO, int DT>
struct T {
  static int run(const DkfArgs& d, hipStream_t st) {
    static_assert(Body<DevB, GEO, DT>::IPASS_BYTES == IPASS_BYTES, "ffc_route.h");
    const BwdRoute r = bwd_route<GEO>(d, false);
    if (r.err) return ffc_fail(r.err);
    constexpr int T_ = GEO::WGW * 64;
    if constexpr (!GEO::OUTER && ZM != 0) {
      return ffc_fail("single-tile sizes are launched by the recomputing unit (run-time spectrum switch)");
    } else if constexpr (!GEO::OUTER) {
      return ffc_launch(bwd_kernel_small<GEO, DT>, "bwd_kernel", r.grid, T_, r.lds_max, r.lds, st, d);
    } else if (r.gs) {
      if constexpr (GEO::N == 32768)
        return pick([&](auto pl) -> int {
          return ffc_launch(bwd_kernel<GEO, DT, true, ZM, true, decltype(pl)::value>, "bwd_kernel (direct store)", r.grid, T_, r.lds_max, r.lds, st, d);
        }, r.pl);
      else
        return ffc_fail("internal: the backward route names a kernel that does not exist");
    } else {
      return pick([&](auto mp, auto half, auto fastk) -> int {
        constexpr bool MP = decltype(mp)::value, HALF = decltype(half)::value, FASTK = decltype(fastk)::value;
        if constexpr (MP && GEO::N == 32768)
          return ffc_launch(bwd_rp_kernel<GEO, DT, HALF, ZM, FASTK>, "bwd_rp_kernel", r.grid, T_, r.lds_max, r.lds, st, d);
        else if constexpr (!MP && !FASTK)
          return ffc_launch(bwd_kernel<GEO, DT, HALF, ZM>, "bwd_kernel", r.grid, T_, r.lds_max, r.lds, st, d);
        else
          return ffc_fail("internal: the backward route names a kernel that does not exist");
      }, r.multi_pass, r.half, r.fastk);
    }
  }
};
};
