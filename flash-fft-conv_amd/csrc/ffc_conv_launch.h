// Launcher of the forward / input-gradient kernels, shared by the two translation units that instantiate them:
//   ffc_k_conv.hip      conv_kernel / conv_rp_kernel          (DevB)
//   ffc_k_conv_res.hip  conv_res_kernel / conv_res_rp_kernel  (DevBA: an addend in the output epilogue; no frequency-sparse form)
// FAM names a unit's kernels: FAM::HAS_ADD, FAM::kernel<GEO, DT, MP, HALF, SZ, SP>() and FAM::what(multi_pass, sz, sp, outer) for the error text.
// The variant, grid and LDS rules are ffc::fwd_route (ffc_route.h).
#pragma once
#include "ffc_dev.h"

template <class FAM>
struct ConvLaunch {
template <class GEO, int DT>
struct T {
  static int run(const ffc::ConvArgs& a, hipStream_t st) {
    using namespace ffc;
    static_assert(Body<DevB, GEO, DT>::IPASS_BYTES == IPASS_BYTES, "ffc_route.h");
    const FwdRoute r = fwd_route<GEO>(a);
    if (r.err) return ffc_fail(r.err);
    if (r.gs) {      // plain rows of fft 32768 at L <= N/2: the kernels whose phase C stores the rows (FAM::kernel_gs)
      if constexpr (!FAM::HAS_ADD && GEO::N == 32768)
        return pick([&](auto sz, auto pl) -> int {      // pl: plain input rows too (ffc::plain_rows_ok)
          return ffc_launch(FAM::template kernel_gs<GEO, DT, decltype(sz)::value, decltype(pl)::value>(), FAM::what(false, decltype(sz)::value, false, true), r.grid, GEO::WGW * 64, r.lds_max, r.lds, st, a);
        }, r.sz, r.pl);
      else
        return ffc_fail("internal: the forward route names a kernel that does not exist");
    }
    return pick([&](auto mp, auto half, auto sz, auto sp) -> int {
      constexpr bool MP = decltype(mp)::value, HALF = decltype(half)::value, SZ = decltype(sz)::value, SP = decltype(sp)::value;
      if constexpr (fwd_kernel_exists<GEO>(FAM::HAS_ADD, MP, HALF, SZ, SP))
        return ffc_launch(FAM::template kernel<GEO, DT, MP, HALF, SZ, SP>(), FAM::what(MP, SZ, SP, GEO::OUTER), r.grid, GEO::WGW * 64, r.lds_max, r.lds, st, a);
      else
        return ffc_fail("internal: the forward route names a kernel that does not exist");
    }, r.multi_pass, r.half, r.sz, r.sp);
  }
};
};
