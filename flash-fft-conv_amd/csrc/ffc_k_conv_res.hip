// Forward kernels with an addend in the output epilogue: y = postgate * conv(u * pregate, k) + addend (ffc_conv_fwd_res; ConvArgs::addend,
// Body::rows_out / rows_out_g / rows_out_rp_t and the merged fft-2048 store with ADD).  The same bodies as conv_kernel / conv_rp_kernel
// (ffc_k_conv.hip) on the DevBA backend: instantiations of their own, so the kernels without an addend stay as they are.  No k -> k_f step
// inside the launch and no frequency-sparse form here.
#include "ffc_conv_launch.h"
using namespace ffc;

static constexpr int SMALL_WAVES = 2;      // as ffc_k_conv.hip
template <class GEO, int DT, bool HALF, bool SZ = false>
__global__ __launch_bounds__(GEO::WGW * 64, GEO::OUTER ? 2 : SMALL_WAVES) void conv_res_kernel(ConvArgs a) {
  using BD = Body<DevBA, GEO, DT>;
  if constexpr ((GEO::OUTER && GEO::NW == 1) || !GEO::OUTER) {
    // persistent workgroups (fft 4096: one per CU; single-tile sizes: two per CU), see conv_kernel
    BD::setup_tables(a.tab, a.t);
    const int total = ((a.H + 7) & ~7) * a.nchunk;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int h, chunk;
      if (map_id(id, a.H, a.nchunk, &h, &chunk)) BD::template conv_job<HALF, false, SZ>(a, h, chunk);
    }
  } else {
    int h, chunk;
    if (!map_block(a.H, a.nchunk, &h, &chunk)) return;
    stagger_start(a.flags);
    BD::template conv<HALF, SZ>(a, h, chunk);
  }
}

// multi-pass sizes (fft 2048, 65536, 131072), see conv_rp_kernel
template <class GEO, int DT, bool HALF, bool SZ = false>
__global__ __launch_bounds__(GEO::WGW * 64, 2) void conv_res_rp_kernel(ConvArgs a) {
  using BD = Body<DevBA, GEO, DT>;
  if constexpr (!GEO::OUTER) {
    BD::setup_tables(a.tab, a.t);
    BD::setup_tables_ipass(a.tab, a.t, a.R);
    const int total = ((a.H + 7) & ~7) * a.nchunk;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int h, chunk;
      if (map_id(id, a.H, a.nchunk, &h, &chunk)) BD::template conv_job<HALF, true, SZ>(a, h, chunk);
    }
  } else {
    int h, chunk;
    if (!map_block(a.H, a.nchunk, &h, &chunk)) return;
    BD::setup_tables(a.tab, a.t);
    BD::template conv_job<HALF, true, SZ>(a, h, chunk);
  }
}

// this unit's kernels for the shared launcher (ffc_conv_launch.h)
struct ConvResKernels {
  static constexpr bool HAS_ADD = true;
  template <class GEO, int DT, bool MP, bool HALF, bool SZ, bool SP>
  static constexpr auto kernel() {
    if constexpr (MP) return conv_res_rp_kernel<GEO, DT, HALF, SZ>;
    else return conv_res_kernel<GEO, DT, HALF, SZ>;
  }
  static const char* what(bool mp, bool sz, bool, bool outer) {
    if (mp) return sz && outer ? "conv_res_rp_kernel (spectrum-saving)" : "conv_res_rp_kernel";
    return sz ? "conv_res_kernel (spectrum-saving)" : "conv_res_kernel";
  }
};

int ffc_conv_res_launch(int N, int dtype, const ConvArgs& a, hipStream_t st) {
  return ffc_dispatch<ConvLaunch<ConvResKernels>::T>(N, dtype, a, st);
}

