// Forward kernels with an addend in the output epilogue: y = postgate * conv(u * pregate, k) + addend (ffc_conv_fwd_res; ConvArgs::addend,
// Body::rows_out / rows_out_g / rows_out_rp_t and the merged fft-2048 store with ADD).  The same bodies as conv_kernel / conv_rp_kernel
// (ffc_k_conv.hip) on the DevBA backend: instantiations of their own, so the kernels without an addend stay as they are.  No k -> k_f step
// inside the launch and no frequency-sparse form here.
#include "ffc_dev.h"
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

template <class K>
static int launch_res(K kernel, const char* what, int grid, int threads, int lds_max, int lds, const ConvArgs& a, hipStream_t st) {
  int rc = ffc_set_lds(kernel, lds_max);
  if (rc) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : ffc_fail(std::string(what) + " launch: " + hipGetErrorString(e));
}

// the grid and variant rules of ConvLaunch (ffc_k_conv.hip)
template <class GEO, int DT>
struct ConvResLaunch {
  static int run(const ConvArgs& a, hipStream_t st) {
    using BD = Body<DevBA, GEO, DT>;
    constexpr int T = GEO::WGW * 64;
    int grid = ((a.H + 7) & ~7) * a.nchunk;
    if (a.R > 1) {
      if constexpr (GEO::N == 32768) {
        const bool half = 16 * GEO::Mi >= a.L;
        if (a.zsave) {
          if (half) return launch_res(conv_res_rp_kernel<GEO, DT, true, true>, "conv_res_rp_kernel (spectrum-saving)", grid, T, GEO::LDS_BYTES, GEO::LDS_BYTES, a, st);
          return launch_res(conv_res_rp_kernel<GEO, DT, false, true>, "conv_res_rp_kernel (spectrum-saving)", grid, T, GEO::LDS_BYTES, GEO::LDS_BYTES, a, st);
        }
        if (half) return launch_res(conv_res_rp_kernel<GEO, DT, true>, "conv_res_rp_kernel", grid, T, GEO::LDS_BYTES, GEO::LDS_BYTES, a, st);
        return launch_res(conv_res_rp_kernel<GEO, DT, false>, "conv_res_rp_kernel", grid, T, GEO::LDS_BYTES, GEO::LDS_BYTES, a, st);
      } else if constexpr (GEO::N == 1024) {
        constexpr int lds = GEO::LDS_BYTES + 2 * BD::IPASS_BYTES;
        const int cap = (a.persist > 0 && a.persist < (1 << 29)) ? 2 * a.persist : (1 << 30);
        const int g = grid > cap ? cap : grid, l = GEO::LDS_BYTES + a.R * BD::IPASS_BYTES;
        if (a.zsave || a.yraw) return launch_res(conv_res_rp_kernel<GEO, DT, false, true>, "conv_res_rp_kernel", g, T, lds, l, a, st);
        return launch_res(conv_res_rp_kernel<GEO, DT, false>, "conv_res_rp_kernel", g, T, lds, l, a, st);
      } else {
        return ffc_fail("multi-pass plan on a geometry without multi-pass kernels");
      }
    }
    if (GEO::OUTER && GEO::NW == 1 && grid > a.persist) grid = a.persist;
    if (!GEO::OUTER && a.persist > 0 && a.persist < (1 << 29) && grid > 2 * a.persist) grid = 2 * a.persist;
    const bool half = GEO::OUTER && (GEO::N1 / 2) * GEO::Mi >= a.L;
    if (a.zsave || (!GEO::OUTER && a.yraw)) {
      if (half) return launch_res(conv_res_kernel<GEO, DT, GEO::OUTER, true>, "conv_res_kernel (spectrum-saving)", grid, T, GEO::LDS_BYTES, GEO::LDS_BYTES, a, st);
      return launch_res(conv_res_kernel<GEO, DT, false, true>, "conv_res_kernel (spectrum-saving)", grid, T, GEO::LDS_BYTES, GEO::LDS_BYTES, a, st);
    }
    if (half) return launch_res(conv_res_kernel<GEO, DT, GEO::OUTER>, "conv_res_kernel", grid, T, GEO::LDS_BYTES, GEO::LDS_BYTES, a, st);
    return launch_res(conv_res_kernel<GEO, DT, false>, "conv_res_kernel", grid, T, GEO::LDS_BYTES, GEO::LDS_BYTES, a, st);
  }
};

int ffc_conv_res_launch(int N, int dtype, const ConvArgs& a, hipStream_t st) { return ffc_dispatch<ConvResLaunch>(N, dtype, a, st); }
