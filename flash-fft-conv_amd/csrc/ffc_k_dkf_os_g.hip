// Gated dk_f accumulation kernel on blocked rows (Modes::dkf_os<true>) + ffc_conv_bwd_dkf_os_gated: the wrapped window of u * pregate,
// the S-sample window of dout * postgate.
#include "ffc_dev.h"
using namespace ffc;

struct DkfOsGArgs {
  DkfArgs d;
  OsRows o;
};

// the dk_f partial sums live in a0..a127 (Modes::WAcc), as in dkf_os_kernel
template <class GEO, int DT>
__global__ __launch_bounds__(GEO::WGW * 64, 2) __attribute__((amdgpu_num_vgpr(128))) void dkf_os_g_kernel(DkfOsGArgs k) {
  const ConvArgs& a = k.d.c;
  if constexpr (GEO::NW == 1) {
    const int total = ((a.H + 7) & ~7) * a.nchunk;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int h, chunk;
      if (map_id(id, a.H, a.nchunk, &h, &chunk)) Modes<DevBO, GEO, DT>::template dkf_os<true>(k.d, k.o, h, chunk, blockIdx.x);
    }
  } else {
    int h, chunk;
    if (!map_block(a.H, a.nchunk, &h, &chunk)) return;
    Modes<DevBO, GEO, DT>::template dkf_os<true>(k.d, k.o, h, chunk, blockIdx.x);
  }
}

template <class GEO, int DT>
struct DkfOsGLaunch {
  static int run(const DkfOsGArgs& k, hipStream_t st) {
    const OsRoute r = os_gated_route<GEO>(k.d.c, k.o, OsGate());
    if (r.err) return ffc_fail(r.err);
    if constexpr (GEO::OUTER) return ffc_launch(dkf_os_g_kernel<GEO, DT>, "dkf_os_g_kernel", r.grid, GEO::WGW * 64, r.lds_max, r.lds, st, k);
    else return ffc_fail(NO_OS_GATED);
  }
};

// ws and the finishing call as ffc_conv_bwd_dkf_os
extern "C" int ffc_conv_bwd_dkf_os_gated(const ffc_plan* p, const void* dout, const void* u, const void* pregate, const void* postgate,
                                         void* ws, int64_t B, int64_t H, int64_t L, void* stream) {
  if (!p || !dout || !u || !ws) return ffc_fail("null arg");
  if (B <= 0 || H <= 0 || L <= 0) return ffc_fail("empty batch/heads/rows");
  if (p->hp.N1 <= 1 || p->hp.R > 1) return ffc_fail(NO_OS_GATED);
  if (const char* e = os_limits(p->hp.N, B, H, L)) return ffc_fail(e);
  DkfOsGArgs k{};
  DkfArgs& d = k.d;
  ConvArgs& a = d.c;
  a.u = u; a.pregate = pregate; a.postgate = postgate; a.tab = p->d_blob; a.t = p->hp.tabs;
  set_os_rows(&a, &k.o, p->hp.N, B, H, L, 1);
  d.sbd = d.sbdu = d.sbdpre = d.sbdpost = H * L;
  a.s_fwd = (float)p->hp.s_fwd;
  const void* const all[] = {u, dout, pregate, postgate};
  a.fast = os_fast(L, all, 4);
  ffc_choose_chunks(p, a.H, a.npair, &a.nchunk, &a.ppc);
  a.persist = ffc_persist(p);
  a.R = 1;
  a.stream = 0;
  a.flags = p->env_flags;
  d.dout = dout; d.ws = (float*)ws; d.zscratch = ffc_zscratch(p, ws, a.H, a.nchunk);
  return ffc_dispatch<DkfOsGLaunch>(p->hp.N, p->hp.dtype, k, (hipStream_t)stream);
}
