// History form of the gated dk_f accumulation kernel on blocked rows (Modes::dkf_os<2>, struct OsHist) + ffc_conv_bwd_dkf_os_hist: the
// wrapped window of u * pregate takes block 0's history half from `hist`; the S-sample window of dout * postgate is dkf_os_g_kernel's.
#include "ffc_dev.h"
using namespace ffc;

struct DkfOsHArgs {
  DkfArgs d;
  OsRows o;
  OsHist oh;
};

// the dk_f partial sums live in a0..a127 (Modes::WAcc), as in dkf_os_kernel
template <class GEO, int DT>
__global__ __launch_bounds__(GEO::WGW * 64, 2) __attribute__((amdgpu_num_vgpr(128))) void dkf_os_h_kernel(DkfOsHArgs k) {
  const ConvArgs& a = k.d.c;
  if constexpr (GEO::NW == 1) {
    const int total = ((a.H + 7) & ~7) * a.nchunk;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int h, chunk;
      if (map_id(id, a.H, a.nchunk, &h, &chunk)) Modes<DevBO, GEO, DT>::template dkf_os<2>(k.d, k.o, h, chunk, blockIdx.x, k.oh);
    }
  } else {
    int h, chunk;
    if (!map_block(a.H, a.nchunk, &h, &chunk)) return;
    Modes<DevBO, GEO, DT>::template dkf_os<2>(k.d, k.o, h, chunk, blockIdx.x, k.oh);
  }
}

template <class GEO, int DT>
struct DkfOsHLaunch {
  static int run(const DkfOsHArgs& k, hipStream_t st) {
    const OsRoute r = os_hist_route<GEO>(k.d.c, k.o, OsGate(), k.oh);
    if (r.err) return ffc_fail(r.err);
    if constexpr (GEO::OUTER) return ffc_launch(dkf_os_h_kernel<GEO, DT>, "dkf_os_h_kernel", r.grid, GEO::WGW * 64, r.lds_max, r.lds, st, k);
    else return ffc_fail(NO_OS_HIST);
  }
};

// ws and the finishing call as ffc_conv_bwd_dkf_os
extern "C" int ffc_conv_bwd_dkf_os_hist(const ffc_plan* p, const void* dout, const void* u, const void* pregate, const void* postgate,
                                        const void* hist, void* ws, int64_t B, int64_t H, int64_t L, void* stream) {
  if (!p || !dout || !u || !ws) return ffc_fail("null arg");
  if (B <= 0 || H <= 0 || L <= 0) return ffc_fail("empty batch/heads/rows");
  if (p->hp.N1 <= 1 || p->hp.R > 1) return ffc_fail(NO_OS_HIST);
  if (const char* e = os_hist_limits(p->hp.N, B, H, L)) return ffc_fail(e);
  DkfOsHArgs k{};
  DkfArgs& d = k.d;
  ConvArgs& a = d.c;
  a.u = u; a.pregate = pregate; a.postgate = postgate; a.tab = p->d_blob; a.t = p->hp.tabs;
  set_os_rows(&a, &k.o, p->hp.N, B, H, L, 1);
  set_os_hist(&a, &k.o, &k.oh, hist, nullptr, B, H);
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
  return ffc_dispatch<DkfOsHLaunch>(p->hp.N, p->hp.dtype, k, (hipStream_t)stream);
}
