// History form of the gated forward / input-gradient kernel on blocked rows (Body::outer_jobs<.., OS, OSG = 2>, struct OsHist) +
// ffc_conv_fwd_os_hist.  conv_os_g_kernel's loop; the wrapped window of block 0 reads its history half from `hist`, and with `dhist` the
// natural-order launch runs a block -1 per row whose S outputs are the gradient of that history.  Gates stay nullable: a call with a
// state and no gate runs this kernel with null gates.
#include "ffc_dev.h"
using namespace ffc;

struct ConvOsHArgs {
  ConvArgs c;
  OsRows o;
  OsGate g;
  OsHist oh;
};

template <class GEO, int DT>
__global__ __launch_bounds__(GEO::WGW * 64, 2) void conv_os_h_kernel(ConvOsHArgs k) {
  using BD = Body<DevB, GEO, DT>;
  const ConvArgs& a = k.c;
  if constexpr (GEO::NW == 1) {
    // one wave per unit (fft 4096): persistent workgroups walk the (head, chunk) jobs
    BD::setup_tables(a.tab, a.t);
    const int total = ((a.H + 7) & ~7) * a.nchunk;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int h, chunk;
      if (map_id(id, a.H, a.nchunk, &h, &chunk)) BD::template conv_job<false, false, false, false, false, false, true, 2>(a, h, chunk, k.o, k.g, k.oh);
    }
  } else {
    int h, chunk;
    if (!map_block(a.H, a.nchunk, &h, &chunk)) return;
    BD::setup_tables(a.tab, a.t);
    BD::template conv_job<false, false, false, false, false, false, true, 2>(a, h, chunk, k.o, k.g, k.oh);
  }
}

template <class GEO, int DT>
struct ConvOsHLaunch {
  static int run(const ConvOsHArgs& k, hipStream_t st) {
    const OsRoute r = os_hist_route<GEO>(k.c, k.o, k.g, k.oh);
    if (r.err) return ffc_fail(r.err);
    if constexpr (GEO::OUTER) return ffc_launch(conv_os_h_kernel<GEO, DT>, "conv_os_h_kernel", r.grid, GEO::WGW * 64, r.lds_max, r.lds, st, k);
    else return ffc_fail(NO_OS_HIST);
  }
};

extern "C" int ffc_conv_fwd_os_hist(const ffc_plan* p, const void* u, const void* kf, const void* pregate, const void* postgate,
                                    const void* addend, void* y, const void* gate2, void* out2, const void* hist, void* dhist, int64_t B,
                                    int64_t H, int64_t L, int conj_kf, int wrap, void* stream) {
  if (!p || !u || !kf || !y) return ffc_fail("null arg");
  if (B <= 0 || H <= 0 || L <= 0) return ffc_fail("empty batch/heads/rows");
  if (p->hp.N1 <= 1 || p->hp.R > 1) return ffc_fail(NO_OS_HIST);
  if ((uintptr_t)kf & 15) return ffc_fail("k_f must be 16-byte aligned");
  if (const char* e = os_hist_limits(p->hp.N, B, H, L)) return ffc_fail(e);
  const void* const outs[] = {y, out2};
  const void* const ins[] = {u, pregate, postgate, addend, gate2};
  if (const char* e = os_hist_alias(outs, 2, ins, 5, B * H * L, hist, dhist, B * H * (p->hp.N / 2))) return ffc_fail(e);
  ConvOsHArgs k{};
  ConvArgs& a = k.c;
  a.u = u; a.y = y; a.kf = kf; a.pregate = pregate; a.postgate = postgate; a.tab = p->d_blob; a.t = p->hp.tabs;
  set_os_rows(&a, &k.o, p->hp.N, B, H, L, wrap ? 1 : 0);
  set_os_gate(&a, &k.g, addend, gate2, out2, H, L);
  set_os_hist(&a, &k.o, &k.oh, hist, dhist, B, H);
  a.conj_kf = conj_kf;
  a.s_inv = (float)p->hp.s_inv; a.s_fwd = (float)p->hp.s_fwd;
  a.flags = p->env_flags;
  const void* const all[] = {u, pregate, postgate, addend, gate2, y, out2};
  a.fast = os_fast(L, all, 7);
  ffc_choose_chunks(p, a.H, a.npair, &a.nchunk, &a.ppc, a.npair <= OS_CHUNK_SEARCH);
  a.persist = ffc_persist(p);
  a.R = 1;
  a.stream = 0;      // sample rows are read twice (block and history), as in ffc_conv_fwd_os: plain accesses
  return ffc_dispatch<ConvOsHLaunch>(p->hp.N, p->hp.dtype, k, (hipStream_t)stream);
}
