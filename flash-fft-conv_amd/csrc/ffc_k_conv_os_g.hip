// Gated forward / input-gradient kernel on blocked rows (Body::outer_jobs<.., OS, OSG>, struct OsGate) + ffc_conv_fwd_os_gated.
// conv_os_kernel's loop with the gated row copies: window of u * pregate in, y = raw * postgate + addend and out2 = raw * gate2 out.
#include "ffc_dev.h"
using namespace ffc;

struct ConvOsGArgs {
  ConvArgs c;
  OsRows o;
  OsGate g;
};

template <class GEO, int DT>
__global__ __launch_bounds__(GEO::WGW * 64, 2) void conv_os_g_kernel(ConvOsGArgs k) {
  using BD = Body<DevB, GEO, DT>;
  const ConvArgs& a = k.c;
  if constexpr (GEO::NW == 1) {
    // one wave per unit (fft 4096): persistent workgroups walk the (head, chunk) jobs
    BD::setup_tables(a.tab, a.t);
    const int total = ((a.H + 7) & ~7) * a.nchunk;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int h, chunk;
      if (map_id(id, a.H, a.nchunk, &h, &chunk)) BD::template conv_job<false, false, false, false, false, false, true, true>(a, h, chunk, k.o, k.g);
    }
  } else {
    int h, chunk;
    if (!map_block(a.H, a.nchunk, &h, &chunk)) return;
    BD::setup_tables(a.tab, a.t);
    BD::template conv_job<false, false, false, false, false, false, true, true>(a, h, chunk, k.o, k.g);
  }
}

template <class GEO, int DT>
struct ConvOsGLaunch {
  static int run(const ConvOsGArgs& k, hipStream_t st) {
    const OsRoute r = os_gated_route<GEO>(k.c, k.o, k.g);
    if (r.err) return ffc_fail(r.err);
    if constexpr (GEO::OUTER) return ffc_launch(conv_os_g_kernel<GEO, DT>, "conv_os_g_kernel", r.grid, GEO::WGW * 64, r.lds_max, r.lds, st, k);
    else return ffc_fail(NO_OS_GATED);
  }
};

extern "C" int ffc_conv_fwd_os_gated(const ffc_plan* p, const void* u, const void* kf, const void* pregate, const void* postgate,
                                     const void* addend, void* y, const void* gate2, void* out2, int64_t B, int64_t H, int64_t L,
                                     int conj_kf, int wrap, void* stream) {
  if (!p || !u || !kf || !y) return ffc_fail("null arg");
  if (B <= 0 || H <= 0 || L <= 0) return ffc_fail("empty batch/heads/rows");
  if (p->hp.N1 <= 1 || p->hp.R > 1) return ffc_fail(NO_OS_GATED);
  if ((uintptr_t)kf & 15) return ffc_fail("k_f must be 16-byte aligned");
  if (const char* e = os_limits(p->hp.N, B, H, L)) return ffc_fail(e);
  const void* const outs[] = {y, out2};
  const void* const ins[] = {u, pregate, postgate, addend, gate2};
  if (const char* e = os_alias(outs, 2, ins, 5, B * H * L)) return ffc_fail(e);
  ConvOsGArgs k{};
  ConvArgs& a = k.c;
  a.u = u; a.y = y; a.kf = kf; a.pregate = pregate; a.postgate = postgate; a.tab = p->d_blob; a.t = p->hp.tabs;
  set_os_rows(&a, &k.o, p->hp.N, B, H, L, wrap ? 1 : 0);
  set_os_gate(&a, &k.g, addend, gate2, out2, H, L);
  a.conj_kf = conj_kf;
  a.s_inv = (float)p->hp.s_inv; a.s_fwd = (float)p->hp.s_fwd;
  a.flags = p->env_flags;
  const void* const all[] = {u, pregate, postgate, addend, gate2, y, out2};
  a.fast = os_fast(L, all, 7);
  ffc_choose_chunks(p, a.H, a.npair, &a.nchunk, &a.ppc, a.npair <= OS_CHUNK_SEARCH);
  a.persist = ffc_persist(p);
  a.R = 1;
  a.stream = 0;      // sample rows are read twice (block and history), as in ffc_conv_fwd_os: plain accesses
  return ffc_dispatch<ConvOsGLaunch>(p->hp.N, p->hp.dtype, k, (hipStream_t)stream);
}
