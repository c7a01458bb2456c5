// Forward / input-gradient kernel on blocked rows (overlap-save form: Body::outer_jobs<.., OS>, struct OsRows) + ffc_conv_fwd_os.
#include "ffc_dev.h"
using namespace ffc;

struct ConvOsArgs {
  ConvArgs c;
  OsRows o;
};

// conv_kernel's three shapes for the sizes with an outer digit, on the OS form of the pair loop
template <class GEO, int DT>
__global__ __launch_bounds__(GEO::WGW * 64, 2) void conv_os_kernel(ConvOsArgs k) {
  using BD = Body<DevB, GEO, DT>;
  const ConvArgs& a = k.c;
  if constexpr (GEO::NW == 1) {
    // one wave per unit (fft 4096): persistent workgroups walk the (head, chunk) jobs
    BD::setup_tables(a.tab, a.t);
    const int total = ((a.H + 7) & ~7) * a.nchunk;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int h, chunk;
      if (map_id(id, a.H, a.nchunk, &h, &chunk)) BD::template conv_job<false, false, false, false, false, false, true>(a, h, chunk, k.o);
    }
  } else {
    int h, chunk;
    if (!map_block(a.H, a.nchunk, &h, &chunk)) return;
    BD::setup_tables(a.tab, a.t);
    BD::template conv_job<false, false, false, false, false, false, true>(a, h, chunk, k.o);
  }
}

template <class GEO, int DT>
struct ConvOsLaunch {
  static int run(const ConvOsArgs& k, hipStream_t st) {
    const OsRoute r = os_route<GEO>(k.c, k.o);
    if (r.err) return ffc_fail(r.err);
    if constexpr (GEO::OUTER) return ffc_launch(conv_os_kernel<GEO, DT>, "conv_os_kernel", r.grid, GEO::WGW * 64, r.lds_max, r.lds, st, k);
    else return ffc_fail(NO_OS);
  }
};

extern "C" int ffc_conv_fwd_os(const ffc_plan* p, const void* u, const void* kf, void* y, int64_t B, int64_t H, int64_t L, int conj_kf,
                               int wrap, void* stream) {
  if (!p || !u || !kf || !y) return ffc_fail("null arg");
  if (B <= 0 || H <= 0 || L <= 0) return ffc_fail("empty batch/heads/rows");
  if (p->hp.N1 <= 1 || p->hp.R > 1) return ffc_fail(NO_OS);
  if ((uintptr_t)kf & 15) return ffc_fail("k_f must be 16-byte aligned");
  if (const char* e = os_limits(p->hp.N, B, H, L)) return ffc_fail(e);
  ConvOsArgs k{};
  ConvArgs& a = k.c;
  a.u = u; a.y = y; a.kf = kf; a.tab = p->d_blob; a.t = p->hp.tabs;
  set_os_rows(&a, &k.o, p->hp.N, B, H, L, wrap ? 1 : 0);
  a.conj_kf = conj_kf;
  a.s_inv = (float)p->hp.s_inv; a.s_fwd = (float)p->hp.s_fwd;
  a.flags = p->env_flags;
  a.fast = (L % 8 == 0) && !(((uintptr_t)u | (uintptr_t)y) & 15);
  // (the forward rule searches every chunk length, one step per pair: above OS_CHUNK_SEARCH pairs, where its choices tie anyway, the closed form)
  ffc_choose_chunks(p, a.H, a.npair, &a.nchunk, &a.ppc, a.npair <= OS_CHUNK_SEARCH);
  a.persist = ffc_persist(p);
  a.R = 1;
  a.stream = 0;      // a block is read twice, as itself and as the next block's history: plain accesses keep it in L2
  return ffc_dispatch<ConvOsLaunch>(p->hp.N, p->hp.dtype, k, (hipStream_t)stream);
}
