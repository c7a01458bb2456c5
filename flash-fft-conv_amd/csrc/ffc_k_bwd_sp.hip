// Frequency-sparse fused backward (Modes::bwd_sp) and the dk_f -> dk kernel on its live-row slabs (Modes::dkifft_sp):
// ffc_conv_bwd_sparse / ffc_kernel_ifft_grad_sp.  A translation unit of its own: the dense backward kernels (ffc_k_bwd.hip,
// ffc_k_bwdz.hip) keep their code and their 128 + 128 register split; this kernel addresses no accumulation register and has the
// whole 256-register file of a wave for two tiles in lock-step (build.py check_agpr: no accumulation register at all).
#include "ffc_dev.h"
using namespace ffc;

template <class GEO, int DT, bool HALF>
__global__ __launch_bounds__(GEO::WGW * 64, 2) void bwd_sp_kernel(DkfArgs d) {
  int h, chunk;
  if (!map_block(d.c.H, d.c.nchunk, &h, &chunk)) return;
  Modes<DevBO, GEO, DT>::template bwd_sp<HALF>(d, h, chunk);
}
template <class GEO, int DT>
__global__ __launch_bounds__(GEO::WGW * 64, 2) void dkifft_sp_kernel(DkSpArgs a) {
  Modes<DevB, GEO, DT>::dkifft_sp(a, blockIdx.x);
}

template <class GEO, int DT>
struct BwdSpLaunch {
  static int run(const DkfArgs& d, int rows, hipStream_t st) {
    const BwdSpRoute r = bwd_sp_route<GEO>(d, rows);
    if (r.err) return ffc_fail(r.err);
    if constexpr (GEO::HAS_SP) {
      return pick([&](auto half) -> int {
        return ffc_launch(bwd_sp_kernel<GEO, DT, decltype(half)::value>, "bwd_sp_kernel", r.grid, GEO::WGW * 64, r.lds_max, r.lds, st, d);
      }, r.half);
    } else {
      return ffc_fail(NO_SPARSE_BWD);
    }
  }
};
template <class GEO, int DT>
struct DkSpLaunch {
  static int run(const DkSpArgs& a, hipStream_t st) {
    if constexpr (GEO::HAS_SP)
      return ffc_launch(dkifft_sp_kernel<GEO, DT>, "dkifft_sp_kernel", dk_sp_grid<GEO>(a.H), GEO::WGW * 64, GEO::LDS_BYTES, GEO::LDS_BYTES, st, a);
    else
      return ffc_fail(NO_SPARSE_BWD);
  }
};

// The fused backward of ffc_conv_bwd_gated for a k_f whose non-zero bins all lie in the spectrum rows k3 < rows or k3 >= 32 - rows
// (the k_f that ffc_conv_fwd_sparse takes): du, dpre / dpost (nullable) and the LIVE rows of the fp32 dk_f slabs in `ws` (the layout of
// ffc_conv_bwd_gated; the other rows are left as they were: finish with ffc_kernel_ifft_grad_sp).  Recomputing form only: `zin` must be
// null.  fft 16384 / 32768, 1 <= rows <= 4; anything else is refused before a launch.
extern "C" int ffc_conv_bwd_sparse(const ffc_plan* p, const void* dout, const void* u, const void* kf, const void* pregate, const void* postgate,
                                   void* du, void* dpre, void* dpost, void* ws, const void* zin, int64_t B, int64_t H, int64_t L, int rows,
                                   void* stream) {
  if (!p || !dout || !u || !kf || !du || !ws) return ffc_fail("null arg");
  if (zin || rows < 1 || rows > 4 || p->hp.R > 1 || p->hp.N1 <= 1 || p->hp.N2 != 32 || p->hp.N3 != 32) return ffc_fail(NO_SPARSE_BWD);
  if (B <= 0 || H <= 0) return ffc_fail("empty batch/heads");
  if (L <= 0 || L > p->hp.N) return ffc_fail("L must be in (0, fft_size]");
  if (((uintptr_t)kf | (uintptr_t)ws) & 15) return ffc_fail("k_f and ws must be 16-byte aligned");
  if ((B - 1) * H * L + H * L >= ((int64_t)1 << 31)) return ffc_fail("tensor too large (>= 2^31 elements)");
  DkfArgs d{};
  ConvArgs& a = d.c;
  a.u = u; a.kf = kf; a.pregate = pregate; a.postgate = postgate; a.tab = p->d_blob; a.t = p->hp.tabs;
  a.B = (int)B; a.H = (int)H; a.L = (int)L; a.npair = (int)((B + 1) / 2); a.s_inv = (float)p->hp.s_inv; a.s_fwd = (float)p->hp.s_fwd;
  a.sbu = a.sbg = a.sbp = a.sby = H * L;
  d.sbd = d.sbdu = d.sbdpre = d.sbdpost = H * L;
  a.fast = (L % 8 == 0) && !(((uintptr_t)u | (uintptr_t)dout | (uintptr_t)pregate | (uintptr_t)postgate | (uintptr_t)du | (uintptr_t)dpre |
                              (uintptr_t)dpost) & 15);
  ffc_choose_chunks(p, a.H, a.npair, &a.nchunk, &a.ppc);
  a.persist = ffc_persist(p);
  a.R = 1;
  a.stream = p->env_stream >= 0 ? p->env_stream : ((!pregate && !postgate) ? 1 : 0);
  a.flags = p->env_flags;
  a.sparse = rows;
  d.dout = dout; d.ws = (float*)ws; d.du = du; d.dpre = dpre; d.dpost = dpost;
  return ffc_dispatch<BwdSpLaunch>(p->hp.N, p->hp.dtype, d, rows, (hipStream_t)stream);
}

// dk (H, Lk) fp32 from the slabs of ffc_conv_bwd_sparse (same B, H): only the live rows are read, every other bin counts as zero, and
// `mask` (kf_elems fp32 0/1, k_f's internal order: the mask the module multiplied into k_f) selects the kept bins of the live rows.
extern "C" int ffc_kernel_ifft_grad_sp(const ffc_plan* p, const void* ws, const float* mask, int rows, int64_t B, int64_t H, int64_t Lk, float* dk,
                                       void* stream) {
  if (!p || !ws || !mask || !dk) return ffc_fail("null arg");
  if (rows < 1 || rows > 4 || p->hp.R > 1 || p->hp.N1 <= 1 || p->hp.N2 != 32 || p->hp.N3 != 32) return ffc_fail(NO_SPARSE_BWD);
  if (H <= 0 || B <= 0 || Lk <= 0 || Lk > p->hp.N) return ffc_fail("dk must be (H, Lk) with 0 < Lk <= fft_size");
  if (((uintptr_t)ws | (uintptr_t)mask) & 15) return ffc_fail("ws and mask must be 16-byte aligned");
  int nchunk, ppc;
  ffc_choose_chunks(p, (int)H, (int)((B + 1) / 2), &nchunk, &ppc);
  DkSpArgs a{};
  // always bf16 arithmetic, as ffc_kernel_ifft_grad
  a.ws = (const float*)ws; a.dk = dk; a.tab = p->d_blob_bf; a.t = p->hp_bf.tabs; a.H = (int)H; a.Lk = (int)Lk;
  a.nslab = nchunk;
  a.scale = (float)(1.0 / p->hp.s_fwd); a.s_inv = (float)p->hp_bf.s_inv;
  a.fast = (Lk % 4 == 0) && !((uintptr_t)dk & 15);
  a.flags = p->env_flags;
  a.R = 1;
  a.mask = mask;
  return ffc_dispatch<DkSpLaunch>(p->hp.N, DT_BF16, a, (hipStream_t)stream);
}
