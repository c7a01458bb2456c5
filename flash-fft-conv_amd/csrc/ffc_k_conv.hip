// FlashFFTConv forward / input-gradient kernel (see ffc_body.h) + ffc_conv_fwd.
#include "ffc_conv_launch.h"
using namespace ffc;

static constexpr int SMALL_WAVES = 2;     // waves per SIMD the single-tile kernels (no outer digit) are compiled for
// SZ: the forward that also stores the pairs' spectra for the backward pass (ConvArgs::zsave; fused sizes with an outer digit)
// GS: phase C stores the output rows itself (Body::outer_inv_half<true>; fft 32768 at L <= N/2, plain rows: ffc::direct_store_ok)
// PL: a GS kernel whose input rows are plain at compile time as well (Body::rows_load_pl; ffc::plain_rows_ok)
template <class GEO, int DT, bool HALF, bool SZ = false, bool SP = false, bool GS = false, bool PL = false>
__global__ __launch_bounds__(GEO::WGW * 64, GEO::OUTER ? 2 : SMALL_WAVES) void conv_kernel(ConvArgs a) {
  using BD = Body<DevB, GEO, DT>;
  if constexpr (GEO::OUTER && GEO::NW == 1) {
    // One wave per unit (fft 4096): persistent workgroups, one per CU, walk the (head, chunk) jobs with a stride of
    // the grid (a multiple of 8, so a workgroup's heads stay on its XCD).  No phase of these units needs a
    // workgroup barrier (Body::unit_barrier), so the eight waves drift apart across jobs: one wave's row loads and
    // stores overlap another's transforms, and the plan tables are copied to LDS once per CU instead of once per head.
    BD::setup_tables(a.tab, a.t);
    const int total = ((a.H + 7) & ~7) * a.nchunk;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int h, chunk;
      if (map_id(id, a.H, a.nchunk, &h, &chunk)) BD::template conv_job<HALF, false, SZ>(a, h, chunk);
    }
  } else if constexpr (!GEO::OUTER) {
    // single-tile sizes (fft <= 1024): persistent workgroups too (two per CU): a job is one tile per wave, copying the plan
    // tables to LDS for every job cost as much as the job
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
    if constexpr (GEO::NW > 1 && !SP) {
      // k -> k_f of this head first (ConvArgs::kfuse_k, one chunk per head): no separate launch for it
      BD::setup_tables(a.tab, a.t);
      if (a.kfuse_k || a.kfuse_x) Modes<DevB, GEO, DT>::kfft_head(a, h);
      BD::template conv_job<HALF, false, SZ, SP, GS, PL>(a, h, chunk);
    } else {
      BD::template conv<HALF, SZ, SP, GS, PL>(a, h, chunk);
    }
  }
}

// multi-pass sizes (fft 65536 / 131072): the R passes of a (head, chunk) job run one after the other in the same workgroup,
// so that the read-modify-write of the output rows stays inside one wave (struct Pass, Body::rows_out_rp)
template <class GEO, int DT, bool HALF, bool SZ = false>
__global__ __launch_bounds__(GEO::WGW * 64, 2) void conv_rp_kernel(ConvArgs a) {
  using BD = Body<DevB, GEO, DT>;
  if constexpr (!GEO::OUTER) {
    // inner-only form (fft 2048): persistent workgroups, tables (incl. the per-pass ones) copied once
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
struct ConvKernels {
  static constexpr bool HAS_ADD = false;
  template <class GEO, int DT, bool MP, bool HALF, bool SZ, bool SP>
  static constexpr auto kernel() {
    if constexpr (MP) return conv_rp_kernel<GEO, DT, HALF, SZ>;
    else return conv_kernel<GEO, DT, HALF, SZ, SP>;
  }
  template <class GEO, int DT, bool SZ, bool PL>
  static constexpr auto kernel_gs() { return conv_kernel<GEO, DT, true, SZ, false, true, PL>; }
  static const char* what(bool mp, bool sz, bool sp, bool outer) {
    if (mp) return sz && outer ? "conv_rp_kernel (spectrum-saving)" : "conv_rp_kernel";
    if (sz) return outer ? "conv_kernel (spectrum-saving)" : "conv_kernel (spectrum-saving, single tile)";
    return sp ? "conv_kernel (frequency-sparse)" : "conv_kernel";
  }
};
// The HALF form of the single-tile sizes is never launched (there is no outer digit to halve).  The launcher once instantiated it by
// accident; the instantiations stay so that the library's kernel set is what it was.
template __global__ void conv_kernel<Geo<1, 16, 16>, DT_BF16, true>(ConvArgs);
template __global__ void conv_kernel<Geo<1, 16, 16>, DT_F16, true>(ConvArgs);
template __global__ void conv_kernel<Geo<1, 16, 32>, DT_BF16, true>(ConvArgs);
template __global__ void conv_kernel<Geo<1, 16, 32>, DT_F16, true>(ConvArgs);
template __global__ void conv_kernel<Geo<1, 32, 32>, DT_BF16, true>(ConvArgs);
template __global__ void conv_kernel<Geo<1, 32, 32>, DT_F16, true>(ConvArgs);

// stride 0 = contiguous (H * L)
static inline bool ffc_stride_ok(int64_t* sb, int64_t B, int64_t H, int64_t L) {
  if (*sb == 0) *sb = H * L;
  return *sb >= H * L && (B - 1) * *sb + H * L < ((int64_t)1 << 31);
}

// spectra saved for the backward pass: [H][npair][N] complex values of the plan dtype (single-tile sizes: see below)
extern "C" int64_t ffc_spectrum_bytes(const ffc_plan* p, int64_t B, int64_t H) {
  if (!p || B <= 0 || H <= 0) return 0;
  if (p->hp.N1 <= 1) {      // single-tile sizes (fft <= 2048): [H][tiles of G pairs][R passes] slots of 1024 complex values
    const int64_t G = (32 / p->hp.N2) * (32 / p->hp.N3);
    return H * (((B + 1) / 2 + G - 1) / G) * p->hp.R * 4096;
  }
  return ((B + 1) / 2) * H * (int64_t)p->hp.N * 4;        // (hp.N = the plan's fft size, R passes x the kernel size)
}

// One forward call, as the entry points below fill it (everything they do not name is zero / null).
struct FwdCall {
  const void *u, *kf, *pregate, *postgate;
  void* y;
  int64_t B, H, L;
  void* stream;
  int conj_kf;
  int64_t sb_u, sb_pre, sb_post, sb_y;      // batch strides in elements, 0 = contiguous (H * L)
  void *zsave, *yraw;                       // spectra / output before the postgate, for the backward pass
  int sparse;                               // > 0: frequency-sparse k_f (ffc_conv_fwd_sparse)
  const void* addend; int64_t sb_add;       // ffc_conv_fwd_res
  // k -> k_f inside the launch, from real k (H, kfuse_Lk) fp32 or from complex rows kfuse_x with the caller's scale: given only when
  // kfft_in_launch() said so
  const float* kfuse_k; int64_t kfuse_Lk;
  const void* kfuse_x; float kfuse_xscale;
};
static FwdCall fwd_call(const void* u, const void* kf, const void* pregate, const void* postgate, void* y, int64_t B, int64_t H, int64_t L,
                        void* stream) {
  FwdCall c{};
  c.u = u; c.kf = kf; c.pregate = pregate; c.postgate = postgate; c.y = y; c.B = B; c.H = H; c.L = L; c.stream = stream;
  return c;
}
// whether the convolution launch of (B, H) takes the k -> k_f step (ffc::fwd_takes_kfft on the chunking the launch will use)
static bool kfft_in_launch(const ffc_plan* p, int64_t B, int64_t H) {
  int nchunk = 0, ppc = 0;
  if (B > 0 && H > 0) ffc_choose_chunks(p, (int)H, (int)((B + 1) / 2), &nchunk, &ppc, true);
  return fwd_takes_kfft(p->hp, nchunk, 0, p->env_flags);
}

static int conv_fwd_impl(const ffc_plan* p, const FwdCall& c) {
  const void *u = c.u, *kf = c.kf, *pregate = c.pregate, *postgate = c.postgate, *addend = c.addend;
  void *y = c.y, *zsave = c.zsave;
  const int64_t B = c.B, H = c.H, L = c.L;
  const int sparse = c.sparse;
  int64_t sb_u = c.sb_u, sb_pre = c.sb_pre, sb_post = c.sb_post, sb_y = c.sb_y, sb_add = c.sb_add;
  if (!p || !u || !kf || !y) return ffc_fail("null arg");
  if (B <= 0 || H <= 0) return ffc_fail("empty batch/heads");
  if (L <= 0 || L > p->hp.N) return ffc_fail("L must be in (0, fft_size]");
  if ((uintptr_t)kf & 15) return ffc_fail("k_f must be 16-byte aligned");
  if (!ffc_stride_ok(&sb_u, B, H, L) || !ffc_stride_ok(&sb_pre, B, H, L) || !ffc_stride_ok(&sb_post, B, H, L) ||
      !ffc_stride_ok(&sb_y, B, H, L) || !ffc_stride_ok(&sb_add, B, H, L))
    return ffc_fail("tensor too large (>= 2^31 elements) or batch stride smaller than H*L");
  ConvArgs a{};
  a.u = u; a.pregate = pregate; a.postgate = postgate; a.y = y; a.kf = kf;
  a.tab = p->d_blob; a.t = p->hp.tabs;
  a.B = (int)B; a.H = (int)H; a.L = (int)L; a.npair = (int)((B + 1) / 2);
  a.sbu = sb_u; a.sbg = sb_pre; a.sbp = sb_post; a.sby = sb_y;
  a.addend = addend; a.sba = sb_add;
  a.conj_kf = c.conj_kf;
  // y_raw without the spectra: the single-tile sizes (fft <= 2048) only -- their backward transforms u * pregate again from rows it
  // loads anyway (dpregate, du) and takes dpostgate = dout * y_raw from its dout row load (round 6)
  a.zsave = zsave; a.yraw = (zsave || p->hp.N1 <= 1) ? c.yraw : nullptr;
  a.sparse = sparse;
  if (sparse && (sparse < 0 || sparse > 4 || zsave || p->hp.R > 1 || p->hp.N2 != 32 || p->hp.N3 != 32 || p->hp.N1 <= 1))
    return ffc_fail("frequency-sparse forward: fft 16384 / 32768, 1 <= rows <= 4, no spectrum buffer");
  if (zsave && (ffc_spectrum_bytes(p, B, H) == 0 || ((uintptr_t)zsave & 15))) return ffc_fail("spectrum buffer: unsupported plan or misaligned");
  a.s_inv = (float)p->hp.s_inv; a.s_fwd = (float)p->hp.s_fwd;
  a.flags = p->env_flags;
  a.fast = (L % 8 == 0) && !(((uintptr_t)u | (uintptr_t)y | (uintptr_t)pregate | (uintptr_t)postgate | (uintptr_t)addend) & 15) &&
           !((sb_u | sb_pre | sb_post | sb_y | sb_add) & 7);
  ffc_choose_chunks(p, a.H, a.npair, &a.nchunk, &a.ppc, true);
  a.persist = ffc_persist(p);
  a.R = p->hp.R;
  // k -> k_f inside this launch (Modes::kfft_head), where the caller found that it may be (kfft_in_launch)
  if (c.kfuse_k) {
    a.kfuse_k = c.kfuse_k; a.kfuse_Lk = (int)c.kfuse_Lk;
    a.kfuse_scale = (float)(p->hp.s_k / p->hp.s_fwd) / (p->hp.dtype == DT_F16 ? 256.f : 1.f);
    a.kfuse_fast = (c.kfuse_Lk % 4 == 0) && !((uintptr_t)c.kfuse_k & 15);
  }
  // ... from complex rows (ffc_conv_fwd_kx: the inner k_f rows of the HBM-level sizes, the caller's scale)
  if (c.kfuse_x) { a.kfuse_x = c.kfuse_x; a.kfuse_scale = c.kfuse_xscale; a.kfuse_Lk = p->hp.N; a.kfuse_fast = 1; }
  // every row is read / written exactly once per launch (multi-pass sizes re-read the rows in every pass: plain accesses)
  a.stream = p->env_stream >= 0 ? p->env_stream : (p->hp.R > 1 ? 0 : 1);
  if (addend) return ffc_conv_res_launch(p->hp.N, p->hp.dtype, a, (hipStream_t)c.stream);      // kernels of their own (ffc_k_conv_res.hip)
  return ffc_dispatch<ConvLaunch<ConvKernels>::T>(p->hp.N, p->hp.dtype, a, (hipStream_t)c.stream);
}

extern "C" int ffc_conv_fwd_strided(const ffc_plan* p, const void* u, const void* kf, const void* pregate, const void* postgate,
                                    void* y, int64_t B, int64_t H, int64_t L, int conj_kf, int64_t sb_u, int64_t sb_pre,
                                    int64_t sb_post, int64_t sb_y, void* stream) {
  FwdCall c = fwd_call(u, kf, pregate, postgate, y, B, H, L, stream);
  c.conj_kf = conj_kf; c.sb_u = sb_u; c.sb_pre = sb_pre; c.sb_post = sb_post; c.sb_y = sb_y;
  return conv_fwd_impl(p, c);
}
// forward that also stores every pair's spectrum FFT(u * pregate) in `zsave` (ffc_spectrum_bytes) for ffc_conv_bwd_z and,
// when y_raw is given (16-byte aligned, contiguous (B,H,L)), the output before the postgate multiply
extern "C" int ffc_conv_fwd_z(const ffc_plan* p, const void* u, const void* kf, const void* pregate, const void* postgate, void* y,
                              void* zsave, void* y_raw, int64_t B, int64_t H, int64_t L, int64_t sb_u, int64_t sb_pre, int64_t sb_post,
                              int64_t sb_y, void* stream) {
  if (!zsave && !(y_raw && p && p->hp.N1 <= 1)) return ffc_fail("null spectrum buffer (y_raw alone: single-tile sizes, fft <= 2048)");
  if (y_raw && ((uintptr_t)y_raw & 15)) return ffc_fail("y_raw must be 16-byte aligned");
  FwdCall c = fwd_call(u, kf, pregate, postgate, y, B, H, L, stream);
  c.zsave = zsave; c.yraw = y_raw; c.sb_u = sb_u; c.sb_pre = sb_pre; c.sb_post = sb_post; c.sb_y = sb_y;
  return conv_fwd_impl(p, c);
}

// y = postgate * conv(u * pregate, k) + addend: the superset of ffc_conv_fwd_strided and ffc_conv_fwd_z (zsave / y_raw nullable, y_raw
// stays the output before gate and addend).  The multi-pass sizes read-modify-write y between their passes, so an addend that overlaps y
// is refused at every size.
extern "C" int ffc_conv_fwd_res(const ffc_plan* p, const void* u, const void* kf, const void* pregate, const void* postgate,
                                const void* addend, void* y, void* zsave, void* y_raw, int64_t B, int64_t H, int64_t L, int conj_kf,
                                int64_t sb_u, int64_t sb_pre, int64_t sb_post, int64_t sb_add, int64_t sb_y, void* stream) {
  if (!p) return ffc_fail("null arg");
  if (y_raw && !zsave && p->hp.N1 > 1) return ffc_fail("y_raw without a spectrum buffer: single-tile sizes only (fft <= 2048)");
  if (y_raw && ((uintptr_t)y_raw & 15)) return ffc_fail("y_raw must be 16-byte aligned");
  if ((zsave || y_raw) && conj_kf) return ffc_fail("spectrum buffer / y_raw: forward pass only (conj_kf = 0)");
  if (addend && y && B > 0 && H > 0 && L > 0) {
    const int64_t sa = sb_add ? sb_add : H * L, sy = sb_y ? sb_y : H * L;
    const uintptr_t a0 = (uintptr_t)addend, a1 = a0 + (uintptr_t)(((B - 1) * sa + H * L) * 2);
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (uintptr_t)(((B - 1) * sy + H * L) * 2);
    if (a0 < y1 && y0 < a1) return ffc_fail("addend overlaps y");
  }
  FwdCall c = fwd_call(u, kf, pregate, postgate, y, B, H, L, stream);
  c.conj_kf = conj_kf; c.zsave = zsave; c.yraw = y_raw; c.addend = addend;
  c.sb_u = sb_u; c.sb_pre = sb_pre; c.sb_post = sb_post; c.sb_y = sb_y; c.sb_add = sb_add;
  return conv_fwd_impl(p, c);
}

// Forward / input-gradient pass with a LOW-PASS k_f: every non-zero bin f has k3 = f / (N1 N2) < rows or >= 32 - rows
// (rows <= 4), i.e. |f| < rows * N / 32 (FrequencySparseFFTConv with N_partial <= N / 4).  Same result as ffc_conv_fwd on the
// same (masked) k_f; the kernel skips the all-zero spectrum rows: half of the k_f loads and of the k_f product, and one of
// the two K-steps of the first inverse stage (reference: the truncated kernels, monarch_cuda/monarch_fwd_complex.h:462-528).
extern "C" int ffc_conv_fwd_sparse(const ffc_plan* p, const void* u, const void* kf, const void* pregate, const void* postgate,
                                   void* y, int64_t B, int64_t H, int64_t L, int conj_kf, int rows, void* stream) {
  if (rows < 1) return ffc_fail("frequency-sparse forward: rows must be >= 1");
  FwdCall c = fwd_call(u, kf, pregate, postgate, y, B, H, L, stream);
  c.conj_kf = conj_kf; c.sparse = rows;
  return conv_fwd_impl(p, c);
}

extern "C" int ffc_conv_fwd(const ffc_plan* p, const void* u, const void* kf, const void* pregate, const void* postgate, void* y,
                            int64_t B, int64_t H, int64_t L, int conj_kf, void* stream) {
  return ffc_conv_fwd_strided(p, u, kf, pregate, postgate, y, B, H, L, conj_kf, 0, 0, 0, 0, stream);
}

// ---- profiling build (N = 32768, bf16 only): same body with s_memtime phase counters
template <class GEO, int DT, bool GS = false, bool PL = false>
__global__ __launch_bounds__(GEO::WGW * 64, 2) void conv_prof_kernel(ConvArgs a) {
  int h, chunk;
  if (!map_block(a.H, a.nchunk, &h, &chunk)) return;
  using BD = Body<DevB, GEO, DT>;
  BD::setup_tables(a.tab, a.t);
  const int wv = DevB::wave();
  typename BD::Unit un;
  un.wq = wv % GEO::NW;
  const int u = wv / GEO::NW;
  un.eb = u * GEO::EBYTES;
  const int p0 = chunk * a.ppc;
  int p1 = p0 + a.ppc;
  if (p1 > a.npair) p1 = a.npair;
  if constexpr (GS) BD::template outer_jobs<true, true, false, false, false, true, PL>(a, h, p0, p1, u, un, blockIdx.x);      // (phase C stores the rows: no rows_out column)
  else if (16 * GEO::Mi >= a.L) BD::template outer_jobs<true, true>(a, h, p0, p1, u, un, blockIdx.x);
  else BD::template outer_jobs<false, true>(a, h, p0, p1, u, un, blockIdx.x);
}

// prof: device buffer of gridDim*8*8 uint64 (zero-initialised by the caller); returns grid size in *grid_out
extern "C" int ffc_conv_fwd_prof(const ffc_plan* p, const void* u, const void* kf, void* y, int64_t B, int64_t H, int64_t L,
                                 unsigned long long* prof, int* grid_out, void* stream) {
  if (!p || p->hp.N != 32768 || p->hp.dtype != DT_BF16) return ffc_fail("prof build: N=32768 bf16 only");
  using GEO = Geo<32, 32, 32>;
  ConvArgs a{};
  a.u = u; a.y = y; a.kf = kf; a.tab = p->d_blob; a.t = p->hp.tabs;
  a.B = (int)B; a.H = (int)H; a.L = (int)L; a.npair = (int)((B + 1) / 2); a.s_inv = (float)p->hp.s_inv; a.s_fwd = (float)p->hp.s_fwd;
  a.fast = (L % 8 == 0) && !(((uintptr_t)u | (uintptr_t)y) & 15);
  a.sbu = a.sbg = a.sbp = a.sby = H * L;
  a.flags = p->env_flags;
  a.prof = prof;
  ffc_choose_chunks(p, a.H, a.npair, &a.nchunk, &a.ppc);
  const FwdRoute r = fwd_route<GEO>(a);
  const int grid = r.grid;
  if (grid_out) *grid_out = grid;
  if (r.pl) return ffc_launch(conv_prof_kernel<GEO, DT_BF16, true, true>, "conv_prof_kernel", grid, GEO::WGW * 64, GEO::LDS_BYTES, GEO::LDS_BYTES, (hipStream_t)stream, a);
  if (r.gs) return ffc_launch(conv_prof_kernel<GEO, DT_BF16, true>, "conv_prof_kernel", grid, GEO::WGW * 64, GEO::LDS_BYTES, GEO::LDS_BYTES, (hipStream_t)stream, a);
  return ffc_launch(conv_prof_kernel<GEO, DT_BF16>, "conv_prof_kernel", grid, GEO::WGW * 64, GEO::LDS_BYTES, GEO::LDS_BYTES, (hipStream_t)stream, a);
}

// The module's forward in one call (see ffc_hip.hip for the backward's): k (H, Lk) fp32 -> kf_out, then y = postgate * conv(u *
// pregate, k); zsave / y_raw as in ffc_conv_fwd_z (both nullable).  Where a workgroup owns its head the k -> k_f step runs inside
// the convolution launch (Modes::kfft_head); otherwise ffc_kernel_fft first.
extern "C" int ffc_conv_fwd_k(const ffc_plan* p, const float* k, int64_t Lk, void* kf_out, const void* u, const void* pregate,
                              const void* postgate, void* y, void* zsave, void* y_raw, int64_t B, int64_t H, int64_t L, void* stream) {
  if (!p || !k || !kf_out) return ffc_fail("null arg");
  if (y_raw && ((uintptr_t)y_raw & 15)) return ffc_fail("y_raw must be 16-byte aligned");
  const bool fuse = kfft_in_launch(p, B, H) && Lk > 0 && Lk <= p->hp.N && H * Lk < ((int64_t)1 << 31);
  if (!fuse) {
    int rc = ffc_kernel_fft(p, k, H, Lk, kf_out, stream);
    if (rc) return rc;
  }
  FwdCall c = fwd_call(u, kf_out, pregate, postgate, y, B, H, L, stream);
  c.zsave = zsave; c.yraw = y_raw;
  if (fuse) { c.kfuse_k = k; c.kfuse_Lk = Lk; }
  return conv_fwd_impl(p, c);
}

// The forward of an HBM-level size's inner convolution in one call: the inner k_f rows from their complex input (pair-plane tensor
// (2, H, N), as ffc_kernel_fft_c; `scale` = that call's scale) into kf_out, then the convolution of the rows `u` (no gates at this
// level), spectra kept in zsave when given.  k -> k_f runs inside the convolution launch where a workgroup owns its "head".
extern "C" int ffc_conv_fwd_kx(const ffc_plan* p, const void* xpair, float scale, void* kf_out, const void* u, void* y, void* zsave,
                               int64_t B, int64_t H, int64_t L, void* stream) {
  if (!p || !xpair || !kf_out) return ffc_fail("null arg");
  const bool fuse = kfft_in_launch(p, B, H) && !((uintptr_t)xpair & 15);
  if (!fuse) {
    int rc = ffc_kernel_fft_c(p, xpair, H, kf_out, scale, stream);
    if (rc) return rc;
  }
  FwdCall c = fwd_call(u, kf_out, nullptr, nullptr, y, B, H, L, stream);
  c.zsave = zsave;
  if (fuse) { c.kfuse_x = xpair; c.kfuse_xscale = scale; }
  return conv_fwd_impl(p, c);
}
