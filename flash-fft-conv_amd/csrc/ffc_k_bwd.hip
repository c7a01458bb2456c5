// Fused backward kernel (Modes::bwd) + ffc_conv_bwd / ffc_conv_bwd_gated(_strided).  (Split from ffc_k_dkf.hip so that the two
// longest translation units of the library compile side by side.)
#include "ffc_bwd_launch.h"

// out[b, h, n] = x[b, h, n] * y[b, h, n] on (B, H, L) rows with batch strides (elements), fp32 product rounded once: the
// dpostgate = dout * y_raw of the multi-pass sizes (fft 65536 / 131072), whose backward kernel has no registers to spare for it
template <int DT>
__global__ __launch_bounds__(256) void mul_rows_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ y, uint16_t* __restrict__ out,
                                                       int64_t HL, int64_t sbx, int64_t sby, int64_t sbo, int fast) {
  const int b = blockIdx.y;
  const uint16_t* xb = x + b * sbx; const uint16_t* yb = y + b * sby; uint16_t* ob = out + b * sbo;
  if (fast) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HL / 8; i += (int64_t)gridDim.x * blockDim.x) {
      const u32x4v a = __builtin_nontemporal_load((const u32x4v*)xb + i), c = __builtin_nontemporal_load((const u32x4v*)yb + i);
      u32x4v o;
#pragma unroll
      for (int q = 0; q < 4; q++)
        o[q] = DevB::pack<DT>(DevB::unpack_lo<DT>(a[q]) * DevB::unpack_lo<DT>(c[q]), DevB::unpack_hi<DT>(a[q]) * DevB::unpack_hi<DT>(c[q]));
      __builtin_nontemporal_store(o, (u32x4v*)ob + i);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HL; i += (int64_t)gridDim.x * blockDim.x)
      ob[i] = (uint16_t)DevB::pack<DT>(DevB::unpack_lo<DT>(xb[i]) * DevB::unpack_lo<DT>(yb[i]), 0.f);
  }
}


// Fused backward: du = pregate * corr(dout*postgate, k), dpre = u * corr(...) (nullable, gated only) and the
// dk_f partial sums in `ws` (same layout as ffc_conv_bwd_dkf; finish with ffc_kernel_ifft_grad).
extern "C" int ffc_conv_bwd(const ffc_plan* p, const void* dout, const void* u, const void* kf, const void* pregate,
                            const void* postgate, void* du, void* dpre, void* ws, int64_t B, int64_t H, int64_t L, void* stream) {
  return ffc_conv_bwd_gated(p, dout, u, kf, pregate, postgate, du, dpre, nullptr, ws, B, H, L, stream);
}
// + dpost = dout * conv(u*pregate, k) (nullable).  Fused sizes >= 4096 produce it inside the same launch (one extra
// inverse transform per pair); the single-tile sizes (fft <= 2048: the 1024 kernel and its 2-pass form) run the forward kernel with dout as the output gate.
// Batch strides in elements (0 = contiguous H * L): every tensor may be a channel slice of a wider (B, C, L) tensor.
// One backward call, as the entry points below fill it (everything they do not name is zero / null).
struct BwdCall {
  const void *dout, *u, *kf, *pregate, *postgate;
  void *du, *dpre, *dpost, *ws;
  int64_t B, H, L;
  void* stream;
  int64_t sb_dout, sb_u, sb_pre, sb_post, sb_du, sb_dpre, sb_dpost;      // batch strides in elements, 0 = contiguous (H * L)
  const void *zin, *yraw;              // what the forward saved: spectra, output before the postgate
  // dk wanted from the same launch: real dk (H, Lk) fp32, or complex rows dk_pair with the caller's scale.  *dk_done says whether the
  // launch wrote it; otherwise the slabs in ws hold dk_f and the caller finishes with ffc_kernel_ifft_grad(_c)
  float* dk; int64_t Lk;
  void* dk_pair; float dk_pair_scale;
  bool* dk_done;
};
static BwdCall bwd_call(const void* dout, const void* u, const void* kf, const void* pregate, const void* postgate, void* du, void* dpre,
                        void* dpost, void* ws, int64_t B, int64_t H, int64_t L, void* stream) {
  BwdCall c{};
  c.dout = dout; c.u = u; c.kf = kf; c.pregate = pregate; c.postgate = postgate; c.du = du; c.dpre = dpre; c.dpost = dpost; c.ws = ws;
  c.B = B; c.H = H; c.L = L; c.stream = stream;
  return c;
}
static void bwd_strides(BwdCall* c, int64_t sb_dout, int64_t sb_u, int64_t sb_pre, int64_t sb_post, int64_t sb_du, int64_t sb_dpre, int64_t sb_dpost) {
  c->sb_dout = sb_dout; c->sb_u = sb_u; c->sb_pre = sb_pre; c->sb_post = sb_post; c->sb_du = sb_du; c->sb_dpre = sb_dpre; c->sb_dpost = sb_dpost;
}
static int conv_bwd_impl(const ffc_plan* p, const BwdCall& c) {
  const void *dout = c.dout, *u = c.u, *kf = c.kf, *pregate = c.pregate, *postgate = c.postgate, *zin = c.zin, *yraw = c.yraw;
  void *du = c.du, *dpre = c.dpre, *dpost = c.dpost, *ws = c.ws, *stream = c.stream;
  const int64_t B = c.B, H = c.H, L = c.L, Lk = c.Lk;
  int64_t sb_dout = c.sb_dout, sb_u = c.sb_u, sb_pre = c.sb_pre, sb_post = c.sb_post, sb_du = c.sb_du, sb_dpre = c.sb_dpre, sb_dpost = c.sb_dpost;
  if (!p || !dout || !kf || !du || !ws) return ffc_fail("null arg");
  // `u` is read by the recomputing kernels, as the gate of dpregate and by the forward run that makes dpostgate without y_raw; on saved
  // spectra without gates nothing reads it and a null pointer says so (the HBM-level sizes' inner call, flashfftconv/conv.py _big_backward)
  if (!u && (!zin || pregate || postgate || dpre || (dpost && !yraw))) return ffc_fail("null u: only with saved spectra and no gates");
  if (yraw && !dpost) return ffc_fail("y_raw needs a dpost output");
  // (single-tile sizes, fft <= 2048: y_raw also without the spectra -- the kernel transforms u * pregate again, rows it loads anyway)
  if (yraw && !zin && p->hp.N1 > 1) return ffc_fail("y_raw without the saved spectra: single-tile sizes (fft <= 2048) only");
  if (zin && (ffc_spectrum_bytes(p, B, H) == 0 || ((uintptr_t)zin & 15))) return ffc_fail("spectrum buffer: unsupported plan or misaligned");
  if (B <= 0 || H <= 0) return ffc_fail("empty batch/heads");
  if (L <= 0 || L > p->hp.N) return ffc_fail("L must be in (0, fft_size]");
  if ((uintptr_t)kf & 15) return ffc_fail("k_f must be 16-byte aligned");
  int64_t* sbs[7] = {&sb_dout, &sb_u, &sb_pre, &sb_post, &sb_du, &sb_dpre, &sb_dpost};
  int64_t any = 0;
  for (int i = 0; i < 7; i++) {
    if (*sbs[i] == 0) *sbs[i] = H * L;
    if (*sbs[i] < H * L || (B - 1) * *sbs[i] + H * L >= ((int64_t)1 << 31))
      return ffc_fail("tensor too large (>= 2^31 elements) or batch stride smaller than H*L");
    any |= *sbs[i];
  }
  DkfArgs d{};
  ConvArgs& a = d.c;
  a.u = u; a.kf = kf; a.pregate = pregate; a.postgate = postgate; a.tab = p->d_blob; a.t = p->hp.tabs;
  a.B = (int)B; a.H = (int)H; a.L = (int)L; a.npair = (int)((B + 1) / 2); a.s_inv = (float)p->hp.s_inv; a.s_fwd = (float)p->hp.s_fwd;
  a.sbu = sb_u; a.sbg = sb_pre; a.sbp = sb_post; a.sby = sb_du;
  d.sbd = sb_dout; d.sbdu = sb_du; d.sbdpre = sb_dpre; d.sbdpost = sb_dpost;
  a.fast = (L % 8 == 0) && !(((uintptr_t)u | (uintptr_t)dout | (uintptr_t)pregate | (uintptr_t)postgate | (uintptr_t)du | (uintptr_t)dpre) & 15) &&
           !(any & 7);
  ffc_choose_chunks(p, a.H, a.npair, &a.nchunk, &a.ppc);
  a.persist = ffc_persist(p);
  a.R = p->hp.R;
  a.stream = p->env_stream >= 0 ? p->env_stream : ((!pregate && !postgate && p->hp.R == 1) ? 1 : 0);    // see Body::gload8
  a.flags = p->env_flags;                        // tuning flags: 2 = k_f streamed, 4 = scratch streamed
  d.dout = dout; d.ws = (float*)ws; d.du = du; d.dpre = dpre; d.zscratch = ffc_zscratch(p, ws, a.H, a.nchunk);
  // dk from the same launch where the workgroup owns all pairs of its head (ffc::bwd_dk_form: Modes::dk_tail, or Modes::dk_tail_rp in every
  // pass of the multi-pass sizes), on the plan's bf16 tables (fp16 plans too)
  if (c.dk && c.dk_done && Lk > 0 && Lk <= p->hp.N && bwd_dk_form(p->hp, a.nchunk, p->env_flags, false) != DK_SEPARATE) {
    set_dk_tail(&d, c.dk, nullptr, (int)Lk, (float)(1.0 / p->hp.s_fwd), (Lk % 4 == 0) && !((uintptr_t)c.dk & 15), p->d_blob_bf, p->hp_bf.tabs);
    *c.dk_done = true;
  }
  // ... as complex rows (ffc_conv_bwd_kx: first step of dk at the HBM-level sizes; always bf16, the caller's scale)
  if (c.dk_pair && c.dk_done && !((uintptr_t)c.dk_pair & 15) && bwd_dk_form(p->hp, a.nchunk, p->env_flags, true) != DK_SEPARATE) {
    set_dk_tail(&d, nullptr, c.dk_pair, p->hp.N, c.dk_pair_scale, 1, p->d_blob_bf, p->hp_bf.tabs);
    *c.dk_done = true;
  }
  d.dpost = (p->hp.N1 > 1 || yraw) ? dpost : nullptr;      // with y_raw every geometry writes dpost from its dout row load
  d.zin = zin;
  d.yraw = yraw;
  if (yraw && p->hp.R > 1 && p->hp.N1 > 1) {
    // multi-pass sizes of the fused 32768 kernel: the product runs as a streaming kernel of its own (see mul_rows_kernel)
    const int64_t HL = H * L;
    const int fast = (HL % 8 == 0) && !((sb_dout | sb_dpost) & 7) && !(((uintptr_t)dout | (uintptr_t)yraw | (uintptr_t)dpost) & 15);
    int64_t nb = (HL / (fast ? 8 : 1) + 255) / 256;
    if (nb > 8192) nb = 8192;
    const dim3 grid((unsigned)nb, (unsigned)B), block(256);
    if (p->hp.dtype == DT_BF16)
      hipLaunchKernelGGL(mul_rows_kernel<DT_BF16>, grid, block, 0, (hipStream_t)stream, (const uint16_t*)dout, (const uint16_t*)yraw,
                         (uint16_t*)dpost, HL, sb_dout, HL, sb_dpost, fast);
    else
      hipLaunchKernelGGL(mul_rows_kernel<DT_F16>, grid, block, 0, (hipStream_t)stream, (const uint16_t*)dout, (const uint16_t*)yraw,
                         (uint16_t*)dpost, HL, sb_dout, HL, sb_dpost, fast);
    HIPCHK(hipGetLastError());
    d.dpost = nullptr; d.yraw = nullptr; dpost = nullptr;
  }
  if (d.dpost && ((((uintptr_t)dpost) | (uintptr_t)yraw) & 15)) a.fast = 0;
  // fused sizes >= 4096 on saved spectra: the ZM = 1 kernels (ffc_k_bwdz.hip); everything else from this unit
  int rc = (zin && p->hp.N1 > 1) ? ffc_bwdz_launch(p->hp.N, p->hp.dtype, d, (hipStream_t)stream)
                                 : ffc_dispatch<BwdLaunchZ<0>::T>(p->hp.N, p->hp.dtype, d, (hipStream_t)stream);
  if (rc || !dpost || d.dpost) return rc;
  return ffc_conv_fwd_strided(p, u, kf, pregate, dout, dpost, B, H, L, 0, sb_u, sb_pre, sb_dout, sb_dpost, stream);
}
extern "C" int ffc_conv_bwd_gated_strided(const ffc_plan* p, const void* dout, const void* u, const void* kf, const void* pregate,
                                          const void* postgate, void* du, void* dpre, void* dpost, void* ws, int64_t B, int64_t H,
                                          int64_t L, int64_t sb_dout, int64_t sb_u, int64_t sb_pre, int64_t sb_post,
                                          int64_t sb_du, int64_t sb_dpre, int64_t sb_dpost, void* stream) {
  BwdCall c = bwd_call(dout, u, kf, pregate, postgate, du, dpre, dpost, ws, B, H, L, stream);
  bwd_strides(&c, sb_dout, sb_u, sb_pre, sb_post, sb_du, sb_dpre, sb_dpost);
  return conv_bwd_impl(p, c);
}
// fused backward on the spectra saved by ffc_conv_fwd_z (same B, H, L, u, pregate): the first transform of every pair is skipped
extern "C" int ffc_conv_bwd_z(const ffc_plan* p, const void* dout, const void* u, const void* kf, const void* pregate,
                              const void* postgate, void* du, void* dpre, void* dpost, void* ws, const void* zin, int64_t B, int64_t H,
                              int64_t L, int64_t sb_dout, int64_t sb_u, int64_t sb_pre, int64_t sb_post,
                              int64_t sb_du, int64_t sb_dpre, int64_t sb_dpost, void* stream) {
  if (!zin) return ffc_fail("null spectrum buffer");
  BwdCall c = bwd_call(dout, u, kf, pregate, postgate, du, dpre, dpost, ws, B, H, L, stream);
  bwd_strides(&c, sb_dout, sb_u, sb_pre, sb_post, sb_du, sb_dpre, sb_dpost);
  c.zin = zin;
  return conv_bwd_impl(p, c);
}
// ... and on the forward output before the postgate multiply that ffc_conv_fwd_z stored (y_raw, contiguous (B,H,L)): dpost =
// dout * y_raw is written from the registers that hold the dout rows (same fp32 product, rounded once, as the output gate)
extern "C" int ffc_conv_bwd_zy(const ffc_plan* p, const void* dout, const void* u, const void* kf, const void* pregate,
                               const void* postgate, void* du, void* dpre, void* dpost, void* ws, const void* zin, const void* y_raw,
                               int64_t B, int64_t H, int64_t L, int64_t sb_dout, int64_t sb_u, int64_t sb_pre, int64_t sb_post,
                               int64_t sb_du, int64_t sb_dpre, int64_t sb_dpost, void* stream) {
  if ((!zin && !(p && p->hp.N1 <= 1)) || !y_raw || !dpost) return ffc_fail("null spectrum / y_raw / dpost buffer (y_raw alone: single-tile sizes, fft <= 2048)");
  BwdCall c = bwd_call(dout, u, kf, pregate, postgate, du, dpre, dpost, ws, B, H, L, stream);
  bwd_strides(&c, sb_dout, sb_u, sb_pre, sb_post, sb_du, sb_dpre, sb_dpost);
  c.zin = zin; c.yraw = y_raw;
  return conv_bwd_impl(p, c);
}
extern "C" int ffc_conv_bwd_gated(const ffc_plan* p, const void* dout, const void* u, const void* kf, const void* pregate,
                                  const void* postgate, void* du, void* dpre, void* dpost, void* ws, int64_t B, int64_t H,
                                  int64_t L, void* stream) {
  return ffc_conv_bwd_gated_strided(p, dout, u, kf, pregate, postgate, du, dpre, dpost, ws, B, H, L, 0, 0, 0, 0, 0, 0, 0, stream);
}

// The module's whole backward in one call: du (+ dpre, dpost) and dk (H, Lk) fp32; zin / y_raw: what ffc_conv_fwd_k saved (nullable:
// recomputing kernel).  dk comes out of the backward launch itself where a workgroup owns its head (Modes::dk_tail), through the
// fp32 slabs in ws + ffc_kernel_ifft_grad otherwise.
extern "C" int ffc_conv_bwd_k(const ffc_plan* p, const void* dout, const void* u, const void* kf, const void* pregate, const void* postgate,
                              void* du, void* dpre, void* dpost, void* ws, const void* zin, const void* y_raw, float* dk, int64_t Lk,
                              int64_t B, int64_t H, int64_t L, void* stream) {
  if (!dk) return ffc_fail("null dk");
  bool dk_done = false;
  BwdCall c = bwd_call(dout, u, kf, pregate, postgate, du, dpre, dpost, ws, B, H, L, stream);
  c.zin = zin; c.yraw = ((zin || p->hp.N1 <= 1) && y_raw && dpost) ? y_raw : nullptr;
  c.dk = dk; c.Lk = Lk; c.dk_done = &dk_done;
  int rc = conv_bwd_impl(p, c);
  if (rc || dk_done) return rc;
  return ffc_kernel_ifft_grad(p, ws, B, H, Lk, dk, stream);
}

// The backward of an HBM-level size's inner convolution in one call: input-gradient rows du and the dk rows as a complex pair-plane
// tensor (2, H, N) bf16 (as ffc_kernel_ifft_grad_c with `scale`), out of the backward launch itself where a workgroup owns its
// "head", through the fp32 slabs in ws otherwise.  zin: the spectra ffc_conv_fwd_kx kept (nullable).
extern "C" int ffc_conv_bwd_kx(const ffc_plan* p, const void* dout, const void* u, const void* kf, void* du, void* ws, const void* zin,
                               void* outpair, float scale, int64_t B, int64_t H, int64_t L, void* stream) {
  if (!outpair) return ffc_fail("null outpair");
  bool dk_done = false;
  BwdCall c = bwd_call(dout, u, kf, nullptr, nullptr, du, nullptr, nullptr, ws, B, H, L, stream);
  c.zin = zin; c.dk_pair = outpair; c.dk_pair_scale = scale; c.dk_done = &dk_done;
  int rc = conv_bwd_impl(p, c);
  if (rc || dk_done) return rc;
  return ffc_kernel_ifft_grad_c(p, ws, B, H, outpair, scale, stream);
}
