// CPU wave simulator: runs the very same kernel body (ffc_body.h) with a 64-lane vector backend,
// one host thread per wavefront, pthread barrier = s_barrier, a byte array = LDS.
// TEST INFRASTRUCTURE ONLY (tests/ and __graft_entry__.build use it); the product path is the
// HIP library.  It models the gfx950 primitives the body relies on:
//   v_mfma_f32_32x32x16_{bf16,f16} and v_mfma_f32_16x16x32_{bf16,f16} operand / accumulator lane layouts, ds_read_b64_tr_b16,
//   RNE fp32->bf16/f16 packing, 8-byte predicated global accesses.
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#define FFC_FN inline __attribute__((always_inline))
#include "ffc_body.h"
#include "ffc_modes.h"
#include "ffc_big.h"
#include "ffc_route.h"

namespace ffc {

template <class T>
struct Vec {
  T v[64];
  Vec() {}
  Vec(T s) { for (int i = 0; i < 64; i++) v[i] = s; }
};
#define VOP(op)                                                                           \
  template <class T> inline Vec<T> operator op(const Vec<T>& a, const Vec<T>& b) {        \
    Vec<T> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] op b.v[i]; return r; }         \
  template <class T> inline Vec<T> operator op(const Vec<T>& a, T b) {                    \
    Vec<T> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] op b; return r; }              \
  template <class T> inline Vec<T> operator op(T a, const Vec<T>& b) {                    \
    Vec<T> r; for (int i = 0; i < 64; i++) r.v[i] = a op b.v[i]; return r; }
VOP(+) VOP(-) VOP(*) VOP(/) VOP(%) VOP(&) VOP(|) VOP(^)
#undef VOP
template <class T> inline Vec<T> operator<<(const Vec<T>& a, int s) { Vec<T> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] << s; return r; }
template <class T> inline Vec<T> operator>>(const Vec<T>& a, int s) { Vec<T> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] >> s; return r; }
// mixed u32 vector with int literal masks
inline Vec<uint32_t> operator&(const Vec<uint32_t>& a, unsigned b) { Vec<uint32_t> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] & b; return r; }
inline Vec<int> operator*(const Vec<int>& a, long b) { return a * (int)b; }
inline Vec<bool> operator<(const Vec<int>& a, int b) { Vec<bool> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] < b; return r; }
inline Vec<bool> operator<(const Vec<int>& a, const Vec<int>& b) { Vec<bool> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] < b.v[i]; return r; }
inline Vec<bool> operator>=(const Vec<int>& a, int b) { Vec<bool> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] >= b; return r; }
inline Vec<bool> operator&&(const Vec<bool>& a, const Vec<bool>& b) { Vec<bool> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] && b.v[i]; return r; }
inline Vec<bool> operator&&(const Vec<bool>& a, bool b) { Vec<bool> r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] && b; return r; }

struct WgCtx {
  std::vector<uint8_t> lds;
  pthread_barrier_t bar;
  int nwaves;
};
static thread_local WgCtx* g_wg = nullptr;
static thread_local int g_wave = 0;
static thread_local Vec<float> g_agpr[128];   // per-wave accumulation registers (DevB: a0..a127)
static std::atomic<long> g_dma_count{0};      // LDS-DMA instructions executed (tests: the path under test really ran)
static std::atomic<long> g_gs_count{0};       // runs of a direct-store kernel variant (FwdRoute::gs / BwdRoute::gs), likewise
static std::atomic<long> g_pl_count{0};       // ... and of their plain-input forms (FwdRoute::pl / BwdRoute::pl)
static int g_sim_flags = 0;                   // tuning flags (FFC_FLAGS) of the next calls: ffcsim_set_flags

static inline float dt_to_f32(int DT, uint16_t h) { return DT == DT_BF16 ? bf16_to_f32(h) : f16_to_f32(h); }
static inline uint16_t f32_to_dt(int DT, float f) { return DT == DT_BF16 ? f32_to_bf16(f) : f32_to_f16(f); }

struct SimB {
  static constexpr bool LEAN_OUTER = false;
  static constexpr bool FAST_ONLY = false;
  static constexpr bool HAS_ADD = false;
  using f32 = Vec<float>;
  using i32 = Vec<int>;
  using u32 = Vec<uint32_t>;
  using pred = Vec<bool>;
  struct U2 { u32 x, y; };
  struct U4 { u32 x, y, z, w; };
  struct A16 { f32 v[16]; f32& operator[](int i) { return v[i]; } const f32& operator[](int i) const { return v[i]; } };
  struct W4 { u32 v[4]; u32& operator[](int i) { return v[i]; } const u32& operator[](int i) const { return v[i]; } };
  struct A4 { f32 v[4]; f32& operator[](int i) { return v[i]; } const f32& operator[](int i) const { return v[i]; } };
  static A4 a4_zero() { A4 z; for (int i = 0; i < 4; i++) z.v[i] = f32(0.f); return z; }
  template <bool CONJ> static void cmul16(A16& re, A16& im, const A16& tr, const A16& ti) {
    for (int r = 0; r < 16; r++) {
      f32 a = re[r], b = im[r];
      if (!CONJ) { re[r] = a * tr[r] - b * ti[r]; im[r] = a * ti[r] + b * tr[r]; }
      else { re[r] = a * tr[r] + b * ti[r]; im[r] = b * tr[r] - a * ti[r]; }
    }
  }
  struct F2 { f32 x, y; };
  static F2 f2(const f32& a, const f32& b) { F2 v; v.x = a; v.y = b; return v; }
  static f32 f2_lo(const F2& v) { return v.x; }
  static f32 f2_hi(const F2& v) { return v.y; }
  static void cmulp(const F2& xr, const F2& xi, const f32& wr, const f32& wi, F2& yr, F2& yi) {
    F2 r, i;
    r.x = xr.x * wr - xi.x * wi; r.y = xr.y * wr - xi.y * wi;
    i.x = xr.x * wi + xi.x * wr; i.y = xr.y * wi + xi.y * wr;
    yr = r; yi = i;
  }
  template <bool CONJ>
  static void cmul2v(A16& re, A16& im, int r0, const F2& tr, const F2& ti) { cmul2<CONJ>(re, im, r0, tr.x, tr.y, ti.x, ti.y); }
  static void cmac2_conj(F2& wr, F2& wi, const A16& a, const A16& b, int r0, const F2& zr, const F2& zi) {
    wr.x = wr.x + (a[r0] * zr.x + b[r0] * zi.x);
    wr.y = wr.y + (a[r0 + 1] * zr.y + b[r0 + 1] * zi.y);
    wi.x = wi.x + (b[r0] * zr.x - a[r0] * zi.x);
    wi.y = wi.y + (b[r0 + 1] * zr.y - a[r0 + 1] * zi.y);
  }
  static void agpr_reserve() {}
  template <int I> static f32 agpr_get() { return g_agpr[I]; }
  template <int I> static void agpr_set(const f32& x) { g_agpr[I] = x; }
  static void pin(W4&) {}
  static void pin4(U4&) {}
  static void sched_fence() {}
  template <bool CONJ>
  static void cmul2(A16& re, A16& im, int r0, const f32& tr0, const f32& tr1, const f32& ti0, const f32& ti1) {
    const f32* tr[2] = {&tr0, &tr1}; const f32* ti[2] = {&ti0, &ti1};
    for (int q = 0; q < 2; q++) {
      f32 a = re[r0 + q], b = im[r0 + q];
      if (!CONJ) { re[r0 + q] = a * *tr[q] - b * *ti[q]; im[r0 + q] = a * *ti[q] + b * *tr[q]; }
      else { re[r0 + q] = a * *tr[q] + b * *ti[q]; im[r0 + q] = b * *tr[q] - a * *ti[q]; }
    }
  }
  static A16 a16_scale(const A16& a, float s) { A16 r; for (int i = 0; i < 16; i++) r[i] = a[i] * f32(s); return r; }
  static A16 a16_zero() { A16 z; for (int i = 0; i < 16; i++) z.v[i] = f32(0.f); return z; }
  static W4 w4(const u32& a, const u32& b, const u32& c, const u32& e) { W4 v; v.v[0] = a; v.v[1] = b; v.v[2] = c; v.v[3] = e; return v; }
  static bool HAS_TR;

  static i32 lane() { i32 r; for (int i = 0; i < 64; i++) r.v[i] = i; return r; }
  static int wave() { return g_wave; }
  static void barrier() { if (g_wg->nwaves > 1) pthread_barrier_wait(&g_wg->bar); }
  static f32 fconst(float c) { return f32(c); }
  static pred ptrue() { return pred(true); }
  static pred pfalse() { return pred(false); }
  static f32 as_f32(const u32& a) { f32 r; for (int i = 0; i < 64; i++) memcpy(&r.v[i], &a.v[i], 4); return r; }
  static u32 as_u32(const f32& a) { u32 r; for (int i = 0; i < 64; i++) memcpy(&r.v[i], &a.v[i], 4); return r; }

  static uint8_t* L() { return g_wg->lds.data(); }
  static void chk(int off, int n) { if (off < 0 || off + n > (int)g_wg->lds.size() || (off & (n - 1))) abort(); }
  static U2 lds_r64(const i32& off) {
    U2 r;
    for (int i = 0; i < 64; i++) { chk(off.v[i], 8); memcpy(&r.x.v[i], L() + off.v[i], 4); memcpy(&r.y.v[i], L() + off.v[i] + 4, 4); }
    return r;
  }
  static void lds_w64(const i32& off, const U2& v) {
    for (int i = 0; i < 64; i++) { chk(off.v[i], 8); memcpy(L() + off.v[i], &v.x.v[i], 4); memcpy(L() + off.v[i] + 4, &v.y.v[i], 4); }
  }
  static void lds_w32(const i32& off, const u32& v) {
    for (int i = 0; i < 64; i++) { chk(off.v[i], 4); memcpy(L() + off.v[i], &v.v[i], 4); }
  }
  static void lds_w128(const i32& off, const U4& v, const pred& p) {
    for (int i = 0; i < 64; i++)
      if (p.v[i]) {
        chk(off.v[i], 16);
        memcpy(L() + off.v[i], &v.x.v[i], 4); memcpy(L() + off.v[i] + 4, &v.y.v[i], 4);
        memcpy(L() + off.v[i] + 8, &v.z.v[i], 4); memcpy(L() + off.v[i] + 12, &v.w.v[i], 4);
      }
  }
  static U4 lds_r128(const i32& off) {
    U4 r;
    for (int i = 0; i < 64; i++) {
      chk(off.v[i], 16);
      memcpy(&r.x.v[i], L() + off.v[i], 4); memcpy(&r.y.v[i], L() + off.v[i] + 4, 4);
      memcpy(&r.z.v[i], L() + off.v[i] + 8, 4); memcpy(&r.w.v[i], L() + off.v[i] + 12, 4);
    }
    return r;
  }
  static void lds_w16(const i32& off, const u32& v) {
    for (int i = 0; i < 64; i++) { chk(off.v[i], 2); uint16_t h = (uint16_t)v.v[i]; memcpy(L() + off.v[i], &h, 2); }
  }
  static u32 lds_r32(const i32& off) {
    u32 r;
    for (int i = 0; i < 64; i++) { chk(off.v[i], 4); memcpy(&r.v[i], L() + off.v[i], 4); }
    return r;
  }
  static u32 lds_r16(const i32& off) {
    u32 r;
    for (int i = 0; i < 64; i++) { chk(off.v[i], 2); uint16_t h; memcpy(&h, L() + off.v[i], 2); r.v[i] = h; }
    return r;
  }
  // ds_read_b64_tr_b16: within each 16-lane group lane i' supplies the address of 4 b16 values
  // M[i'][0..3]; lane i receives elements j=0..3 = M[4j + (i>>2)][i&3].
  static U2 lds_r64_tr(const i32& off) {
    U2 r;
    for (int g = 0; g < 4; g++) {
      uint16_t M[16][4];
      for (int i = 0; i < 16; i++) { chk(off.v[g * 16 + i], 8); memcpy(M[i], L() + off.v[g * 16 + i], 8); }
      for (int i = 0; i < 16; i++) {
        uint16_t e[4];
        for (int j = 0; j < 4; j++) e[j] = M[4 * j + (i >> 2)][i & 3];
        r.x.v[g * 16 + i] = e[0] | ((uint32_t)e[1] << 16);
        r.y.v[g * 16 + i] = e[2] | ((uint32_t)e[3] << 16);
      }
    }
    return r;
  }
  static void lds_fence() {}
  // LDS-DMA model: executed at issue (the simulator has no asynchronous memory pipe; the ordering rules -- vmcnt before the
  // wave's own reads -- are the device code's business)
  template <bool NT>
  static void g2lds32(const void* base, const i32& dw, int lds_off) {
    g_dma_count++;
    for (int i = 0; i < 64; i++) { chk(lds_off + 4 * i, 4); memcpy(L() + lds_off + 4 * i, (const uint32_t*)base + dw.v[i], 4); }
  }
  template <bool NT>
  static void g2lds128(const void* base, const i32& o16, int lds_off) {
    g_dma_count++;
    for (int i = 0; i < 64; i++) { chk(lds_off + 16 * i, 16); memcpy(L() + lds_off + 16 * i, (const uint8_t*)base + 16 * (int64_t)o16.v[i], 16); }
  }
  static void vm_wait0() {}
  template <int N> static void vm_wait() {}
  static void lds_wait0() {}
  static void lds_w32p(const i32& off, const u32& v, const pred& p) {
    for (int i = 0; i < 64; i++) if (p.v[i]) { chk(off.v[i], 4); memcpy(L() + off.v[i], &v.v[i], 4); }
  }
  static pred pnot(const pred& p) { pred r; for (int i = 0; i < 64; i++) r.v[i] = !p.v[i]; return r; }
  static i32 mul24(const i32& a, const i32& b) { return a * b; }
  static unsigned long long clock() { return 0; }
  template <int P> static void setprio() {}
  static U2 u2_from64(unsigned long long v) { U2 r; r.x = u32((uint32_t)v); r.y = u32((uint32_t)(v >> 32)); return r; }
  static void settle(f32&, f32&) {}
  static f32 i2f(const i32& a) { f32 r; for (int i = 0; i < 64; i++) r.v[i] = (float)a.v[i]; return r; }
  static f32 cos_rev(const f32& a) { f32 r; for (int i = 0; i < 64; i++) r.v[i] = (float)cos(6.283185307179586 * (double)a.v[i]); return r; }
  static f32 sin_rev(const f32& a) { f32 r; for (int i = 0; i < 64; i++) r.v[i] = (float)sin(6.283185307179586 * (double)a.v[i]); return r; }
  static i32 opaque(const i32& x) { return x; }
  static u32 uconst(uint32_t c) { return u32(c); }
  static i32 imin(const i32& a, int b) { i32 r; for (int i = 0; i < 64; i++) r.v[i] = a.v[i] < b ? a.v[i] : b; return r; }
  static u32 merge_lo(const u32& a, const u32& b) { u32 r; for (int i = 0; i < 64; i++) r.v[i] = (a.v[i] & 0xffffu) | (b.v[i] << 16); return r; }
  static u32 merge_hi(const u32& a, const u32& b) { u32 r; for (int i = 0; i < 64; i++) r.v[i] = (a.v[i] >> 16) | (b.v[i] & 0xffff0000u); return r; }
  static u32 sel(const pred& p, const u32& a, const u32& b) { u32 r; for (int i = 0; i < 64; i++) r.v[i] = p.v[i] ? a.v[i] : b.v[i]; return r; }
  static u32 g_r16(const void* base, const i32& e, const pred& p) {
    u32 r;
    for (int i = 0; i < 64; i++) { uint16_t h = 0; if (p.v[i]) memcpy(&h, (const uint8_t*)base + (int64_t)e.v[i] * 2, 2); r.v[i] = h; }
    return r;
  }
  static void g_w16(void* base, const i32& e, const u32& v, const pred& p) {
    for (int i = 0; i < 64; i++) if (p.v[i]) { uint16_t h = (uint16_t)v.v[i]; memcpy((uint8_t*)base + (int64_t)e.v[i] * 2, &h, 2); }
  }
  static u32 g_r32(const void* base, const i32& e, const pred& p) {
    u32 r;
    for (int i = 0; i < 64; i++) { uint32_t h = 0; if (p.v[i]) memcpy(&h, (const uint8_t*)base + (int64_t)e.v[i] * 4, 4); r.v[i] = h; }
    return r;
  }
  static void g_w32(void* base, const i32& e, const u32& v, const pred& p) {
    for (int i = 0; i < 64; i++) if (p.v[i]) memcpy((uint8_t*)base + (int64_t)e.v[i] * 4, &v.v[i], 4);
  }
  // the hardware's range check of a raw buffer: lanes at or beyond the row's size in bytes are dropped
  template <bool NT>
  static void row_w64(void* row, int nbytes, const i32& off, const U2& v) {
    for (int i = 0; i < 64; i++)
      if ((uint32_t)off.v[i] < (uint32_t)nbytes) { uint8_t* q = (uint8_t*)row + off.v[i]; memcpy(q, &v.x.v[i], 4); memcpy(q + 4, &v.y.v[i], 4); }
  }
  static U2 g_r64(const void* base, const i32& o8, const pred& p) {
    U2 r;
    for (int i = 0; i < 64; i++) {
      if (p.v[i]) { const uint8_t* q = (const uint8_t*)base + (int64_t)o8.v[i] * 8; memcpy(&r.x.v[i], q, 4); memcpy(&r.y.v[i], q + 4, 4); }
      else { r.x.v[i] = 0; r.y.v[i] = 0; }
    }
    return r;
  }
  static void g_w64(void* base, const i32& o8, const U2& v, const pred& p) {
    for (int i = 0; i < 64; i++)
      if (p.v[i]) { uint8_t* q = (uint8_t*)base + (int64_t)o8.v[i] * 8; memcpy(q, &v.x.v[i], 4); memcpy(q + 4, &v.y.v[i], 4); }
  }
  static void g_w64_nt(void* base, const i32& o8, const U2& v, const pred& p) { g_w64(base, o8, v, p); }
  static U4 g_r128(const void* base, const i32& o16) {
    U4 r;
    for (int i = 0; i < 64; i++) {
      const uint8_t* q = (const uint8_t*)base + (int64_t)o16.v[i] * 16;
      memcpy(&r.x.v[i], q, 4); memcpy(&r.y.v[i], q + 4, 4); memcpy(&r.z.v[i], q + 8, 4); memcpy(&r.w.v[i], q + 12, 4);
    }
    return r;
  }
  static U4 g_r128_nt(const void* base, const i32& o16) { return g_r128(base, o16); }
  static U4 g_r128p(const void* base, const i32& o16, const pred& p) {
    U4 r;
    for (int i = 0; i < 64; i++) {
      if (p.v[i]) {
        const uint8_t* q = (const uint8_t*)base + (int64_t)o16.v[i] * 16;
        memcpy(&r.x.v[i], q, 4); memcpy(&r.y.v[i], q + 4, 4); memcpy(&r.z.v[i], q + 8, 4); memcpy(&r.w.v[i], q + 12, 4);
      } else { r.x.v[i] = r.y.v[i] = r.z.v[i] = r.w.v[i] = 0; }
    }
    return r;
  }
  static void g_w128(void* base, const i32& o16, const U4& v, const pred& p) {
    for (int i = 0; i < 64; i++)
      if (p.v[i]) {
        uint8_t* q = (uint8_t*)base + (int64_t)o16.v[i] * 16;
        memcpy(q, &v.x.v[i], 4); memcpy(q + 4, &v.y.v[i], 4); memcpy(q + 8, &v.z.v[i], 4); memcpy(q + 12, &v.w.v[i], 4);
      }
  }
  static void g_w128_nt(void* base, const i32& o16, const U4& v, const pred& p) { g_w128(base, o16, v, p); }
  // D[i][j] += sum_k A[i][k] B[k][j];  A lane l: A[l&31][8*(l>>5)+e];  B lane l: B[8*(l>>5)+e][l&31];
  // D lane l reg r: D[acc_row(r, l>>5)][l&31].
  template <int DT>
  static void mfma(A16& acc, const W4& a, const W4& b) {
    float A[32][16], Bm[16][32];
    for (int l = 0; l < 64; l++)
      for (int e = 0; e < 8; e++) {
        uint16_t ha = (uint16_t)(a[e >> 1].v[l] >> (16 * (e & 1)));
        uint16_t hb = (uint16_t)(b[e >> 1].v[l] >> (16 * (e & 1)));
        A[l & 31][8 * (l >> 5) + e] = dt_to_f32(DT, ha);
        Bm[8 * (l >> 5) + e][l & 31] = dt_to_f32(DT, hb);
      }
    for (int l = 0; l < 64; l++)
      for (int r = 0; r < 16; r++) {
        int i = acc_row(r, l >> 5), j = l & 31;
        float s = 0;
        for (int k = 0; k < 16; k++) s += A[i][k] * Bm[k][j];
        acc[r].v[l] += s;
      }
  }
  // v_mfma_f32_16x16x32: D[i][j] += sum_k A[i][k] B[k][j];  A lane l: A[l&15][8*(l>>4)+e];  B lane l: B[8*(l>>4)+e][l&15];
  // D lane l reg r: D[4*(l>>4)+r][l&15]  (CDNA4 ISA, MFMA register layouts of the 16x16x32 16-bit forms).
  template <int DT>
  static void mfma16(A4& acc, const W4& a, const W4& b) {
    float A[16][32], Bm[32][16];
    for (int l = 0; l < 64; l++)
      for (int e = 0; e < 8; e++) {
        uint16_t ha = (uint16_t)(a[e >> 1].v[l] >> (16 * (e & 1)));
        uint16_t hb = (uint16_t)(b[e >> 1].v[l] >> (16 * (e & 1)));
        A[l & 15][8 * (l >> 4) + e] = dt_to_f32(DT, ha);
        Bm[8 * (l >> 4) + e][l & 15] = dt_to_f32(DT, hb);
      }
    for (int l = 0; l < 64; l++)
      for (int r = 0; r < 4; r++) {
        int i = 4 * (l >> 4) + r, j = l & 15;
        float s = 0;
        for (int k = 0; k < 32; k++) s += A[i][k] * Bm[k][j];
        acc[r].v[l] += s;
      }
  }
  template <int DT> static u32 pack(const f32& lo, const f32& hi) {
    u32 r;
    for (int i = 0; i < 64; i++) r.v[i] = f32_to_dt(DT, lo.v[i]) | ((uint32_t)f32_to_dt(DT, hi.v[i]) << 16);
    return r;
  }
  // v_pk_mul_f16: the exact fp32 product of two fp16 values rounded once to fp16 (= the native fp16 multiply)
  static u32 pk_mul_f16(const u32& a, const u32& b) {
    u32 r;
    for (int i = 0; i < 64; i++) {
      float lo = f16_to_f32((uint16_t)a.v[i]) * f16_to_f32((uint16_t)b.v[i]);
      float hi = f16_to_f32((uint16_t)(a.v[i] >> 16)) * f16_to_f32((uint16_t)(b.v[i] >> 16));
      r.v[i] = f32_to_f16(lo) | ((uint32_t)f32_to_f16(hi) << 16);
    }
    return r;
  }
  template <int DT> static f32 unpack_lo(const u32& a) { f32 r; for (int i = 0; i < 64; i++) r.v[i] = dt_to_f32(DT, (uint16_t)a.v[i]); return r; }
  template <int DT> static f32 unpack_hi(const u32& a) { f32 r; for (int i = 0; i < 64; i++) r.v[i] = dt_to_f32(DT, (uint16_t)(a.v[i] >> 16)); return r; }
};
bool SimB::HAS_TR = true;
// mirrors DevBO: the backward kernels use the per-tile outer stages
struct SimBO : SimB { static constexpr bool LEAN_OUTER = true; };
struct SimBA : SimB { static constexpr bool HAS_ADD = true; };           // forward kernels with an addend in the output epilogue (DevBA)
struct SimBOF : SimBO { static constexpr bool FAST_ONLY = true; };      // the fast-only instantiation of the multi-pass backward (DevBOF)
static bool g_force_slow = false;

// Run `fn(wg_index)` for one workgroup of nwaves wavefronts with lds_bytes of LDS.
template <class F>
static void run_wg(int nwaves, int lds_bytes, F fn) {
  WgCtx ctx;
  ctx.lds.assign(lds_bytes, 0xCD);
  ctx.nwaves = nwaves;
  pthread_barrier_init(&ctx.bar, nullptr, nwaves);
  std::vector<std::thread> th;
  for (int w = 0; w < nwaves; w++)
    th.emplace_back([&, w]() { g_wg = &ctx; g_wave = w; fn(); });
  for (auto& t : th) t.join();
  pthread_barrier_destroy(&ctx.bar);
}

// Every runner below asks the library's launch rules (ffc_route.h) which instantiation a call takes and runs that one, one workgroup
// per (head, chunk) job.  -8: the library has no kernel for the call.
static constexpr int NO_KERNEL = -8;
// LDS of the backward-side runners: the single-tile sizes with room for the per-pass tables of fft 2048
template <class GEO> constexpr int sim_lds() { return GEO::LDS_BYTES + (GEO::OUTER ? 0 : 4 * IPASS_BYTES); }
// job(h, c) as one workgroup of 8 waves per (head, chunk)
template <class F>
static int sim_jobs(int H, int nchunk, int lds, F job) {
  for (int h = 0; h < H; h++)
    for (int c = 0; c < nchunk; c++) run_wg(8, lds, [&]() { job(h, c); });
  return 0;
}

// SB: SimB (conv_kernel / conv_rp_kernel), or SimBA for the forward with an addend (conv_res_kernel / conv_res_rp_kernel)
template <class GEO, int DT, class SB = SimB>
static int sim_conv_t(const ConvArgs& a) {
  using BD = Body<SB, GEO, DT>;
  static_assert(BD::IPASS_BYTES == IPASS_BYTES && GEO::WGW == 8, "ffc_route.h");
  const FwdRoute r = fwd_route<GEO>(a);
  if (r.err) return NO_KERNEL;
  if (r.gs) {      // conv_kernel<.., GS>: phase C stores the rows (ConvLaunch)
    if constexpr (!SB::HAS_ADD && GEO::N == 32768) {
      g_gs_count++;
      if (r.pl) g_pl_count++;
      return pick([&](auto sz, auto pl) -> int {
        return sim_jobs(a.H, a.nchunk, r.lds, [&](int h, int c) {
          BD::setup_tables(a.tab, a.t);
          if (a.kfuse_k || a.kfuse_x) Modes<SB, GEO, DT>::kfft_head(a, h);
          BD::template conv_job<true, false, decltype(sz)::value, false, true, decltype(pl)::value>(a, h, c);
        });
      }, r.sz, r.pl);
    } else {
      return NO_KERNEL;
    }
  }
  return pick([&](auto mp, auto half, auto sz, auto sp) -> int {
    constexpr bool MP = decltype(mp)::value, HALF = decltype(half)::value, SZ = decltype(sz)::value, SP = decltype(sp)::value;
    if constexpr (!fwd_kernel_exists<GEO>(SB::HAS_ADD, MP, HALF, SZ, SP)) {
      return NO_KERNEL;
    } else if constexpr (MP) {      // the passes run one after the other in the same workgroup
      return sim_jobs(a.H, a.nchunk, r.lds, [&](int h, int c) {
        BD::setup_tables(a.tab, a.t);
        if constexpr (!GEO::OUTER) BD::setup_tables_ipass(a.tab, a.t, a.R);
        BD::template conv_job<HALF, true, SZ>(a, h, c);
      });
    } else {
      return sim_jobs(a.H, a.nchunk, r.lds, [&](int h, int c) {
        if constexpr (GEO::OUTER && GEO::NW > 1 && !SP && !SB::HAS_ADD) {
          if (a.kfuse_k || a.kfuse_x) {   // k -> k_f of this head inside the same workgroup (ConvArgs::kfuse_k / kfuse_x)
            BD::setup_tables(a.tab, a.t);
            Modes<SB, GEO, DT>::kfft_head(a, h);
            BD::template conv_job<HALF, false, SZ>(a, h, c);
            return;
          }
        }
        BD::template conv<HALF, SZ, SP>(a, h, c);
      });
    }
  }, r.multi_pass, r.half, r.sz, r.sp);
}

// FN<Geo, DT>::run(args...) of the fft size and dtype (ffc::with_geo holds the table); -1: unsupported size
template <template <class, int> class FN, class... A>
static int dispatch(int N, int dtype, A&&... args) {
  int rc = 0;
  const bool found = with_geo(N, [&](auto geo) {
    using GEO = decltype(geo);
    rc = dtype == DT_BF16 ? FN<GEO, DT_BF16>::run(args...) : FN<GEO, DT_F16>::run(args...);
  });
  return found ? rc : -1;
}
template <class GEO, int DT> struct ConvRun { static int run(const ConvArgs& a) { return sim_conv_t<GEO, DT>(a); } };
template <class GEO, int DT> struct ConvResRun { static int run(const ConvArgs& a) { return sim_conv_t<GEO, DT, SimBA>(a); } };
template <class GEO, int DT> struct KfRun {
  static int run(const KfArgs& a) {
    const int nunits = GEO::OUTER ? a.H : (a.H + GEO::G - 1) / GEO::G;
    for (int wg = 0; wg < (nunits + GEO::UPW - 1) / GEO::UPW; wg++)
      run_wg(GEO::WGW, sim_lds<GEO>(), [&]() { Modes<SimB, GEO, DT>::kfft(a, wg); });
    return 0;
  }
};
template <class GEO, int DT> struct KfBiRun {
  static int run(const KfBiArgs& a) {
    const int nunits = GEO::OUTER ? a.H : (a.H + GEO::G - 1) / GEO::G;
    for (int wg = 0; wg < (nunits + GEO::UPW - 1) / GEO::UPW; wg++)
      run_wg(GEO::WGW, sim_lds<GEO>(), [&]() { Modes<SimB, GEO, DT>::kfft(a, wg); });
    return 0;
  }
};
// dkf = true: dkf_kernel / dkf_rp_kernel / dkf_kernel_small; false: bwd_kernel / bwd_rp_kernel / bwd_kernel_small (the library runs the
// saved-spectra form of the fused sizes as its own instantiation, ZM = 1: ffc_k_bwdz.hip)
template <class GEO, int DT, bool DKF>
static int sim_bwd_t(const DkfArgs& d) {
  using MO = Modes<SimBO, GEO, DT>;
  const BwdRoute r = bwd_route<GEO>(d, DKF);
  if (r.err) return NO_KERNEL;
  const int H = d.c.H, nchunk = d.c.nchunk, lds = sim_lds<GEO>();
  if (r.gs) {      // bwd_kernel<.., GS> (BwdLaunchZ)
    if constexpr (GEO::N == 32768) {
      g_gs_count++;
      if (r.pl) g_pl_count++;
      return pick([&](auto zm, auto pl) -> int {
        return sim_jobs(H, nchunk, lds, [&](int h, int c) {
          MO::template bwd<true, false, true, decltype(zm)::value ? 1 : 0, true, decltype(pl)::value>(d, h, c, h * nchunk + c);
        });
      }, d.zin != nullptr, r.pl);
    } else {
      return NO_KERNEL;
    }
  }
  return pick([&](auto mp, auto half, auto fastk, auto zm) -> int {
    constexpr bool MP = decltype(mp)::value, HALF = decltype(half)::value, FASTK = decltype(fastk)::value, ZM = decltype(zm)::value;
    if constexpr (!GEO::OUTER) {       // single-tile kernels: one instantiation, saved spectra decided at run time
      if constexpr (MP || HALF || FASTK || ZM) return NO_KERNEL;
      else if constexpr (DKF) return sim_jobs(H, nchunk, lds, [&](int h, int c) { MO::dkf(d, h, c, h * nchunk + c); });
      else return sim_jobs(H, nchunk, lds, [&](int h, int c) { MO::bwd(d, h, c, h * nchunk + c); });
    } else if constexpr (MP) {
      if constexpr (GEO::N != 32768 || (DKF && (FASTK || ZM))) {
        return NO_KERNEL;
      } else {
        using MK = Modes<typename std::conditional<FASTK, SimBOF, SimBO>::type, GEO, DT>;
        return sim_jobs(H, nchunk, lds, [&](int h, int c) {
          MK::BD::setup_tables(d.c.tab, d.c.t);
          for (int k0 = 0; k0 < d.c.R; k0++) {
            if constexpr (DKF) MK::template dkf<HALF, true>(d, h, c, h * nchunk + c, k0, SimBO::wave());
            else MK::template bwd<HALF, true>(d, h, c, h * nchunk + c, k0, SimBO::wave());
          }
        });
      }
    } else if constexpr (FASTK || (DKF && ZM)) {
      return NO_KERNEL;
    } else if constexpr (DKF) {
      return sim_jobs(H, nchunk, lds, [&](int h, int c) { MO::template dkf<HALF>(d, h, c, h * nchunk + c); });
    } else if constexpr (ZM) {
      return sim_jobs(H, nchunk, lds, [&](int h, int c) { MO::template bwd<HALF, false, true, 1>(d, h, c, h * nchunk + c); });
    } else {
      return sim_jobs(H, nchunk, lds, [&](int h, int c) { MO::template bwd<HALF>(d, h, c, h * nchunk + c); });
    }
  }, r.multi_pass, r.half, r.fastk, !DKF && GEO::OUTER && !r.multi_pass && d.zin != nullptr);
}
template <class GEO, int DT> struct DkfRun { static int run(const DkfArgs& d) { return sim_bwd_t<GEO, DT, true>(d); } };
template <class GEO, int DT> struct BwdRun { static int run(const DkfArgs& d) { return sim_bwd_t<GEO, DT, false>(d); } };
template <class GEO, int DT> struct DkRun {
  static int run(const DkArgs& a) {
    const int nunits = GEO::OUTER ? a.H : (a.H + GEO::G - 1) / GEO::G;
    for (int wg = 0; wg < (nunits + GEO::UPW - 1) / GEO::UPW; wg++)
      run_wg(GEO::WGW, sim_lds<GEO>(), [&]() { Modes<SimB, GEO, DT>::dkifft(a, wg); });
    return 0;
  }
};
template <class GEO, int DT> struct DkBiRun {
  static int run(const DkBiArgs& a) {
    const int nunits = GEO::OUTER ? a.H : (a.H + GEO::G - 1) / GEO::G;
    for (int wg = 0; wg < (nunits + GEO::UPW - 1) / GEO::UPW; wg++)
      run_wg(GEO::WGW, sim_lds<GEO>(), [&]() { Modes<SimB, GEO, DT>::dkifft(a, wg); });
    return 0;
  }
};
template <class GEO, int DT> struct UpwGet { static int run(int* out) { *out = GEO::UPW; return 0; } };

// Body::outer_inv_half<false> alone on one unit of fft 32768: e_in [2 planes][32 rows k1][1024 columns] dtype bits (natural order) is laid
// out in E, the stage runs on the workgroup's 8 waves, e_out [2 planes][16 rows n1][1024 columns] is read back from E
template <int DT>
static void sim_outer_inv_half(const HostPlan& p, const uint16_t* e_in, uint16_t* e_out) {
  using GEO = Geo<32, 32, 32>;
  using BD = Body<SimB, GEO, DT>;
  run_wg(8, GEO::LDS_BYTES, [&]() {
    BD::setup_tables(p.blob.data(), p.tabs);
    typename BD::Unit un;
    un.eb = 0; un.wq = g_wave;
    if (g_wave == 0)
      for (int pl = 0; pl < 2; pl++)
        for (int row = 0; row < 32; row++)
          for (int m = 0; m < 1024; m++)
            memcpy(SimB::L() + pl * GEO::PLANE + e_off<GEO, int>(row, m), &e_in[(pl * 32 + row) * 1024 + m], 2);
    SimB::barrier();
    BD::template outer_inv_half<false>(un);
    SimB::barrier();
    if (g_wave == 0)
      for (int pl = 0; pl < 2; pl++)
        for (int row = 0; row < 16; row++)
          for (int m = 0; m < 1024; m++)
            memcpy(&e_out[(pl * 16 + row) * 1024 + m], SimB::L() + pl * GEO::PLANE + e_off<GEO, int>(row, m), 2);
  });
}
}  // namespace ffc

using namespace ffc;

extern "C" {

void ffcsim_set_tr(int on) { SimB::HAS_TR = on != 0; }
void ffcsim_force_slow_io(int on) { g_force_slow = on != 0; }

// Mirror of ffc_selftest_primitives (ffc_hip.hip selftest_kernel) on the simulator backend.
int ffcsim_selftest_primitives(const uint32_t* in, uint32_t* out) {
  run_wg(1, 1024, [&]() {
    using Bk = SimB;
    Bk::W4 a, b;
    for (int i = 0; i < 4; i++) for (int l = 0; l < 64; l++) { a[i].v[l] = in[l * 8 + i]; b[i].v[l] = in[l * 8 + 4 + i]; }
    Bk::A16 acc = Bk::a16_zero(), acc2 = Bk::a16_zero();
    Bk::mfma<DT_BF16>(acc, a, b);
    Bk::mfma<DT_F16>(acc2, a, b);
    Bk::i32 lane = Bk::lane();
    Bk::U2 w; w.x = a[0]; w.y = a[1];
    Bk::lds_w64(lane * 8, w);
    Bk::U2 t = Bk::lds_r64_tr(((lane * 5 + 3) & 63) * 8);
    Bk::u32 p0 = Bk::pack<DT_BF16>(acc[0], acc[1]), p1 = Bk::pack<DT_F16>(acc[0], acc[1]);
    Bk::f32 u0 = Bk::unpack_lo<DT_F16>(a[2]), u1 = Bk::unpack_hi<DT_F16>(a[2]);
    Bk::f32 u2 = Bk::unpack_lo<DT_BF16>(a[2]), u3 = Bk::unpack_hi<DT_BF16>(a[2]);
    for (int l = 0; l < 64; l++) {
      for (int i = 0; i < 16; i++) { memcpy(&out[l * 40 + i], &acc[i].v[l], 4); memcpy(&out[l * 40 + 16 + i], &acc2[i].v[l], 4); }
      out[l * 40 + 32] = t.x.v[l]; out[l * 40 + 33] = t.y.v[l];
      out[l * 40 + 34] = p0.v[l]; out[l * 40 + 35] = p1.v[l];
      memcpy(&out[l * 40 + 36], &u0.v[l], 4); memcpy(&out[l * 40 + 37], &u1.v[l], 4);
      memcpy(&out[l * 40 + 38], &u2.v[l], 4); memcpy(&out[l * 40 + 39], &u3.v[l], 4);
    }
  });
  return 0;
}

// B::mfma16 alone: a, b [64 lanes][4 dwords] operand registers, d [64 lanes][4] accumulator registers (in: C, out: D)
int ffcsim_mfma16(int dtype, const uint32_t* a, const uint32_t* b, float* d) {
  SimB::W4 wa, wb;
  SimB::A4 acc;
  for (int l = 0; l < 64; l++)
    for (int i = 0; i < 4; i++) { wa[i].v[l] = a[l * 4 + i]; wb[i].v[l] = b[l * 4 + i]; acc[i].v[l] = d[l * 4 + i]; }
  if (dtype == DT_BF16) SimB::mfma16<DT_BF16>(acc, wa, wb);
  else SimB::mfma16<DT_F16>(acc, wa, wb);
  for (int l = 0; l < 64; l++)
    for (int i = 0; i < 4; i++) d[l * 4 + i] = acc[i].v[l];
  return 0;
}

int ffcsim_outer_inv_half(int dtype, const uint16_t* e_in, uint16_t* e_out) {
  HostPlan p;
  if (!build_plan(32768, dtype, &p)) return -1;
  if (dtype == DT_BF16) sim_outer_inv_half<DT_BF16>(p, e_in, e_out);
  else sim_outer_inv_half<DT_F16>(p, e_in, e_out);
  return 0;
}

// Plan introspection (also used by tests to build k_f in internal order on the host).
int ffcsim_plan_info(int N, int dtype, int* nt, double* s_fwd, double* s_k, int32_t* kf_freq /* nt*1024 or null */) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  *nt = p.NT * p.R; *s_fwd = p.s_fwd; *s_k = p.s_k;      // k_f tiles per head (R passes x NT)
  if (kf_freq) memcpy(kf_freq, p.kf_freq.data(), p.kf_freq.size() * 4);
  return 0;
}

// Same contract as ffc_conv_fwd (include/flashfftconv_hip.h) but on host memory.
static int g_sparse_rows = 0;
void ffcsim_set_sparse(int rows) { g_sparse_rows = rows; }      // next ffcsim_conv_fwd calls run the frequency-sparse variant
// spectrum buffer ([H][npair][N] complex dtype pairs) / pre-postgate output of the NEXT ffcsim_conv_fwd (written) and
// ffcsim_conv_bwd (read) calls: the ffc_conv_fwd_z / ffc_conv_bwd_z(y) pair.  Fused single-pass sizes >= 4096.  flags: ConvArgs::flags.
static void* g_z = nullptr; static void* g_yraw = nullptr; static int g_flags = 0;
void ffcsim_set_z(void* z, void* yraw, int flags) { g_z = z; g_yraw = yraw; g_flags = flags; }
long ffcsim_dma_count() { return g_dma_count.exchange(0); }
long ffcsim_gs_count() { return g_gs_count.exchange(0); }
long ffcsim_pl_count() { return g_pl_count.exchange(0); }
void ffcsim_set_flags(int flags) { g_sim_flags = flags; }      // ConvArgs::flags of the next forward / backward calls (256: earlier phase C)
// dk (H, Lk) fp32 written by the NEXT ffcsim_conv_bwd itself (DkfArgs::dk_out, Modes::dk_tail; the caller passes nchunk = 1)
static float* g_dk_out = nullptr; static int g_dk_lk = 0;
void ffcsim_set_fused_dk(float* dk, int Lk) { g_dk_out = dk; g_dk_lk = Lk; }
// k (H, Lk) fp32 transformed by the NEXT ffcsim_conv_fwd itself into its kf argument (ConvArgs::kfuse_k, Modes::kfft_head)
static const float* g_kfuse_k = nullptr; static int g_kfuse_lk = 0;
void ffcsim_set_fused_k(const float* k, int Lk) { g_kfuse_k = k; g_kfuse_lk = Lk; }
// complex forms (HBM-level sizes): k_f rows from a pair-plane tensor (ConvArgs::kfuse_x), dk rows into one (DkfArgs::dk_pair)
static const void* g_kfuse_x = nullptr; static float g_kfuse_xscale = 1.f;
void ffcsim_set_fused_kx(const void* xpair, float scale) { g_kfuse_x = xpair; g_kfuse_xscale = scale; }
static void* g_dk_pair = nullptr; static float g_dk_pair_scale = 1.f;
void ffcsim_set_fused_dkpair(void* outpair, float scale) { g_dk_pair = outpair; g_dk_pair_scale = scale; }
static int g_big_pipe = 0;      // as in the library: opt-in
void ffcsim_set_big_pipe(int on) { g_big_pipe = on; }      // 0: every outer pass through BigBody::run (one block per workgroup)
int ffcsim_conv_fwd(int N, int dtype, const void* u, const void* kf, const void* pregate, const void* postgate,
                    void* y, int B, int H, int L, int conj_kf) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  if (L > N || L <= 0) return -2;
  ConvArgs a{};
  a.u = u; a.pregate = pregate; a.postgate = postgate; a.y = y; a.kf = kf;
  a.tab = p.blob.data(); a.t = p.tabs;
  a.B = B; a.H = H; a.L = L; a.npair = (B + 1) / 2;
  a.sbu = a.sbg = a.sbp = a.sby = (int64_t)H * L;
  a.nchunk = 1; a.ppc = a.npair; a.conj_kf = conj_kf; a.s_inv = (float)p.s_inv; a.s_fwd = (float)p.s_fwd;
  a.fast = (L % 8 == 0) && !g_force_slow;
  a.R = p.R;
  a.flags = g_sim_flags;
  a.sparse = g_sparse_rows;
  if (p.N1 > 1 && p.R == 1) { a.zsave = g_z; a.yraw = g_z ? g_yraw : nullptr; }
  if (p.N1 <= 1) { a.zsave = g_z; a.yraw = g_yraw; }      // single-tile sizes: either one alone too (conv_fwd_impl)
  const bool kfuse = fwd_takes_kfft(p, a.nchunk, a.sparse, 0);      // the library's rule for k -> k_f inside the launch
  if (g_kfuse_x && kfuse) {
    a.kfuse_x = g_kfuse_x; a.kfuse_scale = g_kfuse_xscale; a.kfuse_Lk = N; a.kfuse_fast = 1;
  }
  if (g_kfuse_k && kfuse) {
    a.kfuse_k = g_kfuse_k; a.kfuse_Lk = g_kfuse_lk; a.kfuse_scale = (float)(p.s_k / p.s_fwd) / (dtype == DT_F16 ? 256.f : 1.f); a.kfuse_fast = (g_kfuse_lk % 4 == 0) && !g_force_slow;
  }
  return dispatch<ConvRun>(N, dtype, a);
}

// Same contract as ffc_conv_fwd_res (include/flashfftconv_hip.h) on host memory: the forward with an addend in the output epilogue, batch
// strides in elements (0 = contiguous), optional spectrum buffer / output before gate and addend.  -3: y_raw without a spectrum buffer
// at a size with an outer digit, -4: the addend overlaps y.
int ffcsim_conv_fwd_res(int N, int dtype, const void* u, const void* kf, const void* pregate, const void* postgate, const void* addend,
                        void* y, void* zsave, void* y_raw, int B, int H, int L, int conj_kf, int64_t sb_u, int64_t sb_pre, int64_t sb_post,
                        int64_t sb_add, int64_t sb_y) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  if (L > N || L <= 0 || B <= 0 || H <= 0) return -2;
  if (y_raw && !zsave && p.N1 > 1) return -3;
  const int64_t hl = (int64_t)H * L;
  if (!sb_u) sb_u = hl; if (!sb_pre) sb_pre = hl; if (!sb_post) sb_post = hl; if (!sb_add) sb_add = hl; if (!sb_y) sb_y = hl;
  if (sb_u < hl || sb_pre < hl || sb_post < hl || sb_add < hl || sb_y < hl) return -2;
  if (addend) {
    const uintptr_t a0 = (uintptr_t)addend, a1 = a0 + (uintptr_t)(((B - 1) * sb_add + hl) * 2);
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (uintptr_t)(((B - 1) * sb_y + hl) * 2);
    if (a0 < y1 && y0 < a1) return -4;
  }
  ConvArgs a{};
  a.u = u; a.pregate = pregate; a.postgate = postgate; a.y = y; a.kf = kf; a.addend = addend;
  a.tab = p.blob.data(); a.t = p.tabs;
  a.B = B; a.H = H; a.L = L; a.npair = (B + 1) / 2;
  a.sbu = sb_u; a.sbg = sb_pre; a.sbp = sb_post; a.sby = sb_y; a.sba = sb_add;
  a.nchunk = 1; a.ppc = a.npair; a.conj_kf = conj_kf; a.s_inv = (float)p.s_inv; a.s_fwd = (float)p.s_fwd;
  a.fast = (L % 8 == 0) && !((sb_u | sb_pre | sb_post | sb_y | sb_add) & 7) && !g_force_slow;
  a.R = p.R;
  a.flags = g_sim_flags;
  a.zsave = zsave; a.yraw = y_raw;
  if (!addend) return dispatch<ConvRun>(N, dtype, a);
  return dispatch<ConvResRun>(N, dtype, a);
}



// HBM-level outer pass (ffc_big.h).  fwd: in = long side (Bp_valid rows, Hin, Llong), out = (2*npair, Hin*N0, Mi).
// *_strided: with the batch pitches of the long-side operands (ffc_outer_pass*_strided), on the same kernel body.
// What the level runners fill alike, by the library's rules (ffc_route.h decode_dtype / set_level): -1 bad dtype flags, -4 half rows with
// more than one row per head, -5 no length, -7 long side.  Simulator-side: the contiguous entry points (no pitch given) take any host pointer,
// so there the long side is judged before the pointers are filled in; g_force_slow takes the 16-byte accesses away.
static int sim_level_args(BigArgs* a, int* dtype, int fwd, const void* in, void* out, const void* gate, int Bp_valid, int npair, int Hin, int Mi,
                          int Llong, float scale, int64_t pitch_in, int64_t pitch_out, int64_t pitch_gate) {
  *dtype = decode_dtype(*dtype, fwd, a);
  if (*dtype < 0) return -1;
  if (!half_rows_ok(*a, Bp_valid, npair)) return -4;
  if (Llong <= 0) return -5;
  if (pitch_in || pitch_out || (gate && pitch_gate)) { a->in = in; a->out = out; a->gate = gate; }
  const bool bad = set_level(a, fwd, Bp_valid, npair, Hin, Mi, Llong, scale, pitch_in, pitch_out, pitch_gate) != nullptr;
  a->in = in; a->out = out; a->gate = gate;
  if (bad) return -7;
  if (g_force_slow) a->fast = 0;
  return 0;
}
// R > 1: pass c of a factor R * 32 (ffc_outer_pass_r; tables of the R-pass plan of the fused 32768 kernel)
int ffcsim_big_outer_r_strided(int N0, int R, int c, int dtype, int fwd, const void* in, void* out, const void* gate, int Bp_valid, int npair,
                               int Hin, int Mi, int Llong, float scale, int64_t pitch_in, int64_t pitch_out, int64_t pitch_gate) {
  HostPlan p;
  if (R > 1 && N0 != 32) return -3;
  BigArgs a{};
  a.R = R; a.c = c;
  const int rc = sim_level_args(&a, &dtype, fwd, in, out, gate, Bp_valid, npair, Hin, Mi, Llong, scale, pitch_in, pitch_out, pitch_gate);
  if (!build_plan(R > 1 ? 32768 * R : (N0 == 16 ? 16384 : 32768), dtype, &p)) return -1;   // only for the N0-point operand table
  if (rc) return rc;
  a.fmat = p.blob.data() + (R > 1 ? p.tabs.matk[c][fwd ? 0 : 1] : p.tabs.mat[0]);
  if (Mi % (N0 == 16 ? GeoBig<16>::Mi : GeoBig<32>::Mi)) return -2;
  // the pipelined form where the library's rule allows it and the test asked for it; here 3 "workgroups" walk the blocks so that every
  // one of them runs several iterations
  const bool pipe = level_pipe(a, fwd != 0, g_big_pipe != 0);
  return level_dispatch(N0, dtype == DT_F16, fwd != 0, [&](auto n0, auto dt, auto fw) -> int {
    constexpr int NN = decltype(n0)::value, DD = decltype(dt)::value;
    constexpr bool FF = decltype(fw)::value;
    const int nblk = (int)level_blocks(a, GeoBig<NN>::Mi), npw = pipe ? (nblk < 3 ? nblk : 3) : nblk;
    for (int wg = 0; wg < npw; wg++)
      run_wg(GeoBig<NN>::WGW + (pipe ? 1 : 0), pipe ? BigBody<SimB, NN, DD>::PIPE_LDS : GeoBig<NN>::LDS_BYTES, [&]() {
        if (pipe) BigBody<SimB, NN, DD>::template run_pipe<FF>(a, wg, npw);
        else if (a.strided) BigBody<SimB, NN, DD, true>::template run<FF>(a, wg);
        else BigBody<SimB, NN, DD>::template run<FF>(a, wg);
      });
    return 0;
  });
}
int ffcsim_big_outer_r(int N0, int R, int c, int dtype, int fwd, const void* in, void* out, const void* gate, int Bp_valid, int npair,
                       int Hin, int Mi, int Llong, float scale) {
  return ffcsim_big_outer_r_strided(N0, R, c, dtype, fwd, in, out, gate, Bp_valid, npair, Hin, Mi, Llong, scale, 0, 0, 0);
}
int ffcsim_big_outer(int N0, int dtype, int fwd, const void* in, void* out, const void* gate, int Bp_valid, int npair,
                     int Hin, int Mi, int Llong, float scale) {
  return ffcsim_big_outer_r(N0, 1, 0, dtype, fwd, in, out, gate, Bp_valid, npair, Hin, Mi, Llong, scale);
}
int ffcsim_big_outer_strided(int N0, int dtype, int fwd, const void* in, void* out, const void* gate, int Bp_valid, int npair,
                             int Hin, int Mi, int Llong, float scale, int64_t pitch_in, int64_t pitch_out, int64_t pitch_gate) {
  return ffcsim_big_outer_r_strided(N0, 1, 0, dtype, fwd, in, out, gate, Bp_valid, npair, Hin, Mi, Llong, scale, pitch_in, pitch_out, pitch_gate);
}

// all R passes in one workgroup run (ffc_outer_pass_all, BigBody::run_all; the wide form BigBody::run_wide beyond the first 32 rows)
int ffcsim_big_outer_all_strided(int R, int dtype, int fwd, const void* in, void* out, const void* gate, int Bp_valid, int npair,
                                 int Hin, int Mi, int Llong, float scale, int64_t pitch_in, int64_t pitch_out, int64_t pitch_gate) {
  HostPlan p;
  BigArgs a{};
  a.R = R; a.c = 0;
  const int rc = sim_level_args(&a, &dtype, fwd, in, out, gate, Bp_valid, npair, Hin, Mi, Llong, scale, pitch_in, pitch_out, pitch_gate);
  if (R < 2 || R > 4 || !build_plan(32768 * R, dtype, &p)) return -1;
  if (rc) return rc;
  for (int c = 0; c < R; c++) a.fmats[c] = p.blob.data() + p.tabs.matk[c][fwd ? 0 : 1];
  a.fmat = a.fmats[0];
  if (Mi % GeoBig<32>::Mi) return -2;
  if (Llong > R * 32 * Mi) return -5;
  if (level_wide(a)) {
    BigArgs w = a;
    w.strided = 0;
    if (level_wide_check(w)) return -6;
    if (pitch_in || pitch_out || pitch_gate) return -7;      // contiguous long side only, as in the library
    a.wide = 1;
  }
  return level_dispatch(32, dtype == DT_F16, fwd != 0, [&](auto n0, auto dt, auto fw) -> int {
    constexpr int DD = decltype(dt)::value;
    constexpr bool FF = decltype(fw)::value;
    if constexpr (decltype(n0)::value != 32) return -3;
    const int nblk = (int)level_blocks(a, a.wide ? level_wide_cols(a.R) : GeoBig<32>::Mi);
    for (int wg = 0; wg < nblk; wg++)
      run_wg(GeoBig<32>::WGW, GeoBig<32>::LDS_BYTES, [&]() {
        if (a.wide) BigBody<SimB, 32, DD>::template run_wide<FF>(a, wg);
        else if (a.strided) BigBody<SimB, 32, DD, true>::template run_all<FF>(a, wg);
        else BigBody<SimB, 32, DD>::template run_all<FF>(a, wg);
      });
    return 0;
  });
}
int ffcsim_big_outer_all(int R, int dtype, int fwd, const void* in, void* out, const void* gate, int Bp_valid, int npair,
                         int Hin, int Mi, int Llong, float scale) {
  return ffcsim_big_outer_all_strided(R, dtype, fwd, in, out, gate, Bp_valid, npair, Hin, Mi, Llong, scale, 0, 0, 0);
}

int ffcsim_upw(int N) { int u = 0; dispatch<UpwGet>(N, 0, &u); return u; }

// The launch rules of ffc_route.h for one call, as ints (tests/test_launch_rules.py holds them against hand-written values).
// flags: the library's tuning flags (FFC_FLAGS: 32, 64, 128) | 1 << 16: a spectrum buffer is given | 1 << 17: y_raw is given
// | 1 << 18: frequency-sparse k_f | 1 << 19: the rows take 16-byte accesses (ConvArgs::fast).
// out[0..7]   forward            {multi_pass, half, sz, sp, grid, lds_max, lds, no kernel}
// out[8..15]  fused backward     {multi_pass, half, fastk, small, grid, lds_max, lds, no kernel}
// out[16..23] dk_f accumulation  (as the backward)
// out[24] k -> k_f inside the forward launch; out[25] / out[26] dk out of the backward launch as real dk / as complex rows (DK_*)
int ffcsim_launch_route(int N, int dtype, int B, int H, int L, int nchunk, int persist, int flags, int* out) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  static char buf[16];
  DkfArgs d{};
  ConvArgs& a = d.c;
  a.B = B; a.H = H; a.L = L; a.npair = (B + 1) / 2; a.nchunk = nchunk; a.persist = persist; a.R = p.R;
  a.zsave = (flags & (1 << 16)) ? buf : nullptr; a.yraw = (flags & (1 << 17)) ? buf : nullptr;
  a.sparse = (flags & (1 << 18)) ? 2 : 0; a.fast = (flags & (1 << 19)) ? 1 : 0;
  with_geo(N, [&](auto geo) {
    using GEO = decltype(geo);
    const FwdRoute f = fwd_route<GEO>(a);
    const int fo[8] = {f.multi_pass, f.half, f.sz, f.sp, f.grid, f.lds_max, f.lds, f.err != nullptr};
    memcpy(out, fo, sizeof fo);
    for (int dkf = 0; dkf < 2; dkf++) {
      const BwdRoute b = bwd_route<GEO>(d, dkf != 0);
      const int bo[8] = {b.multi_pass, b.half, b.fastk, b.small, b.grid, b.lds_max, b.lds, b.err != nullptr};
      memcpy(out + 8 + 8 * dkf, bo, sizeof bo);
    }
  });
  out[24] = fwd_takes_kfft(p, nchunk, a.sparse, flags & 0xffff);
  out[25] = bwd_dk_form(p, nchunk, flags & 0xffff, false);
  out[26] = bwd_dk_form(p, nchunk, flags & 0xffff, true);
  return 0;
}

// Which sink phase C takes (ffc::direct_store_ok through fwd_route / bwd_route): out[0] forward, out[1] fused backward, out[2] dk_f
// accumulation; 1 = the output rows are stored by phase C itself.  flags as ffcsim_launch_route | 1 << 20: an output gate (forward) / an
// input gate (backward) | 1 << 21: an addend (forward) / a dpregate output (backward).
int ffcsim_launch_sink(int N, int dtype, int B, int H, int L, int flags, int* out) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  static char buf[16];
  DkfArgs d{};
  ConvArgs& a = d.c;
  a.B = B; a.H = H; a.L = L; a.npair = (B + 1) / 2; a.nchunk = 1; a.R = p.R; a.flags = flags & 0xffff;
  a.zsave = (flags & (1 << 16)) ? buf : nullptr; a.yraw = (flags & (1 << 17)) ? buf : nullptr;
  a.sparse = (flags & (1 << 18)) ? 2 : 0; a.fast = (flags & (1 << 19)) ? 1 : 0;
  with_geo(N, [&](auto geo) {
    using GEO = decltype(geo);
    ConvArgs f = a;
    f.postgate = (flags & (1 << 20)) ? buf : nullptr; f.addend = (flags & (1 << 21)) ? buf : nullptr;
    out[0] = fwd_route<GEO>(f).gs;
    a.pregate = (flags & (1 << 20)) ? buf : nullptr; d.dpre = (flags & (1 << 21)) ? buf : nullptr;
    out[1] = bwd_route<GEO>(d, false).gs;
    out[2] = bwd_route<GEO>(d, true).gs;
  });
  return 0;
}

// Which direct-store calls also take their input rows plain (ffc::plain_rows_ok through fwd_route / bwd_route): out[0] forward, out[1] fused
// backward.  flags as ffcsim_launch_route | 1 << 20: an input gate | 1 << 21: the forward's / backward's dpost side product (aux_in / y_raw)
// | 1 << 22: a dpost output without y_raw (backward).
int ffcsim_launch_plain(int N, int dtype, int B, int H, int L, int flags, int* out) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  static char buf[16];
  DkfArgs d{};
  ConvArgs& a = d.c;
  a.B = B; a.H = H; a.L = L; a.npair = (B + 1) / 2; a.nchunk = 1; a.R = p.R; a.flags = flags & 0xffff;
  a.zsave = (flags & (1 << 16)) ? buf : nullptr;
  a.fast = (flags & (1 << 19)) ? 1 : 0;
  with_geo(N, [&](auto geo) {
    using GEO = decltype(geo);
    ConvArgs f = a;
    f.pregate = (flags & (1 << 20)) ? buf : nullptr; f.aux_in = (flags & (1 << 21)) ? buf : nullptr;
    out[0] = fwd_route<GEO>(f).pl;
    a.postgate = (flags & (1 << 20)) ? buf : nullptr;
    d.zin = a.zsave; a.zsave = nullptr;
    if (flags & (3 << 21)) d.dpost = buf;
    d.yraw = (flags & (1 << 21)) ? buf : nullptr;
    out[1] = bwd_route<GEO>(d, false).pl;
  });
  return 0;
}

int ffcsim_kernel_fft_c(int N, int dtype, const void* xpair, int H, void* kf, float scale) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  KfArgs a{};
  a.xpair = xpair; a.kf = kf; a.tab = p.blob.data(); a.t = p.tabs; a.H = H; a.Lk = N; a.scale = scale; a.prescale = 1.f; a.s_fwd = (float)p.s_fwd; a.fast = 1;
  a.R = p.R;
  return dispatch<KfRun>(N, dtype, a);
}

int ffcsim_kernel_fft(int N, int dtype, const float* k, int H, int Lk, void* kf) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  KfArgs a{};
  a.k = k; a.kf = kf; a.tab = p.blob.data(); a.t = p.tabs; a.H = H; a.Lk = Lk;
  a.s_fwd = (float)p.s_fwd;
  a.prescale = dtype == DT_F16 ? 256.f : 1.f;
  a.scale = (float)(p.s_k / p.s_fwd) / a.prescale; a.fast = (Lk % 4 == 0) && !g_force_slow;
  a.R = p.R;
  return dispatch<KfRun>(N, dtype, a);
}

// two-tensor form (ffc_kernel_fft_bi): k (H, Lk) and k_rev (H, Lr)
int ffcsim_kernel_fft_bi(int N, int dtype, const float* k, int Lk, const float* k_rev, int Lr, int H, void* kf) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  if (!k || !k_rev || Lk <= 0 || Lk > N || Lr <= 0 || Lr > N) return -1;
  KfBiArgs a{};
  a.k = k; a.kr = k_rev; a.kf = kf; a.tab = p.blob.data(); a.t = p.tabs; a.H = H; a.Lk = Lk; a.Lr = Lr;
  a.s_fwd = (float)p.s_fwd;
  a.prescale = dtype == DT_F16 ? 256.f : 1.f;
  a.scale = (float)(p.s_k / p.s_fwd) / a.prescale; a.fast = (Lk % 4 == 0) && (Lr % 4 == 0) && !g_force_slow;
  a.R = p.R;
  return dispatch<KfBiRun>(N, dtype, a);
}

// ws must hold nchunk*UPW*H*NT*2048 floats
int ffcsim_conv_bwd_dkf(int N, int dtype, const void* dout, const void* u, const void* pregate, const void* postgate,
                        float* ws, int B, int H, int L, int nchunk) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  DkfArgs d{};
  ConvArgs& a = d.c;
  a.u = u; a.pregate = pregate; a.postgate = postgate; a.tab = p.blob.data(); a.t = p.tabs;
  a.B = B; a.H = H; a.L = L; a.npair = (B + 1) / 2; a.s_fwd = (float)p.s_fwd;
  a.sbu = a.sbg = a.sbp = a.sby = (int64_t)H * L; d.sbd = d.sbdu = d.sbdpre = d.sbdpost = (int64_t)H * L;
  int upw = ffcsim_upw(N);
  int per_iter = p.N1 > 1 ? upw : upw * p.G;
  int iters_total = (a.npair + per_iter - 1) / per_iter;
  if (nchunk > iters_total) nchunk = iters_total;
  int ipc = (iters_total + nchunk - 1) / nchunk;
  a.ppc = ipc * per_iter; a.nchunk = (a.npair + a.ppc - 1) / a.ppc;
  a.fast = (L % 8 == 0) && !g_force_slow;
  a.R = p.R;
  d.dout = dout; d.ws = ws;
  std::vector<uint8_t> zs((size_t)H * a.nchunk * upw * N * 4 + 16);
  d.zscratch = zs.data();
  int rc = dispatch<DkfRun>(N, dtype, d);
  return rc < 0 ? rc : a.nchunk;   // number of slabs written (one per chunk)
}

// fused backward: du (and dpre if non-null) + dk_f slabs; returns the number of slabs
int ffcsim_conv_bwd(int N, int dtype, const void* dout, const void* u, const void* kf, const void* pregate, const void* postgate,
                    void* du, void* dpre, void* dpost, float* ws, int B, int H, int L, int nchunk) {
  HostPlan p;
  if (!build_plan(N, dtype, &p)) return -1;
  DkfArgs d{};
  ConvArgs& a = d.c;
  a.u = u; a.kf = kf; a.pregate = pregate; a.postgate = postgate; a.tab = p.blob.data(); a.t = p.tabs;
  a.B = B; a.H = H; a.L = L; a.npair = (B + 1) / 2; a.s_inv = (float)p.s_inv; a.s_fwd = (float)p.s_fwd;
  a.sbu = a.sbg = a.sbp = a.sby = (int64_t)H * L; d.sbd = d.sbdu = d.sbdpre = d.sbdpost = (int64_t)H * L;
  int upw = ffcsim_upw(N);
  int per_iter = p.N1 > 1 ? upw : upw * p.G;
  int iters_total = (a.npair + per_iter - 1) / per_iter;
  if (nchunk > iters_total) nchunk = iters_total;
  int ipc = (iters_total + nchunk - 1) / nchunk;
  a.ppc = ipc * per_iter; a.nchunk = (a.npair + a.ppc - 1) / a.ppc;
  a.fast = (L % 8 == 0) && !g_force_slow;
  a.R = p.R;
  d.dout = dout; d.ws = ws; d.du = du; d.dpre = dpre; d.dpost = (p.N1 > 1 || g_yraw) ? dpost : nullptr;
  a.flags = g_sim_flags;
  if (p.N1 > 1 && p.R == 1 && g_z) { d.zin = g_z; d.yraw = g_yraw; a.flags = g_flags | g_sim_flags; a.stream = 1; }
  if (p.N1 <= 1) { d.zin = g_z; d.yraw = dpost ? g_yraw : nullptr; }      // (conv_bwd_impl: y_raw with or without the spectra)
  HostPlan pbf;
  // the library's rule for dk out of the backward launch, with fft 8192 asked for as tuning flag 128 does
  if (g_dk_pair && bwd_dk_form(p, a.nchunk, 128, true) != DK_SEPARATE) {
    if (!build_plan(N, DT_BF16, &pbf)) return -1;
    set_dk_tail(&d, nullptr, g_dk_pair, N, g_dk_pair_scale, 1, pbf.blob.data(), pbf.tabs);
  } else if (g_dk_out && bwd_dk_form(p, a.nchunk, 128, false) != DK_SEPARATE) {
    if (!build_plan(N, DT_BF16, &pbf)) return -1;
    set_dk_tail(&d, g_dk_out, nullptr, g_dk_lk, (float)(1.0 / p.s_fwd), (g_dk_lk % 4 == 0) && !g_force_slow, pbf.blob.data(), pbf.tabs);
  }
  std::vector<uint8_t> zs((size_t)H * a.nchunk * upw * N * 4 + 16);
  d.zscratch = zs.data();
  int rc = dispatch<BwdRun>(N, dtype, d);
  return rc < 0 ? rc : a.nchunk;
}

int ffcsim_kernel_ifft_grad_c(int N, const float* ws, int nslab, int H, void* outpair, float scale) {
  HostPlan p;
  if (!build_plan(N, DT_BF16, &p)) return -1;
  DkArgs a{};
  a.ws = ws; a.outpair = outpair; a.tab = p.blob.data(); a.t = p.tabs; a.H = H; a.Lk = N; a.nslab = nslab; a.scale = scale; a.s_inv = (float)p.s_inv; a.fast = 1;
  a.R = p.R;
  return dispatch<DkRun>(N, DT_BF16, a);
}

int ffcsim_kernel_ifft_grad(int N, int dtype, const float* ws, int nslab, int H, int Lk, float* dk) {
  HostPlan p;
  (void)dtype;                      // the dk inverse always runs in bf16 arithmetic (see ffc_k_dk.hip)
  dtype = DT_BF16;
  if (!build_plan(N, dtype, &p)) return -1;
  DkArgs a{};
  a.ws = ws; a.dk = dk; a.tab = p.blob.data(); a.t = p.tabs; a.H = H; a.Lk = Lk; a.nslab = nslab;
  a.scale = (float)(1.0 / p.s_fwd); a.s_inv = (float)p.s_inv;   // tile_inv applies s_inv = 1/(N s_fwd)
  a.fast = (Lk % 4 == 0) && !g_force_slow;
  a.R = p.R;
  return dispatch<DkRun>(N, dtype, a);
}

// two-tensor form (ffc_kernel_ifft_grad_bi): dk (H, Lk) and dk_rev (H, Lr) from one inverse
int ffcsim_kernel_ifft_grad_bi(int N, int dtype, const float* ws, int nslab, int H, int Lk, float* dk, int Lr, float* dk_rev) {
  HostPlan p;
  (void)dtype;                      // bf16 arithmetic, as ffcsim_kernel_ifft_grad
  dtype = DT_BF16;
  if (!build_plan(N, dtype, &p)) return -1;
  if (!dk || !dk_rev || Lk <= 0 || Lk > N || Lr <= 0 || Lr > N) return -1;
  DkBiArgs a{};
  a.ws = ws; a.dk = dk; a.dkr = dk_rev; a.tab = p.blob.data(); a.t = p.tabs; a.H = H; a.Lk = Lk; a.Lr = Lr; a.nslab = nslab;
  a.scale = (float)(1.0 / p.s_fwd); a.s_inv = (float)p.s_inv;
  a.fast = (Lk % 4 == 0) && (Lr % 4 == 0) && !g_force_slow;
  a.R = p.R;
  return dispatch<DkBiRun>(N, dtype, a);
}

}  // extern "C"
