// Windowed self-attention (HyperTile) for gfx950, head_dim 64, q prescaled: mx_attention_window.
//
// A sample's L = gh x gw tokens are a row-major grid cut into (gh / wh) x (gw / ww) windows; token (y, x) attends to the wh ww tokens of its own
// window.  The window's tokens are NOT gathered: the kernel reads q / k rows and V^T columns where the QKV epilogue left them and writes o rows in the
// same order.  Window-local token t is row (wy wh + t / ww) gw + wx ww + t % ww of the sample.  ww % 16 == 0, so
//   * a window row starts on a 16-key group of MX_VT_POS: the permutation inside the group is the same in window-local and in sample order, and a
//     16-byte V^T chunk (8 positions) or a run of 16 keys never straddles a window row;
//   * a tile of 64 window-local keys is 64 K rows and, per feature row, 8 V^T chunks, each at a per-thread 32-bit byte offset from a wave-uniform
//     (sample, head, window) base.  A thread keeps the (row, column) of the keys it stages and advances them by one tile with two compares: the
//     loop holds no division and no 64-bit vector arithmetic.
// The LDS image of a tile, the fragment reads, S^T = K Q^T with the reference k-step, the lazy-reference softmax and O^T += V^T P^T are the pieces of
// attn_tile.h (the arithmetic of attn_fwd_kernel<true>); the work split and the staging are this kernel's.
//
// RESIDENT form (wh ww <= MX_WIN_RESIDENT_MAX = 256 keys: the 16 x 16 windows of both SDXL levels at a 128-pixel tile): one workgroup owns one
// (sample, head, window).  It stages the window's whole K / V^T image -- up to four tiles of 16 KB, 64 KB: two workgroups a CU -- once, passes ONE
// barrier, and its four waves then walk the window's 32-query blocks against the resident keys: no double buffer, no barrier per tile, and K / V^T
// are fetched once per window rather than once per 128 query rows.
// STREAMED form (more keys: the 32 x 32 windows of a 256-pixel tile, 32 x 48 ...): one workgroup owns a 128-row query block of a window and walks the
// window's keys in 64-key tiles through two LDS buffers, the next tile in registers while the current one computes (attn_fwd_kernel's pipeline).
// Both: a ragged last key tile (wh ww % 64 in {16, 32, 48}: whole 16-key groups, so a V^T chunk is all there or all padding) is zero-filled in LDS
// and its scores masked; query rows past the window's end are clamped on the load and not stored.
// Workgroups: the query blocks of one (sample, head, window) are consecutive on one XCD when the number of such units is a multiple of 8 (attn_locate's deal).
#include <algorithm>

#include "common.h"
#include "../../include/mxdenoise.h"
#include "attn_tile.h"

#ifndef MX_WIN_RESIDENT_MAX
#define MX_WIN_RESIDENT_MAX 256                // keys; 0 builds a library whose streamed form serves every window (tools/hypertile_bench.py times the two)
#endif

namespace mx {

struct WinArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* vt; bf16_t* o;
  int ldq, ldk, ldvt, ldo;
  long vt_bstride;
  int B, H, L, gw, wh, ww, nwx, nwin;          // nwx windows across, nwin = windows a sample
  int nk;                                      // wh ww: keys = queries of a window
  int tile_dy, tile_dx;                        // 64 keys on: KT / ww window rows and KT % ww columns
  int nqb;                                     // workgroups a window (streamed: 128-row query blocks; resident: 1)
  int xcd_map;
};

// sample row of window-local token t of the window whose first token is row `w0`
__device__ __forceinline__ int win_row(const WinArgs& p, const int w0, const int t) { return w0 + (t / p.ww) * p.gw + t % p.ww; }

// The staging state of one thread: which 16-byte chunks of a 64-key tile it fetches (two K rows, srow and srow + 32, at head chunk sch; V^T feature rows
// srow and srow + 32 at key chunk sch) and where the current tile's lie.  (ky, kx) / (vy, vx): window row and column of the thread's K rows / of its V^T
// chunk's first key.  next() moves all of them 64 keys on.
struct WinStage {
  const WinArgs& p;
  const char* kbase; const char* vbase;        // wave-uniform: the window's first K row at the head's slice / first V^T position of the head's feature row 0
  int ky[2], kx[2], vy, vx;
  unsigned vrow[2];                            // byte offset of the thread's two V^T feature rows, + its chunk of the K row in kcol
  unsigned kcol;
  int key0;                                    // first key of the tile (ky, kx, vy, vx) stand at
  unsigned st_off;                             // byte offset of the thread's first K chunk inside a tile image (swizzled)
  u32x4 rk[2], rv[2];

  __device__ __forceinline__ WinStage(const WinArgs& p_, const int b, const int head, const int w0, const int tid) : p(p_) {
    const int srow = tid >> 3, sch = tid & 7;
    kbase = (const char*)(p.k + ((long)b * p.L + w0) * p.ldk + head * 64);
    vbase = (const char*)(p.vt + (long)b * p.vt_bstride + ((long)head * 64) * p.ldvt + w0);
    kcol = (unsigned)(sch * 16);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = srow + 32 * i;
      ky[i] = t / p.ww; kx[i] = t % p.ww;
      vrow[i] = (unsigned)((srow + 32 * i) * p.ldvt * 2);
    }
    vy = (8 * sch) / p.ww; vx = (8 * sch) % p.ww;
    key0 = 0;
    st_off = (unsigned)(srow * 128 + ((sch ^ ((srow >> 1) & 7)) * 16));
  }
  // the tile at key0 into registers; keys >= nk (ragged last tile) are zeros: 0 * garbage must not be NaN
  __device__ __forceinline__ void load() {
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const int srow = (int)(st_off >> 7);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool kin = key0 + srow + 32 * i < p.nk;
      rk[i] = kin ? *reinterpret_cast<const u32x4*>(kbase + (unsigned)((ky[i] * p.gw + kx[i]) * p.ldk * 2) + kcol) : zero4;
    }
    const bool vin = key0 + (int)(kcol >> 1) < p.nk;   // chunk sch = positions 8 sch .. + 7 of the tile: one half of a 16-key group
    const unsigned voff = (unsigned)((vy * p.gw + vx) * 2);
#pragma unroll
    for (int i = 0; i < 2; ++i) rv[i] = vin ? *reinterpret_cast<const u32x4*>(vbase + vrow[i] + voff) : zero4;
  }
  __device__ __forceinline__ void next() {
    key0 += KT;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      kx[i] += p.tile_dx; ky[i] += p.tile_dy;
      if (kx[i] >= p.ww) { kx[i] -= p.ww; ++ky[i]; }
    }
    vx += p.tile_dx; vy += p.tile_dy;
    if (vx >= p.ww) { vx -= p.ww; ++vy; }
  }
  __device__ __forceinline__ void store(char* img) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u32x4*>(img + st_off + i * 4096) = rk[i];
      *reinterpret_cast<u32x4*>(img + st_off + 8192 + i * 4096) = rv[i];
    }
  }
};

// the lane's part of window-local queries q0 .. q0 + 31 (past the window's end: its last): load_q's fragment through the window's row map
__device__ __forceinline__ void win_load_q(const WinArgs& p, const int b, const int head, const int w0, const int q0, const int lane, bf16x8 (&qf)[4]) {
  const int r = lane & 31, hh = lane >> 5;
  int qi = q0 + r;
  if (qi > p.nk - 1) qi = p.nk - 1;
  const bf16_t* qp = p.q + ((long)b * p.L + win_row(p, w0, qi)) * p.ldq + head * 64 + hh * 8;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
}
// store_o through the window's row map: 8-byte pieces (ldo % 4 == 0), lane (r, hh) holds d = 32 db + 8 g + 4 hh + {0..3} of query qi
__device__ __forceinline__ void win_store_o(const WinArgs& p, const int b, const int head, const int w0, const int qi, const int hh, const float l_run,
                                            const f32x16 (&oacc)[2]) {
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_tot;
  if (qi < p.nk) {
    bf16_t* op = p.o + ((long)b * p.L + win_row(p, w0, qi)) * p.ldo + head * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * hh;
        const u32x2 o = {pack2(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv), pack2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv)};
        *reinterpret_cast<u32x2*>(op + d) = o;
      }
  }
}

// One 32-query block's running state and its step over one staged tile (the body of attn_fwd_kernel<true>'s loop)
struct WinBlock {
  f32x16 oacc[2];
  float l_run = 0.f, m_ref = 0.f;
  u32x4 qm = {0u, 0u, 0u, 0u};
  __device__ __forceinline__ WinBlock() {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    oacc[0] = zero16; oacc[1] = zero16;
  }
  // tile image at `img` (K then V^T, attn_tile.h's layout); valid: keys of the tile that exist (64 unless it is the ragged last one)
  __device__ __forceinline__ void tile(const char* img, const unsigned (&koff)[4], const bf16x8 (&qf)[4], const bf16x8 kone, const int hh, const bool first,
                                       const int valid) {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bf16x8 fr[8];
    read_k(fr, img, koff);
    __builtin_amdgcn_sched_barrier(0);
    f32x16 s[2];
    qk(s, fr, qf, zero16);
    ref_step(s, kone, qm);
    read_v(fr, img, koff);                     // V^T fragments (same registers): in flight while the softmax runs
    __builtin_amdgcn_sched_barrier(0);
    if (valid < KT) {                          // (wave-uniform) ragged last tile: its missing keys never count
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh >= valid) s[kb][e] = -INFINITY;
    }
    const float mx_ = col_max(s);
    if (first || __any(mx_ > 8.0f))
      move_reference(s, mx_, first, m_ref, l_run, oacc, [&](float m) __attribute__((always_inline)) { qm[0] = ref_step_word(m, hh); });
    l_run += exp_sum(s);
    pv(oacc, s, fr);
  }
};

// workgroup -> (query block of the window, unit = (b H + head) nwin + window)
__device__ __forceinline__ void win_locate(const WinArgs& p, int& qb, int& unit) {
  const int lin = blockIdx.x;
  if (p.xcd_map) {
    const int local = lin >> 3;
    qb = local % p.nqb;
    unit = ((local / p.nqb) << 3) + (lin & 7);
  } else {
    qb = lin % p.nqb;
    unit = lin / p.nqb;
  }
}
// unit -> sample, head, first row of the window
__device__ __forceinline__ void win_unit(const WinArgs& p, const int unit, int& b, int& head, int& w0) {
  const int win = unit % p.nwin, bh = unit / p.nwin;
  head = bh % p.H;
  b = bh / p.H;
  w0 = (win / p.nwx) * p.wh * p.gw + (win % p.nwx) * p.ww;
}

#if MX_WIN_RESIDENT_MAX > 0
constexpr int WIN_RES_TILES = MX_WIN_RESIDENT_MAX / KT;
__global__ __launch_bounds__(256, 2) void attn_window_resident_kernel(const WinArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[WIN_RES_TILES * kBufBytes];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  int qb, unit, b, head, w0;
  win_locate(p, qb, unit);
  win_unit(p, unit, b, head, w0);
  const int ntiles = (p.nk + KT - 1) / KT;     // <= WIN_RES_TILES (launcher)

  // the whole window: every tile's loads are issued before the first store waits for them
  WinStage st(p, b, head, w0, tid);
  u32x4 hk[WIN_RES_TILES][2], hv[WIN_RES_TILES][2];
#pragma unroll
  for (int kt = 0; kt < WIN_RES_TILES; ++kt) {
    if (kt < ntiles) {
      st.load();
      st.next();
#pragma unroll
      for (int i = 0; i < 2; ++i) { hk[kt][i] = st.rk[i]; hv[kt][i] = st.rv[i]; }
    }
  }
  bf16x8 qf[4], qn[4];
  win_load_q(p, b, head, w0, wave * 32, lane, qf);
#pragma unroll
  for (int kt = 0; kt < WIN_RES_TILES; ++kt) {
    if (kt < ntiles) {
#pragma unroll
      for (int i = 0; i < 2; ++i) { st.rk[i] = hk[kt][i]; st.rv[i] = hv[kt][i]; }
      st.store(smem + kt * kBufBytes);
    }
  }
  __syncthreads();                             // the kernel's only barrier

  unsigned koff[4];
  frag_offsets(r, hh, koff);
  const bf16x8 kone = ref_step_ones(hh);
  const int last_valid = p.nk - (ntiles - 1) * KT;
  // the window's 32-query blocks, dealt round-robin to the four waves; the next block's Q rows travel while this one computes
  for (int q0 = wave * 32; q0 < p.nk; q0 += 128) {
    const bool more = q0 + 128 < p.nk;
    if (more) win_load_q(p, b, head, w0, q0 + 128, lane, qn);
    WinBlock blk;
    for (int kt = 0; kt < ntiles; ++kt) blk.tile(smem + kt * kBufBytes, koff, qf, kone, hh, kt == 0, kt + 1 < ntiles ? KT : last_valid);
    win_store_o(p, b, head, w0, q0 + r, hh, blk.l_run, blk.oacc);
    if (more) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
    }
  }
}
#endif

__global__ __launch_bounds__(256, 2) void attn_window_streamed_kernel(const WinArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kBufBytes];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  int qb, unit, b, head, w0;
  win_locate(p, qb, unit);
  win_unit(p, unit, b, head, w0);
  const int q0 = qb * 128 + wave * 32;         // (a wave whose rows all lie past the window's end still stages and keeps the barriers)

  bf16x8 qf[4];
  win_load_q(p, b, head, w0, q0, lane, qf);
  WinStage st(p, b, head, w0, tid);
  unsigned koff[4];
  frag_offsets(r, hh, koff);
  const bf16x8 kone = ref_step_ones(hh);
  const int ntiles = (p.nk + KT - 1) / KT;
  const int last_valid = p.nk - (ntiles - 1) * KT;

  st.load();
  st.next();
  st.store(smem);
  __syncthreads();
  WinBlock blk;
  unsigned bofs = 0;                           // the buffer of the tile being computed
  for (int kt = 0; kt < ntiles; ++kt) {
    const bool has_next = kt + 1 < ntiles;
    if (has_next) { st.load(); st.next(); }
    blk.tile(smem + bofs, koff, qf, kone, hh, kt == 0, has_next ? KT : last_valid);
    bofs ^= kBufBytes;
    if (has_next) st.store(smem + bofs);
    __syncthreads();
  }
  win_store_o(p, b, head, w0, q0 + r, hh, blk.l_run, blk.oacc);
}

}  // namespace mx

extern "C" int mx_attention_window(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, int64_t vt_batch_stride, void* o,
                                   int ldo, int B, int H, int gh, int gw, int wh, int ww) {
  using namespace mx;
  MX_CHECK(q && k && vt && o, "attention_window: null operand");
  MX_CHECK(B > 0 && H > 0 && gh > 0 && gw > 0 && wh > 0 && ww > 0, "attention_window: empty problem");
  MX_CHECK((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)o) & 15) == 0, "attention_window: operand pointers must be 16-byte aligned");
  MX_CHECK(gh % wh == 0 && gw % ww == 0, "attention_window: the window must divide the token grid (gh % wh == 0 and gw % ww == 0)");
  MX_CHECK(ww % 16 == 0, "attention_window: the window width must be a multiple of 16 (MX_VT_POS permutes keys inside groups of 16)");
  MX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0, "attention_window: ldq, ldk, ldvt must be multiples of 8 elements and ldo of 4");
  MX_CHECK(ldq >= H * 64 && ldk >= H * 64 && ldo >= H * 64, "attention_window: row stride smaller than H*64");
  const long L = (long)gh * gw;
  MX_CHECK(ldvt >= MX_VT_LD(L), "attention_window: ldvt must cover MX_VT_LD(gh*gw) (keys are stored in MX_VT_POS order)");
  MX_CHECK(vt_batch_stride % 8 == 0 && vt_batch_stride >= (int64_t)H * 64 * ldvt, "attention_window: bad vt_batch_stride");
  // the per-thread staging offsets are 32-bit byte offsets inside one sample's K rows / one head's V^T rows
  MX_CHECK(L * ldk * 2 < 2147483647L && 64L * ldvt * 2 < 2147483647L && (long)B * L < 2147483647L, "attention_window: sample too large for 32-bit staging offsets");
  WinArgs a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.vt = (const bf16_t*)vt; a.o = (bf16_t*)o;
  a.ldq = ldq; a.ldk = ldk; a.ldvt = ldvt; a.ldo = ldo; a.vt_bstride = (long)vt_batch_stride;
  a.B = B; a.H = H; a.L = (int)L; a.gw = gw; a.wh = wh; a.ww = ww; a.nwx = gw / ww; a.nwin = (gh / wh) * a.nwx;
  a.nk = wh * ww;
  a.tile_dy = KT / ww; a.tile_dx = KT % ww;
  const bool resident = a.nk <= MX_WIN_RESIDENT_MAX;
  a.nqb = resident ? 1 : cdiv(a.nk, 128);
  const long units = (long)B * H * a.nwin;
  a.xcd_map = units % 8 == 0 ? 1 : 0;
  const long blocks = units * a.nqb;
  MX_CHECK(blocks < 2147483647L, "attention_window: too many workgroups");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  prof_begin(st, PROF_ATTN, 4.0 * B * H * (double)L * a.nk * 64.0, 2.0 * B * H * 64.0 * 4.0 * (double)L, B * H, (int)L, a.nk);
#if MX_WIN_RESIDENT_MAX > 0
  if (resident) hipLaunchKernelGGL(attn_window_resident_kernel, grid, block, 0, st, a);
  else
#endif
    hipLaunchKernelGGL(attn_window_streamed_kernel, grid, block, 0, st, a);
  prof_end(st);
  MX_LAUNCH_CHECK();
  return 0;
}
