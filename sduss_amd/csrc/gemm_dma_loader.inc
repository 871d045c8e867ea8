// The operand loader of one BM x BN output tile (BM = 64 * MI rows of X, BN rows of W, K tiles of DMA_BK) for a 512-thread workgroup: the single
// definition behind gemm_v2_kernel (gemm_bf16_v2.hip) and gemm_v5_tile (gemm_bf16_v5.hip).  A FRAGMENT, included inside the kernel body, not a
// header: see gemm_dma_loader.h for why, and for the primitives it uses.
//
// in scope at the point of inclusion:
//   BN, MI, CONV             the kernel's template parameters
//   const GemmArgs p         the tile's problem (after gemm_select_seg)
//   int tm, tn               the output tile
//   constexpr bool SPLIT_K   the kernel has split-K: the stream may start at a K tile other than 0
//   int k_first, nk          the K tiles the stream covers: [k_first, k_first + nk) (SPLIT_K: a slice; otherwise 0, K / DMA_BK)
//   bf16_t* smem             the LDS ring, stages of DmaTile<BN, MI>::STAGE_ELEMS
//   int tid, lane, wave      threadIdx.x, tid & 63, tid >> 6 (wave-uniform: readfirstlane)
// defined here -- the interface:
//   setup_tile()             per-thread sources of K tile k_first
//   issue_group(stage)       issue the DMA group at the cursor into ring stage `stage`; branch-free
//   advance_cursor()         move the cursor to the next K tile: all of the loader's control flow
// (and the cursor state and conv_set_tap / park_on_zero_page behind them, which the kernels do not touch)
//
// issue_group() is branch-free so that it can share a basic block with the MFMAs (the scheduler can then place each LDS-DMA in an MFMA shadow);
// everything with control flow -- moving to the next K tile or conv tap, into the second A source, or off the end of the stream -- happens in
// advance_cursor(), which the caller runs after the MFMAs.  A DMA group can be issued in EVERY iteration: past the end of the stream it reads the
// zero page (into a stage nobody reads), so one counted wait serves every iteration.  CONV: per-row source pointers are recomputed only when the
// tap changes (every Cin / 64 K tiles) and otherwise just advance by one K tile; out-of-image taps and rows beyond M read the zero page
// instead of branching.
  constexpr int BM = DmaTile<BN, MI>::BM, WCH = DmaTile<BN, MI>::WCH, XI = DmaTile<BN, MI>::XI, WI = DmaTile<BN, MI>::WI, STAGE_ELEMS = DmaTile<BN, MI>::STAGE_ELEMS;
  const char* zero = reinterpret_cast<const char*>(g_zero_page);
  const int cs = tid & 7;
  const int tiles_per_tap = CONV ? p.Cin / DMA_BK : 1;

  // ---- the cursor: the K tile the NEXT DMA group belongs to, and ready-made per-thread source pointers for it ----
  bool parked = false;          // the cursor ran past the end of the stream
  int is_kt = 0;
  const char* xsrc[XI];         // source of the thread's X chunks for the next group
  long xjump[XI];               // split A operand: extra byte step of the thread's X chunks when K reaches k_split (into the second source)
  const char* wsrc[WI];
  int cb[XI], cy[XI], cx[XI];   // CONV: image, y, x of the row's output pixel (input coordinates of the centre tap)
  unsigned xchb[XI];            // CONV: byte offset of the thread's swizzled chunk inside a K tile
  int tap_next = 0, in_tap = 0;

  // CONV: (re)compute the row pointers for tap `tap` at channel byte offset `cbyte`
  auto conv_set_tap = [&](int tap, int cbyte = 0) __attribute__((always_inline)) {
    const int dy = tap / 3 - 1;
    const int dx = tap - (tap / 3) * 3 - 1;
    const int Hv = p.Hin << p.up, Wv = p.Win << p.up;
    const int P = p.corner_patch;
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      int iy = cy[i] + dy;
      const int ix = cx[i] + dx;
      if (P > 0 && dy != 0 && dx != 0) {
        // halo-corner rule of the reference's sliced path (norm_silu_concat.cu:210-221, 228-239)
        const bool cross_r = ((iy + P) / P) != ((cy[i] + P) / P);
        const bool cross_c = ((ix + P) / P) != ((cx[i] + P) / P);
        if (cross_r && cross_c) iy = cy[i];
      }
      const bool ok = (cb[i] >= 0) && (iy >= -p.vhalo) && (iy < Hv + p.vhalo) && (ix >= 0) && (ix < Wv);
      const long off = ((((long)cb[i] * (p.Hin + 2 * p.vhalo) + (iy >> p.up) + p.vhalo) * p.Win + (ix >> p.up)) * p.Cin) * 2;
      xsrc[i] = (ok ? reinterpret_cast<const char*>(p.a) + off + cbyte : zero) + xchb[i];
    }
  };

  // per-thread sources of K tile k_first of tile (tm, tn)
  auto setup_tile = [&]() __attribute__((always_inline)) {
    const int m0 = tm * BM;
    const int n0 = tn * BN;
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int row = (i * 512 + tid) >> 3;
      const int ch = swz(row, cs);           // logical k-chunk this thread fetches for its slot
      const int m = m0 + row;
      if constexpr (!CONV) {
        const int mc = m < p.M ? m : p.M - 1; // clamped rows are computed and discarded by the epilogue mask
        xsrc[i] = reinterpret_cast<const char*>(p.a) + (gemm_in_row(p, mc) * p.lda + ch * 8) * 2;
        xjump[i] = p.a2 != nullptr ? (reinterpret_cast<const char*>(p.a2) + ((long)mc * p.lda2 + ch * 8) * 2) - (xsrc[i] + (long)p.k_split * 2) : 0;
      } else {
        xchb[i] = ch * 16;
        if (m < p.M) {
          const int hw = p.Hout * p.Wout;
          const int b = m / hw;
          const int r = m - b * hw;
          const int oy = r / p.Wout;
          cb[i] = b; cy[i] = oy * p.stride; cx[i] = (r - oy * p.Wout) * p.stride;
        } else {
          cb[i] = -1; cy[i] = 0; cx[i] = 0;
        }
      }
    }
    // (split-K: this workgroup's K range starts at K tile k_first -- tap k_first / tiles_per_tap, channel tile k_first % tiles_per_tap)
    if constexpr (SPLIT_K) { tap_next = CONV ? k_first / tiles_per_tap : 0; in_tap = CONV ? k_first - tap_next * tiles_per_tap : 0; }
    if constexpr (CONV) conv_set_tap(tap_next, in_tap * DMA_BK * 2);
    else if constexpr (SPLIT_K) {
#pragma unroll
      for (int i = 0; i < XI; ++i) xsrc[i] += (long)k_first * DMA_BK * 2;
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      int q = i * 512 + tid;
      if (q >= WCH) q -= WCH;                 // BN=160: the last instruction re-fetches rows 0..31 (same bytes, same slot)
      const int row = q >> 3;
      wsrc[i] = reinterpret_cast<const char*>(p.w) + ((long)(n0 + row) * p.K + (long)k_first * DMA_BK + swz(row, cs) * 8) * 2;
    }
  };
  auto park_on_zero_page = [&]() __attribute__((always_inline)) {            // past the end of the stream: same instruction count, harmless bytes
#pragma unroll
    for (int i = 0; i < XI; ++i) xsrc[i] = zero + lane * 16;
#pragma unroll
    for (int i = 0; i < WI; ++i) wsrc[i] = zero + lane * 16;
  };

  // issue the DMA group at the cursor into ring stage `stage` (no control flow)
  auto issue_group = [&](int stage) __attribute__((always_inline)) {
    bf16_t* st = smem + stage * STAGE_ELEMS;
    bf16_t* sw = st + BM * DMA_BK;
#pragma unroll
    for (int i = 0; i < XI; ++i) glds16(xsrc[i], st + (i * 512 + wave * 64) * 8);
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int qb = (i * 512 + wave * 64 >= WCH) ? i * 512 + wave * 64 - WCH : i * 512 + wave * 64;  // wave-uniform slot base
      glds16(wsrc[i], sw + qb * 8);
    }
  };
  // move the cursor (and the source pointers) to the next K tile of the stream
  auto advance_cursor = [&]() __attribute__((always_inline)) {
    if (parked) return;
    if (++is_kt == nk) {                      // the end of the stream: the rest of the ring slots get harmless bytes
      is_kt = 0;
      parked = true;
      park_on_zero_page();
      return;
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) wsrc[i] += DMA_BK * 2;
    if constexpr (!CONV) {
      // at K = k_split the A operand continues in its second source (gemm_args.h): one more byte step, selected without a branch
      // (the branchy form of this switch was miscompiled once the epilogue grew: the prologue's second advance lost its increment)
      const bool to_a2 = p.a2 != nullptr && is_kt * DMA_BK == p.k_split;
#pragma unroll
      for (int i = 0; i < XI; ++i) xsrc[i] += DMA_BK * 2 + (to_a2 ? xjump[i] : 0L);
    } else {
      if (++in_tap == tiles_per_tap) {
        in_tap = 0;
        conv_set_tap(++tap_next);
      } else {
#pragma unroll
        for (int i = 0; i < XI; ++i) xsrc[i] += DMA_BK * 2;
      }
    }
  };
