// Tables and launchers of the patch-unit block cache (patch_cache.hip; used by unet_sdxl.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mxdenoise.h"

namespace mx {
// level-0 description of a sample of the batch: first row of its image in the concatenated level-0 activations, latent size, its row of the state
// tensors (one per request), patches per image row.  At level l: image (h >> l) x (w >> l), first row row0 >> 2l, patch edge p0 >> l.
// The tables are the public ones of include/mxdenoise.h (the one-launch entry points take them as they are).
using PcSample = mx_pc_sample;   // { long long row0; int h, w, slot, npx; }
using PcPatch = mx_pc_patch;     // { int b, py, px, pad; }
using PcRange = mx_pc_range;     // { long long row0; int rows, slot, srow0; }: rows [row0, row0 + rows) of a batch tensor <-> rows [srow0, ...) of state row `slot`

int launch_pc_image_copy(hipStream_t st, void* batch, void* state, const void* samp, int B, int level, int C, long state_row_elems, int to_batch,
                         const float* vec, int ldvec, const void* residual, long max_image_elems, int gate = 0);
int launch_pc_rows_load_stats(hipStream_t st, void* batch, const void* state, const void* samp, int B, int level, int C, long state_row_elems, const void* residual,
                              float* stats1, float* fin, float eps, long max_image_rows);
int launch_pc_range_copy(hipStream_t st, void* batch, void* state, long state_row_elems, int C, const void* ranges, int n, int to_batch, long max_range_elems);
int launch_pc_range_sq_diff(hipStream_t st, const void* x, const void* state, long state_row_elems, int C, const void* ranges, int n, double* partial);
int launch_pc_gather(hipStream_t st, const void* src, int ld_src, int C, void* dst, const void* list, int n, const void* samp, int level, int p, int halo_lo,
                     int halo_hi, int up);
int launch_pc_scatter(hipStream_t st, const void* src, int Ps, int o0, int C, void* state, long state_row_elems, const void* list, int n, const void* samp,
                      int level, int p);
int launch_pc_patch_store(hipStream_t st, const void* batch, void* state, long state_row_elems, int C, const void* list, int n, const void* samp, int level, int p);
int launch_pc_patch_sq_diff(hipStream_t st, const void* x, const void* state, long state_row_elems, int C, const void* list, int n, const void* samp, int level,
                            int p, double* partial);
// The block's decision on the device (pc_decide_kernel; the rule is skip_decide.h): ONE workgroup walks the units in row order in chunks of its
// own size, finalises their features, walks the forest, applies the counter rule and compacts the asking units in order (see mx_skip_decide_args).
int launch_pc_decide(hipStream_t st, const mx_skip_decide_args& a);

// What follows the counters in mx_block_cache.dev_counters: the tables and outputs of the kernel.  record | flags are adjacent: one copy reads both.
struct SkipScratch {
  int32_t *counters, *sample_group, *unit_sample, *record;
  unsigned char *flags, *valid;
  static size_t counter_elems(int n_blocks, int n_slots, int ups) { return (size_t)n_blocks * n_slots * ups; }
  static size_t record_ints(int n_slots) { return (size_t)MX_SKIP_REC_FIRST + n_slots + 1; }
  static size_t bytes(int n_blocks, int n_slots, int ups) {
    const size_t ints = counter_elems(n_blocks, n_slots, ups) + n_slots + (size_t)n_slots * ups + record_ints(n_slots);
    return (ints * sizeof(int32_t) + (size_t)n_slots * ups + n_slots + 255) & ~(size_t)255;
  }
  SkipScratch() : counters(nullptr), sample_group(nullptr), unit_sample(nullptr), record(nullptr), flags(nullptr), valid(nullptr) {}
  SkipScratch(int32_t* base, int n_blocks, int n_slots, int ups) {
    counters = base; sample_group = counters + counter_elems(n_blocks, n_slots, ups); unit_sample = sample_group + n_slots;
    record = unit_sample + (size_t)n_slots * ups; flags = (unsigned char*)(record + record_ints(n_slots)); valid = flags + (size_t)n_slots * ups;
  }
};

// a pinned host buffer that lives with a model handle (the read-back of the device decision)
struct PinnedBuf {
  void* p = nullptr; size_t n = 0;
  void* get(size_t bytes) {
    if (bytes <= n) return p;
    if (p) (void)hipHostFree(p);
    p = nullptr; n = 0;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { p = nullptr; return nullptr; }
    n = bytes;
    return p;
  }
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
};
}  // namespace mx
