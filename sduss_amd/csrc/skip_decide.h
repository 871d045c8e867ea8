// The block-skip decision, stated ONCE for the host and the device (include/mxdenoise.h: mx_skip_decide_host, mx_skip_decide_device; the kernel
// is patch_cache.hip pc_decide_kernel).  It restates, operation for operation, what the host path of the patch / chunk unit computes:
//   - the feature of a unit: the fp64 sum of its partial sums IN ORDER, divided by the element count, rounded to fp32
//     (unet_sdxl.cpp run_block_pc; mmdit_sd3.cpp, the chunk decision);
//   - the feature row [block index, timestep of the unit's sample, mse of each input (oldest skip first)] in fp32;
//   - the forest walk of mx_forest_predict (capi.cpp): left when (double)x[f] <= threshold, leaves marked by left < 0, acc += p1[leaf] in tree
//     order, answer acc / n_trees > 0.5;
//   - the counter rule of PatchSkipCache._predict + decide() (sduss_amd/block_cache.py; cache_manager.py:128-136, 150-156).
// Nothing here may be contracted or reassociated: every function switches contraction off, and the sums are written as loops in source order.
#pragma once
#include <stdint.h>
#include "../../include/mxdenoise.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MX_SKIP_HD __host__ __device__
#else
#define MX_SKIP_HD
#endif

namespace mx {

// mse of one input of one unit: `count` partial sums, `elems` = the elements they cover
MX_SKIP_HD inline float skip_finalise(const double* part, int count, double elems) {
#pragma clang fp contract(off)
  double t = 0.0;
  for (int r = 0; r < count; ++r) t += part[r];
  return (float)(t / elems);
}

// "nothing cached for this unit": what PatchSkipCache._predict reads off the first input's feature (the marker, or anything as large)
MX_SKIP_HD inline bool skip_uncached(float mse0) { return (double)mse0 >= (double)MX_MSE_UNCACHED * 0.5; }

// mx_forest_predict for one row: 0 / 1, or -1 when the tables point outside themselves (mx_forest_predict reports that as an error; a walk
// longer than the forest has nodes is a cycle)
MX_SKIP_HD inline int skip_forest_row(const mx_device_forest& f, const float* x) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int t = 0; t < f.n_trees; ++t) {
    int node = f.roots[t];
    if (node < 0 || node >= f.n_nodes) return -1;
    int steps = 0;
    while (f.left[node] >= 0) {
      const int ft = f.feature[node];
      if (ft < 0 || ft >= f.n_feat || ++steps > f.n_nodes) return -1;
      node = (double)x[ft] <= f.threshold[node] ? f.left[node] : f.right[node];
      if (node < 0 || node >= f.n_nodes) return -1;
    }
    acc += f.p1[node];
  }
  return acc / f.n_trees > 0.5 ? 1 : 0;
}

// the counter rule: returns run, leaves the unit's new counter
MX_SKIP_HD inline int skip_rule(int raw, bool uncached, int counter, int forced_after, int32_t* new_counter) {
  const int prev = uncached ? 0 : counter;                 // "0 if not in the cache else previous"
  const bool forced = prev == forced_after;
  const bool run = raw != 0 || forced || uncached;
  *new_counter = (uncached || run) ? 0 : prev + 1;
  return run ? 1 : 0;
}

// one unit, from its finalised features x[2 ..] (x[0], x[1] filled by the caller): run flag; *bad is set when the forest is malformed
MX_SKIP_HD inline int skip_unit(const mx_device_forest& f, const float* x, int counter, int forced_after, int32_t* new_counter, int* bad) {
  const bool uncached = skip_uncached(x[2]);
  int raw = 1;                                             // an uncached unit runs whatever the forest says: its walk is not needed
  if (!uncached) {
    raw = skip_forest_row(f, x);
    if (raw < 0) { *bad = 1; raw = 1; }
  }
  return skip_rule(raw, uncached, counter, forced_after, new_counter);
}

}  // namespace mx
