// The host scaffold every step plan stands on (unet_sdxl.cpp, mmdit_sd3.cpp, vae_sdxl.cpp, clip_text.cpp, t5_text.cpp).  Host only: nothing
// here launches a kernel of its own, and all of it is reached by the dry sizing walks (tests/asan_walk.cpp).
//   * Arena        -- the stack allocator over the caller's workspace; a dry arena hands out placeholder addresses and only counts;
//   * WeightTable  -- blob + name -> (offset, bytes) of a handle, filled by mx_*_set_weights, read through one checked lookup;
//   * PlanBase     -- what every Plan is made of: stream, arena, the dry / lookup / mute switches, the first error, w / wb / wf, alloc<T>,
//                     the gemm / conv wrapper and the stage dump of the trace entry points.  Copyable (the recording walk copies a plan);
//   * Groups       -- the resolution groups of a forward (one unless the batch is mixed);
//   * DenoiserPlan -- PlanBase + Groups + the patch-parallel exchange + the per-sample block-cache bookkeeping shared by the cached entry
//                     points of the two denoisers (which samples hold state, the slot table, the timesteps, rows in / out of the state, the
//                     comparison partial sums read back as per-row MSEs);
//   * ForwardCall  -- one forward of a denoiser as named fields, and run_forward, the driver both denoisers share: generic checks -> the
//                     model's checks -> plan set-up -> recording walk of a stale patch-parallel layout -> eager run or hipGraph replay.
//                     Plain, mixed, trace, patch-parallel and block-skip-cached forwards and every sizing walk go through it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mxdenoise.h"
#include "common.h"
#include "graph_cache.h"
#include "patch_cache.h"
#include "pp_exchange.h"

namespace mx {
int launch_copy_rows(hipStream_t s, void* batch, void* slotted, size_t bytes_per_sample, int B, const int* slot, int scatter);

struct Arena {
  char* base = nullptr; size_t cap = 0; size_t top = 0; size_t peak = 0; bool dry = false;
  void reset(void* b, size_t c, bool d) { base = (char*)b; cap = c; top = 0; peak = 0; dry = d; }
  void* alloc(size_t bytes) {
    const size_t a = (top + 255) & ~(size_t)255;
    top = a + bytes;
    if (top > peak) peak = top;
    if (dry) return (void*)(uintptr_t)(0x1000 + a);  // never dereferenced on the host
    return (top <= cap) ? base + a : nullptr;
  }
  size_t mark() const { return top; }
  void release(size_t m) { top = m; }
};

struct WeightTable {
  const char* blob = nullptr;
  uint64_t blob_bytes = 0;
  std::unordered_map<std::string, std::pair<uint64_t, uint64_t>> table;
  // mx_*_set_weights after the handle has dropped what depended on the old table; `who` prefixes the messages
  int set(const char* who, const void* b, uint64_t bytes, const mx_weight_entry* entries, int n) {
    const std::string p = std::string(who) + ": ";
    MX_CHECK(b && entries && n > 0, p + "bad arguments");
    table.clear();
    for (int i = 0; i < n; ++i) {
      MX_CHECK(entries[i].name != nullptr, p + "null name");
      MX_CHECK(entries[i].offset % 16 == 0, p + "tensor offsets must be 16-byte aligned");
      MX_CHECK(entries[i].offset + entries[i].bytes <= bytes, p + "entry exceeds blob");
      table[entries[i].name] = {entries[i].offset, entries[i].bytes};
    }
    blob = (const char*)b; blob_bytes = bytes;
    return 0;
  }
  // the tensor `name` of exactly `bytes` bytes; nullptr with `err` filled otherwise
  const void* find(const std::string& name, size_t bytes, std::string& err) const {
    auto it = table.find(name);
    if (it == table.end()) { err = "missing weight '" + name + "'"; return nullptr; }
    if (it->second.second != bytes) { err = "weight '" + name + "' has " + std::to_string(it->second.second) + " bytes, expected " + std::to_string(bytes); return nullptr; }
    return blob + it->second.first;
  }
};

struct PlanBase {
  const WeightTable* weights = nullptr;
  hipStream_t stream = nullptr;
  Arena ar;
  bool dry = false;         // size-only pass: no launches
  bool lookup = false;      // dry pass that still resolves every weight (mx_*_validate)
  bool mute = false;        // block-skip cache: walk a block's plan (allocations, cursors) without launching it
  std::string err;          // the first failure
  const char* stage = nullptr; void* stage_out = nullptr; size_t stage_bytes = 0; bool stage_hit = false;   // mx_*_forward_trace

  void begin(const WeightTable& wt, hipStream_t s, void* workspace, size_t workspace_bytes) { weights = &wt; stream = s; dry = false; ar.reset(workspace, workspace_bytes, false); }
  void begin_dry(const WeightTable& wt) { weights = &wt; dry = true; ar.reset(nullptr, 0, true); }
  bool ok() const { return err.empty(); }
  bool fail(const std::string& m) { if (err.empty()) err = m; return false; }
  bool quiet() const { return dry || mute; }

  const void* w(const std::string& name, size_t bytes) {
    if (dry && !lookup) return (const void*)(uintptr_t)0x1000;
    std::string e;
    const void* p = weights->find(name, bytes, e);
    if (!p) fail(e);
    return p;
  }
  const bf16_t* wb(const std::string& name, size_t elems) { return (const bf16_t*)w(name, elems * 2); }
  const float* wf(const std::string& name, size_t elems) { return (const float*)w(name, elems * 4); }
  template <typename T> T* alloc(size_t elems) {
    T* p = (T*)ar.alloc(elems * sizeof(T));
    if (!p) fail("workspace too small");
    return p;
  }
  bool gemm(mx_gemm_desc& d, bool conv = false) {
    if (!ok()) return false;
    if (quiet()) return true;
    if (conv ? mx_conv3x3(stream, &d) : mx_gemm(stream, &d)) return fail(std::string("gemm/conv: ") + mx_last_error());
    return true;
  }
  // the trace entry points: copy the tensor the caller named out of the running plan
  void dump(const std::string& name, const bf16_t* t, size_t elems) {
    if (!stage || quiet() || !ok() || stage_hit) return;
    if (name != stage) return;
    if (elems * 2 > stage_bytes) { fail("stage buffer too small for '" + name + "'"); return; }
    if (hipMemcpyAsync(stage_out, t, elems * 2, hipMemcpyDeviceToDevice, stream) != hipSuccess) fail("stage copy failed");
    stage_hit = true;
  }
  // the end of a run_impl / sizing walk: the peak, the error
  int finish(bool okr, size_t* peak) {
    if (peak) *peak = ar.peak;
    if (!okr) { set_error(err); return 1; }
    return 0;
  }
};

// A group = the samples of one resolution; B = samples of ALL groups; H, W = the first group's latent size (the only one unless mixed)
struct Groups {
  int ng = 1, B = 0, H = 0, W = 0;
  int gB[MX_MAX_SEGS], gH[MX_MAX_SEGS], gW[MX_MAX_SEGS], gb0[MX_MAX_SEGS];   // per group: samples, latent size, first sample
  const void* g_lat[MX_MAX_SEGS]; void* g_out[MX_MAX_SEGS];
  void set_single(int batch, int h, int w, const void* lat, void* out) { const mx_unet_group g{lat, out, batch, h, w}; set_groups(&g, 1); }
  void set_groups(const mx_unet_group* groups, int n) {     // n in 1..MX_MAX_SEGS: the caller has checked
    ng = n; B = 0; H = groups[0].H; W = groups[0].W;
    for (int g = 0; g < n; ++g) {
      gB[g] = groups[g].batch; gH[g] = groups[g].H; gW[g] = groups[g].W; gb0[g] = B; g_lat[g] = groups[g].latents; g_out[g] = groups[g].out;
      B += groups[g].batch;
    }
  }
  std::vector<int> group_of() const {     // per sample: its group
    std::vector<int> of(B);
    for (int g = 0; g < ng; ++g) for (int k = 0; k < gB[g]; ++k) of[gb0[g] + k] = g;
    return of;
  }
};

struct DenoiserPlan : PlanBase, Groups {
  PPExchange px;                  // the exchange itself, synchronous / warm-up / stale (pp_exchange.h)
  // ---- per-sample block-cache bookkeeping (mx_*_forward_cached, mx_*_forward_cached_mixed; mx_block_cache in include/mxdenoise.h) ----
  mx_block_cache* bc = nullptr;
  int bc_rows = 0;                // samples a state tensor holds: the batch, or bc->n_slots when the caller keeps one slot per request
  const int* bc_dslot = nullptr;  // device copy of bc->slots (null: sample i lives in row i)
  std::vector<unsigned char> bc_valid;   // per sample: the state holds its tensors of an earlier step
  bool bc_all_valid = false, bc_any_valid = false;
  bool bc_keyed = false;          // the per-sample forms: the cache remembers (batch_key, batch, H, W) of the step its state belongs to
  std::vector<float> h_timesteps; // host copy of the timesteps for the predictor
  // head of the state: `part_rows` rows of comparison partial sums (64 doubles per sample), then `tables` int tables (the slot table first)
  static size_t bc_head_bytes(int part_rows, int tables, int rows) {
    return (((size_t)part_rows * rows * 64 * sizeof(double) + (size_t)tables * rows * sizeof(int)) + 255) & ~(size_t)255;
  }
  int* bc_table(int part_rows, int k) const { return (int*)((char*)bc->state + (size_t)part_rows * bc_rows * 64 * sizeof(double)) + (size_t)k * bc_rows; }

  void bc_fold() {
    bc_all_valid = true; bc_any_valid = false;
    for (unsigned char v : bc_valid) { bc_all_valid = bc_all_valid && v; bc_any_valid = bc_any_valid || v; }
  }
  // one state row per request (the reference's dictionaries are keyed by request id, cache_manager.py:105-133): the caller says where each
  // sample lives and whether that row holds tensors of an earlier step at this latent size
  int bc_begin_slots(const std::string& who, mx_block_cache* cache, int batch) {
    bc = cache;
    MX_CHECK(cache->slots && cache->slot_valid && cache->n_slots >= batch, who + ": slots need slot_valid and n_slots >= batch");
    bc_valid.assign(batch, 0);
    std::vector<char> seen(cache->n_slots, 0);
    for (int b = 0; b < batch; ++b) {
      MX_CHECK(cache->slots[b] >= 0 && cache->slots[b] < cache->n_slots && !seen[cache->slots[b]], who + ": slots must be distinct and inside [0, n_slots)");
      seen[cache->slots[b]] = 1;
      bc_valid[b] = cache->slot_valid[b] ? 1 : 0;
    }
    bc_fold();
    return 0;
  }
  // the per-sample forms: slots as above, or the whole batch in rows 0 .. batch-1, valid while (batch_key, batch, H, W) repeat
  int bc_begin(const std::string& who, mx_block_cache* cache, int batch, int h, int w) {
    bc_keyed = true;
    bc_rows = cache->slots ? cache->n_slots : batch;
    if (cache->slots) return bc_begin_slots(who, cache, batch);
    bc = cache;
    cache->cached_valid = cache->cached_valid && cache->cached_key == cache->batch_key && cache->cached_batch == batch && cache->cached_h == h && cache->cached_w == w;
    bc_valid.assign(batch, cache->cached_valid ? 1 : 0);
    bc_fold();
    return 0;
  }
  // the slot table into the head of the state (behind `part_rows` rows of partial sums)
  int bc_send_slots(const std::string& who, int part_rows, int tables, int batch) {
    if (!bc->slots) return 0;
    MX_CHECK(bc_head_bytes(part_rows, tables, bc_rows) <= bc->state_bytes, who + ": state buffer too small");
    int* dslot = bc_table(part_rows, 0);
    MX_CHECK(hipMemcpyAsync(dslot, bc->slots, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, stream) == hipSuccess, who + ": sending the slot table failed");
    bc_dslot = dslot;
    return 0;
  }
  // the predictor's timestep feature: the per-sample timesteps live in device memory like the rest of the step's operands.  Synchronises the
  // stream, so whatever tables the caller has queued on it have arrived as well.
  int bc_read_timesteps(const std::string& who, const float* timesteps, int batch) {
    h_timesteps.resize(batch);
    if (hipMemcpyAsync(h_timesteps.data(), timesteps, (size_t)batch * sizeof(float), hipMemcpyDeviceToHost, stream) == hipSuccess &&
        hipStreamSynchronize(stream) == hipSuccess) return 0;
    if (bc_keyed) bc->cached_valid = 0;
    set_error(who + ": reading the timesteps failed");
    return 1;
  }
  // Partial sums -> host MSE: reads back `n` rows of `len` doubles from the device buffer `part`, synchronises, and folds each row in index
  // order -- a plain left-to-right double sum: skip_decide.h and the device decision are bit-compared with it -- into
  // mse[at] = float(sum / elems).  where(r) = {sample, elems, at} of row r; a row whose sample holds no state is skipped, so its entry
  // keeps what the caller put there (MX_MSE_UNCACHED).  `msg`: the caller's error text.
  struct MseRow { int sample; double elems; size_t at; };
  template <class Where> bool bc_read_mse(const double* part, size_t n, int len, float* mse, const char* msg, Where where) {
    std::vector<double> hp(n * len);
    if (hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) return fail(msg);
    for (size_t r = 0; r < n; ++r) {
      const MseRow w = where(r);
      if (!bc_valid[w.sample]) continue;
      double t = 0.0;
      for (int k = 0; k < len; ++k) t += hp[r * len + k];
      mse[w.at] = (float)(t / w.elems);
    }
    return true;
  }
  // ---- the decision on the device (mx_block_cache.dev_down; the patch / chunk unit: mx_*_forward_cached_mixed) ----
  // The host keeps what sizes the following launches: per block it reads back ONE record (n_ask, first[], the group counts; the flags when
  // somebody wants them) instead of every partial sum, and calls nobody.
  bool bc_dev = false;
  SkipScratch bc_skip;
  int bc_dev_ups = 0;                        // units of a slot's max_h x max_w grid
  const float* bc_dev_ts = nullptr;          // the caller's device timesteps
  std::vector<int> bc_dev_unit_b, bc_dev_group;   // host: sample of each unit, group of each sample
  int32_t* bc_dev_rec = nullptr;             // pinned, owned by the model handle: the record, then the flags
  size_t bc_dev_dec = 0;                     // flags written to bc->decisions_out so far
  // what can be refused before anything is launched: n_in_down / n_in_up = inputs of the blocks dev_down / dev_up decide (0: no such block)
  static int bc_dev_check(const std::string& who, const mx_block_cache* cache, int n_blocks, int ups, int n_in_down, int n_in_up) {
    if (!cache->dev_down) return 0;
    MX_CHECK(cache->observe == nullptr, who + ": observe is a host callback and must be NULL with a device forest (dev_down)");
    const mx_device_forest* up = cache->dev_up ? cache->dev_up : cache->dev_down;
    MX_CHECK(n_in_down <= MX_SKIP_MAX_IN && n_in_up <= MX_SKIP_MAX_IN, who + ": a block has more inputs than MX_SKIP_MAX_IN");
    MX_CHECK(cache->dev_down->n_feat == 2 + n_in_down,
             who + ": dev_down has n_feat " + std::to_string(cache->dev_down->n_feat) + ", its blocks need " + std::to_string(2 + n_in_down));
    MX_CHECK(n_in_up == 0 || up->n_feat == 2 + n_in_up, who + ": dev_up has n_feat " + std::to_string(up->n_feat) + ", its blocks need " + std::to_string(2 + n_in_up));
    MX_CHECK(cache->forced_after >= 0, who + ": forced_after must not be negative");
    MX_CHECK(cache->dev_counters && ((uintptr_t)cache->dev_counters & 7) == 0 && cache->dev_counters_bytes >= SkipScratch::bytes(n_blocks, cache->n_slots, ups),
             who + ": dev_counters too small (mx_skip_counters_bytes)");
    return 0;
  }
  // carve the scratch behind the counters and send this forward's tables; `unit_b`: the sample of every unit in row order
  int bc_dev_begin(const std::string& who, PinnedBuf& pin, int n_blocks, int ups, const float* timesteps, std::vector<int> unit_b, std::vector<int> group_of,
                   bool send_unit_b) {
    bc_dev = bc->dev_down != nullptr;
    if (!bc_dev) return 0;
    bc_skip = SkipScratch(bc->dev_counters, n_blocks, bc->n_slots, ups);
    bc_dev_ups = ups; bc_dev_ts = timesteps; bc_dev_unit_b = std::move(unit_b); bc_dev_group = std::move(group_of); bc_dev_dec = 0;
    MX_CHECK((int)bc_dev_unit_b.size() <= bc->n_slots * ups && (int)bc_dev_group.size() == B, who + ": more units than the counters hold");
    bc_dev_rec = (int32_t*)pin.get(SkipScratch::record_ints(bc->n_slots) * sizeof(int32_t) + (size_t)bc->n_slots * ups);
    MX_CHECK(bc_dev_rec != nullptr, who + ": no pinned memory for the decision record");
    MX_CHECK(hipMemcpyAsync(bc_skip.valid, bc_valid.data(), (size_t)B, hipMemcpyHostToDevice, stream) == hipSuccess &&
             hipMemcpyAsync(bc_skip.sample_group, bc_dev_group.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream) == hipSuccess &&
             (!send_unit_b || hipMemcpyAsync(bc_skip.unit_sample, bc_dev_unit_b.data(), bc_dev_unit_b.size() * sizeof(int), hipMemcpyHostToDevice, stream) == hipSuccess),
             who + ": sending the decision's tables failed");
    return 0;
  }
  // One block: the caller has filled the unit tables, the partial sums and the forest of `a`.  Returns the record (MX_SKIP_REC_*), the flags behind
  // it in *flags -- read back from the device, or, when no sample holds state (every unit runs; the kernel only zeroes their counters), written
  // here without any synchronisation.
  const int32_t* bc_dev_decide(mx_skip_decide_args& a, int block, bool want_flags, const unsigned char** flags) {
    const int n = (int)bc_dev_unit_b.size();
    a.block = block; a.forced_after = bc->forced_after; a.n = n; a.n_samples = B;
    a.counters = bc_skip.counters + (size_t)block * bc->n_slots * bc_dev_ups; a.units_per_slot = bc_dev_ups; a.n_counters = bc->n_slots * bc_dev_ups;
    a.sample_valid = bc_skip.valid; a.sample_group = bc_skip.sample_group; a.timesteps = bc_dev_ts; a.run = bc_skip.flags; a.record = bc_skip.record;
    if (launch_pc_decide(stream, a)) { fail(mx_last_error()); return nullptr; }
    int32_t* rec = bc_dev_rec;
    unsigned char* fl = (unsigned char*)(rec + SkipScratch::record_ints(bc->n_slots));
    want_flags = want_flags || bc->decisions_out != nullptr;
    if (bc_any_valid) {
      const size_t bytes = SkipScratch::record_ints(bc->n_slots) * sizeof(int32_t) + (want_flags ? (size_t)n : 0);
      if (hipMemcpyAsync(rec, bc_skip.record, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        fail("block cache: reading the decision record failed"); return nullptr;
      }
      if (rec[MX_SKIP_REC_STATUS] != 0) { fail("block cache: the device forest or the unit tables point outside themselves"); return nullptr; }
    } else {
      std::memset(rec, 0, SkipScratch::record_ints(bc->n_slots) * sizeof(int32_t));
      std::memset(fl, 1, (size_t)n);
      rec[MX_SKIP_REC_NASK] = n;
      for (int j = 0; j < n; ++j) { const int b = bc_dev_unit_b[j]; rec[MX_SKIP_REC_FIRST + b + 1]++; rec[MX_SKIP_REC_GASK + bc_dev_group[b]]++; rec[MX_SKIP_REC_GTOT + bc_dev_group[b]]++; }
      for (int b = 0; b < B; ++b) rec[MX_SKIP_REC_FIRST + b + 1] += rec[MX_SKIP_REC_FIRST + b];
    }
    if (bc->decisions_out) { std::memcpy(bc->decisions_out + bc_dev_dec, fl, (size_t)n); bc_dev_dec += (size_t)n; }
    if (flags) *flags = fl;
    return rec;
  }
  // batch-ordered tensor <-> its rows in the state
  bool bc_store(char* region, const void* t, size_t per_sample_bytes) {
    if (bc_dslot) { if (launch_copy_rows(stream, (void*)t, region, per_sample_bytes, B, bc_dslot, 1)) return fail(mx_last_error()); return true; }
    if (hipMemcpyAsync(region, t, per_sample_bytes * B, hipMemcpyDeviceToDevice, stream) != hipSuccess) return fail("block cache: copy into the state failed");
    return true;
  }
  bool bc_load(void* t, char* region, size_t per_sample_bytes) {
    if (bc_dslot) { if (launch_copy_rows(stream, t, region, per_sample_bytes, B, bc_dslot, 0)) return fail(mx_last_error()); return true; }
    if (hipMemcpyAsync(t, region, per_sample_bytes * B, hipMemcpyDeviceToDevice, stream) != hipSuccess) return fail("block cache: copy out of the state failed");
    return true;
  }
  // the end of a cached forward: which blocks ran and, in the per-sample forms, what the state now holds
  int bc_finish(bool okr, unsigned long long blocks_run) {
    bc->blocks_run = (unsigned)(blocks_run & 0xffffffffull); bc->blocks_run_hi = (unsigned)(blocks_run >> 32);
    if (bc_keyed) {
      bc->cached_valid = okr ? 1 : 0;
      if (okr) { bc->cached_key = bc->batch_key; bc->cached_batch = B; bc->cached_h = H; bc->cached_w = W; }
    }
    return finish(okr, nullptr);
  }
};

// One forward of a denoiser.  An entry point fills the fields it means; the rest keep their defaults.
struct ForwardCall {
  void* stream = nullptr;
  const void* latents = nullptr; void* out = nullptr; int io_dtype = MX_BF16;
  const float* timesteps = nullptr;
  const void* ehs = nullptr;                                             // encoder_hidden_states
  const void* text_embeds = nullptr; const float* time_ids = nullptr;   // UNet: the added conditions
  const void* pooled = nullptr;                                          // MMDiT: pooled_projections
  int batch = 0, H = 0, W = 0, ctx_len = 0;
  int gn_patch = 0;                                                      // UNet: is_sliced
  void* workspace = nullptr; size_t workspace_bytes = 0;
  const char* stage = nullptr; void* stage_out = nullptr; size_t stage_bytes = 0;   // trace: the tensor to copy out
  bool dry = false;                      // host-only walk: sizes, comm plan
  bool lookup = false;                   // dry walk that resolves every weight
  const mx_pp_comm* comm = nullptr; const mx_pp_stale* stale = nullptr;  // patch-parallel
  size_t* peak = nullptr;                // out: workspace bytes the plan took
  size_t* state_need = nullptr;          // out: bytes of the stale patch-parallel state
  const mx_unet_group* groups = nullptr; int n_groups = 0;               // mixed-resolution batch (then batch, H, W, latents, out are the first group's)
  // block-skip cache: the caller's descriptor, or the zeroed one with n_slots, max_h, max_w of a sizing walk.  Its unit is the sample, or over
  // `groups` the patch / chunk of `patch` latent pixels a side (the UNet's is its gn_patch)
  mx_block_cache* cache = nullptr; int patch = 0;
  size_t* state_bytes = nullptr;         // out: bytes of the cache's state a dry plan took
  bool pp() const { return comm != nullptr && comm->world > 1; }
  bool units() const { return cache != nullptr && groups != nullptr; }
  std::string cached_who(const std::string& model) const { return model + (groups ? "_forward_cached_mixed" : "_forward_cached"); }   // prefix of the cached entries' own messages
};
// the call of a host-only walk of the plan at one shape
inline ForwardCall dry_call(int batch, int H, int W, int ctx_len) {
  ForwardCall c;
  c.dry = true; c.batch = batch; c.H = H; c.W = W; c.ctx_len = ctx_len;
  return c;
}
inline mx_pp_comm sizing_comm(int world) { mx_pp_comm c; c.rank = 0; c.world = world; c.all_gather = nullptr; c.ctx = nullptr; return c; }
// the descriptor a sizing walk of the patch / chunk unit runs against: one state row per sample, as large as the largest group
inline mx_block_cache sizing_cache(const mx_unet_group* groups, int n_groups) {
  mx_block_cache s{};
  for (int g = 0; g < n_groups; ++g) { s.n_slots += groups[g].batch; s.max_h = std::max(s.max_h, groups[g].H); s.max_w = std::max(s.max_w, groups[g].W); }
  return s;
}
// the group list of a cached entry point (the driver's own check speaks of a mixed batch)
inline int check_cached_groups(const std::string& who, const mx_unet_group* groups, int n_groups) {
  MX_CHECK(groups && n_groups >= 1 && n_groups <= MX_MAX_SEGS, who + ": 1..MX_MAX_SEGS resolution groups");
  return 0;
}
// A cached call over groups against its unit of `unit` > 0 latent pixels a side (`word` names it in the messages): state rows of whole units that
// hold every group, one row per sample; then what the device decision needs (n_blocks, n_in_down, n_in_up: DenoiserPlan::bc_dev_check)
inline int check_cache_units(const std::string& who, const ForwardCall& c, int unit, const std::string& word, int n_blocks, int n_in_down, int n_in_up) {
  const mx_block_cache* cache = c.cache;
  MX_CHECK(cache->n_slots > 0 && cache->max_h > 0 && cache->max_w > 0 && cache->max_h % unit == 0 && cache->max_w % unit == 0,
           who + ": cache->n_slots, max_h, max_w (multiples of " + word + ") are required");
  int B = 0;
  for (int g = 0; g < c.n_groups; ++g) {
    const mx_unet_group& q = c.groups[g];
    MX_CHECK(q.batch > 0 && q.H > 0 && q.W > 0 && q.H % unit == 0 && q.W % unit == 0, who + ": every group's H, W must be multiples of " + word);
    MX_CHECK(q.H <= cache->max_h && q.W <= cache->max_w, who + ": a group is larger than the state rows (max_h, max_w)");
    B += q.batch;
  }
  MX_CHECK(B <= cache->n_slots, who + ": more samples than state rows (n_slots)");
  return DenoiserPlan::bc_dev_check(who, cache, n_blocks, (cache->max_h / unit) * (cache->max_w / unit), n_in_down, n_in_up);
}

// The driver of both denoisers.  Handle: weights, graphs, pp_sizes.  Model (one object per call) supplies
//   name                         -- the prefix of the messages;
//   check_units(u, c)            -- a cached call over groups: the unit, the state rows and the groups against them, the device decision's arguments;
//   check(u, c)                  -- the model's own shape and operand checks (0 = fine; c.batch / H / W already describe the first group);
//   begin(u, c) / end(u, c, ok)  -- around the run (the UNet's stored cross-attention K / V^T);
//   setup(p, u, c)               -- the model's fields of a fresh plan (0 = fine); a cached call: the cache's mode, its tables sent, the timesteps read;
//   run(p, c)                    -- p.run(...) with the call's operands;
//   cache_bytes(p)               -- state bytes a dry cached plan took;
//   key_scalars(c), key_operands(c) -- its extra fields of the graph key (the scalars also key the recorded exchange sizes).
// A cached call runs eagerly (its decision synchronises the stream or calls back into the host) and is never looked up among the graphs.
template <class Plan, class Handle, class Model>
int run_forward(Handle* u, ForwardCall c, Model& m) {
  const std::string name = m.name;
  MX_CHECK(u != nullptr, name + ": null handle");
  if (c.units() && m.check_units(u, c)) return 1;
  if (c.groups) {
    MX_CHECK(c.n_groups >= 1 && c.n_groups <= MX_MAX_SEGS && c.comm == nullptr, name + ": a mixed batch has 1..MX_MAX_SEGS resolution groups and does not run patch-parallel");
    c.batch = c.groups[0].batch; c.H = c.groups[0].H; c.W = c.groups[0].W; c.latents = c.groups[0].latents; c.out = c.groups[0].out;
    for (int g = 0; g < c.n_groups; ++g) {
      MX_CHECK(c.groups[g].batch > 0 && c.groups[g].H > 0 && c.groups[g].W > 0, name + ": bad group shape");
      MX_CHECK(c.dry || (c.groups[g].latents && c.groups[g].out), name + ": null group operand");
    }
  }
  const bool pp = c.pp();
  if (pp) MX_CHECK(c.comm->rank >= 0 && c.comm->rank < c.comm->world && (c.dry || c.comm->all_gather != nullptr), name + " pp: bad communicator");
  MX_CHECK(c.batch > 0 && c.H > 0 && c.W > 0 && c.ctx_len > 0, name + ": bad shape");
  if (m.check(u, c)) return 1;
  if (!c.dry) {
    MX_CHECK(c.latents && c.timesteps && c.ehs && c.out && c.workspace, name + ": null operand");
    MX_CHECK(u->weights.blob != nullptr, name + ": weights not set");
    MX_CHECK(c.io_dtype == MX_F32 || c.io_dtype == MX_F16 || c.io_dtype == MX_BF16, name + ": bad io dtype");
  }
  m.begin(u, c);
  std::string err;
  size_t plan_peak = 0;
  auto enqueue = [&](hipStream_t s) {
    Plan p;
    if (c.dry) p.begin_dry(u->weights); else p.begin(u->weights, s, c.workspace, c.workspace_bytes);
    p.stream = s; p.lookup = c.lookup; p.stage = c.stage; p.stage_out = c.stage_out; p.stage_bytes = c.stage_bytes;
    if (c.groups) p.set_groups(c.groups, c.n_groups); else p.set_single(c.batch, c.H, c.W, c.latents, c.out);
    if (pp) p.px.set(c.comm, c.stale);
    if (m.setup(p, u, c)) { err = mx_last_error(); return false; }
    if (pp && c.stale) {      // the state layout (exchanges dealt into chunks, pp_exchange.h) from a host-only recording walk of the same plan
      std::vector<long> lk = {(long)c.batch, (long)c.H, (long)c.W, (long)c.ctx_len};
      for (uint64_t v : m.key_scalars(c)) lk.push_back((long)v);
      lk.push_back((long)c.comm->world); lk.push_back((long)c.io_dtype);
      auto it = u->pp_sizes.find(lk);
      if (it == u->pp_sizes.end()) {
        std::vector<size_t> sizes;
        Plan q = p;
        q.begin_dry(u->weights); q.stage = nullptr; q.lookup = false;
        q.px.record = &sizes;
        ForwardCall none; none.io_dtype = c.io_dtype;
        if (!m.run(q, none)) { err = q.err; return false; }
        it = u->pp_sizes.emplace(lk, std::move(sizes)).first;
      }
      p.px.build_layout(it->second);
    }
    const bool okr = m.run(p, c);
    plan_peak = p.ar.peak;
    if (c.state_need) *c.state_need = p.px.state_top;
    if (c.state_bytes) *c.state_bytes = m.cache_bytes(p);
    if (c.cache && !c.dry) p.bc_finish(okr, p.blocks_run);
    if (!okr) err = p.err;
    return okr;
  };
  bool okr;
  if (c.dry || c.stage || pp || c.cache) {     // (the all-gather callbacks of a patch-parallel forward cannot be captured)
    okr = enqueue((hipStream_t)c.stream);
  } else {
    auto ptr = [](const void* q) { return (uint64_t)(uintptr_t)q; };
    std::vector<uint64_t> key = {(uint64_t)c.batch, (uint64_t)c.H, (uint64_t)c.W, (uint64_t)c.ctx_len};
    for (uint64_t v : m.key_scalars(c)) key.push_back(v);
    for (uint64_t v : {(uint64_t)c.io_dtype, ptr(c.latents), ptr(c.timesteps), ptr(c.ehs)}) key.push_back(v);
    for (const void* q : m.key_operands(c)) key.push_back(ptr(q));
    for (uint64_t v : {ptr(c.out), ptr(c.workspace), (uint64_t)c.workspace_bytes, ptr(u->weights.blob)}) key.push_back(v);
    for (int g = 1; g < c.n_groups; ++g)
      for (uint64_t v : {(uint64_t)c.groups[g].batch, (uint64_t)c.groups[g].H, (uint64_t)c.groups[g].W, ptr(c.groups[g].latents), ptr(c.groups[g].out)})
        key.push_back(v);
    okr = u->graphs.run((hipStream_t)c.stream, key, enqueue, /*capture_on_miss=*/c.n_groups <= 1);
  }
  if (c.peak) *c.peak = plan_peak;
  m.end(u, c, okr);
  if (!okr) { set_error(err); return 1; }
  return 0;
}

}  // namespace mx
