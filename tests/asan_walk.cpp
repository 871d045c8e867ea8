// Host-only walk of every step plan under AddressSanitizer + UBSan (SURVEY.md section 5 "race detection / sanitizers"; GPU sanitizers are not
// available on this pool, so the sanitizer covers what runs on the host: the ~3k lines of arena / cursor / offset arithmetic of the plans).
// Built by `make -C sduss_amd/csrc asan` from the library's own sources compiled --cuda-host-only; nothing here launches a kernel: only the
// dry-run entry points are called (workspace / state sizing, comm plans, grouped-launch tile bookkeeping), at the sizes the benchmark uses.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/mxdenoise.h"

#define REQUIRE(cond)                                                                    \
  do {                                                                                   \
    if (!(cond)) { std::fprintf(stderr, "asan_walk: %s failed at line %d: %s\n", #cond, __LINE__, mx_last_error()); return 1; } \
  } while (0)

// One line per call -- entry point, arguments, returned value -- so that two builds of the library can be compared line for line
// (profiles/plan_scaffold_walk.txt).  say(call(...), value) prints the line and hands the value on to the REQUIRE around it.
static char call_buf[256];
static const char* call(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); std::vsnprintf(call_buf, sizeof(call_buf), fmt, ap); va_end(ap);
  return call_buf;
}
static size_t say(const char* what, size_t v) { std::printf("%s -> %zu\n", what, v); return v; }

static int n_exchanges = 0;
static size_t ws_limit = 0;
static uint64_t exchange_hash = 0;        // FNV-1a over every (send offset, recv offset, bytes) of a comm-plan walk, in order
static int count_gather(void*, void*, const void* send, void* recv, size_t bytes) {
  const size_t so = (size_t)send - 0x1000, ro = (size_t)recv - 0x1000;
  if (so + bytes > ws_limit || ro + 8 * bytes > ws_limit + 8 * bytes) return 1;
  ++n_exchanges;
  for (uint64_t v : {(uint64_t)so, (uint64_t)ro, (uint64_t)bytes})
    for (int k = 0; k < 8; ++k) { exchange_hash ^= (v >> (8 * k)) & 0xff; exchange_hash *= 0x100000001b3ull; }
  return 0;
}
static void begin_exchanges(size_t ws) { n_exchanges = 0; ws_limit = ws; exchange_hash = 0xcbf29ce484222325ull; }
static void say_exchanges(const char* what) { std::printf("%s: %d exchanges, hash %016llx\n", what, n_exchanges, (unsigned long long)exchange_hash); }

static mx_unet_config sdxl_base() {
  mx_unet_config c; std::memset(&c, 0, sizeof(c));
  c.in_channels = 4; c.out_channels = 4; c.n_levels = 3; c.layers_per_block = 2;
  const int ch[3] = {320, 640, 1280}, tl[3] = {1, 2, 10}, at[3] = {0, 1, 1};
  for (int i = 0; i < 3; ++i) { c.block_out_channels[i] = ch[i]; c.transformer_layers[i] = tl[i]; c.down_has_attn[i] = at[i]; c.num_heads[i] = ch[i] / 64; }
  c.cross_attention_dim = 2048; c.addition_time_embed_dim = 256; c.projection_class_embeddings_input_dim = 2816; c.norm_num_groups = 32;
  c.norm_eps = 1e-5f; c.transformer_norm_eps = 1e-6f; c.layer_norm_eps = 1e-5f;
  return c;
}

// the small UNet / MMDiT of tests/test_cpu.py (config.UNetConfig.tiny / MMDiTConfig.tiny): the patch-unit cache walks run at its sizes
static mx_unet_config unet_tiny() {
  mx_unet_config c = sdxl_base();
  const int ch[3] = {64, 128, 256}, tl[3] = {1, 1, 2}, at[3] = {0, 1, 1};
  for (int i = 0; i < 3; ++i) { c.block_out_channels[i] = ch[i]; c.transformer_layers[i] = tl[i]; c.down_has_attn[i] = at[i]; c.num_heads[i] = ch[i] / 64; }
  c.cross_attention_dim = 128; c.addition_time_embed_dim = 32; c.projection_class_embeddings_input_dim = 64 + 6 * 32;
  return c;
}
static mx_mmdit_config mmdit_tiny() {
  mx_mmdit_config c; std::memset(&c, 0, sizeof(c));
  c.patch_size = 2; c.in_channels = 16; c.out_channels = 16; c.num_layers = 4; c.num_attention_heads = 2; c.joint_attention_dim = 128;
  c.pooled_projection_dim = 64; c.pos_embed_max_size = 24; c.norm_eps = 1e-6f;
  c.dual_attention[0] = c.dual_attention[1] = 1;
  return c;
}

int main() {
  // ---- SDXL UNet: every batch / resolution of the predictor table's range, mixed groups, patch-parallel worlds, block-cache state ----
  mx_unet_config uc = sdxl_base();
  mx_unet* u = mx_unet_create(&uc);
  REQUIRE(u != nullptr);
  for (int batch : {1, 2, 3, 8, 16})
    for (int hw : {64, 96, 128}) REQUIRE(say(call("mx_unet_workspace_bytes(%d, %d, %d, 77)", batch, hw, hw), mx_unet_workspace_bytes(u, batch, hw, hw, 77)) > 0);
  REQUIRE(say("mx_unet_workspace_bytes(2, 40, 24, 77)", mx_unet_workspace_bytes(u, 2, 40, 24, 77)) > 0);                       // odd, non-square
  REQUIRE(say("mx_unet_workspace_bytes(2, 30, 32, 77)", mx_unet_workspace_bytes(u, 2, 30, 32, 77)) == 0);                      // not divisible by 2^(levels-1): rejected, not walked
  REQUIRE(say("mx_unet_validate(2, 32, 32, 77) without weights", (size_t)mx_unet_validate(u, 2, 32, 32, 77)) != 0);
  mx_unet_group g[4];
  std::memset(g, 0, sizeof(g));
  const int res[3] = {64, 96, 128};
  for (int a = 1; a <= 4; a += 3)
    for (int b = 1; b <= 3; b += 2)
      for (int c = 1; c <= 4; c += 3) {
        const int n[3] = {2 * a, 2 * b, 2 * c};
        for (int i = 0; i < 3; ++i) { g[i].batch = n[i]; g[i].H = g[i].W = res[i]; }
        REQUIRE(say(call("mx_unet_workspace_bytes_mixed(%d x 64, %d x 96, %d x 128; 77)", n[0], n[1], n[2]), mx_unet_workspace_bytes_mixed(u, g, 3, 77)) > 0);
      }
  g[3].batch = 2; g[3].H = g[3].W = 32;
  REQUIRE(say("mx_unet_workspace_bytes_mixed(8 x 64, 6 x 96, 8 x 128, 2 x 32; 77)", mx_unet_workspace_bytes_mixed(u, g, 4, 77)) > 0);
  REQUIRE(say("mx_unet_workspace_bytes_mixed(5 groups)", mx_unet_workspace_bytes_mixed(u, g, 5, 77)) == 0);
  for (int world : {2, 4, 8}) {
    const size_t ws = say(call("mx_unet_workspace_bytes_pp(2, %d, 128, 77, %d)", 128 / world, world), mx_unet_workspace_bytes_pp(u, 2, 128 / world, 128, 77, world));
    REQUIRE(ws > 0);
    REQUIRE(say(call("mx_unet_pp_state_bytes(2, %d, 128, 77, %d)", 128 / world, world), mx_unet_pp_state_bytes(u, 2, 128 / world, 128, 77, world)) > 0);
    mx_pp_comm comm; comm.rank = world - 1; comm.world = world; comm.all_gather = count_gather; comm.ctx = nullptr;
    begin_exchanges(ws);
    REQUIRE(say(call("mx_unet_pp_comm_plan(2, %d, 128, 77, rank %d of %d)", 128 / world, world - 1, world), (size_t)mx_unet_pp_comm_plan(u, 2, 128 / world, 128, 77, &comm)) == 0);
    say_exchanges("mx_unet_pp_comm_plan");
    REQUIRE(n_exchanges > 100);
  }
  REQUIRE(say("mx_unet_workspace_bytes_pp(2, 8, 64, 77, 8)", mx_unet_workspace_bytes_pp(u, 2, 8, 64, 77, 8)) == 0);            // 8 local tokens per image at the deepest level
  REQUIRE(say("mx_unet_block_cache_bytes(8, 128, 128)", mx_unet_block_cache_bytes(u, 8, 128, 128)) > 0);
  REQUIRE(say("mx_unet_block_cache_bytes(8, 30, 32)", mx_unet_block_cache_bytes(u, 8, 30, 32)) == 0);
  mx_unet_destroy(u);

  // ---- the patch-unit cache of the UNet (tests/test_cpu.py::test_patch_unit_cache_sizing_walks_on_host), with its rejected arguments ----
  {
    mx_unet_config tc = unet_tiny();
    mx_unet* t = mx_unet_create(&tc);
    REQUIRE(t != nullptr);
    REQUIRE(say("mx_unet_patch_cache_bytes(8, 32, 32, 8)", mx_unet_patch_cache_bytes(t, 8, 32, 32, 8)) > 0);
    REQUIRE(say("mx_unet_patch_cache_bytes(16, 32, 32, 8)", mx_unet_patch_cache_bytes(t, 16, 32, 32, 8)) > 0);
    REQUIRE(say("mx_unet_patch_cache_bytes(8, 32, 32, 5)", mx_unet_patch_cache_bytes(t, 8, 32, 32, 5)) == 0);                  // rows must be whole patches
    REQUIRE(say("mx_unet_patch_cache_bytes(8, 32, 32, 4)", mx_unet_patch_cache_bytes(t, 8, 32, 32, 4)) == 0);                  // one pixel at the deepest level
    REQUIRE(say("mx_unet_patch_cache_bytes(0, 32, 32, 8)", mx_unet_patch_cache_bytes(t, 0, 32, 32, 8)) == 0);
    REQUIRE(say("mx_unet_block_cache_bytes(8, 32, 32)", mx_unet_block_cache_bytes(t, 8, 32, 32)) > 0);
    mx_unet_group tg[2]; std::memset(tg, 0, sizeof(tg));
    tg[0].batch = 1; tg[0].H = tg[0].W = 16; tg[1].batch = 2; tg[1].H = tg[1].W = 32;
    REQUIRE(say("mx_unet_workspace_bytes_cached_mixed(1 x 16, 2 x 32; 77, 8)", mx_unet_workspace_bytes_cached_mixed(t, tg, 2, 77, 8)) > 0);
    REQUIRE(say("mx_unet_workspace_bytes_mixed(1 x 16, 2 x 32; 77)", mx_unet_workspace_bytes_mixed(t, tg, 2, 77)) > 0);
    REQUIRE(say("mx_unet_workspace_bytes_cached_mixed(1 x 16, 2 x 32; 77, 0)", mx_unet_workspace_bytes_cached_mixed(t, tg, 2, 77, 0)) == 0);     // needs is_sliced
    REQUIRE(say("mx_unet_workspace_bytes_cached_mixed(1 x 16, 2 x 32; 77, 32)", mx_unet_workspace_bytes_cached_mixed(t, tg, 2, 77, 32)) == 0);   // 16 is not a multiple of 32
    REQUIRE(say("mx_unet_workspace_bytes_cached_mixed(no groups)", mx_unet_workspace_bytes_cached_mixed(t, nullptr, 0, 77, 8)) == 0);
    REQUIRE(say("mx_unet_workspace_bytes_cached_mixed(1 x 16, 2 x 32; 0, 8)", mx_unet_workspace_bytes_cached_mixed(t, tg, 2, 0, 8)) == 0);
    // three resolutions in one launch sequence, and the patch-parallel plan down to its smallest legal split (16 local rows over three levels)
    mx_unet_group t3[3]; std::memset(t3, 0, sizeof(t3));
    const int tres[3] = {16, 24, 32};
    for (int i = 0; i < 3; ++i) { t3[i].batch = i + 1; t3[i].H = t3[i].W = tres[i]; }
    REQUIRE(say("mx_unet_workspace_bytes_mixed(1 x 16, 2 x 24, 3 x 32; 77)", mx_unet_workspace_bytes_mixed(t, t3, 3, 77)) > 0);
    for (int world : {2, 4}) {
      const int hl = 64 / world;
      const size_t ws = say(call("tiny mx_unet_workspace_bytes_pp(2, %d, 64, 77, %d)", hl, world), mx_unet_workspace_bytes_pp(t, 2, hl, 64, 77, world));
      REQUIRE(ws > 0);
      REQUIRE(say(call("tiny mx_unet_pp_state_bytes(2, %d, 64, 77, %d)", hl, world), mx_unet_pp_state_bytes(t, 2, hl, 64, 77, world)) > 0);
      mx_pp_comm comm; comm.rank = world - 1; comm.world = world; comm.all_gather = count_gather; comm.ctx = nullptr;
      begin_exchanges(ws);
      REQUIRE(say(call("tiny mx_unet_pp_comm_plan(2, %d, 64, 77, rank %d of %d)", hl, world - 1, world), (size_t)mx_unet_pp_comm_plan(t, 2, hl, 64, 77, &comm)) == 0);
      say_exchanges("tiny mx_unet_pp_comm_plan");
      REQUIRE(n_exchanges > 0);
    }
    mx_unet_destroy(t);
  }

  // ---- grouped-launch bookkeeping of the GEMM front end: tile choice and statistics slabs over problem lists ----
  {
    mx_gemm_seg s[3]; std::memset(s, 0, sizeof(s));
    const int ms[3] = {512, 1152, 2048};
    for (int i = 0; i < 3; ++i) { s[i].M = ms[i]; s[i].a = (const void*)(uintptr_t)(0x100000 * (i + 1)); s[i].c = (void*)(uintptr_t)(0x9000000 + 0x100000 * i); }
    mx_gemm_desc d; std::memset(&d, 0, sizeof(d));
    d.a = s[0].a; d.w = (const void*)0x1000; d.c = s[0].c; d.N = 1280; d.K = 1280; d.lda = 1280; d.ldc = 1280; d.segs = s; d.n_segs = 3;
    REQUIRE(mx_gemm_stats_slabs(&d) > 0);
    d.N = 10240; d.flags = MX_EPI_GEGLU; d.ldc = 5120;
    (void)mx_gemm_ln_prefers_pass(&d);
  }

  // ---- SD3.5-medium MMDiT ----
  mx_mmdit_config mc; std::memset(&mc, 0, sizeof(mc));
  mc.patch_size = 2; mc.in_channels = 16; mc.out_channels = 16; mc.num_layers = 24; mc.num_attention_heads = 24; mc.joint_attention_dim = 4096;
  mc.pooled_projection_dim = 2048; mc.pos_embed_max_size = 384; mc.norm_eps = 1e-6f;
  for (int i = 0; i < 13; ++i) mc.dual_attention[i] = 1;
  mx_mmdit* m = mx_mmdit_create(&mc);
  REQUIRE(m != nullptr);
  for (int batch : {1, 2, 8})
    for (int hw : {64, 96, 128}) REQUIRE(say(call("mx_mmdit_workspace_bytes(%d, %d, %d, 333)", batch, hw, hw), mx_mmdit_workspace_bytes(m, batch, hw, hw, 333)) > 0);
  REQUIRE(say("mx_mmdit_workspace_bytes(2, 63, 64, 333)", mx_mmdit_workspace_bytes(m, 2, 63, 64, 333)) == 0);                  // not whole patches
  REQUIRE(say("mx_mmdit_validate(2, 16, 16, 37) without weights", (size_t)mx_mmdit_validate(m, 2, 16, 16, 37)) != 0);
  for (int world : {2, 4, 8}) {
    const size_t ws = say(call("mx_mmdit_workspace_bytes_pp(2, %d, 128, 333, %d)", 128 / world, world), mx_mmdit_workspace_bytes_pp(m, 2, 128 / world, 128, 333, world));
    REQUIRE(ws > 0);
    REQUIRE(say(call("mx_mmdit_pp_state_bytes(2, %d, 128, 333, %d)", 128 / world, world), mx_mmdit_pp_state_bytes(m, 2, 128 / world, 128, 333, world)) > 0);
    mx_pp_comm comm; comm.rank = world - 1; comm.world = world; comm.all_gather = count_gather; comm.ctx = nullptr;
    begin_exchanges(ws);
    REQUIRE(say(call("mx_mmdit_pp_comm_plan(2, %d, 128, 333, rank %d of %d)", 128 / world, world - 1, world), (size_t)mx_mmdit_pp_comm_plan(m, 2, 128 / world, 128, 333, &comm)) == 0);
    say_exchanges("mx_mmdit_pp_comm_plan");
    REQUIRE(n_exchanges > 0);
  }
  REQUIRE(say("mx_mmdit_workspace_bytes_pp(2, 2, 4, 333, 2)", mx_mmdit_workspace_bytes_pp(m, 2, 2, 4, 333, 2)) == 0);           // 2 local image tokens: not a multiple of 16
  REQUIRE(say("mx_mmdit_block_cache_bytes(8, 128, 128, 333)", mx_mmdit_block_cache_bytes(m, 8, 128, 128, 333)) > 0);
  REQUIRE(say("mx_mmdit_block_cache_bytes(8, 127, 128, 333)", mx_mmdit_block_cache_bytes(m, 8, 127, 128, 333)) == 0);
  for (int i = 0; i < 3; ++i) { g[i].batch = 2 * (i + 1); g[i].H = g[i].W = res[i]; }
  REQUIRE(say("mx_mmdit_workspace_bytes_mixed(2 x 64, 4 x 96, 6 x 128; 333)", mx_mmdit_workspace_bytes_mixed(m, g, 3, 333)) > 0);
  REQUIRE(say("mx_mmdit_workspace_bytes_mixed(2 x 64, 4 x 96; 333)", mx_mmdit_workspace_bytes_mixed(m, g, 2, 333)) > 0);
  REQUIRE(say("mx_mmdit_workspace_bytes_mixed(5 groups)", mx_mmdit_workspace_bytes_mixed(m, g, 5, 333)) == 0);
  mx_mmdit_destroy(m);

  // ---- the chunk-unit cache of the MMDiT at the small model of tests/test_cpu.py, with its rejected arguments ----
  {
    mx_mmdit_config tc = mmdit_tiny();
    mx_mmdit* t = mx_mmdit_create(&tc);
    REQUIRE(t != nullptr);
    REQUIRE(say("mx_mmdit_patch_cache_bytes(8, 32, 32, 8, 37)", mx_mmdit_patch_cache_bytes(t, 8, 32, 32, 8, 37)) > 0);
    REQUIRE(say("mx_mmdit_patch_cache_bytes(16, 32, 32, 8, 37)", mx_mmdit_patch_cache_bytes(t, 16, 32, 32, 8, 37)) > 0);
    REQUIRE(say("mx_mmdit_patch_cache_bytes(8, 32, 32, 5, 37)", mx_mmdit_patch_cache_bytes(t, 8, 32, 32, 5, 37)) == 0);          // not a multiple of patch_size
    REQUIRE(say("mx_mmdit_patch_cache_bytes(8, 64, 64, 8, 37)", mx_mmdit_patch_cache_bytes(t, 8, 64, 64, 8, 37)) == 0);          // larger than the positional table
    REQUIRE(say("mx_mmdit_patch_cache_bytes(8, 32, 32, 8, 0)", mx_mmdit_patch_cache_bytes(t, 8, 32, 32, 8, 0)) == 0);
    REQUIRE(say("mx_mmdit_block_cache_bytes(8, 32, 32, 37)", mx_mmdit_block_cache_bytes(t, 8, 32, 32, 37)) > 0);
    mx_unet_group tg[2]; std::memset(tg, 0, sizeof(tg));
    tg[0].batch = 1; tg[0].H = tg[0].W = 16; tg[1].batch = 2; tg[1].H = tg[1].W = 32;
    REQUIRE(say("mx_mmdit_workspace_bytes_cached_mixed(1 x 16, 2 x 32; 37, 8)", mx_mmdit_workspace_bytes_cached_mixed(t, tg, 2, 37, 8)) > 0);
    REQUIRE(say("mx_mmdit_workspace_bytes_mixed(1 x 16, 2 x 32; 37)", mx_mmdit_workspace_bytes_mixed(t, tg, 2, 37)) > 0);
    REQUIRE(say("mx_mmdit_workspace_bytes_cached_mixed(1 x 16, 2 x 32; 37, 0)", mx_mmdit_workspace_bytes_cached_mixed(t, tg, 2, 37, 0)) == 0);
    REQUIRE(say("mx_mmdit_workspace_bytes_cached_mixed(1 x 16, 2 x 32; 37, 32)", mx_mmdit_workspace_bytes_cached_mixed(t, tg, 2, 37, 32)) == 0);  // 16 is not a multiple of 32
    REQUIRE(say("mx_mmdit_workspace_bytes_cached_mixed(no groups)", mx_mmdit_workspace_bytes_cached_mixed(t, nullptr, 0, 37, 8)) == 0);
    // three resolutions in one cached launch sequence with the state of its four requests, and the patch-parallel plan at 32 and 16 local tokens
    mx_unet_group t3[3]; std::memset(t3, 0, sizeof(t3));
    const int tres[3] = {16, 24, 32}, tb[3] = {1, 2, 1};
    for (int i = 0; i < 3; ++i) { t3[i].batch = tb[i]; t3[i].H = t3[i].W = tres[i]; }
    REQUIRE(say("mx_mmdit_workspace_bytes_cached_mixed(1 x 16, 2 x 24, 1 x 32; 37, 8)", mx_mmdit_workspace_bytes_cached_mixed(t, t3, 3, 37, 8)) > 0);
    REQUIRE(say("mx_mmdit_workspace_bytes_mixed(1 x 16, 2 x 24, 1 x 32; 37)", mx_mmdit_workspace_bytes_mixed(t, t3, 3, 37)) > 0);
    REQUIRE(say("mx_mmdit_patch_cache_bytes(4, 32, 32, 8, 37)", mx_mmdit_patch_cache_bytes(t, 4, 32, 32, 8, 37)) > 0);
    for (int world : {2, 4}) {
      const int hl = 16 / world;
      const size_t ws = say(call("tiny mx_mmdit_workspace_bytes_pp(2, %d, 16, 37, %d)", hl, world), mx_mmdit_workspace_bytes_pp(t, 2, hl, 16, 37, world));
      REQUIRE(ws > 0);
      REQUIRE(say(call("tiny mx_mmdit_pp_state_bytes(2, %d, 16, 37, %d)", hl, world), mx_mmdit_pp_state_bytes(t, 2, hl, 16, 37, world)) > 0);
      mx_pp_comm comm; comm.rank = world - 1; comm.world = world; comm.all_gather = count_gather; comm.ctx = nullptr;
      begin_exchanges(ws);
      REQUIRE(say(call("tiny mx_mmdit_pp_comm_plan(2, %d, 16, 37, rank %d of %d)", hl, world - 1, world), (size_t)mx_mmdit_pp_comm_plan(t, 2, hl, 16, 37, &comm)) == 0);
      say_exchanges("tiny mx_mmdit_pp_comm_plan");
      REQUIRE(n_exchanges > 0);
    }
    mx_mmdit_destroy(t);
  }

  // ---- VAE decoder, CLIP, T5 ----
  mx_vae_config vc; std::memset(&vc, 0, sizeof(vc));
  vc.latent_channels = 4; vc.out_channels = 3; vc.n_levels = 4; vc.layers_per_block = 2; vc.norm_num_groups = 32; vc.norm_eps = 1e-6f;
  const int vch[4] = {128, 256, 512, 512};
  for (int i = 0; i < 4; ++i) vc.block_out_channels[i] = vch[i];
  mx_vae* v = mx_vae_create(&vc);
  REQUIRE(v != nullptr);
  for (int hw : {64, 96, 128}) REQUIRE(say(call("mx_vae_workspace_bytes(2, %d, %d)", hw, hw), mx_vae_workspace_bytes(v, 2, hw, hw)) > 0);
  REQUIRE(say("mx_vae_workspace_bytes(0, 64, 64)", mx_vae_workspace_bytes(v, 0, 64, 64)) == 0);
  REQUIRE(say("mx_vae_validate(1, 16, 16) without weights", (size_t)mx_vae_validate(v, 1, 16, 16)) != 0);
  mx_vae_destroy(v);
  mx_clip_config cc; std::memset(&cc, 0, sizeof(cc));
  cc.vocab_size = 49408; cc.hidden_size = 1280; cc.intermediate_size = 5120; cc.num_hidden_layers = 32; cc.num_attention_heads = 20;
  cc.max_position_embeddings = 77; cc.hidden_act = 1; cc.projection_dim = 1280; cc.eos_token_id = 2; cc.hidden_layer = -2; cc.layer_norm_eps = 1e-5f;
  mx_clip* c = mx_clip_create(&cc);
  REQUIRE(c != nullptr && say("mx_clip_workspace_bytes(8)", mx_clip_workspace_bytes(c, 8)) > 0);
  REQUIRE(say("mx_clip_workspace_bytes(0)", mx_clip_workspace_bytes(c, 0)) == 0);
  REQUIRE(say("mx_clip_validate(2) without weights", (size_t)mx_clip_validate(c, 2)) != 0);
  mx_clip_destroy(c);
  mx_t5_config tc; std::memset(&tc, 0, sizeof(tc));
  tc.vocab_size = 32128; tc.d_model = 4096; tc.d_ff = 10240; tc.num_layers = 24; tc.num_heads = 64; tc.layer_norm_epsilon = 1e-6f;
  mx_t5* t = mx_t5_create(&tc);
  REQUIRE(t != nullptr && say("mx_t5_workspace_bytes(2, 256)", mx_t5_workspace_bytes(t, 2, 256)) > 0);
  REQUIRE(say("mx_t5_workspace_bytes(2, 250)", mx_t5_workspace_bytes(t, 2, 250)) == 0);          // not a multiple of 8
  REQUIRE(say("mx_t5_validate(2, 256) without weights", (size_t)mx_t5_validate(t, 2, 256)) != 0);
  mx_t5_destroy(t);
  std::printf("ASAN_WALK_OK\n");
  return 0;
}
