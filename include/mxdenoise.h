/*
 * mxdenoise -- MI355X (gfx950) native denoiser for the sduss/Mixfusion model slot.  C ABI.
 *
 * Plain pointers and sizes only (no torch types).  Every device pointer is a HIP device
 * address owned by the caller; every entry point takes an explicit hipStream_t (as void*),
 * launches asynchronously on it and never synchronises the device.  Return value: 0 on
 * success, non-zero on error (mx_last_error() gives the message for the calling thread).
 *
 * Reference interfaces replaced (paths relative to the sduss tree):
 *   inner boundary  esymred_mp.groupnorm / mock_groupnorm
 *                   sduss/model_executor/modules/kernels/norm_silu_concat.cpp:66-101
 *                   (called from modules/groupnorm.py:33,50,58)
 *   outer boundary  PatchUNet.forward            sduss/model_executor/modules/unet.py:205-530
 *                   (invoked once per step at
 *                    diffusers/pipelines/stable_diffusion_xl/pipeline_stable_diffusion_xl_esymred.py:369-380)
 *   step either side EulerDiscreteScheduler.batch_scale_model_input / batch_step
 *                   diffusers/schedulers/scheduling_euler_discrete.py:161-274 and the CFG combine
 *                   pipeline_stable_diffusion_xl_esymred.py:382-385
 */
#ifndef MXDENOISE_H
#define MXDENOISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types of caller tensors */
enum { MX_F32 = 0, MX_F16 = 1, MX_BF16 = 2 };

const char* mx_last_error(void);
int mx_version(void);
/* Optional per-launch timing for bench.py's roofline leg: while enabled, every GEMM / conv / attention / norm launch
 * is bracketed by hipEvents on its own stream.  mx_profile_collect (after the stream is synchronised) fills
 * out[4 * MX_PROF_KINDS] = for kind in {gemm<128>, gemm<64>, conv3x3<128>, conv3x3<64>, attention, groupnorm,
 *           gemm_v2<160>, conv3x3_v2<160>, gemm_v2<128>, conv3x3_v2<128>, gemm 256x256, cross-attention (Lk <= 96)}:
 *           {launches, milliseconds, algorithmic flops, algorithmic bytes}. */
#define MX_PROF_KINDS 12
int mx_profile_enable(int on);
int mx_profile_collect(double* out);
/* per-launch records of the last collect: out[6*i..] = {kind, M, N, K, ms, flops}; returns the number written */
int mx_profile_records(double* out, int max_records);

/* ------------------------------------------------------------------------------------------
 * Inner boundary: drop-in for the reference's only native op (NCHW patch batches).
 *
 * mx_groupnorm_halo == esymred_mp.groupnorm (norm_silu_concat.cpp:75-101):
 *   per-(patch,group) moments -> cross-patch merge per latent (mean of means, mean of biased
 *   variances; norm_silu_concat.cu:361-386) -> y = x*(rstd*gamma) + (beta - rstd*gamma*mean)
 *   (no SiLU, cu:157-163) -> if padding: result placed in the interior of a zero-filled
 *   [N,C,H+2,W+2] tensor and each patch's edge rows/cols/corners scattered into its neighbours'
 *   halo cells (cu:164-241).  `cpg` is what the reference calls `group` (channels per group).
 *   x: [N,C,H,W] contiguous, y: [N,C,H+2p,W+2p] (p = padding?1:0), gamma/beta: [C] of `dtype`,
 *   latent_offset: int32[n_latents+1], patch_map: int32[N] (1-based latent index),
 *   padding_idx: int32[4N] = (top,left,bottom,right) neighbour patch index or -1.
 *   workspace: >= mx_groupnorm_halo_workspace_bytes(N, C, cpg) bytes of device scratch.
 *   Differences, on purpose: statistics are kept in fp32 (the reference rounds them to the
 *   tensor dtype, cpp:84-85); the merge is out of place (the reference's in-place merge races);
 *   no device synchronisation (reference: cudaDeviceSynchronize after every launch).
 *   The halo is GATHERED by the receiving plane through the inverse of padding_idx (receiver r's side d is written by the b with
 *   padding_idx[b][opposite(d)] == r) with the SENDER's statistics, so the result equals the reference's sender-driven scatter for every
 *   table in which a halo side has at most one writer -- symmetric adjacency (what split_sample produces) is NOT required; with two
 *   writers for one cell the reference's scatter races and the value here is that of one of them.  Entries must be -1 or in [0, N).
 *
 * mx_halo_only == esymred_mp.mock_groupnorm (cpp:66-74): the same scatter with identity values.
 * ------------------------------------------------------------------------------------------ */
size_t mx_groupnorm_halo_workspace_bytes(int N, int C, int cpg);
int mx_groupnorm_halo(void* stream, const void* x, const void* gamma, const void* beta, void* y,
                      int N, int C, int H, int W, int cpg, double eps, int padding,
                      const int32_t* latent_offset, int n_latents, const int32_t* patch_map,
                      const int32_t* padding_idx, int dtype, void* workspace);
int mx_halo_only(void* stream, const void* x, void* y, int N, int C, int H, int W,
                 const int32_t* padding_idx, int dtype);

/* ------------------------------------------------------------------------------------------
 * Building blocks of the step plan (NHWC / token-major bf16, fp32 accumulate).  Exported so the
 * parity tests can check each kernel against the oracle through the same ABI the plan uses.
 * ------------------------------------------------------------------------------------------ */

/* epilogue flags for mx_gemm / mx_conv3x3 */
enum {
  MX_EPI_SILU     = 1 << 0,  /* out = silu(v) */
  MX_EPI_GEGLU    = 1 << 1,  /* weight rows interleaved [32 hidden | 32 gate]; out[M, N/2] = h * gelu(g) */
  MX_EPI_OUT_F32  = 1 << 2,  /* C is fp32 instead of bf16 */
  MX_EPI_QKV      = 1 << 3,  /* column segments of width seg: segment s with (s % period) == period-1
                                is written transposed into vt[b][vcol][key]; others row-major, compacted.
                                Excludes rowbias / gate / residual (error otherwise) */
  MX_EPI_GELU_TANH = 1 << 4, /* out = gelu(v), tanh approximation (diffusers FeedForward "gelu-approximate") */
  MX_EPI_RES_BCAST = 1 << 5, /* residual row = output row modulo rows_per_batch (positional table broadcast over the batch) */
  MX_EPI_RMSNORM  = 1 << 6,  /* with MX_EPI_QKV: RMS-normalise every 64-wide head of the q and k segments (see rms_wq below) */
  MX_EPI_GELU     = 1 << 7,  /* out = gelu(v), exact (erf) form: the OpenCLIP text encoder's MLP */
  MX_EPI_QUICK_GELU = 1 << 8, /* out = v * sigmoid(1.702 v): the CLIP ViT-L text encoder's MLP */
  MX_EPI_GEGLU_TANH = 1 << 9 /* with MX_EPI_GEGLU: the gate takes the tanh form of GELU ("gelu_new": T5 v1.1 gated-gelu) */
};

/* One problem of a GROUPED launch (mx_gemm_desc.segs): mixed-resolution batches run every op of the step plan ONCE over the requests of all
 * resolutions present (the reference's reason to exist: modules/unet.py:104-185 cuts the latents of all resolutions into one patch batch).
 * The problems of a group share w, bias, N, K, the leading dimensions, flags and every scalar of the descriptor; each has its own rows,
 * per-batch structure and operand bases.  Output tiles never straddle two problems (a workgroup finds its problem from its tile index with
 * two compares and then runs the ordinary kernel body on it), nothing is padded in memory, and every output element sees exactly the
 * arithmetic of a separate launch with the same tile shape.  Pointer fields that the descriptor leaves NULL must be NULL here too. */
/* At most MX_MAX_SEGS resolutions share one launch sequence (the reference serves 512 / 768 / 1024 px).  A batch with MORE distinct resolutions is
 * not an error: the host mirrors (MxUNet.forward / SDXLDenoiser.denoising_step and the SD3 ones) then fall back to one launch sequence per
 * resolution on concurrent streams -- same results, the mixed-batch speed-up is lost. */
#define MX_MAX_SEGS 4
typedef struct mx_gemm_seg {
  const void* a;          /* this problem's A rows (conv: its first image) */
  const void* a2;
  void* c;
  const void* residual;
  void* vt;
  const float* rowbias;   /* row 0 = this problem's first sample */
  const float* gate;
  const float* ln_stats;
  float* stats_out;
  int M;                  /* rows (conv: B * Hout * Wout) */
  int rows_per_batch;
  int ldvt;
  int B, Hin, Win, Hout, Wout;                              /* conv geometry */
  int a_batch_rows, a_row_off, c_batch_rows, c_row_off;     /* joint-sequence remap */
} mx_gemm_seg;

typedef struct mx_gemm_desc {
  const void* a;        /* bf16 [M, K] row stride lda (elements); conv: NHWC input [B, Hin, Win, Cin] */
  const void* w;        /* bf16 [N, K] row-major (K = 9*Cin tap-major for conv) */
  void* c;              /* bf16 (or fp32) [M, ldc] */
  const float* bias;    /* fp32 [N] or NULL */
  const float* rowbias; /* fp32 [M / rows_per_batch, ldrb] or NULL (time-embedding add of resnet conv1) */
  const void* residual; /* bf16 [M, ldr] or NULL, added before the activation */
  void* vt;             /* MX_EPI_QKV: bf16 [batches][N/period][ldvt] */
  int M, N, K;
  int lda, ldc, ldr, ldrb;
  int rows_per_batch;
  int flags;
  int seg, period, ldvt; /* MX_EPI_QKV */
  /* conv geometry (ignored by mx_gemm) */
  int B, Hin, Win, Cin;  /* stored input */
  int Hout, Wout;        /* output grid; M = B*Hout*Wout */
  int stride;            /* 1 or 2 */
  int up;                /* 1: input is nearest-upsampled x2 on the fly (Hout = 2*Hin) */
  int corner_patch;      /* >0: sliced-mode halo-corner rule with this patch edge (output-grid pixels
                            for stride 1, input-grid pixels for stride 2); 0: plain zero padding */
  /* joint-sequence support (MMDiT): rows live in per-sample blocks of a longer sequence.
   * input  row of m = (m / rows_per_batch) * a_batch_rows + a_row_off + m % rows_per_batch   (a_batch_rows > 0)
   * output row of m = (m / rows_per_batch) * c_batch_rows + c_row_off + m % rows_per_batch   (c_batch_rows > 0);
   * it addresses C, the residual and, under MX_EPI_QKV, the key index of vt (then ldvt >= MX_VT_LD(c_batch_rows)). */
  int a_batch_rows, a_row_off, c_batch_rows, c_row_off;
  const float* gate;     /* fp32 [M / rows_per_batch, ldg] or NULL: v = gate * (acc + bias) before the residual add */
  int ldg;
  float out_scale;       /* != 0: v = (acc + bias) * out_scale, before row bias / gate / residual.  Under MX_EPI_QKV only the
                          * first segment of every group (q) is scaled -- for mx_attention_prescaled */
  /* MX_EPI_RMSNORM (with MX_EPI_QKV, period 3, N % 128 == 0): every 64-wide head of the q and k segments is RMS-normalised
   * before it is stored: x * rsqrt(mean(x^2) + rms_eps) * w, w = rms_wq / rms_wk (fp32 [64]); out_scale then multiplies the
   * normalised q.  Fuses diffusers' norm_q / norm_k (RMSNorm(64)) of the SD3 attention into the projection. */
  const float* rms_wq;
  const float* rms_wk;
  float rms_eps;
  /* conv3x3, patch-parallel (mx_unet_forward_pp): 1 = every image of `a` is stored with ONE extra row above and below
   * ([B, Hin + 2, Win, Cin], `a` pointing at the top halo row of image 0); taps that leave the image vertically read those
   * rows (the neighbour ranks' boundary rows, or zeros at the true image border) instead of zero padding. */
  int vhalo;
  /* mx_gemm: the A operand as a concatenation along K read in place: columns [0, k_split) from a (row stride lda), columns
   * [k_split, K) from a2 (row stride lda2); k_split % 64 == 0.  a2 == NULL: one source.  (The 1x1 shortcut conv of an up block
   * reads torch.cat([hidden_states, res_hidden_states]); not combined with the joint-sequence row remap.) */
  const void* a2;
  int lda2, k_split;
  /* LayerNorm folded into the GEMM that consumes it (the SDXL BasicTransformerBlock's norm1 / norm2 / norm3, modules/transformer.py:191,
   * 239, 266: each feeds exactly one linear).  With W' = W * gamma (per input feature, packed in `w`), colsum[n] = sum_k W'[n][k] (fp32, of
   * the bf16-rounded W') and bias' = bias + W beta (in `bias`):
   *     LayerNorm(x) W^T + bias  ==  rstd_m * (x W'^T - mean_m * colsum) + bias'
   * so the GEMM reads the UN-normalised x and its epilogue applies the row statistics: no LayerNorm pass, no rounding of the normalised
   * activations.  ln_stats != NULL selects it: fp32 pairs (sum x, sum x^2) per row and slab, ln_stats[(m * pitch + slab) * 2 + {0, 1}] with
   * pitch = MX_STATS_PITCH(ln_slabs), summed over ln_slabs slabs (written by the producing GEMM through stats_out, or by mx_row_stats
   * with one slab; entries past the last slab are never read); 16-byte aligned; the LN width is K.  Not combined with MX_EPI_RMSNORM or
   * the row remaps.
   * stats_out != NULL (plain bf16 output, no GEGLU / QKV / remap): the epilogue also writes, for every output row, the sum and the sum of
   * squares of the values it stores, one slab per wave column panel; mx_gemm_stats_slabs(d) tells how many slabs THIS launch writes
   * (0: the kernel chosen for d cannot, use mx_row_stats). */
  const float* ln_stats;
  const float* ln_colsum;
  int ln_slabs;
  float ln_eps;
  float* stats_out;
  /* grouped launch: n_segs in [1, MX_MAX_SEGS] problems (see mx_gemm_seg); 0 = the single problem described above.  With segs the
   * descriptor's own a / c / residual / vt / rowbias / gate / ln_stats / stats_out only say WHICH operands exist (non-NULL), M is ignored. */
  const mx_gemm_seg* segs;
  int n_segs;
  /* split-K (see mx_gemm_splitk): 0 = the library decides from the shape (a split is taken where its estimate beats the unsplit launch by 25 %),
   * 1 = never, 2..4 = that many slices wherever the launch is eligible at all (a 128-row tiling, >= 8 K tiles per slice, no split A operand) */
  int splitk;
  /* FINALISED row statistics (round 4): the form of the folded LayerNorm the persistent 256 x 256 kernel can afford.  A producer launched with
   * stats_out AND ln_final_out != NULL (256-row x 160 / 128 tiles only: mx_gemm_ln_final_supported) also leaves, per output row, the pair
   * (mean, rstd) over its N columns in ln_final_out[m * 2 + {0, 1}] (rstd with the producer's own ln_eps): the LAST workgroup of a 256-row
   * panel to finish -- a ticket in ln_final_cnt[panel], one unsigned per 256 rows, ZERO before the launch and zero again after it -- adds the
   * panel's slabs in slab order (bit-stable run to run).  A consumer launched with ln_final != NULL (and ln_colsum; ln_stats NULL; no grouped
   * launch, no row remap) reads those 8 bytes per row instead of the slabs: it runs on the 256 x 256 kernel where the plain launch would, and
   * the normalisation pass in front of it disappears.  16-byte aligned. */
  const float* ln_final;
  float* ln_final_out;
  unsigned* ln_final_cnt;
  /* GroupNorm statistics from the producing launch (round 4): gn_part_out != NULL makes a conv / GEMM on a 256-row tile whose epilogue is bias (+ per-sample
   * row bias) only ALSO leave, per 64 consecutive output rows and per channel, the sum and the sum of squares of its ACCUMULATORS -- the values it stores minus
   * the per-channel constants bias[n] + rowbias[sample][n] (fp32): gn_part_out[(m / 64 * N + n) * 2 + {0, 1}], M % 64 == 0 (and rows_per_batch % 64 == 0 with a row
   * bias).  mx_groupnorm_nhwc_from_partials, given the same bias / row bias, adds the constants back in closed form and needs no statistics pass over the tensor
   * (the reference's resnet: conv1 + time embedding -> norm2, resnet.py:414-429).  mx_gemm_gn_partials_supported(d,
   * conv) tells whether the launch can. */
  float* gn_part_out;
  /* mx_conv3x3 (round 5): > 0 = only the first cin_valid (<= 8) channels of every input pixel are non-zero -- the UNet's conv_in reads the 4 latent channels
   * zero-padded to Cin = 64.  The launch may then contract over 9 x 8 instead of 9 x Cin (conv_small_n.hip); 0 = every channel counts.  Never changes the result. */
  int cin_valid;
} mx_gemm_desc;

int mx_gemm(void* stream, const mx_gemm_desc* d);      /* C = A * W^T (+epilogue) */
/* 2 where mx_gemm cuts d along N (TAIL SPLIT: a launch of the persistent 256 x 256 kernel whose last round would be less than half full -- one
 * 1024 px request's GEGLU projection is 1.25 rounds -- runs its whole rounds there and the remaining column panels as ONE round of a smaller tile;
 * plain / gated epilogues, ungrouped, no statistics), else 1.  Shape-based and host-only. */
int mx_gemm_launches(const mx_gemm_desc* d);
int mx_gemm_stats_slabs(const mx_gemm_desc* d);        /* slabs d->stats_out receives from mx_gemm(d); 0 = not supported for this shape */
/* 1 when mx_gemm(d) with ln_stats would run on the persistent 256 x 256 kernel, where applying the statistics costs more than a separate
 * normalisation pass saves (10-20 us per launch in the hand-over between two tiles against an 11-us pass at M = 8192); the step plan then
 * normalises with mx_layernorm(gamma = NULL) and launches d without ln_stats.  The 256 / 128-row kernels hide the statistics behind their
 * first operand fetch: 0. */
int mx_gemm_ln_prefers_pass(const mx_gemm_desc* d);
/* 1 when mx_gemm(d) with stats_out can also write ln_final_out (the launch takes a 256-row tile of the register-exchange kernels, ungrouped) */
int mx_gemm_ln_final_supported(const mx_gemm_desc* d);
int mx_gemm_gn_partials_supported(const mx_gemm_desc* d, int conv);   /* 1 when mx_gemm / mx_conv3x3 (d) can write gn_part_out */
/* By which route each of the three folded LayerNorms of an SDXL transformer block of width C over M token rows reaches its consuming GEMM in the UNet's
 * step plan (the plan asks the same function; the rule is the table in sduss_amd/csrc/ln_route.h) -- host only.  routes[0..2] = norm1 (q|k|v), norm2
 * (attn2.to_q), norm3 (GEGLU projection): 0 = a normalisation pass, 1 = ln_stats slabs from the producing launch, 2 = finalised (mean, rstd), ln_final;
 * routes[3] = 1 when norm3's finalised statistics come from the patch cache's merge kernel.  layers: transformer blocks of the model; n_groups > 1: a
 * mixed batch, taken as n_groups equal parts of M of one image each; flags: MX_LN_ROUTES_*, TICKETS = the plan holds panel tickets that cover M rows.
 * Returns non-zero on bad arguments. */
enum { MX_LN_ROUTES_PATCH_PARALLEL = 1, MX_LN_ROUTES_PATCH_CACHE = 2, MX_LN_ROUTES_TICKETS = 4 };
int mx_unet_ln_routes(int M, int C, int layers, int n_groups, int flags, int routes[4]);
/* Which kernel family serves mx_gemm (conv = 0) / mx_conv3x3 (conv = 1) of d -- host only, the same chooser the launch uses:
 *   MX_FORM_TILE_GENERIC   the 128-row register-prefetch tile kernel (small or odd shapes)
 *   MX_FORM_TILE_256       a 256-row tile of the ping-pong kernels (256 x 160 / 128, one tile per CU)
 *   MX_FORM_TILE_128       a 128-row tile of the lock-step LDS-DMA kernel (small M; possibly split along K)
 *   MX_FORM_PERSISTENT_256 the persistent 256 x 256 kernel
 *   MX_FORM_SMALL_M        round 5: M <= 16 rows as a weight stream (bias, per-row residual, SiLU, bf16 / fp32 out; N % 16 == 0; above 64 MB of weights M (K + 8) <= 32 K elements)
 *   MX_FORM_CONV_SMALL_N   round 5: 3 x 3 conv with N <= 16 output channels (stride 1, bias only; weights + one staged chunk within 64 KB of LDS)
 *   MX_FORM_CONV_SMALL_CIN round 5: 3 x 3 conv whose descriptor names cin_valid <= 8 input channels (stride 1, bias only, N % 80 == 0) */
enum { MX_FORM_TILE_GENERIC = 0, MX_FORM_TILE_256 = 1, MX_FORM_TILE_128 = 2, MX_FORM_PERSISTENT_256 = 3, MX_FORM_SMALL_M = 4, MX_FORM_CONV_SMALL_N = 5, MX_FORM_CONV_SMALL_CIN = 6 };
int mx_gemm_form(const mx_gemm_desc* d, int conv);
/* Which kernel INSTANTIATION serves launch number `launch` of mx_gemm (conv = 0) / mx_conv3x3 (conv = 1) of d -- host only, the chooser the launch
 * dispatches on: its name (the kernel and its template arguments, e.g. "gemm_v2_kernel<160, 2, true, EPI_F_ALL, false>") goes to buf (cap bytes,
 * NUL-terminated).  launch: 0, and 1 for the second launch of mx_gemm's tail split (mx_gemm_launches).  Returns the name's length, 0 past the last
 * launch, -1 when no instantiation serves d.  mx_gemm_kernel_names: every instantiation the GEMM / conv launchers can start, one per line; returns
 * the length of the whole list. */
int mx_gemm_kernel_name(const mx_gemm_desc* d, int conv, int launch, char* buf, int cap);
int mx_gemm_kernel_names(char* buf, int cap);
/* The same for one attention launch over a problem of this shape (B, H, Lq, Lk, ldo; prescaled q; causal, bias and key_chunk as the attention entry
 * points take them; force_cross = mx_attention_cross_prescaled).  Returns the name's length, -1 when no instantiation serves it. */
int mx_attention_kernel_name(int B, int H, int Lq, int Lk, int ldo, int prescaled, int causal, int bias, int key_chunk, int force_cross, char* buf, int cap);
int mx_attention_kernel_names(char* buf, int cap);
#define MX_STATS_PITCH(slabs) (((slabs) + 3) & ~3)     /* slabs per row of a statistics buffer: [M][pitch][2] floats */
/* stats[m * 4 * 2 + {0, 1}] = (sum_c x[m][c], sum_c x[m][c]^2), x bf16 [M, C] with row stride ldx: the one-slab input of ln_stats
 * (buffer of M * MX_STATS_PITCH(1) * 2 floats) */
int mx_row_stats(void* stream, const void* x, int ldx, float* stats, int M, int C);
int mx_conv3x3(void* stream, const mx_gemm_desc* d);   /* implicit GEMM, pad 1 */
/* The same conv with the input staged once per 64-channel chunk (csrc/conv_halo.hip; an operator of its own, not a route of mx_conv3x3): a tile is
 * 256 output pixels = whole image rows x 160 features, K runs chunk-major, and the nine taps of a chunk read one staged (rows + 2) x width tile of
 * 128-byte pixel lines instead of nine copies of it.  Same products, fp32 accumulation and epilogue (bias, row bias, residual, gn_part_out) as the
 * 256-row tile of mx_conv3x3; the order in which a pixel's products are added differs, so last bits may.
 * mx_conv3x3_halo_serves (host only, needs no device): the LDS bytes of the launch when ALL of these hold, else 0 -- one resolution group (n_segs 0);
 * stride 1, up 0, vhalo 0, corner_patch 0; Cin % 64 == 0, Cin <= 8192, K == 9 Cin, cin_valid 0; N % 160 == 0; image width 32 or 64; Hin Win % 256 == 0;
 * flags 0, no gate, out_scale 0, splitk <= 1; 16-byte aligned operands with ldc % 8 == 0 (and ldr % 8 == 0 with a residual); and (width, Cin, N) is
 * not one of the two shapes that did not count as faster in the per-shape A/B (profiles/conv_halo_ab.txt): (32, 640, 1280), (64, 320, 640).
 * mx_conv3x3_halo fails on a descriptor it does not serve: the caller asks first and runs mx_conv3x3 otherwise. */
int mx_conv3x3_halo_serves(const mx_gemm_desc* d);
int mx_conv3x3_halo(void* stream, const mx_gemm_desc* d);
/* The same kernel for images 128 pixels wide, where two whole rows do not fit its staged buffers: a tile is HALF a block of rows, 4 output rows x
 * 64 columns at column 0 or 64, staged like a 64-wide tile from an image whose rows are 128 pixels apart, plus the one neighbouring column of the
 * other half (6 more lines per staged buffer); the outer column is the image edge (zeros).  Same arithmetic and epilogue as mx_conv3x3_halo.
 * mx_conv3x3_halfrow_serves (host only, needs no device): the LDS bytes of the launch when the conditions of mx_conv3x3_halo_serves hold with
 * image width 128 and Hin % 4 == 0 in place of its width and Hin Win % 256 conditions (no shape is excluded by the per-shape A/B,
 * profiles/conv_halfrow_ab.txt), else 0.  mx_conv3x3_halfrow fails on a descriptor it does not serve: ask first, run mx_conv3x3 otherwise. */
int mx_conv3x3_halfrow_serves(const mx_gemm_desc* d);
int mx_conv3x3_halfrow(void* stream, const mx_gemm_desc* d);
/* Slices the K range of d is dealt to (1 = no split).  Small launches -- fewer 128-row tiles than CUs and >= 16 K tiles: one request, light mixed
 * batches -- run SPLIT-K: every output tile is computed by up to 4 workgroups over disjoint K ranges; each leaves its fp32 partial tile in a
 * library-owned scratch (96 MB + counters per stream, allocated at a stream's first split launch -- also while that stream is being captured:
 * the allocation does not touch the capturing stream) and takes a ticket; the last arriver adds the partials IN SLICE ORDER (bit-stable run to
 * run) and runs the ordinary epilogue.  The value returned is what mx_gemm / mx_conv3x3 (d) DOES: the decision depends on the descriptor alone, so a
 * shape adds its products in the same order eagerly, under capture and on replay; a scratch that cannot be allocated makes the launch fail (set
 * d->splitk = 1 to run unsplit).  Shape-based and host-only. */
int mx_gemm_splitk(const mx_gemm_desc* d, int conv);
/* frees the split-K scratch of `stream` (all != 0: of every stream) after waiting for that stream; library unload frees what is left */
void mx_gemm_release_scratch(void* stream, int all);

/* V^T key order.  The attention kernel feeds its softmax accumulator straight back to the matrix core as the
 * P operand, and that register layout interleaves keys in blocks of four (lane half h owns keys 4h..4h+3 and
 * 8+4h..8+4h+3 of every 16).  V^T is therefore stored with bits 2 and 3 of the key index swapped, so that each
 * lane's eight V^T values are one aligned 16-byte word.  MX_VT_POS is its own inverse; rows are MX_VT_LD(Lk) long.
 * mx_gemm's MX_EPI_QKV epilogue writes this order; pad positions need not be initialised. */
#define MX_VT_POS(key) (((key) & ~12) | (((key) & 4) << 1) | (((key) & 8) >> 1))
#define MX_VT_LD(Lk) (((Lk) + 15) / 16 * 16)

/* softmax(Q K^T * scale) V per (batch, head); head_dim 64.
 * q: bf16 rows (b*Lq + i), head h at columns [64h, 64h+64), row stride ldq; k likewise (Lk, ldk);
 * vt: bf16, V transposed: element (b, h, d, key) at vt[b*vt_batch_stride + (h*64 + d)*ldvt + MX_VT_POS(key)],
 *     ldvt >= MX_VT_LD(Lk) and a multiple of 8;
 * o: bf16 [B*Lq, ldo]. */
int mx_attention(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                 int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk, float scale);
/* Same, for q that the producer already multiplied by MX_ATTN_QSCALE(scale) = scale * log2(e) (mx_gemm's out_scale, or
 * mx_rmsnorm_heads' q_scale, do it in fp32 before their single rounding): the kernel then subtracts the softmax reference
 * inside the matrix core and runs ~35 % fewer vector instructions per key tile (attention.hip).  What the step plans use. */
#define MX_ATTN_QSCALE(scale) ((scale) * 1.4426950408889634f)
int mx_attention_prescaled(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                           int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk);
/* the same through the SHORT-KEY kernel whatever Lq (Lk <= 96: every wave keeps the head's K / V^T in registers);
 * mx_attention_prescaled itself takes this kernel from Lq >= 2048 and the general one below (the two differ in bf16 rounding of P) */
int mx_attention_cross_prescaled(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                 int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk);
/* Grouped form: the attention problems of all resolutions present in a mixed batch in ONE launch (see mx_gemm_seg).  The problems share the row
 * strides and the head count; each has its own batch, sequence lengths and operand bases.  One kernel serves the whole launch (chosen by the
 * longest query sequence); the arithmetic per problem is that of mx_attention_prescaled with the same kernel. */
typedef struct mx_attn_problem {
  const void* q; const void* k; const void* vt; void* o;
  int64_t vt_batch_stride;
  int B, Lq, Lk, ldvt;
} mx_attn_problem;
int mx_attention_prescaled_grouped(void* stream, const mx_attn_problem* probs, int n, int ldq, int ldk, int ldo, int H);
/* softmax(q k^T + bias[h]) v: q and the fp32 bias [H][Lq][ldb] both already multiplied by log2(e) (T5: no 1/sqrt(d) scaling, bucketed relative
 * position bias shared by all layers); ldb % 4 == 0, ldb >= Lk rounded up to 64 */
int mx_attention_prescaled_bias(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk, const float* bias, int ldb);
/* the same with the causal mask (key j counts for query i only when j <= i), Lq == Lk == L: the CLIP text encoders */
int mx_attention_prescaled_causal(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                  int64_t vt_batch_stride, void* o, int ldo, int B, int H, int L);

/* y = LayerNorm(x) * gamma + beta over the last dim C; x,y bf16 [M, C]; gamma/beta fp32 [C], or both NULL: plain (x - mean) * rstd, the
 * input of a linear whose weights carry the affine (weights folded for mx_gemm_desc.ln_stats work unchanged on it, without ln_stats) */
int mx_layernorm(void* stream, const void* x, void* y, const float* gamma, const float* beta,
                 int M, int C, float eps);

/* y = x * rsqrt(mean(x^2) + eps) * w over the last dim C (T5LayerNorm: no mean subtraction, no bias); x,y bf16 [M, C], w fp32 [C] */
int mx_rmsnorm(void* stream, const void* x, void* y, const float* w, int M, int C, float eps);

/* AdaLN modulate: y = LayerNorm(x) * (1 + scale[b]) + shift[b] (no affine), optional second output y2 with
 * (scale2, shift2) sharing the normalisation; x,y bf16 [M, C]; scale/shift fp32 rows with stride ldmod, b = row / rows_per_batch */
int mx_layernorm_mod(void* stream, const void* x, void* y, void* y2, const float* scale, const float* shift,
                     const float* scale2, const float* shift2, int ldmod, int M, int C, int rows_per_batch, float eps);
/* the same over a mixed batch: n groups of rows one after the other, group g = batches[g] samples of rows_per_batch[g] rows each; scale / shift
 * rows are per sample in group order (one launch for the image stream of all resolutions, see mx_gemm_seg) */
int mx_layernorm_mod_grouped(void* stream, const void* x, void* y, void* y2, const float* scale, const float* shift, const float* scale2,
                             const float* shift2, int ldmod, int C, float eps, const int* batches, const int* rows_per_batch, int n);
/* in-place RMSNorm over every 64-wide head of rows (b*batch_rows + row_off + i), i < rows_per_batch, of a bf16 [*, ld] matrix;
 * heads [0, heads_q) use weight wq[64], heads [heads_q, heads_total) use wk[64] (fp32) */
int mx_rmsnorm_heads(void* stream, void* x, int ld, int nbatch, int rows_per_batch, int batch_rows, int row_off,
                     int heads_total, int heads_q, const float* wq, const float* wk, float eps, float q_scale);
/* q_scale multiplies the q heads after normalisation (1 = none; MX_ATTN_QSCALE(1/8) for mx_attention_prescaled) */

/* NHWC GroupNorm (+ optional SiLU): x,y bf16 [B, H, W, C]; gamma/beta fp32 [C].
 * patch > 0 selects the reference's sliced statistics (average over patch x patch tiles of
 * per-tile mean and biased variance, norm_silu_concat.cu:361-386); 0 = exact GroupNorm.
 * workspace >= mx_groupnorm_nhwc_workspace_bytes(B, H, W, C). */
size_t mx_groupnorm_nhwc_workspace_bytes(int B, int H, int W, int C);
int mx_groupnorm_nhwc(void* stream, const void* x, void* y, const float* gamma, const float* beta,
                      int B, int H, int W, int C, int groups, float eps, int silu, int patch,
                      void* workspace);

/* The same over a channel concatenation read in place: channels [0, C1) from x ([B, H, W, C1]), channels [C1, C) from x2
 * ([B, H, W, C - C1]); y is [B, H, W, C].  Serves the up blocks' torch.cat([hidden_states, res_hidden_states], dim=1) feeding
 * norm1 (unet_2d_blocks.py via unet.py:458-462) without materialising the concatenation.  x2 == NULL: mx_groupnorm_nhwc. */
int mx_groupnorm_nhwc_cat(void* stream, const void* x, int C1, const void* x2, void* y, const float* gamma, const float* beta,
                          int B, int H, int W, int C, int groups, float eps, int silu, int patch, void* workspace);
/* GroupNorm (+SiLU) of x [B, H, W, C] from per-chunk partial sums a producing launch left (mx_gemm_desc.gn_part_out): part[(token / chunk * C + c) * 2 + {0, 1}] over
 * `chunk` consecutive tokens (chunk divides H * W), exact statistics only (no sliced form).  add_bias [C] (may be NULL) / add_rowbias [B][ldrb] (may be NULL): the
 * partial sums are those of x[.., c] - (add_bias[c] + add_rowbias[image][c]) -- the producer's bias and per-sample row bias.  Fold + apply: the statistics read
 * pass does not run.  workspace: mx_groupnorm_nhwc_workspace_bytes(B, H, W, C). */
int mx_groupnorm_nhwc_from_partials(void* stream, const void* x, void* y, const float* gamma, const float* beta, int B, int H, int W, int C, int groups, float eps,
                                    int silu, const float* part, int chunk, const float* add_bias, const float* add_rowbias, int ldrb, void* workspace);

/* Grouped form (see mx_gemm_seg): the GroupNorms of all resolutions present in a mixed batch as ONE stats / fold / apply launch each.  x2 as in
 * mx_groupnorm_nhwc_cat (all problems or none); workspace >= mx_groupnorm_nhwc_grouped_workspace_bytes(probs, n, C). */
typedef struct mx_gn_problem { const void* x; const void* x2; void* y; int B, H, W; } mx_gn_problem;
size_t mx_groupnorm_nhwc_grouped_workspace_bytes(const mx_gn_problem* probs, int n, int C);
int mx_groupnorm_nhwc_grouped(void* stream, const mx_gn_problem* probs, int n, int C1, const float* gamma, const float* beta, int C, int groups,
                              float eps, int silu, int patch, void* workspace);

/* ------------------------------------------------------------------------------------------
 * Outer boundary: the SDXL UNet in the model slot.
 * ------------------------------------------------------------------------------------------ */
typedef struct mx_unet_config {
  int in_channels, out_channels;
  int n_levels;                    /* <= 4 */
  int block_out_channels[4];
  int layers_per_block;
  int down_has_attn[4];
  int transformer_layers[4];
  int num_heads[4];                /* head_dim must be 64 */
  int cross_attention_dim;
  int addition_time_embed_dim;
  int projection_class_embeddings_input_dim;
  int norm_num_groups;
  float norm_eps, transformer_norm_eps, layer_norm_eps;
} mx_unet_config;

typedef struct mx_weight_entry {
  const char* name;   /* packed-tensor name, see sduss_amd/weights.py */
  uint64_t offset;    /* byte offset into the blob */
  uint64_t bytes;
} mx_weight_entry;

typedef struct mx_unet mx_unet;

mx_unet* mx_unet_create(const mx_unet_config* cfg);
void mx_unet_destroy(mx_unet* u);
/* the blob (device memory, packed by sduss_amd/weights.py) stays owned by the caller and must
 * outlive the handle; the table is copied */
int mx_unet_set_weights(mx_unet* u, const void* blob, uint64_t blob_bytes,
                        const mx_weight_entry* table, int n_entries);
/* PER-COMPOSITION store of the cross-attention K / V^T (round 5).  The text embeddings of a request do not change over its steps, yet the
 * reference's step re-concatenates them and every forward projects them again for all 70 transformer layers (pipeline_stable_diffusion_xl_esymred.py:
 * 287-339; attention.py:59-110 to_kv).  A caller that knows the batch composition names it before each forward: key != 0 announces that the NEXT
 * forward of this handle (ONE call: the key is consumed by it) receives encoder_hidden_states with the same CONTENT and row order as every earlier
 * forward announced with this key did (same batch, same ctx_len).  The first such forward projects into library-owned device buffers, later ones
 * read them -- the same GEMM's output, bit for bit (up to 4 compositions are kept, least recently used first out; ~26 MB per sample row at SDXL-base
 * width).  A forward that was not announced projects as before.  Applies to mx_unet_forward / _forward_mixed (not to the patch-parallel or block-cache entry points, nor under MX_GRAPH=1);
 * mx_unet_set_weights drops every stored projection.  Entries are handed between streams through events: forwards of one handle may be issued on
 * several streams, from one host thread. */
int mx_unet_set_context_key(mx_unet* u, uint64_t key);
int mx_unet_context_stats(const mx_unet* u, long* hits, long* misses);   /* forwards served from / written to the store since creation */
size_t mx_unet_workspace_bytes(const mx_unet* u, int batch, int H, int W, int ctx_len);
/* host-only walk of the step plan that resolves every packed tensor by name and size (no launches, no GPU needed) */
int mx_unet_validate(const mx_unet* u, int batch, int H, int W, int ctx_len);
/* One UNet forward over `batch` whole latents of one resolution (CFG rows included by the caller).
 *   latents  [batch, in_channels, H, W]  of `io_dtype` (NCHW, as the reference passes them)
 *   timesteps fp32 [batch]; ehs bf16 [batch, ctx_len, cross_attention_dim];
 *   text_embeds bf16 [batch, text_dim]; time_ids fp32 [batch, 6]
 *   out      [batch, out_channels, H, W] of `io_dtype`
 *   gn_patch 0 = is_sliced False (exact GroupNorm, zero-padded convs);
 *            p>0 = is_sliced True with latent patch edge p: patch-averaged GroupNorm statistics and the
 *            halo-corner rule, i.e. the same real-number arithmetic as the reference's sliced path, evaluated on whole
 *            images (not bit-for-bit: bf16 storage and fp32 statistics here, fp16 storage and fp16-rounded statistics
 *            there, norm_silu_concat.cpp:84-85; tolerance stated in tests/test_unet_gpu.py). */
int mx_unet_forward(mx_unet* u, void* stream, const void* latents, int io_dtype, const float* timesteps,
                    const void* ehs, const void* text_embeds, const float* time_ids, void* out,
                    int batch, int H, int W, int ctx_len, int gn_patch, void* workspace, size_t workspace_bytes);
/* Mixed-resolution batch (BASELINE configs[4]): the requests of EVERY resolution present run through ONE launch sequence --
 * what the reference obtains by cutting the latents of all resolutions into one batch of 256-px patches (modules/unet.py:104-185, split_sample)
 * and regrouping per latent before attention (attention.py:152-203).  Here nothing is cut: a group = the samples of one resolution, the
 * activations of a level are the groups' images one after the other, per-token ops are single launches over all rows and the ops with per-image
 * structure are grouped launches (mx_gemm_seg, mx_attention_prescaled_grouped, mx_groupnorm_nhwc_grouped).  The conditioning rows (timesteps, ehs,
 * text_embeds, time_ids) are those of all groups concatenated in group order -- the reference's row order, ascending resolution
 * (pipeline_stable_diffusion_xl_esymred.py:275-276).  Per request the arithmetic is that of mx_unet_forward on its group alone up to the tile
 * shapes a larger launch selects and the grouping of the fp32 partial sums of the GroupNorm / LayerNorm statistics. */
typedef struct mx_unet_group { const void* latents; void* out; int batch, H, W; } mx_unet_group;   /* [batch, C, H, W] of io_dtype each */
size_t mx_unet_workspace_bytes_mixed(const mx_unet* u, const mx_unet_group* groups, int n_groups, int ctx_len);
int mx_unet_forward_mixed(mx_unet* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                          const void* ehs, const void* text_embeds, const float* time_ids, int ctx_len, int gn_patch, void* workspace,
                          size_t workspace_bytes);
/* the same with a stage dump (tests): the NHWC bf16 activation of all groups after `stage`, [sum of the groups' pixels, C] */
int mx_unet_forward_mixed_trace(mx_unet* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                                const void* ehs, const void* text_embeds, const float* time_ids, int ctx_len, int gn_patch, void* workspace,
                                size_t workspace_bytes, const char* stage, void* stage_out, size_t stage_out_bytes);
/* debugging / parity: copy of the NHWC bf16 activation after the named stage of the LAST forward
 * is not kept; instead a forward can be asked to stop after `stage` and dump it (tests only). */
int mx_unet_forward_trace(mx_unet* u, void* stream, const void* latents, int io_dtype, const float* timesteps,
                          const void* ehs, const void* text_embeds, const float* time_ids, void* out,
                          int batch, int H, int W, int ctx_len, int gn_patch, void* workspace,
                          size_t workspace_bytes, const char* stage, void* stage_out, size_t stage_out_bytes);

/* ------------------------------------------------------------------------------------------
 * Patch parallelism (BASELINE.json configs[3]): ONE request's latent rows split over `world` GPUs, the bundled distrifuser
 * baseline's DistriUNetPP (distrifuser/distrifuser/distrifuser/models/distri_sdxl_unet_pp.py:15-216) in its synchronous mode
 * (every step exchanges fresh tensors; utils.py:119-214 PatchParallelismCommManager, modules/pp/{conv2d,groupnorm,attn}.py):
 *   - 3x3 convs read one boundary row of each neighbour rank (all-gather of [2][batch][W * C] per conv),
 *   - GroupNorm folds the ranks' per-(image, group) {sum, sum of squares} (all-gather of 16-byte records),
 *   - self-attention keeps its local queries and gathers the other ranks' K rows and V^T columns,
 *   - everything per-token (LayerNorm, projections, GEGLU, cross-attention, 1x1 convs) is local.
 * Rank r owns latent rows [r * H_local, (r + 1) * H_local); H_local must be divisible by 2^(levels - 1) and H_local * W / 4^level
 * a multiple of 64 at every attention level.  The collective is supplied by the caller: all_gather(ctx, stream, send, recv,
 * bytes_per_rank) must place rank k's `send` at recv + k * bytes_per_rank, ordered after prior work on `stream` and before
 * later work on it, and return 0.  sduss_amd/patch_parallel.py binds it to torch.distributed (backend "nccl" == RCCL over
 * xGMI on MI355X; gloo through host memory in the tests).  send / recv always lie inside `workspace`.
 * Results equal mx_unet_forward on the whole latent (gn_patch 0) up to the summation order of the GroupNorm statistics.
 * ------------------------------------------------------------------------------------------ */
typedef int (*mx_allgather_fn)(void* ctx, void* stream, const void* send, void* recv, size_t bytes_per_rank);
typedef struct mx_pp_comm { int rank, world; mx_allgather_fn all_gather; void* ctx; } mx_pp_comm;
size_t mx_unet_workspace_bytes_pp(const mx_unet* u, int batch, int H_local, int W, int ctx_len, int world);
/* latents_local / out_local: [batch, C, H_local, W] of io_dtype (this rank's rows, NCHW) */
int mx_unet_forward_pp(mx_unet* u, void* stream, const void* latents_local, int io_dtype, const float* timesteps, const void* ehs,
                       const void* text_embeds, const float* time_ids, void* out_local, int batch, int H_local, int W, int ctx_len,
                       const mx_pp_comm* comm, void* workspace, size_t workspace_bytes);
/* Stale-asynchronous steps: distrifuser's default mode after its warm-up (synchronous while counter <= warmup_steps: warmup_steps + 1 = 5
 * synchronous steps at the default of 4; utils.py:30-32, 180-214;
 * modules/pp/conv2d.py:97-117, attn.py:136-146, groupnorm.py:46-66).  Every exchange k of a forward owns region k of a state buffer the caller
 * keeps across steps.  A WARMUP step is a synchronous step that also leaves what it gathered in the state.  A STALE step reads, for every
 * exchange, the OTHER ranks' slots as they were sent one step earlier and its own slot fresh, and hands its fresh slot to
 * all_gather_async(ctx, stream, region, bytes_per_rank): an in-place all-gather over the `world` slots of `region` (this rank's slot is already
 * filled) that must start after the work queued on `stream` so far and may complete at any time before the NEXT forward's first launch -- the
 * caller orders that (sduss_amd/patch_parallel.py: a side stream and an event per step).  Approximate by construction: with unchanged inputs a
 * stale step reproduces the synchronous result bit for bit; otherwise it lags one step in what it sees of the other ranks' rows.
 * corrected_gn: 0 = "stale_gn" (fresh own sums beside stale remote ones), 1 = "corrected_async_gn", distrifuser's default (stale whole-image
 * moments + this rank's change, local variance where that turns negative).  distrifuser's unbiased-variance factor is not applied in either
 * mode: the synchronous arithmetic here is nn.GroupNorm's. */
#define MX_PP_SYNC 0
#define MX_PP_WARMUP 1
#define MX_PP_STALE 2
typedef int (*mx_allgather_inplace_fn)(void* ctx, void* stream, void* region, size_t bytes_per_rank);
typedef struct mx_pp_stale { void* state; size_t state_bytes; int mode; int corrected_gn; mx_allgather_inplace_fn all_gather_async; } mx_pp_stale;
size_t mx_unet_pp_state_bytes(const mx_unet* u, int batch, int H_local, int W, int ctx_len, int world);
int mx_unet_forward_pp_stale(mx_unet* u, void* stream, const void* latents_local, int io_dtype, const float* timesteps, const void* ehs,
                             const void* text_embeds, const float* time_ids, void* out_local, int batch, int H_local, int W, int ctx_len,
                             const mx_pp_comm* comm, const mx_pp_stale* stale, void* workspace, size_t workspace_bytes);
/* Host-only walk of the patch-parallel plan (no launches, no GPU): calls comm->all_gather once per exchange of a forward, in
 * order, with send / recv = (void*)(0x1000 + byte offset of the region inside the workspace). */
int mx_unet_pp_comm_plan(const mx_unet* u, int batch, int H_local, int W, int ctx_len, const mx_pp_comm* comm);
/* mx_attention_prescaled for K / V^T gathered rank-major: keys [c * key_chunk, (c + 1) * key_chunk) of batch b have their K rows at
 * k + c * k_chunk_stride + b * k_batch_stride (row stride ldk) and their V^T words at vt + c * vt_chunk_stride + b * vt_batch_stride
 * + (h * 64 + d) * ldvt + MX_VT_POS(key - c * key_chunk); key_chunk % 64 == 0, Lk % key_chunk == 0 (strides in elements). */
int mx_attention_prescaled_chunked(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                                   int64_t vt_batch_stride, void* o, int ldo, int B, int H, int Lq, int Lk, int key_chunk,
                                   int64_t k_batch_stride, int64_t k_chunk_stride, int64_t vt_chunk_stride);

/* ------------------------------------------------------------------------------------------
 * Outer boundary: the SD3.5 MMDiT in the ``transformer`` slot
 * (PatchSD3Transformer2DModel.forward, sduss/model_executor/modules/SD3Transformer.py:60-262, invoked at
 *  pipelines/stable_diffusion_3/pipeline_stable_diffusion_3_esymred.py:312-322).
 * ------------------------------------------------------------------------------------------ */
typedef struct mx_mmdit_config {
  int patch_size, in_channels, out_channels;
  int num_layers;               /* <= 64 */
  int num_attention_heads;      /* head_dim is 64 */
  int joint_attention_dim, pooled_projection_dim, pos_embed_max_size;
  int dual_attention[64];       /* 1 where the block has the second, image-only attention (SD3.5 dual_attention_layers) */
  float norm_eps;
} mx_mmdit_config;

typedef struct mx_mmdit mx_mmdit;
mx_mmdit* mx_mmdit_create(const mx_mmdit_config* cfg);
void mx_mmdit_destroy(mx_mmdit* u);
int mx_mmdit_set_weights(mx_mmdit* u, const void* blob, uint64_t blob_bytes, const mx_weight_entry* table, int n_entries);
size_t mx_mmdit_workspace_bytes(const mx_mmdit* u, int batch, int H, int W, int ctx_len);
int mx_mmdit_validate(const mx_mmdit* u, int batch, int H, int W, int ctx_len);
/* latents [batch, in_channels, H, W] of io_dtype (NCHW); timesteps fp32 [batch]; ehs bf16 [batch, ctx_len, joint_attention_dim];
 * pooled bf16 [batch, pooled_projection_dim]; out [batch, out_channels, H, W] of io_dtype */
int mx_mmdit_forward(mx_mmdit* u, void* stream, const void* latents, int io_dtype, const float* timesteps, const void* ehs,
                     const void* pooled, void* out, int batch, int H, int W, int ctx_len, void* workspace, size_t workspace_bytes);
int mx_mmdit_forward_trace(mx_mmdit* u, void* stream, const void* latents, int io_dtype, const float* timesteps, const void* ehs,
                           const void* pooled, void* out, int batch, int H, int W, int ctx_len, void* workspace,
                           size_t workspace_bytes, const char* stage, void* stage_out, size_t stage_out_bytes);

/* Mixed-resolution batch for the SD3 / SD3.5 transformer, as mx_unet_forward_mixed: group g = the samples of one resolution ([batch, C, H, W]
 * latents in, the same shape out); timesteps / encoder_hidden_states / pooled_projections are the rows of all groups in group order.  The
 * reference re-chunks the tokens of all resolutions into one batch (modules/utils.py:86-122) and regroups them per latent before attention. */
size_t mx_mmdit_workspace_bytes_mixed(const mx_mmdit* u, const mx_unet_group* groups, int n_groups, int ctx_len);
int mx_mmdit_forward_mixed(mx_mmdit* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                           const void* encoder_hidden_states, const void* pooled_projections, int ctx_len, void* workspace, size_t workspace_bytes);

/* Patch parallelism for the SD3 / SD3.5 transformer (distrifuser models/distri_sd3_transformer_pp.py:87-97: the positional embedding is taken
 * for the whole grid, then the image tokens are sliced by rank; modules/pp/attn.py:202-277: the joint attention keeps its local queries -- this
 * rank's image tokens and the text tokens -- and gathers the other ranks' image K / V; the text stream is computed by every rank).
 * Rank r owns latent rows [r * H_local, (r + 1) * H_local); (H_local / patch_size) * (W / patch_size) must be a multiple of 16.
 * Per joint block: one all-gather of the image tokens' K rows [batch][L_local][d], one of their V^T columns [batch][d][L_local] (attn2 of the
 * dual blocks: two more).  stale = NULL: every step
 * synchronous; otherwise as mx_unet_forward_pp_stale.  Equal to mx_mmdit_forward on the whole latent up to the GEMM tile selection. */
size_t mx_mmdit_workspace_bytes_pp(const mx_mmdit* u, int batch, int H_local, int W, int ctx_len, int world);
size_t mx_mmdit_pp_state_bytes(const mx_mmdit* u, int batch, int H_local, int W, int ctx_len, int world);
int mx_mmdit_forward_pp(mx_mmdit* u, void* stream, const void* latents_local, int io_dtype, const float* timesteps, const void* encoder_hidden_states,
                        const void* pooled_projections, void* out_local, int batch, int H_local, int W, int ctx_len, const mx_pp_comm* comm,
                        const mx_pp_stale* stale, void* workspace, size_t workspace_bytes);
int mx_mmdit_pp_comm_plan(const mx_mmdit* u, int batch, int H_local, int W, int ctx_len, const mx_pp_comm* comm);

/* ------------------------------------------------------------------------------------------
 * The step after the loop: the SDXL VAE decoder (AutoencoderKL.decode as post_inference calls it,
 * pipelines/stable_diffusion_xl/pipeline_stable_diffusion_xl_esymred.py:406-463).  SURVEY.md section 8f rank 2.
 * latents [batch, latent_channels, H, W] of io_dtype (NCHW, NOT yet divided by the scaling factor: 1 / scaling_factor is folded
 * into the packed post_quant_conv weight) -> images [batch, out_channels, 8H, 8W] of out_dtype in [-1, 1] (before the pipeline's
 * image_processor.postprocess).
 * ------------------------------------------------------------------------------------------ */
typedef struct mx_vae_config {
  int latent_channels, out_channels;
  int n_levels;                   /* <= 4 */
  int block_out_channels[4];      /* encoder order, e.g. 128, 256, 512, 512: the decoder walks them backwards */
  int layers_per_block;           /* the decoder has layers_per_block + 1 resnets per up block */
  int norm_num_groups;
  float norm_eps;
} mx_vae_config;
typedef struct mx_vae mx_vae;
mx_vae* mx_vae_create(const mx_vae_config* cfg);
void mx_vae_destroy(mx_vae* v);
int mx_vae_set_weights(mx_vae* v, const void* blob, uint64_t blob_bytes, const mx_weight_entry* table, int n_entries);
size_t mx_vae_workspace_bytes(const mx_vae* v, int batch, int H, int W);
int mx_vae_validate(const mx_vae* v, int batch, int H, int W);
int mx_vae_decode(mx_vae* v, void* stream, const void* latents, int io_dtype, void* out, int out_dtype, int batch, int H, int W,
                  void* workspace, size_t workspace_bytes);
/* The same decode ending in the image the client receives (image_processor.postprocess(output_type="pil"), :455): out is
 * uint8 [batch, 8H, 8W, 3] (interleaved RGB; 8 = 2^(n_levels - 1)).  The plan is mx_vae_decode's up to conv_norm_out; then one launch
 * (mx_conv3x3_rgb8 below) stands in for conv_out and the NCHW float store, so every byte is rounded once from the fp32 accumulator.
 * Needs out_channels == 3.  Sized by mx_vae_workspace_bytes as well: this path never takes more workspace than mx_vae_decode. */
int mx_vae_decode_rgb8(mx_vae* v, void* stream, const void* latents, int io_dtype, void* out, int batch, int H, int W, void* workspace,
                       size_t workspace_bytes);
/* 3x3 convolution (pad 1, stride 1) to three channels with the 8-bit image epilogue, the operator on its own (csrc/conv_rgb8.hip; not a
 * route of mx_conv3x3):
 *   x NHWC bf16 [B, H, W, Cin], Cin % 64 == 0;  w packed bf16 [4, 9 Cin] ((kh, kw, cin) order; row 3 is padding and is not read);
 *   bias fp32 [4] (entry 3 unused);  x, w and bias 16-byte aligned;  out uint8 [B, H, W, 3], contiguous.
 * Per element in fp32: y = acc + bias;  t = y * 0.5 + 0.5;  t = min(max(t, 0), 1) with NaN -> 0;  out = rint(t * 255) (half to even).
 * Rows leave as dwords when W % 4 == 0 and out is 4-byte aligned, as bytes otherwise.  Refused without a launch: null operands, sizes
 * <= 0, Cin % 64 != 0, B H W Cin >= 2^31 (32-bit source offsets), weights + one staged chunk past 64 KB of LDS. */
int mx_conv3x3_rgb8(void* stream, const void* x, const void* w, const float* bias, void* out, int B, int H, int W, int Cin);

/* ------------------------------------------------------------------------------------------
 * The step before the loop for a request that starts from an image: the VAE encoder (AutoencoderKL.encode + the posterior + the latent
 * scaling), so that image-to-image, inpainting preparation and refiner hand-offs get their starting latents from this library
 * (prepare_inference takes a request's latents from the caller: pipeline_stable_diffusion_xl_esymred.py:154-168).
 * The same handle as the decoder: its weight table may hold "encoder.*" and "quant_conv.*" tensors (sduss_amd/vae.py, pack_vae_encoder);
 * quant_conv (a padded [64, 64] linear over the moments) runs when the table names it -- SD3's AutoencoderKL has none.
 * The encoder's downsampler pads asymmetrically (F.pad(x, (0, 1, 0, 1)), stride 2, pad 0); rotated by 180 degrees that is the library's
 * stride-2 pad-1 conv, so the plan runs in the rotated orientation: the first launch reads the image backwards, every 3x3 weight is rotated
 * at pack time, the last launch reads the moments backwards ("The encoder runs rotated").
 *   image    MX_IMAGE_RGB8_HWC: uint8 [batch, H, W, 3] as a client sends it (value = 2 (u / 255) - 1 in fp32, then one rounding to bf16);
 *            MX_IMAGE_F32_CHW:  fp32 [batch, 3, H, W] in [-1, 1] (image_processor.preprocess);  H, W: image pixels, multiples of 2^(n_levels - 1)
 *   latents  [batch, latent_channels, H / f, W / f] of io_dtype, NCHW, f = 2^(n_levels - 1): (z - shift_factor) * scaling_factor with
 *            z = the posterior's mode (posterior_noise NULL) or mean + std * posterior_noise; with start_noise, then
 *            keep[b] * latents + sigma[b] * start_noise (the noise of the start step: Euler add_noise keep = 1, flow-match scale_noise keep = 1 - sigma)
 *   posterior_noise, start_noise: NCHW of io_dtype, shaped as latents, or NULL;  keep, sigma: fp32 [batch], needed with start_noise.
 * Refused without a launch: out_channels != 3, H or W not a multiple of 2^(n_levels - 1), null operands, a workspace smaller than
 * the sizing walk's answer.
 * ------------------------------------------------------------------------------------------ */
enum { MX_IMAGE_RGB8_HWC = 0, MX_IMAGE_F32_CHW = 1 };
typedef struct mx_vae_encode_args {
  const void* image;
  int image_format;               /* MX_IMAGE_* */
  const void* posterior_noise;    /* optional */
  const void* start_noise;        /* optional */
  const float* keep;              /* with start_noise */
  const float* sigma;             /* with start_noise */
  void* latents;
  int io_dtype;                   /* of latents and both noises */
  float scaling_factor, shift_factor;
} mx_vae_encode_args;
size_t mx_vae_encode_workspace_bytes(const mx_vae* v, int batch, int H, int W);
int mx_vae_encode_validate(const mx_vae* v, int batch, int H, int W);
int mx_vae_encode(mx_vae* v, void* stream, const mx_vae_encode_args* args, int batch, int H, int W, void* workspace, size_t workspace_bytes);
/* The encoder's conv_in on its own (csrc/conv_rgb_in.hip; not a route of the generic 3x3 conv): 3x3, pad 1, stride 1, the image's 3 channels -> N.
 *   image as above;  w bf16 [N, 32], column (ky 3 + kx) 3 + c for the 27 taps, columns 27..31 padding that is read as zero whatever it holds;
 *   bias fp32 [N];  y NHWC bf16 [B, H, W, N] = bf16(acc + bias), N % 16 == 0;  w, bias and y 16-byte aligned.
 *   rotate = 1: output pixel (y, x) is the conv centred on image pixel (H-1-y, W-1-x) of the image rotated by 180 degrees;  0: the plain conv.
 * Refused without a launch: null operands, sizes <= 0, N % 16 != 0, a bad format or rotate, misaligned operands, 3 B H W >= 2^31. */
int mx_conv3x3_rgb_in(void* stream, const void* image, int image_format, const void* w, const float* bias, void* y, int B, int H, int W, int N,
                      int rotate);
/* The encoder's last launch on its own (csrc/elementwise.hip): moments bf16 [B h w, ld], columns [0, lc) mean and [lc, 2 lc) logvar -> latents
 * NCHW [B, lc, h, w] of io_dtype.  Per element in fp32, each operation rounded on its own:
 *   z = mean                                                       posterior_noise NULL
 *   z = mean + expf{0.5f * min[max[logvar, -30], 20]} * eps        otherwise
 *   lat = {z - shift} * scaling;   lat = keep[b] * lat + sigma[b] * start_noise     (start_noise given: mul, mul, add)
 * rotate = 1: element (b, c, y, x) comes from moments row (h-1-y) w + (w-1-x) of image b. */
int mx_vae_latent_finish(void* stream, const void* moments, int ld, void* out, int io_dtype, int B, int lc, int h, int w, float scaling, float shift,
                         const void* posterior_noise, const void* start_noise, const float* keep, const float* sigma, int rotate);

/* ------------------------------------------------------------------------------------------
 * CLIP text encoder (csrc/clip_text.cpp): what diffusers' encode_prompt runs per prompt before the denoising loop
 * (prepare_inference, pipeline_stable_diffusion_xl_esymred.py:118-140): transformers CLIPTextModel (SDXL text_encoder: ViT-L, quick_gelu,
 * no projection) and CLIPTextModelWithProjection (text_encoder_2: OpenCLIP bigG, gelu, text_projection).  Packed weights keep the
 * transformers names except q_proj / k_proj / v_proj, fused into "<layer>.self_attn.qkv_proj.{weight [3H, H], bias [3H]}".
 *   ids: int32 [batch, max_position_embeddings] token ids (the tokenizer stays on the host);
 *   hidden_out: bf16 [batch, L, H] = transformers' hidden_states[hidden_layer] (-2 for SDXL: the output of the last-but-one layer; -1 =
 *               the last layer's output, before final_layer_norm), or NULL;
 *   pooled_out: fp32 [batch, projection_dim] = text_projection(final_layer_norm(last)[eos position]), or NULL.
 * ------------------------------------------------------------------------------------------ */
typedef struct mx_clip_config {
  int vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, max_position_embeddings;
  int hidden_act;                 /* 0 = quick_gelu, 1 = gelu (erf) */
  int projection_dim;             /* 0: no text_projection */
  int eos_token_id;               /* 2 = the legacy configs: pooled row = position of the largest id */
  int hidden_layer;               /* which hidden state hidden_out receives, a negative index as in Python: -2 (SDXL, clip_skip None), -1 ... */
  float layer_norm_eps;
} mx_clip_config;
typedef struct mx_clip mx_clip;
mx_clip* mx_clip_create(const mx_clip_config* cfg);
void mx_clip_destroy(mx_clip* c);
int mx_clip_set_weights(mx_clip* c, const void* blob, uint64_t blob_bytes, const mx_weight_entry* table, int n_entries);
size_t mx_clip_workspace_bytes(const mx_clip* c, int batch);
int mx_clip_validate(const mx_clip* c, int batch);
int mx_clip_encode(mx_clip* c, void* stream, const int32_t* ids, void* hidden_out, void* pooled_out, int batch, void* workspace,
                   size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * T5 v1.1 encoder (csrc/t5_text.cpp): SD3's text_encoder_3 (transformers T5EncoderModel, XXL: 24 blocks x 4096, 64 heads of 64, d_ff 10240,
 * gated gelu_new), run by encode_prompt on 256 token ids per prompt without an attention mask; out = last_hidden_state bf16 [batch, L, d_model].
 * Packed weights keep the transformers names except: q / k / v fused into "<block>.layer.0.SelfAttention.qkv.weight" [3 * 64 heads, d_model],
 * wi_1 | wi_0 interleaved for the GEGLU epilogue into "<block>.layer.1.DenseReluDense.wi.weight" [2 d_ff, d_model], and the relative position
 * bias of block 0 expanded for the sequence length into "encoder.position_bias.<L>" fp32 [heads, L, ceil64(L)], times log2(e)
 * (sduss_amd/t5.py::pack_t5).
 * ------------------------------------------------------------------------------------------ */
typedef struct mx_t5_config {
  int vocab_size, d_model, d_ff, num_layers, num_heads;    /* d_kv = 64 */
  float layer_norm_epsilon;
} mx_t5_config;
typedef struct mx_t5 mx_t5;
mx_t5* mx_t5_create(const mx_t5_config* cfg);
void mx_t5_destroy(mx_t5* t);
int mx_t5_set_weights(mx_t5* t, const void* blob, uint64_t blob_bytes, const mx_weight_entry* table, int n_entries);
size_t mx_t5_workspace_bytes(const mx_t5* t, int batch, int L);
int mx_t5_validate(const mx_t5* t, int batch, int L);
int mx_t5_encode(mx_t5* t, void* stream, const int32_t* ids, void* out, int batch, int L, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * Block-skip cache ("Mix-Cache"): the reference's CacheManager with ESYMRED_USE_CACHE=TRUE (modules/cache_manager.py:101-191, called at the
 * top of each of the UNet's seven blocks -- three down, mid, three up: unet_2d_blocks.py:40,102,180,250,345).  Before a block runs, every
 * sample's block input (for the up blocks also each skip tensor it consumes) is compared with the input that block saw at its last run: the
 * mean squared difference.  The host predictor sees the reference's feature rows [block index, timestep, mse (, mse of each skip: oldest skip
 * first, the first-consumed one last, as res_hidden_states_tuple is ordered: cache_manager.py:110-121)] and answers
 * run / reuse per sample; a reused block's outputs (hidden state and, for the down blocks, the skip tensors) come from the cache.
 * Approximate by design and OFF on the exact path (mx_unet_forward never consults it).
 * Granularity of THIS entry (mx_unet_forward_cached, one resolution): the SAMPLE (a request's CFG row).  A block is skipped as a whole only when
 * NO sample asks to run it (save_and_get_block_states: mask.sum() == 0, cache_manager.py:60-67); when it runs, a sample that did not ask keeps the
 * OUTPUTS the block produced for it at its last run (the block is evaluated for the whole batch and those rows are restored from the state).
 * Round 4: this sample unit is this library's own reading, kept for callers that run unsliced -- the reference has no working unsliced cache (the
 * unsliced branches of its attention hand update_and_return ALL rows together with a partial mask, attention.py:204-224, which cannot broadcast),
 * and inside a running block it does not restore block outputs: GroupNorm, LayerNorms, projections, the feed-forward and the residual paths of a
 * patch that did not ask are computed fresh and only its convolutions and attention sub-blocks reuse their own cached outputs.  That behaviour, at
 * the reference's unit (the 256-px patch, is_sliced=True) and with the compute of the not-asking patches actually skipped, is
 * mx_unet_forward_cached_mixed below; the MMDiT's is mx_mmdit_forward_cached_mixed.  The cached state belongs to one batch composition: a different
 * batch_key, batch size or latent size invalidates it (every block runs once and refills it).  Not combined with patch parallelism.
 *   predict(ctx, block, is_up, n_samples, n_feat, timesteps[n], mse[n * n_feat], run_out[n]): mse = MX_MSE_UNCACHED when the block has no
 *   cached input; return non-zero to abort the forward.  The reference's predictors are cuML random forests that are not loadable here:
 *   sduss_amd/block_cache.py ships a threshold rule with the reference's forced recompute after four reuses (cache_manager.py:134,154) and
 *   takes any object with .predict(features).
 * ------------------------------------------------------------------------------------------ */
#define MX_MSE_UNCACHED 9.2233720368547758e18f      /* float(sys.maxsize), cache_manager.py:19 */
typedef int (*mx_skip_predict_fn)(void* ctx, int block, int is_up, int n_samples, int n_feat, const float* timesteps, const float* mse,
                                  unsigned char* run_out);
/* Host-side (no GPU) evaluation of a fitted binary random forest, the form the reference's predictors have (cuML forests; here fitted with
 * scikit-learn by tools/fit_skip_predictor.py and flattened by sduss_amd/block_cache.py CompiledForest): all trees' nodes in one array, node i
 * goes to left[i] when x[feature[i]] <= threshold[i] (x in fp32, as scikit-learn evaluates), else right[i]; left[i] < 0 marks a leaf whose
 * class-1 probability is p1[i]; out[r] = mean over trees > 0.5.  A mx_skip_predict_fn built on it costs microseconds per block. */
int mx_forest_predict(const int32_t* left, const int32_t* right, const int32_t* feature, const double* threshold, const double* p1,
                      const int32_t* roots, int n_trees, const float* X, int n_rows, int n_feat, unsigned char* out);
typedef void (*mx_skip_observe_fn)(void* ctx, int block, int n_samples, const float* out_mse);
/* A flattened forest in DEVICE memory, the layout mx_forest_predict takes (sduss_amd/block_cache.py CompiledForest.to_device).  The struct itself
 * lives on the host. */
typedef struct mx_device_forest {
  const int32_t *left, *right, *feature; const double *threshold, *p1; const int32_t* roots;
  int n_trees, n_nodes, n_feat;
} mx_device_forest;
typedef struct mx_block_cache {
  mx_skip_predict_fn predict;
  void* ctx;
  void* state;                /* device memory, mx_unet_block_cache_bytes(...) bytes, kept by the caller across steps */
  size_t state_bytes;
  uint64_t batch_key;         /* in: identifies the batch composition (e.g. a hash of the request ids in row order) */
  uint64_t cached_key;        /* library-owned from here on: zero-initialise the struct once */
  int cached_valid, cached_batch, cached_h, cached_w;
  unsigned blocks_run;        /* out: bit i set = block i ran in the last forward */
  unsigned blocks_run_hi;     /* out: blocks 32..63 (MMDiT) */
  mx_skip_observe_fn observe; /* optional (NULL): after a block RAN while its previous output was cached, the per-sample mean squared difference
                                 between the new and the previous hidden-state output -- the label a predictor is fitted on (the reference's
                                 files are named for it: exp/sdxl-upsample-threshold0.01.pkl); tools/fit_skip_predictor.py */
  /* Optional: one state row per REQUEST instead of per batch position -- what the reference's dictionaries keyed by request id give
   * (cache_manager.py:105-133: a request that stays while the batch around it changes keeps its cached tensors; a new one has none and makes
   * the block run).  slots (host array [batch]): the state row of each sample, distinct, in [0, n_slots); slot_valid (host array [batch]):
   * 1 = that row holds this sample's tensors of an earlier step at this latent size.  The caller owns the request -> row table
   * (sduss_amd/block_cache.py); the state is then mx_*_block_cache_bytes(u, n_slots, ...) large and batch_key / cached_* are not consulted. */
  const int32_t* slots;
  const unsigned char* slot_valid;
  int n_slots;
  /* mx_unet_forward_cached_mixed (the patch unit): the latent size the state rows are laid out for (every group's H, W <= these; multiples of
   * gn_patch), and, out, the patches that asked / the patches seen over the blocks of the last forward */
  int max_h, max_w;
  unsigned long long patches_asked, patches_total;
  /* Opt-in, patch / chunk unit only (mx_unet_forward_cached_mixed, mx_mmdit_forward_cached_mixed): the decision taken ON THE DEVICE.  With
   * dev_down set, each block's features, forest answer, counter rule and list of asking units come from one kernel launch and the host reads back
   * only the counts that size the following launches; predict may be NULL and is never called, observe must be NULL.  dev_down decides the down
   * and mid blocks (and every MMDiT block), dev_up the up blocks (NULL: dev_down); a forest's n_feat must be 2 + the inputs of every block it
   * serves.  dev_counters (device, zeroed by the caller once): the reuse counters, laid out [block][slot][unit of the slot's max_h x max_w grid],
   * followed by the kernel's scratch; the layout follows the REQUEST (its state row), so a composition change needs no remapping, and a sample
   * with slot_valid 0 reads as zero and is overwritten.  decisions_out (optional, host): the run flags of every block of the forward, in call order
   * (units in row order).  All zero: nothing changes.  Setting dev_down on the sample-unit entries (mx_unet_forward_cached,
   * mx_mmdit_forward_cached) is an error: they keep the host decision. */
  const struct mx_device_forest* dev_down;
  const struct mx_device_forest* dev_up;
  int32_t* dev_counters;
  size_t dev_counters_bytes;  /* >= mx_skip_counters_bytes(blocks of the model, n_slots, (max_h / patch) * (max_w / patch)) */
  int forced_after;
  unsigned char* decisions_out;
} mx_block_cache;
size_t mx_unet_block_cache_bytes(const mx_unet* u, int batch, int H, int W);
int mx_unet_forward_cached(mx_unet* u, void* stream, const void* latents, int io_dtype, const float* timesteps,
                           const void* encoder_hidden_states, const void* text_embeds, const float* time_ids, void* out,
                           int batch, int H, int W, int ctx_len, int gn_patch, void* workspace, size_t workspace_bytes, mx_block_cache* cache);
/* The cache AT THE REFERENCE'S OWN UNIT -- the 256-px patch -- over a mixed-resolution batch in ONE launch sequence (round 4).  The reference's
 * cache only works with is_sliced=True (its unsliced update_and_return receives all rows with a partial mask), which is what its mixed policies
 * force (policy/FCFS_Mixed.py:69-70); every cache is keyed "<request id>-<h>-<w>" (modules/utils.py:37,60; unet.py:163).  Semantics reproduced:
 *   - per block ONE decision for the patches of all samples of all groups: predict(ctx, block, is_up, n_patches, n_feat, timesteps[n_patches],
 *     mse[n_patches * n_feat], run_out[n_patches]) -- rows in the reference's order (group, sample, patch row, patch column), mse = mean over the
 *     patch's pixels and channels of (input - cached input)^2, for the up blocks also of each skip tensor (oldest first); MX_MSE_UNCACHED for a
 *     request without cached tensors (slot_valid 0), which always runs;
 *   - a block none of whose patches asks is skipped: every output (hidden state, the down blocks' skip tensors) comes from the state;
 *   - in a running block the ops that own a CacheManager in the reference -- resnet conv1 / conv2, the down / upsampler conv, attn1's core +
 *     to_out, the whole attn2 -- are COMPUTED FOR THE ASKING PATCHES ONLY (3x3 convs on a compact batch of halo'd patches gathered with the
 *     reference's halo / corner rule, per-token work on the compact rows, self-attention of the asking queries against all keys of their latent)
 *     and every other patch takes that op's own cached output; GroupNorm (statistics, halos, SiLU), the LayerNorms, proj_in / proj_out, the
 *     q | k | v projection, the feed-forward, the 1x1 shortcut, the time-embedding add and the residual adds run on all rows, on the fresh tensors
 *     (resnet.py:390-460, 280-378; transformer.py:32-128, 167-290; attention.py:59-232; cache_manager.py:84-99).
 * State: one row per request (slots / slot_valid / n_slots as above, required), rows laid out for max_h x max_w latents;
 * mx_unet_patch_cache_bytes(u, n_slots, max_h, max_w, gn_patch) bytes.  Needs gn_patch > 0 with every group's H, W multiples of it.  The
 * workspace is larger than mx_unet_workspace_bytes_mixed (compact patch batches): mx_unet_workspace_bytes_cached_mixed.  Not graph-captured
 * (one read-back per block).  Oracle: oracle/cache_patch_ref.py; tests/test_block_cache_gpu.py. */
size_t mx_unet_patch_cache_bytes(const mx_unet* u, int n_slots, int max_h, int max_w, int gn_patch);
size_t mx_unet_workspace_bytes_cached_mixed(const mx_unet* u, const mx_unet_group* groups, int n_groups, int ctx_len, int gn_patch);
int mx_unet_forward_cached_mixed(mx_unet* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                                 const void* encoder_hidden_states, const void* text_embeds, const float* time_ids, int ctx_len, int gn_patch,
                                 void* workspace, size_t workspace_bytes, mx_block_cache* cache);
/* The same for the SD3 / SD3.5 transformer: one cache point per joint block (SD3Transformer.py:54-57, 151, 172, 219-228 with
 * cache_manager.py:163-191): the feature row is [block index, timestep, mse of the image stream]; a reused block restores both the image and
 * the context stream it produced.  The reference forces a run after TWO reuses here (cache_manager.py:184). */
size_t mx_mmdit_block_cache_bytes(const mx_mmdit* u, int batch, int H, int W, int ctx_len);
int mx_mmdit_forward_cached(mx_mmdit* u, void* stream, const void* latents, int io_dtype, const float* timesteps,
                            const void* encoder_hidden_states, const void* pooled_projections, void* out, int batch, int H, int W,
                            int ctx_len, void* workspace, size_t workspace_bytes, mx_block_cache* cache);

/* The MMDiT cache at the reference's unit over a mixed batch in ONE launch sequence (round 4).  The unit is the token CHUNK: the sliced branch cuts
 * every latent into (res / patch)^2 equal token ranges keyed "<request id>-<k>" (modules/utils.py:86-122); `patch` is that patch edge in LATENT
 * pixels (patch_size / 8 of the reference's call).  Per joint block ONE predict call for the chunks of all samples of all groups (rows: group,
 * sample, chunk; n_feat 1; forced run after two reuses is the host's, cache_manager.py:163-191); a block none of whose chunks asks takes the image
 * and the text stream from the state (SD3Transformer.py:151-228).  In a running block every op runs on all tokens except the attention
 * (attention.py:296-372, 407-415): a resolution group with no asking chunk skips its joint attention and takes attn.output's cached to_out result
 * (image tokens) and attn.encoder_output's cached to_add_out result (text tokens); a group with any asking chunk computes it whole.  The image-only
 * attn2 of the dual blocks does the same, and a group whose asking ratio is <= 1/16 renews its asking chunks only (:303-325).  State: one row per
 * request (slots / slot_valid / n_slots / max_h / max_w as for mx_unet_forward_cached_mixed).  Oracle: oracle/cache_patch_ref.CachedSlicedMMDiTRef. */
size_t mx_mmdit_patch_cache_bytes(const mx_mmdit* u, int n_slots, int max_h, int max_w, int patch, int ctx_len);
size_t mx_mmdit_workspace_bytes_cached_mixed(const mx_mmdit* u, const mx_unet_group* groups, int n_groups, int ctx_len, int patch);
int mx_mmdit_forward_cached_mixed(mx_mmdit* u, void* stream, const mx_unet_group* groups, int n_groups, int io_dtype, const float* timesteps,
                                  const void* encoder_hidden_states, const void* pooled_projections, int ctx_len, int patch, void* workspace,
                                  size_t workspace_bytes, mx_block_cache* cache);

/* The device-side decision of the patch / chunk unit (mx_block_cache.dev_down).  One statement of the rule serves both sides
 * (sduss_amd/csrc/skip_decide.h): a unit's feature is the fp64 sum of its partial sums in order / its element count, rounded to fp32
 * (MX_MSE_UNCACHED for a sample that is not valid); the row [block, timestep of the unit's sample, features] goes through the forest as in
 * mx_forest_predict; prev = uncached ? 0 : counter, forced = prev == forced_after, run = raw | forced | uncached, new counter =
 * (uncached | run) ? 0 : prev + 1; the asking units are listed in row order; first[b] = index of sample b's first asking unit, first[B] = n_ask. */
#define MX_SKIP_MAX_IN 8
size_t mx_skip_counters_bytes(int n_blocks, int n_slots, int max_units_per_slot);
/* Host twin of the kernel, for CPU tests and as the documentation of the exact semantics (no GPU needed).  forest: HOST pointers.  n units in row
 * order (unit_sample non-decreasing), n_in = forest->n_feat - 2 finalised features per unit (mse[n][n_in]; rows of a sample that is not valid are
 * ignored), counters[n]: one per unit, in / out.  ask_out[n]: the indices of the asking units, first_out[n_samples + 1]. */
int mx_skip_decide_host(const mx_device_forest* forest, int block, int forced_after, int n, int n_samples, const int32_t* unit_sample,
                        const unsigned char* sample_valid, const float* timesteps, const float* mse, int32_t* counters, unsigned char* run_out,
                        int32_t* ask_out, int32_t* first_out, int32_t* n_ask_out);
/* The kernel itself on caller-made tables (what the step plans launch once per block; tests/test_skip_decide_gpu.py).  Every pointer but `forest`
 * is device memory.  kind 0: units = patches {int32 b, py, px, pad} over samples {int64 row0; int32 h, w, slot, npx}, the counter of a patch is
 * [slot][py * grid_w + px], input i has part_len[i] partial sums per unit from partial + part_off[i] over part_elems[i] elements; kind 1: units =
 * token ranges {int64 row0; int32 rows, slot, srow0} with unit_sample naming their sample, counter [slot][srow0 / rows], 64 partial sums per unit
 * over rows * part_elems[0] elements.  record (int32 [MX_SKIP_REC_FIRST + n_samples + 1]): status (non-zero: the forest points outside itself),
 * n_ask, asking and total units per group (sample_group, optional), first[].  ask_units (kind 0, optional): the asking patches, in order. */
#define MX_SKIP_REC_STATUS 0
#define MX_SKIP_REC_NASK 1
#define MX_SKIP_REC_GASK 2
#define MX_SKIP_REC_GTOT (2 + MX_MAX_SEGS)
#define MX_SKIP_REC_FIRST (2 + 2 * MX_MAX_SEGS)
typedef struct mx_skip_decide_args {
  const mx_device_forest* forest;
  int block, forced_after, n, n_samples, n_in, kind;
  const void* units; const void* samples;
  const int32_t* unit_sample; const int32_t* sample_group;
  const unsigned char* sample_valid; const float* timesteps;
  const double* partial; int64_t part_off[MX_SKIP_MAX_IN]; int part_len[MX_SKIP_MAX_IN]; double part_elems[MX_SKIP_MAX_IN];
  int32_t* counters; int units_per_slot, grid_w, n_counters;     /* this block's row of the counters and its length */
  unsigned char* run; void* ask_units; int32_t* ask_index; int32_t* record;
} mx_skip_decide_args;
int mx_skip_decide_device(void* stream, const mx_skip_decide_args* args);

/* ------------------------------------------------------------------------------------------
 * Block-skip cache kernels, one launch each (tests and tools).  The step plans call the launchers of sduss_amd/csrc/patch_cache.hip and
 * elementwise.hip directly; these wrappers start exactly one of them on caller-made tables, so that every kernel that moves the cache's
 * state can be checked alone (tests/test_cache_move_gpu.py).  Every pointer is device memory, activations and state are bf16 with C % 8 == 0
 * (16-byte vectors).  Nothing is allocated, copied or synchronised inside a call.  Returns 0, or 1 with the reason in the last error (a null
 * operand, a shape the launcher refuses, a failed launch).
 *
 * Geometry: samples are described at LEVEL 0 (latent resolution) and every call takes the level of its tensor: image (h >> level) x
 * (w >> level), first row row0 >> 2 level, patch edge p0 >> level.  A state tensor holds one row of state_row_elems elements per REQUEST; a
 * sample's row is its slot.  Batch tensors are NHWC / token-major with the samples' images one after the other.
 * ------------------------------------------------------------------------------------------ */
typedef struct mx_pc_sample { long long row0; int h, w, slot, npx; } mx_pc_sample;   /* first level-0 row, latent size, state row, patches per image row */
typedef struct mx_pc_patch { int b, py, px, pad; } mx_pc_patch;                      /* sample, patch row, patch column */
typedef struct mx_pc_range { long long row0; int rows, slot, srow0; } mx_pc_range;   /* batch rows [row0, row0 + rows) <-> rows [srow0, ...) of state row `slot` */
/* Every sample's image between the batch tensor and its state row.  to_batch = 0: state <- batch.  to_batch = 1: batch <- state, optionally
 * (fp32, one rounding to bf16) + vec[i][c] (gate = 0) or * vec[i][c] (gate = 1) with i the sample's POSITION in the table and ldvec floats
 * between positions, then + residual (a batch tensor).  max_image_elems: elements of the largest image at this level (sizes the grid). */
int mx_pc_image_copy(void* stream, void* batch, void* state, const mx_pc_sample* samples, int n_samples, int level, int C, int64_t state_row_elems,
                     int to_batch, const float* vec, int ldvec, const void* residual, int64_t max_image_elems, int gate);
/* batch <- bf16(state + residual) token row by token row, with the statistics of the stored values: stats1[m][8] floats, of which [0..1] =
 * (sum, sum of squares) are written, and / or fin[m][2] = (mean, rsqrt(max(var, 0) + eps)); m = the row of the batch tensor. */
int mx_pc_rows_load_stats(void* stream, void* batch, const void* state, const mx_pc_sample* samples, int n_samples, int level, int C,
                          int64_t state_row_elems, const void* residual, float* stats1, float* fin, float eps, int64_t max_image_rows);
/* The listed patches of a whole-image tensor (row stride ld_src >= C) -> dst [n][P][P][C], P = p + halo_lo + halo_hi: the patch, halo rows from
 * the vertical neighbours, halo columns AND corners from the horizontal neighbour's pixel of the patch's own first / last row, zeros at the
 * image border; (halo_lo, halo_hi) = (0, 0), (1, 1) or (2, 0), the last with an outer ring of zeros in front; up = 1: src holds the image at
 * half the size and is read through a nearest 2x upsample (p is the patch edge AFTER it). */
int mx_pc_gather(void* stream, const void* src, int ld_src, int C, void* dst, const mx_pc_patch* list, int n, const mx_pc_sample* samples, int level,
                 int p, int halo_lo, int halo_hi, int up);
/* src [n][Ps][Ps][C]: the p x p pixels from (o0, o0) of every compact patch -> the patch's place in its request's state row */
int mx_pc_scatter(void* stream, const void* src, int Ps, int o0, int C, void* state, int64_t state_row_elems, const mx_pc_patch* list, int n,
                  const mx_pc_sample* samples, int level, int p);
/* the listed patches of a whole-image batch tensor -> their places in the state rows */
int mx_pc_patch_store(void* stream, const void* batch, void* state, int64_t state_row_elems, int C, const mx_pc_patch* list, int n,
                      const mx_pc_sample* samples, int level, int p);
/* partial[patch][row] (n * p doubles) = sum over the patch's pixel row of (x - state)^2 */
int mx_pc_patch_sq_diff(void* stream, const void* x, const void* state, int64_t state_row_elems, int C, const mx_pc_patch* list, int n,
                        const mx_pc_sample* samples, int level, int p, double* partial);
/* token ranges between a batch tensor and state rows (to_batch = 1: batch <- state); max_range_elems sizes the grid */
int mx_pc_range_copy(void* stream, void* batch, void* state, int64_t state_row_elems, int C, const mx_pc_range* ranges, int n, int to_batch,
                     int64_t max_range_elems);
/* partial[range][64]: the range's rows * C / 8 vectors are cut into 64 chunks of ceil(vectors / 64); each gets its sum of (x - state)^2 */
int mx_pc_range_sq_diff(void* stream, const void* x, const void* state, int64_t state_row_elems, int C, const mx_pc_range* ranges, int n,
                        double* partial);
/* The per-request pair (elementwise.hip).  partial[i][64] = the chunk sums of (a[i] - b[slot ? slot[i] : i])^2 over rows of elems_per_sample. */
int mx_sq_diff_partial(void* stream, const void* a, const void* b, int64_t elems_per_sample, int n_samples, double* partial, const int32_t* slot);
/* rows of bytes_per_sample (a multiple of 16): scatter = 1: slotted[slot[i]] <- batch[i]; 0: batch[i] <- slotted[slot[i]]; slot[i] < 0: not touched */
int mx_copy_rows(void* stream, void* batch, void* slotted, size_t bytes_per_sample, int n_samples, const int32_t* slot, int scatter);

/* ------------------------------------------------------------------------------------------
 * Glue kernels, one launch each (tests and tools).  The step plans call the launchers of sduss_amd/csrc/elementwise.hip directly; these
 * wrappers start exactly one of them on caller-made operands, so that every kernel at a model's boundary can be checked alone
 * (tests/test_glue_gpu.py).  Every pointer is device memory; `dtype` is an io dtype code (MX_F32, MX_F16, MX_BF16), every other activation is
 * bf16.  Nothing is allocated, copied or synchronised inside a call.  Returns 0, or 1 with the reason in the last error: a null operand
 * (only `pos` of mx_clip_embed may be null), an empty shape, a shape the launcher refuses, a pointer that is not 16-byte aligned where the
 * kernel moves 16-byte vectors (mx_prep_latent's out, mx_crop_pos, mx_softmax_rows, mx_clip_embed, mx_clip_pool), a failed launch.
 * ------------------------------------------------------------------------------------------ */
/* in NCHW [B][Cin][HW] of `dtype` -> out NHWC bf16 [B * HW][CP], channels Cin..CP written as +0; CP % 8 == 0, Cin <= CP */
int mx_prep_latent(void* stream, const void* in, int dtype, void* out, int B, int Cin, int HW, int CP);
/* in NHWC bf16 [B * HW][ld], the first C <= ld columns -> out NCHW [B][C][HW] of `dtype` (one rounding from the bf16 value) */
int mx_nhwc_to_nchw(void* stream, const void* in, void* out, int dtype, int B, int C, int HW, int ld);
/* Timesteps(dim, flip_sin_to_cos = True, downscale_freq_shift = 0) = [cos | sin](t exp(-ln(1e4) j / (dim / 2))), rounded once to bf16:
 * tsin [B][d0] of timesteps [B]; addin [B][text_dim + 6 da] = [text_embeds [B][text_dim] (copied) | the da-wide sinusoid of each of the 6
 * time_ids [B][6]].  d0 and da even. */
int mx_time_embed(void* stream, const float* timesteps, const void* text_embeds, const float* time_ids, void* tsin, void* addin, int B, int d0,
                  int text_dim, int da);
/* out [B][dim] bf16 = the same sinusoid of t [B]; dim even */
int mx_sinus_embed(void* stream, const float* t, void* out, int B, int dim);
/* in NCHW [B][C][H][W] of `dtype` -> out bf16 [B * (H / ps) * (W / ps)][ps * ps * C], column (dy * ps + dx) * C + c; H % ps == W % ps == 0 */
int mx_patchify(void* stream, const void* in, int dtype, void* out, int B, int C, int H, int W, int ps);
/* in bf16 [B * (H / ps) * (W / ps)][ld], the first ps * ps * C <= ld columns in (p, q, c) order -> out NCHW [B][C][H][W] of `dtype`
 * ("nhwpqc->nchpwq") */
int mx_unpatchify(void* stream, const void* in, void* out, int dtype, int B, int C, int H, int W, int ps, int ld);
/* table bf16 [m][m][d] -> out [h * w][d]: rows (top + y, left + x), top = (m - h) / 2, left = (m - w) / 2 rounded down; d % 8 == 0, h, w <= m */
int mx_crop_pos(void* stream, const void* table, void* out, int m, int h, int w, int d);
/* scores bf16 [rows][ld]: the first L columns of every row <- their softmax (fp32 math, the row maximum subtracted, one rounding), in place;
 * columns L..ld are neither read nor written; L % 8 == ld % 8 == 0 */
int mx_softmax_rows(void* stream, void* scores, int64_t rows, int L, int64_t ld);
/* out bf16 [rows][H] = tok[clamp(ids[r], 0, vocab - 1)] + pos[r % L] (fp32 sum of the two bf16 rows, one rounding); pos == NULL: no position
 * table (the sum's second operand is +0); H % 8 == 0 */
int mx_clip_embed(void* stream, const int32_t* ids, const void* tok, const void* pos, void* out, int rows, int L, int H, int vocab);
/* out bf16 [B][H] = x[b][e(b)], x [B][L][H]; e(b) = the first position of ids [B][L] holding eos_id, 0 where none does; eos_id < 0: the first
 * position of the largest id; H % 8 == 0 */
int mx_clip_pool(void* stream, const int32_t* ids, const void* x, void* out, int B, int L, int H, int eos_id);

/* ------------------------------------------------------------------------------------------
 * The element-wise steps either side of the model call.
 * ------------------------------------------------------------------------------------------ */
/* out[b] = x[b mod n_lat] / sqrt(sigma[b mod n_lat]^2 + 1) for b in [0, n_rows)   (batch_scale_model_input, CFG
 * duplication of the latents fused: n_rows = 2*n_lat under CFG, pipeline_..._esymred.py:327) */
int mx_euler_scale_input(void* stream, const void* latents, void* out, const float* sigma,
                         int n_lat, int n_rows, int64_t elems_per_latent, int dtype);
/* latents <- latents + ((u + g (t - u))) * (sigma_next - sigma), fp32 math, stored in `dtype`
 * noise: [2*n_lat, elems] = [uncond..., cond...] (guidance > 0) ; epsilon-prediction Euler step */
int mx_cfg_euler_step(void* stream, const void* noise, void* latents, const float* sigma, const float* sigma_next,
                      float guidance_scale, int n_lat, int64_t elems_per_latent, int dtype);

/* latents <- latents + (sigma_next - sigma) * (u + g (t - u))   (FlowMatchEulerDiscreteScheduler.batch_step,
 * schedulers/scheduling_flow_match_euler_discrete.py:159-202; CFG combine pipeline_stable_diffusion_3_esymred.py:365-367) */
int mx_cfg_flow_step(void* stream, const void* noise, void* latents, const float* sigma, const float* sigma_next,
                     float guidance_scale, int n_lat, int64_t elems_per_latent, int dtype);

/* The same two steps on the WORLD GATHER of the split-batch patch parallelism (sduss_amd/patch_parallel.py; distrifuser
 * models/distri_sdxl_unet_pp.py:135-171, distri_sd3_transformer_pp.py:242-278), read where it lies: no concatenation into a [2 n, C, H, W] tensor.
 *   gathered [2 * n_slabs][n_lat][C][H / n_slabs][W] of `dtype`: slot k < n_slabs holds the unconditional prediction of latent rows
 *            [k * H / n_slabs, (k + 1) * H / n_slabs), slot n_slabs + k the conditional prediction of the same rows (rank-major: the ranks of the
 *            unconditional half of the world first).  With guidance_scale <= 0 only the first n_slabs slots are read (the plain prediction).
 *   latents  [n_lat][C][H][W] of `dtype`, updated in place.
 * Per element the operations are those of mx_cfg_euler_step / mx_cfg_flow_step in the same order (one device function serves both), so the
 * result equals, bit for bit, re-assembling the gather and calling them; n_slabs == 1 is their `noise` layout.  Any positive sizes with
 * H % n_slabs == 0; everything else is an error and nothing is launched.  16-byte accesses where both buffers are 16-byte aligned and
 * (H / n_slabs) * W elements are a whole number of them, element accesses otherwise. */
int mx_cfg_euler_step_rows(void* stream, const void* gathered, void* latents, const float* sigma, const float* sigma_next,
                           float guidance_scale, int n_lat, int C, int H, int W, int n_slabs, int dtype);
int mx_cfg_flow_step_rows(void* stream, const void* gathered, void* latents, const float* sigma, const float* sigma_next,
                          float guidance_scale, int n_lat, int C, int H, int W, int n_slabs, int dtype);

/* ------------------------------------------------------------------------------------------
 * Inpainting (sduss_amd/csrc/scheduler_step.hip for the masked step, inpaint.hip for the rest): repaint the masked part of an image, keep the rest.  diffusers' 4-channel rule of
 * StableDiffusionXLInpaintPipeline / StableDiffusion3InpaintPipeline, which needs no 9-channel UNet: after every scheduler step
 *     init_proper = add_noise / scale_noise(image_latents, noise, t_next);   latents = (1 - mask) * init_proper + mask * latents.
 * ------------------------------------------------------------------------------------------ */
/* The inpainting rows of one masked step launch.  Plain and inpainting requests step together: row r of the latents is an inpainting row when
 * slot[r] is in [0, k), and then reads row slot[r] of init / noise / mask.  The slots live in device memory, where the host cannot check them: any
 * other value (-1 by convention) makes a plain row and is never used as an index. */
typedef struct {
  int k;                 /* inpainting rows in this launch; 0 = none (the four pointers are then not read) */
  const int* slot;       /* device int32 [n_lat]: row -> index in [0, k), or -1 for a plain row */
  const void* init;      /* [k, C, hw] of dtype: the image's clean latents */
  const void* noise;     /* [k, C, hw] of dtype: the request's fixed N(0,1) noise */
  const uint8_t* mask;   /* [k, hw]: non-zero = repaint, 0 = keep */
} mx_inpaint_rows;
/* mx_cfg_euler_step / mx_cfg_flow_step with the kept region put back in the same launch.
 *   noise_pred [2 n_lat | n_lat][C][hw] of `dtype` as for the plain steps (guidance_scale <= 0 reads the first n_lat rows only);
 *   latents    [n_lat][C][hw] of `dtype`, in place; sigma, sigma_next fp32 [n_lat].
 * Per element of row r the stepped value is the plain step's, by the same device functions in the same order (sduss_amd/csrc/step_math.h), so a
 * launch with k = 0 or no slot in [0, k) leaves the bits of the plain step.  Where j = slot[r] is in [0, k) and mask[j][p] == 0 the element becomes
 *     keep * init[j][c][p] + sigma_next[r] * noise[j][c][p]      keep = 1 (Euler: EulerDiscreteScheduler.add_noise), 1 - sigma_next[r] (flow: scale_noise)
 * instead: two fp32 products and one sum, each rounded on its own, one rounding to `dtype` at the store; the mask is binary, so the selection equals
 * (1 - m) a + m b for finite values.  After the last step (sigma_next = 0) that is init itself (a -0 of init may come back as +0).
 * Refused, with nothing launched: a null operand or `rows`, a non-positive size, a bad dtype, k < 0, k > 0 with a null slot / init / noise / mask.
 * Offsets are 64-bit.  16-byte accesses when latents, noise_pred, init and noise are 16-byte aligned, the mask is aligned to the elements of a
 * vector and hw is a whole number of vectors (a vector then lies in one plane and its mask bytes are one load); element accesses otherwise. */
int mx_cfg_euler_step_masked(void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                             int n_lat, int C, int hw, int dtype, const mx_inpaint_rows* rows);
int mx_cfg_flow_step_masked(void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                            int n_lat, int C, int hw, int dtype, const mx_inpaint_rows* rows);
/* out[r][e] = keep[r] * init[r][e] + sigma[r] * noise[r][e] for n rows of `elems` elements of `dtype`; keep, sigma fp32 [n].  The arithmetic of the kept
 * region above (one device function): a request's starting latents from its clean latents as they are stored, i.e. already rounded to `dtype`.
 * Refused: a null operand, a non-positive size, a bad dtype, out == init or out == noise.  16-byte accesses when the three tensors are 16-byte aligned
 * and elems is a whole number of vectors, element accesses otherwise. */
int mx_inpaint_renoise(void* stream, const void* init, const void* noise, void* out, const float* keep, const float* sigma, int n, int64_t elems,
                       int dtype);
/* A client's mask on the latent grid: mask uint8 [B][H][W] -> out uint8 [B][H / f][W / f], out[b][y][x] = mask[b][f y][f x] >= 128 (1 = repaint, 0 = keep).
 * diffusers' mask processor: binarise at 0.5 of 255 (exact on bytes: 127 -> 0, 128 -> 1), then the nearest interpolation to the latent grid, which for an
 * integer factor takes source pixel (f y, f x).  Refused: a null operand, a non-positive size, H or W no multiple of f. */
int mx_mask_to_latent(void* stream, const uint8_t* mask, uint8_t* out, int B, int H, int W, int f);
/* Outside the mask the client gets its own pixels back, not their VAE round trip: decoded uint8 [B][H][W][3] in place, pixel (b, y, x) becomes
 * original's where mask[b][y][x] < 128 (original uint8 [B][H][W][3], mask uint8 [B][H][W], the full-resolution mask as the client sent it).  Any H, W.
 * Dword accesses over whole groups of four pixels when the three bases are 4-byte aligned, bytes otherwise and for the pixels past the last group.
 * Refused: a null operand, a non-positive size, decoded == original. */
int mx_rgb8_paste(void* stream, uint8_t* decoded, const uint8_t* original, const uint8_t* mask, int B, int H, int W);

/* ------------------------------------------------------------------------------------------
 * Second-order multistep samplers (sduss_amd/csrc/scheduler_step.hip, sampler_coeffs.cpp): DPM-Solver++ 2M for the epsilon model and the second-order
 * Adams-Bashforth step (AB2) for both models, beside the model's own Euler step in ONE launch over a batch whose requests use different samplers.
 * Both are linear in the latent x, this step's quantity D and the previous step's D:
 *     x_next = cx * x + c0 * D + c1 * D_prev        D = x - sigma * m  (the data prediction, DPM-Solver++)   or   D = m  (the derivative, AB2)
 * with m the guided model output.  The latents keep the Euler scaling (k-diffusion's variance-exploding form of sample_dpmpp_2m, equal to diffusers'
 * variance-preserving DPMSolverMultistepScheduler: dpmsolver++, order 2, midpoint, lower_order_final), so mx_euler_scale_input, the start noise of
 * image-to-image and the re-noising of inpainting are unchanged.  The three coefficients of every step are made on the host (mx_sampler_coeffs).
 * ------------------------------------------------------------------------------------------ */
enum { MX_SAMPLER_EULER = 0, MX_SAMPLER_DPMPP_2M = 1, MX_SAMPLER_AB2 = 2 };
/* The multistep rows of one step launch.  Everything lives in device memory. */
typedef struct {
  const int*   kind;   /* device int32 [n_lat]: 0 = the model's Euler step, 1 = multistep on D = x - sigma*m, 2 = multistep on D = m; anything else = 0 */
  const float* coef;   /* device fp32 [n_lat][3]: cx, c0, c1 of this step (read for kind 1 / 2 only) */
  float*       hist;   /* device fp32 [n_lat][C][hw]: D of each row's previous step, read where c1 != 0, then overwritten with this step's D (kind 1 / 2 only) */
} mx_multistep_rows;
/* One scheduler step over rows of different samplers, with the kept region of inpainting rows put back in the same launch.
 *   noise_pred, latents, sigma, sigma_next, guidance_scale, n_lat, C, hw, dtype: as for mx_cfg_euler_step_masked; flow != 0 selects the flow-match
 *   Euler step for kind-0 rows and the flow keep factor 1 - sigma_next of the kept region.
 * Per element of row r, in fp32 with one rounding per operation (no contraction), m = the CFG combine of mx_cfg_euler_step:
 *   kind 0 (and any kind other than 1 or 2): the Euler / flow step by the device functions of the plain steps: their bits; hist is not touched.
 *   kind 1: D = x - (sigma*m);   kind 2: D = m;   acc = (cx*x) + (c0*D);   where c1 != 0: acc = acc + (c1*hist);   latent = acc rounded once to
 *   `dtype`;   hist = D (fp32).  hist is not read where c1 == 0: on a request's first step it holds uninitialised memory.
 *   An inpainting row (`inpaint`: NULL or k = 0 for none) then takes keep * init + sigma_next * noise where its mask is 0, exactly as
 *   mx_cfg_*_step_masked; hist receives D there too (diffusers does not mask its model_outputs either).
 * Refused, with nothing launched: a null operand, `ms` or member of it, a non-positive size, a bad dtype, hist aliasing latents or noise_pred,
 * an `inpaint` with k < 0 or with k > 0 and a null member.  Offsets are 64-bit.  16-byte accesses when latents, noise_pred, hist (and init, noise;
 * the mask to a vector's elements) are 16-byte aligned and hw is a whole number of vectors -- a vector of 8 bf16 / f16 elements is two 16-byte
 * accesses of hist -- element accesses otherwise. */
int mx_cfg_multistep_step(void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                          int n_lat, int C, int hw, int dtype, int flow, const mx_multistep_rows* ms, const mx_inpaint_rows* inpaint /* NULL or k = 0: none */);
/* The coefficients of every step of a schedule, on the host (plain C++, double arithmetic rounded to float once; no GPU needed).
 *   sigmas [n_steps + 1], strictly decreasing, non-negative, the last may be 0;   out [n_steps][4] = (cx, c0 first order, c0 second order, c1 second
 *   order) of the step from s = sigmas[i] to sn = sigmas[i + 1].  A row steps second order when it holds the previous step's D, first order otherwise;
 *   step 0 has no second order: its last two entries repeat the first-order ones with c1 = 0.
 * MX_SAMPLER_DPMPP_2M (flow = 0 only): lambda(sigma) = -log sigma, h = lambda(sn) - lambda(s), E = -expm1(-h), cx = sn / s; first order c0 = E;
 *   second order with r = (lambda(s) - lambda(sigmas[i - 1])) / h: c0 = E (1 + 1 / (2 r)), c1 = -E / (2 r).  Where sn == 0 the step is first order
 *   whatever came before, (0, 1, 1, 0): the result is the data prediction itself (diffusers' lower_order_final with final_sigmas_type "zero",
 *   k-diffusion's sigmas[i + 1] == 0 rule).  Refused for flow = 1: lambda is -infinity at sigma = 1, and on the analytic Gaussian problem the
 *   sampler is worse than Euler on the flow schedule at every step count.
 * MX_SAMPLER_AB2 (both models): h = sn - s, cx = 1; first order c0 = h (the Euler step); second order with w = h / (2 (s - sigmas[i - 1])):
 *   c0 = h (1 + w), c1 = -h w.  The final step stays second order.
 * Returns 0; non-zero, with the reason in the last error, for a null table, n_steps < 1, sigmas not strictly decreasing, a negative sigma, an
 * unknown sampler or MX_SAMPLER_EULER (which has no coefficients). */
int mx_sampler_coeffs(int sampler, int flow, const float* sigmas, int n_steps, float* out);

/* ------------------------------------------------------------------------------------------
 * Seeded requests and stochastic samplers (sduss_amd/csrc/noise.h, noise.hip, scheduler_step.hip, sampler_coeffs.cpp).  A request's noise is a pure
 * function of (seed, purpose, step, element index within the request): Philox4x32-10 with the Random123 constants (multipliers 0xD2511F53,
 * 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), key = (seed low, seed high), counter = (q low, q high, step, domain) with q = idx >> 2 and idx
 * the element's index in the request's OWN [C, h, w] tensor -- never the batch's; element idx takes normal idx & 3 of its group.  From the output
 * words (w0, w1, w2, w3):  u = (2 (w0 >> 9) + 1) 2^-24 in (0, 1),  t2 = (2 (w1 >> 9) + 1) 2^-23 in (0, 2),  r = sqrtf(-2 logf(u)),
 * z0 = r cospif(t2),  z1 = r sinpif(t2);  (w2, w3) give (z2, z3) the same way.  The image of a seeded request therefore does not depend on its row
 * in a batch or on who it is batched with, and a rewound request (step index reset) reproduces itself.
 * ------------------------------------------------------------------------------------------ */
enum { MX_NOISE_INIT = 0, MX_NOISE_START = 1, MX_NOISE_STEP = 2, MX_NOISE_POSTERIOR = 3 };   /* the domain: what the noise is for */
/* out [n][elems] of `dtype` = scale[r] * z(seed[r], step[r], domain, i): one fp32 multiply, rounded once to `dtype` at the store (scale NULL: 1).
 * seed device uint64 [n], step device uint32 [n], scale device fp32 [n] or NULL.  raw = 1: out is uint32 [n][elems] and holds the Philox words
 * themselves (word idx & 3 of group idx >> 2; dtype and scale ignored), so that the integer half can be held bit for bit.  16-byte stores where out
 * is 16-byte aligned and elems a whole number of vectors, element stores otherwise; offsets are 64-bit.  Refused: a null out, seed or step, a
 * non-positive size, a negative domain, a bad dtype, raw other than 0 / 1. */
int mx_noise_fill(void* stream, void* out, int dtype, int n, int64_t elems, const uint64_t* seed, const uint32_t* step, int domain,
                  const float* scale, int raw);
/* The noise rows of one stochastic step launch.  Everything lives in device memory. */
typedef struct {
  const float*    cn;     /* device fp32 [n_lat]: the noise coefficient of this step; 0 = no noise for the row */
  const uint64_t* seed;   /* device [n_lat]: the request's seed (read where cn != 0 on a kind-1 / kind-2 row only) */
  const uint32_t* step;   /* device [n_lat]: the request's step index, the counter's step word (read like seed) */
} mx_noise_rows;
/* mx_cfg_multistep_step with noise: a kind-1 or kind-2 row with cn[r] != 0 takes, behind acc of the multistep update, acc = acc + (cn * z), both
 * operations rounded on their own, z = the noise function at domain MX_NOISE_STEP and idx = the element's index in its row -- made in registers, no
 * noise tensor exists.  A row with cn == 0 and every kind-0 row read neither seed nor step, run no generator and leave the bits of
 * mx_cfg_multistep_step; the put-back of inpainting rows follows as there.  A 16-byte vector of 8 sixteen-bit elements is two Philox calls, one of 4
 * fp32 elements is one, the element path makes one per element.  nz NULL: mx_cfg_multistep_step itself.  Refused, with nothing launched: everything
 * mx_cfg_multistep_step refuses, and a non-null nz with a null member. */
int mx_cfg_stochastic_step(void* stream, const void* noise_pred, void* latents, const float* sigma, const float* sigma_next, float guidance_scale,
                           int n_lat, int C, int hw, int dtype, int flow, const mx_multistep_rows* ms, const mx_inpaint_rows* inpaint,
                           const mx_noise_rows* nz);
/* The stochastic samplers' coefficients on the host: both step as kind-1 rows (D = x - sigma m) of mx_cfg_stochastic_step. */
enum { MX_SAMPLER_EULER_A = 3, MX_SAMPLER_DPMPP_2M_SDE = 4 };
/* mx_sampler_coeffs with a fifth column: out [n_steps][5] = (cx, c0 first order, c0 second order, c1 second order, cn); double arithmetic, each
 * rounded to float once.  sampler: any of mx_sampler_coeffs' (cn = 0; eta is not used) or
 * MX_SAMPLER_EULER_A (k-diffusion's sample_euler_ancestral): su = min(sn, eta sqrt(sn^2 (s^2 - sn^2) / s^2)), sd = sqrt(sn^2 - su^2); cx = sd / s,
 *   c0 = 1 - sd / s (both orders), c1 = 0, cn = su.
 * MX_SAMPLER_DPMPP_2M_SDE (sample_dpmpp_2m_sde, midpoint): h as for MX_SAMPLER_DPMPP_2M, E = -expm1(-h - eta h), cx = (sn / s) exp(-eta h); first
 *   order c0 = E; second order c0 = E (1 + 1 / (2 r)), c1 = -E / (2 r); cn = sn sqrt(-expm1(-2 eta h)).  The code is MX_SAMPLER_DPMPP_2M's: at
 *   eta = 0 the first four columns are that sampler's bits and cn = 0.
 * Both: sn == 0 gives (0, 1, 1, 0, 0).  Refused: what mx_sampler_coeffs refuses, eta < 0 (or NaN), and flow = 1 for the two stochastic samplers. */
int mx_sampler_coeffs_eta(int sampler, int flow, const float* sigmas, int n_steps, double eta, float* out);

/* ------------------------------------------------------------------------------------------
 * Resize of a client's 8-bit image or mask to the request's resolution (sduss_amd/csrc/image_resize.hip, resize_coeffs.cpp), bit-equal to
 * Pillow's Image.resize for modes "RGB" and "L" -- what diffusers' VaeImageProcessor.preprocess does in front of the VAE, and its mask
 * processor in front of the binarisation.  Pillow's 8-bit resampler (ImagingResample) is integer arithmetic on integer coefficient tables:
 *   per axis, scale = in / out, fs = max(scale, 1), support = filter_support * fs, and per output index xx (all in double, int() truncates)
 *     center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in), n = xmax - xmin,
 *     w[j] = filter((j + xmin - center + 0.5) * (1 / fs)) for j < n, ww = sum of w[j] in index order, w[j] /= ww when ww != 0,
 *     k[j] = int(w[j] * 2^22 +- 0.5) (- for negative w);
 *   one output byte = clip(((1 << 21) + sum_j src[xmin + j] * k[j]) >> 22, 0, 255), int32 sum, arithmetic shift;
 *   horizontal first into bytes, then vertical over those bytes; a pass whose in == out is skipped; channels are independent.
 * The filter values double as PIL.Image.Resampling's.
 * ------------------------------------------------------------------------------------------ */
#define MX_RESIZE_LANCZOS 1     /* sinc(x) sinc(x / 3) on -3 <= x < 3, support 3 */
#define MX_RESIZE_BILINEAR 2    /* support 1 */
#define MX_RESIZE_BICUBIC 3     /* a = -0.5, support 2 */
#define MX_RESIZE_PRECISION_BITS 22
#define MX_RESIZE_MAX_SIZE (1 << 24)
/* One axis' tables on the host, no GPU needed: bounds[out][2] = (xmin, n) and k[out][ksize] with ksize = 2 * ceil(support) + 1 (entries past n are
 * zero); `cap` = the int32 entries k holds.  Returns ksize; with bounds == k == NULL that is all it does (the size query).  Returns -1, with
 * the reason in the last error, for a size outside [1, MX_RESIZE_MAX_SIZE], an unknown filter, one null table, or cap < out * ksize.  The device
 * never evaluates a filter: these tables, uploaded once, are the only source of coefficients. */
int mx_resize_coeffs(int in, int out, int filter, int32_t* bounds, int32_t* k, int cap);
/* A resize plan: both axes' tables in library-owned device memory (built and uploaded here, once, off the hot path; an axis whose in == out gets
 * the identity table, which copies exactly) and the tile shape the launch uses.  NULL, with the reason in the last error, for a non-positive
 * or too large size, an unknown filter, a failed allocation or copy, or a downscale so steep (thousands to one) that the
 * input bytes under the taps of four output bytes of one row do not fit a workgroup's LDS. */
typedef struct mx_resize mx_resize;
mx_resize* mx_resize_create(int in_h, int in_w, int out_h, int out_w, int filter);
void mx_resize_destroy(mx_resize* r);
/* src uint8 [B][in_h][in_w][C] -> dst uint8 [B][out_h][out_w][C], C = 1 or 3, both passes in ONE launch: the horizontally filtered bytes live in
 * LDS only.  No allocation, copy or synchronisation inside the call; any alignment of src and dst (whole-dword accesses where a row allows them).
 * Refused, with nothing launched: a null operand, B <= 0, C other than 1 or 3, src == dst, more tiles than one launch holds. */
int mx_resize_u8(mx_resize* r, void* stream, const uint8_t* src, uint8_t* dst, int B, int C);

/* ------------------------------------------------------------------------------------------
 * Inpainting only the masked region of a client-size photo (sduss_amd/csrc/inpaint_overlay.hip, inpaint_region.cpp): diffusers'
 * VaeImageProcessor.blur, get_crop_region and apply_overlay, which are Pillow calls on the host there.  All of it is integer arithmetic on bytes
 * and bit-equal to Pillow.
 * ------------------------------------------------------------------------------------------ */
#define MX_BLUR_MAX_RADIUS 1024
#define MX_BLUR_MAX_WIDTH 16384    /* a row and its blurred copy live in a workgroup's LDS */
/* The box of Pillow's ImageFilter.GaussianBlur(radius) (src/libImaging/BoxBlur.c), host only, no GPU needed.  Pillow blurs with three box passes
 * per axis; one pass over a line in[0..n) is
 *     out[x] = (ww * sum_{d=-r..r} in[clamp(x + d)] + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + 2^23) >> 24,   clamp to [0, n - 1],
 * with, in single precision and in this order,
 *     sigma2 = radius * radius / 3;  L = sqrt(12 * sigma2 + 1);  l = floor((L - 1) / 2);
 *     a = (2 l + 1) * (l * (l + 1) - 3 * sigma2) / (6 * (sigma2 - (l + 1) * (l + 1)));  fr = l + a;
 *     r = (int)fr;  ww = (uint32)((float)(1 << 24) / (fr * 2 + 1));  fw = ((1 << 24) - (2 r + 1) * ww) / 2.
 * (Pillow forms L in double; that moves l only where 12 sigma2 + 1 is an odd square to the last place, and there the two boxes, (r, ww, ww) and
 * (r + 1, ww, 0), are the same filter.)  Returns 0, or 1 with the reason in the last error for a null result or a radius outside
 * (0, MX_BLUR_MAX_RADIUS]. */
int mx_blur_box_params(float radius, int* r, uint32_t* ww, uint32_t* fw);
/* src uint8 [B][H][W] -> dst, every plane bit-equal to Image.fromarray(plane, "L").filter(ImageFilter.GaussianBlur(radius)): three box passes along
 * the rows, then three along the columns, each rounded to bytes on its own (so they cannot be merged).  radius <= 0 copies.  Four launches: the row
 * passes in one (a line stays in LDS between them), one per column pass through `scratch` (B * H * W bytes of device memory from the caller; may be
 * NULL when radius <= 0).  No allocation or synchronisation inside the call.  Dword accesses when W % 4 == 0 and the buffers are 4-byte aligned.
 * Refused, with nothing launched: a null src or dst, a null scratch at a positive radius, a non-positive size, W > MX_BLUR_MAX_WIDTH, a radius that
 * is NaN or above MX_BLUR_MAX_RADIUS, dst or scratch overlapping another buffer. */
int mx_gaussian_blur_u8(void* stream, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, float radius);
/* mask uint8 [B][H][W] -> box int32 [B][4] in device memory: (x_min, y_min, x_max + 1, y_max + 1) over the non-zero bytes of each plane, PIL's
 * Image.getbbox; an empty plane gives (W, H, 0, 0).  One memset of the record and one launch: integer minima and maxima by atomics, so the result
 * does not depend on their order.  Refused: a null operand, a non-positive size, a misaligned record. */
int mx_mask_bbox_u8(void* stream, const uint8_t* mask, int32_t* box, int B, int H, int W);
/* diffusers' get_crop_region applied to the bounding box (x1, y1, x2, y2) of a mask of mask_w x mask_h, for an image to be processed at
 * width x height.  Host only.  In Python's terms (ints; / is the double division, int() truncates):
 *     x1 = max(x1 - pad, 0); y1 = max(y1 - pad, 0); x2 = min(x2 + pad, mask_w); y2 = min(y2 + pad, mask_h)
 *     if (x2 - x1) / (y2 - y1) > width / height:
 *         diff = int((x2 - x1) / (width / height) - (y2 - y1));  y1 -= diff // 2;  y2 += diff - diff // 2
 *         if y2 >= mask_h: d = y2 - mask_h; y2 -= d; y1 -= d
 *         if y1 < 0: y2 -= y1; y1 = 0
 *         if y2 >= mask_h: y2 = mask_h
 *     else: the same on x with diff = int((y2 - y1) * (width / height) - (x2 - x1)) and mask_w
 * out[4] = (x1, y1, x2, y2).  Returns 0, or 1 with the reason in the last error: a null result, a non-positive size, a negative pad, an empty box
 * (what an empty mask gives), a box that does not lie inside the mask. */
int mx_crop_region(int x1, int y1, int x2, int y2, int mask_w, int mask_h, int width, int height, int pad, int32_t* out);
/* The client's image with the repainted crop blended in: decoded uint8 [B][h][w][3] (the decoder's image, resized to the region), original uint8
 * [B][H][W][3], mask uint8 [B][H][W] soft (255 = repaint), the region at (x, y) .. (x + w, y + h) -> out uint8 [B][H][W][3], ONE launch that writes
 * every byte.  Outside the box out is original; inside it is what diffusers' apply_overlay computes with Pillow (paste of the premultiplied original
 * under the inverted mask, then alpha_composite), per channel with A = 255 - m, d the decoded and o the original byte:
 *     t = o * A + 128;  p = ((t >> 8) + t) >> 8;  c = min(255, (255 * p) / A)            (A = 0: the result is d)
 *     u = c * (A * 128) + d * (255 * 128 - A * 128) + (0x80 << 7);  out = (((u >> 8) + u) >> 8) >> 7
 * which is o itself where m = 0 and, on a 0 / 255 mask, the hard paste of mx_rgb8_paste.  Dword accesses when original, mask and out are 4-byte
 * aligned.  Refused: a null operand, a non-positive size, a box that does not lie inside the image, out overlapping an input. */
int mx_rgb8_overlay(void* stream, const uint8_t* decoded, const uint8_t* original, const uint8_t* mask, uint8_t* out, int B, int H, int W, int x, int y,
                    int w, int h);

/* ------------------------------------------------------------------------------------------
 * LoRA adapters merged into the packed weights on the device (lora_merge.hip, lora_terms.cpp; sduss_amd/lora.py builds the tables).
 * Every packing transform of sduss_amd/weights.py is linear in W, so a low-rank update is applied in packed space: ONE launch walks a table of
 * terms.  A term covers rows row0 .. row0 + rows of one packed bf16 matrix [N, K] at byte offset w_off of the blob:
 *     out[n][k] = bf16_rn( f32(base[n][k]) + sum_t scale_t * sum_r up_t[n - row0][r] * down_t[k][r] )
 * over all terms of the table with the same (w_off, row0, rows), in table order: bf16 MFMA products with fp32 accumulation per term, scale_t
 * applied in fp32, ONE rounding at the end.  base and out are DIFFERENT buffers with the same layout (the pristine blob and the active one): the
 * kernel never reads what it writes, so merging a set twice, or after another set, cannot accumulate.  Rows outside the range are not touched.
 *   up      bf16 [rows, R]  in the packed row order (weights._geglu_interleave applied where the matrix has it)
 *   down_t  bf16 [K, R]     the down factor TRANSPOSED, so that both MFMA operands are 16-byte loads per lane
 *   R       a multiple of 32 (the packer pads with zeros), at most MX_LORA_MAX_RANK summed over the terms of one row range
 * Matrices with a folded LayerNorm (attn1.to_qkv, attn2.to_q, ff.net.0.proj: weights.fold_layernorm) carry two derived fp32 vectors, written by the
 * same launch where colsum_off != MX_LORA_NO_VECTOR:
 *     colsum[n] = the fp32 sum over k of the ROUNDED out[n][k] just stored (a workgroup owns whole rows: no atomics, the same bits every run)
 *     bias[n]   = bias_base[n] + sum_t scale_t * dbias_t[n - row0]           (dbias fp32 [rows]; a null dbias adds nothing)
 * at byte offsets colsum_off / bias_off of the blobs (vectors of N entries, indexed by the row n of the matrix).
 * The divisibility rule of the tiling: row0 % 16 == 0, rows % 16 == 0, rows > 0, K % 64 == 0, K > 0, R % 32 == 0, R > 0; every linear of SDXL-base
 * and of UNetConfig.tiny() satisfies it (widths 64 .. 1280 and their multiples, context 128 / 2048).  Offsets: w_off a multiple of 16 bytes,
 * vector offsets multiples of 4; up / down_t 16-byte aligned, dbias 4-byte aligned.
 * mx_lora_merge_validate (host only, no GPU) returns 0, or 1 with the reason in the last error: a null table with n > 0, a term outside the blob
 * (matrix or vectors), a shape outside the rule, a null or misaligned operand, a non-finite scale, row ranges of two terms of one matrix that
 * overlap without being identical (identical ranges are stacked adapters and must then agree in N, K and the vector offsets), a row range whose ranks
 * sum to more than MX_LORA_MAX_RANK.  n == 0 is valid and launches nothing.
 * mx_lora_merge validates, builds the device table in `table_dev` (caller-provided device memory of at least mx_lora_table_bytes(n) bytes; nothing
 * is allocated inside the call), copies it on `stream` and launches one grid over (row range, row block).  It waits for the stream once, before the
 * launch, so that the table has left host memory when the call returns. */
#define MX_LORA_NO_VECTOR (~(uint64_t)0)
#define MX_LORA_MAX_RANK 512
typedef struct mx_lora_term {
  uint64_t w_off;             /* byte offset of the packed matrix [N, K] in the blob */
  int N, K, row0, rows;
  const void* up;             /* device, bf16 [rows, R] */
  const void* down_t;         /* device, bf16 [K, R] */
  int R;
  float scale;
  uint64_t colsum_off, bias_off;   /* MX_LORA_NO_VECTOR (both) where the matrix has no folded LayerNorm */
  const float* dbias;         /* device, fp32 [rows], or NULL */
} mx_lora_term;
int mx_lora_merge_validate(const mx_lora_term* t, int n, uint64_t blob_bytes);   /* host only */
size_t mx_lora_table_bytes(int n);                                               /* host only; 0 for n < 0 */
int mx_lora_merge(void* stream, const void* base_blob, void* active_blob, uint64_t blob_bytes, const mx_lora_term* terms, int n, void* table_dev,
                  size_t table_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MXDENOISE_H */
