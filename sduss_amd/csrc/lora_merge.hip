// LoRA adapters merged into the packed weights (include/mxdenoise.h, "LoRA adapters"): one launch over a table of terms,
//     out[n][k] = bf16_rn( f32(base[n][k]) + sum_t scale_t * sum_r up_t[n][r] * down_t[k][r] )          (gfx950)
// A workgroup (4 waves) owns 32 rows of one row range over ALL of K, so the row sums of folded matrices need no atomics; its waves deal the
// 64-wide k chunks among themselves.  The product is computed TRANSPOSED, D[k][n] = sum_r down_t[k][r] up[n][r], with v_mfma_f32_16x16x32_bf16:
//   A = down_t: lane l holds A[row l & 15][r = 8 (l >> 4) + j]        = 16 contiguous bytes of one row of down_t [K, R]
//   B = up:     lane l holds B[r = 8 (l >> 4) + j][col l & 15]        = 16 contiguous bytes of one row of up [rows, R]
//   D:          lane l holds column n = l & 15, rows 4 (l >> 4) + reg
// A row i of A is ours to choose: MFMA `a` (0, 1) of a 32-wide half chunk loads down_t row k = k0 + 8 (i >> 2) + 4 a + (i & 3), so that the two
// results of lane group g = l >> 4 are k0 + 8 g + 4 a + reg: EIGHT consecutive k of row n, one 16-byte load of base and one 16-byte store of out per
// lane, and the four lane groups of the two half chunks cover 128 contiguous bytes of every row.  The up fragments of every term of the row range
// are staged once per workgroup in LDS, in fragment order (one ds_read_b128 per lane, no bank conflict).
// At R = 64 this is 128 flop per weight element against 4 bytes of HBM traffic: the matrix cores keep it memory-bound, the vector ALU would not.
#include "common.h"
#include "lora_terms.h"

namespace mx {
void set_error(const std::string& msg);

struct LoraArgs {
  const char* base;
  char* out;
  const LoraDevGroup* groups;
  const LoraDevTerm* terms;
  int n_groups;
};

constexpr int kLoraThreads = 256;
constexpr int kLoraWaves = kLoraThreads / kWave;

__device__ __forceinline__ u32x4 lora_ld16(const void* p) { return *reinterpret_cast<const u32x4*>(p); }

__global__ __launch_bounds__(kLoraThreads) void lora_merge_kernel(const LoraArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u32x4* s_up = reinterpret_cast<u32x4*>(smem);                        // [r-step of every term][tile 0, 1][lane]: the B fragments
  __shared__ float s_sum[kLoraWaves][kLoraBlockRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, grp = lane >> 4;

  // the row range of this workgroup: the last group whose first block is not past it
  int lo = 0, hi = p.n_groups - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.groups[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const LoraDevGroup g = p.groups[lo];
  const LoraDevTerm* terms = p.terms + g.first_term;
  const int lrow0 = ((int)blockIdx.x - g.block0) * kLoraBlockRows;      // first row of the block inside the range
  const int ntiles = (g.rows - lrow0) >= kLoraBlockRows ? 2 : 1;        // (rows % 16 == 0: the tail block holds one tile)
  const int K = g.K;

  int steps_before = 0;
  for (int t = 0; t < g.n_terms; ++t) {
    const int R = terms[t].R, steps = R >> 5;
    const bf16_t* up = reinterpret_cast<const bf16_t*>(terms[t].up);
    for (int idx = tid; idx < steps * 2 * kWave; idx += kLoraThreads) {
      const int s = idx >> 7, tile = (idx >> 6) & 1, ln = idx & 63;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (tile < ntiles) v = lora_ld16(up + (long)(lrow0 + tile * kLoraTileRows + (ln & 15)) * R + s * 32 + 8 * (ln >> 4));
      s_up[((steps_before + s) * 2 + tile) * kWave + ln] = v;
    }
    steps_before += steps;
  }
  __syncthreads();

  const long wrow = (long)(g.row0 + lrow0 + col) * K;                    // element offset of this lane's row of tile 0
  const bf16_t* wbase = reinterpret_cast<const bf16_t*>(p.base + g.w_off);
  bf16_t* wout = reinterpret_cast<bf16_t*>(p.out + g.w_off);
  float rowsum[2] = {0.f, 0.f};

  for (int kb = wave * kLoraChunkK; kb < K; kb += kLoraWaves * kLoraChunkK) {
    float tot[2][2][8];                                                // [tile][half chunk][k]
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        u32x4 w = {0u, 0u, 0u, 0u};
        if (ti < ntiles) w = lora_ld16(wbase + wrow + (long)ti * kLoraTileRows * K + kb + h * 32 + grp * 8);
        unpack_bf16x8(w, tot[ti][h]);
      }
    int sb = 0;
    for (int t = 0; t < g.n_terms; ++t) {
      const int R = terms[t].R, steps = R >> 5;
      const float scale = terms[t].scale;
      const bf16_t* down = reinterpret_cast<const bf16_t*>(terms[t].down_t);
      f32x4 acc[2][2][2];                                              // [tile][half chunk][a]
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i >> 2][(i >> 1) & 1][i & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < steps; ++s) {
        bf16x8 af[2][2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            const int k = kb + h * 32 + 8 * (col >> 2) + 4 * a + (col & 3);
            af[h][a] = __builtin_bit_cast(bf16x8, lora_ld16(down + (long)k * R + s * 32 + 8 * grp));
          }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
          const bf16x8 bfrag = __builtin_bit_cast(bf16x8, s_up[((sb + s) * 2 + ti) * kWave + lane]);
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int a = 0; a < 2; ++a) acc[ti][h][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[h][a], bfrag, acc[ti][h][a], 0, 0, 0);
        }
      }
      sb += steps;
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 8; ++e) tot[ti][h][e] = fmaf(scale, acc[ti][h][e >> 2][e & 3], tot[ti][h][e]);
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
      if (ti < ntiles) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const u32x4 o = pack_bf16x8(tot[ti][h]);
          *reinterpret_cast<u32x4*>(wout + wrow + (long)ti * kLoraTileRows * K + kb + h * 32 + grp * 8) = o;
          float r[8];
          unpack_bf16x8(o, r);
#pragma unroll
          for (int e = 0; e < 8; ++e) rowsum[ti] += r[e];
        }
      }
  }

  if (g.colsum_off == MX_LORA_NO_VECTOR) return;
  // row sums: the four lane groups of a wave, then the four waves, always in this order
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    float v = rowsum[ti];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lane < 16) s_sum[wave][ti * kLoraTileRows + lane] = v;
  }
  __syncthreads();
  if (tid < ntiles * kLoraTileRows) {
    const int n = g.row0 + lrow0 + tid;
    float cs = 0.f;
#pragma unroll
    for (int w = 0; w < kLoraWaves; ++w) cs += s_sum[w][tid];
    reinterpret_cast<float*>(p.out + g.colsum_off)[n] = cs;
    float b = reinterpret_cast<const float*>(p.base + g.bias_off)[n];
    for (int t = 0; t < g.n_terms; ++t)
      if (terms[t].dbias) b = fmaf(terms[t].scale, terms[t].dbias[lrow0 + tid], b);
    reinterpret_cast<float*>(p.out + g.bias_off)[n] = b;
  }
}

}  // namespace mx

extern "C" int mx_lora_merge(void* stream, const void* base_blob, void* active_blob, uint64_t blob_bytes, const mx_lora_term* terms, int n,
                             void* table_dev, size_t table_bytes) {
  static thread_local std::vector<unsigned char> table;
  int n_groups = 0, max_rank = 0;
  const long blocks = mx::lora_build_table(terms, n, blob_bytes, &table, &n_groups, &max_rank);
  if (blocks < 0) return 1;
  if (n == 0) return 0;
  if (!base_blob || !active_blob) { mx::set_error("lora_merge: null blob"); return 1; }
  if (((uintptr_t)base_blob | (uintptr_t)active_blob) & 15) { mx::set_error("lora_merge: misaligned blob (16 bytes)"); return 1; }
  {
    const uintptr_t b = (uintptr_t)base_blob, a = (uintptr_t)active_blob;
    if (b < a + blob_bytes && a < b + blob_bytes) { mx::set_error("lora_merge: the base and the active blob overlap"); return 1; }
  }
  if (!table_dev || ((uintptr_t)table_dev & 15) || table_bytes < table.size()) { mx::set_error("lora_merge: table_dev is null, misaligned or holds fewer than mx_lora_table_bytes(n) bytes"); return 1; }
  hipStream_t s = (hipStream_t)stream;
  // the table is read from this thread's vector: it must have left host memory before the next call fills the vector again
  if (hipMemcpyAsync(table_dev, table.data(), table.size(), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    mx::set_error("lora_merge: sending the table failed");
    return 1;
  }
  mx::LoraArgs a;
  a.base = (const char*)base_blob;
  a.out = (char*)active_blob;
  a.groups = (const mx::LoraDevGroup*)table_dev;
  a.terms = (const mx::LoraDevTerm*)((const char*)table_dev + (size_t)n_groups * sizeof(mx::LoraDevGroup));
  a.n_groups = n_groups;
  const size_t lds = (size_t)(max_rank / 32) * 2 * mx::kWave * 16;     // the up fragments of the widest row range
  hipLaunchKernelGGL(mx::lora_merge_kernel, dim3((unsigned)blocks), dim3(mx::kLoraThreads), lds, s, a);
  if (hipGetLastError() != hipSuccess) { mx::set_error("lora_merge: launch failed"); return 1; }
  return 0;
}
