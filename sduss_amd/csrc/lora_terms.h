// The device table of one LoRA merge launch (lora_merge.hip), as lora_terms.cpp builds it on the host.  Plain C++: no HIP type appears here.
// Layout in table_dev: [LoraDevGroup x n_groups][LoraDevTerm x n_terms]; the terms of a group are contiguous and in the caller's table order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/mxdenoise.h"

namespace mx {

constexpr int kLoraBlockRows = 32;   // rows one workgroup owns (two 16-row MFMA tiles); the last block of a range may hold 16
constexpr int kLoraTileRows = 16;
constexpr int kLoraChunkK = 64;      // the k extent one wave covers per step: 128 contiguous bytes of every row

struct LoraDevTerm {
  const void* up;
  const void* down_t;
  const float* dbias;
  int R;
  float scale;
};

struct LoraDevGroup {
  uint64_t w_off, colsum_off, bias_off;   // byte offsets into both blobs; the matrix offset is that of row 0 of the matrix
  int K, row0, rows;
  int first_term, n_terms;
  int block0;                             // the first workgroup of this row range; it has (rows + 31) / 32 of them
};

// Groups the terms by row range (stable: table order inside a group) into `table`; returns the number of workgroups, or -1 after set_error;
// max_rank = the largest sum of ranks over one row range (the launch sizes its LDS by it).
// Validates first (mx_lora_merge_validate).
long lora_build_table(const mx_lora_term* t, int n, uint64_t blob_bytes, std::vector<unsigned char>* table, int* n_groups, int* max_rank);

}  // namespace mx
