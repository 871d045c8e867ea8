// The term table of the LoRA merge (lora_merge.hip) on the host: every check the kernel's addressing relies on, and the grouping of the terms by
// row range into the device table.  Host only and plain C++: nothing of HIP is included, so tests/lora_terms_walk.cpp links this file alone.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "lora_terms.h"

namespace mx {
void set_error(const std::string& msg);   // capi.cpp (the walk brings its own)

static int refuse(int i, const char* what) {
  set_error("lora_merge: term " + std::to_string(i) + ": " + what);
  return 1;
}

// [off, off + bytes) inside [0, total), with no wrap-around
static bool inside(uint64_t off, uint64_t bytes, uint64_t total) { return off <= total && bytes <= total - off; }

static bool same_range(const mx_lora_term& a, const mx_lora_term& b) { return a.w_off == b.w_off && a.row0 == b.row0 && a.rows == b.rows; }

// the order of the groups: by the first byte of the row range, then table order (stable sort)
static uint64_t first_byte(const mx_lora_term& t) { return t.w_off + (uint64_t)t.row0 * (uint64_t)t.K * 2; }

static int check_term(const mx_lora_term& t, int i, uint64_t blob_bytes) {
  if (t.N <= 0 || t.K <= 0 || t.rows <= 0 || t.row0 < 0 || (int64_t)t.row0 + t.rows > t.N) return refuse(i, "the row range does not lie inside the matrix");
  if (t.K % kLoraChunkK) return refuse(i, "K must be a multiple of 64");
  if (t.rows % kLoraTileRows || t.row0 % kLoraTileRows) return refuse(i, "row0 and rows must be multiples of 16");
  if (t.R <= 0 || t.R % 32) return refuse(i, "R must be a positive multiple of 32");
  if (t.R > MX_LORA_MAX_RANK) return refuse(i, "the ranks of one row range sum to more than MX_LORA_MAX_RANK");
  if (!std::isfinite(t.scale)) return refuse(i, "the scale is not finite");
  if (!t.up || !t.down_t) return refuse(i, "null factor");
  if (((uintptr_t)t.up | (uintptr_t)t.down_t) & 15) return refuse(i, "misaligned factor (16 bytes)");
  if ((uintptr_t)t.dbias & 3) return refuse(i, "misaligned dbias (4 bytes)");
  if (t.w_off & 15) return refuse(i, "misaligned matrix offset (16 bytes)");
  if (!inside(t.w_off, (uint64_t)t.N * (uint64_t)t.K * 2, blob_bytes)) return refuse(i, "the matrix lies outside the blob");
  const bool cs = t.colsum_off != MX_LORA_NO_VECTOR, bs = t.bias_off != MX_LORA_NO_VECTOR;
  if (cs != bs) return refuse(i, "colsum_off and bias_off go together");
  if (!cs && t.dbias) return refuse(i, "dbias without a folded bias to add it to");
  if (cs) {
    if ((t.colsum_off | t.bias_off) & 3) return refuse(i, "misaligned vector offset (4 bytes)");
    if (!inside(t.colsum_off, (uint64_t)t.N * 4, blob_bytes) || !inside(t.bias_off, (uint64_t)t.N * 4, blob_bytes)) return refuse(i, "a derived vector lies outside the blob");
  }
  return 0;
}

// indices of the terms ordered by row range; empty after a refusal
static std::vector<int> ordered(const mx_lora_term* t, int n, uint64_t blob_bytes, bool* ok) {
  *ok = false;
  std::vector<int> idx;
  if (n < 0 || (n > 0 && !t)) { set_error("lora_merge: null table or negative count"); return idx; }
  for (int i = 0; i < n; ++i)
    if (check_term(t[i], i, blob_bytes)) return idx;
  idx.resize((size_t)n);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return first_byte(t[a]) < first_byte(t[b]); });
  // sorted by first byte: a range that overlaps any earlier one overlaps the one that reaches furthest so far
  int far = -1;
  uint64_t far_end = 0;
  int rank_sum = 0;
  for (int j = 0; j < n; ++j) {
    const mx_lora_term& c = t[idx[j]];
    const uint64_t b = first_byte(c), e = b + (uint64_t)c.rows * (uint64_t)c.K * 2;
    if (far >= 0 && b < far_end) {
      const mx_lora_term& p = t[far];
      if (!same_range(p, c)) { refuse(idx[j], ("its row range overlaps that of term " + std::to_string(far) + " without being identical").c_str()); idx.clear(); return idx; }
      if (p.N != c.N || p.K != c.K || p.colsum_off != c.colsum_off || p.bias_off != c.bias_off) {
        refuse(idx[j], ("it stacks on term " + std::to_string(far) + " but names another shape or other vectors").c_str()); idx.clear(); return idx;
      }
      rank_sum += c.R;
      if (rank_sum > MX_LORA_MAX_RANK) { refuse(idx[j], "the ranks of one row range sum to more than MX_LORA_MAX_RANK"); idx.clear(); return idx; }
    } else {
      rank_sum = c.R;
    }
    if (far < 0 || e > far_end) { far = idx[j]; far_end = e; }
  }
  *ok = true;
  return idx;
}

long lora_build_table(const mx_lora_term* t, int n, uint64_t blob_bytes, std::vector<unsigned char>* table, int* n_groups, int* max_rank) {
  bool ok = false;
  const std::vector<int> idx = ordered(t, n, blob_bytes, &ok);
  if (!ok) return -1;
  std::vector<LoraDevGroup> groups;
  std::vector<LoraDevTerm> terms;
  long blocks = 0;
  int rank = 0;
  *max_rank = 0;
  for (int j = 0; j < n; ++j) {
    const mx_lora_term& c = t[idx[j]];
    if (j == 0 || !same_range(t[idx[j - 1]], c)) {
      LoraDevGroup g;
      std::memset(&g, 0, sizeof g);
      g.w_off = c.w_off; g.colsum_off = c.colsum_off; g.bias_off = c.bias_off;
      g.K = c.K; g.row0 = c.row0; g.rows = c.rows;
      g.first_term = j; g.n_terms = 0;
      if (blocks > 0x7fffffffL - (c.rows + kLoraBlockRows - 1) / kLoraBlockRows) { set_error("lora_merge: more than 2^31 row blocks"); return -1; }
      g.block0 = (int)blocks;
      blocks += (c.rows + kLoraBlockRows - 1) / kLoraBlockRows;
      groups.push_back(g);
      rank = 0;
    }
    rank += c.R;
    *max_rank = std::max(*max_rank, rank);
    groups.back().n_terms++;
    LoraDevTerm d;
    std::memset(&d, 0, sizeof d);
    d.up = c.up; d.down_t = c.down_t; d.dbias = c.dbias; d.R = c.R; d.scale = c.scale;
    terms.push_back(d);
  }
  table->resize(groups.size() * sizeof(LoraDevGroup) + terms.size() * sizeof(LoraDevTerm));
  if (!groups.empty()) std::memcpy(table->data(), groups.data(), groups.size() * sizeof(LoraDevGroup));
  if (!terms.empty()) std::memcpy(table->data() + groups.size() * sizeof(LoraDevGroup), terms.data(), terms.size() * sizeof(LoraDevTerm));
  *n_groups = (int)groups.size();
  return blocks;
}

}  // namespace mx

extern "C" int mx_lora_merge_validate(const mx_lora_term* t, int n, uint64_t blob_bytes) {
  bool ok = false;
  (void)mx::ordered(t, n, blob_bytes, &ok);
  return ok ? 0 : 1;
}

extern "C" size_t mx_lora_table_bytes(int n) {
  return n < 0 ? 0 : (size_t)n * (sizeof(mx::LoraDevGroup) + sizeof(mx::LoraDevTerm));
}
