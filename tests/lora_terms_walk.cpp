// The LoRA merge's term table (sduss_amd/csrc/lora_terms.cpp) under AddressSanitizer + UBSan, on the CPU: a program of its own, built by
// `make -C sduss_amd/csrc lora_walk` from that one source file.  It walks good tables (single terms, stacked adapters, row ranges of one matrix, a
// folded matrix, shuffled order, the empty table) and checks what the kernel's addressing relies on in the device table they become: groups ordered
// and disjoint, block0 the running sum of ceil(rows / 32), every term in exactly one group and in table order, max_rank the widest group.  Then
// every refused kind of table, each with its message.  No pointer of a term is ever followed: the factors are made-up aligned addresses.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/mxdenoise.h"
#include "../sduss_amd/csrc/lora_terms.h"

static std::string last_error;
namespace mx {
void set_error(const std::string& msg) { last_error = msg; }
}  // namespace mx

#define REQUIRE(cond)                                                                                                              \
  do {                                                                                                                             \
    if (!(cond)) { std::fprintf(stderr, "lora_terms_walk: %s failed at line %d: %s\n", #cond, __LINE__, last_error.c_str()); return 1; } \
  } while (0)

static const uint64_t kBlob = 64u << 20;

static mx_lora_term term(uint64_t w_off, int N, int K, int row0, int rows, int R, uintptr_t fake) {
  mx_lora_term t;
  std::memset(&t, 0, sizeof t);
  t.w_off = w_off; t.N = N; t.K = K; t.row0 = row0; t.rows = rows; t.R = R; t.scale = 0.75f;
  t.up = (const void*)(fake); t.down_t = (const void*)(fake + 0x100000);
  t.colsum_off = MX_LORA_NO_VECTOR; t.bias_off = MX_LORA_NO_VECTOR; t.dbias = nullptr;
  return t;
}

// the device table of a good table: the invariants the kernel relies on
static int walk_good(const std::vector<mx_lora_term>& t, int want_groups, long want_blocks, int want_rank) {
  REQUIRE(mx_lora_merge_validate(t.data(), (int)t.size(), kBlob) == 0);
  std::vector<unsigned char> table;
  int n_groups = -1, max_rank = -1;
  const long blocks = mx::lora_build_table(t.data(), (int)t.size(), kBlob, &table, &n_groups, &max_rank);
  REQUIRE(blocks == want_blocks && n_groups == want_groups && max_rank == want_rank);
  REQUIRE(table.size() == n_groups * sizeof(mx::LoraDevGroup) + t.size() * sizeof(mx::LoraDevTerm));
  REQUIRE(table.size() <= mx_lora_table_bytes((int)t.size()));
  std::vector<mx::LoraDevGroup> g((size_t)n_groups);
  std::vector<mx::LoraDevTerm> d(t.size());
  if (n_groups) std::memcpy(g.data(), table.data(), g.size() * sizeof g[0]);
  if (!d.empty()) std::memcpy(d.data(), table.data() + g.size() * sizeof g[0], d.size() * sizeof d[0]);
  long b = 0;
  int next_term = 0;
  uint64_t prev_end = 0;
  for (int i = 0; i < n_groups; ++i) {
    REQUIRE(g[i].block0 == b && g[i].first_term == next_term && g[i].n_terms > 0);
    REQUIRE(g[i].rows > 0 && g[i].rows % 16 == 0 && g[i].row0 % 16 == 0 && g[i].K % 64 == 0);
    const uint64_t first = g[i].w_off + (uint64_t)g[i].row0 * g[i].K * 2, end = first + (uint64_t)g[i].rows * g[i].K * 2;
    REQUIRE(first >= prev_end && end <= kBlob);                       // disjoint, ordered, inside the blob
    prev_end = end;
    int rank = 0;
    for (int j = 0; j < g[i].n_terms; ++j) {
      const mx::LoraDevTerm& x = d[(size_t)next_term + j];
      REQUIRE(x.R > 0 && x.R % 32 == 0 && x.up && x.down_t);
      rank += x.R;
      // table order inside a group: the made-up addresses grow with the caller's index
      if (j > 0) REQUIRE((uintptr_t)x.up > (uintptr_t)d[(size_t)next_term + j - 1].up);
    }
    REQUIRE(rank <= max_rank && rank <= MX_LORA_MAX_RANK);
    b += (g[i].rows + 31) / 32;
    next_term += g[i].n_terms;
  }
  REQUIRE(b == blocks && next_term == (int)t.size());
  return 0;
}

static int refused(std::vector<mx_lora_term> t, const char* needle, uint64_t blob = kBlob) {
  last_error.clear();
  REQUIRE(mx_lora_merge_validate(t.data(), (int)t.size(), blob) == 1);
  if (last_error.find(needle) == std::string::npos) {
    std::fprintf(stderr, "lora_terms_walk: expected a refusal naming \"%s\", got \"%s\"\n", needle, last_error.c_str());
    return 1;
  }
  std::vector<unsigned char> table;
  int n_groups = 0, max_rank = 0;
  REQUIRE(mx::lora_build_table(t.data(), (int)t.size(), blob, &table, &n_groups, &max_rank) == -1);
  return 0;
}

int main() {
  int n = 0;
  // ---- good tables ----
  if (walk_good({}, 0, 0, 0)) return 1;
  REQUIRE(mx_lora_merge_validate(nullptr, 0, 0) == 0);
  if (walk_good({term(0, 16, 64, 0, 16, 32, 0x1000)}, 1, 1, 32)) return 1;
  if (walk_good({term(256, 80, 192, 0, 80, 32, 0x1000)}, 1, 3, 32)) return 1;                 // 80 rows: two blocks of 32 and a tail of 16
  // stacked adapters on one range, another matrix in between in table order
  if (walk_good({term(0, 320, 2048, 0, 320, 32, 0x1000), term(4u << 20, 64, 64, 0, 64, 64, 0x2000), term(0, 320, 2048, 0, 320, 64, 0x3000)}, 2, 12, 96)) return 1;
  // q | k | v row ranges of one matrix, given out of order
  if (walk_good({term(1024, 384, 128, 256, 128, 32, 0x1000), term(1024, 384, 128, 0, 128, 32, 0x2000), term(1024, 384, 128, 128, 128, 32, 0x3000)}, 3, 12, 32)) return 1;
  {  // a folded matrix: vectors inside the blob, dbias given
    mx_lora_term t = term(0, 512, 64, 0, 512, 32, 0x1000);
    t.colsum_off = 1u << 20; t.bias_off = (1u << 20) + 4096; t.dbias = (const float*)0x5000;
    if (walk_good({t}, 1, 16, 32)) return 1;
    mx_lora_term u = t;
    u.up = (const void*)0x9000; u.R = 480;
    if (walk_good({t, u}, 1, 16, 512)) return 1;                                              // exactly MX_LORA_MAX_RANK
    u.colsum_off += 4;
    if (refused({t, u}, "stacks on term 0")) return 1;
    u = t; u.bias_off = MX_LORA_NO_VECTOR;
    if (refused({u}, "go together")) return 1;
    u = t; u.colsum_off = kBlob - 4;
    if (refused({u}, "derived vector lies outside")) return 1;
    u = t; u.bias_off += 2;
    if (refused({u}, "misaligned vector offset")) return 1;
    u = t; u.dbias = (const float*)0x5002;
    if (refused({u}, "misaligned dbias")) return 1;
    u = term(0, 512, 64, 0, 512, 32, 0x1000); u.dbias = (const float*)0x5000;
    if (refused({u}, "dbias without")) return 1;
    n += 8;
  }
  // the last matrix may end exactly at the end of the blob
  if (walk_good({term(kBlob - 1280ull * 1280 * 2, 1280, 1280, 0, 1280, 64, 0x1000)}, 1, 40, 64)) return 1;
  n += 6;

  // ---- refused tables ----
  const mx_lora_term ok = term(4096, 128, 128, 0, 128, 32, 0x1000);
  mx_lora_term t = ok;
  REQUIRE(mx_lora_merge_validate(nullptr, 1, kBlob) == 1 && mx_lora_merge_validate(&ok, -1, kBlob) == 1);
  if (refused({ok}, "outside the blob", 4096 + 128 * 128 * 2 - 1)) return 1;
  t = ok; t.w_off = ~(uint64_t)0 - 15;
  if (refused({t}, "outside the blob")) return 1;                                               // offset + size would wrap
  t = ok; t.row0 = 64;
  if (refused({t}, "does not lie inside the matrix")) return 1;
  t = ok; t.rows = 0;
  if (refused({t}, "does not lie inside the matrix")) return 1;
  t = ok; t.row0 = -16;
  if (refused({t}, "does not lie inside the matrix")) return 1;
  t = ok; t.row0 = 0x7ffffff0; t.rows = 32;
  if (refused({t}, "does not lie inside the matrix")) return 1;
  t = ok; t.rows = 24;
  if (refused({t}, "multiples of 16")) return 1;
  t = ok; t.row0 = 8; t.rows = 16;
  if (refused({t}, "multiples of 16")) return 1;
  t = ok; t.K = 96;
  if (refused({t}, "multiple of 64")) return 1;
  t = ok; t.K = 0;
  if (refused({t}, "does not lie inside the matrix")) return 1;
  t = ok; t.R = 16;
  if (refused({t}, "multiple of 32")) return 1;
  t = ok; t.R = 0;
  if (refused({t}, "multiple of 32")) return 1;
  t = ok; t.R = MX_LORA_MAX_RANK + 32;
  if (refused({t}, "MX_LORA_MAX_RANK")) return 1;
  t = ok; t.w_off = 4096 + 8;
  if (refused({t}, "misaligned matrix offset")) return 1;
  t = ok; t.up = (const void*)0x1008;
  if (refused({t}, "misaligned factor")) return 1;
  t = ok; t.down_t = nullptr;
  if (refused({t}, "null factor")) return 1;
  t = ok; t.scale = 1.0f / 0.0f;
  if (refused({t}, "not finite")) return 1;
  // overlapping without being identical: a range inside another, a shifted one, two matrices laid over each other
  if (refused({ok, term(4096, 128, 128, 64, 64, 32, 0x2000)}, "overlaps that of term 0")) return 1;
  if (refused({term(4096, 128, 128, 0, 96, 32, 0x1000), term(4096, 128, 128, 64, 64, 32, 0x2000)}, "overlaps")) return 1;
  if (refused({ok, term(4096 + 256, 128, 128, 0, 128, 32, 0x2000)}, "overlaps")) return 1;
  if (refused({ok, term(4096, 256, 64, 0, 256, 32, 0x2000)}, "overlaps")) return 1;                                            // same bytes, another shape
  {  // ranks of one range summing past the limit
    std::vector<mx_lora_term> many;
    for (int i = 0; i < 9; ++i) many.push_back(term(4096, 128, 128, 0, 128, 64, 0x1000 + 0x1000 * i));
    if (refused(many, "MX_LORA_MAX_RANK")) return 1;
    many.pop_back();
    if (walk_good(many, 1, 4, 512)) return 1;
  }
  n += 23;
  REQUIRE(mx_lora_table_bytes(-1) == 0 && mx_lora_table_bytes(0) == 0 && mx_lora_table_bytes(3) >= 3 * (sizeof(mx::LoraDevGroup) + sizeof(mx::LoraDevTerm)));
  std::printf("LORA_TERMS_WALK_OK %d tables\n", n);
  return 0;
}
