// Stand-alone check of csrc/commit_next.h's node-id prefix (commit_line_prefix: the accepted samples before every
// 64-sample group, from the KC_ACC words of k_commit's workgroup lines) against a plain running sum.  The lines are laid
// out as on the device (SFFK_PUB_WORDS words per line, the word under test first); a word counts when it carries the
// commit's launch number.  Cases for 1, 2, 64, 65, 256, 257 and 1024 lines: every stamp current, stale stamps at the top
// (the lines above the round's size), one stale line in the middle, counts of 0 and of 64, random counts.
// Prints "ok <cases>" or the first difference.
#include <cstdio>
#include <cstdint>
#include <random>
#include <vector>
#include "commit_next.h"

using namespace sffk;

static int cases = 0;

// counts[g] < 0: a stale line (an earlier launch's number) holding -counts[g] - 1
static int check(const char* what, const std::vector<int>& counts, unsigned seq) {
  const int n = (int)counts.size();
  std::vector<unsigned long long> lines((size_t)n * SFFK_PUB_WORDS, ~0ULL);   // (the other words of a line: never looked at)
  for (int g = 0; g < n; ++g) {
    const bool stale = counts[g] < 0;
    const unsigned v = (unsigned)(stale ? -counts[g] - 1 : counts[g]);
    lines[(size_t)g * SFFK_PUB_WORDS] = ((unsigned long long)(stale ? seq - 1u - (unsigned)(g % 3) : seq) << 32) | v;
  }
  std::vector<int32_t> pref((size_t)n + 1, -7);
  const int total = commit_line_prefix(lines.data(), SFFK_PUB_WORDS, n, seq, pref.data());
  int run = 0;
  for (int g = 0; g < n; ++g) {
    if (pref[g] != run) { printf("%s, %d lines: prefix of line %d is %d, the running sum %d\n", what, n, g, pref[g], run); return 1; }
    if (counts[g] > 0) run += counts[g];
  }
  if (total != run) { printf("%s, %d lines: total %d, the running sum %d\n", what, n, total, run); return 1; }
  if (pref[n] != -7) { printf("%s, %d lines: wrote behind the last line\n", what, n); return 1; }
  ++cases;
  return 0;
}

int main() {
  std::mt19937 rng(2024);
  const int sizes[] = {1, 2, 64, 65, 256, 257, 1024};
  const unsigned seqs[] = {1u, 7u, 0x80000001u, 0xffffffffu};
  for (int n : sizes)
    for (unsigned seq : seqs) {
      std::vector<int> c((size_t)n);
      for (int fill : {0, 64, 1}) {                                    // every line empty, every line full, one sample each
        for (int g = 0; g < n; ++g) c[g] = fill;
        if (check("all current, equal counts", c, seq)) return 1;
      }
      for (int g = 0; g < n; ++g) c[g] = (int)(rng() % 65u);
      if (check("all current", c, seq)) return 1;
      for (int g = 0; g < n; ++g) c[g] = (g & 1) ? 64 : 0;             // 0 and 64 side by side
      if (check("counts of 0 and 64", c, seq)) return 1;
      for (int top : {1, n / 2, n}) {                                  // stale lines at the top (n: the whole round is stale)
        for (int g = 0; g < n; ++g) c[g] = (int)(rng() % 65u);
        for (int g = n - top; g < n; ++g) c[g] = -1 - (int)(rng() % 65u);
        if (check("stale at the top", c, seq)) return 1;
      }
      for (int mid : {n / 2, n / 2 - 1, 63, 64}) {                     // one stale line in the middle: it counts 0
        if (mid < 0 || mid >= n) continue;
        for (int g = 0; g < n; ++g) c[g] = 1 + (int)(rng() % 64u);
        c[mid] = -1 - 64;
        if (check("one stale line", c, seq)) return 1;
      }
    }
  int32_t none[1] = {-7};
  const unsigned long long w = 5ULL << 32 | 9ULL;
  if (commit_line_prefix(&w, SFFK_PUB_WORDS, 0, 5u, none) != 0 || none[0] != -7) { printf("no lines\n"); return 1; }
  if (commit_line_prefix(&w, SFFK_PUB_WORDS, SFFK_DEV_MAX_GROUPS + 1, 5u, none) != -1 || none[0] != -7) { printf("too many lines\n"); return 1; }
  if (commit_line_count(w, 5u) != 9u || commit_line_count(w, 6u) != 0u) { printf("commit_line_count\n"); return 1; }
  printf("ok %d\n", cases);
  return 0;
}
