// persistence_table_check.cpp -- a stand-alone program around persistence_table.h, the host-side builder of
// the ancestor table, meant to be compiled with -fsanitize=address,undefined and run on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       persistence_table_check.cpp -o persistence_table_check && ./persistence_table_check
//
// It feeds the builder the ladder hierarchies of the tests (heights 1 .. 20, and 65535), a three-level
// hierarchy with sparse ids up to 2^30 listed out of order, a hierarchy that lacks an id and empty inputs,
// and compares every entry with GetParentId walked from level 0.  Prints "ok" and returns 0, or says what
// differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "persistence_table.h"

namespace {

struct Ref {
  int32_t id, parent_id;
};
typedef std::vector<std::vector<Ref>> Hier;

// GetParentId(id, 0, level) from scratch; -2 when a level lacks the id.
int32_t Walk(const Hier& hier, int32_t id, size_t level) {
  for (size_t l = 0; l < level; ++l) {
    bool found = false;
    for (const Ref& c : hier[l]) {
      if (c.id == id) {
        id = c.parent_id;
        found = true;
        break;
      }
    }
    if (!found) return -2;
  }
  return id;
}

int failures = 0;

void Check(const char* what, const Hier& hier, const std::vector<int32_t>& ids, bool walk_all) {
  std::vector<int32_t> table;
  int bad_level = -1;
  int32_t bad_id = -1;
  const bool ok = vsg_render_impl::BuildAncestorTable(hier, ids.data(), ids.size(), &table, &bad_level, &bad_id);
  const size_t L = vsg_render_impl::PersistenceHeight(hier.size());
  if (!ok) {
    std::printf("%s: refused at level %d, id %d\n", what, bad_level, bad_id);
    ++failures;
    return;
  }
  if (table.size() != (L - 1) * ids.size()) {
    std::printf("%s: %zu entries, expected %zu\n", what, table.size(), (L - 1) * ids.size());
    ++failures;
    return;
  }
  const size_t step = walk_all ? 1 : (L / 16 + 1);
  for (size_t l = 1; l < L; l += step) {
    for (size_t r = 0; r < ids.size(); ++r) {
      const int32_t want = Walk(hier, ids[r], l);
      if (table[(l - 1) * ids.size() + r] != want) {
        std::printf("%s: A_%zu(%d) = %d, expected %d\n", what, l, ids[r], table[(l - 1) * ids.size() + r], want);
        ++failures;
        return;
      }
    }
  }
}

// The tests' ladder: regions 0 .. L of level 0; at level l the regions 0 .. l are one, named 1000 l (ids above
// 65 levels would collide, so the name's step is `scale`), k > l is 1000 l + k.
Hier Ladder(int L, int64_t scale) {
  auto name = [&](int l, int k) { return (int32_t)(l == 0 ? k : scale * l + (k <= l ? 0 : k)); };
  Hier hier;
  if (L == 1) return hier;
  for (int l = 0; l < L; ++l) {
    std::vector<Ref> level;
    for (int k = 0; k <= L; ++k) {
      if (l > 0 && k <= l && k > 0) continue;   // merged into the level's first region
      level.push_back(Ref{name(l, k), l + 1 < L ? name(l + 1, k) : -1});
    }
    hier.push_back(level);
  }
  return hier;
}

}  // namespace

int main() {
  for (int L : {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 20}) {
    std::vector<int32_t> ids;
    for (int k = L; k >= 0; --k) ids.push_back(k);   // not in id order
    char what[32];
    std::snprintf(what, sizeof(what), "ladder %d", L);
    Check(what, Ladder(L, 1000), ids, true);
  }
  {
    // 65535 levels of two regions that never merge: the tallest hierarchy the calls accept
    Hier hier(65535);
    for (size_t l = 0; l < hier.size(); ++l) {
      const int32_t a = (int32_t)(2 * l), b = (int32_t)(2 * l + 1);
      hier[l] = {Ref{a, l + 1 < hier.size() ? a + 2 : -1}, Ref{b, l + 1 < hier.size() ? b + 2 : -1}};
    }
    Check("tallest", hier, {1, 0}, false);
  }
  {
    // three levels, sparse ids that reach 2^30, eight level-0 regions
    const int32_t big = (1 << 30) - 50;
    Hier hier(3);
    std::vector<int32_t> ids;
    for (int k = 0; k < 8; ++k) {
      hier[0].push_back(Ref{3 + 7 * k, big + 2 * (k / 2)});
      ids.push_back(3 + 7 * (7 - k));
    }
    for (int g = 0; g < 4; ++g) hier[1].push_back(Ref{big + 2 * g, g < 2 ? 1 : (1 << 30) + 7});
    hier[2] = {Ref{1, -1}, Ref{(1 << 30) + 7, -1}};
    Check("three levels", hier, ids, true);
    Check("three levels, no region", hier, {}, true);
    // an id the middle level lacks
    hier[0][5].parent_id = big + 1;
    std::vector<int32_t> table;
    int bad_level = -1;
    int32_t bad_id = -1;
    if (vsg_render_impl::BuildAncestorTable(hier, ids.data(), ids.size(), &table, &bad_level, &bad_id) ||
        bad_level != 1 || bad_id != big + 1) {
      std::printf("missing id: not refused at level 1 (%d, %d)\n", bad_level, bad_id);
      ++failures;
    }
    // an id level 0 lacks
    ids.push_back(4);
    if (vsg_render_impl::BuildAncestorTable(hier, ids.data(), ids.size(), &table, &bad_level, &bad_id) ||
        bad_level != 0 || bad_id != 4) {
      std::printf("missing id: not refused at level 0 (%d, %d)\n", bad_level, bad_id);
      ++failures;
    }
  }
  {
    Hier none;
    Check("no hierarchy", none, {5, 9, 2}, true);
    Check("nothing", none, {}, true);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
