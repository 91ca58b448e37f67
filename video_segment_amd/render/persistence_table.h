// persistence_table.h -- the ancestor table of the boundary persistence calls, built on the host.
//
// For R region ids and a hierarchy of L = max(1, levels) levels the table has L - 1 rows of R int32:
// row l - 1 holds A_l(r) = GetParentId(r, 0, l) of every region, l in [1, L).  A_0 is the id itself and
// is not stored.  Row l is made from row l - 1 with one binary search per region in hierarchy level l
// (A_{l+1} = parent_l(A_l)), so the whole table costs (L - 1) * R searches; the top level is never
// searched, as in vsg_render_id_image at level L - 1.
//
// Host code without a device dependency, so that a stand-alone program can run it under a sanitizer
// (persistence_table_check.cpp).
#ifndef VSG_RENDER_PERSISTENCE_TABLE_H_
#define VSG_RENDER_PERSISTENCE_TABLE_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vsg_render_impl {

// Height of a hierarchy with `levels` levels: a desc without one has the one level of its regions.
inline size_t PersistenceHeight(size_t levels) { return levels ? levels : 1; }

// hier[l] is sorted by .id and has .id and .parent_id.  table receives (L - 1) * n_ids values.  Returns
// true, or false with the level and the id that level lacks.
template <class Hier>
bool BuildAncestorTable(const Hier& hier, const int32_t* ids, size_t n_ids, std::vector<int32_t>* table,
                        int* bad_level, int32_t* bad_id) {
  const size_t L = PersistenceHeight(hier.size());
  table->assign((L - 1) * n_ids, 0);
  const int32_t* below = ids;
  for (size_t l = 0; l + 1 < L; ++l) {
    const auto& level = hier[l];
    int32_t* row = table->data() + l * n_ids;
    for (size_t r = 0; r < n_ids; ++r) {
      const int32_t id = below[r];
      auto it = std::lower_bound(level.begin(), level.end(), id,
                                 [](const decltype(*level.begin())& c, int32_t key) { return c.id < key; });
      if (it == level.end() || it->id != id) {
        *bad_level = (int)l;
        *bad_id = id;
        return false;
      }
      row[r] = it->parent_id;
    }
    below = row;
  }
  return true;
}

}  // namespace vsg_render_impl

#endif  // VSG_RENDER_PERSISTENCE_TABLE_H_
