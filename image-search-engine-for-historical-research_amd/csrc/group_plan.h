// The host half of mi_gallery_set_groups (api_group.hip): the caller's labels -> the dense relabelling the kernels
// of group_select.hip read.  Plain C++, nothing of HIP: a stand-alone program can include it alone (tests/group_plan_check.cpp).
//   labels >= 0 name a group, -1 makes the row a group of its own, anything else is refused
//   dense ids: the labelled groups first, in ascending label order (so the dense id of a label is its place in `sorted_labels`),
//   then the singleton rows in row order
//   group_off / group_rows: the CSR of the groups, the rows of a group ascending (a stable sort of the rows by group)
//   chunk_g0: the groups cut into chunks of whole groups of at most `chunk_rows` rows; a larger group is a chunk of its own
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

struct GroupPlan {
  std::vector<uint32_t> grp;             // [n] dense group of a row
  std::vector<int32_t> label_of_group;   // [G] the caller's label, -1 for a singleton row
  std::vector<uint32_t> group_off;       // [G + 1]
  std::vector<uint32_t> group_rows;      // [n]
  std::vector<uint32_t> chunk_g0;        // [chunks + 1]
  std::vector<int32_t> sorted_labels;    // the labels >= 0 in use, ascending
  int64_t groups() const { return (int64_t)label_of_group.size(); }
  int64_t chunks() const { return chunk_g0.empty() ? 0 : (int64_t)chunk_g0.size() - 1; }
};

constexpr uint32_t GROUP_NONE = 0xFFFFFFFFu;

// false: a label below -1 (nothing of *p is meaningful then).  n < 2^32 - 1
static inline bool group_plan_build(const int32_t* labels, int64_t n, int64_t chunk_rows, GroupPlan* p) {
  *p = GroupPlan();
  for (int64_t i = 0; i < n; ++i)
    if (labels[i] < -1) return false;
  auto sort_key = [&](uint32_t r) { return labels[r] >= 0 ? (uint64_t)labels[r] : ((uint64_t)1 << 31) + r; };
  p->group_rows.resize((size_t)n);
  std::iota(p->group_rows.begin(), p->group_rows.end(), 0u);
  std::stable_sort(p->group_rows.begin(), p->group_rows.end(), [&](uint32_t a, uint32_t b) { return sort_key(a) < sort_key(b); });
  p->grp.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t r = p->group_rows[(size_t)i];
    if (i == 0 || sort_key(r) != sort_key(p->group_rows[(size_t)i - 1])) {
      p->group_off.push_back((uint32_t)i);
      p->label_of_group.push_back(labels[r]);
      if (labels[r] >= 0) p->sorted_labels.push_back(labels[r]);
    }
    p->grp[r] = (uint32_t)p->label_of_group.size() - 1;
  }
  p->group_off.push_back((uint32_t)n);
  const int64_t G = p->groups();
  p->chunk_g0.push_back(0);
  int64_t held = 0;                      // rows of the chunk being filled
  for (int64_t g = 0; g < G; ++g) {
    const int64_t size = (int64_t)p->group_off[(size_t)g + 1] - p->group_off[(size_t)g];
    if (held > 0 && held + size > chunk_rows) {
      p->chunk_g0.push_back((uint32_t)g);
      held = 0;
    }
    held += size;
  }
  if (G > 0) p->chunk_g0.push_back((uint32_t)G);
  return true;
}

// the dense id of the group that carries `label`, GROUP_NONE when no row does (or the label is negative)
static inline uint32_t group_plan_find(const GroupPlan& p, int32_t label) {
  if (label < 0) return GROUP_NONE;
  const auto it = std::lower_bound(p.sorted_labels.begin(), p.sorted_labels.end(), label);
  return it != p.sorted_labels.end() && *it == label ? (uint32_t)(it - p.sorted_labels.begin()) : GROUP_NONE;
}
