// tpe_group_plan.hpp -- the groups of the per-group joint model, as data.
// Pure host code: group_partition maps a compiled space's condition tables to
// the partition of its hps into sets that are always active together, and
// group_layout to what the kernels of tpe_group.hip index by.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "tpe_internal.hpp"

namespace tpe {

// A group is a maximal set of hps with the same set of immediate
// (parent, branch) alternatives.  Group 0 holds the hps without a condition
// (it exists even when empty); the others follow in ascending order of their
// smallest hp index.  Members are kept in ascending hp index.
struct GroupPartition {
  std::vector<int32_t> group_of_hp;            // [P]
  std::vector<std::vector<int32_t>> members;   // [G]
};

inline GroupPartition group_partition(const std::vector<tpe_hp> &hps,
                                      const std::vector<int32_t> &cond_parent,
                                      const std::vector<int32_t> &cond_branch) {
  typedef std::vector<std::pair<int32_t, int32_t>> Key;
  GroupPartition gp;
  gp.group_of_hp.assign(hps.size(), 0);
  gp.members.assign(1, {});
  std::map<Key, int32_t> seen;
  seen[Key()] = 0;
  for (size_t i = 0; i < hps.size(); ++i) {
    const tpe_hp &x = hps[i];
    Key key;
    for (int c = 0; c < x.cond_count; ++c)
      key.emplace_back(cond_parent[(size_t)x.cond_begin + c], cond_branch[(size_t)x.cond_begin + c]);
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    auto it = seen.find(key);
    if (it == seen.end()) {
      it = seen.emplace(key, (int32_t)gp.members.size()).first;
      gp.members.emplace_back();
    }
    gp.group_of_hp[i] = it->second;
    gp.members[(size_t)it->second].push_back((int32_t)i);
  }
  return gp;
}

// The dims of every group back to back (group by group, ascending hp index in
// a group; JointDim::slot counts from 0 in each group, opt_off over all dims),
// and per group its descriptor.  level_hps: every hp, parents first -- a
// group's lead is its first hp in that order.
struct GroupLayout {
  std::vector<JointDim> dims;        // [P]
  std::vector<int32_t> dim_of_hp;    // [P] index into dims
  std::vector<GroupDesc> groups;     // [G]
  int32_t max_slots = 0;             // the widest group's staged values
  int64_t n_opt = 0;                 // options of all categorical hps
  int64_t tab_doubles = 0;           // all groups' scoring tables
};

inline GroupLayout group_layout(const GroupPartition &gp, const std::vector<tpe_hp> &hps,
                                const std::vector<int32_t> &level_hps, int64_t kcap) {
  GroupLayout L;
  L.dim_of_hp.assign(hps.size(), -1);
  std::vector<int32_t> pos(hps.size(), 0);
  for (size_t j = 0; j < level_hps.size(); ++j) pos[(size_t)level_hps[j]] = (int32_t)j;
  for (const std::vector<int32_t> &mem : gp.members) {
    GroupDesc g{};
    g.dim_begin = (int32_t)L.dims.size();
    g.n_dim = (int32_t)mem.size();
    g.lead = -1;
    g.tab_off = L.tab_doubles;
    int32_t slot = 0;
    for (int32_t hp : mem) {
      const tpe_hp &x = hps[(size_t)hp];
      JointDim d{};
      d.hp = hp;
      d.kind = score_kind(x);
      d.slot = slot;
      d.upper = x.family == TPE_CAT ? x.upper : 0;
      d.opt_off = L.n_opt;
      slot += joint_slots(d.kind);
      L.n_opt += d.upper;
      L.dim_of_hp[(size_t)hp] = (int32_t)L.dims.size();
      L.dims.push_back(d);
      if (g.lead < 0 || pos[(size_t)hp] < pos[(size_t)g.lead]) g.lead = hp;
    }
    g.n_slots = slot;
    L.max_slots = std::max(L.max_slots, slot);
    L.tab_doubles += 2 * (kcap / kCoefBlock) * joint_stride(g.n_dim);
    L.groups.push_back(g);
  }
  return L;
}

}  // namespace tpe
