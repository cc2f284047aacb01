// group_plan_check.cpp -- host-only checks of the partition of a compiled
// space into groups of hps that are always active together, and of the layout
// the group kernels index by (tpe_group_plan.hpp).  The condition tables are
// built by hand and every expected value is written out from the documented
// rules; none is computed by the code under test.
// Built and run by tests/test_group_host.py; exit status 0: all checks passed.
#include <cstdio>

#include "../../hyperopt_amd/csrc/tpe_group_plan.hpp"

using namespace tpe;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static_assert(kCoefBlock == 8 && kJointFields == 3, "constants the cases use");

typedef std::vector<int32_t> V;

static tpe_hp uniform_hp() {
  tpe_hp x{};
  x.family = TPE_GMM;
  x.flags = TPE_HAS_LOW | TPE_HAS_HIGH;
  x.prior_sigma = 1.0;
  x.high = 1.0;
  return x;
}
static tpe_hp quniform_hp() {
  tpe_hp x = uniform_hp();
  x.flags |= TPE_HAS_Q;
  x.q = 1.0;
  return x;
}
static tpe_hp choice_hp(int upper) {
  tpe_hp x{};
  x.family = TPE_CAT;
  x.upper = upper;
  return x;
}

// the condition tables of a space: conds[i] = the (parent, branch) list of hp i
struct Space {
  std::vector<tpe_hp> hps;
  V parent, branch;
  void add(tpe_hp x, const std::vector<std::pair<int, int>> &conds) {
    x.cond_begin = (int32_t)parent.size();
    x.cond_count = (int32_t)conds.size();
    for (auto &c : conds) { parent.push_back(c.first); branch.push_back(c.second); }
    hps.push_back(x);
  }
};

static void flat_space() {
  Space s;
  for (int i = 0; i < 3; ++i) s.add(uniform_hp(), {});
  const GroupPartition gp = group_partition(s.hps, s.parent, s.branch);
  CHECK(gp.group_of_hp == (V{0, 0, 0}));
  CHECK(gp.members.size() == 1 && gp.members[0] == (V{0, 1, 2}));
  const GroupLayout L = group_layout(gp, s.hps, V{0, 1, 2}, 64);
  CHECK(L.groups.size() == 1 && L.groups[0].lead == 0 && L.groups[0].n_dim == 3);
  CHECK(L.groups[0].n_slots == 3 && L.max_slots == 3 && L.n_opt == 0);
  CHECK(L.tab_doubles == 2 * 8 * 8 * (1 + 3 * 3));
}

// hp 3 is the root choice although hps 0..2 come first; hps 4 and 5 hang under
// two branches (listed in different orders); hp 6 lists one condition twice;
// hp 7 is nested under hp 2
static Space branched() {
  Space s;
  s.add(uniform_hp(), {{3, 0}});           // 0
  s.add(quniform_hp(), {{3, 0}});          // 1
  s.add(choice_hp(2), {{3, 1}});           // 2
  s.add(choice_hp(2), {});                 // 3
  s.add(uniform_hp(), {{3, 1}, {3, 0}});   // 4
  s.add(uniform_hp(), {{3, 0}, {3, 1}});   // 5
  s.add(choice_hp(3), {{3, 0}, {3, 0}});   // 6
  s.add(uniform_hp(), {{2, 1}});           // 7
  return s;
}

static void branched_partition() {
  const Space s = branched();
  const GroupPartition gp = group_partition(s.hps, s.parent, s.branch);
  // group 0 the root; then by smallest hp index: {0, 1, 6}, {2}, {4, 5}, {7}
  CHECK(gp.group_of_hp == (V{1, 1, 2, 0, 3, 3, 1, 4}));
  CHECK(gp.members.size() == 5);
  CHECK(gp.members[0] == (V{3}));
  CHECK(gp.members[1] == (V{0, 1, 6}));
  CHECK(gp.members[2] == (V{2}));
  CHECK(gp.members[3] == (V{4, 5}));
  CHECK(gp.members[4] == (V{7}));
}

static void branched_layout() {
  const Space s = branched();
  const GroupPartition gp = group_partition(s.hps, s.parent, s.branch);
  // parents first; inside the first level below the root hp 1 comes before hp 0
  const GroupLayout L = group_layout(gp, s.hps, V{3, 1, 0, 6, 2, 4, 5, 7}, 64);
  CHECK(L.groups.size() == 5 && L.dims.size() == 8);
  const int lead[5] = {3, 1, 2, 4, 7}, begin[5] = {0, 1, 4, 5, 7}, ndim[5] = {1, 3, 1, 2, 1};
  // slots: LSE 1, ERF 2, CAT 4
  const int slots[5] = {4, 1 + 2 + 4, 4, 2, 1};
  int64_t off = 0;
  for (int g = 0; g < 5; ++g) {
    CHECK(L.groups[g].lead == lead[g]);
    CHECK(L.groups[g].dim_begin == begin[g]);
    CHECK(L.groups[g].n_dim == ndim[g]);
    CHECK(L.groups[g].n_slots == slots[g]);
    CHECK(L.groups[g].tab_off == off);
    off += 2 * (64 / 8) * 8 * (1 + 3 * ndim[g]);  // [side][block][8 log2 w | 3 x 8 per dim]
  }
  CHECK(L.tab_doubles == off);
  CHECK(L.max_slots == 7);
  // dims group by group, ascending hp index inside a group
  const int hp_of_dim[8] = {3, 0, 1, 6, 2, 4, 5, 7};
  const int slot_of_dim[8] = {0, 0, 1, 3, 0, 0, 1, 0};
  for (int d = 0; d < 8; ++d) {
    CHECK(L.dims[d].hp == hp_of_dim[d]);
    CHECK(L.dims[d].slot == slot_of_dim[d]);
    CHECK(L.dim_of_hp[hp_of_dim[d]] == d);
  }
  CHECK(L.dims[0].kind == KIND_CAT && L.dims[1].kind == KIND_LSE_G && L.dims[2].kind == KIND_ERF_G);
  // options: hp 3 (2), hp 6 (3), hp 2 (2), in dim order
  CHECK(L.dims[0].opt_off == 0 && L.dims[0].upper == 2);
  CHECK(L.dims[3].opt_off == 2 && L.dims[3].upper == 3);
  CHECK(L.dims[4].opt_off == 5 && L.dims[4].upper == 2);
  CHECK(L.dims[1].upper == 0 && L.n_opt == 7);
}

// group 0 exists even when no hp is unconditional (the engine rejects the fit)
static void no_root() {
  Space s;
  s.add(choice_hp(2), {{1, 0}});
  s.add(choice_hp(2), {{0, 0}});
  const GroupPartition gp = group_partition(s.hps, s.parent, s.branch);
  CHECK(gp.group_of_hp == (V{1, 2}));
  CHECK(gp.members.size() == 3 && gp.members[0].empty());
}

int main() {
  flat_space();
  branched_partition();
  branched_layout();
  no_root();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("group plan checks passed\n");
  return 0;
}
