// Role-batched launch (gfx950, fp32): up to kStepMaxRoles of a training
// step's small fold / permute / copy kernels in ONE launch.  Each of them
// sits on the floor of a graph-replayed launch and none depends on a big
// kernel after it, so the step queues them and issues them together (see
// docs/KERNELS.md "Step batching").
//
// The table of roles travels by value in the kernel arguments.  A block
// finds its role by scanning the block prefix; the choice is uniform over
// the block, so a body may keep its barriers.  The bodies are the
// stand-alone kernels' bodies (step_roles.h), called with the block index
// inside the role and the role's own grid size: what a role writes is
// bitwise what its stand-alone kernel writes.  No atomics, no grid sync;
// roles of one launch must not depend on each other.
#include "common.h"
#include "launchers.h"
#include "step_roles.h"

struct StepTable {
  int n;
  StepRole r[kStepMaxRoles];
};

__global__ __launch_bounds__(kBlock)
void step_batch_k(const StepTable t) {
  __shared__ float sh[kBlock];
  const int ri = step_role_of(t.r, t.n, (int)blockIdx.x);
  if (ri < 0) return;
  const StepRole& r = t.r[ri];
  const int v = (int)blockIdx.x - r.first;
  const int bx = v % r.gx, by = v / r.gx;
  const int gx = r.gx;
  switch (r.kind) {
    case kRoleConvDbStage1:
      conv_db_stage1_body(bx, by, (const float*)r.p[0], (float*)r.p[1], r.l0,
                          r.i[0], r.i[1], r.i[2]);
      break;
    case kRoleConvDbStage2:
      conv_db_stage2_body(bx, (const float*)r.p[0], (float*)r.p[1], r.i[0],
                          r.i[1], sh);
      break;
    case kRoleSplitkPartial:
      splitk_partial_body(bx, gx, (const float*)r.p[0], (float*)r.p[1], r.l0,
                          r.i[0], r.i[1]);
      break;
    case kRoleSplitkReduce:
      splitk_reduce_body(bx, gx, (const float*)r.p[0], (float*)r.p[1],
                         (const float*)r.p[2], r.i[0], r.i[1], r.i[2],
                         r.i[3], r.i[4]);
      break;
    case kRoleSplitkReduceDwperm:
      splitk_reduce_dwperm_body(bx, gx, (const float*)r.p[0],
                                (float*)r.p[1], r.i[0], r.i[1], r.i[2],
                                r.i[3]);
      break;
    case kRoleConvSmallBwdwReduce:
      conv_small_bwdw_reduce_body(bx, (const float*)r.p[0], (float*)r.p[1],
                                  r.i[0], r.i[1], r.i[2], r.i[3]);
      break;
    case kRoleColsum:
      colsum_body(bx, (const float*)r.p[0], (float*)r.p[1], r.i[0], r.i[1]);
      break;
    case kRoleFcHeadReduce:
      fc_head_reduce_body(bx, (const float*)r.p[0], (const float*)r.p[1],
                          (const float*)r.p[2], (float*)r.p[3],
                          (float*)r.p[4], (float*)r.p[5], r.i[0], r.i[1],
                          r.i[2], r.i[3], r.i[4], r.i[5], sh);
      break;
    case kRoleWpermRscKo:
      wperm_rsc_ko_body(bx, gx, (const float*)r.p[0], (float*)r.p[1], r.i[0],
                        r.i[1], r.i[2]);
      break;
    case kRoleWpermRskoC:
      wperm_rsko_c_body(bx, gx, (const float*)r.p[0], (float*)r.p[1], r.i[0],
                        r.i[1], r.i[2]);
      break;
    case kRoleGatherRows:
      gather_rows_body(bx, gx, (const uint32_t*)r.p[0], (const long*)r.p[1],
                       (uint32_t*)r.p[2], r.l0, r.i[0], r.i[1], r.i[2]);
      break;
    case kRoleAddU64:
      add_u64_body((unsigned long long*)r.p[0], (unsigned long long)r.l0);
      break;
    default:
      break;
  }
}

extern "C" {

int step_batch_max_roles() { return kStepMaxRoles; }

// first[r] = sum of counts[0 .. r); returns the total block count
int step_batch_plan(const int* counts, int n, int* first) {
  int total = 0;
  for (int r = 0; r < n; ++r) {
    first[r] = total;
    total += counts[r] > 0 ? counts[r] : 0;
  }
  return total;
}

// the role (and, in *vblock, the block index inside it) that flat block
// `block` of a launch planned from `counts` runs; -1 when it runs none.
// The kernel's own scan (step_role_of), on the planned table.
int step_batch_lookup(const int* counts, int n, int block, int* vblock) {
  StepRole roles[kStepMaxRoles] = {};
  int first[kStepMaxRoles];
  if (n < 0 || n > kStepMaxRoles) return -1;
  step_batch_plan(counts, n, first);
  for (int r = 0; r < n; ++r) {
    roles[r].first = first[r];
    roles[r].count = counts[r] > 0 ? counts[r] : 0;
  }
  int ri = step_role_of(roles, n, block);
  if (ri >= 0 && vblock) *vblock = block - roles[ri].first;
  return ri;
}

// returns 0, or -1 (nothing launched) when n > kStepMaxRoles
int launch_step_batch(const StepRole* roles, int n, void* s) {
  if (n <= 0) return 0;
  if (n > kStepMaxRoles) return -1;
  StepTable t{};
  int counts[kStepMaxRoles], first[kStepMaxRoles];
  for (int r = 0; r < n; ++r) counts[r] = roles[r].count;
  int total = step_batch_plan(counts, n, first);
  if (total <= 0) return 0;
  t.n = n;
  for (int r = 0; r < n; ++r) {
    t.r[r] = roles[r];
    t.r[r].first = first[r];
    if (t.r[r].count < 0) t.r[r].count = 0;
    if (t.r[r].gx < 1) t.r[r].gx = 1;
  }
  step_batch_k<<<total, kBlock, 0, (hipStream_t)s>>>(t);
  return 0;
}

// dst row r = src row sel[r], rows of row_words 32-bit words; sel must
// index [0, src_rows) (gather_rows_body never reads outside it)
StepRole step_role_gather_rows(const void* src, const long* sel, void* dst,
                               long rows, int row_words, int src_rows) {
  int vec = (row_words % 4) == 0 && ((uintptr_t)src % 16) == 0 &&
            ((uintptr_t)dst % 16) == 0;
  long items = rows * (vec ? row_words / 4 : row_words);
  StepRole r{};
  r.kind = kRoleGatherRows;
  r.gx = items > 0 ? grid_for(items) : 0;
  r.gy = 1;
  r.count = r.gx;
  r.p[0] = src; r.p[1] = sel; r.p[2] = dst;
  r.l0 = rows;
  r.i[0] = row_words; r.i[1] = vec; r.i[2] = src_rows;
  return r;
}

StepRole step_role_add_u64(unsigned long long* p, unsigned long long delta) {
  StepRole r{};
  r.kind = kRoleAddU64;
  r.gx = 1;
  r.gy = 1;
  r.count = 1;
  r.p[0] = p;
  r.l0 = (long)delta;
  return r;
}
}
