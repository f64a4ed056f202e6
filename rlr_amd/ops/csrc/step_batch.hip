// The two kernels that run a step's roles (gfx950, fp32).  A role is one of
// a training step's small fold / permute / copy kernels as data: a StepRole
// (launchers.h) made by the maker beside the kernels it belongs to, run by
// step_role_run (step_roles.h).  step_role_k<KIND> runs one role alone, now;
// step_batch_k runs up to kStepMaxRoles of them in ONE launch.  Each of them
// sits on the floor of a graph-replayed launch and none depends on a big
// kernel after it, so the step queues them and issues them together (see
// docs/KERNELS.md "Step batching").
//
// The table of roles travels by value in the kernel arguments.  A block
// finds its role by scanning the block prefix; the choice is uniform over
// the block, so a body may keep its barriers.  Both kernels call the same
// step_role_run with the block index inside the role's grid: what a role
// writes in a batch is bitwise what it writes alone.  No atomics, no grid
// sync; roles of one launch must not depend on each other.
#include <utility>

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
  step_role_run(r.kind, r, v % r.gx, v / r.gx, sh);
}

// one role on its own grid (gx, gy); LDS only for the kinds that use it
template <int KIND>
__global__ __launch_bounds__(kBlock)
void step_role_k(const StepRole r) {
  float* sh = nullptr;
  if constexpr (step_role_uses_lds(KIND)) {
    __shared__ float lds[kBlock];
    sh = lds;
  }
  step_role_run(KIND, r, (int)blockIdx.x, (int)blockIdx.y, sh);
}

// step_role_k<kind>, one instantiation per StepRoleKind
using StepRoleKernel = void (*)(StepRole);
template <int... KIND>
static StepRoleKernel step_role_kernel(int kind,
                                       std::integer_sequence<int, KIND...>) {
  static const StepRoleKernel table[] = {step_role_k<KIND>...};
  return table[kind];
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

// returns 0, or -1 (nothing launched) for a kind that does not exist
int launch_step_role(const StepRole* r, void* s) {
  if (r->kind < 0 || r->kind >= kStepRoleKinds) return -1;
  if (r->count <= 0) return 0;
  StepRoleKernel k = step_role_kernel(
      r->kind, std::make_integer_sequence<int, kStepRoleKinds>{});
  k<<<dim3(r->gx, r->gy), kBlock, 0, (hipStream_t)s>>>(*r);
  return 0;
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
// index [0, src_rows) (the body never reads outside it)
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
  r.gather_rows.src = (const uint32_t*)src;
  r.gather_rows.sel = sel;
  r.gather_rows.dst = (uint32_t*)dst;
  r.gather_rows.rows = rows;
  r.gather_rows.row_words = row_words;
  r.gather_rows.vec = vec;
  r.gather_rows.src_rows = src_rows;
  return r;
}

StepRole step_role_add_u64(unsigned long long* p, unsigned long long delta) {
  StepRole r{};
  r.kind = kRoleAddU64;
  r.gx = 1;
  r.gy = 1;
  r.count = 1;
  r.add_u64.p = p;
  r.add_u64.delta = delta;
  return r;
}
}
