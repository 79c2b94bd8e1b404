// The launchers of the fused LAMB's kernels (zs_lamb.hip).  The C entry points stand in
// zs_kernels.hip, which owns zs_adamset and has checked every argument: what arrives here is
// launched as it is.
#pragma once

#include <cstdint>

#include "zs_common.h"

namespace zs {

// A set's two tables as the update kernels take them (AdamSeg arrays with their chunk prefixes),
// and the grid of each: min(chunks, the update's cap for that table).
struct LambTables {
  const void* vec;
  const int64_t* vec_prefix;
  int64_t nvec, vec_chunks;
  const void* sca;
  const int64_t* sca_prefix;
  int64_t nsca, sca_chunks;
  int vec_grid, sca_grid;
  int g_dtype;  // ZS_F32 or ZS_BF16
  bool split;   // the split master's geometry
};

// zs_adamset_run_stats's partials: two planes of nslots doubles, and each table entry's first slot
struct LambPlanes {
  double* planes;
  int64_t nslots;
  const int64_t* vec_off;
  const int64_t* sca_off;
};

int lamb_moments(const LambTables& t, const zs_lamb_hparams& h, const float* coef,
                 const LambPlanes& planes, uintptr_t stream);
int lamb_finish(const float* sums3, int64_t n_params, const float* lr, float* norms2, float* ratios,
                float* neg_s, uintptr_t stream);
// entry_param: one parameter index per table entry, the vector table's first
int lamb_apply(const LambTables& t, const zs_lamb_hparams& h, const int32_t* entry_param,
               const float* neg_s, uintptr_t stream);

}  // namespace zs
