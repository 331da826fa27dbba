// =====================================================================================================
// mw_stack_shape.h -- the shape limits of a dense surrogate stack n_in -> H1 -> ... -> HL -> 4 and their ONE host check, shared by the unit
// that runs stacks (mw_mlp_stack.hip) and the unit that trains them (mw_train_stack.hip): what can be trained can be run, nothing else.
// =====================================================================================================
#pragma once
#include "mw_common.h"
#include <cmath>
#include <string>

#define MW_STACK_MAX_HIDDEN 4
#define MW_STACK_MAX_WIDTH 64
#define MW_STACK_DENSE (MW_STACK_MAX_HIDDEN + 1)                   // Dense layers of the deepest model
#define MW_STACK_UB (MW_STACK_MAX_WIDTH / 16)                      // unit blocks of the widest layer

namespace mw {

// Refuses (return 1, error text set, prefixed with `who`) n_in other than 5 or 9, a depth outside [1, 4], a null pointer (widths, slopes,
// or `other_null`: the caller's own pointers, tested at the same place), a width outside [1, 64], a negative or non-finite slope.
// *need: the parameter count of the shape, W (in, out) then b per Dense.
inline int stack_shape_check(const char *who, int n_in, int nhidden, const int *widths, const float *slopes, bool other_null, long long *need) {
  const std::string w(who);
  if (n_in != 5 && n_in != 9) MW_FAIL(w + ": n_in must be 5 (single cell) or 9 (stencil), got " + std::to_string(n_in));
  if (nhidden < 1 || nhidden > MW_STACK_MAX_HIDDEN)
    MW_FAIL(w + ": the number of hidden layers must be in [1, " + std::to_string(MW_STACK_MAX_HIDDEN) + "], got " + std::to_string(nhidden));
  if (!widths || !slopes || other_null) MW_FAIL(w + ": null pointer");
  *need = 0;
  for (int l = 0; l < nhidden; l++) {
    if (widths[l] < 1 || widths[l] > MW_STACK_MAX_WIDTH)
      MW_FAIL(w + ": hidden layer " + std::to_string(l) + " has " + std::to_string(widths[l]) + " units; a width is in [1, " + std::to_string(MW_STACK_MAX_WIDTH) + "]");
    if (!(slopes[l] >= 0.f) || std::isinf(slopes[l]))
      MW_FAIL(w + ": the slope of hidden layer " + std::to_string(l) + " must be finite and >= 0");
    *need += (long long)((l ? widths[l - 1] : n_in) + 1) * widths[l];
  }
  *need += (long long)(widths[nhidden - 1] + 1) * 4;
  return 0;
}

} // namespace mw
