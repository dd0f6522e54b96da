// Argument of the plan-emitting kernel variants (pilot_ot_plans.hip): an explicit list of ordered pairs and the dense K x K
// output of each.  Kept apart from EmdParams / GenericParams so that the pair-grid kernels load exactly what they loaded before.
#pragma once

namespace pilot {

struct PlanArgs {
    const int *pair_i, *pair_j;    // n_pairs rows (a = P[pair_i]) and columns (b = P[pair_j])
    long n_pairs;
    double *plans;                 // n_pairs x K x K, row-major; item t writes plans[t K^2 ..]
};

}  // namespace pilot
