// calipso_options.hpp — options.jl:6-59 as one C++ struct, shared by libcalipso_hip.so and by the user libraries that instantiate the batched small-problem
// kernels (calipso_smallnewton.hpp): the kernels take it by value, so both sides must see the same layout.
#pragma once
#include <stdint.h>

namespace calipso {

typedef int64_t i64;

// options.jl:6-59 (hot-path relevant subset + the rest for API parity)
struct Options {
    double residual_norm = 1.0, constraint_norm = 1.0;
    i64 max_outer_iterations = 10, max_residual_iterations = 100;
    double scaling_line_search = 0.5;
    i64 max_residual_line_search = 25, max_cone_line_search = 25;
    i64 iterative_refinement = 1, max_iterative_refinement = 10, min_iterative_refinement = 1;
    double iterative_refinement_tolerance = 1.0e-10;
    double central_path_initial = 1.0, central_path_update_tolerance = 10.0, central_path_scaling = 0.2, central_path_exponent = 1.5;
    double penalty_initial = 1.0, penalty_scaling = 10.0, dual_initial = 0.0;
    double residual_tolerance = 1.0e-4, optimality_tolerance = 1.0e-4, slack_tolerance = 1.0e-4, equality_tolerance = 1.0e-4,
           complementarity_tolerance = 1.0e-4;
    double min_regularization = 1.0e-20, primal_regularization_initial = 1.0e-7, dual_regularization_initial = 1.0e-7,
           max_regularization = 1.0e40, dual_regularization = 1.0e-8, dual_regularization_exponent = 0.25,
           scaling_regularization_initial = 100.0, scaling_regularization = 8.0, scaling_regularization_last = 1.0 / 3.0;
    double min_central_path = 1.0e-8, max_penalty = 1.0e8;
    double constraint_tensor = 1.0, update_factorization = 1.0;
    double violation_tolerance = 1.0e-5, violation_exponent = 1.1, merit_tolerance = 1.0e-5, merit_exponent = 2.3,
           armijo_tolerance = 1.0e-4, machine_tolerance = 1.0e-16;
    double max_filter = 1000, differentiate = 1.0, warmstart = 0.0;
};

}  // namespace calipso
