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

// the regularisation and refinement options (inertia.jl:30-80, iterative_refinement.jl:1-52) by name: one table for the set_option entry of a handle that runs
// search_direction! alone.  false: `name` is none of them
inline bool set_search_direction_option(Options& o, const char* name, double value) {
    struct Real { const char* name; double Options::*field; };
    struct Int { const char* name; i64 Options::*field; };
    static const Real reals[] = {{"iterative_refinement_tolerance", &Options::iterative_refinement_tolerance}, {"min_regularization", &Options::min_regularization},
                                 {"primal_regularization_initial", &Options::primal_regularization_initial}, {"dual_regularization_initial", &Options::dual_regularization_initial},
                                 {"max_regularization", &Options::max_regularization}, {"dual_regularization", &Options::dual_regularization},
                                 {"dual_regularization_exponent", &Options::dual_regularization_exponent}, {"scaling_regularization_initial", &Options::scaling_regularization_initial},
                                 {"scaling_regularization", &Options::scaling_regularization}, {"scaling_regularization_last", &Options::scaling_regularization_last}};
    static const Int ints[] = {{"iterative_refinement", &Options::iterative_refinement}, {"max_iterative_refinement", &Options::max_iterative_refinement},
                               {"min_iterative_refinement", &Options::min_iterative_refinement}};
    const auto same = [](const char* a, const char* b) { while (*a && *a == *b) { ++a; ++b; } return *a == *b; };
    for (const Real& r : reals) if (same(r.name, name)) { o.*(r.field) = value; return true; }
    for (const Int& r : ints) if (same(r.name, name)) { o.*(r.field) = (i64)value; return true; }
    return false;
}

}  // namespace calipso
