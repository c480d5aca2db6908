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

// every other option solve! reads (solve.jl:8-377, merit.jl, filter.jl, line_search.jl, initialize.jl:38-48) by name, for the set_option entry of a handle that runs a
// whole solve!.  residual_norm and constraint_norm are not in it: the kernels take the 1-norms, the options' defaults.  false: `name` is none of them
inline bool set_solve_option(Options& o, const char* name, double value) {
    struct Real { const char* name; double Options::*field; };
    struct Int { const char* name; i64 Options::*field; };
    static const Real reals[] = {{"scaling_line_search", &Options::scaling_line_search}, {"central_path_initial", &Options::central_path_initial},
                                 {"central_path_update_tolerance", &Options::central_path_update_tolerance}, {"central_path_scaling", &Options::central_path_scaling},
                                 {"central_path_exponent", &Options::central_path_exponent}, {"penalty_initial", &Options::penalty_initial},
                                 {"penalty_scaling", &Options::penalty_scaling}, {"dual_initial", &Options::dual_initial}, {"residual_tolerance", &Options::residual_tolerance},
                                 {"optimality_tolerance", &Options::optimality_tolerance}, {"slack_tolerance", &Options::slack_tolerance},
                                 {"equality_tolerance", &Options::equality_tolerance}, {"complementarity_tolerance", &Options::complementarity_tolerance},
                                 {"max_penalty", &Options::max_penalty}, {"violation_tolerance", &Options::violation_tolerance}, {"violation_exponent", &Options::violation_exponent},
                                 {"merit_tolerance", &Options::merit_tolerance}, {"merit_exponent", &Options::merit_exponent}, {"armijo_tolerance", &Options::armijo_tolerance},
                                 {"machine_tolerance", &Options::machine_tolerance}, {"max_filter", &Options::max_filter}, {"warmstart", &Options::warmstart}};
    static const Int ints[] = {{"max_outer_iterations", &Options::max_outer_iterations}, {"max_residual_iterations", &Options::max_residual_iterations},
                               {"max_residual_line_search", &Options::max_residual_line_search}, {"max_cone_line_search", &Options::max_cone_line_search}};
    const auto same = [](const char* a, const char* b) { while (*a && *a == *b) { ++a; ++b; } return *a == *b; };
    for (const Real& r : reals) if (same(r.name, name)) { o.*(r.field) = value; return true; }
    for (const Int& r : ints) if (same(r.name, name)) { o.*(r.field) = (i64)value; return true; }
    return false;
}

}  // namespace calipso
