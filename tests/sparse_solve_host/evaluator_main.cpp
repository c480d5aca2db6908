// The argument checks of the evaluator's entries on the sparse handle (calipso.jl_amd/csrc/sparse_solve.hpp: check_evaluate, check_set_evaluator,
// check_set_parameters, and the names get answers besides the vectors) on the CPU, under the address and undefined-behaviour sanitizers
// (tests/test_trajectory_sparse_route_cpu.py).  Prints one line per check: the refusal's text, or "ok".
#include <cstdio>
#include <string>

#include "../../calipso.jl_amd/csrc/sparse_solve.hpp"
#include "../../calipso.jl_amd/csrc/step_decisions.hpp"

using namespace calipso::sparse_solve;

static void show(const std::string& text) { std::printf("%s\n", text.empty() ? "ok" : text.c_str()); }

int main() {
    const uint32_t every = EVAL_EVERYTHING;
    show(check_evaluate(0, every));
    show(check_evaluate(1, EVAL_POINT));
    show(check_evaluate(2, every));
    show(check_evaluate(0, 0));
    for (int bit = 11; bit < 16; ++bit) show(check_evaluate(0, every | (1u << bit)));
    show(check_evaluate(0, every | (1u << 5)));
    show(check_evaluate(0, every | (1u << 9)));
    show(check_evaluate(0, every | (1u << 16)));
    show(check_set_evaluator(0));
    show(check_set_evaluator(-1));
    double x = 0.0;
    show(check_set_parameters("set_parameters", true, 3, &x));
    show(check_set_parameters("set_parameters", true, 0, nullptr));
    show(check_set_parameters("set_parameters", true, 3, nullptr));
    show(check_set_parameters("set_parameters", false, 0, nullptr));
    const calipso::i64 nnz[3] = {40, 30, 20};
    for (int v = V_OBJECTIVE; v < V_NAMED; ++v) std::printf("%s %lld %lld\n", vector_name(v), (long long)vector_length(v, 12, 4, 12, nnz), (long long)vector_length(v, 12, 4, 12));
    show(check_named_vector("get", "lagrangian_hessian", &x, 40, 12, 4, 12, false, nnz));
    show(check_named_vector("get", "lagrangian_hessian", &x, 41, 12, 4, 12, false, nnz));
    show(check_named_vector("set", "equality_jacobian_variables", &x, 30, 12, 4, 12, true, nnz));
    std::printf("flags %u %u\n", EVAL_EVERYTHING, EVAL_POINT);
    std::printf("done\n");
    return 0;
}
