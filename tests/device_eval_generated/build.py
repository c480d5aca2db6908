"""Generate and compile the evaluators of problems.py: BUILT into this directory (test fixtures of tests/test_gpu_codegen.py, built by `python __graft_entry__.py build`).
Each takes about a minute — the entry instantiates every build of the kernels — so they compile side by side, and Problem.compile skips what is up to date.
Leaves built.json beside them: per problem the library, its entry and the dimensions, for a user who wants the library without deriving the problem again."""
import concurrent.futures
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fixture_problems


def build(hipcc=None, arch="gfx950"):
    gp = fixture_problems.load("generated_problems", HERE)
    problems = [gp.generated(name) for name in gp.BUILT]
    with concurrent.futures.ThreadPoolExecutor(len(problems)) as pool:          # (threads that wait for a hipcc each)
        built = list(pool.map(lambda P: P.compile(directory=HERE, hipcc=hipcc, arch=arch), problems))
    manifest = {name: dict(library=os.path.basename(c.path), symbol=c.symbol, dims=[P.nx, P.ne, P.nc, P.np], n_nonnegative=P.n_nonnegative, second_order_dims=P.second_order_dims)
                for name, P, c in zip(gp.BUILT, problems, built)}
    with open(os.path.join(HERE, "built.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    gp.load_codegen().sweep(HERE, ("generated_", "libgenerated_"), built)
    return [c.path for c in built]


if __name__ == "__main__":
    for path in build(hipcc=os.environ.get("HIPCC"), arch=os.environ.get("ARCH", "gfx950")):
        print(path)
