"""Generate and compile the evaluators of problems.py: BUILT into this directory (test fixtures of tests/test_gpu_codegen.py, built by `python __graft_entry__.py build`).
Each takes about a minute — the entry instantiates every build of the kernels — so they compile side by side, and Problem.compile skips what is up to date.
Leaves built.json beside them: per problem the library, its entry and the dimensions, for a user who wants the library without deriving the problem again."""
import concurrent.futures
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _problems():
    if "generated_problems" in sys.modules:
        return sys.modules["generated_problems"]
    spec = importlib.util.spec_from_file_location("generated_problems", os.path.join(HERE, "problems.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["generated_problems"] = m
    spec.loader.exec_module(m)
    return m


def build(hipcc=None, arch="gfx950"):
    gp = _problems()
    problems = [gp.generated(name) for name in gp.BUILT]
    with concurrent.futures.ThreadPoolExecutor(len(problems)) as pool:          # (threads that wait for a hipcc each)
        built = list(pool.map(lambda P: P.compile(directory=HERE, hipcc=hipcc, arch=arch), problems))
    manifest = {name: dict(library=os.path.basename(c.path), symbol=c.symbol, dims=[P.nx, P.ne, P.nc, P.np], n_nonnegative=P.n_nonnegative, second_order_dims=P.second_order_dims)
                for name, P, c in zip(gp.BUILT, problems, built)}
    with open(os.path.join(HERE, "built.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    current = {os.path.basename(p) for c in built for p in (c.path, c.source_path)}
    for name in sorted(os.listdir(HERE)):           # what an earlier state of the generator or of the headers left behind
        if name.startswith(("generated_", "libgenerated_")) and name.endswith((".hip", ".so")) and name not in current:
            os.remove(os.path.join(HERE, name))
    return [c.path for c in built]


if __name__ == "__main__":
    for path in build(hipcc=os.environ.get("HIPCC"), arch=os.environ.get("ARCH", "gfx950")):
        print(path)
