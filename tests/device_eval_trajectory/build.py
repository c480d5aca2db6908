"""Generate and compile the evaluators of problems.py: BUILT into this directory (test fixtures of tests/test_gpu_trajectory_codegen.py, built by
`python __graft_entry__.py build`).  Plain kernels: each takes seconds; TrajectoryProblem.compile skips what is up to date, and problems that differ only in their
horizon share a library."""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _problems():
    if "trajectory_problems" in sys.modules:
        return sys.modules["trajectory_problems"]
    spec = importlib.util.spec_from_file_location("trajectory_problems", os.path.join(HERE, "problems.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["trajectory_problems"] = m
    spec.loader.exec_module(m)
    return m


def build(hipcc=None, arch="gfx950"):
    tp = _problems()
    built = [tp.trajectory(name).compile(directory=HERE, hipcc=hipcc, arch=arch) for name in tp.BUILT]
    current = {os.path.basename(p) for c in built for p in (c.path, c.source_path)}
    for name in sorted(os.listdir(HERE)):           # what an earlier state of the generator or of the header left behind
        if name.startswith(("trajectory_", "libtrajectory_")) and name.endswith((".hip", ".so")) and name not in current:
            os.remove(os.path.join(HERE, name))
    return sorted({c.path for c in built})


if __name__ == "__main__":
    for path in build(hipcc=os.environ.get("HIPCC"), arch=os.environ.get("ARCH", "gfx950")):
        print(path)
