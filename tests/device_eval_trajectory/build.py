"""Generate and compile the evaluators of problems.py: BUILT into this directory (test fixtures of tests/test_gpu_trajectory_codegen.py, built by
`python __graft_entry__.py build`).  Plain kernels: each takes seconds; TrajectoryProblem.compile skips what is up to date, and problems that differ only in their
horizon share a library."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fixture_problems


def build(hipcc=None, arch="gfx950"):
    tp = fixture_problems.load("trajectory_problems", HERE)
    built = [tp.trajectory(name).compile(directory=HERE, hipcc=hipcc, arch=arch) for name in tp.BUILT]
    tp.load_codegen().sweep(HERE, ("trajectory_", "libtrajectory_"), built)
    return sorted({c.path for c in built})


if __name__ == "__main__":
    for path in build(hipcc=os.environ.get("HIPCC"), arch=os.environ.get("ARCH", "gfx950")):
        print(path)
