"""The loader the build.py of a generated-fixture directory (device_eval_generated, device_eval_trajectory) uses for its problems.py: under a module name of its own
(`problems` is tests/problems.py), once per process."""
import importlib.util
import os
import sys


def load(module_name, directory):
    if module_name not in sys.modules:
        spec = importlib.util.spec_from_file_location(module_name, os.path.join(directory, "problems.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[module_name] = m
        spec.loader.exec_module(m)
    return sys.modules[module_name]
