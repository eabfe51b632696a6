#!/usr/bin/env python3
"""Generate tests/golden/algorithms.json: the names of the REAL reference's algorithm classes that
define a serverGradient of their own (fl_pytorch/utils/algorithms.py).

Test infrastructure only, run in the development container where the reference is mounted
read-only (imported, never copied; third-party modules it lacks are the throwaway stubs of
make_golden.py).  tests/test_host.py checks install()'s mapping against the recorded names.
"""
import inspect
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402


def main():
    tmp = tempfile.mkdtemp(prefix="flstubs_")
    make_golden._write_stubs(tmp)
    sys.path.insert(0, tmp)
    sys.path.insert(0, os.path.join(make_golden.REF, "utils"))
    sys.path.insert(0, make_golden.REF)
    sys.dont_write_bytecode = True
    os.chdir(tmp)
    from utils import algorithms
    names = sorted(n for n, c in inspect.getmembers(algorithms, inspect.isclass)
                   if c.__module__ == algorithms.__name__ and "serverGradient" in c.__dict__)
    with open(os.path.join(HERE, "algorithms.json"), "w") as f:
        json.dump({"source": "fl_pytorch/utils/algorithms.py",
                   "classes_defining_serverGradient": names}, f, indent=1)
        f.write("\n")
    print("algorithms:", names)


if __name__ == "__main__":
    main()
