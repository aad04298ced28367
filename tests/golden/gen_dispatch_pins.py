"""Generator of dispatch_pins.json (tests/test_gpu_dispatch_pins.py): runs the
test's cases on the GPU against the engine of a tree (default: this one; --tree
DIR: a built checkout of the commit to pin) and records the ce_last_kernel()
strings.  Every case also checks its results against the CPU oracle.

    python tests/golden/gen_dispatch_pins.py [--tree DIR] [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(HERE, "dispatch_pins.json"))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "consensus-entropy_amd"), os.path.join(ROOT, "tests")]
    import test_gpu_dispatch_pins as T

    ce = T._ce()
    kernels = {}
    for name, run in T.CASES.items():
        kernels[name] = run(ce)
        print(name, kernels[name], flush=True)
    from ce_amd import _lib

    groups = {}  # the cases grouped by what they record: one line per group
    for name, ks in kernels.items():
        groups.setdefault(json.dumps(ks), []).append(name)
    with open(args.out, "w") as f:
        f.write('{"version": %s,\n "groups": [\n' % json.dumps(_lib.load().ce_version().decode()))
        f.write(",\n".join('  {"kernels": %s, "cases": %s}' % (k, json.dumps(sorted(v))) for k, v in sorted(groups.items())))
        f.write("\n ]}\n")
    print("wrote", args.out, len(kernels), "cases")


if __name__ == "__main__":
    main()
