"""Child process of tests/test_gpu_conv_instances.py: the exactness part of the conv instance table
(tests/conv_instance_cases.py) in a fresh process, so that the launcher's process-wide A/B switches -- RAC_TILE_UNROLL3,
RAC_TILE_UNROLL5, RAC_TILE_YMAJOR, RAC_ROWS_GENERIC, RAC_ROWS_PERSIST, RAC_XCD_GROUP: read once, kept in statics -- take
the values the parent put into the environment.  `all`: every case; any other argument: the cases whose name starts with
it.  Prints one line per case, `case <name> exact`; the first failing case ends the process with a traceback."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from tests import conv_instance_cases as cc
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    dev = torch.device("cuda", 0)
    for c in cc.CASES:
        if which != "all" and not c.name.startswith(which):
            continue
        cc.exact_case(dev, c)
        print("case %s exact" % c.name, flush=True)


if __name__ == "__main__":
    main()
