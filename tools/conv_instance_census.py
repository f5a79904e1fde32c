"""Which kernel does every case of tests/conv_instance_cases.py really launch?

    python tools/conv_instance_census.py            (on an MI355X, from the repository root)

runs the case table in order, exactly ONE rac_conv2d_fwd_split launch per case, in a child process under
`rocprofv3 --kernel-trace` (nothing else is traced or counted), keeps the trace records whose kernel name starts with
`conv16_` -- the i-th such record, by start time, belongs to the i-th case -- and writes tests/conv_instance_record.json:
case name -> demangled kernel name.  tests/test_conv_instances_host.py holds the table to that record; regenerate it with
this tool whenever the launcher's choice of kernel changes.  `--out FILE` writes elsewhere; `--timeout S` bounds the child."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    import torch
    from tests import conv_instance_cases as cc
    dev = torch.device("cuda", 0)
    for c in cc.CASES:
        x, w = cc.int_operands(c)
        cc.launch(dev, c, x, w)  # (NaN / guard checks included: a census of launches that went wrong is worth nothing)
        print("launched %s" % c.name, flush=True)


def conv16_name(kernel_name):
    """The demangled name without its return type and namespace, or None for other kernels."""
    m = re.match(r"(?:void\s+)?(?:\w+::)*(conv16_.*)$", kernel_name.strip())
    return m.group(1) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "conv_instance_record.json"))
    ap.add_argument("--timeout", type=int, default=420)
    a = ap.parse_args()
    if a.child:
        return child()
    from tests import conv_instance_cases as cc
    with tempfile.TemporaryDirectory() as tmp:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--child"]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.timeout)
        if res.returncode != 0:
            sys.exit("the traced child failed (%d):\n%s\n%s" % (res.returncode, res.stdout[-2000:], res.stderr[-4000:]))
        launched = [ln.split()[1] for ln in res.stdout.splitlines() if ln.startswith("launched ")]
        assert launched == [c.name for c in cc.CASES], launched
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert len(traces) == 1, traces
        with open(traces[0], newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [n for n in (conv16_name(r["Kernel_Name"]) for r in rows) if n]
    assert len(names) == len(cc.CASES), "%d conv16_ launches for %d cases" % (len(names), len(cc.CASES))
    record = {c.name: n for c, n in zip(cc.CASES, names)}
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    wrong = [(c.name, c.instance, record[c.name]) for c in cc.CASES if cc.kernel_instance(record[c.name]) != c.instance]
    reached = {cc.kernel_instance(n) for n in names}
    print("%d cases, %d distinct instances, %d rows the table expected otherwise" % (len(names), len(reached), len(wrong)))
    for w in wrong:
        print("  %s: expected %s, launched %s" % w)
    for inst in cc.ALL_INSTANCES:
        if inst not in reached:
            print("  not reached: %s%s" % (inst, "  (listed unreachable)" if inst in cc.UNREACHABLE else "  <-- UNACCOUNTED"))


if __name__ == "__main__":
    main()
